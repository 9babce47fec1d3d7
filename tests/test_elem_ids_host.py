"""Element ids on the host (no GPU): tfrg_hash64 against its known answers and the Python restatement,
the vocabulary's table against a Python model of the documented table, the host lookup against a dict
(displaced words, the empty word, near misses), what tfrg_vocab_create refuses, the numpy path
(``BatchResult.element_ids`` / ``idsify``) against tests/_ids_ref.py, and the layout of tfrg_ids_spec
against the header (the method of tests/test_select_abi.py). Every comparison is exact."""

import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _bytes_ref as B
from tests import _columns
from tests import _ids_ref as IR
from tests.golden.gen_golden import entry, i64
from tests.test_dense_rows_host import row_lists
from tfr_reader import _native as N
from tfr_reader import ids as I
from tfr_reader import synth

INCLUDE = Path(__file__).resolve().parents[1] / "include"
WORDS48 = [b"w%02d" % i for i in range(48)]
W17 = bytes(range(100, 117))
NEAR = [bytes([W17[0] ^ 1]) + W17[1:], W17[:7] + bytes([W17[7] ^ 0x80]) + W17[8:], W17[:8] + bytes([W17[8] ^ 1]) + W17[9:],
        W17[:16] + bytes([W17[16] ^ 0x40]), W17[:16], W17 + b"\0"]


# ------------------------------------------------------------------------------------ raw vocabularies
class RawVocab:
    """A tfrg_vocab made through the C entry points alone (device -1: the host table)."""

    def __init__(self, words: list[bytes], ids=None, device: int = -1, offsets=None, n_words=None) -> None:
        self.lib = N.lib()
        self.ptr = C.c_void_p()
        offs = np.zeros(len(words) + 1, np.uint64)
        np.cumsum([len(w) for w in words], out=offs[1:])
        offs = offs if offsets is None else np.asarray(offsets, np.uint64)
        ids_a = None if ids is None else np.asarray(ids, np.int64)
        self.rc = self.lib.tfrg_vocab_create(device, b"".join(words), N.ptr(offs, N.u64p), len(words) if n_words is None else n_words,
                                             N.ptr(ids_a, N.i64p) if ids_a is not None else None, C.byref(self.ptr))

    def info(self) -> tuple[int, int, int, int]:
        nw, cap, db, mp = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        assert self.lib.tfrg_vocab_info(self.ptr, C.byref(nw), C.byref(cap), C.byref(mp), C.byref(db)) == 0
        return nw.value, cap.value, mp.value, db.value

    def lookup(self, s: bytes, missing: int = -7) -> int:
        return self.lib.tfrg_vocab_lookup_host(self.ptr, s, len(s), missing)

    def close(self) -> None:
        assert self.lib.tfrg_vocab_destroy(self.ptr) == 0
        self.ptr = C.c_void_p()


# ------------------------------------------------------------------------------------ 1. the hash
def test_hash_known_answers_and_lengths():
    lib = N.lib()
    for s, want in IR.KNOWN:
        assert IR.hash64(s) == want, s
        assert lib.tfrg_hash64(s, len(s)) == want, s
        assert I.hash64(s) == want and I.hash64_py(s) == want, s
    blob = np.random.default_rng(5).integers(0, 256, 64, dtype=np.uint8).tobytes()
    seen = set()
    for n in range(41):
        for at in (0, 1, 3):  # (the C function reads an unaligned pointer as well)
            s = blob[at : at + n]
            assert lib.tfrg_hash64(s, n) == IR.hash64(s) == I.hash64_py(s), (n, at)
        seen.add(IR.hash64(blob[:n]))
    assert len(seen) == 41
    assert IR.hash64(b"a") != IR.hash64(b"a\0") != IR.hash64(b"a\0\0")  # (the length is hashed)


# ------------------------------------------------------------------------------------ 2. the table
def test_table_matches_the_model():
    model = IR.TableModel(WORDS48)
    assert model.capacity == 128 and model.max_probe == 3  # (the model alone)
    v = RawVocab(WORDS48)
    try:
        assert v.rc == 0 and v.info() == (48, model.capacity, model.max_probe, 0)
    finally:
        v.close()
    for n, cap in ((0, 16), (1, 16), (8, 16), (9, 32), (64, 128), (65, 256), (1000, 2048)):
        words = [b"k%d" % i for i in range(n)]
        m = IR.TableModel(words)
        assert m.capacity == cap
        v = RawVocab(words)
        try:
            assert v.rc == 0 and v.info() == (n, cap, m.max_probe, 0), n
        finally:
            v.close()


def test_python_vocabulary_reports_the_models_table():
    v = I.Vocabulary(WORDS48)
    model = IR.TableModel(WORDS48)
    assert len(v) == 48 and v.device is None
    assert v.info == {"n_words": 48, "capacity": model.capacity, "max_probe": model.max_probe, "device_bytes": 0}
    assert v.lookup(b"w07") == 7 == v.id_of(b"w07") and v.lookup("w07") == 7 and v.lookup(b"w48") == -1 and v.lookup(b"w48", 99) == 99
    v.close()
    with pytest.raises(ValueError):
        v.lookup(b"w07")
    with pytest.raises(ValueError):
        I.Vocabulary([b"a", b"b", b"a"])
    with pytest.raises(ValueError):
        I.Vocabulary([b"a", b"b"], ids=[1])
    with pytest.raises(TypeError):
        I.Vocabulary([1, 2])


# ------------------------------------------------------------------------------------ 3. host lookup
def test_host_lookup_equals_the_dict():
    model = IR.TableModel(WORDS48)
    assert model.max_probe >= 2  # (on the model, before a displaced word's lookup is trusted)
    displaced = [w for w, d in zip(WORDS48, model.disp) if d >= 2]
    assert displaced
    ids = [3 * i - 50 for i in range(48)]  # (negative ids included)
    table = dict(zip(WORDS48, ids))
    v = RawVocab(WORDS48, ids)
    try:
        for w in WORDS48:
            assert v.lookup(w) == table[w], w
        for w in displaced:
            assert v.lookup(w) == table[w]
        for s in (b"", b"w", b"w0", b"w48", b"w000", b"W00", b"w00\0", b"x" * 300):
            assert v.lookup(s) == table.get(s, -7), s
        assert v.lookup(b"w05", 123) == table[b"w05"] and v.lookup(b"nope", 123) == 123
    finally:
        v.close()
    default = RawVocab(WORDS48)
    try:
        assert [default.lookup(w) for w in WORDS48] == list(range(48))  # (ids NULL: the word's position)
    finally:
        default.close()


def test_host_lookup_empty_word_padding_and_near_misses():
    words = [b"a", W17, b"", b"12345678", b"123456789"]
    table = {w: i for i, w in enumerate(words)}
    v = RawVocab(words)
    try:
        for s in [*words, b"a\0", b"a\0\0", b"\0", *NEAR, W17[1:], b"1234567", b"12345678\0"]:
            assert v.lookup(s) == table.get(s, -7), s
        assert v.lookup(b"") == 2
    finally:
        v.close()
    without = RawVocab([b"a\0", W17])
    try:
        assert without.lookup(b"") == -7 and without.lookup(b"a") == -7 and without.lookup(b"a\0") == 0
        assert [without.lookup(s) for s in NEAR] == [-7] * len(NEAR) and without.lookup(W17) == 1
    finally:
        without.close()


# ------------------------------------------------------------------------------------ 4. refusals
def test_what_vocab_create_refuses_and_the_empty_vocabulary():
    lib = N.lib()
    dup = RawVocab([b"x", b"yy", b"x"])
    assert dup.rc == -1 and not dup.ptr and b"word 2 equals word 0" in lib.tfrg_last_error()
    assert lib.tfrg_last_error().startswith(b"tfrg_vocab_create: ")
    dup_empty = RawVocab([b"", b"q", b""])
    assert dup_empty.rc == -1 and not dup_empty.ptr
    desc = RawVocab([b"ab", b"cd"], offsets=[0, 3, 2])
    assert desc.rc == -1 and not desc.ptr and b"descend" in lib.tfrg_last_error()
    many = RawVocab([b"ab"], n_words=1 << 31)  # (refused before an offset is read)
    assert many.rc == -1 and not many.ptr and b"2^31" in lib.tfrg_last_error()
    big = RawVocab([b"ab"], offsets=[0, 1 << 32])
    assert big.rc == -1 and not big.ptr and b"2^32" in lib.tfrg_last_error()
    assert lib.tfrg_vocab_create(-1, b"", None, 0, None, None) == -1
    assert lib.tfrg_vocab_destroy(None) == 0
    empty = RawVocab([])
    try:
        assert empty.rc == 0 and empty.info() == (0, 16, 0, 0)
        assert empty.lookup(b"") == -7 and empty.lookup(b"a") == -7
    finally:
        empty.close()
    null_offsets = C.c_void_p()
    assert lib.tfrg_vocab_create(-1, None, None, 0, None, C.byref(null_offsets)) == 0 and null_offsets
    assert lib.tfrg_vocab_destroy(null_offsets) == 0
    shifted = RawVocab([b"zzab", b"cd"], offsets=[2, 4, 6])  # (offsets[0] need not be 0)
    try:
        assert shifted.rc == 0 and shifted.lookup(b"ab") == 0 and shifted.lookup(b"cd") == 1 and shifted.lookup(b"zzab") == -7
    finally:
        shifted.close()


def test_result_elem_ids_without_a_context_is_an_argument_error():
    lib = N.lib()
    spec = N.TfrgIdsSpec(slot=0, max_elems=0, reserved0=0, reserved1=0, vocab=None, num_oov_buckets=4, oov_base=0, default_id=0,
                         elem_cap=0, ids=None, row_offsets=16)
    assert lib.tfrg_result_elem_ids(None, C.byref(spec), 1, None, N.ROWS_I64, 1, 0, None, None, None) == -1
    assert lib.tfrg_last_error().startswith(b"tfrg_result_elem_ids: ")


# ------------------------------------------------------------------------------------ 5. the numpy path
LENGTHS = [0, 1, 3, 4, 7, 8, 9, 15, 16, 17, 31, 33]
PER_RECORD = [0, 1, 2, 3, 7]


def batch() -> tuple[list[bytes], list[dict]]:
    elems = B.random_elems([LENGTHS[i % len(LENGTHS)] for i in range(300)], 22)
    elems[5:5] = [W17, *NEAR, b"a", b"a\0"]
    payloads, items = B.pack(elems, PER_RECORD)
    for i in range(0, len(payloads), 9):
        payloads[i], items[i] = B.record({}, entry(b"n", i64(i)))
    return payloads, items


@pytest.fixture(scope="module")
def decoded():
    payloads, items = batch()
    return _columns.batch_from_oracle(*synth.framed(payloads)), items


def rules_and_specs(items):
    """(tests/_ids_ref.py rule, tfr_reader.ids spec) pairs over the same tables."""
    elems = [e for it in items for e in it.get("b", [])]
    words = list(dict.fromkeys([*elems[::2], W17, b"a"]))
    words = [w for w in words if w not in NEAR and w != b"a\0"]
    ids = [7 * i - 100 for i in range(len(words))]
    v_pos, v_ids, v_none = I.Vocabulary(words), I.Vocabulary(words, ids), I.Vocabulary([])
    t_pos, t_ids = {w: i for i, w in enumerate(words)}, dict(zip(words, ids))
    nw = len(words)
    return [
        (IR.Rule("b", t_pos, default=-1), I.ElementIds("b", v_pos)),
        (IR.Rule("b", t_ids, default=-5), I.ElementIds("b", v_ids, default_id=-5, name="ids")),
        (IR.Rule("b", t_pos, 7, nw), I.ElementIds("b", v_pos, num_oov_buckets=7, name="oov7")),
        (IR.Rule("b", t_pos, 1000, 0), I.ElementIds("b", v_pos, num_oov_buckets=1000, oov_base=0, name="oov1000")),
        (IR.Rule("b", None, 1 << 40, 0), I.ElementIds("b", num_oov_buckets=1 << 40, name="hash")),
        (IR.Rule("b", {}, default=9), I.ElementIds("b", v_none, default_id=9, name="none")),
        (IR.Rule("b", t_pos, 3, nw, max_elems=2), I.ElementIds("b", v_pos, num_oov_buckets=3, max_elems=2, name="e2")),
        (IR.Rule("zz", t_pos), I.ElementIds("zz", v_pos, name="absent")),
    ]


def check(got, items, pairs, rows) -> None:
    for rule, sp in pairs:
        k = sp.out_name
        want = IR.expect(items, rule, rows)
        ids, ro = got[k]
        assert ids.dtype == np.int64 and ro.dtype == np.int64, k
        assert np.array_equal(ro, want.row_offsets) and np.array_equal(ids, want.ids), k
        assert got.stats[k].tolist() == want.stats and got.totals[k] == want.total, k
        assert got.capacity[k] == want.total and got.overflowed[k] is False, k


def test_idsify_gives_the_references_ids(decoded):
    res, items = decoded
    pairs = rules_and_specs(items)
    specs = [sp for _, sp in pairs]
    whole = IR.expect(items, pairs[0][0])
    assert 0 < whole.matched < whole.total
    near = IR.expect(items, pairs[0][0], [1, 2, 3, 4])
    assert W17 in near.elems and all(s in near.elems for s in NEAR)
    for rows in [None, *row_lists(len(items))]:
        check(res.element_ids(specs, rows=rows), items, pairs, rows)
    got = I.idsify(specs, n=len(res), slot_key=res.slot_key, slot_kind=res.slot_kind, row_splits=res.row_splits,
                   slot_base=res.slot_base, bytes_off=res.bytes_off, bytes_len=res.bytes_len, buf=res.buf, rows=[4, 4, 0, 1])
    check(got, items, pairs, [4, 4, 0, 1])
    assert I.IDS_STAT_NAMES == ("rows_truncated", "unmatched", "empty", "skipped")


def test_specs_that_are_refused(decoded):
    res = decoded[0]
    v = I.Vocabulary([b"q"])
    with pytest.raises(ValueError):
        I.ElementIds("b")  # (no vocabulary and no buckets)
    for bad in (dict(num_oov_buckets=-1), dict(num_oov_buckets=1 << 64), dict(max_elems=0), dict(max_elems=1 << 32),
                dict(default_id=1 << 63), dict(oov_base=-(1 << 63) - 1)):
        with pytest.raises(ValueError):
            I.ElementIds("b", v, **bad)
    with pytest.raises(TypeError):
        I.ElementIds(b"b", v)
    with pytest.raises(TypeError):
        I.ElementIds("b", {b"q": 0})
    assert I.ElementIds("b", v, num_oov_buckets=3).base == 1 and I.ElementIds("b", num_oov_buckets=3).base == 0
    with pytest.raises(ValueError):
        res.element_ids([I.ElementIds("b", v), I.ElementIds("b", v, default_id=0)])  # (two outputs of one name)
    with pytest.raises(ValueError):
        res.element_ids([])
    with pytest.raises(ValueError):
        res.element_ids([I.ElementIds("b", v, name=str(i)) for i in range(N.IDS_MAX_SPECS + 1)])
    with pytest.raises(IndexError):
        res.element_ids([I.ElementIds("b", v)], rows=[0, len(res)])


# ------------------------------------------------------------------------------------ 6. the layout
STRUCTS = {"tfrg_ids_spec": N.TfrgIdsSpec}
CONSTANTS = {"TFRG_IDS_MAX_SPECS": N.IDS_MAX_SPECS}


def _c_layout(tmp_path: Path) -> dict:
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "tfrg.h"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'  printf("{cname} {fname} %zu %zu\\n", offsetof({cname}, {fname}), sizeof((({cname}*)0)->{fname}));')
    for name in CONSTANTS:
        lines.append(f'  printf("const {name} %lld 0\\n", (long long)({name}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(INCLUDE), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    res: dict = {}
    for line in out.splitlines():
        parts = line.split()
        if parts[1] == "size":
            res[(parts[0], "__size__")] = int(parts[2])
        else:
            res[(parts[0], parts[1])] = (int(parts[2]), int(parts[3]))
    return res


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_ids_spec_matches_the_header(tmp_path):
    c = _c_layout(tmp_path)
    for cname, py in STRUCTS.items():
        assert c[(cname, "__size__")] == C.sizeof(py) == 72, cname
        for fname, _ in py._fields_:
            f = getattr(py, fname)
            assert c[(cname, fname)] == (f.offset, f.size), (cname, fname)
    for name, value in CONSTANTS.items():
        assert c[("const", name)][0] == value, name


def test_every_header_field_and_entry_point_is_mirrored():
    text = re.sub(r"/\*.*?\*/", "", (INCLUDE / "tfrg.h").read_text(), flags=re.S)
    for cname, py in STRUCTS.items():
        m = re.search(r"typedef struct " + cname + r"\s*\{(.*?)\}\s*" + cname + r"\s*;", text, flags=re.S)
        assert m, cname
        names = re.findall(r"\b(\w+)\s*(?:\[\s*\d+\s*\])?\s*[;,]", m.group(1))
        assert names == [f for f, _ in py._fields_], (cname, names)
    for ret, fn, nargs in (("uint64_t", "tfrg_hash64", 2), ("int", "tfrg_vocab_create", 6), ("int", "tfrg_vocab_destroy", 1),
                           ("int", "tfrg_vocab_info", 5), ("int64_t", "tfrg_vocab_lookup_host", 4),
                           ("int", "tfrg_result_elem_ids", 10)):
        assert re.search(r"\b" + ret + " " + fn + r"\(", text) and fn in N.SIGNATURES, fn
        assert hasattr(N.lib(), fn) and len(N.SIGNATURES[fn][1]) == nargs, fn
