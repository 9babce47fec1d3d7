"""Bytes predicates on the host (no GPU): ``BytesTerm`` / ``bytes_in`` and what they refuse, the host
path (``BatchResult.select`` / ``select_mask``) against Python's own ``bytes`` semantics applied to the
very lists the test wrote into the file (``==``, ``<``, ``startswith``, ``endswith``, ``in``: neither the
host nor the device path has a part in that oracle), and the term table ``fold`` builds for
``tfrg_result_select_match``: the operand packing, the pattern blob, its limits, absent keys. Every
case that is not an "all" or "none" case selects, by the oracle alone, some records and not all."""

import ctypes as C
import types

import numpy as np
import pytest

from tests import _columns
from tfr_reader import _native as N
from tfr_reader import hip, synth, writer
from tfr_reader import select as S
from tfr_reader.select import BytesTerm, Status, Term, bytes_in

OPS = ["==", "!=", "<", "<=", ">", ">=", "startswith", "endswith", "contains"]
PY = dict(S._PY_OPS)
PY.update({"startswith": lambda e, p: e.startswith(p), "endswith": lambda e, p: e.endswith(p),
           "contains": lambda e, p: p in e})


# ------------------------------------------------------------------------------------ the oracle
def py_bytes_term(elems, t: BytesTerm) -> bool:
    """One bytes term for a record whose list is ``elems`` (None: the key is absent), in Python's words."""
    elems = elems or []
    pattern = t.operand if isinstance(t.operand, bytes) else t.operand.encode()
    if t.subject == "value":
        return len(elems) > t.index and bool(PY[t.op](elems[t.index], pattern))
    return any(PY[t.op](e, pattern) for e in elems)


def py_mask(recs: list[dict], where, failed=()) -> list[bool]:
    """The records' verdicts. ``recs[g]``: {key: list of bytes, or list of ints}; a failed record has
    no values and a nonzero status."""
    groups = [g if isinstance(g, list) else [g] for g in where]

    def term(g: int, t) -> bool:
        rec = {} if g in failed else recs[g]
        if isinstance(t, BytesTerm):
            vals = rec.get(t.key)
            # (a key written as an int64 list has no bytes list: it is absent to a bytes term)
            return py_bytes_term(None if vals and not isinstance(vals[0], bytes) else vals, t)
        if isinstance(t, Status):
            return bool(S._PY_OPS[t.op](1 if g in failed else 0, 0)) if t.operand == 0 else False
        vals = rec.get(t.key) or []
        if t.subject == "count":
            return bool(S._PY_OPS[t.op](len(vals), t.operand))
        if t.subject == "bytes_len":
            return bool(S._PY_OPS[t.op](len(vals[0]) if vals else 0, t.operand))
        return len(vals) > t.index and bool(S._PY_OPS[t.op](vals[t.index], t.operand))

    return [all(any(term(g, t) for t in grp) for grp in groups) for g in range(len(recs))]


def py_rows(recs, where, kind: str = "some", failed=()) -> list[int]:
    mask = py_mask(recs, where, failed)
    got = [g for g, v in enumerate(mask) if v]
    if kind == "some":
        assert 0 < len(got) < len(recs), (where, len(got))
    elif kind == "all":
        assert len(got) == len(recs) > 0, where
    elif kind == "none":
        assert not got and recs, where
    return got


# ------------------------------------------------------------------------------------ a small mixed file
POOL = [b"cat", b"", b"category", b"ca", b"bobcat", b"cat\x00", b"\x80\xffcat", b"c\xe1t", b"rose garden", b"dog",
        b"train/cat.jpg", b"tomcat", b"cas", b"cau", b"\xff", b"\x80"]


def mixed_bytes(n: int = 240) -> tuple[list[bytes], list[dict]]:
    """(payloads, what was written). Record g: ``label`` [g]; ``names`` absent (g % 4 == 0), an empty
    list (1), one element (2) or three (3), drawn from POOL so that every op meets equal, shorter,
    longer, smaller and larger elements, the empty one included."""
    payloads, recs = [], []
    for g in range(n):
        rec = {"label": [g]}
        feats = [("label", "int64_list", [g])]
        if g % 4:
            k = (0, 0, 1, 3)[g % 4]
            rec["names"] = [POOL[(g // 4 * 5 + 3 * j + g) % len(POOL)] for j in range(k)]
            feats.append(("names", "bytes_list", rec["names"]))
        payloads.append(writer.encode_example(feats))
        recs.append(rec)
    return payloads, recs


@pytest.fixture(scope="module")
def small():
    payloads, recs = mixed_bytes()
    return _columns.batch_from_oracle(*synth.framed(payloads)), recs


def check(res, recs, where, kind: str = "some"):
    want = py_rows(recs, where, kind)
    got, stats = res.select(where)
    assert got.dtype == np.int64 and got.tolist() == want and tuple(stats) == (len(want), 0), where
    return want


def test_every_op_and_both_subjects_against_python_bytes(small):
    res, recs = small
    assert any(r.get("names") == [] for r in recs) and any("names" not in r for r in recs)
    assert any(b"" in (r.get("names") or []) for r in recs)
    for pattern in (b"cat", b"ca", b"cas", b"cat\x00", b"\x80\xffcat"):  # (each is an element somewhere)
        for op in OPS:
            check(res, recs, [BytesTerm("names", op, pattern)])
            check(res, recs, [BytesTerm("names", op, pattern, "any")])
            check(res, recs, [BytesTerm("names", op, pattern, index=2)])
    # the empty pattern: equal to the empty element alone; a prefix, suffix and substring of every element
    has_first = [g for g, r in enumerate(recs) if r.get("names")]
    for op in ("startswith", "endswith", "contains", ">="):
        assert check(res, recs, [BytesTerm("names", op, b"")]) == has_first
    want = check(res, recs, [BytesTerm("names", "==", b"")])
    assert want == [g for g in has_first if recs[g]["names"][0] == b""]
    check(res, recs, [BytesTerm("names", "<", b"")], kind="none")
    # NE on a record without the element is false
    want = check(res, recs, [BytesTerm("names", "!=", b"no such name", index=1)])
    assert want == [g for g, r in enumerate(recs) if len(r.get("names") or []) > 1]
    # a str operand is its UTF-8 bytes; unsigned order: 0xe1 sorts above every ASCII letter
    assert BytesTerm("names", "==", "cát").operand == b"c\xc3\xa1t"
    check(res, recs, [BytesTerm("names", "==", "cát")], kind="none")  # (the file holds the Latin-1 bytes c e1 t)
    check(res, recs, [BytesTerm("names", "==", "cat")])
    want = check(res, recs, [BytesTerm("names", ">", b"cz")])
    assert any(recs[g]["names"][0] == b"c\xe1t" for g in want) and any(recs[g]["names"][0][0] == 0x80 for g in want)


def test_groups_mixed_terms_and_absent_keys(small):
    res, recs = small
    check(res, recs, [bytes_in("names", [b"cat", b"dog", b"nobody"])])
    check(res, recs, [BytesTerm("names", "contains", b"cat", "any"), Term("label", "int64", "<", 150)])
    check(res, recs, [[BytesTerm("names", "endswith", b"cat"), Term("label", "int64", ">=", 200)], Status("==", 0)])
    check(res, recs, [BytesTerm("names", "startswith", b"c"), BytesTerm("names", "endswith", b"t", "any")])
    for op in OPS:
        check(res, recs, [BytesTerm("absent", op, b"")], kind="none")
        check(res, recs, [BytesTerm("absent", op, b"x", "any")], kind="none")
        check(res, recs, [BytesTerm("label", op, b"")], kind="none")  # (a key of another kind has no bytes slot)
    check(res, recs, [[BytesTerm("absent", "==", b"cat"), BytesTerm("names", "==", b"cat")]])
    # candidates and row0 are apply_mask's, as for every other term
    where = [BytesTerm("names", "contains", b"cat")]
    want = py_rows(recs, where)
    rows = [want[0], -1, len(recs), want[0], 1, want[-1]]
    got, stats = res.select(where, rows=rows)
    assert got.tolist() == [want[0], want[0], want[-1]] and tuple(stats) == (3, 2) and 1 not in want
    got, stats = res.select(where, rows=[1000 + want[1], want[1]], row0=1000)
    assert got.tolist() == [1000 + want[1]] and tuple(stats) == (1, 1)


def test_materialized_columns_give_the_same_mask(small):
    """``select_mask`` from a materialized byte column (bytes_data / bytes_offsets) and from views."""
    res, recs = small
    cols = S.batch_columns(res)
    assert cols["bytes_data"] is None
    lens = res.bytes_len.astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    data = np.concatenate([res.buf[int(o) : int(o) + int(ln)] for o, ln in zip(res.bytes_off, lens)] or [np.zeros(0, np.uint8)])
    mat = dict(cols, bytes_data=data, bytes_offsets=offs, buf=None, bytes_off=None, bytes_len=None)
    for where in ([BytesTerm("names", "contains", b"cat", "any")], [BytesTerm("names", "<", b"cat", index=1)]):
        want = py_mask(recs, where)
        assert 0 < sum(want) < len(recs)
        assert S.select_mask(where, **cols).tolist() == want == S.select_mask(where, **mat).tolist()


# ------------------------------------------------------------------------------------ validation
def test_bytes_term_validation():
    for bad in (dict(op="~"), dict(op="in"), dict(subject="count"), dict(subject="bytes_len"), dict(operand=7),
                dict(operand=None), dict(operand=[b"a"]), dict(operand=b"x" * 257), dict(operand="é" * 129),
                dict(index=-1), dict(index=1 << 32), dict(index=True), dict(subject="any", index=1), dict(key=b"names")):
        kw = dict(key="names", op="==", operand=b"cat")
        kw.update(bad)
        with pytest.raises((ValueError, TypeError)):
            BytesTerm(**kw)
    with pytest.raises(TypeError):
        BytesTerm("names", "==", 1.5)
    with pytest.raises(ValueError, match="256"):
        BytesTerm("names", "contains", b"\x00" * 257)
    assert len(BytesTerm("names", "==", b"x" * 256).operand) == 256 and len(BytesTerm("n", "==", "é" * 128).operand) == 256
    t = BytesTerm("names", "startswith", "träin/")
    assert t.operand == "träin/".encode() and t.subject == "value" and t.index == 0 and t.dtype == "uint8" and t.kind == 1
    assert BytesTerm("names", "==", bytearray(b"ab")).operand == b"ab"
    assert BytesTerm("names", "==", b"a") == BytesTerm("names", "==", "a") and hash(t) == hash(t)
    assert [x.operand for x in bytes_in("names", [b"a", "b"])] == [b"a", b"b"]
    assert all(x.op == "==" and x.subject == "value" for x in bytes_in("names", ["a"]))
    # Term itself is as it was
    with pytest.raises(ValueError, match="needs an int64 or float32 feature, not bytes"):
        Term("names", "uint8", "==", 1)
    # check_where takes the three kinds of term together, under the same limits
    i = Term("label", "int64", "==", 1)
    assert S.check_where([t, [t, i, Status("==", 0)]]) == [[t], [t, i, Status("==", 0)]]
    for bad in (t, [[b"names"]], [[t, [t]]]):
        with pytest.raises(TypeError):
            S.check_where(bad)
    with pytest.raises(ValueError, match="32 terms"):
        S.check_where([[t] * 33])
    with pytest.raises(ValueError, match="32 groups"):
        S.check_where([t] * 33)


# ------------------------------------------------------------------------------------ fold
def fake_decoder(slots: list[tuple[str, int]]):
    """What ``fold`` asks of a decoder: its key table, and how many slots of it are on the device."""
    kt = hip.KeyTable()
    for key, kind in slots:
        kt.intern(key.encode(), kind)
    return types.SimpleNamespace(keys=kt, _pushed_slots=len(slots))


def test_fold_packs_operands_into_one_blob():
    dec = fake_decoder([("label", 3), ("names", 1), ("path", 1)])
    assert S.pack_pattern(5, 3) == 5 | (3 << 32) and S.pack_pattern(0, 0) == 0 and S.pack_pattern(2047, 256) >> 32 == 256
    where = [bytes_in("names", [b"cat", b"dog", b"cat"]), BytesTerm("path", "startswith", b"train/"),
             [BytesTerm("names", "contains", b"cat", "any"), Term("label", "int64", ">", 5)], BytesTerm("path", "!=", b"")]
    table = S.fold(dec, S.check_where(where))
    assert table.patterns == b"catdogtrain/"  # (equal operands once; the empty one takes no room)
    cat, dog, train = S.pack_pattern(0, 3), S.pack_pattern(3, 3), S.pack_pattern(6, 6)
    assert list(table) == [(1, N.SEL_BYTES, N.SEL_EQ, 0, 0, cat), (1, N.SEL_BYTES, N.SEL_EQ, 0, 0, dog),
                           (1, N.SEL_BYTES, N.SEL_EQ, 0, 0, cat), (2, N.SEL_BYTES, N.SEL_PREFIX, 1, 0, train),
                           (1, N.SEL_BYTES_ANY, N.SEL_CONTAINS, 2, 0, cat), (0, N.SEL_VALUE, N.SEL_GT, 2, 0, 5),
                           (2, N.SEL_BYTES, N.SEL_NE, 3, 0, S.pack_pattern(0, 0))]
    for _slot, subject, _op, _g, _i, bits in table:
        if subject in (N.SEL_BYTES, N.SEL_BYTES_ANY):
            assert (bits & 0xFFFFFFFF) + (bits >> 32) <= len(table.patterns)
    # an operand that lies inside an earlier one is found there
    t2 = S.fold(dec, [[BytesTerm("names", "==", b"category")], [BytesTerm("names", "endswith", b"gory")]])
    assert t2.patterns == b"category" and t2[1][5] == S.pack_pattern(4, 4)
    idx = S.fold(dec, [[BytesTerm("names", "<=", b"b", index=7)]])
    assert list(idx) == [(1, N.SEL_BYTES, N.SEL_LE, 0, 7, S.pack_pattern(0, 1))]
    # a where without a bytes term is what it was: a table with no patterns
    plain = S.fold(dec, [[Term("label", "int64", "==", 3)]])
    assert plain == [(0, N.SEL_VALUE, N.SEL_EQ, 0, 0, 3)] and plain.patterns == b""


def test_fold_limits_and_absent_keys():
    dec = fake_decoder([("label", 3), ("names", 1)])
    pats = [bytes([65 + k]) * 256 for k in range(8)]
    full = S.fold(dec, [[BytesTerm("names", "==", p)] for p in pats])
    assert len(full.patterns) == N.SEL_MAX_PATTERN_BYTES == 2048 and len(full) == 8
    # (the same operand again costs nothing)
    assert len(S.fold(dec, [[BytesTerm("names", "==", p)] for p in pats + pats[:3]]).patterns) == 2048
    with pytest.raises(ValueError, match="2048"):
        S.fold(dec, [[BytesTerm("names", "==", p)] for p in pats] + [[BytesTerm("names", "==", b"!")]])
    # an absent key, or a key that has no bytes slot: a constant false term
    for key in ("absent", "label"):
        for op in OPS:
            assert S.fold(dec, [[BytesTerm(key, op, b"")]]) is None  # (its group is emptied)
            assert S.fold(dec, [[BytesTerm(key, op, b"x", "any")], [Term("label", "int64", "==", 1)]]) is None
        kept = S.fold(dec, [[BytesTerm(key, "==", b"zzz"), BytesTerm("names", "==", b"cat")]])
        assert list(kept) == [(1, N.SEL_BYTES, N.SEL_EQ, 0, 0, S.pack_pattern(0, 3))] and kept.patterns == b"cat"
    # a slot that is not on the device yet is absent too
    dec._pushed_slots = 1
    assert S.fold(dec, [[BytesTerm("names", "==", b"cat")]]) is None
    # a group a true constant removes takes its operands with it
    dec._pushed_slots = 2
    gone = S.fold(dec, [[Term("absent", "int64", "==", 0, "count"), BytesTerm("names", "==", b"cat")],
                        [BytesTerm("names", "==", b"dog")]])
    assert list(gone) == [(1, N.SEL_BYTES, N.SEL_EQ, 0, 0, S.pack_pattern(0, 3))] and gone.patterns == b"dog"


# ------------------------------------------------------------------------------------ the C ABI without a device
def test_select_match_without_a_context_and_the_constants():
    lib = N.lib()
    term = N.TfrgSelectTerm(slot=0, subject=N.SEL_BYTES, op=N.SEL_CONTAINS, group=0, index=0, reserved=0,
                            operand=S.pack_pattern(0, 3))
    rc = lib.tfrg_result_select_match(None, C.byref(term), 1, b"cat", 3, None, N.ROWS_I64, 1, 0, C.c_void_p(16),
                                      N.ROWS_I64, 1, C.c_void_p(16), None, 0, None)
    assert rc == -1 and lib.tfrg_last_error() == b"tfrg_result_select_match: no context"
    assert lib.tfrg_ctx_set_select_scan(None, 16) == -1
    assert lib.tfrg_abi_version() == 1
    assert (N.SEL_BYTES, N.SEL_BYTES_ANY, N.SEL_PREFIX, N.SEL_SUFFIX, N.SEL_CONTAINS) == (5, 6, 6, 7, 8)
    assert (N.SEL_MAX_PATTERN, N.SEL_MAX_PATTERN_BYTES) == (256, 2048) and N.SEL_SCAN_MIN <= 16
    assert len(N.SIGNATURES["tfrg_result_select_match"][1]) == len(N.SIGNATURES["tfrg_result_select_rows"][1]) + 2
