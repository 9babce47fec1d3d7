"""Dense outputs on the host (no GPU): the numpy densifier behind ``BatchResult.dense`` against the
oracle's decode of every record, the ``Dense`` spec validation, and the C-ABI of tfrg_result_dense
(struct layout against the header, argument check without a context)."""

import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O
from tests import _columns
from tfr_reader import _native as N
from tfr_reader import dense as D
from tfr_reader import synth, writer

INCLUDE = Path(__file__).resolve().parents[1] / "include"
KIND = {"int64": "int64_list", "int32": "int64_list", "float32": "float_list", "uint8": "bytes_list"}
QNAN = np.array(0x7FC01234, np.uint32).view(np.float32)


def oracle_dense(buf, starts, ends, sp: D.Dense):
    """(values as unsigned bits, lengths, stats) of one spec, straight from the oracle's entries."""
    orc = O.Oracle()
    raw = buf.tobytes()
    udt = D.DTYPES[sp.dtype][3]
    n = len(starts)
    out = np.full((n, sp.width), sp.fill_bits, udt)
    lens = np.zeros(n, np.int32)
    st = np.zeros(4, np.uint32)
    for r, (s, e) in enumerate(zip(np.asarray(starts).tolist(), np.asarray(ends).tolist())):
        status, _, ent = orc.decode(raw[s + 12 : e - 4], views=True)
        assert status == 0
        vals = None
        for key, kind, v in ent:
            if key == sp.key.encode() and kind == KIND[sp.dtype]:
                vals = v
        c = len(vals) if vals else 0
        if sp.dtype == "uint8":
            ln = 0
            if c:
                o, ln = vals[0]
                elem = np.frombuffer(raw, np.uint8, ln, s + 12 + o)
                out[r, : min(ln, sp.width)] = elem[: sp.width]
            st[3] += c > 1
        else:
            ln = c
            mask = (1 << (8 * np.dtype(udt).itemsize)) - 1
            for j in range(min(c, sp.width)):
                out[r, j] = int(vals[j]) & mask
        lens[r] = ln
        st[0] += ln > sp.width
        st[1] += ln < sp.width
        st[2] += c == 0
    return out, lens, st


def check(buf, st, en, specs):
    res = _columns.batch_from_oracle(buf, st, en)
    got = res.dense(specs)
    same = D.densify(specs, n=len(res), slot_key=res.slot_key, slot_kind=res.slot_kind, row_splits=res.row_splits,
                     slot_base=res.slot_base, i64=res.i64, f32=res.f32, bytes_off=res.bytes_off,
                     bytes_len=res.bytes_len, buf=res.buf)
    for sp in specs:
        want, lens, stats = oracle_dense(buf, st, en, sp)
        name = sp.out_name
        assert got[name].dtype == D.DTYPES[sp.dtype][2] and got[name].shape == (len(st), sp.width)
        assert np.array_equal(got[name].view(want.dtype), want), name
        assert np.array_equal(same[name].view(want.dtype), want), name
        assert np.array_equal(got.stats[name], stats), (name, got.stats[name], stats)
        if sp.lengths:
            assert np.array_equal(got.lengths[name], lens), name
        else:
            assert name not in got.lengths
    return got


def test_c1_against_the_oracle():
    buf, st, en = synth.framed(synth.c1_payloads(300))
    got = check(buf, st, en, [
        D.Dense("label", "int64", lengths=True),
        D.Dense("label", "int32", 3, fill=-1, name="label32"),
        D.Dense("id", "uint8", 12, lengths=True),
        D.Dense("id", "uint8", 16, fill=0x20, name="id16"),
        D.Dense("id", "uint8", 8, name="id8", lengths=True),
    ])
    assert got["label"][:, 0].tolist() == [i % 1000 for i in range(300)]
    assert bytes(got["id"][7]) == b"img-00000007" and bytes(got["id16"][7]) == b"img-00000007    "
    assert got.stats["id8"].tolist() == [300, 0, 0, 0] and got.stats["label32"].tolist() == [0, 300, 0, 0]


def test_c3_against_the_oracle():
    buf, st, en = synth.framed(synth.c3_payloads(64))
    res = _columns.batch_from_oracle(buf, st, en)
    ints = [k for k, kd in zip(res.slot_key, res.slot_kind) if kd == 3][:3]
    flts = [k for k, kd in zip(res.slot_key, res.slot_kind) if kd == 2][:3]
    assert ints and flts
    specs = [D.Dense(k, "int64", 17, fill=-1, lengths=True) for k in ints]
    specs += [D.Dense(k, "float32", 64, fill=QNAN, lengths=True) for k in flts]
    specs += [D.Dense(ints[0], "int32", 1, name="narrow"), D.Dense(flts[0], "float32", 5, name="f5")]
    got = check(buf, st, en, specs)
    assert int(got.stats[ints[0]][0]) > 0 and int(got.stats[ints[0]][1]) > 0  # truncation and padding both occur


def test_missing_keys_empty_lists_and_two_kinds():
    recs = []
    for i in range(40):
        ent = []
        if i % 2:
            ent.append(("half", "int64_list", [i, -i]))
        ent.append(("empty", "float_list", [] if i % 3 else [1.5, 2.5, 3.5]))
        ent.append(("two", "int64_list" if i % 4 else "float_list", [7] if i % 4 else [0.25]))
        ent.append(("names", "bytes_list", [b"a" * (i % 7), b"second"][: 1 + (i % 5 == 0)] if i % 6 else []))
        recs.append(writer.encode_example(ent))
    buf, st, en = synth.framed(recs)
    got = check(buf, st, en, [
        D.Dense("half", "int64", 2, fill=-9, lengths=True),
        D.Dense("empty", "float32", 3, fill=QNAN, lengths=True),
        D.Dense("two", "int64", 1, fill=-1, name="two_i", lengths=True),
        D.Dense("two", "float32", 1, fill=-1.0, name="two_f", lengths=True),
        D.Dense("names", "uint8", 4, fill=0xEE, lengths=True),
        D.Dense("names", "uint8", 5, name="names5"),
        D.Dense("absent", "int64", 2, fill=3, lengths=True),
    ])
    assert (got["absent"] == 3).all() and not got.lengths["absent"].any()
    assert got.stats["absent"].tolist() == [0, 40, 40, 0]
    assert int(got.stats["names"][3]) > 0 and int(got.stats["half"][2]) == 20
    res = _columns.batch_from_oracle(buf, st, en)
    with pytest.raises(KeyError):
        res.dense([D.Dense("absent", "int64")], strict=True)
    with pytest.raises(ValueError, match="half"):
        res.dense([D.Dense("half", "int64", 2)], strict=True)
    assert res.dense([D.Dense("two", "int64", 1, fill=-1)])["two"][:, 0].tolist() == [7 if i % 4 else -1 for i in range(40)]


def test_strict_passes_on_fixed_shapes():
    buf, st, en = synth.framed(synth.c1_payloads(20))
    res = _columns.batch_from_oracle(buf, st, en)
    got = res.dense([D.Dense("label", "int64"), D.Dense("id", "uint8", 12)], strict=True)
    assert got["label"].shape == (20, 1)
    with pytest.raises(ValueError, match="'id'"):
        res.dense([D.Dense("id", "uint8", 13)], strict=True)


def test_spec_validation():
    with pytest.raises(ValueError):
        D.Dense("k", "float64")
    for w in (0, 4097, 1.5):
        with pytest.raises(ValueError):
            D.Dense("k", "int64", w)
    with pytest.raises(ValueError):
        D.Dense("k", "uint8", fill=256)
    with pytest.raises(ValueError):
        D.Dense("k", "int32", fill=1 << 40)
    with pytest.raises(TypeError):
        D.Dense(b"k", "int64")
    assert D.Dense("k", "float32", fill=1.0).fill_bits == 0x3F800000
    assert D.Dense("k", "int64", fill=-1).fill_bits == (1 << 64) - 1
    assert D.Dense("k", "int32", fill=-2).fill_bits == 0xFFFFFFFE
    with pytest.raises(ValueError):
        D.check_specs([])
    with pytest.raises(ValueError):
        D.check_specs([D.Dense(f"k{i}", "int64") for i in range(65)])
    with pytest.raises(ValueError, match="name="):
        D.check_specs([D.Dense("k", "int64"), D.Dense("k", "int32")])
    with pytest.raises(TypeError):
        D.check_specs(["k"])


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_dense_spec_layout_matches_the_header(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "tfrg.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(tfrg_dense_spec));']
    for fname, _ in N.TfrgDenseSpec._fields_:
        lines.append(f'  printf("{fname} %zu %zu\\n", offsetof(tfrg_dense_spec, {fname}), '
                     f"sizeof(((tfrg_dense_spec*)0)->{fname}));")
    lines.append('  printf("consts %d %d %d %d %d %d\\n", TFRG_DENSE_I64, TFRG_DENSE_I32, TFRG_DENSE_F32, TFRG_DENSE_U8, '
                 "TFRG_DENSE_MAX_SPECS, TFRG_DENSE_MAX_WIDTH);")
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(INCLUDE), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert int(out[0].split()[1]) == C.sizeof(N.TfrgDenseSpec)
    for line, (fname, _) in zip(out[1:], N.TfrgDenseSpec._fields_):
        name, off, size = line.split()
        f = getattr(N.TfrgDenseSpec, fname)
        assert (name, int(off), int(size)) == (fname, f.offset, f.size)
    assert [int(x) for x in out[-1].split()[1:]] == [N.DENSE_I64, N.DENSE_I32, N.DENSE_F32, N.DENSE_U8,
                                                     N.DENSE_MAX_SPECS, N.DENSE_MAX_WIDTH]


def test_result_dense_without_a_context_is_an_argument_error():
    lib = N.lib()
    spec = N.TfrgDenseSpec(slot=0, dtype=N.DENSE_I64, width=1, reserved=0, fill=0, out=16, lengths=None)
    assert lib.tfrg_result_dense(None, C.byref(spec), 1, None, None) == -1  # TFRG_E_ARG
    assert b"tfrg_result_dense" in lib.tfrg_last_error()
