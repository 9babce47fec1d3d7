"""Ragged outputs on the host (no GPU): ``BatchResult.ragged`` / ``raggedify`` -- the numpy reference
the device path (tfrg_result_ragged_rows) is tested against -- must give, for row k, the oracle's
values of record ``rows[k]``, offsets that are the cumulative lengths, the four counters, and the
same rows as the other reference (``dense``) once padded or truncated; what it refuses; and the
C-ABI's argument check without a context. Every comparison is bit for bit (floats as uint32)."""

import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import _columns
from tests.test_dense_rows_host import bits, mixed, row_lists
from tfr_reader import _native as N
from tfr_reader import dense as D
from tfr_reader import ragged as R
from tfr_reader import synth

KINDS = {"int64": "int64_list", "int32": "int64_list", "float32": "float_list", "uint8": "bytes_list"}


def oracle_rows(buf, starts, ends) -> list[dict]:
    """Per record: (key, kind name) -> the oracle's value list (floats as uint32 bits, bytes as bytes)."""
    orc = O.Oracle()
    raw = buf.tobytes()
    out = []
    for s, e in zip(np.asarray(starts).tolist(), np.asarray(ends).tolist()):
        st, _, ent = orc.decode(raw[s + 12 : e - 4])
        assert st == 0
        out.append({(key.decode(), kind): vals for key, kind, vals in ent})
    return out


def want_row(rec: dict, sp: R.Ragged) -> tuple[np.ndarray, int, int]:
    """(the row's elements as unsigned bits before max_len, the record's value count, its length)."""
    udt = D.DTYPES[sp.dtype][3]
    vals = rec.get((sp.key, KINDS[sp.dtype]), [])
    if sp.dtype == "uint8":
        row = np.frombuffer(bytes(vals[0]), np.uint8) if vals else np.zeros(0, np.uint8)
    elif sp.dtype == "float32":
        row = np.array(vals, np.uint32)
    else:
        row = np.array(vals, np.int64).view(np.uint64).astype(udt)
    return row, len(vals), int(row.size)


def check(res, recs: list[dict], specs, rows) -> R.RaggedBatch:
    got = res.ragged(specs, rows=rows)
    picked = list(range(len(recs))) if rows is None else [int(v) for v in np.asarray(rows).reshape(-1)]
    m = len(picked)
    for sp in specs:
        k = sp.out_name
        values, offsets = got[k]
        assert values.dtype == D.DTYPES[sp.dtype][2] and offsets.dtype == np.int64 and offsets.shape == (m + 1,), k
        lens, st = [], [0, 0, 0, 0]
        for j, g in enumerate(picked):
            row, cnt, full = want_row(recs[g], sp)
            if sp.max_len is not None and full > sp.max_len:
                row = row[: sp.max_len]
                st[0] += 1
            st[1] += cnt == 0
            st[2] += sp.dtype == "uint8" and cnt > 1
            lens.append(row.size)
            have = bits(values[int(offsets[j]) : int(offsets[j + 1])])
            assert np.array_equal(have, row), (k, j, g)
        assert offsets.tolist() == np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.int64).tolist(), k
        assert values.size == offsets[m] == got.totals[k], k
        assert got.stats[k].tolist() == st, k
        assert got.overflowed[k] is False
    return got


def check_against_dense(res, specs, rows, width: int) -> None:
    """The other reference: dense(width=W) row k is the ragged slice padded or truncated to W."""
    got = res.ragged(specs, rows=rows)
    dn = res.dense([D.Dense(sp.key, sp.dtype, width, fill=0, lengths=True, name=sp.out_name) for sp in specs], rows=rows)
    for sp in specs:
        k = sp.out_name
        values, offsets = got[k]
        for j in range(len(offsets) - 1):
            row = bits(values[int(offsets[j]) : int(offsets[j + 1])])
            if sp.max_len is None:
                assert int(dn.lengths[k][j]) == row.size, (k, j)
            pad = np.zeros(width, row.dtype)
            pad[: min(width, row.size)] = row[:width]
            w = width if sp.max_len is None else min(width, sp.max_len)
            assert np.array_equal(bits(dn[k][j])[:w], pad[:w]), (k, j)
            if sp.max_len is None:
                assert np.array_equal(bits(dn[k][j]), pad), (k, j)


def variants(specs) -> list:
    """Every spec whole, and with max_len 1 and 3."""
    out = list(specs)
    for ml in (1, 3):
        out += [R.Ragged(sp.key, sp.dtype, ml, f"{sp.out_name}@{ml}") for sp in specs]
    return out


C1_SPECS = [R.Ragged("label", "int64"), R.Ragged("label", "int32", name="l32"), R.Ragged("id", "uint8")]
MIXED_SPECS = [R.Ragged("half", "int64"), R.Ragged("half", "int32", name="half32"), R.Ragged("empty", "float32"),
               R.Ragged("two", "int64", name="two_i"), R.Ragged("two", "float32", name="two_f"),
               R.Ragged("names", "uint8"), R.Ragged("absent", "int64")]


@pytest.fixture(scope="module")
def c1():
    fr = synth.framed(synth.c1_payloads(200))
    return _columns.batch_from_oracle(*fr), oracle_rows(*fr)


def test_c1_rows_are_the_oracles_records(c1):
    res, recs = c1
    specs = variants(C1_SPECS)
    for r in [None, *row_lists(200)]:
        check(res, recs, specs, r)
    got = check(res, recs, specs, [199, 0, 0, 63])
    assert got["label"][0].tolist() == [199, 0, 0, 63] and got["label"][1].tolist() == [0, 1, 2, 3, 4]
    assert bytes(got["id"][0]) == b"".join(b"img-%08d" % i for i in (199, 0, 0, 63))
    assert got.stats["id@3"].tolist() == [4, 0, 0, 0]  # a record drawn twice counts twice
    check_against_dense(res, specs, [5, 199, 5], 12)
    check_against_dense(res, specs, None, 2)


def test_mixed_rows_are_the_oracles_records():
    fr = synth.framed(mixed(120))
    res, recs = _columns.batch_from_oracle(*fr), oracle_rows(*fr)
    specs = variants(MIXED_SPECS)
    for r in [None, *row_lists(120)]:
        check(res, recs, specs, r)
    got = check(res, recs, specs, [5, 5, 5, 6, 0])
    # record 5: names = [b"aaaaa", b"second"] (two elements, the first one taken); 6 and 0: no element
    assert got.stats["names"].tolist() == [0, 2, 3, 0] and got.stats["names@3"].tolist() == [3, 2, 3, 0]
    assert got.stats["absent"].tolist() == [0, 5, 0, 0] and got.totals["absent"] == 0
    assert got["absent"][1].tolist() == [0] * 6 and got["absent"][0].dtype == np.int64
    for w in (1, 4):
        check_against_dense(res, specs, row_lists(120)[1], w)


def test_c3_rows_are_the_oracles_records():
    fr = synth.framed(synth.c3_payloads(24))
    res, recs = _columns.batch_from_oracle(*fr), oracle_rows(*fr)
    ints = [k for k, kd in zip(res.slot_key, res.slot_kind) if kd == 3]
    flts = [k for k, kd in zip(res.slot_key, res.slot_kind) if kd == 2]
    specs = variants([R.Ragged(ints[0], "int64"), R.Ragged(ints[3], "int32"), R.Ragged(flts[0], "float32"),
                      R.Ragged(flts[31], "float32")])
    for r in [None, *row_lists(24)[:4]]:
        check(res, recs, specs, r)
    check_against_dense(res, specs, row_lists(24)[0], 17)
    check_against_dense(res, specs, None, 64)


def test_raggedify_takes_plain_columns(c1):
    res = c1[0]
    got = R.raggedify([R.Ragged("label", "int64")], n=len(res), slot_key=res.slot_key, slot_kind=res.slot_kind,
                      row_splits=res.row_splits, slot_base=res.slot_base, i64=res.i64, f32=res.f32,
                      bytes_off=res.bytes_off, bytes_len=res.bytes_len, buf=res.buf, rows=[3, 1, 3])
    assert got["label"][0].tolist() == [3, 1, 3] and got["label"][1].tolist() == [0, 1, 2, 3]
    assert R.STAT_NAMES == ("truncated", "empty", "multi", "skipped")


def test_rows_and_specs_that_are_refused(c1):
    res = c1[0]
    sp = [R.Ragged("label", "int64")]
    with pytest.raises(IndexError, match=r"rows\[1\] = -1 "):
        res.ragged(sp, rows=[0, -1, 200])
    with pytest.raises(IndexError, match=r"rows\[2\] = 200 "):
        res.ragged(sp, rows=[0, 199, 200])
    with pytest.raises(IndexError):
        res.ragged(sp, rows=np.array([1 << 40]))
    with pytest.raises(ValueError, match="one-dimensional"):
        res.ragged(sp, rows=[[0, 1], [2, 3]])
    with pytest.raises(ValueError, match="integers"):
        res.ragged(sp, rows=[0.0, 1.0])
    empty = res.ragged(sp, rows=[])
    assert empty["label"][0].shape == (0,) and empty["label"][1].tolist() == [0]
    with pytest.raises(ValueError):
        R.Ragged("label", "int16")
    with pytest.raises(ValueError):
        R.Ragged("label", "int64", max_len=0)
    with pytest.raises(ValueError):
        res.ragged([R.Ragged("label", "int64"), R.Ragged("label", "int32")])  # (two outputs of one name)
    with pytest.raises(ValueError):
        res.ragged([])
    with pytest.raises(TypeError):
        res.ragged([D.Dense("label", "int64")])


def test_result_ragged_rows_without_a_context_is_an_argument_error():
    lib = N.lib()
    spec = N.TfrgRaggedSpec(slot=0, dtype=N.DENSE_I64, max_len=0, reserved=0, cap=0, values=None, offsets=16)
    assert lib.tfrg_result_ragged_rows(None, C.byref(spec), 1, None, N.ROWS_I64, 1, 0, None, None, None) == -1
    assert lib.tfrg_last_error().startswith(b"tfrg_result_ragged_rows")
    assert lib.tfrg_ctx_set_ragged_tile(None, 64) == -1
    assert C.sizeof(N.TfrgRaggedSpec) == 40 and N.RAGGED_MAX_SPECS == 64
