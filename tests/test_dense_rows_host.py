"""Row-selected dense outputs on the host (no GPU): ``densify(rows=r)`` -- the numpy reference the
device path (tfrg_result_dense_rows) is tested against -- must be ``densify()`` indexed by ``r``, with
the lengths, and with the counters recomputed for the rows of the output; what it refuses; and the
C-ABI's argument check without a context."""

import ctypes as C

import numpy as np
import pytest

from tests import _columns
from tfr_reader import _native as N
from tfr_reader import dense as D
from tfr_reader import synth, writer

QNAN = np.array(0x7FC01234, np.uint32).view(np.float32)


def mixed(n: int) -> list[bytes]:
    """Absent keys, empty lists, one key with two kinds, several bytes elements."""
    recs = []
    for i in range(n):
        ent = []
        if i % 2:
            ent.append(("half", "int64_list", [i, -i]))
        ent.append(("empty", "float_list", [] if i % 3 else [1.5, 2.5, 3.5]))
        ent.append(("two", "int64_list" if i % 4 else "float_list", [7] if i % 4 else [0.25]))
        ent.append(("names", "bytes_list", [b"a" * (i % 7), b"second"][: 1 + (i % 5 == 0)] if i % 6 else []))
        recs.append(writer.encode_example(ent))
    return recs


MIXED_SPECS = [
    D.Dense("half", "int64", 2, fill=-9, lengths=True),
    D.Dense("empty", "float32", 3, fill=QNAN, lengths=True),
    D.Dense("two", "int64", 1, fill=-1, name="two_i", lengths=True),
    D.Dense("two", "float32", 1, fill=-1.0, name="two_f", lengths=True),
    D.Dense("names", "uint8", 4, fill=0xEE, lengths=True),
    D.Dense("names", "uint8", 5, name="names5", lengths=True),
    D.Dense("absent", "int64", 2, fill=3, lengths=True),
]
C1_SPECS = [
    D.Dense("label", "int64", lengths=True),
    D.Dense("label", "int32", 3, fill=-1, name="l32x3", lengths=True),
    D.Dense("id", "uint8", 12, lengths=True),
    D.Dense("id", "uint8", 16, fill=0x20, name="id16", lengths=True),
    D.Dense("id", "uint8", 7, name="id7", lengths=True),
]


def bits(a: np.ndarray) -> np.ndarray:
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def counters(lens: np.ndarray, width: int, multi: np.ndarray, empty: np.ndarray) -> list[int]:
    return [int((lens > width).sum()), int((lens < width).sum()), int(empty.sum()), int(multi.sum())]


def per_record(res, sp: D.Dense) -> tuple[np.ndarray, np.ndarray]:
    """(records without a value, records with more than one bytes element) of a spec's slot, from
    the row splits."""
    n = len(res)
    s = D.find_slot(res.slot_key, res.slot_kind, sp.key, D.DTYPES[sp.dtype][1])
    if s is None:
        return np.ones(n, bool), np.zeros(n, bool)
    c = np.diff(np.asarray(res.row_splits[s]).astype(np.int64))
    return c == 0, (c > 1) if sp.dtype == "uint8" else np.zeros(n, bool)


def check_rows(res, specs, r) -> D.DenseBatch:
    """``res.dense(specs, rows=r)`` against ``res.dense(specs)`` indexed by r."""
    full = res.dense(specs)
    got = res.dense(specs, rows=r)
    idx = np.asarray(r, np.int64).reshape(-1)
    for sp in specs:
        k = sp.out_name
        assert got[k].dtype == full[k].dtype and got[k].shape == (idx.size, sp.width), k
        assert np.array_equal(bits(got[k]), bits(full[k])[idx]), k
        assert np.array_equal(got.lengths[k], full.lengths[k][idx]), k
        empty, multi = per_record(res, sp)
        assert got.stats[k].tolist() == counters(full.lengths[k][idx], sp.width, multi[idx], empty[idx]), k
    assert got.skipped == 0
    return got


def row_lists(n: int) -> list:
    rng = np.random.default_rng(11)
    return [rng.permutation(n), rng.integers(0, n, 2 * n + 3), np.full(5, n - 1), [], np.zeros(0, np.int32),
            list(range(n - 1, -1, -1)), rng.integers(0, n, 9).astype(np.int32), rng.integers(0, n, 9).astype(np.uint8)]


@pytest.fixture(scope="module")
def c1():
    return _columns.batch_from_oracle(*synth.framed(synth.c1_payloads(200)))


def test_c1_rows_equal_indexing(c1):
    for r in row_lists(200):
        got = check_rows(c1, C1_SPECS, r)
    r = [199, 0, 0, 63]
    got = check_rows(c1, C1_SPECS, r)
    assert got["label"][:, 0].tolist() == r and [bytes(x) for x in got["id"]] == [b"img-%08d" % i for i in r]
    assert got.stats["id7"].tolist() == [4, 0, 0, 0] and got.stats["id16"].tolist() == [0, 4, 0, 0]  # a record drawn twice counts twice


def test_mixed_rows_equal_indexing():
    res = _columns.batch_from_oracle(*synth.framed(mixed(120)))
    for r in row_lists(120):
        got = check_rows(res, MIXED_SPECS, r)
    got = check_rows(res, MIXED_SPECS, [5, 5, 5])
    assert got.stats["names"].tolist() == [3, 0, 0, 3] and got.stats["absent"].tolist() == [0, 3, 3, 0]


def test_c3_rows_equal_indexing():
    res = _columns.batch_from_oracle(*synth.framed(synth.c3_payloads(256, max_len=64)))
    ints = [k for k, kd in zip(res.slot_key, res.slot_kind) if kd == 3]
    flts = [k for k, kd in zip(res.slot_key, res.slot_kind) if kd == 2]
    specs = [D.Dense(ints[0], "int64", 64, fill=-1, lengths=True), D.Dense(ints[3], "int32", 17, fill=-1, lengths=True),
             D.Dense(flts[0], "float32", 64, fill=QNAN, lengths=True), D.Dense(flts[31], "float32", 1, fill=QNAN, lengths=True)]
    for r in row_lists(256)[:4]:
        check_rows(res, specs, r)


def test_densify_takes_rows_directly(c1):
    r = [3, 1, 3]
    got = D.densify([D.Dense("label", "int64")], n=len(c1), slot_key=c1.slot_key, slot_kind=c1.slot_kind,
                    row_splits=c1.row_splits, slot_base=c1.slot_base, i64=c1.i64, f32=c1.f32, bytes_off=c1.bytes_off,
                    bytes_len=c1.bytes_len, buf=c1.buf, rows=r)
    assert got["label"][:, 0].tolist() == r


def test_rows_out_of_range_and_of_the_wrong_shape(c1):
    sp = [D.Dense("label", "int64")]
    with pytest.raises(IndexError, match=r"rows\[1\] = -1 "):
        c1.dense(sp, rows=[0, -1, 200])
    with pytest.raises(IndexError, match=r"rows\[2\] = 200 "):
        c1.dense(sp, rows=[0, 199, 200])
    with pytest.raises(IndexError):
        c1.dense(sp, rows=np.array([1 << 40]))
    with pytest.raises(ValueError, match="one-dimensional"):
        c1.dense(sp, rows=[[0, 1], [2, 3]])
    with pytest.raises(ValueError, match="integers"):
        c1.dense(sp, rows=[0.0, 1.0])
    with pytest.raises(ValueError, match="integers"):
        c1.dense(sp, rows=np.array([True, False]))
    assert c1.dense(sp, rows=[])["label"].shape == (0, 1)


def test_result_dense_rows_without_a_context_is_an_argument_error():
    lib = N.lib()
    spec = N.TfrgDenseSpec(slot=0, dtype=N.DENSE_I64, width=1, reserved=0, fill=0, out=16, lengths=None)
    assert lib.tfrg_result_dense_rows(None, C.byref(spec), 1, C.c_void_p(16), N.ROWS_I64, 1, 0, None, None, None) == -1
    assert lib.tfrg_last_error().startswith(b"tfrg_result_dense_rows")
    assert (N.ROWS_I32, N.ROWS_I64) == (0, 1)
