"""Filtered row lists on the device (tfrg_result_select_rows: k_sel_eval / k_sel_scan / k_sel_write):
the selection must equal the numpy reference -- ``BatchResult.select`` over the same decode's fetched
columns (tests/test_select_host.py checks that one against the oracle) -- exactly: the list, the
count, the two counters. Every output is prefilled with 0xA5 inside a larger buffer: what lies before
``d_out``, after the stored prefix and after ``cap`` keeps the poison. Every predicate that is not an
explicit "all" / "none" case selects, by the reference alone, some candidates and not all of them."""

import ctypes as C
import math

import numpy as np
import pytest

from tests.test_dense_rows_host import mixed
from tests.test_ragged_gpu import BYTE_LENS, bytes_payloads
from tfr_reader import _native as N
from tfr_reader import dense as D
from tfr_reader import hip, shard, synth, writer
from tfr_reader import ragged as R
from tfr_reader import select as S
from tfr_reader.select import Status, Term, is_in

pytestmark = pytest.mark.gpu

COLS = ("status", "aux", "verdict", "order", "row_splits", "i64", "f32", "bytes_off", "bytes_len", "slot_base")
POISON = 0xA5
GUARD = 256
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
OPS = list(S.OPS)
ISZ = {N.ROWS_I32: 4, N.ROWS_I64: 8}


def dev():
    import torch

    return torch.device("cuda", 0)


def to_dev(rows, dtype=np.int64):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(rows, dtype))).to(dev())


def new_decoder(env: dict | None = None, spec_varint: bool = False):
    mp = pytest.MonkeyPatch()
    mp.setenv("TFRG_OPTIMISTIC", "1")  # (read at context creation; the suite may run with 0)
    mp.setenv("TFRG_TEMPLATES", "1")
    for k, v in (env or {}).items():
        mp.setenv(k, v)
    try:
        return hip.HipDecoder(0, spec_varint)
    finally:
        mp.undo()


@pytest.fixture
def dec():
    d = new_decoder()
    yield d
    d.close()


class Ref:
    """The host reference of one decode: per ``where`` the records' verdicts, computed once
    (``select_mask`` over the fetched columns), then applied to candidate lists."""

    def __init__(self, res) -> None:
        self.res, self.n, self.cols, self.masks = res, len(res), S.batch_columns(res), {}

    def mask(self, where) -> np.ndarray:
        key = repr(where)
        if key not in self.masks:
            self.masks[key] = S.select_mask(where, **self.cols)
        return self.masks[key]

    def expect(self, where, rows=None, row0: int = 0, kind: str = "some"):
        """(entries, (selected, skipped)); ``kind`` is asserted on the reference alone."""
        want, (sel, skip) = S.apply_mask(self.mask(where), rows, row0)
        cands = self.n if rows is None else len(rows)
        if kind == "some":
            assert 0 < sel < cands - skip, (where, sel, skip, cands)
        elif kind == "all":
            assert sel == cands - skip > 0, where
        elif kind == "none":
            assert sel == 0 and cands - skip > 0, where
        return want, (sel, skip)


def run(d, where, want, wstats, rows=None, rdt=np.int64, row0: int = 0, odt: int = N.ROWS_I64, cap=None, m=None,
        null_out: bool = False, base=None):
    """One raw ``tfrg_result_select_rows`` call over poisoned outputs, checked against (want, wstats).
    ``cap``: default the count + 3. ``base``: a count to APPEND to (the list then starts there)."""
    import torch

    terms = S.fold(d, S.check_where(where))
    assert terms is not None
    isz = ISZ[odt]
    start = 0 if base is None else base
    cap = start + len(want) + 3 if cap is None else cap
    big = torch.full((GUARD + cap * isz + GUARD,), POISON, dtype=torch.uint8, device=dev())
    cnt = torch.full((GUARD + 8 + GUARD,), POISON, dtype=torch.uint8, device=dev())
    st = torch.full((GUARD + 8 + GUARD,), POISON, dtype=torch.uint8, device=dev())
    count = cnt[GUARD : GUARD + 8].view(torch.int64)
    if base is not None:
        count.fill_(base)
    rw = None
    if rows is not None:
        d_rows = to_dev(rows, rdt)
        rw = (d_rows.data_ptr(), N.ROWS_I64 if rdt == np.int64 else N.ROWS_I32)
        m = len(rows)
    elif m is None:
        m = d._last_n
    out_ptr = None if null_out else big.data_ptr() + GUARD
    # (no consumer stream is given, so nothing orders the call's memsets on the decode's stream after the
    # poison fills queued above on torch's: without a row list to upload, they have to be waited for here)
    torch.cuda.synchronize()
    S.launch(d, terms, rw, m, row0, (out_ptr, odt), cap, count.data_ptr(), st.data_ptr() + GUARD,
             N.SEL_APPEND if base is not None else 0, None)
    torch.cuda.synchronize()
    host, hc, hs = big.cpu().numpy(), cnt.cpu().numpy(), st.cpu().numpy()
    assert int(hc[GUARD : GUARD + 8].view(np.int64)[0]) == start + len(want)
    assert (hc[:GUARD] == POISON).all() and (hc[GUARD + 8 :] == POISON).all()
    assert tuple(hs[GUARD : GUARD + 8].view(np.uint32).tolist()) == tuple(wstats)
    assert (hs[:GUARD] == POISON).all() and (hs[GUARD + 8 :] == POISON).all()
    kept = 0 if null_out else max(0, min(start + len(want), cap) - start)
    lo = GUARD + start * isz
    if kept:
        got = host[lo : lo + kept * isz].view(np.int64 if odt == N.ROWS_I64 else np.int32)
        assert got.tolist() == [int(v) for v in want[:kept]]
    assert (host[:lo] == POISON).all() and (host[lo + kept * isz :] == POISON).all()


def check_api(d, ref: Ref, where, rows=None, dtype=np.int64, kind: str = "some"):
    """``HipDecoder.select``: exact, with a padded capacity, and into ``out=``."""
    import torch

    want, wstats = ref.expect(where, rows, 0, kind)
    d_rows = None if rows is None else to_dev(rows, dtype)
    sel = d.select(where, rows=d_rows)
    assert sel.rows.dtype == torch.int64 and sel.rows.cpu().tolist() == want.tolist()
    assert sel.count == len(want) and sel.stats == wstats and not sel.overflowed
    pad = d.select(where, rows=d_rows, capacity=len(want) + 5, dtype="int32")
    assert pad.rows.dtype == torch.int32 and pad.rows.cpu().tolist() == want.tolist() + [-1] * 5
    assert pad.count == len(want) and pad.stats == wstats and not pad.overflowed
    if len(want) > 1:
        short = d.select(where, rows=d_rows, capacity=len(want) - 1)
        assert short.rows.cpu().tolist() == want.tolist()[:-1] and short.overflowed and short.count == len(want)
    return want


# ------------------------------------------------------------------------------------ 1. optimistic C1
N1 = 5000
BAD64 = [-1, N1, N1 + 1, (1 << 31) - 1, I64_MIN, I64_MAX, -N1, 1 << 32, (1 << 32) + 5, -(1 << 32)]
BAD32 = [-1, N1, N1 + 1, (1 << 31) - 1, -(1 << 31), -N1]
C1_SOME = [[Term("label", "int64", op, 500)] for op in OPS] + [
    [Term("label", "int64", ">=", 10), Term("label", "int32", "<", 20)],
    [[Term("label", "int64", "==", 1), Term("label", "int64", "==", 3), Term("label", "int64", ">", 990)]],
]
C1_ALL = [[Term("id", "uint8", "==", 12, "bytes_len")], [Term("label", "int64", "==", 1, "count")], [Status("==", 0)],
          [Term("id", "uint8", "==", 1, "count"), Status("==", 0), Term("id", "uint8", ">", 11, "bytes_len")], []]
C1_NONE = [[Term("id", "uint8", "!=", 12, "bytes_len")], [Status("!=", 0)]]


def with_bad(bad: list[int], m: int) -> list[int]:
    good = np.random.default_rng(m).integers(0, N1, m).tolist()
    return [bad[(k // 3) % len(bad)] if k % 3 == 1 else good[k] for k in range(m)]


def c1_row_lists() -> list:
    rng = np.random.default_rng(1)
    return [(None, np.int64), (rng.permutation(N1), np.int64), (rng.permutation(N1)[:1237], np.int32),
            (rng.integers(0, N1, 2 * N1 + 3), np.int64), (rng.integers(0, N1, 777), np.int32),
            (with_bad(BAD64, 1027), np.int64), (with_bad(BAD32, 1027), np.int32)]


def check_c1(d, res, fr) -> None:
    ref = Ref(res)
    lists = c1_row_lists()
    for j, where in enumerate(C1_SOME):
        for i, (rows, dtype) in enumerate(lists):
            want, wstats = ref.expect(where, rows)
            run(d, where, want, wstats, rows, dtype, odt=N.ROWS_I32 if (i + j) % 2 else N.ROWS_I64, m=N1)
    for where in C1_ALL:
        run(d, where, *ref.expect(where, kind="all"), m=N1)
        run(d, where, *ref.expect(where, lists[5][0], kind="all"), lists[5][0])
    for where in C1_NONE:
        run(d, where, *ref.expect(where, kind="none"), m=N1)
        run(d, where, *ref.expect(where, BAD64 + [7], kind="none"), BAD64 + [7])
    # every candidate out of range: nothing is read, nothing selected
    assert ref.expect(C1_SOME[0], BAD64, kind=None)[1] == (0, len(BAD64))
    run(d, C1_SOME[0], *ref.expect(C1_SOME[0], BAD64, kind=None), BAD64)
    run(d, C1_SOME[0], *ref.expect(C1_SOME[0], BAD32, kind=None), BAD32, np.int32, odt=N.ROWS_I32)
    # row0 through the C call
    where = C1_SOME[6]
    row0 = 1 << 40
    rows = [row0 + (7 * k) % N1 for k in range(3000)]
    rows[3], rows[10], rows[11], rows[40] = row0 - 1, row0 + N1, 5, I64_MIN  # (5: in range only without row0)
    run(d, where, *ref.expect(where, rows, row0), rows, np.int64, row0)
    rows = [100 + (11 * k) % (N1 + 50) for k in range(3000)]
    run(d, where, *ref.expect(where, rows, 100), rows, np.int32, 100, odt=N.ROWS_I32)
    rows = [-3 + k for k in range(400)]
    run(d, where, *ref.expect(where, rows, -3), rows, np.int32, -3, odt=N.ROWS_I32)
    run(d, where, *ref.expect(where, list(range(N1 + 70))), None, m=N1 + 70)  # (rows NULL, m above n: the tail is skipped)
    # capacities, the count-only call, both output types
    where = C1_SOME[2]
    rows = lists[3][0]
    want, wstats = ref.expect(where, rows)
    for odt in (N.ROWS_I32, N.ROWS_I64):
        for cap in (len(want) + 3, len(want), len(want) - 1, 0):
            run(d, where, want, wstats, rows, odt=odt, cap=cap)
        run(d, where, want, wstats, rows, odt=odt, null_out=True)
    # appending to a count that is already there
    run(d, where, want, wstats, rows, base=17)
    run(d, where, want, wstats, rows, base=17, cap=17 + len(want) - 5)
    # the Python entry
    check_api(d, ref, C1_SOME[7])
    check_api(d, ref, C1_SOME[1], lists[6][0], np.int32)
    # the full view is still there afterwards
    again = d._fetch(*fr, d.info(), False)
    for k in COLS:
        assert np.array_equal(getattr(again, k), getattr(res, k)), k


def test_optimistic_c1_decode():
    d = new_decoder()
    try:
        fr = synth.framed(synth.c1_payloads(N1))
        res = d.decode(*fr)
        assert int(res.info.implicit_cols) == 7 and int(res.info.placed_slots) & 3 == 3
        check_c1(d, res, fr)
        fresh = new_decoder()
        try:
            want = fresh.decode(*fr)
            again = d._fetch(*fr, d.info(), False)
            for k in COLS:
                assert np.array_equal(getattr(again, k), getattr(want, k)), k
        finally:
            fresh.close()
    finally:
        d.close()


# ------------------------------------------------------------------------------------ 2. other decode paths
def test_c1_decode_that_stores_row_splits_and_lengths():
    d = new_decoder({"TFRG_OPTIMISTIC": "0"})
    try:
        fr = synth.framed(synth.c1_payloads(N1))
        res = d.decode(*fr)
        assert int(res.info.implicit_cols) == 0
        check_c1(d, res, fr)
    finally:
        d.close()


def test_c1_after_a_hinted_decode_that_reruns(dec):
    fr = synth.framed(synth.c1_payloads(N1))
    dec.set_value_caps(100, 100, 100)  # far below the batch's values
    res = dec.decode(*fr)
    assert dec.device_bytes()[1] >= 1
    check_c1(dec, res, fr)


# ------------------------------------------------------------------------------------ 3. mixed
def test_absent_keys_empty_lists_two_kinds_and_several_elements(dec):
    n = 600
    res = dec.decode(*synth.framed(mixed(n)))
    ref = Ref(res)
    rng = np.random.default_rng(n)
    lists = [None, rng.permutation(n), rng.integers(0, n, 2 * n + 5), [0, n, -1, 5, I64_MAX, 7, 8, 9, 10, 11, 12, 13]]
    some = [[Term("half", "int64", "<", 0, index=1)], [Term("empty", "float32", "==", 3.5, index=2)],
            [Term("two", "int64", "==", 7)], [Term("two", "float32", "==", 0.25)], [Term("two", "int32", "!=", 8)],
            [Term("names", "uint8", "==", 0, "count")], [Term("names", "uint8", "==", 1, "count")],
            [Term("names", "uint8", "==", 2, "count")], [is_in("half", "int64", [1, 3, 5, 7, 9, 11, 13, 301])],
            [[Term("two", "float32", "<", 1.0, "any"), Term("half", "int64", ">", 300, "any")],
             Term("empty", "float32", "<=", 3, "count")]]
    some += [[Term("names", "uint8", "==", ln, "bytes_len")] for ln in range(7)]
    for where in some:
        for rows in lists:
            run(dec, where, *ref.expect(where, rows), rows, m=n)
    # NE on a missing value is false: only records that have the value pass
    where = [Term("half", "int64", "!=", 5)]
    want = check_api(dec, ref, where)
    assert all(g % 2 for g in want.tolist()) and 5 not in want.tolist()
    # an absent key under every subject: folded on the host (value / any false, count / bytes_len compare 0)
    for op in OPS:
        zero = S._PY_OPS[op](0, 0)
        for t in (Term("absent", "int64", op, 0), Term("absent", "float32", op, 0.0, "any")):
            assert S.fold(dec, [[t]]) is None
            sel = dec.select([t], rows=to_dev(lists[3]))
            assert sel.rows.numel() == 0 and sel.count == 0 and sel.stats == (0, 3)
            check_api(dec, ref, [[t, Term("half", "int64", ">", 100)]])
        for t in (Term("absent", "int64", op, 0, "count"), Term("absent", "uint8", op, 0, "bytes_len")):
            assert S.fold(dec, [[t]]) == ([] if zero else None)
            check_api(dec, ref, [t], kind="all" if zero else "none")
            check_api(dec, ref, [t, Term("half", "int64", ">", 100)], kind="some" if zero else "none")


# ------------------------------------------------------------------------------------ 4. lists and tiles
@pytest.fixture(scope="module")
def c3():
    d = new_decoder()
    res = d.decode(*synth.framed(synth.c3_payloads(96)))
    ints = [k for k, kd in zip(res.slot_key, res.slot_kind) if kd == 3]
    flts = [k for k, kd in zip(res.slot_key, res.slot_kind) if kd == 2]
    assert len(ints) == 32 and len(flts) == 32
    yield d, Ref(res), ints, flts
    d.close()


def test_c3_any_late_values_and_full_term_tables(c3):
    d, ref, ints, flts = c3
    rng = np.random.default_rng(3)
    lists = [None, rng.integers(0, 96, 1000), with_small_bad(300)]
    wheres = [[Term(ints[0], "int64", "<", 0, "any")], [Term(flts[0], "float32", ">", 2.0, "any")],
              [Term(ints[5], "int64", ">", 1 << 29, "any"), Term(flts[7], "float32", "<", -1.5, "any")],
              [[Term(k, "int64", ">=", 0, index=63) for k in ints]], [Term(flts[1], "float32", "<", 0.0, index=40)],
              [Term(k, "int64", ">", 1, "count") for k in ints],  # 32 terms in 32 groups
              [[Term(k, "float32", "==", 0, "count") for k in flts]]]  # 32 terms in one group
    for where in wheres:
        for rows in lists:
            run(d, where, *ref.expect(where, rows), rows, m=96)


def with_small_bad(m: int) -> list[int]:
    good = np.random.default_rng(m).integers(0, 96, m).tolist()
    bad = [-1, 96, I64_MIN, I64_MAX, 1 << 32]
    return [bad[(k // 5) % len(bad)] if k % 5 == 2 else good[k] for k in range(m)]


def test_small_tiles_and_the_scans_second_pass(c3):
    d, ref, ints, flts = c3
    where = [Term(ints[2], "int64", "<", 0, "any"), Term(flts[2], "float32", ">", 0.0, "any")]
    d.set_select_tile(64)
    try:
        rng = np.random.default_rng(4)
        for m in (0, 1, 63, 64, 65, 127, 128, 129, 4097):
            rows = rng.integers(0, 96, m)
            run(d, where, *ref.expect(where, rows, kind="some" if m > 60 else None), rows, np.int32 if m % 2 else np.int64)
        edge = N.SEL_SCAN_THREADS * N.SEL_TILE_MIN  # that many candidates fill the scan's first pass
        for m in (edge - 1, edge, edge + 1):
            rows = rng.integers(-2, 98, m)
            run(d, where, *ref.expect(where, rows), rows, np.int32, odt=N.ROWS_I32)
    finally:
        d.set_select_tile(0)
    for bad in (1, 32, 96, 8192):
        with pytest.raises(N.NativeError):
            d.set_select_tile(bad)


def test_default_tile_with_many_candidates(c3):
    d, ref, ints, flts = c3
    where = [Term(ints[3], "int64", ">", 10, "count")]
    rows = np.random.default_rng(6).integers(0, 96, 70001)
    rows[::1000] = -1
    before = d.device_bytes()[0]
    run(d, where, *ref.expect(where, rows), rows)
    assert d.device_bytes()[0] >= max(before, (70001 // 64) * 8)  # (the ballot words live in the context)


# ------------------------------------------------------------------------------------ 5. value edges
DEN = float(np.array(1, np.uint32).view(np.float32))
FLOATS = [math.nan, 0.0, -0.0, math.inf, -math.inf, DEN, -DEN, 1.5, -1.5]
INTS = [I64_MIN, -1, 0, 1, I64_MAX]


def edge_payloads() -> list[bytes]:
    out = []
    nf, ni = len(FLOATS), len(INTS)
    for i in range(nf * ni):
        f, g = FLOATS[i % nf], FLOATS[(i // nf + i) % nf]
        a, b = INTS[i % ni], INTS[(i // ni + 2 * i) % ni]
        out.append(writer.encode_example([("f", "float_list", np.array([f], np.float32)),
                                          ("fs", "float_list", np.array([g, f, g][: i % 4], np.float32)),
                                          ("i", "int64_list", [a]), ("is", "int64_list", [b, a, b][: i % 4])]))
    return out


@pytest.fixture
def spec_dec():
    d = new_decoder(spec_varint=True)  # (varints by the protobuf rules: every int64 arrives as written)
    yield d
    d.close()


def test_float_and_int_edge_values(spec_dec):
    dec = spec_dec
    res = dec.decode(*synth.framed(edge_payloads()))
    assert np.array_equal(np.unique(res.f32), np.unique(np.array(FLOATS, np.float32).view(np.uint32)))
    assert np.unique(res.i64).tolist() == INTS
    ref = Ref(res)
    n = len(res)
    for key, dtype, operands, least in (("f", "float32", FLOATS, 5), ("i", "int64", INTS, 4)):
        for rhs in operands:
            for subject, k in (("value", key), ("any", key + "s")):
                some = 0
                for op in OPS:
                    where = [Term(k, dtype, op, rhs, subject)]
                    want, wstats = ref.expect(where, kind=None)
                    some += 0 < wstats[0] < n
                    run(dec, where, want, wstats, m=n)
                # (a NaN operand is the explicit all / none case: true under != alone)
                if not (isinstance(rhs, float) and math.isnan(rhs)):
                    assert some >= least - (subject == "any"), (k, rhs, some)
    # the rules themselves, on the device: what the values are is known here
    f = np.array([FLOATS[i % len(FLOATS)] for i in range(n)], np.float32)
    for where, want in (([Term("f", "float32", "==", 0.0)], np.flatnonzero(f == 0)),
                        ([Term("f", "float32", ">", 0.0)], np.flatnonzero(f > 0)),
                        ([Term("f", "float32", "<", -0.0)], np.flatnonzero(f < 0)),
                        ([Term("f", "float32", "!=", math.nan)], np.arange(n)),
                        ([Term("f", "float32", "<=", math.nan)], np.zeros(0, np.int64)),
                        ([Term("f", "float32", "!=", 1.5)], np.flatnonzero(f != 1.5)),
                        ([Term("f", "float32", ">=", DEN)], np.flatnonzero(f >= np.float32(DEN)))):
        assert dec.select(where).rows.cpu().tolist() == want.tolist(), where
    assert 0 < len(np.flatnonzero(f > 0)) < n and (f == 0).sum() == 2 * (n // len(FLOATS))


# ------------------------------------------------------------------------------------ 6. bytes lengths
@pytest.mark.parametrize("materialize", [False, True])
def test_bytes_lengths(dec, materialize):
    res = dec.decode(*synth.framed(bytes_payloads()), materialize_bytes=materialize)
    assert (res.bytes_data is not None) == materialize
    ref = Ref(res)
    n = len(BYTE_LENS)
    rows = np.random.default_rng(10).integers(0, n, 200)
    for op, ln in (("==", 7), ("!=", 7), ("<", 40), ("<=", 4096), (">", 4096), (">=", 70000), ("==", 0), (">", 0)):
        where = [Term("blob", "uint8", op, ln, "bytes_len")]
        want = check_api(dec, ref, where)
        assert want.tolist() == [g for g, v in enumerate(BYTE_LENS) if S._PY_OPS[op](v, ln)]
        run(dec, where, *ref.expect(where, rows), rows)
    check_api(dec, ref, [Term("blob", "uint8", "<", 70001, "bytes_len")], kind="all")
    check_api(dec, ref, [Term("blob", "uint8", "<", 0, "bytes_len")], kind="none")


# ------------------------------------------------------------------------------------ 7. failed records
def test_failed_records_have_a_status_and_no_values(dec):
    payloads = synth.c1_payloads(300)
    bad = [5, 64, 65, 299]
    for g in bad:
        payloads[g] = b"\xff" * 10
    res = dec.decode(*synth.framed(payloads))
    assert np.flatnonzero(res.status).tolist() == bad
    ref = Ref(res)
    assert check_api(dec, ref, [Status("!=", 0)]).tolist() == bad
    good = [g for g in range(300) if g not in bad]
    assert check_api(dec, ref, [Status("==", 0)]).tolist() == good
    assert check_api(dec, ref, [Term("label", "int64", ">=", 0)]).tolist() == good
    assert check_api(dec, ref, [Term("label", "int64", "!=", 7)]).tolist() == [g for g in good if g != 7]
    assert check_api(dec, ref, [Term("id", "uint8", "==", 0, "bytes_len")]).tolist() == bad
    assert check_api(dec, ref, [[Status(">", 0), Status("<", 0)], Term("label", "int64", "==", 0, "count")]).tolist() == bad
    st = int(res.status[5])
    assert check_api(dec, ref, [Status("==", st)]).tolist() == [g for g in bad if int(res.status[g]) == st]


# ------------------------------------------------------------------------------------ 8. across contexts
@pytest.fixture(scope="module")
def sharded():
    """Three C1 files decoded by a ShardDecoder in at least 3 batches on 2 streams: (decoder, plan,
    the one-batch truth's result)."""
    import torch

    d = new_decoder()
    imgs = [synth.c4_file(f, "c1", base=2500) for f in range(3)]
    sb = shard.ShardBatch([synth.c4_file_name(f) for f in range(3)], imgs)
    truth = d.decode(sb.buf, sb.starts, sb.ends)
    d.close()
    sd = shard.ShardDecoder(0, batch_bytes=sb.nbytes // 3 + 4096, n_streams=2)
    plan = sd.plan(sb.starts, sb.ends, sb.nbytes)
    assert len(plan) >= 3
    d_bytes = torch.zeros(((sb.nbytes + 15) // 16) * 16 + 16, dtype=torch.uint8, device=dev())
    d_bytes[: sb.nbytes].copy_(torch.from_numpy(sb.buf))
    rst, ren, firsts = sd.rebase32(plan, sb.starts, sb.ends)
    assert rst is None
    d_en = torch.from_numpy(ren.view(np.int32)).to(dev())
    sd.learn(plan, sb.buf, sb.starts, sb.ends)
    streams = [torch.cuda.Stream(dev()), torch.cuda.Stream(dev())]
    torch.cuda.synchronize(dev())
    sd.decode_device32(plan, d_bytes.data_ptr(), None, d_en.data_ptr(), firsts, streams=[s.cuda_stream for s in streams])
    yield sd, plan, truth, (d_bytes, d_en, streams)
    sd.close()


def test_select_appends_across_the_contexts_of_a_plan(sharded):
    import torch

    sd, plan, truth, _ = sharded
    n = len(truth)
    assert int(plan[-1, 1]) == n
    ref = Ref(truth)
    labels = D.densify([D.Dense("label", "int64")], n=n, slot_key=truth.slot_key, slot_kind=truth.slot_kind,
                       row_splits=truth.row_splits, slot_base=truth.slot_base, i64=truth.i64, f32=truth.f32)["label"][:, 0]
    lo, hi = int(np.percentile(labels, 30)), int(np.percentile(labels, 60))
    where = [Term("label", "int64", ">=", lo), Term("label", "int64", "<", hi)]
    want, wstats = ref.expect(where)
    sel = sd.select(plan, where)
    assert sel.rows.cpu().tolist() == want.tolist() and sel.count == len(want) and sel.stats == wstats
    assert (np.diff(want) > 0).all() and want[0] < plan[1, 0] <= plan[2, 0] <= want[-1]  # ascending, over every batch
    # a device list that crosses the batches, with entries that no batch holds
    rng = np.random.default_rng(8)
    rows = rng.integers(0, n, 3000).tolist()
    for k, v in zip((1, 2, 500, 2999), (-1, n, I64_MAX, I64_MIN)):
        rows[k] = v
    want, wstats = ref.expect(where, rows)
    assert wstats[1] == 4
    got = sd.select(plan, where, rows=to_dev(rows), dtype="int32")
    # (the contexts append in plan order: the list is the concatenation of their own selections)
    parts = [[v for v in want.tolist() if r0 <= v < r1] for r0, r1, _, _ in plan.tolist()]
    assert got.rows.cpu().tolist() == [v for p in parts for v in p] and got.stats == wstats
    assert sorted(got.rows.cpu().tolist()) == sorted(want.tolist())
    # select -> dense with a padded capacity, nothing read back in between
    want, wstats = ref.expect(where)
    cap = len(want) + 37
    sel = sd.select(plan, where, capacity=cap)
    batch = sd.dense(plan, [D.Dense("label", "int64", fill=-7)], rows=sel.rows,
                     out={"label": torch.full((cap, 1), -9, dtype=torch.int64, device=dev())})
    got = batch["label"][:, 0].cpu().numpy()
    assert batch.skipped == cap - sel.count == 37 and not sel.overflowed
    assert np.array_equal(got[: len(want)], labels[want]) and (got[len(want) :] == -9).all()
    assert ((got[: len(want)] >= lo) & (got[: len(want)] < hi)).all()
    # an overflow: the prefix that fits, the whole count
    short = sd.select(plan, where, capacity=len(want) - int(plan[2, 1] - plan[2, 0]) // 2)
    assert short.overflowed and short.count == len(want)
    assert short.rows.cpu().tolist() == want.tolist()[: short.capacity]


# ------------------------------------------------------------------------------------ 9. streams
def test_rows_made_just_before_and_results_used_just_after(c3):
    """The candidates are produced by kernels queued on the consumer stream immediately before the
    call and the selection is consumed by ``ragged(rows=)`` on it immediately after, with no
    synchronisation in between: on a side stream, on the legacy default stream, and with a raw
    ``stream=`` handle. Two identical calls give identical bytes."""
    import torch

    d, ref, ints, flts = c3
    where = [Term(ints[7], "int64", "<", 0, "any")]
    spec = [R.Ragged(ints[7], "int64")]
    full = ref.res.ragged(spec)[ints[7]]

    def expect_values(want):
        v, o = full
        return np.concatenate([v[int(o[g]) : int(o[g + 1])] for g in want.tolist()] or [np.zeros(0, np.int64)])

    cap = 1 << 14
    for stream in (torch.cuda.Stream(dev()), torch.cuda.default_stream(dev())):
        with torch.cuda.stream(stream):
            big = torch.arange(1 << 22, device=dev(), dtype=torch.int64)
            rows = (big.flip(0)[:cap] * 7919) % 96  # (queued on the stream; not finished at the call)
            sel = d.select(where, rows=rows, capacity=cap)
            got = d.ragged(spec, rows=sel.rows, capacity=1 << 20)
            twice = d.select(where, rows=rows, capacity=cap)
            v, o = got[ints[7]]
            picked = torch.where(torch.arange(1 << 20, device=dev()) < o[-1], v, torch.zeros_like(v)).sum()
            total = int(picked)
        want, wstats = ref.expect(where, rows.cpu().numpy())
        assert sel.count == len(want) and sel.stats == wstats
        assert sel.rows.cpu().tolist() == want.tolist() + [-1] * (cap - len(want))
        assert torch.equal(sel.rows, twice.rows) and twice.count == sel.count and twice.stats == sel.stats
        vals = expect_values(want)
        assert total == int(vals.sum()) and got.totals[ints[7]] == len(vals)
        assert got.stats[ints[7]][3] == cap - len(want)  # (the -1 tail: skipped rows)
    # stream=: a raw handle as the consumer stream, the rows made on it; the current stream is another
    s = torch.cuda.Stream(dev())
    with torch.cuda.stream(s):
        rows = (torch.arange(1 << 20, device=dev(), dtype=torch.int64).flip(0)[:5000] * 31) % 96
    sel = d.select(where, rows=rows, stream=s.cuda_stream)  # (capacity=None: the count is read back)
    want, wstats = ref.expect(where, rows.cpu().numpy())
    assert sel.rows.cpu().tolist() == want.tolist() and sel.stats == wstats
    got = d.ragged(spec, rows=sel.rows, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(got[ints[7]][0].cpu().numpy(), expect_values(want))


# ------------------------------------------------------------------------------------ 10. C level
def test_c_level_argument_errors_and_empty_cases(dec):
    import torch

    lib = N.lib()
    out = torch.full((64,), -1, dtype=torch.int64, device=dev())
    cnt = torch.full((2,), -1, dtype=torch.int64, device=dev())
    st = torch.full((2,), 77, dtype=torch.int32, device=dev())
    d_rows = to_dev([0, 1, 2])

    def call(k=1, rows_ptr=d_rows.data_ptr(), rdt=N.ROWS_I64, m=3, row0=0, out_ptr=out.data_ptr(), odt=N.ROWS_I64, cap=64,
             cnt_ptr=cnt.data_ptr(), flags=0, **kw):
        f = dict(slot=0, subject=N.SEL_VALUE, op=N.SEL_GE, group=0, index=0, reserved=0, operand=0)
        f.update(kw)
        arr = (N.TfrgSelectTerm * max(k, 1))(*[N.TfrgSelectTerm(**f) for _ in range(max(k, 1))])
        return lib.tfrg_result_select_rows(dec._ctx, arr, k, C.c_void_p(rows_ptr) if rows_ptr else None, rdt, m, row0,
                                           C.c_void_p(out_ptr) if out_ptr else None, odt, cap,
                                           C.c_void_p(cnt_ptr) if cnt_ptr else None, C.c_void_p(st.data_ptr()), flags, None)

    assert call() == -1 and b"no result" in lib.tfrg_last_error()
    assert lib.tfrg_last_error().startswith(b"tfrg_result_select_rows: ")
    fr = synth.framed(synth.c1_payloads(10))
    res = dec.decode(*fr)
    s_label, s_id = res.slot_key.index("label"), res.slot_key.index("id")
    for bad in (dict(k=33), dict(slot=len(res.slot_key)), dict(slot=s_id, subject=N.SEL_VALUE),
                dict(slot=s_id, subject=N.SEL_ANY), dict(slot=s_label, subject=N.SEL_BYTES_LEN),
                dict(slot=max(s_label, s_id), subject=N.SEL_STATUS) if max(s_label, s_id) else dict(subject=9),
                dict(slot=s_label, subject=5), dict(slot=s_label, op=6), dict(slot=s_label, group=32),
                dict(slot=s_label, subject=N.SEL_ANY, index=1), dict(slot=s_label, subject=N.SEL_COUNT, index=1),
                dict(slot=s_label, reserved=1), dict(slot=s_label, rdt=2), dict(slot=s_label, odt=2),
                dict(slot=s_label, m=1 << 31), dict(slot=s_label, m=(1 << 32) - 1), dict(slot=s_label, cnt_ptr=None),
                dict(slot=s_label, cnt_ptr=cnt.data_ptr() + 4), dict(slot=s_label, out_ptr=out.data_ptr() + 4),
                dict(slot=s_label, out_ptr=out.data_ptr() + 2, odt=N.ROWS_I32),
                dict(slot=s_label, odt=N.ROWS_I32, row0=(1 << 31) - 9), dict(slot=s_label, odt=N.ROWS_I32, row0=-(1 << 31) - 1),
                dict(slot=s_label, flags=2), dict(slot=s_label, flags=1 << 31)):
        assert call(**bad) == -1, bad
        assert lib.tfrg_last_error().startswith(b"tfrg_result_select_rows: "), bad
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [-1] * 64 and cnt.cpu().tolist() == [-1, -1] and st.cpu().tolist() == [77, 77]
    # what is allowed: rows NULL with any rows_dtype and m above n, cap == 0 with an output, an int32
    # output at the edges of its range, out NULL, an output that is only 4-byte aligned for int32
    assert call(slot=s_label, rows_ptr=None, rdt=9, m=14) == 0
    torch.cuda.synchronize()
    assert out.cpu().tolist()[:11] == [*range(10), -1] and cnt.cpu().tolist() == [10, -1] and st.cpu().tolist() == [10, 4]
    assert call(slot=s_label, cap=0) == 0 and call(slot=s_label, out_ptr=None) == 0
    assert call(slot=s_label, odt=N.ROWS_I32, row0=(1 << 31) - 10, out_ptr=out.data_ptr() + 36) == 0
    assert call(slot=s_label, odt=N.ROWS_I32, row0=-(1 << 31)) == 0
    # a float operand with high bits set, on a float slot
    fres = dec.decode(*synth.framed(mixed(24)))
    s_empty = fres.slot_key.index("empty")
    assert fres.slot_kind[s_empty] == 2
    assert call(slot=s_empty, operand=1 << 32) == -1 and lib.tfrg_last_error().startswith(b"tfrg_result_select_rows: ")
    assert call(slot=s_empty, subject=N.SEL_ANY, operand=(1 << 63) | 5) == -1
    assert call(slot=s_empty, subject=N.SEL_COUNT, operand=(1 << 63) | 5) == 0  # (a count's operand is an int64)
    assert call(slot=s_empty, operand=0x3FC00000) == 0
    # m == 0: no kernel; the count is 0, or with APPEND what it was
    res = dec.decode(*fr)
    out.fill_(-1)
    cnt.fill_(41)
    assert call(slot=s_label, m=0, rows_ptr=None) == 0
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [0, 41] and st.cpu().tolist() == [0, 0] and out.cpu().tolist() == [-1] * 64
    cnt.fill_(41)
    assert call(slot=s_label, m=0, rows_ptr=None, flags=N.SEL_APPEND) == 0
    assert call(k=0, m=0, flags=N.SEL_APPEND) == 0
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [41, 41] and st.cpu().tolist() == [0, 0]
    # n_terms == 0 selects every candidate that is not skipped; APPEND starts at the count
    cnt.fill_(5)
    assert call(k=0, flags=N.SEL_APPEND) == 0
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [8, 5] and out.cpu().tolist()[:9] == [-1] * 5 + [0, 1, 2, -1] and st.cpu().tolist() == [3, 0]
    # n == 0: every candidate is skipped
    assert len(dec.decode(fr[0][:0], fr[1][:0], fr[2][:0])) == 0
    out.fill_(-1)
    cnt.fill_(41)
    assert call(slot=s_label) == 0
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [0, 41] and st.cpu().tolist() == [0, 3] and out.cpu().tolist() == [-1] * 64
    cnt.fill_(41)
    assert call(slot=s_label, flags=N.SEL_APPEND) == 0
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [41, 41] and st.cpu().tolist() == [0, 3]
    sel = dec.select([Term("label", "int64", ">=", 0)], rows=to_dev([0, 5]))
    assert sel.rows.numel() == 0 and sel.count == 0 and sel.stats == (0, 2)


# ------------------------------------------------------------------------------------ 11. minibatches
def test_minibatches_over_the_selected_records(dec):
    n = 1500
    dec.decode(*synth.framed(synth.c1_payloads(n)))
    where = [Term("label", "int64", ">=", 300), Term("label", "int64", "<", 1100)]
    chosen = [i for i in range(n) if 300 <= i % 1000 < 1100]
    assert 0 < len(chosen) < n
    specs = [D.Dense("id", "uint8", 12), D.Dense("label", "int64")]

    def drawn(batches) -> list[int]:
        out = []
        for b in batches:
            ids = [int(bytes(x)[4:]) for x in b["id"].cpu().numpy()]
            assert b["label"][:, 0].cpu().tolist() == [i % 1000 for i in ids] and b.skipped == 0
            out += ids
        return out

    a = drawn(dec.minibatches(specs, 256, seed=3, where=where))
    assert sorted(a) == chosen and a != chosen
    assert drawn(dec.minibatches(specs, 256, seed=3, where=where)) == a
    assert drawn(dec.minibatches(specs, 256, seed=4, where=where)) != a
    assert drawn(dec.minibatches(specs, 256, seed=3, where=where, drop_last=True)) == a[: len(chosen) // 256 * 256]
    # where=None is what it was: a permutation of every record by the same generator
    import torch

    gen = torch.Generator(device=dev())
    gen.manual_seed(3)
    perm = torch.randperm(n, generator=gen, device=dev()).cpu().tolist()
    assert drawn(dec.minibatches(specs, 256, seed=3)) == perm == drawn(dec.minibatches(specs, 256, seed=3, where=None))
    # ragged
    rspecs = [R.Ragged("id", "uint8"), R.Ragged("label", "int64")]

    def rdrawn(batches) -> list[int]:
        out = []
        for b in batches:
            v, o = (t.cpu().numpy() for t in b["id"])
            out += [int(bytes(v[12 * k + 4 : 12 * k + 12])) for k in range(len(o) - 1)]
            assert b.stats["id"].tolist() == [0, 0, 0, 0]
        return out

    r = rdrawn(dec.ragged_minibatches(rspecs, 256, seed=3, where=where))
    assert r == a  # (the same select and the same generator)
    assert rdrawn(dec.ragged_minibatches(rspecs, 256, seed=3)) == perm
    assert list(dec.minibatches(specs, 256, where=[Status("!=", 0)])) == []
