"""Ragged device outputs (tfrg_result_ragged_rows: k_rg_len / k_rg_scan / k_rg_gather):
``HipDecoder.ragged`` must equal the numpy reference -- ``BatchResult.ragged`` over the same decode's
fetched columns (tests/test_ragged_host.py checks that one against the oracle, row list by row list)
-- bit for bit (floats as uint32): values, all m + 1 offsets, totals and counters. Every output is
prefilled with 0xA5 inside a larger buffer: what lies before ``values``, after the stored prefix and
after ``cap`` keeps the poison."""

import ctypes as C

import numpy as np
import pytest

from tests.test_dense_rows_host import mixed
from tfr_reader import _native as N
from tfr_reader import dense as D
from tfr_reader import hip, synth, writer
from tfr_reader import ragged as R

pytestmark = pytest.mark.gpu

COLS = ("status", "aux", "verdict", "order", "row_splits", "i64", "f32", "bytes_off", "bytes_len", "slot_base")
POISON = 0xA5
GUARD = 256
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
ISZ = {"int64": 8, "int32": 4, "float32": 4, "uint8": 1}


def dev():
    import torch

    return torch.device("cuda", 0)


def to_dev(rows, dtype=np.int64):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(rows, dtype))).to(dev())


def new_decoder(env: dict | None = None):
    mp = pytest.MonkeyPatch()
    mp.setenv("TFRG_OPTIMISTIC", "1")  # (read at context creation; the suite may run with 0)
    mp.setenv("TFRG_TEMPLATES", "1")
    for k, v in (env or {}).items():
        mp.setenv(k, v)
    try:
        return hip.HipDecoder(0)
    finally:
        mp.undo()


@pytest.fixture
def dec():
    d = new_decoder()
    yield d
    d.close()


def ubits(a: np.ndarray) -> np.ndarray:
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


class Ref:
    """The host reference of one decode, computed once over every record (``BatchResult.ragged``)
    and indexed per row list: a row out of range is an empty row that counts in ``skipped`` alone."""

    def __init__(self, res, specs) -> None:
        self.res, self.specs, self.n = res, list(specs), len(res)
        full = res.ragged(self.specs)
        whole = res.ragged([R.Ragged(s.key, s.dtype, None, s.out_name) for s in self.specs])  # (before max_len)
        self.values = {k: ubits(v) for k, (v, _) in full.items()}
        self.offsets = {k: o for k, (_, o) in full.items()}
        self.flags = {}
        for s in self.specs:
            k = s.out_name
            slot = D.find_slot(res.slot_key, res.slot_kind, s.key, D.DTYPES[s.dtype][1])
            cnt = np.zeros(self.n, np.int64) if slot is None else np.diff(np.asarray(res.row_splits[slot]).astype(np.int64))
            trunc = np.diff(whole[k][1]) > np.diff(self.offsets[k])
            self.flags[k] = (trunc, cnt == 0, (cnt > 1) if s.dtype == "uint8" else np.zeros(self.n, bool))
        assert all(full.stats[k].tolist() == [int(f.sum()) for f in self.flags[k]] + [0] for k in full)

    def expect(self, rows, row0: int = 0) -> dict:
        """name -> (values as unsigned bits, offsets, the four counters) for a row list (None: every
        record), entries being Python ints or an array."""
        if rows is None:
            rows = np.arange(self.n)
        rows = [int(v) for v in np.asarray(rows, object).reshape(-1)]
        ok = np.array([row0 <= v < row0 + self.n for v in rows], bool)
        idx = np.array([v - row0 if o else 0 for v, o in zip(rows, ok.tolist())], np.int64)
        out = {}
        for s in self.specs:
            k = s.out_name
            off = self.offsets[k]
            lens = np.diff(off)[idx] * ok if len(rows) else np.zeros(0, np.int64)
            offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            src = np.repeat(off[:-1][idx] - offsets[:-1], lens) + np.arange(int(offsets[-1]))
            stats = [int(f[idx][ok].sum()) for f in self.flags[k]] + [int((~ok).sum())]
            out[k] = (self.values[k][src], offsets, stats)
        return out


class Outs:
    """Poisoned outputs for ``specs`` and m rows: per spec one byte buffer that holds GUARD bytes,
    ``shift`` more bytes, ``cap`` elements of values and GUARD bytes again."""

    def __init__(self, specs, m: int, caps: dict, shift: int = 0) -> None:
        import torch

        tdt = {"int64": torch.int64, "int32": torch.int32, "float32": torch.float32, "uint8": torch.uint8}
        self.specs, self.m, self.caps, self.bufs, self.out, self.lo = list(specs), m, caps, {}, {}, {}
        for s in self.specs:
            k, isz = s.out_name, ISZ[s.dtype]
            lo = GUARD + shift
            assert lo % isz == 0
            big = torch.full((lo + caps[k] * isz + GUARD,), POISON, dtype=torch.uint8, device=dev())
            off = torch.full(((m + 1) * 8 + 16,), POISON, dtype=torch.uint8, device=dev())
            self.bufs[k], self.lo[k] = (big, off), lo
            self.out[k] = (big[lo : lo + caps[k] * isz].view(tdt[s.dtype]), off[: (m + 1) * 8].view(torch.int64))

    def check(self, got, want: dict, stats: bool = True) -> None:
        for s in self.specs:
            k, isz = s.out_name, ISZ[s.dtype]
            values, offsets, st = want[k]
            total, cap = int(offsets[-1]), self.caps[k]
            big, off = (t.cpu().numpy() for t in self.bufs[k])
            assert np.array_equal(off[: (self.m + 1) * 8].view(np.int64), offsets), k
            assert (off[(self.m + 1) * 8 :] == POISON).all(), k
            kept = min(total, cap)
            lo = self.lo[k]
            assert np.array_equal(big[lo : lo + kept * isz], values[:kept].view(np.uint8)), k
            assert (big[:lo] == POISON).all() and (big[lo + kept * isz :] == POISON).all(), k
            if got is not None:
                assert got.totals[k] == total and got.overflowed[k] == (total > cap), k
                if stats:
                    assert got.stats[k].tolist() == st, k


def run(dec, ref: Ref, rows, dtype=np.int64, slack: int = 3, shift: int = 0, caps: dict | None = None):
    """``dec.ragged(rows=, out=)`` over poisoned outputs (capacity: the total + slack, or ``caps``),
    checked against the reference. ``rows``: None, or entries for a device list of ``dtype``."""
    want = ref.expect(rows)
    caps = caps or {k: int(w[1][-1]) + slack for k, w in want.items()}
    m = ref.n if rows is None else len(rows)
    outs = Outs(ref.specs, m, caps, shift)
    got = dec.ragged(ref.specs, rows=None if rows is None else to_dev(rows, dtype), out=outs.out)
    outs.check(got, want)
    return got


def run_c(dec, ref: Ref, rows, rdt, row0: int):
    """The same through the C entry point, with a row0 and raw counters."""
    import torch

    want = ref.expect(rows, row0)
    m = len(rows)
    caps = {k: int(w[1][-1]) + 1 for k, w in want.items()}
    outs = Outs(ref.specs, m, caps)
    k = len(ref.specs)
    totals = torch.full((k,), -1, dtype=torch.int64, device=dev())
    stats = torch.full((k, 4), 77, dtype=torch.int32, device=dev())
    items = [(D.resolve_slot(dec, s), D.DTYPES[s.dtype][0], s.limit, caps[s.out_name], outs.out[s.out_name][0].data_ptr(),
              outs.out[s.out_name][1].data_ptr()) for s in ref.specs]
    d_rows = to_dev(rows, np.int64 if rdt == N.ROWS_I64 else np.int32)
    R.launch(dec, items, (d_rows.data_ptr(), rdt), m, row0, totals.data_ptr(), stats.data_ptr(), None)
    torch.cuda.synchronize()
    outs.check(None, want)
    assert totals.cpu().tolist() == [int(want[s.out_name][1][-1]) for s in ref.specs]
    assert stats.cpu().numpy().view(np.uint32).tolist() == [want[s.out_name][2] for s in ref.specs]


# ------------------------------------------------------------------------------------ 1. optimistic C1
N1 = 5000
C1_SPECS = [R.Ragged("label", "int64"), R.Ragged("label", "int32", name="l32"), R.Ragged("id", "uint8"),
            R.Ragged("id", "uint8", 5, name="id5")]
BAD64 = [-1, N1, N1 + 1, (1 << 31) - 1, I64_MIN, I64_MAX, -N1, 1 << 32, (1 << 32) + 5, -(1 << 32)]
BAD32 = [-1, N1, N1 + 1, (1 << 31) - 1, -(1 << 31), -N1]


def with_bad(bad: list[int], m: int) -> list[int]:
    good = np.random.default_rng(m).integers(0, N1, m).tolist()
    return [bad[(k // 3) % len(bad)] if k % 3 == 1 else good[k] for k in range(m)]


def c1_row_lists() -> list:
    rng = np.random.default_rng(1)
    return [(None, np.int64), (rng.permutation(N1), np.int64), (rng.permutation(N1)[:1237], np.int32),
            (rng.integers(0, N1, 2 * N1 + 3), np.int64), (rng.integers(0, N1, 777), np.int32), (np.full(70, N1 - 1), np.int64),
            (with_bad(BAD64, 1027), np.int64), (with_bad(BAD32, 1027), np.int32), (BAD64, np.int64), (BAD32, np.int32)]


def check_c1(d, res, fr) -> None:
    ref = Ref(res, C1_SPECS)
    for rows, dtype in c1_row_lists():
        got = run(d, ref, rows, dtype)
        if rows is not None and len(rows) == 70:
            assert got["label"][0][:70].cpu().tolist() == [(N1 - 1) % 1000] * 70  # the generator's truth
            assert bytes(got["id"][0][:12].cpu().numpy()) == b"img-%08d" % (N1 - 1)
    row0 = 1 << 40
    rows = [row0 + (7 * k) % N1 for k in range(300)]
    rows[3], rows[10], rows[11], rows[40] = row0 - 1, row0 + N1, 5, I64_MIN  # (5: in range only without row0)
    run_c(d, ref, rows, N.ROWS_I64, row0)
    run_c(d, ref, [100 + (11 * k) % (N1 + 50) for k in range(300)], N.ROWS_I32, 100)
    run_c(d, ref, [-3 + k for k in range(40)], N.ROWS_I32, -3)
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
MIXED_SPECS = [R.Ragged("half", "int64"), R.Ragged("half", "int32", 1, name="half32"), R.Ragged("empty", "float32"),
               R.Ragged("two", "int64", name="two_i"), R.Ragged("two", "float32", name="two_f"),
               R.Ragged("names", "uint8"), R.Ragged("names", "uint8", 3, name="names3"), R.Ragged("absent", "int64")]


def test_absent_keys_empty_lists_two_kinds_and_several_elements(dec):
    n = 600
    res = dec.decode(*synth.framed(mixed(n)))
    ref = Ref(res, MIXED_SPECS)
    rng = np.random.default_rng(n)
    for rows in (None, rng.permutation(n), rng.integers(0, n, 2 * n + 5), np.full(70, n - 1)):
        got = run(dec, ref, rows)
        m = n if rows is None else len(rows)
        assert got.stats["absent"].tolist() == [0, m, 0, 0] and got.totals["absent"] == 0
        assert got.stats["names"][2] > 0 or m == 70
    # a device list with entries out of range: the absent key's rows are skipped like the others'
    rows = [0, n, -1, 5, I64_MAX]
    got = run(dec, ref, rows)
    assert got.stats["absent"].tolist() == [0, 2, 0, 3] and got.stats["names"][3] == 3
    # without out=: exact allocations behind one read-back of the totals
    got = dec.ragged(MIXED_SPECS, rows=to_dev(rows))
    want = ref.expect(rows)
    for k, (v, o) in got.items():
        assert np.array_equal(ubits(v.cpu().numpy()), want[k][0]) and np.array_equal(o.cpu().numpy(), want[k][1]), k
        assert got.stats[k].tolist() == want[k][2] and not got.overflowed[k], k


# ------------------------------------------------------------------------------------ 4. tile edges
@pytest.fixture(scope="module")
def c3():
    d = new_decoder()
    res = d.decode(*synth.framed(synth.c3_payloads(96)))
    ints = [k for k, kd in zip(res.slot_key, res.slot_kind) if kd == 3]
    flts = [k for k, kd in zip(res.slot_key, res.slot_kind) if kd == 2]
    assert len(ints) == 32 and len(flts) == 32
    yield d, res, ints, flts
    d.close()


def test_c3_every_slot_in_one_call_with_small_tiles(c3):
    d, res, ints, flts = c3
    specs = [R.Ragged(k, "int64" if i % 2 else "int32", None if i % 3 else 17) for i, k in enumerate(ints)]
    specs += [R.Ragged(k, "float32", None if i % 3 else 5) for i, k in enumerate(flts)]
    assert len(specs) == N.RAGGED_MAX_SPECS
    ref = Ref(res, specs)
    d.set_ragged_tile(64)
    try:
        rng = np.random.default_rng(4)
        run(d, ref, None)
        for m in (0, 1, 63, 64, 65, 127, 128, 129, 4097):
            run(d, ref, rng.integers(0, 96, m), np.int32 if m % 2 else np.int64)
    finally:
        d.set_ragged_tile(0)


def test_tile_scan_carries_into_its_second_pass(c3):
    d, res, ints, flts = c3
    specs = [R.Ragged(ints[0], "int64"), R.Ragged(ints[1], "int32", 9), R.Ragged(flts[0], "float32")]
    ref = Ref(res, specs)
    d.set_ragged_tile(N.RAGGED_TILE_MIN)
    try:
        edge = N.RAGGED_SCAN_THREADS * N.RAGGED_TILE_MIN  # that many rows fill the scan's first pass
        rng = np.random.default_rng(5)
        for m in (edge - 1, edge, edge + 1):
            run(d, ref, rng.integers(0, 96, m), np.int32)
    finally:
        d.set_ragged_tile(0)
    for bad in (1, 32, 96, 8192):
        with pytest.raises(N.NativeError):
            d.set_ragged_tile(bad)


def test_default_tile_with_many_rows(c3):
    d, res, ints, flts = c3
    specs = [R.Ragged(ints[2], "int64"), R.Ragged(flts[3], "float32", 16)]
    rows = np.random.default_rng(6).integers(0, 96, 70001)
    rows[::1000] = -1
    run(d, Ref(res, specs), rows)


# ------------------------------------------------------------------------------------ 5. length edges
LIST_LENS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 20000]
BYTE_LENS = [*range(41), *range(4095, 4101), 70000]
MAX_LENS = [None, 1, 3, 16, 4096]


def list_payloads() -> list[bytes]:
    rng = np.random.default_rng(7)
    out = []
    for ln in LIST_LENS:
        ints = rng.integers(-(1 << 40), 1 << 40, ln).tolist()
        out.append(writer.encode_example([("tok", "int64_list", ints),
                                          ("w", "float_list", rng.standard_normal(ln).astype(np.float32))]))
    return out


def shifts(dtype: str) -> list[int]:
    """Byte offsets of ``values`` from a 16-byte boundary: none, one element, and 1, 2, 3 bytes for uint8."""
    return [0, ISZ[dtype]] + ([2, 3] if dtype == "uint8" else [])


@pytest.mark.parametrize("max_len", MAX_LENS)
def test_list_lengths(dec, max_len):
    res = dec.decode(*synth.framed(list_payloads()))
    n = len(LIST_LENS)
    rng = np.random.default_rng(8)
    for dtype, key in (("int64", "tok"), ("int32", "tok"), ("float32", "w")):
        ref = Ref(res, [R.Ragged(key, dtype, max_len)])
        for shift in shifts(dtype):
            run(dec, ref, None, shift=shift)
            run(dec, ref, rng.integers(0, n, 40), shift=shift)


def bytes_payloads() -> list[bytes]:
    rng = np.random.default_rng(9)
    return [writer.encode_example([("blob", "bytes_list", [rng.integers(0, 256, ln, dtype=np.uint8).tobytes()])])
            for ln in BYTE_LENS]


@pytest.mark.parametrize("materialize", [False, True])
@pytest.mark.parametrize("max_len", MAX_LENS)
def test_bytes_lengths(dec, max_len, materialize):
    res = dec.decode(*synth.framed(bytes_payloads()), materialize_bytes=materialize)
    assert (res.bytes_data is not None) == materialize
    n = len(BYTE_LENS)
    ref = Ref(res, [R.Ragged("blob", "uint8", max_len)])
    rng = np.random.default_rng(10)
    for shift in shifts("uint8"):
        run(dec, ref, None, shift=shift)
        run(dec, ref, rng.integers(0, n, 60), shift=shift)


# ------------------------------------------------------------------------------------ 6. capacity
def test_capacity_and_the_offsets_only_call(c3):
    import torch

    d, res, ints, flts = c3
    specs = [R.Ragged(ints[4], "int64"), R.Ragged(ints[5], "int32"), R.Ragged(flts[6], "float32", 7)]
    ref = Ref(res, specs)
    rows = np.random.default_rng(11).integers(0, 96, 300)
    want = ref.expect(rows)
    totals = {k: int(w[1][-1]) for k, w in want.items()}
    assert all(t > 1 for t in totals.values())
    for delta in (0, -1, 1, None):
        caps = {k: (t + delta if delta is not None else 0) for k, t in totals.items()}
        got = run(d, ref, rows, caps=caps)
        assert all(got.overflowed[k] == (delta in (-1, None)) for k in totals)
    # capacity= allocates here, and makes one call without a read-back
    got = d.ragged(specs, rows=to_dev(rows), capacity={k: t - 1 for k, t in totals.items()})
    for k, (v, o) in got.items():
        assert v.numel() == totals[k] - 1 and got.overflowed[k] and got.totals[k] == totals[k]
        assert np.array_equal(ubits(v.cpu().numpy()), want[k][0][:-1]) and np.array_equal(o.cpu().numpy(), want[k][1])
    got = d.ragged(specs, rows=to_dev(rows), capacity=max(totals.values()))
    assert not any(got.overflowed.values())
    # the offsets-only call: values NULL, whatever cap says
    m = len(rows)
    outs = Outs(specs, m, dict.fromkeys(totals, 0))
    tot = torch.full((3,), -1, dtype=torch.int64, device=dev())
    st = torch.full((3, 4), 77, dtype=torch.int32, device=dev())
    items = [(D.resolve_slot(d, s), D.DTYPES[s.dtype][0], s.limit, 1 << 40, None, outs.out[s.out_name][1].data_ptr())
             for s in specs]
    d_rows = to_dev(rows)
    R.launch(d, items, (d_rows.data_ptr(), N.ROWS_I64), m, 0, tot.data_ptr(), st.data_ptr(), None)
    torch.cuda.synchronize()
    outs.check(None, want)
    assert tot.cpu().tolist() == [totals[s.out_name] for s in specs]
    assert st.cpu().numpy().view(np.uint32).tolist() == [want[s.out_name][2] for s in specs]


def test_c_level_argument_errors_and_empty_cases(dec):
    import torch

    lib = N.lib()
    offs = torch.full((8,), -1, dtype=torch.int64, device=dev())
    vals = torch.full((64,), -1, dtype=torch.int64, device=dev())
    tot = torch.full((2,), -1, dtype=torch.int64, device=dev())
    st = torch.full((2, 4), 77, dtype=torch.int32, device=dev())
    d_rows = to_dev([0, 1, 2])

    def call(k=1, rows_ptr=d_rows.data_ptr(), rdt=N.ROWS_I64, m=3, **kw):
        f = dict(slot=0, dtype=N.DENSE_I64, max_len=0, reserved=0, cap=64, values=vals.data_ptr(), offsets=offs.data_ptr())
        f.update(kw)
        arr = (N.TfrgRaggedSpec * max(k, 1))(*[N.TfrgRaggedSpec(**f) for _ in range(max(k, 1))])
        return lib.tfrg_result_ragged_rows(dec._ctx, arr, k, C.c_void_p(rows_ptr) if rows_ptr else None, rdt, m, 0,
                                           C.c_void_p(tot.data_ptr()), C.c_void_p(st.data_ptr()), None)

    assert call() == -1 and b"no result" in lib.tfrg_last_error()
    assert lib.tfrg_last_error().startswith(b"tfrg_result_ragged_rows")
    fr = synth.framed(synth.c1_payloads(10))
    res = dec.decode(*fr)
    s_label, s_id = res.slot_key.index("label"), res.slot_key.index("id")
    for bad in (dict(k=0), dict(k=65), dict(slot=len(res.slot_key)), dict(slot=s_label, dtype=N.DENSE_F32),
                dict(slot=s_label, dtype=N.DENSE_U8), dict(slot=s_id, dtype=N.DENSE_I32), dict(slot=s_label, dtype=4),
                dict(slot=s_label, offsets=None), dict(slot=s_label, reserved=1), dict(slot=s_label, rdt=2),
                dict(slot=s_label, m=1 << 31), dict(slot=s_label, m=(1 << 32) - 1)):
        assert call(**bad) == -1, bad
        assert lib.tfrg_last_error().startswith(b"tfrg_result_ragged_rows"), bad
    # rows NULL: every record in order, rows_dtype ignored; m may differ from n
    assert call(slot=s_label, rows_ptr=None, rdt=9, m=7) == 0
    assert call(k=2, slot=s_label, m=0, rows_ptr=None) == 0  # (m == 0: offsets[0] = 0, no kernel)
    torch.cuda.synchronize()
    assert offs.cpu().tolist() == [0, 1, 2, 3, 4, 5, 6, 7] and vals.cpu().tolist()[:8] == [0, 1, 2, 3, 4, 5, 6, -1]
    offs.fill_(-1)
    assert call(k=2, slot=s_label, m=0, rows_ptr=None) == 0
    torch.cuda.synchronize()
    assert offs.cpu().tolist() == [0] + [-1] * 7 and tot.cpu().tolist() == [0, 0] and st.cpu().tolist() == [[0] * 4] * 2
    # n == 0: every row is skipped, all offsets are 0
    assert len(dec.decode(fr[0][:0], fr[1][:0], fr[2][:0])) == 0
    offs.fill_(-1)
    assert call(k=2, slot=s_label) == 0
    torch.cuda.synchronize()
    assert offs.cpu().tolist() == [0, 0, 0, 0] + [-1] * 4 and tot.cpu().tolist() == [0, 0]
    assert st.cpu().tolist() == [[0, 0, 0, 3]] * 2
    got = dec.ragged([R.Ragged("label", "int64")], rows=to_dev([0, 5]))
    assert got["label"][1].cpu().tolist() == [0, 0, 0] and got.stats["label"].tolist() == [0, 0, 0, 2]


def test_python_out_is_checked(dec):
    """``out=``: tensors of the right dtype and shape are written into; a wrong dtype, shape or device
    is refused."""
    import torch

    dec.decode(*synth.framed(synth.c1_payloads(6)))
    specs = [R.Ragged("label", "int64")]
    rows = to_dev([0, 6, -1, 5, 2, 2, 3])
    ok = (torch.full((8,), -1, dtype=torch.int64, device=dev()), torch.full((8,), -1, dtype=torch.int64, device=dev()))
    got = dec.ragged(specs, rows=rows, out={"label": ok})
    assert got["label"][0] is ok[0] and got["label"][1] is ok[1] and got.capacity["label"] == 8
    assert ok[1].cpu().tolist() == [0, 1, 1, 1, 2, 3, 4, 5] and ok[0].cpu().tolist() == [0, 5, 2, 2, 3, -1, -1, -1]
    assert got.totals["label"] == 5 and got.stats["label"].tolist() == [0, 0, 0, 2] and not got.overflowed["label"]
    for i, wrong in ((0, ok[0].to(torch.int32)), (0, ok[0].cpu()), (0, ok[0].view(2, 4)), (0, ok[0][::2]),
                     (1, ok[1].to(torch.int32)), (1, ok[1][:-1]), (1, ok[1].cpu())):
        with pytest.raises(ValueError):
            dec.ragged(specs, rows=rows, out={"label": tuple(wrong if j == i else t for j, t in enumerate(ok))})


# ------------------------------------------------------------------------------------ 7. streams
def test_rows_made_just_before_and_results_used_just_after(c3):
    """The row list is produced by kernels queued on the consumer stream immediately before the call
    and the outputs are consumed on it immediately after, with no synchronisation in between: on a
    side stream, and on the legacy default stream."""
    import torch

    d, res, ints, flts = c3
    specs = [R.Ragged(ints[7], "int64"), R.Ragged(flts[8], "float32")]
    ref = Ref(res, specs)
    for stream in (torch.cuda.Stream(dev()), torch.cuda.default_stream(dev())):
        with torch.cuda.stream(stream):
            big = torch.arange(1 << 22, device=dev(), dtype=torch.int64)
            rows = (big.flip(0)[: 1 << 14] * 7919) % 96  # (queued on the stream; not finished at the call)
            got = d.ragged(specs, rows=rows, capacity=1 << 20)
            v, o = got[ints[7]]
            picked = torch.where(torch.arange(1 << 20, device=dev()) < o[-1], v, torch.zeros_like(v)).sum()
            twice = d.ragged(specs, rows=rows, capacity=1 << 20)
            total = int(picked)
        want = ref.expect(rows.cpu().numpy())
        w = want[ints[7]][0]
        assert total == int(w.view(np.int64).sum())
        for k in got:
            kept = int(want[k][1][-1])
            for b in (got, twice):
                assert np.array_equal(ubits(b[k][0].cpu().numpy())[:kept], want[k][0]), k
                assert np.array_equal(b[k][1].cpu().numpy(), want[k][1]), k
            assert got.stats[k].tolist() == twice.stats[k].tolist() == want[k][2]
    # stream=: a raw handle as the consumer stream, the rows made on it; the current stream is another
    s = torch.cuda.Stream(dev())
    with torch.cuda.stream(s):
        rows = (torch.arange(1 << 20, device=dev(), dtype=torch.int64).flip(0)[:5000] * 31) % 96
    before = d.device_bytes()[0]
    got = d.ragged(specs, rows=rows, stream=s.cuda_stream)  # (capacity=None: offsets, totals, gather)
    assert d.device_bytes()[0] >= before  # (the per-tile sums live in the context)
    s.synchronize()
    want = ref.expect(rows.cpu().numpy())
    for k, (v, o) in got.items():
        assert np.array_equal(ubits(v.cpu().numpy()), want[k][0]) and np.array_equal(o.cpu().numpy(), want[k][1]), k


# ------------------------------------------------------------------------------------ 8. minibatches
def test_ragged_minibatches_cover_an_epoch(dec):
    n = 1500
    dec.decode(*synth.framed(synth.c1_payloads(n)))
    specs = [R.Ragged("id", "uint8"), R.Ragged("label", "int64")]

    def drawn(batches) -> list[int]:
        out = []
        for b in batches:
            v, o = (t.cpu().numpy() for t in b["id"])
            assert np.array_equal(np.diff(o), np.full(len(o) - 1, 12)) and not b.overflowed["id"]
            nums = [int(bytes(v[12 * k + 4 : 12 * k + 12])) for k in range(len(o) - 1)]
            assert b["label"][0].cpu().tolist()[: len(nums)] == [i % 1000 for i in nums]
            assert b.stats["id"].tolist() == [0, 0, 0, 0]
            out += nums
        return out

    a = drawn(dec.ragged_minibatches(specs, 512, seed=3))
    assert sorted(a) == list(range(n)) and a != list(range(n))
    assert drawn(dec.ragged_minibatches(specs, 512, seed=3)) == a
    assert drawn(dec.ragged_minibatches(specs, 512, seed=4)) != a
    part = drawn(dec.ragged_minibatches(specs, 512, seed=3, drop_last=True, capacity=512 * 12))
    assert part == a[: 2 * 512]
