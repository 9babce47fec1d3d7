"""Two-level ragged device outputs (tfrg_result_ragged_elems: k_el_len / k_el_scan / k_el_offs /
k_el_copy): ``HipDecoder.ragged_elements`` and the C entry point must give, for a list of rows, every
element of the rows' bytes_lists exactly as the generator made them (tests/_elems_ref.py builds the
expected arrays from the generator's own items, never from the device's columns), with the numpy path
(``BatchResult.ragged_elements``) as a second reference. Every output is prefilled with 0xA5 inside a
larger buffer: what lies before an array, after its stored prefix and after its capacity keeps the
poison."""

import ctypes as C

import numpy as np
import pytest

from tests import _bytes_ref as B
from tests import test_implicit_off_gpu as IO
from tests._elems_ref import expect
from tests.golden.gen_golden import entry, i64
from tests.test_ragged_gpu import BAD32, BAD64, COLS, GUARD, I64_MAX, I64_MIN, POISON, dev, new_decoder, to_dev
from tfr_reader import _native as N
from tfr_reader import ragged as R
from tfr_reader import select as SEL
from tfr_reader import synth

pytestmark = pytest.mark.gpu

TILE = 64
LENGTHS = [0, 1, 3, 4, 15, 16, 17, 31, 33, 40]
EL = R.RaggedElements


# ------------------------------------------------------------------------------------ poisoned outputs
class Outs:
    """Poisoned outputs of one spec over m rows: ``values`` [cap] at ``shift`` bytes past a 16-byte
    boundary, ``elem_offsets`` [elem_cap + 1] and ``row_offsets`` [m + 1], each between GUARD bytes of
    poison. ``elem_cap`` None: no elem_offsets and no values; ``cap`` None: no values."""

    def __init__(self, m: int, elem_cap: int | None, cap: int | None, shift: int = 0) -> None:
        import torch

        def poisoned(nbytes: int):
            return torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device=dev())

        self.m, self.elem_cap, self.cap, self.shift = m, elem_cap, cap, shift
        self.ro_buf = poisoned((m + 1) * 8)
        self.ro = self.ro_buf[GUARD : GUARD + (m + 1) * 8].view(torch.int64)
        self.eo_buf = self.eo = self.v_buf = self.v = None
        if elem_cap is not None:
            self.eo_buf = poisoned((elem_cap + 1) * 8)
            self.eo = self.eo_buf[GUARD : GUARD + (elem_cap + 1) * 8].view(torch.int64)
            if cap is not None:
                self.v_buf = poisoned(shift + cap)
                assert self.v_buf.data_ptr() % 16 == 0
                self.v = self.v_buf[GUARD + shift : GUARD + shift + cap]

    @property
    def out(self) -> tuple:
        return self.v, self.eo, self.ro

    def item(self, slot: int, sp) -> tuple:
        """The spec as ``ragged.launch_elems`` takes it."""
        return (slot, sp.elems_limit, sp.limit, self.elem_cap or 0, self.cap or 0,
                self.v.data_ptr() if self.v is not None and self.cap else None,
                self.eo.data_ptr() if self.eo is not None else None, self.ro.data_ptr())

    def untouched(self) -> None:
        for b in (self.ro_buf, self.eo_buf, self.v_buf):
            assert b is None or bool((b == POISON).all())

    def check(self, want) -> None:
        ro = self.ro_buf.cpu().numpy()
        assert np.array_equal(ro[GUARD:-GUARD].view(np.int64), want.row_offsets)
        assert (ro[:GUARD] == POISON).all() and (ro[-GUARD:] == POISON).all()
        if self.eo_buf is None:
            return
        E, _ = want.totals
        e1 = min(E, self.elem_cap)
        eo = self.eo_buf.cpu().numpy()
        assert np.array_equal(eo[GUARD : GUARD + (e1 + 1) * 8].view(np.int64), want.elem_offsets[: e1 + 1])
        assert (eo[:GUARD] == POISON).all() and (eo[GUARD + (e1 + 1) * 8 :] == POISON).all()
        if self.v_buf is None:
            return
        kept = min(int(want.elem_offsets[e1]), self.cap)
        v = self.v_buf.cpu().numpy()
        lo = GUARD + self.shift
        assert np.array_equal(v[lo : lo + kept], want.values[:kept])
        assert (v[:lo] == POISON).all() and (v[lo + kept :] == POISON).all()


def run(dec, items, specs, rows, dtype=np.int64, slack: int = 3, shift: int = 0, caps: dict | None = None):
    """``dec.ragged_elements(rows=, out=)`` over poisoned outputs (capacities: the totals + slack, or
    ``caps``: name -> (elem_cap, cap)), checked against the generator's items. ``rows``: None, or
    entries for a device list of ``dtype``."""
    m = len(items) if rows is None else len(rows)
    wants = {sp.out_name: expect(items, sp, rows) for sp in specs}
    outs = {}
    for sp in specs:
        k = sp.out_name
        ec, cp = caps[k] if caps else (wants[k].totals[0] + slack, wants[k].totals[1] + slack)
        outs[k] = Outs(m, ec, cp, shift)
    got = dec.ragged_elements(specs, rows=None if rows is None else to_dev(rows, dtype), out={k: o.out for k, o in outs.items()})
    for sp in specs:
        k = sp.out_name
        outs[k].check(wants[k])
        assert got.totals[k] == wants[k].totals and got.stats[k].tolist() == wants[k].stats, k
        assert got.capacity[k] == (outs[k].elem_cap, outs[k].cap), k
        assert got.overflowed[k] == (wants[k].totals[0] > outs[k].elem_cap or wants[k].totals[1] > outs[k].cap), k
    return got, wants


def slot_of(dec, key: str) -> int:
    from tfr_reader import dense as D

    return D.resolve_slot(dec, EL(key))


def run_c(dec, items, specs, rows, rdt, row0: int, outs: list | None = None):
    """The same through the C entry point, with a row0 and raw totals and counters."""
    import torch

    m = len(rows)
    wants = [expect(items, sp, rows, row0) for sp in specs]
    outs = outs or [Outs(m, w.totals[0] + 1, w.totals[1] + 1) for w in wants]
    k = len(specs)
    totals = torch.full((k, 2), -1, dtype=torch.int64, device=dev())
    stats = torch.full((k, 4), 77, dtype=torch.int32, device=dev())
    d_rows = to_dev(rows, np.int64 if rdt == N.ROWS_I64 else np.int32)
    R.launch_elems(dec, [o.item(slot_of(dec, sp.key), sp) for o, sp in zip(outs, specs)], (d_rows.data_ptr(), rdt), m, row0,
                   totals.data_ptr(), stats.data_ptr(), None)
    torch.cuda.synchronize()
    for o, w in zip(outs, wants):
        o.check(w)
    assert totals.cpu().tolist() == [list(w.totals) for w in wants]
    assert stats.cpu().numpy().view(np.uint32).tolist() == [w.stats for w in wants]
    return wants


# ------------------------------------------------------------------------------------ the mixed decode
N_MIXED = 600
PER_RECORD = [0, 1, 3, 2, 0, 7]


def mixed_batch() -> tuple[list[bytes], list[dict]]:
    n_elems = sum(PER_RECORD) * (N_MIXED // len(PER_RECORD))
    payloads, items = B.pack(B.random_elems([LENGTHS[i % len(LENGTHS)] for i in range(n_elems)], 31), PER_RECORD)
    assert len(payloads) == N_MIXED
    return payloads, items


@pytest.fixture(scope="module")
def mixed():
    d = new_decoder()
    payloads, items = mixed_batch()
    res = d.decode(*synth.framed(payloads))
    d.set_ragged_tile(TILE)
    yield d, res, items
    d.close()


SPEC = [EL("b")]
LIMITS = ([EL("b", max_elems=me, name=f"e{me}") for me in (1, 2, 5)]
          + [EL("b", max_len=ml, name=f"l{ml}") for ml in (1, 3, 16, 17)]
          + [EL("b", max_len=ml, max_elems=me, name=f"l{ml}e{me}") for ml in (1, 3, 16, 17) for me in (1, 2, 5)])


def with_bad(bad: list[int], n: int, m: int) -> list[int]:
    good = np.random.default_rng(m).integers(0, n, m).tolist()
    bad = [*bad, n, n + 1, -n]
    return [bad[(k // 3) % len(bad)] if k % 3 == 1 else good[k] for k in range(m)]


# ------------------------------------------------------------------------------------ 1. mixed lists
def test_mixed_lists_over_row_lists(mixed):
    d, res, items = mixed
    n = N_MIXED
    rng = np.random.default_rng(1)
    lists = [(None, np.int64), (rng.permutation(n), np.int64), (rng.permutation(n)[:237], np.int32),
             (rng.integers(0, n, 2 * n + 5), np.int64), (rng.integers(0, n, 2 * n + 5), np.int32), (np.full(70, n - 1), np.int64),
             (with_bad(BAD64, n, 327), np.int64), (with_bad(BAD32, n, 327), np.int32), (BAD64, np.int64), (BAD32, np.int32)]
    for rows, dtype in lists:
        got, wants = run(d, items, SPEC, rows, dtype)
        if rows is not None and all(0 <= int(v) < n for v in rows):  # the numpy path, the second reference
            host = res.ragged_elements(SPEC, rows=np.asarray(rows))
            for a, b in zip(got["b"], host["b"]):
                assert np.array_equal(a.cpu().numpy()[: b.size], b)
            assert host.totals["b"] == wants["b"].totals and host.stats["b"].tolist() == wants["b"].stats
    assert len(items[n - 1]["b"]) == 7  # (the 70 copies: rows of seven elements)
    row0 = 1 << 40
    rows = [row0 + (7 * k) % n for k in range(300)]
    rows[3], rows[10], rows[11], rows[40] = row0 - 1, row0 + n, 5, I64_MIN  # (5: in range only without row0)
    run_c(d, items, SPEC, rows, N.ROWS_I64, row0)
    run_c(d, items, SPEC, [100 + (11 * k) % (n + 50) for k in range(300)], N.ROWS_I32, 100)
    run_c(d, items, SPEC, [-3 + k for k in range(40)], N.ROWS_I32, -3)
    run_c(d, items, SPEC, [I64_MAX, 0, I64_MIN, 3], N.ROWS_I64, 0)


# ------------------------------------------------------------------------------------ 2. tile edges
@pytest.mark.parametrize("m", [63, 64, 65, 127, 128, 129])
def test_tile_edges(mixed, m):
    d, _, items = mixed
    rows = np.random.default_rng(m).integers(0, N_MIXED, m)
    run(d, items, SPEC, rows, np.int32 if m % 2 else np.int64)


# ------------------------------------------------------------------------------------ 3. the scan's second pass
def test_tile_scan_carries_into_its_second_pass(mixed):
    d, _, items = mixed
    m = TILE * N.ELEMS_SCAN_THREADS + 70  # more tiles than the scan kernel takes in one pass
    rows = np.random.default_rng(3).integers(0, N_MIXED, m)
    run(d, items, SPEC, rows, np.int32)


# ------------------------------------------------------------------------------------ 4. long list, long element
def long_batch() -> tuple[list[bytes], list[dict]]:
    rng = np.random.default_rng(4)
    counts = [int(c) for c in rng.integers(0, 4, 40)]
    counts[11], counts[29] = 5000, 1
    lens = []
    for r, c in enumerate(counts):
        lens += [300_000] if r == 29 else rng.integers(0, 10, c).tolist()
    elems = B.random_elems(lens, 41)
    payloads, items, at = [], [], 0
    for r, c in enumerate(counts):
        p, it = B.record({b"b": elems[at : at + c]}, entry(b"n", i64(r)))
        payloads.append(p)
        items.append(it)
        at += c
    return payloads, items


@pytest.mark.parametrize("tile", [TILE, 0])
def test_one_long_list_and_one_long_element(tile):
    d = new_decoder()
    try:
        payloads, items = long_batch()
        d.decode(*synth.framed(payloads))
        d.set_ragged_tile(tile)
        assert len(items[11]["b"]) == 5000 and len(items[29]["b"][0]) == 300_000
        run(d, items, SPEC, None)
        rows = np.random.default_rng(5).permutation(np.concatenate([np.arange(40), [11, 29, 29]]))
        run(d, items, SPEC, rows, shift=7)
        run(d, items, [EL("b", max_len=70_001, max_elems=4099)], rows, np.int32)
    finally:
        d.close()


# ------------------------------------------------------------------------------------ 5. capacities
def test_capacities(mixed):
    import torch

    d, _, items = mixed
    rows = np.random.default_rng(6).integers(0, N_MIXED, 200).tolist()
    m = len(rows)
    # E and B from a totals-only call: no elem_offsets, no values
    first = Outs(m, None, None)
    want = run_c(d, items, SPEC, rows, N.ROWS_I64, 0, outs=[first])[0]
    E, Bt = want.totals
    ro, eo = want.row_offsets, want.elem_offsets
    k = next(k for k in range(m) if ro[k + 1] - ro[k] >= 3 and ro[k] >= 2)
    e = next(e for e in range(E) if eo[e + 1] - eo[e] >= 3 and eo[e] >= 2)
    inside_row, inside_elem = int(ro[k]) + 1, int(eo[e]) + 1
    assert 1 < inside_row < E - 1 and 1 < inside_elem < Bt - 1
    shifts = [0, 1, 7, 15]
    i = 0
    for ec in (0, 1, inside_row, E - 1, E, E + 3):
        for cp in (0, 1, inside_elem, Bt - 1, Bt, Bt + 3):
            for shift in shifts if (ec, cp) in ((E, Bt), (inside_row, Bt + 3), (E + 3, inside_elem)) else [shifts[i % 4]]:
                got, _ = run(d, items, SPEC, rows, caps={"b": (ec, cp)}, shift=shift)
                assert got.overflowed["b"] == (ec < E or cp < Bt) and got.totals["b"] == (E, Bt)
            i += 1
    # elem_offsets without values: the offsets are complete, B still counts every element
    outs = Outs(m, E, None)
    run_c(d, items, SPEC, rows, N.ROWS_I64, 0, outs=[outs])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ 6. limits
def test_max_elems_and_max_len_with_their_counters(mixed):
    d, res, items = mixed
    rng = np.random.default_rng(7)
    for rows in (None, rng.integers(0, N_MIXED, 333)):
        got, wants = run(d, items, LIMITS, rows)
        assert wants["e1"].stats[0] > 0 and wants["l3"].stats[1] > 0 and min(wants["l16e2"].stats[:2]) > 0
    assert len(LIMITS) == 19 <= N.ELEMS_MAX_SPECS
    rows = with_bad(BAD64, N_MIXED, 90)
    run_c(d, items, LIMITS[3:9], rows, N.ROWS_I64, 0)


# ------------------------------------------------------------------------------------ 7. sources
@pytest.mark.parametrize("materialize", [False, True])
def test_views_and_materialized_column(materialize):
    d = new_decoder()
    try:
        payloads, items = mixed_batch()
        res = d.decode(*synth.framed(payloads), materialize_bytes=materialize)
        assert (res.bytes_data is not None) == materialize
        d.set_ragged_tile(TILE)
        specs = [EL("b"), EL("b", max_len=16, max_elems=2, name="cut")]
        rows = np.random.default_rng(8).integers(0, N_MIXED, 777)
        for r in (None, rows):
            got, _ = run(d, items, specs, r, shift=1)
            host = res.ragged_elements(specs, rows=r)
            for k in host:
                for a, b in zip(got[k], host[k]):
                    assert np.array_equal(a.cpu().numpy()[: b.size], b), k
    finally:
        d.close()


N1 = 5000
C1_ITEMS = [{"id": [b"img-%08d" % i]} for i in range(N1)]


def check_c1(d, res, fr) -> None:
    check_c1_rows(d)
    again = d._fetch(*fr, d.info(), False)  # the full view is still there afterwards
    for k in COLS:
        assert np.array_equal(getattr(again, k), getattr(res, k)), k


def check_c1_rows(d) -> None:
    d.set_ragged_tile(TILE)
    spec = [EL("id"), EL("id", max_len=5, name="id5")]
    rng = np.random.default_rng(9)
    for rows, dtype in ((None, np.int64), (rng.permutation(N1), np.int64), (rng.integers(0, N1, 2 * N1 + 3), np.int32),
                        (with_bad(BAD64, N1, 1027), np.int64), (np.full(70, N1 - 1), np.int32)):
        got, wants = run(d, C1_ITEMS, spec, rows, dtype)
        # one element per record: the call agrees with ragged (U8) over the same rows
        d_rows = None if rows is None else to_dev(rows, dtype)
        rg = d.ragged([R.Ragged("id", "uint8")], rows=d_rows)
        v, eo, ro = (t.cpu().numpy() for t in got["id"])
        rv, roff = (t.cpu().numpy() for t in rg["id"])
        E, Bt = got.totals["id"]
        assert rg.totals["id"] == Bt and np.array_equal(v[:Bt], rv[:Bt])
        assert np.array_equal(eo[ro[:-1][np.diff(ro) > 0]], roff[:-1][np.diff(ro) > 0]) and int(roff[-1]) == int(eo[E])
        assert np.array_equal(np.diff(roff), 12 * np.diff(ro))
        if rows is not None and len(rows) == 70:
            assert bytes(v[:12]) == b"img-%08d" % (N1 - 1)
    run_c(d, C1_ITEMS, spec, [100 + (11 * k) % (N1 + 50) for k in range(300)], N.ROWS_I32, 100)


@pytest.mark.parametrize("mode", ["ends", "u32"])
def test_optimistic_c1_decode_with_implicit_offsets(mode):
    """A device-resident decode with u32 record ends: the ``id`` slot's bytes_off words are not stored
    (tfrg_info.implicit_off_slots) and the column is poisoned before the decode, so every byte comes
    from the end-relative view."""
    fr = synth.framed(synth.c1_payloads(N1))
    d = IO.new_decoder(fr)
    fresh = IO.new_decoder(fr, optimistic="0")
    try:
        want = IO.Run(fresh, *fr, mode).fetch()
        sid = want.slot_key.index("id")
        assert int(want.info.implicit_cols) == 0 and int(want.info.implicit_off_slots) == 0
        run = IO.Run(d, *fr, mode)  # (no info, fetch or view before the calls: they confirm the decode)
        check_c1_rows(d)
        info = run.info()
        assert int(info.implicit_cols) == 7 and int(info.implicit_off_slots) == 1 << sid and run.reruns() == 0
        run.assert_raw(want, 1 << sid)  # (poison still: the calls neither read nor wrote the column)
        IO.assert_equal_columns(run.fetch(), want)  # the full view afterwards: as a decode that stores every column
    finally:
        fresh.close()
        d.close()


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


def test_c1_decode_that_stores_every_column():
    d = new_decoder({"TFRG_OPTIMISTIC": "0"})
    try:
        fr = synth.framed(synth.c1_payloads(N1))
        res = d.decode(*fr)
        assert int(res.info.implicit_cols) == 0
        check_c1(d, res, fr)
    finally:
        d.close()


def test_c1_after_a_hinted_decode_that_reruns():
    d = new_decoder()
    try:
        fr = synth.framed(synth.c1_payloads(N1))
        d.set_value_caps(100, 100, 100)  # far below the batch's values
        res = d.decode(*fr)
        assert d.device_bytes()[1] >= 1
        check_c1(d, res, fr)
    finally:
        d.close()


# ------------------------------------------------------------------------------------ 8. element 0
def test_element_zero_is_what_ragged_takes(mixed):
    d, _, items = mixed
    rows = np.random.default_rng(10).integers(0, N_MIXED, 500)
    d_rows = to_dev(rows)
    got = d.ragged_elements(SPEC, rows=d_rows)
    rg = d.ragged([R.Ragged("b", "uint8")], rows=d_rows)
    v, eo, ro = (t.cpu().numpy() for t in got["b"])
    rv, roff = (t.cpu().numpy() for t in rg["b"])
    for k in range(len(rows)):
        first = bytes(v[eo[ro[k]] : eo[ro[k] + 1]]) if ro[k + 1] > ro[k] else b""
        assert first == bytes(rv[roff[k] : roff[k + 1]]) == (items[rows[k]]["b"] or [b""])[0], k
    assert int(rg.stats["b"][2]) == int((np.diff(ro) > 1).sum()) > 0  # ragged's multi rows: more than one element here


# ------------------------------------------------------------------------------------ 9. determinism
def test_two_equal_calls_write_equal_bytes(mixed):
    d, _, items = mixed
    rows = np.random.default_rng(11).integers(0, N_MIXED, 1000)
    want = expect(items, SPEC[0], rows)
    bufs = []
    for _ in range(2):
        o = Outs(len(rows), want.totals[0] - 5, want.totals[1] - 40, shift=15)
        d.ragged_elements(SPEC, rows=to_dev(rows), out={"b": o.out})
        o.check(want)
        bufs.append([b.cpu().numpy() for b in (o.v_buf, o.eo_buf, o.ro_buf)])
    for a, b in zip(*bufs):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------ 10. stream order
def test_rows_made_just_before_and_results_used_just_after(mixed):
    """The row list is produced by kernels queued on the consumer stream immediately before the call
    and the outputs are consumed on it immediately after, with no synchronisation in between: on a
    side stream, and on the legacy default stream."""
    import torch

    d, _, items = mixed
    for stream in (torch.cuda.Stream(dev()), torch.cuda.default_stream(dev())):
        with torch.cuda.stream(stream):
            big = torch.arange(1 << 22, device=dev(), dtype=torch.int64)
            rows = (big.flip(0)[: 1 << 13] * 7919) % N_MIXED  # (queued on the stream; not finished at the call)
            got = d.ragged_elements(SPEC, rows=rows, capacity=(1 << 16, 1 << 20))
            v, eo, ro = got["b"]
            nbytes = eo[ro[-1]]
            picked = torch.where(torch.arange(1 << 20, device=dev()) < nbytes, v.to(torch.int64), 0).sum()
            twice = d.ragged_elements(SPEC, rows=rows, capacity=(1 << 16, 1 << 20))
            total = int(picked)
        want = expect(items, SPEC[0], rows.cpu().numpy())
        E, Bt = want.totals
        assert total == int(want.values.astype(np.int64).sum())
        for b in (got, twice):
            assert np.array_equal(b["b"][0].cpu().numpy()[:Bt], want.values)
            assert np.array_equal(b["b"][1].cpu().numpy()[: E + 1], want.elem_offsets)
            assert np.array_equal(b["b"][2].cpu().numpy(), want.row_offsets)
            assert b.stats["b"].tolist() == want.stats and b.totals["b"] == (E, Bt) and not b.overflowed["b"]
    # stream=: a raw handle as the consumer stream, the rows made on it; the current stream is another
    s = torch.cuda.Stream(dev())
    with torch.cuda.stream(s):
        rows = (torch.arange(1 << 20, device=dev(), dtype=torch.int64).flip(0)[:5000] * 31) % N_MIXED
    got = d.ragged_elements(SPEC, rows=rows, stream=s.cuda_stream)  # (capacity=None: totals, then the gather)
    s.synchronize()
    want = expect(items, SPEC[0], rows.cpu().numpy())
    for a, b in zip(got["b"], (want.values, want.elem_offsets, want.row_offsets)):
        assert np.array_equal(a.cpu().numpy(), b)


# ------------------------------------------------------------------------------------ 11. arguments
def test_c_level_argument_errors_and_empty_cases():
    import torch

    lib = N.lib()
    d = new_decoder()
    try:
        m = 3
        d_rows = to_dev([0, 1, 2])
        tot = torch.full((2, 2), -1, dtype=torch.int64, device=dev())
        st = torch.full((2, 4), 77, dtype=torch.int32, device=dev())
        outs = Outs(7, 16, 256)

        def call(k=1, rows_ptr=d_rows.data_ptr(), rdt=N.ROWS_I64, m=m, ctx=True, **kw):
            f = dict(slot=0, max_elems=0, max_len=0, reserved=0, elem_cap=16, cap=256, values=outs.v.data_ptr(),
                     elem_offsets=outs.eo.data_ptr(), row_offsets=outs.ro.data_ptr())
            f.update(kw)
            arr = (N.TfrgElemsSpec * max(k, 1))(*[N.TfrgElemsSpec(**f) for _ in range(max(k, 1))])
            return lib.tfrg_result_ragged_elems(d._ctx if ctx else None, arr, k, C.c_void_p(rows_ptr) if rows_ptr else None,
                                                rdt, m, 0, C.c_void_p(tot.data_ptr()), C.c_void_p(st.data_ptr()), None)

        def refused(**bad) -> None:
            assert call(**bad) == -1, bad
            assert lib.tfrg_last_error().startswith(b"tfrg_result_ragged_elems: "), bad
            torch.cuda.synchronize()
            outs.untouched()
            assert tot.cpu().tolist() == [[-1, -1]] * 2 and st.cpu().tolist() == [[77] * 4] * 2, bad

        refused(ctx=False)
        refused()  # no result
        assert b"no result" in lib.tfrg_last_error()
        fr = synth.framed(synth.c1_payloads(10))
        res = d.decode(*fr)
        s_label, s_id = res.slot_key.index("label"), res.slot_key.index("id")
        ro_ptr, eo_ptr = outs.ro.data_ptr(), outs.eo.data_ptr()
        for bad in (dict(k=0), dict(k=N.ELEMS_MAX_SPECS + 1), dict(slot=len(res.slot_key)), dict(slot=s_label),
                    dict(slot=s_id, row_offsets=None), dict(slot=s_id, row_offsets=ro_ptr + 4),
                    dict(slot=s_id, elem_offsets=eo_ptr + 4), dict(slot=s_id, elem_offsets=None),  # (values without them)
                    dict(slot=s_id, reserved=1), dict(slot=s_id, rdt=2), dict(slot=s_id, m=1 << 31),
                    dict(slot=s_id, m=(1 << 32) - 1)):
            refused(**bad)
        # rows NULL: every record in order, rows_dtype ignored; m may differ from n
        assert call(slot=s_id, rows_ptr=None, rdt=9, m=7) == 0
        torch.cuda.synchronize()
        outs.check(expect(C1_ITEMS[:10], EL("id"), list(range(7))))
        assert tot.cpu().tolist()[0] == [7, 84] and st.cpu().tolist()[0] == [0, 0, 0, 0]
        # m == 0: row_offsets[0] = 0, elem_offsets[0] = 0, totals 0, no kernel
        outs = Outs(7, 16, 256)
        assert call(k=1, slot=s_id, m=0, rows_ptr=None) == 0
        torch.cuda.synchronize()
        assert outs.ro.cpu().tolist()[0] == 0 and outs.eo.cpu().tolist()[0] == 0
        assert bool((outs.ro_buf[GUARD + 8 :] == POISON).all()) and bool((outs.eo_buf[GUARD + 8 :] == POISON).all())
        assert bool((outs.v_buf == POISON).all())
        assert tot.cpu().tolist()[0] == [0, 0] and st.cpu().tolist()[0] == [0] * 4
        # n == 0: every row is skipped, all offsets and totals are 0
        assert len(d.decode(fr[0][:0], fr[1][:0], fr[2][:0])) == 0
        outs = Outs(3, 16, 256)
        tot.fill_(-1)
        assert call(slot=s_id) == 0
        torch.cuda.synchronize()
        assert outs.ro.cpu().tolist() == [0, 0, 0, 0] and outs.eo.cpu().tolist()[0] == 0
        assert bool((outs.eo_buf[GUARD + 8 :] == POISON).all()) and bool((outs.v_buf == POISON).all())
        assert tot.cpu().tolist()[0] == [0, 0] and st.cpu().tolist()[0] == [0, 0, 0, 3]
        got = d.ragged_elements([EL("id")], rows=to_dev([0, 5]))
        assert got["id"][2].cpu().tolist() == [0, 0, 0] and got.stats["id"].tolist() == [0, 0, 0, 2]
        assert got.totals["id"] == (0, 0) and got["id"][1].cpu().tolist() == [0]
    finally:
        d.close()


# ------------------------------------------------------------------------------------ 12. Python
def test_python_capacity_out_select_rows_and_absent_key(mixed):
    import torch

    d, _, items = mixed
    rows = np.random.default_rng(12).integers(0, N_MIXED, 400)
    d_rows = to_dev(rows)
    want = expect(items, SPEC[0], rows)
    E, Bt = want.totals
    # capacity=None: exact sizes behind one read-back
    got = d.ragged_elements(SPEC, rows=d_rows)
    v, eo, ro = got["b"]
    assert v.numel() == Bt and eo.numel() == E + 1 and ro.numel() == len(rows) + 1 and got.capacity["b"] == (E, Bt)
    assert np.array_equal(v.cpu().numpy(), want.values) and np.array_equal(eo.cpu().numpy(), want.elem_offsets)
    assert np.array_equal(ro.cpu().numpy(), want.row_offsets)
    assert got.totals["b"] == (E, Bt) and got.stats["b"].tolist() == want.stats and not got.overflowed["b"]
    # a capacity pair with an overflow: the prefixes that fit, complete row offsets
    for cap, over in (((E - 1, Bt), True), ((E, Bt - 1), True), ({"b": (E, Bt)}, False)):
        got = d.ragged_elements(SPEC, rows=d_rows, capacity=cap)
        ec, cp = cap["b"] if isinstance(cap, dict) else cap
        v, eo, ro = (t.cpu().numpy() for t in got["b"])
        assert v.size == cp and eo.size == ec + 1 and got.overflowed["b"] == over and got.totals["b"] == (E, Bt)
        kept = min(int(want.elem_offsets[min(E, ec)]), cp)
        assert np.array_equal(v[:kept], want.values[:kept]) and np.array_equal(eo, want.elem_offsets[: ec + 1])
        assert np.array_equal(ro, want.row_offsets)
    for bad in (5, (1,), (1, -1), (1.5, 2), "ab"):
        with pytest.raises(ValueError):
            d.ragged_elements(SPEC, rows=d_rows, capacity=bad)
    # out= is checked
    ok = (torch.empty(8, dtype=torch.uint8, device=dev()), torch.empty(4, dtype=torch.int64, device=dev()),
          torch.empty(len(rows) + 1, dtype=torch.int64, device=dev()))
    for i, wrong in ((0, ok[0].to(torch.int32)), (0, ok[0].cpu()), (1, ok[1].to(torch.int32)), (1, ok[1][:0]),
                     (2, ok[2][:-1]), (2, ok[2].to(torch.int32))):
        with pytest.raises(ValueError):
            d.ragged_elements(SPEC, rows=d_rows, out={"b": tuple(wrong if j == i else t for j, t in enumerate(ok))})
    # rows=dec.select(...).rows with its -1 tail: the tail's rows are skipped (empty) rows
    sel = d.select([SEL.Term("n", "int64", "<", 100)], capacity=130)
    assert sel.rows.numel() == 130 and sel.rows.cpu().tolist()[100:] == [-1] * 30
    got = d.ragged_elements(SPEC, rows=sel.rows)
    want = expect(items, SPEC[0], sel.rows.cpu().numpy())
    assert want.stats[3] == 30 and got.stats["b"].tolist() == want.stats and got.totals["b"] == want.totals
    for a, b in zip(got["b"], (want.values, want.elem_offsets, want.row_offsets)):
        assert np.array_equal(a.cpu().numpy(), b)
    # an absent key: all-empty rows without a launch, beside a present one
    specs = [EL("zz", name="absent"), EL("b")]
    got = d.ragged_elements(specs, rows=to_dev([0, N_MIXED, -1, 5, I64_MAX]))
    assert got["absent"][2].cpu().tolist() == [0] * 6 and got["absent"][1].cpu().tolist() == [0]
    assert got.stats["absent"].tolist() == [0, 0, 2, 3] and got.totals["absent"] == (0, 0) and not got.overflowed["absent"]
    assert got.stats["b"].tolist() == expect(items, SPEC[0], [0, N_MIXED, -1, 5, I64_MAX]).stats
