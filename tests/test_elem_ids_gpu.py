"""Element ids on the device (tfrg_result_elem_ids: k_id_len / k_id_scan / k_id_write): every case is a
raw call of the C entry point whose ids and row offsets must equal tests/_ids_ref.py -- the generator's
own items, a Python dict and the Python restatement of tfrg_hash64; nothing from a decode's columns or
the C lookup. Every output lies inside a larger buffer prefilled with 0xA5: the guards and everything
past the stored prefix keep the poison. Where a case wants "some" elements to match, the reference
alone is asserted to have 0 < matched < E."""

import ctypes as C

import numpy as np
import pytest

from tests import _bytes_ref as B
from tests import _ids_ref as IR
from tests import test_implicit_off_gpu as IO
from tests.golden.gen_golden import entry, i64
from tests.test_elem_ids_host import NEAR, W17, RawVocab
from tests.test_ragged_gpu import GUARD, I64_MAX, I64_MIN, POISON, dev, new_decoder, to_dev
from tfr_reader import _native as N
from tfr_reader import dense as D
from tfr_reader import ids as I
from tfr_reader import ragged as R
from tfr_reader import synth

pytestmark = pytest.mark.gpu

TILE = 64
LENGTHS = [0, 1, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4099]
PER = [0, 1, 2, 5]
N_REC = 200
LONG_REC, LONG_COUNT = 57, 1100  # more than one pass of 4 x 256 elements inside a tile
SPECIALS = [W17, *NEAR, b"a", b"a\0", b""]


# ------------------------------------------------------------------------------------ poisoned outputs
class Outs:
    """Poisoned outputs of one spec over m rows: ``ids`` [cap] (None: a NULL ids) and ``row_offsets``
    [m + 1], each between GUARD bytes of poison."""

    def __init__(self, m: int, cap: int | None) -> None:
        import torch

        def poisoned(nbytes: int):
            return torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device=dev())

        self.m, self.cap = m, cap
        self.ro_buf = poisoned((m + 1) * 8)
        self.ro = self.ro_buf[GUARD : GUARD + (m + 1) * 8].view(torch.int64)
        self.id_buf = self.ids = None
        if cap is not None:
            self.id_buf = poisoned(cap * 8)
            self.ids = self.id_buf[GUARD : GUARD + cap * 8].view(torch.int64)

    def untouched(self) -> None:
        for b in (self.ro_buf, self.id_buf):
            assert b is None or bool((b == POISON).all())

    def check(self, want) -> None:
        ro = self.ro_buf.cpu().numpy()
        assert np.array_equal(ro[GUARD:-GUARD].view(np.int64), want.row_offsets)
        assert (ro[:GUARD] == POISON).all() and (ro[-GUARD:] == POISON).all()
        if self.id_buf is None:
            return
        kept = min(want.total, self.cap)
        got = self.id_buf.cpu().numpy()
        ids = got[GUARD : GUARD + kept * 8].view(np.int64)
        bad = np.flatnonzero(ids != want.ids[:kept])
        assert bad.size == 0, (int(bad[0]), int(ids[bad[0]]), int(want.ids[bad[0]]), want.elems[bad[0]][:40], bad.size)
        assert (got[:GUARD] == POISON).all() and (got[GUARD + kept * 8 :] == POISON).all()


def slot_of(dec, key: str) -> int:
    return D.resolve_slot(dec, R.RaggedElements(key))


def call_c(dec, cases, outs, rows_ptr, rdt, m, row0, totals, stats, **over) -> int:
    """One raw tfrg_result_elem_ids call: ``cases`` are (rule, vocabulary handle or None)."""
    arr = (N.TfrgIdsSpec * len(cases))()
    for a, (rule, voc), o in zip(arr, cases, outs):
        a.slot, a.max_elems, a.reserved0, a.reserved1 = slot_of(dec, rule.key), rule.max_elems or 0, 0, 0
        a.vocab = voc.ptr.value if voc is not None else None
        a.num_oov_buckets, a.oov_base, a.default_id = rule.buckets, rule.base, rule.default
        a.elem_cap = o.cap or 0
        a.ids = o.ids.data_ptr() if o.ids is not None and o.cap else None
        a.row_offsets = o.ro.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
    return dec._lib.tfrg_result_elem_ids(dec._ctx, arr, len(cases), C.c_void_p(rows_ptr) if rows_ptr else None, rdt, m, row0,
                                         C.c_void_p(totals.data_ptr()) if totals is not None else None,
                                         C.c_void_p(stats.data_ptr()) if stats is not None else None, None)


def run_c(dec, items, cases, rows, rdt=N.ROWS_I64, row0: int = 0, caps=None, with_stats: bool = True):
    """The call over poisoned outputs (capacity: E + 3, or ``caps[i]``; None: a NULL ids), checked
    against the reference. ``rows``: None, or the entries of a device list."""
    import torch

    m = len(items) if rows is None else len(rows)
    wants = [IR.expect(items, rule, rows, row0) for rule, _ in cases]
    caps = caps if caps is not None else [w.total + 3 for w in wants]
    outs = [Outs(m, c) for c in caps]
    k = len(cases)
    totals = torch.full((k,), -1, dtype=torch.int64, device=dev())
    stats = torch.full((k, 4), 77, dtype=torch.int32, device=dev()) if with_stats else None
    d_rows = None if rows is None else to_dev(rows, np.int64 if rdt == N.ROWS_I64 else np.int32)
    rc = call_c(dec, cases, outs, d_rows.data_ptr() if d_rows is not None else None, rdt, m, row0, totals, stats)
    assert rc == 0, dec._lib.tfrg_last_error()
    torch.cuda.synchronize()
    for o, w in zip(outs, wants):
        o.check(w)
    assert totals.cpu().tolist() == [w.total for w in wants]
    if with_stats:
        assert stats.cpu().numpy().view(np.uint32).tolist() == [w.stats for w in wants]
    return wants, outs


# ------------------------------------------------------------------------------------ the batch
def main_batch() -> tuple[list[bytes], list[dict]]:
    """200 records of 0, 1, 2 or 5 elements under b"b" (one of 1100), the lengths cut from one random
    blob, the special elements early; one to three short tags under b"c". The b"b" list is a record's
    last field, so the last record's last element ends at the end of the input."""
    counts = [PER[r % len(PER)] for r in range(N_REC)]
    counts[LONG_REC] = LONG_COUNT
    total = sum(counts)
    elems = B.random_elems([LENGTHS[i % len(LENGTHS)] for i in range(total - len(SPECIALS))], 51)
    elems[3:3] = SPECIALS
    payloads, items, at = [], [], 0
    for r, c in enumerate(counts):
        p, it = B.record({b"c": [b"tag%d" % ((r + j) % 7) for j in range(r % 3 + 1)], b"b": elems[at : at + c]}, entry(b"n", i64(r)))
        payloads.append(p)
        items.append(it)
        at += c
    assert at == total == len(elems)
    return payloads, items


def payload_input(payloads):
    lens = np.array([len(p) for p in payloads], np.uint64)
    en = np.cumsum(lens, dtype=np.uint64)
    return np.frombuffer(b"".join(payloads), np.uint8), en - lens, en


class Tables:
    """The vocabularies of the cases, each as a device tfrg_vocab and as the reference's dict."""

    def __init__(self, items) -> None:
        elems = [e for it in items for e in it["b"]]
        half = list(dict.fromkeys([*elems[::2], W17, b"a", b""]))
        self.words = [w for w in half if w not in NEAR and w != b"a\0"]
        self.model = IR.TableModel(self.words)
        self.neg_ids = [5 * i - 1000 for i in range(len(self.words))]
        self.other = [w for w in self.words if w not in (b"", b"a")] + [b"a\0"]  # no empty word, b"a\0" for b"a"
        self.tags = [b"tag%d" % i for i in range(0, 7, 2)]
        self.t_half = {w: i for i, w in enumerate(self.words)}
        self.t_neg = dict(zip(self.words, self.neg_ids))
        self.t_other = {w: i for i, w in enumerate(self.other)}
        self.t_tags = {w: i for i, w in enumerate(self.tags)}
        self.v_half, self.v_neg = RawVocab(self.words, device=0), RawVocab(self.words, self.neg_ids, device=0)
        self.v_other, self.v_tags, self.v_none = RawVocab(self.other, device=0), RawVocab(self.tags, device=0), RawVocab([], device=0)
        self.all = [self.v_half, self.v_neg, self.v_other, self.v_tags, self.v_none]
        for v in self.all:
            assert v.rc == 0, N.lib().tfrg_last_error()
        nw, cap, probe, dbytes = self.v_half.info()
        assert (nw, cap, probe) == (len(self.words), self.model.capacity, self.model.max_probe) and dbytes > 0

    def close(self) -> None:
        for v in self.all:
            v.close()


@pytest.fixture(scope="module")
def main():
    d = new_decoder()
    payloads, items = main_batch()
    buf, st, en = payload_input(payloads)
    last = items[-1]["b"][-1]
    assert buf.size % 16 != 0 and len(last) > 0 and bytes(buf[-len(last) :]) == last  # (it ends at nbytes)
    res = d.decode(buf, st, en, payload_only=True)
    assert len(res) == N_REC and int(res.status.max()) == 0
    d.set_ragged_tile(TILE)
    t = Tables(items)
    yield d, res, items, t
    t.close()
    d.close()


BAD64 = [-1, N_REC, N_REC + 1, (1 << 31) - 1, I64_MIN, I64_MAX, -N_REC, 1 << 32, (1 << 32) + 5, -(1 << 32)]
BAD32 = [-1, N_REC, N_REC + 1, (1 << 31) - 1, -(1 << 31), -N_REC]


def with_bad(bad: list[int], m: int, row0: int = 0) -> list[int]:
    good = (np.random.default_rng(m).integers(0, N_REC, m) + row0).tolist()
    return [bad[(k // 3) % len(bad)] if k % 3 == 1 else good[k] for k in range(m)]


# ------------------------------------------------------------------------------------ 1. shapes
def test_the_batch_has_the_shapes(main):
    _, _, items, t = main
    counts = [len(it["b"]) for it in items]
    assert set(counts) == {0, 1, 2, 5, LONG_COUNT} and counts[LONG_REC] == LONG_COUNT > 4 * 256
    lens = {len(e) for it in items for e in it["b"]}
    assert lens >= set(LENGTHS)
    whole = IR.expect(items, IR.Rule("b", t.t_half))
    assert 0 < whole.matched < whole.total and 0.3 < whole.matched / whole.total < 0.7  # about half
    assert t.model.max_probe >= 1
    displaced = {w for w, dd in zip(t.words, t.model.disp) if dd >= 1}
    assert displaced & set(whole.elems)  # a displaced word is looked up
    for s in NEAR:
        assert s in whole.elems and s not in t.t_half
    assert W17 in t.t_half and b"" in t.t_half and b"" not in t.t_other and b"a\0" in t.t_other and b"a" not in t.t_other


# ------------------------------------------------------------------------------------ 2. row lists
def test_row_lists(main):
    d, _, items, t = main
    n = N_REC
    cases = [(IR.Rule("b", t.t_half, 7, len(t.words)), t.v_half)]
    rng = np.random.default_rng(1)
    wants, _ = run_c(d, items, cases, None)
    assert 0 < wants[0].matched < wants[0].total and wants[0].total > LONG_COUNT
    assert n % TILE != 0  # an m that is not a multiple of the tile
    run_c(d, items, cases, rng.permutation(n), N.ROWS_I64)
    run_c(d, items, cases, rng.permutation(n)[:137], N.ROWS_I32)
    run_c(d, items, cases, [LONG_REC, 3, LONG_REC, 3, 3, 7, LONG_REC], N.ROWS_I32)  # duplicates
    run_c(d, items, cases, with_bad(BAD64, 327), N.ROWS_I64)
    run_c(d, items, cases, with_bad(BAD32, 327), N.ROWS_I32)
    wants, _ = run_c(d, items, cases, BAD64, N.ROWS_I64)  # a list of only skipped rows
    assert wants[0].stats == [0, 0, 0, len(BAD64)] and wants[0].total == 0
    run_c(d, items, cases, BAD32, N.ROWS_I32)
    row0 = 1 << 40
    rows = [row0 + (7 * k) % n for k in range(300)]
    rows[3], rows[10], rows[11], rows[40] = row0 - 1, row0 + n, 5, I64_MIN  # (5: in range only without row0)
    run_c(d, items, cases, rows, N.ROWS_I64, row0)
    run_c(d, items, cases, [100 + (11 * k) % (n + 50) for k in range(300)], N.ROWS_I32, 100)
    run_c(d, items, cases, [-3 + k for k in range(70)], N.ROWS_I32, -3)
    run_c(d, items, cases, [I64_MAX, 0, I64_MIN, LONG_REC], N.ROWS_I64, 0)


@pytest.mark.parametrize("m", [63, 64, 65, 129])
def test_tile_edges(main, m):
    d, _, items, t = main
    rows = np.random.default_rng(m).integers(0, N_REC, m)
    run_c(d, items, [(IR.Rule("b", t.t_half, default=-9), t.v_half)], rows, N.ROWS_I32 if m % 2 else N.ROWS_I64)


def test_tile_scan_carries_into_its_second_pass(main):
    d, _, items, t = main
    m = TILE * N.IDS_SCAN_THREADS + 70  # more tiles than the scan kernel takes in one pass
    rows = np.random.default_rng(8).integers(0, N_REC, m)
    wants, _ = run_c(d, items, [(IR.Rule("c", t.t_tags, 5, 10), t.v_tags)], rows, N.ROWS_I32)  # (short tags: a quick reference)
    assert wants[0].total > m and 0 < wants[0].matched < wants[0].total


# ------------------------------------------------------------------------------------ 3. tables
def table_cases(t) -> list:
    nw = len(t.words)
    cases = [(IR.Rule("b", t.t_half, default=-1), t.v_half), (IR.Rule("b", t.t_half, default=I64_MIN), t.v_half)]
    cases += [(IR.Rule("b", t.t_half, nb, base), t.v_half) for nb in (1, 7, 1000) for base in (0, nw)]
    cases += [(IR.Rule("b", t.t_neg, default=12345), t.v_neg), (IR.Rule("b", t.t_neg, 7, -3), t.v_neg)]
    cases += [(IR.Rule("b", t.t_other, default=-2), t.v_other)]
    cases += [(IR.Rule("b", {}, default=4), t.v_none), (IR.Rule("b", {}, 1000, 10), t.v_none)]  # a vocabulary of 0 words
    cases += [(IR.Rule("b", None, nb, 0), None) for nb in (1, 7, 1000, 1024, (1 << 40) + 1, (1 << 64) - 1)]  # pure hashing
    cases += [(IR.Rule("b", None, 7, I64_MAX), None)]  # (int64 arithmetic wraps)
    return cases


def test_tables_and_oov_handling_in_one_call(main):
    d, _, items, t = main
    cases = table_cases(t)
    assert 2 < len(cases) <= N.IDS_MAX_SPECS  # the same slot with different tables
    rows = np.random.default_rng(2).permutation(np.concatenate([np.arange(0, N_REC, 2), [LONG_REC, 0, 1, 2, 3, 4, 5, 6, 7]]))
    wants, _ = run_c(d, items, cases, rows)
    for (rule, _), w in zip(cases, wants):
        if rule.table:
            assert 0 < w.matched < w.total, rule
        else:
            assert w.matched == 0 and w.stats[1] == w.total
    by_elem = dict(zip(wants[0].elems, wants[0].ids.tolist()))
    assert by_elem[W17] == t.t_half[W17] and all(by_elem[s] == -1 for s in NEAR)  # the near misses
    assert by_elem[b"a"] == t.t_half[b"a"] and by_elem[b"a\0"] == -1 and by_elem[b""] == t.t_half[b""]
    other = dict(zip(wants[10].elems, wants[10].ids.tolist()))
    assert cases[10][1] is t.v_other and other[b"a"] == -2 and other[b""] == -2 and other[b"a\0"] == t.t_other[b"a\0"]
    assert cases[8][1] is t.v_neg and (wants[8].ids < 0).any() and (wants[8].ids == 12345).any()  # explicit ids, negative too
    run_c(d, items, cases, None)


def test_two_slots_in_one_call(main):
    d, _, items, t = main
    cases = [(IR.Rule("c", t.t_tags, 3, 100), t.v_tags), (IR.Rule("b", t.t_half, default=-1), t.v_half),
             (IR.Rule("c", None, 5, 0), None)]
    for rows in (None, with_bad(BAD64, 150)):
        wants, _ = run_c(d, items, cases, rows)
        assert 0 < wants[0].matched < wants[0].total and wants[0].stats[2] == 0


def test_max_elems_with_its_counter(main):
    d, _, items, t = main
    cases = [(IR.Rule("b", t.t_half, 7, 0, max_elems=me), t.v_half) for me in (1, 2, 5, 1024, 1099, 1100)]
    cases += [(IR.Rule("c", t.t_tags, default=-1, max_elems=2), t.v_tags)]
    for rows in (None, with_bad(BAD32, 200), [LONG_REC] * 3):
        wants, _ = run_c(d, items, cases, rows, N.ROWS_I32)
        assert wants[0].stats[0] > 0
        if rows is None:  # (every record: the long list and the records of three tags are cut)
            assert wants[4].stats[0] == 1 and wants[6].stats[0] > 0
    assert IR.expect(items, cases[5][0]).stats[0] == 0


# ------------------------------------------------------------------------------------ 4. capacities
def test_elem_cap_below_the_total_and_null_ids(main):
    d, _, items, t = main
    rule = IR.Rule("b", t.t_half, 7, 0)
    rows = np.random.default_rng(3).integers(0, N_REC, 150).tolist() + [LONG_REC]
    E = IR.expect(items, rule, rows).total
    assert E > 1200
    for cap in (0, 1, 255, 256, 1024, E - 1, E, E + 3):
        run_c(d, items, [(rule, t.v_half)], rows, caps=[cap])
    run_c(d, items, [(rule, t.v_half)], rows, caps=[7], with_stats=False)  # (no counters: the tail is not even read)
    run_c(d, items, [(rule, t.v_half)], rows, caps=[None])  # ids NULL: offsets and counters, unmatched included
    run_c(d, items, [(rule, t.v_half)], rows, caps=[None], with_stats=False)
    run_c(d, items, [(rule, t.v_half), (rule, t.v_half)], rows, caps=[None, 40])


# ------------------------------------------------------------------------------------ 5. sources
def test_materialized_column():
    d = new_decoder()
    t = None
    try:
        payloads, items = main_batch()
        res = d.decode(*payload_input(payloads), payload_only=True, materialize_bytes=True)
        assert res.bytes_data is not None
        d.set_ragged_tile(TILE)
        t = Tables(items)
        cases = [(IR.Rule("b", t.t_half, 7, len(t.words)), t.v_half), (IR.Rule("b", None, 1000, 0), None),
                 (IR.Rule("c", t.t_tags, default=-1), t.v_tags)]
        for rows in (None, with_bad(BAD64, 200)):
            wants, _ = run_c(d, items, cases, rows)
            assert 0 < wants[0].matched < wants[0].total
    finally:
        if t:
            t.close()
        d.close()


N1 = 5000
C1_ITEMS = [{"id": [b"img-%08d" % i]} for i in range(N1)]


@pytest.mark.parametrize("mode", ["ends", "u32"])
def test_optimistic_decode_with_implicit_offsets_and_its_confirmation(mode):
    """A device-resident optimistic decode with u32 record ends: the ``id`` slot's bytes_off words are
    not stored (the column is poisoned before the decode), so every byte comes from the end-relative
    view. The first call comes directly after the decode, with no tfrg_result_info before it: the
    call confirms the decode itself."""
    fr = synth.framed(synth.c1_payloads(N1))
    d = IO.new_decoder(fr)
    words = [b"img-%08d" % i for i in range(0, N1, 3)] + [b"img-0000000", b"img-000000010"]
    table = {w: i for i, w in enumerate(words)}
    v = RawVocab(words, device=0)
    try:
        assert v.rc == 0
        run = IO.Run(d, *fr, mode)  # (no info, fetch or view before the calls)
        d.set_ragged_tile(TILE)
        cases = [(IR.Rule("id", table, 11, len(words)), v), (IR.Rule("id", None, 1 << 20, 0), None)]
        first, outs_first = run_c(d, C1_ITEMS, cases, None)
        assert 0 < first[0].matched < first[0].total == N1
        info = run.info()
        sid = slot_of(d, "id")
        assert int(info.implicit_off_slots) >> sid & 1 and int(info.implicit_off_slots) == 1 << sid and run.reruns() == 0
        rng = np.random.default_rng(4)
        run_c(d, C1_ITEMS, cases, rng.integers(0, N1, 2 * N1 + 3), N.ROWS_I32)
        run_c(d, C1_ITEMS, cases, [(N1 - 5 + k) % (N1 + 9) - 2 for k in range(333)], N.ROWS_I64)
        again, outs_again = run_c(d, C1_ITEMS, cases, None)  # after the confirmation: the same output
        for a, b in zip(outs_first, outs_again):
            assert bool((a.id_buf == b.id_buf).all()) and bool((a.ro_buf == b.ro_buf).all())
        fresh = IO.new_decoder(fr, optimistic="0")
        try:
            want = IO.Run(fresh, *fr, mode).fetch()
        finally:
            fresh.close()
        run.assert_raw(want, 1 << sid)  # (poison still: the calls neither read nor wrote the column)
    finally:
        v.close()
        d.close()


# ------------------------------------------------------------------------------------ 6. ragged_elems
def test_row_offsets_are_ragged_elems_byte_for_byte(main):
    import torch

    d, _, items, t = main
    for me, rows, rdt in ((0, None, N.ROWS_I64), (2, with_bad(BAD64, 327), N.ROWS_I64), (5, with_bad(BAD32, 130), N.ROWS_I32)):
        m = N_REC if rows is None else len(rows)
        rule = IR.Rule("b", t.t_half, 7, 0, max_elems=me or None)
        _, outs = run_c(d, items, [(rule, t.v_half)], rows, rdt)
        el = torch.full(((m + 1) * 8,), POISON, dtype=torch.uint8, device=dev())
        d_rows = None if rows is None else to_dev(rows, np.int64 if rdt == N.ROWS_I64 else np.int32)
        R.launch_elems(d, [(slot_of(d, "b"), me, 0, 0, 0, None, None, el.data_ptr())],
                       None if rows is None else (d_rows.data_ptr(), rdt), m, 0, None, None, None)
        torch.cuda.synchronize()
        assert bool((outs[0].ro_buf[GUARD:-GUARD] == el).all())


# ------------------------------------------------------------------------------------ 7. determinism
def test_two_equal_calls_write_equal_bytes(main):
    d, _, items, t = main
    rows = np.random.default_rng(5).integers(0, N_REC, 500)
    cases = [(IR.Rule("b", t.t_half, 1000, 0), t.v_half), (IR.Rule("c", None, 7, 0), None)]
    E = IR.expect(items, cases[0][0], rows).total
    bufs = []
    for _ in range(2):
        _, outs = run_c(d, items, cases, rows, caps=[E - 40, 5000])
        bufs.append([b.cpu().numpy() for o in outs for b in (o.id_buf, o.ro_buf)])
    for a, b in zip(*bufs):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------ 8. a large vocabulary
def test_100000_words_looked_up_by_50000_elements():
    rng = np.random.default_rng(6)
    words = [b"item-%07d" % i for i in range(100_000)]
    table = {w: i for i, w in enumerate(words)}
    draws = rng.integers(0, 140_000, 50_000)
    elems = [b"item-%07d" % i for i in draws]
    payloads, items = B.pack(elems, [10])
    d = new_decoder()
    v = RawVocab(words, device=0)
    try:
        assert v.rc == 0 and v.info()[:2] == (100_000, 262_144)
        res = d.decode(*payload_input(payloads), payload_only=True)
        assert len(res) == 5000
        for tile in (TILE, 0):
            d.set_ragged_tile(tile)
            wants, _ = run_c(d, items, [(IR.Rule("b", table, 1000, 100_000), v), (IR.Rule("b", table, default=-1), v)], None)
            assert wants[0].total == 50_000 and 0 < wants[0].matched < 50_000
    finally:
        v.close()
        d.close()


# ------------------------------------------------------------------------------------ 9. arguments
def test_refusals_leave_the_poison_and_empty_cases(main):
    import torch

    d, res, items, t = main
    lib = N.lib()
    fresh = new_decoder()
    host_only = RawVocab([b"q"])
    try:
        m = 3
        d_rows = to_dev([0, 1, 2])
        tot = torch.full((2,), -1, dtype=torch.int64, device=dev())
        st = torch.full((2, 4), 77, dtype=torch.int32, device=dev())
        outs = Outs(7, 16)
        s_b, s_n = slot_of(d, "b"), next(s for s in range(len(res.slot_key)) if res.slot_key[s] == "n")

        def call(dec=d, k=1, rows_ptr=d_rows.data_ptr(), rdt=N.ROWS_I64, m=m, ctx=True, **kw):
            f = dict(slot=s_b, max_elems=0, reserved0=0, reserved1=0, vocab=t.v_half.ptr.value, num_oov_buckets=0, oov_base=0,
                     default_id=-1, elem_cap=16, ids=outs.ids.data_ptr(), row_offsets=outs.ro.data_ptr())
            f.update(kw)
            arr = (N.TfrgIdsSpec * max(k, 1))(*[N.TfrgIdsSpec(**f) for _ in range(max(k, 1))])
            return lib.tfrg_result_elem_ids(dec._ctx if ctx else None, arr, k, C.c_void_p(rows_ptr) if rows_ptr else None,
                                            rdt, m, 0, C.c_void_p(tot.data_ptr()), C.c_void_p(st.data_ptr()), None)

        def refused(**bad) -> None:
            assert call(**bad) == -1, bad
            assert lib.tfrg_last_error().startswith(b"tfrg_result_elem_ids: "), bad
            torch.cuda.synchronize()
            outs.untouched()
            assert tot.cpu().tolist() == [-1, -1] and st.cpu().tolist() == [[77] * 4] * 2, bad

        refused(ctx=False)
        refused(dec=fresh)  # no result
        assert b"no result" in lib.tfrg_last_error()
        ro_ptr, id_ptr = outs.ro.data_ptr(), outs.ids.data_ptr()
        for bad in (dict(k=0), dict(k=N.IDS_MAX_SPECS + 1), dict(slot=len(res.slot_key)), dict(slot=s_n),
                    dict(row_offsets=None), dict(row_offsets=ro_ptr + 4), dict(ids=id_ptr + 4), dict(reserved0=1),
                    dict(reserved1=1), dict(vocab=None), dict(vocab=host_only.ptr.value), dict(rdt=2), dict(m=1 << 31),
                    dict(m=(1 << 32) - 1)):
            refused(**bad)
        if torch.cuda.device_count() > 1:  # a vocabulary on another device than the context's
            far = RawVocab([b"q"], device=1)
            try:
                refused(vocab=far.ptr.value)
            finally:
                far.close()
        # rows NULL: every record in order, rows_dtype ignored; m may differ from n
        assert call(rows_ptr=None, rdt=9, m=7) == 0
        torch.cuda.synchronize()
        outs.check(IR.expect(items, IR.Rule("b", t.t_half), list(range(7))))
        # m == 0: row_offsets[0] = 0, totals 0, no kernel
        outs = Outs(7, 16)
        tot.fill_(-1)
        assert call(m=0, rows_ptr=None) == 0
        torch.cuda.synchronize()
        assert outs.ro.cpu().tolist()[0] == 0 and bool((outs.ro_buf[GUARD + 8 :] == POISON).all())
        assert bool((outs.id_buf == POISON).all()) and tot.cpu().tolist()[0] == 0 and st.cpu().tolist()[0] == [0] * 4
        # n == 0: every row is skipped
        buf, s0, e0 = payload_input(main_batch()[0])
        assert len(fresh.decode(buf[: int(e0[4])], s0[:5], e0[:5], payload_only=True)) == 5  # (the keys get their slots)
        assert len(fresh.decode(buf[:0], s0[:0], e0[:0], payload_only=True)) == 0
        assert slot_of(fresh, "b") is not None
        outs = Outs(3, 16)
        tot.fill_(-1)
        assert call(dec=fresh, slot=slot_of(fresh, "b")) == 0
        torch.cuda.synchronize()
        assert outs.ro.cpu().tolist() == [0, 0, 0, 0] and bool((outs.id_buf == POISON).all())
        assert tot.cpu().tolist()[0] == 0 and st.cpu().tolist()[0] == [0, 0, 0, 3]
    finally:
        host_only.close()
        fresh.close()


# ------------------------------------------------------------------------------------ 10. Python
def test_python_device_path_against_the_numpy_path(main):
    import torch

    d, res, items, t = main
    vocab = I.Vocabulary(t.words, device=0)
    tags = I.Vocabulary(t.tags, t.neg_ids[: len(t.tags)], device=0)
    host_only = I.Vocabulary(t.tags)
    try:
        assert vocab.info["device_bytes"] > 0 and vocab.info["max_probe"] == t.model.max_probe
        specs = [I.ElementIds("b", vocab, num_oov_buckets=7), I.ElementIds("b", num_oov_buckets=1000, name="hash"),
                 I.ElementIds("c", tags, default_id=-77, max_elems=2, name="tags"), I.ElementIds("zz", vocab, name="absent")]
        rules = [IR.Rule("b", t.t_half, 7, len(t.words)), IR.Rule("b", None, 1000, 0),
                 IR.Rule("c", dict(zip(t.tags, t.neg_ids)), default=-77, max_elems=2), IR.Rule("zz", t.t_half)]
        rows = np.random.default_rng(7).integers(0, N_REC, 300)
        for r in (None, rows):
            host = res.element_ids(specs, rows=r)
            got = d.element_ids(specs, rows=None if r is None else to_dev(r))  # no capacity: exact tensors
            m = N_REC if r is None else len(r)
            for sp, rule in zip(specs, rules):
                k = sp.out_name
                want = IR.expect(items, rule, r)
                ids, ro = got[k]
                assert ids.numel() == want.total == got.capacity[k] and ro.numel() == m + 1, k
                assert np.array_equal(ids.cpu().numpy(), host[k][0]) and np.array_equal(ro.cpu().numpy(), host[k][1]), k
                assert np.array_equal(host[k][0], want.ids) and np.array_equal(host[k][1], want.row_offsets), k
                assert got.totals[k] == host.totals[k] == want.total and not got.overflowed[k], k
                assert got.stats[k].tolist() == host.stats[k].tolist() == want.stats, k
        # capacity=: no read-back before the call returns; an overflow keeps the prefix
        want = IR.expect(items, rules[0], rows)
        E = want.total
        for cap, over in ((E + 10, False), ({"b": E - 1, "hash": E, "tags": 10_000, "absent": 0}, True)):
            got = d.element_ids(specs, rows=to_dev(rows), capacity=cap)
            c = cap["b"] if isinstance(cap, dict) else cap
            ids, ro = got["b"]
            assert ids.numel() == c and got.overflowed["b"] == over and got.totals["b"] == E
            assert np.array_equal(ids.cpu().numpy()[: min(c, E)], want.ids[: min(c, E)]) and np.array_equal(ro.cpu().numpy(), want.row_offsets)
        # out=
        out = {"b": (torch.empty(E, dtype=torch.int64, device=dev()), torch.empty(len(rows) + 1, dtype=torch.int64, device=dev()))}
        got = d.element_ids(specs[:1], rows=to_dev(rows), out=out)
        assert got["b"][0] is out["b"][0] and np.array_equal(out["b"][0].cpu().numpy(), want.ids)
        for bad in ((out["b"][0].to(torch.int32), out["b"][1]), (out["b"][0], out["b"][1][:-1]), (out["b"][0].cpu(), out["b"][1])):
            with pytest.raises(ValueError):
                d.element_ids(specs[:1], rows=to_dev(rows), out={"b": bad})
        for bad in (-1, 1.5, (1, 2), "ab"):
            with pytest.raises(ValueError):
                d.element_ids(specs[:1], capacity=bad)
        with pytest.raises(ValueError, match="device"):
            d.element_ids([I.ElementIds("c", host_only)])
    finally:
        for v in (vocab, tags, host_only):
            v.close()


def test_python_absent_key_over_a_list_with_entries_out_of_range(main):
    """An absent key beside a present one, over a device row list with -1 and n in it: the absent key's
    rows are empty or skipped like the present one's, without a launch for it, and offsets the caller
    provides for it are zeroed."""
    import torch

    d, _, items, t = main
    vocab = I.Vocabulary(t.words, device=0)
    try:
        rows = [0, N_REC, -1, 5, I64_MAX, 3, 3]
        specs = [I.ElementIds("zz", vocab, name="absent"), I.ElementIds("b", vocab, num_oov_buckets=7)]
        want = IR.expect(items, IR.Rule("b", t.t_half, 7, len(t.words)), rows)
        assert want.stats[3] == 3 and want.total > 0
        got = d.element_ids(specs, rows=to_dev(rows))
        assert got["absent"][0].numel() == 0 and got["absent"][1].cpu().tolist() == [0] * 8
        assert got.stats["absent"].tolist() == [0, 0, 4, 3] and got.totals["absent"] == 0 and not got.overflowed["absent"]
        assert np.array_equal(got["b"][0].cpu().numpy(), want.ids) and np.array_equal(got["b"][1].cpu().numpy(), want.row_offsets)
        assert got.stats["b"].tolist() == want.stats and got.totals["b"] == want.total
        out = {"absent": (torch.full((4,), -1, dtype=torch.int64, device=dev()), torch.full((8,), -1, dtype=torch.int64, device=dev()))}
        got = d.element_ids(specs, rows=to_dev(rows), out=out)
        assert out["absent"][1].cpu().tolist() == [0] * 8 and out["absent"][0].cpu().tolist() == [-1] * 4
        assert got.capacity["absent"] == 4 and np.array_equal(got["b"][0].cpu().numpy(), want.ids)
    finally:
        vocab.close()


def test_python_path_over_a_decode_of_no_records():
    """No record: every row of a device list is skipped, nothing is launched, all offsets are 0."""
    fresh = new_decoder()
    vocab = I.Vocabulary([b"q"], device=0)
    try:
        buf, s0, e0 = payload_input(main_batch()[0])
        assert len(fresh.decode(buf[: int(e0[4])], s0[:5], e0[:5], payload_only=True)) == 5  # (the keys get their slots)
        assert len(fresh.decode(buf[:0], s0[:0], e0[:0], payload_only=True)) == 0
        got = fresh.element_ids([I.ElementIds("b", vocab)], rows=to_dev([0, 5]))
        assert got["b"][0].numel() == 0 and got["b"][1].cpu().tolist() == [0, 0, 0]
        assert got.stats["b"].tolist() == [0, 0, 0, 2] and got.totals["b"] == 0 and not got.overflowed["b"]
    finally:
        vocab.close()
        fresh.close()
