"""TFRG_FLAG_MATERIALIZE_BYTES (k_bytes_scan / k_bytes_copy, csrc/tfrg_bytes.hip) against a host
reference built from the generator's own items (tests/_bytes_ref.py): which element lands where, and
every byte of it. Bytes and integers compare exactly.

The shapes sit on the kernels' boundaries -- the scan tile (kBsTile = 4096 elements), the long
element threshold (kBigElem = 128 bytes), the 64-element copy groups, every destination (0..15) and
source (0..3) alignment of the wave copy, and an element that ends on the input's last byte -- and
each test states, from its own construction, that it reaches them."""

import ctypes
import functools

import numpy as np
import pytest

from tests import _bytes_ref as R
from tests.golden.gen_golden import entry, i64
from tfr_reader import _native as N
from tfr_reader import dense as D
from tfr_reader import hip, synth, writer

pytestmark = pytest.mark.gpu

TILE = 4096  # kBsTile: elements per scan tile
BIG = 128    # kBigElem: longer elements are copied one wave each


@pytest.fixture
def dec():
    d = hip.HipDecoder(0)
    yield d
    d.close()


def _want(res: hip.BatchResult, items) -> R.Expected:
    return R.expected(items, res.slot_key, res.slot_kind, res.slot_base, res.row_splits)


def _check(res: hip.BatchResult, items) -> R.Expected:
    """The four assertions every case makes: offsets, data, bytes_data_len and the element count."""
    assert res.bytes_data is not None and not res.status.any()
    want = _want(res, items)
    diff = R.first_difference(res.bytes_offsets, res.bytes_data, want, res.bytes_off)
    assert diff is None, diff
    assert int(res.info.bytes_data_len) == int(want.offsets[-1])
    assert int(res.info.kind_totals[1]) == want.lengths.size
    return want


def _dev_copy(ptr, count: int, dt) -> np.ndarray:
    rt = ctypes.CDLL("libamdhip64.so")
    host = np.zeros(count, dt)
    if count:
        p = ctypes.cast(ptr, ctypes.c_void_p).value
        assert rt.hipMemcpy(ctypes.c_void_p(host.ctypes.data), ctypes.c_void_p(p), ctypes.c_size_t(host.nbytes), 2) == 0
    return host


def _upload(buf, st, en):
    import torch

    dev = torch.device("cuda", 0)
    d_b = torch.zeros(buf.size + 32, dtype=torch.uint8, device=dev)
    d_b[: buf.size].copy_(torch.from_numpy(np.array(buf)))  # (a writable copy: torch warns about read-only arrays)
    d_s = torch.from_numpy(st.view(np.int64)).to(dev)
    d_e = torch.from_numpy(en.view(np.int64)).to(dev)
    torch.cuda.synchronize(dev)
    return d_b, d_s, d_e


def test_shapes_follow_the_kernel_constants():
    """The shapes below are placed by these two numbers: a retune must fail here, not quietly move
    the cases off the boundaries."""
    assert R.kernel_constants() == {"tile": TILE, "big": BIG}


# ---------------------------------------------------------------------------------- 1. scan tiles
SCAN_NB = [0, 1, 4095, 4096, 4097, 8192, 3 * 4096 + 5, 64 * 4096 + 1]


def _tiles(nb: int) -> int:
    return nb // TILE + 1  # the tiles cover offsets[0..nb]: nb + 1 entries


def test_scan_cases_reach_the_tile_counts():
    assert [_tiles(nb) for nb in SCAN_NB] == [1, 1, 1, 2, 2, 3, 4, 65]


@functools.lru_cache(maxsize=None)
def _one_byte_batch(nb: int):
    """nb one-byte elements of one slot, 64 per record."""
    blob = np.random.default_rng(nb + 1).integers(0, 256, nb + 1, dtype=np.uint8).tobytes()
    payloads, items = R.pack([blob[j : j + 1] for j in range(nb)], [64])
    return synth.framed(payloads), items


@pytest.mark.parametrize("nb", SCAN_NB)
def test_scan_tiles(dec, nb):
    (buf, st, en), items = _one_byte_batch(nb)
    want = _check(dec.decode(buf, st, en, materialize_bytes=True), items)
    assert want.lengths.size == nb and int(want.offsets[-1]) == nb


def test_scan_slot_boundaries_inside_tiles(dec):
    """Three bytes slots of 3,000, 2,500 and 1,000 elements: their boundaries (3,000 and 5,500) fall
    inside the first and the second tile."""
    per = {b"a": 30, b"b": 25, b"c": 10}
    elems = {k: R.random_elems([(7 * j + m) % 6 for j in range(100 * m)], seed=m) for k, m in per.items()}
    payloads, items = [], []
    for r in range(100):
        p, it = R.record({k: elems[k][r * m : (r + 1) * m] for k, m in per.items()})
        payloads.append(p)
        items.append(it)
    buf, st, en = synth.framed(payloads)
    res = dec.decode(buf, st, en, materialize_bytes=True)
    want = _check(res, items)
    assert want.lengths.size == 6500
    bases = sorted(int(res.slot_base[s]) for s in range(len(res.slot_kind)) if res.slot_kind[s] == 1)
    assert bases == [0, 3000, 5500] and [b // TILE for b in bases] == [0, 0, 1]


def test_scan_empty_elements_across_the_tile_edge(dec):
    lengths = np.ones(4200, np.int64)
    lengths[[4095, 4096]] = 0
    payloads, items = R.pack(R.random_elems(lengths, seed=3), [64])
    buf, st, en = synth.framed(payloads)
    want = _check(dec.decode(buf, st, en, materialize_bytes=True), items)
    assert want.lengths[4094:4098].tolist() == [1, 0, 0, 1]


# ------------------------------------------------------------- 2. long elements, every alignment
LONG_LENGTHS = [129, 130, 143, 144, 145, 160, 1039, 1040, 1041, 1168, 5000]


@functools.lru_cache(maxsize=None)
def _alignment_batch():
    """One record per (length, d, s): a pad element that brings the column to ``d`` mod 16, then the
    long element, whose address in the framed batch is ``s`` mod 4 (by the length of the first key).
    Returns the framed batch, its items and the (length, dst & 15, src & 3) of every long element."""
    rng = np.random.default_rng(2)
    payloads, items, triples = [], [], []
    run = pos = 0  # bytes of the column, and of the framed batch, before this record
    for ln in LONG_LENGTHS:
        for d in range(16):
            for s in range(4):
                pad, big = rng.bytes((d - run) % 16), rng.bytes(ln)
                for kp in range(4):
                    p, it = R.record({b"b": [pad, big]}, entry(b"n" + b"x" * kp, i64(1)))
                    src = pos + 12 + len(p) - ln  # the long element is the payload's last bytes
                    if src % 4 == s:
                        break
                else:
                    raise AssertionError((ln, d, s))
                assert p.endswith(big)
                triples.append((ln, (run + len(pad)) % 16, src % 4))
                payloads.append(p)
                items.append(it)
                run += len(pad) + ln
                pos += len(p) + 16
    return synth.framed(payloads), items, triples


def test_alignment_batch_reaches_every_triple():
    _, items, triples = _alignment_batch()
    assert len(items) == 704 and len(set(triples)) == 704
    assert set(triples) == {(ln, d, s) for ln in LONG_LENGTHS for d in range(16) for s in range(4)}
    # 64 or more 16-byte body pieces behind a head: the wave copy's second loop iteration
    assert all((ln - 15) // 16 >= 64 for ln in (1039, 1040, 1041, 1168))


@pytest.mark.parametrize("lane_max", [hip.DEFAULT_LANE_MAX, 0])
def test_long_elements_at_every_alignment(dec, lane_max):
    (buf, st, en), items, triples = _alignment_batch()
    dec.set_lane_max(lane_max)
    res = dec.decode(buf, st, en, materialize_bytes=True)
    want = _check(res, items)
    # the column is where the construction put it (base pointers are 16-byte aligned allocations)
    big = np.flatnonzero(want.lengths > BIG)
    assert [(int(want.lengths[e]), int(want.offsets[e]) & 15, int(res.bytes_off[e]) & 3) for e in big] == triples


# ------------------------------------------------------------------------------ 3. short elements
SHORT_TOTALS = [0, 1, 63, 64, 65, 127, 128, 64 * 128]


def _short_groups() -> list[list[int]]:
    longs = [129, 200, 1041, 130]
    mixed = []
    for j in range(32):  # long and short elements interleaved: the short ones sum to 127
        mixed += [longs[j % 4], 4 if j < 31 else 3]
    return [
        [0] * 64,                                                      # T = 0
        [1] + [0] * 63,                                                # T = 1: only the first element
        [0] * 63 + [63],                                               # T = 63: only the last element
        [0, 20, 0, 0, 20] + [0] * 31 + [24] + [0] * 27,                # T = 64: runs of 1, 2, 31 empties
        [2] + [1] * 63,                                                # T = 65
        mixed,                                                         # T = 127
        [128, 129] + [0] * 62,                                         # T = 128: 128 next to 129
        [128] * 64,                                                    # T = 64 * 128
        [129, 128] * 32,                                               # every other lane long
        [(5 * j) % 131 for j in range(64)],                            # mixed lengths 0..130
    ]


def _group_totals(lengths) -> list[int]:
    lengths = np.asarray(lengths, np.int64)
    full = lengths[: lengths.size // 64 * 64].reshape(-1, 64)
    return np.where(full <= BIG, full, 0).sum(axis=1).tolist()


@functools.lru_cache(maxsize=None)
def _short_batch(tail: int, per_record: tuple):
    lengths = [x for g in _short_groups() for x in g] + [(7 * j + 1) % 130 for j in range(tail)]
    payloads, items = R.pack(R.random_elems(lengths, seed=40 + tail), list(per_record))
    return synth.framed(payloads), items, lengths


def test_short_groups_reach_every_total():
    groups = _short_groups()
    assert all(len(g) == 64 for g in groups)
    assert _group_totals([x for g in groups for x in g])[:8] == SHORT_TOTALS
    g = groups[3]
    assert [i for i, x in enumerate(g) if x] == [1, 4, 36]  # 1, 2 and 31 empties before them


@pytest.mark.parametrize("tail,per_record", [(1, (64,)), (63, (64,)), (1, (40, 88, 7)), (63, (100,))])
def test_short_element_groups(dec, tail, per_record):
    """Groups of 64 elements, one per record or spanning records, with a ragged last group."""
    (buf, st, en), items, lengths = _short_batch(tail, per_record)
    want = _check(dec.decode(buf, st, en, materialize_bytes=True), items)
    assert want.lengths.tolist() == lengths and want.lengths.size % 64 == tail
    assert _group_totals(want.lengths)[:8] == SHORT_TOTALS


# --------------------------------------------------------------------------- 4. end of the input
@pytest.mark.parametrize("last", [1, 3, 128, 129, 145, 1040])
def test_element_ends_on_the_last_input_byte(dec, last):
    """Bare payloads from host memory: the last record's last entry is the bytes element, so it ends
    on byte nbytes - 1, at nbytes % 16 in {0, 1, 13, 14, 15}. tfrg_decode_host uploads into a buffer
    of round_up(nbytes, 16) + 16 bytes, zero past nbytes: readable as include/tfrg.h asks."""
    elem = R.random_elems([last], seed=last)[0]
    tail, tail_items = R.record({b"b": [elem]})
    seen = set()
    for k in range(16):
        head, head_items = R.record({b"b": [b"y" * k]}, entry(b"n", i64(k)))
        nbytes = len(head) + len(tail)
        if nbytes % 16 not in (0, 1, 13, 14, 15):
            continue
        seen.add(nbytes % 16)
        buf = np.frombuffer(head + tail, np.uint8)
        st = np.array([0, len(head)], np.uint64)
        en = np.array([len(head), nbytes], np.uint64)
        res = dec.decode(buf, st, en, payload_only=True, materialize_bytes=True)
        want = _check(res, [head_items, tail_items])
        assert want.elems[-1] == elem and int(res.bytes_off[-1]) + last == nbytes == buf.size
    assert seen == {0, 1, 13, 14, 15}


# ---------------------------------------------------------------------- 5. device-resident decode
def test_device_resident_decode(dec):
    (buf, st, en), items = _one_byte_batch(3 * 4096 + 5)
    dec.decode(buf, st, en)  # (learns the keys)
    d_b, d_s, d_e = _upload(buf, st, en)
    n = st.shape[0]
    dec.decode_device(d_b.data_ptr(), buf.size, d_s.data_ptr(), d_e.data_ptr(), n, materialize_bytes=True)
    info = dec.info()
    cols = dec.device_columns()
    S = int(info.n_slots)
    kt = dec.keys
    want = R.expected(items, [kt.key_str[k] for k in kt.slot_key[:S]], kt.slot_kind[:S],
                      _dev_copy(cols.slot_base, S, np.uint64),
                      _dev_copy(cols.row_splits, S * (n + 1), np.uint32).reshape(S, n + 1))
    nb = int(info.kind_totals[1])
    assert nb == want.lengths.size == 3 * 4096 + 5
    offs = _dev_copy(cols.bytes_offsets, nb + 1, np.uint64)
    data = _dev_copy(cols.bytes_data, int(want.offsets[-1]), np.uint8)
    diff = R.first_difference(offs, data, want, _dev_copy(cols.bytes_off, nb, np.uint32))
    assert diff is None, diff
    assert int(info.bytes_data_len) == int(want.offsets[-1])


# ------------------------------------------------------------------------- 6. optimistic decode
def _c1_items(ids) -> list[dict]:
    return [{"id": [b"img-%08d" % i]} for i in ids]


def test_optimistic_decode_materializes_after_its_confirmation(monkeypatch):
    monkeypatch.setenv("TFRG_OPTIMISTIC", "1")  # (read at context creation; the suite may run with 0)
    on = hip.HipDecoder(0)
    try:
        buf, st, en = synth.framed(synth.c1_payloads(3000))
        on.decode(buf, st, en)  # (learns the record shapes)
        buf, st, en = synth.framed(synth.c1_payloads(5000, offset=11))
        res = on.decode(buf, st, en, materialize_bytes=True)
        assert on.device_bytes()[1] == 0  # not re-run: the gather was launched by the confirmation
        assert int(res.info.tpl_groups_missed) == 0
        want = _check(res, _c1_items(range(11, 5011)))
        assert want.lengths.size == 5000 > TILE
        # one record no template takes: re-run in full, gathered from the ordinary place
        pl = synth.c1_payloads(5000, offset=23)
        pl[4321] = writer.encode_example([("label", "int64_list", [100000]), ("id", "bytes_list", [b"img-%08d" % 4344])])
        buf, st, en = synth.framed(pl)
        res = on.decode(buf, st, en, materialize_bytes=True)
        assert on.device_bytes()[1] == 1
        _check(res, _c1_items(range(23, 5023)))
    finally:
        on.close()


# ----------------------------------------------------------------------------- 7. capacity paths
def test_small_bytes_hint_is_rerun_at_the_worst_case(dec):
    lengths = [(11 * j) % 140 for j in range(5000)]
    payloads, items = R.pack(R.random_elems(lengths, seed=7), [50])
    buf, st, en = synth.framed(payloads)
    dec.set_value_caps(0, 0, 100)  # far below the batch's 5,000 elements
    res = dec.decode(buf, st, en, materialize_bytes=True)
    assert dec.device_bytes()[1] >= 1
    want = _check(res, items)
    assert want.lengths.size == 5000
    dec.set_value_caps(0, 0, 5000)  # exact: no re-run
    before = dec.device_bytes()[1]
    res = dec.decode(buf, st, en, materialize_bytes=True)
    assert dec.device_bytes()[1] == before
    _check(res, items)


def test_repeated_host_ranges(dec):
    """Records selected with replacement from host memory: the column is sized from the ranges."""
    recs = [R.record({b"b": [e]}, entry(b"n", i64(k))) for k, e in enumerate(R.random_elems([5, 129, 3000], seed=8))]
    buf, st, en = synth.framed([p for p, _ in recs])
    reps = np.random.default_rng(9).permutation(np.tile(np.arange(3), 40))
    res = dec.decode(buf, st[reps], en[reps], materialize_bytes=True)
    want = _check(res, [recs[i][1] for i in reps.tolist()])
    assert want.lengths.size == 120 and int(want.offsets[-1]) == 40 * 3134 > buf.size


def test_overlapping_device_ranges_report_the_data_overflow(dec):
    """One record with a 3,000-byte element selected 50 times on the device path: the 50 elements fit
    the offsets, the 150,000 gathered bytes do not fit the data column (input bytes + 16). The copy
    kernel returns before any store and the decode reports the overflow; the context stays usable."""
    import torch

    p, it = R.record({b"b": R.random_elems([3000], seed=10)})
    buf, st, en = synth.framed([p])
    dev = torch.device("cuda", 0)
    d_buf = torch.zeros(buf.size + 32, dtype=torch.uint8, device=dev)
    d_buf[: buf.size].copy_(torch.from_numpy(np.array(buf)))  # (a writable copy: torch warns about read-only arrays)
    reps = np.zeros(50, np.int64)
    d_st = torch.from_numpy(st[reps].view(np.int64)).to(dev)
    d_en = torch.from_numpy(en[reps].view(np.int64)).to(dev)
    _check(dec.decode(buf, st, en, materialize_bytes=True), [it])  # (learns the key)
    assert 50 <= buf.size // 2 + 16 and 50 * 3000 > buf.size + 16
    torch.cuda.synchronize(dev)
    dec.decode_device(d_buf.data_ptr(), buf.size, d_st.data_ptr(), d_en.data_ptr(), 50, materialize_bytes=True)
    with pytest.raises(N.NativeError, match="overflow"):
        dec.info()
    torch.cuda.synchronize(dev)
    _check(dec.decode(buf, st, en, materialize_bytes=True), [it])


# ---------------------------------------------------------- 8. dense from the materialized column
def test_dense_reads_the_materialized_column(dec):
    from tests.test_dense_gpu import same

    rng = np.random.default_rng(11)
    counts = rng.integers(0, 3, 300)
    lengths = rng.choice([0, 1, 3, 4, 5, 16, 129], int(counts.sum()))
    elems = R.random_elems(lengths, seed=12)
    payloads, items, at = [], [], 0
    for r in range(300):
        p, it = R.record({b"names": elems[at : at + counts[r]]}, entry(b"n", i64(r)))
        payloads.append(p)
        items.append(it)
        at += int(counts[r])
    assert set(counts.tolist()) == {0, 1, 2} and set(lengths.tolist()) == {0, 1, 3, 4, 5, 16, 129}
    buf, st, en = synth.framed(payloads)
    specs = [D.Dense("names", "uint8", w, fill=0xEE, lengths=True, name=f"w{w}") for w in (1, 3, 4, 7, 16, 130)]
    views = dec.decode(buf, st, en)
    want = _want(views, items)
    ref = D.densify(specs, n=300, slot_key=views.slot_key, slot_kind=views.slot_kind, row_splits=views.row_splits,
                    slot_base=views.slot_base, i64=views.i64, f32=views.f32, bytes_data=want.data,
                    bytes_offsets=want.offsets)
    same(dec.dense(specs), ref, specs)
    mat = dec.decode(buf, st, en, materialize_bytes=True)
    _check(mat, items)
    same(dec.dense(specs), ref, specs)
    assert int(ref.stats["w1"][3]) == int((counts == 2).sum()) > 0 and int(ref.stats["w130"][0]) == 0


# --------------------------------------------------------------------------------------- 9. fetch
def _check_fetch(res: hip.BatchResult, items) -> None:
    for i in range(0, len(items), 7):
        f = res.feature(i)
        for key, its in items[i].items():
            s = [k for k in range(len(res.slot_key)) if res.slot_key[k] == key and res.slot_kind[k] == 1][0]
            assert res.slot_values(s, i) == its, (i, key)
            assert f[key].value == its, (i, key)


def test_fetch_slices_the_materialized_column(dec):
    (buf, st, en), items, _ = _alignment_batch()
    _check_fetch(dec.decode(buf, st, en, materialize_bytes=True), items)
    (buf, st, en), items, _ = _short_batch(63, (100,))
    res = dec.decode(buf, st, en, materialize_bytes=True)
    assert res.bytes_data is not None
    _check_fetch(res, items)
