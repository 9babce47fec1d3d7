"""k_tpl_lane's staged windows and packed CRC tables: a group of 64 records whose ends do not
decrease, lie in the batch and span at most the wave's stage is read as one span through LDS; any
other group, and every group with TFRG_TPL_STAGE=0, takes the per-lane window loads (as do batches
too small to be bound by bandwidth, unless TFRG_TPL_STAGE=2 stages them too). Both must give
the same columns, info words and re-runs on every input, and the oracle's values record by record.

Inputs are the smallest that reach every path: several groups per wave and a ragged last group,
the three offset modes, a batch starting at byte 0 (records ending before byte 64) and a record-range
cut of a larger image, groups the stage must refuse (permuted records, gaps, one large record),
corrupted bytes at the first, middle and last lane of the first and last group, the 16-template
variable-id shape (whichever variant the LDS budget selects), a W = 32 shape whose CRC runs the
chain beside packed tables, and empty / single-record batches.
"""

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gpu_parity import _compare_to_oracle
from tfr_reader import hip, synth, writer

pytestmark = pytest.mark.gpu

COLS = ("status", "verdict", "order", "row_splits", "i64", "f32", "bytes_off", "bytes_len", "slot_base")
INFO = ("n_records", "n_slots", "n_errors", "first_error", "n_miss_records", "n_miss_entries", "n_big",
        "tpl_groups_missed", "implicit_cols", "placed_slots")
N = 5003  # 78 whole groups and one of 11 records


@pytest.fixture(scope="module")
def orc():
    return O.Oracle()


@pytest.fixture(scope="module")
def c1():
    """C1 records whose labels cross 127 / 128 in most groups (58- and 59-byte records mixed)."""
    blob, offs = synth.c1_blob(N, 100, 7)
    buf = synth.frame_blob(blob, offs)
    ends = (offs[1:] + 16 * np.arange(1, N + 1)).astype(np.uint64)
    starts = np.concatenate([[0], ends[:-1]]).astype(np.uint64)
    assert int(ends[-1]) == buf.size and len(set((ends - starts).tolist())) == 2
    return buf, starts, ends


def _pair(monkeypatch, sample):
    """Two fresh contexts that learned the same sample: staged windows on batches of any size, and
    forced off."""
    monkeypatch.setenv("TFRG_OPTIMISTIC", "1")  # (read at context creation, as TFRG_TPL_STAGE)
    monkeypatch.setenv("TFRG_TPL_STAGE", "2")
    on = hip.HipDecoder(0)
    monkeypatch.setenv("TFRG_TPL_STAGE", "0")
    off = hip.HipDecoder(0)
    for d in (on, off):
        d.decode(*sample)
        assert d.template_count() >= 1
    return on, off


def _device(dec, buf, st, en, mode, first=0, count=None):
    """One device-resident decode of records [first, first + count) through `mode` offsets."""
    import torch

    dev = torch.device("cuda", 0)
    n = len(st) - first if count is None else count
    st, en = np.ascontiguousarray(st[first : first + n]), np.ascontiguousarray(en[first : first + n])
    d_b = torch.zeros(buf.size + 32, dtype=torch.uint8, device=dev)
    d_b[: buf.size].copy_(torch.from_numpy(buf.copy()))
    if mode == "u64":
        d_s = torch.from_numpy(st.astype(np.int64)).to(dev)
        d_e = torch.from_numpy(en.astype(np.int64)).to(dev)
    else:
        d_s = torch.from_numpy(st.astype(np.uint32).view(np.int32)).to(dev)
        d_e = torch.from_numpy(en.astype(np.uint32).view(np.int32)).to(dev)
    torch.cuda.synchronize(dev)
    dec.set_record_bound(int((en - st).max()) if n else 16)
    before = dec.device_bytes()[1]
    if mode == "u64":
        dec.decode_device(d_b.data_ptr(), buf.size, d_s.data_ptr(), d_e.data_ptr(), n)
    else:
        dec.decode_device32(d_b.data_ptr(), buf.size, d_s.data_ptr() if mode == "u32" else None, d_e.data_ptr(),
                            int(st[0]) if n else 0, n)
    info = dec.info()  # (confirms an optimistic decode: re-runs it when a record took no template)
    r = dec._fetch(buf, st, en, info, False)
    torch.cuda.synchronize(dev)
    return r, dec.device_bytes()[1] - before


def _both(pair, buf, st, en, mode, **kw):
    (a, ra), (b, rb) = (_device(d, buf, st, en, mode, **kw) for d in pair)
    for k in COLS:
        assert np.array_equal(np.array(getattr(a, k)), np.array(getattr(b, k))), k
    for k in INFO:
        assert int(getattr(a.info, k)) == int(getattr(b.info, k)), k
    assert list(a.info.kind_totals) == list(b.info.kind_totals)
    assert ra == rb
    return a, ra


def _oracle(r, orc, buf, idx):
    bad = _compare_to_oracle(r, orc, buf, r.starts, r.ends, idx=idx)
    assert not bad, bad


@pytest.mark.parametrize("mode", ["ends", "u32", "u64"])
def test_offset_modes_from_byte_0(monkeypatch, orc, c1, mode):
    buf, st, en = c1
    pair = _pair(monkeypatch, c1)
    try:
        r, reruns = _both(pair, buf, st, en, mode)
        assert reruns == 0 and int(r.info.implicit_cols) == 7 and not np.array(r.status).any()
        _oracle(r, orc, buf, list(range(0, 130)) + list(range(130, N, 61)) + list(range(N - 70, N)))
    finally:
        for d in pair:
            d.close()


def test_record_range_cut_of_a_larger_image(monkeypatch, orc, c1):
    buf, st, en = c1
    pair = _pair(monkeypatch, c1)
    try:
        for mode in ("ends", "u32"):
            r, reruns = _both(pair, buf, st, en, mode, first=1001, count=3500)
            assert reruns == 0 and len(r) == 3500
            _oracle(r, orc, buf, list(range(0, 70)) + list(range(70, 3500, 53)) + list(range(3430, 3500)))
    finally:
        for d in pair:
            d.close()


def test_groups_the_stage_refuses(monkeypatch, orc, c1):
    buf, st, en = c1
    pair = _pair(monkeypatch, c1)
    try:
        # the records of group 10 in reverse order, and two records of group 20 swapped (u32 pairs)
        p = np.arange(N)
        p[640:704] = p[640:704][::-1]
        p[[1290, 1300]] = p[[1300, 1290]]
        r, reruns = _both(pair, buf, st[p], en[p], "u32")
        assert reruns == 0
        _oracle(r, orc, buf, list(range(560, 780)) + list(range(1270, 1350)))
        # a few bytes between some records (5 bytes after every 50th, 200 after record 2000)
        parts, gst, gen, pos = [], [], [], 0
        for i in range(N):
            rec = buf[int(st[i]) : int(en[i])]
            gst.append(pos)
            pos += rec.size
            gen.append(pos)
            parts.append(rec)
            pad = 200 if i == 2000 else 5 if i % 50 == 49 else 0
            if pad:
                parts.append(np.full(pad, 0xA5, np.uint8))
                pos += pad
        gbuf = np.concatenate(parts)
        gst, gen = np.array(gst, np.uint64), np.array(gen, np.uint64)
        for mode in ("u32", "u64"):
            r, reruns = _both(pair, gbuf, gst, gen, mode)
            assert reruns == 0 and not np.array(r.status).any()
            _oracle(r, orc, gbuf, list(range(0, 130)) + list(range(1960, 2100)) + list(range(N - 70, N)))
        # one 5,000-byte record in the middle of a group: no template takes it; it goes to the
        # general passes, with the stage and without
        pl = synth.c1_payloads(3000, offset=90)
        pl[1000] = writer.encode_example([("label", "int64_list", [5]), ("id", "bytes_list", [b"x" * 4950])])
        bbuf, bst, ben = synth.framed(pl)
        assert int(ben[1000] - bst[1000]) > 4900
        for mode in ("ends", "u32"):
            r, reruns = _both(pair, bbuf, bst, ben, mode)
            assert not np.array(r.status).any()  # (re-runs: equal, _both)
            _oracle(r, orc, bbuf, list(range(930, 1100)) + list(range(0, 3000, 101)))
    finally:
        for d in pair:
            d.close()


def test_corrupted_bytes_at_lane_and_group_edges(monkeypatch, orc, c1):
    buf, st, en = c1
    pair = _pair(monkeypatch, c1)
    last = (N - 1) // 64 * 64
    try:
        for what in ("id digit", "label byte", "stored crc"):
            bad = buf.copy()
            hit = [0, 31, 63, last, last + 5, N - 1, 64 * 40 + 31]
            for i in hit:
                s, e = int(st[i]), int(en[i])
                at = e - 7 if what == "id digit" else s + 12 + 17 if what == "label byte" else e - 1
                bad[at] ^= 0x01
            r, reruns = _both(pair, bad, st, en, "ends")
            assert reruns == 1  # (a record no template took: the full decode, which keeps its values)
            v = np.array(r.verdict)
            assert sorted(np.flatnonzero(v != 7).tolist()) == sorted(hit) and (v[hit] == 3).all()
            _oracle(r, orc, bad, list(range(0, 130)) + hit + list(range(last - 64, N)))
    finally:
        for d in pair:
            d.close()


def test_variable_length_ids_16_templates(monkeypatch, orc):
    blob, offs = synth.c1v_blob(5000, 0, 11)
    buf = synth.frame_blob(blob, offs)
    en = (offs[1:] + 16 * np.arange(1, 5001)).astype(np.uint64)
    st = np.concatenate([[0], en[:-1]]).astype(np.uint64)
    pair = _pair(monkeypatch, (buf, st, en))
    try:
        assert pair[0].template_count() == 16
        for mode in ("ends", "u64"):
            r, reruns = _both(pair, buf, st, en, mode)
            assert reruns == 0 and not np.array(r.status).any()
            _oracle(r, orc, buf, list(range(0, 130)) + list(range(130, 5000, 67)))
    finally:
        for d in pair:
            d.close()


def test_w32_chain_beside_packed_tables(monkeypatch, orc):
    """Payloads of 49 .. 112 bytes take W = 32; the label and the id lie more than 32 bytes before
    the payload's end, so their CRC contribution runs the slice-by-4 chain on T_0 .. T_3."""
    pl = [writer.encode_example([("label", "int64_list", [i % 1000]), ("id", "bytes_list", [b"img-%08d" % i]),
                                 ("tail", "bytes_list", [b"t%039d" % (i * 7919)])]) for i in range(2100)]
    assert all(49 <= len(p) <= 112 for p in pl)
    buf, st, en = synth.framed(pl)
    pair = _pair(monkeypatch, (buf, st, en))
    try:
        r, reruns = _both(pair, buf, st, en, "ends")
        assert reruns == 0 and not np.array(r.status).any() and (np.array(r.verdict) == 7).all()
        _oracle(r, orc, buf, range(0, 2100, 7))
        bad = buf.copy()
        bad[int(st[700]) + 12 + 17] ^= 0x01  # a label byte: the chain's input
        r, reruns = _both(pair, bad, st, en, "ends")
        assert reruns == 1 and int(r.verdict[700]) == 3 and (np.delete(np.array(r.verdict), 700) == 7).all()
    finally:
        for d in pair:
            d.close()


def test_empty_and_single_record_batches(monkeypatch, orc, c1):
    buf, st, en = c1
    pair = _pair(monkeypatch, c1)
    try:
        for mode in ("ends", "u32", "u64"):
            r, _ = _both(pair, buf, st, en, mode, count=0)
            assert len(r) == 0
            for first in (0, 1, 4000):
                r, reruns = _both(pair, buf, st, en, mode, first=first, count=1)
                assert reruns == 0 and len(r) == 1
                _oracle(r, orc, buf, [0])
    finally:
        for d in pair:
            d.close()
