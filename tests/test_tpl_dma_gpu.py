"""k_tpl_lane's pipelined stage: the span of group g + 1 is requested by LDS-DMA into the wave's one
stage as soon as group g's windows are out of it, and waited for (the wave's own vmcnt) at the top of
the next step. A stale or half-landed stage gives other labels and a CRC miss, so every case decodes
C1 records with mixed 58- / 59-byte lengths and random-looking labels on two contexts, staged windows
on batches of any size (TFRG_TPL_STAGE=2) against per-lane window loads (=0), and asks for equal
columns, info words, kind totals and re-run counts, and for the oracle's values on a sample that
holds every group's first and last lane.

At a few thousand records launch_tpl_lane would give every wave one group, and the loop body would
never run twice; TFRG_TPL_GPW (read at context creation) gives a wave 2, 4 or 8 groups on a batch of
any size. The kernel reports nothing about the path it took, so "reaches the pipelined loop" is
asserted from the launch arithmetic: more groups than one wave's share, so the first wave runs
TFRG_TPL_GPW steps, each but the last with a fill in flight across its match and stores.
"""

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gpu_parity import _compare_to_oracle
from tests.test_tpl_stage_gpu import COLS, INFO, N
from tests.test_unchecked_frames_gpu import _device
from tfr_reader import hip, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    return O.Oracle()


def _c1(crc=True):
    blob, offs = synth.c1_blob(N, 100, 7)
    buf = synth.frame_blob(blob, offs, crc)
    ends = (offs[1:] + 16 * np.arange(1, N + 1)).astype(np.uint64)
    starts = np.concatenate([[0], ends[:-1]]).astype(np.uint64)
    assert int(ends[-1]) == buf.size and len(set((ends - starts).tolist())) == 2
    return buf, starts, ends


@pytest.fixture(scope="module")
def c1():
    return _c1()


@pytest.fixture(scope="module")
def c1_zero():
    return _c1(False)


def _pair(monkeypatch, sample, gpw):
    """Two fresh contexts that learned the same sample, both with `gpw` groups per wave: the
    pipelined stage on batches of any size, and per-lane windows."""
    monkeypatch.setenv("TFRG_OPTIMISTIC", "1")
    monkeypatch.setenv("TFRG_TPL_GPW", str(gpw))
    monkeypatch.setenv("TFRG_TPL_STAGE", "2")
    on = hip.HipDecoder(0)
    monkeypatch.setenv("TFRG_TPL_STAGE", "0")
    off = hip.HipDecoder(0)
    for d in (on, off):
        d.decode(*sample)
        assert d.template_count() >= 1
    return on, off


def _close(pair):
    for d in pair:
        d.close()


def _both(pair, gpw, buf, st, en, mode, **kw):
    n = kw.get("count", len(st) - kw.get("first", 0))
    assert (n + 63) // 64 > gpw >= 2  # (the first wave runs gpw steps of the group loop)
    (a, ra), (b, rb) = (_device(d, buf, st, en, mode, **kw) for d in pair)
    for k in COLS:
        assert np.array_equal(np.array(getattr(a, k)), np.array(getattr(b, k))), k
    for k in INFO:
        assert int(getattr(a.info, k)) == int(getattr(b.info, k)), k
    assert list(a.info.kind_totals) == list(b.info.kind_totals)
    assert ra == rb
    return a, ra


def _edges(n, extra=()):
    """Every group's first and last lane, the batch's last record, and `extra`."""
    idx = set(range(0, n, 64)) | set(range(63, n, 64)) | {n - 1} | set(extra)
    return sorted(i for i in idx if 0 <= i < n)


def _oracle(r, orc, buf, idx, check_crc=True):
    bad = _compare_to_oracle(r, orc, buf, r.starts, r.ends, check_crc=check_crc, idx=idx)
    assert not bad, bad


@pytest.mark.parametrize("mode", ["ends", "u32", "u64"])
@pytest.mark.parametrize("gpw", [2, 4, 8])
def test_steady_state(monkeypatch, orc, c1, gpw, mode):
    buf, st, en = c1
    pair = _pair(monkeypatch, c1, gpw)
    try:
        # from byte 0: head_fix, and lanes whose window is not whole (the first record, the last group)
        assert int(en[0]) < 64
        r, reruns = _both(pair, gpw, buf, st, en, mode)
        assert reruns == 0 and int(r.info.implicit_cols) == 7 and not np.array(r.status).any()
        _oracle(r, orc, buf, _edges(N, range(0, 66)))
        # a record-range cut of the same image
        r, reruns = _both(pair, gpw, buf, st, en, mode, first=1001, count=3500)
        assert reruns == 0 and len(r) == 3500 and not np.array(r.status).any()
        _oracle(r, orc, buf, _edges(3500, range(0, 3500, 53)))
    finally:
        _close(pair)


def test_alternating_eligibility_inside_one_wave(monkeypatch, orc, c1):
    """GPW 8, u32 pairs. First wave (groups 0 .. 7): the records of groups 1, 4 and 5 reversed, so
    staged, per-lane, staged, staged, per-lane, per-lane, staged, staged. Second wave (groups 8 .. 15):
    group 14's last record far above the stage span, so a per-lane group between staged ones there
    too; each per-lane window is consumed while the next group's DMA is issued behind it."""
    buf, st, en = c1
    pair = _pair(monkeypatch, c1, 8)
    try:
        p = np.arange(N)
        for g in (1, 4, 5):
            p[64 * g : 64 * g + 64] = p[64 * g : 64 * g + 64][::-1]
        far = 14 * 64 + 63
        p[[far, 4000]] = p[[4000, far]]
        assert int(en[p[far]]) - int(en[p[far - 63]]) > 8192
        r, reruns = _both(pair, 8, buf, st[p], en[p], "u32")
        assert reruns == 0 and not np.array(r.status).any() and int(r.info.tpl_groups_missed) == 0
        _oracle(r, orc, buf, _edges(N, list(range(0, 1024)) + list(range(3968, 4032))))
    finally:
        _close(pair)


def test_the_batchs_last_group(monkeypatch, orc, c1):
    """ends, GPW 8: a batch whose last record ends on a 16-byte piece (the last group's span is whole
    pieces inside the batch: staged) and one whose does not (per-lane)."""
    buf, st, en = c1
    pair = _pair(monkeypatch, c1, 8)
    try:
        on_piece = [k for k in range(4700, N) if int(en[k - 1]) % 16 == 0 and k % 64 not in (0, 1)]
        off_piece = [k for k in range(4700, N) if int(en[k - 1]) % 16 not in (0, 15) and k % 64 not in (0, 1)]
        assert on_piece and off_piece
        for k in (on_piece[-1], off_piece[-1]):
            cut = np.ascontiguousarray(buf[: int(en[k - 1])])
            r, reruns = _both(pair, 8, cut, st, en, "ends", count=k)
            assert reruns == 0 and len(r) == k and not np.array(r.status).any()
            _oracle(r, orc, cut, _edges(k, range(k - 70, k)))
    finally:
        _close(pair)


def test_corrupted_bytes_at_wave_edges(monkeypatch, orc, c1):
    """One payload byte flipped at the first and last lane of groups 0, 7, 8 and the last: a wave's
    first and last group, the next wave's first (GPW 8)."""
    buf, st, en = c1
    pair = _pair(monkeypatch, c1, 8)
    last = (N - 1) // 64 * 64
    try:
        hit = [0, 63, 7 * 64, 7 * 64 + 63, 8 * 64, 8 * 64 + 63, last, N - 1]
        bad = buf.copy()
        for i in hit:
            bad[int(en[i]) - 7] ^= 0x01  # an id digit
        r, reruns = _both(pair, 8, bad, st, en, "ends")  # (tpl_groups_missed and statuses: equal, _both)
        assert reruns == 1 and int(r.info.tpl_groups_missed) == 4
        v = np.array(r.verdict)
        assert sorted(np.flatnonzero(v != 7).tolist()) == sorted(hit) and (v[hit] == 3).all()
        _oracle(r, orc, bad, _edges(N, hit))
    finally:
        _close(pair)


@pytest.mark.parametrize("which", ["zero_crc_file", "crc_off_decode"])
def test_frame_class_kernel(monkeypatch, orc, c1, c1_zero, which):
    """The instantiation that knows frame classes, GPW 8: a file written with both CRC fields 0, and
    a crc=False decode of the spec-framed file."""
    buf, st, en = c1_zero if which == "zero_crc_file" else c1
    flags = {} if which == "zero_crc_file" else {"crc": False}
    pair = _pair(monkeypatch, (buf, st, en), 8)
    try:
        r, reruns = _both(pair, 8, buf, st, en, "ends", **flags)
        assert reruns == 0 and int(r.info.tpl_groups_missed) == 0
        assert not np.array(r.status).any() and (np.array(r.verdict) == 1).all()
        _oracle(r, orc, buf, _edges(N, range(0, 66)), check_crc=which == "zero_crc_file")
    finally:
        _close(pair)


def test_variable_length_ids_16_templates(monkeypatch, orc):
    """c1v at GPW 8, whichever variant the LDS budget selects."""
    n = 5000
    blob, offs = synth.c1v_blob(n, 0, 11)
    buf = synth.frame_blob(blob, offs)
    en = (offs[1:] + 16 * np.arange(1, n + 1)).astype(np.uint64)
    st = np.concatenate([[0], en[:-1]]).astype(np.uint64)
    pair = _pair(monkeypatch, (buf, st, en), 8)
    try:
        assert pair[0].template_count() == 16
        for mode in ("ends", "u64"):
            r, reruns = _both(pair, 8, buf, st, en, mode)
            assert reruns == 0 and not np.array(r.status).any()
        _oracle(r, orc, buf, _edges(n, range(0, 66)))
    finally:
        _close(pair)
