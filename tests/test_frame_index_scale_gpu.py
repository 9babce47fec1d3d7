"""The parts of tfrg_index_device that exist only on the GPU (csrc/tfrg_frame.hip: the guess's stride
and ballot, the block scans and k_fr_scan's carry, k_fr_write's rank, the device fr_ld32, the atomics,
the launch schedule) at sizes where they run more than their first iteration, and on images the
suite only gave the CPU model; then HipDecoder.decode_image on indexes it had not seen. The device is
compared with the model (tfrg_index_chunked_host) and the model with the host walk
(tfrg_index_split); every comparison is exact equality."""

import numpy as np
import pytest
import torch

from tests import _frame_images as F
from tests.test_frame_index_gpu import _assert_same, _upload
from tfr_reader import hip, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    d = hip.HipDecoder(0)
    yield d
    d.close()


def _index(dec, d_buf, nbytes, sizes, chunk):
    dec.set_index_chunk(chunk)
    try:
        return dec.index_device(d_buf, nbytes, sizes)
    finally:
        dec.set_index_chunk(0)


def _compare(ix, model, host, chunk):
    """device == model on everything; model == host walk when it reports no fallback. A differing
    column names its first differing row, that row's chunk and block."""
    info, m_st, m_en, m_pr = model
    assert ix.fallback == info.fallback
    if info.fallback:
        return
    assert (ix.n, ix.tiled, ix.first_start, ix.n_chunks, ix.repaired_chunks, ix.repair_rounds) == (
        info.n_records, info.tiled, info.first_start, info.n_chunks, info.repaired_chunks, info.repair_rounds)
    shift = (chunk or 4096).bit_length() - 1
    st = ix.start.cpu().numpy().view(np.uint64)
    en = ix.end.cpu().numpy().view(np.uint64)
    e32 = ix.end32.cpu().numpy().view(np.uint32)
    m_e32 = (m_en & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    for got, want, what in ((st, m_st, "start"), (en, m_en, "end"), (e32, m_e32, "end32")):
        msg = F.first_difference(got, want, m_st, shift, f"device {what} against the model")
        assert msg is None, msg
    assert np.array_equal(ix.piece_records, m_pr.astype(np.int64))
    h_st, h_en, h_cnt = host
    assert info.n_records == h_st.size
    for got, want, what in ((m_st, h_st, "start"), (m_en, h_en, "end")):
        msg = F.first_difference(got, want, h_st, shift, f"model {what} against the host walk")
        assert msg is None, msg
    assert np.array_equal(m_pr, h_cnt)


def _check(dec, data, sizes=None, chunk=0):
    d_buf, nbytes = _upload(data)
    ix = _index(dec, d_buf, nbytes, sizes, chunk)
    model = F.chunked(data, sizes, chunk)
    _compare(ix, model, None if model[0].fallback else F.host_index(data, sizes), chunk)
    return ix


# ------------------------------------------------------------------- past the single-iteration sizes
def test_scale_image_past_one_scan_iteration(dec):
    """One image of more than 1024 x 256 chunks, whole and in uneven pieces at chunk 64 (k_fr_scan's
    carry, k_fr_guess's stride, 19 jumps), then at the default chunk: the table shrinks after having
    grown and the scan is back to one iteration."""
    F.assert_scale_coverage(64, torch.cuda.get_device_properties(0).multi_processor_count)
    c = F.scale_case()
    d_buf, nbytes = _upload(c["data"])
    for sizes, host in ((None, c["one"]), (c["sizes"], c["cut"]), (None, c["one"])):
        for chunk in (64, 0):
            ix = _index(dec, d_buf, nbytes, sizes, chunk)
            model = F.chunked(c["data"], sizes, chunk, cap=int(host[0].size))
            assert model[0].fallback == 0 and model[0].repaired_chunks > 0
            _compare(ix, model, host, chunk)
            assert ix.n_chunks > F.SCALE_BLOCKS * 256 or not chunk


# ------------------------------------------------------------------ the fuzzed images on the device
@pytest.fixture(scope="module")
def fuzz():
    imgs = F.fuzz_images()
    assert len(imgs) == 200 and all(F.walk_terminates(d, 4 * len(d)) for d in imgs)  # (before any host walk)
    return imgs


@pytest.mark.parametrize("chunk", (64, 256))
def test_random_images_alone(dec, fuzz, chunk):
    for data in fuzz:
        _check(dec, data, None, chunk)


@pytest.mark.parametrize("chunk", (64, 256, 4096))
def test_random_images_packed_as_pieces(dec, fuzz, chunk):
    for g in range(0, len(fuzz), F.FUZZ_PACK):
        pack = fuzz[g : g + F.FUZZ_PACK]
        ix = _check(dec, b"".join(pack), [len(b) for b in pack], chunk)
        assert ix.fallback == 0 and ix.repaired_chunks > 0


# ------------------------------------------------------------------- two proposals to one chunk
@pytest.mark.parametrize("offs", ((0, 8), (8, 0)), ids=("low_first", "low_second"))
def test_the_lowest_of_two_proposals_is_kept(dec, offs):
    """fr_min on the device: two chunks propose different entries to one chunk in the same launch
    (tests/test_frame_index_host.py asserts that the choice shows in the counters)."""
    data = F.two_proposals(*offs)
    assert F.walk_terminates(data, 64)
    ix = _check(dec, data, None, 256)
    assert (ix.fallback, ix.repaired_chunks, ix.repair_rounds) == (0, 1, 1)


# ---------------------------------------------------------------- zero-CRC images with zero bytes
@pytest.mark.parametrize("chunk", (64, 256, 4096))
@pytest.mark.parametrize("kind", ("zeros", "zeros90", "lists"))
def test_zero_crc_images_with_zero_runs(dec, kind, chunk):
    fallbacks = 0
    for data in F.zero_images(kind, chunk):
        assert F.walk_terminates(data, 4 * len(data))
        fallbacks += _check(dec, data, None, chunk).fallback != 0
    assert fallbacks == F.ZERO_FALLBACKS[kind, chunk]


# --------------------------------------------------------- decode_image on what it had not seen
def _image_vs_host_index(data, sizes=None, fallback=0):
    """decode_image against decode over the host index, the expected mode from that index; the
    device index is asked first and must report the given fallback (-> its DeviceIndex)"""
    d = hip.HipDecoder(0)
    try:
        h_st, h_en, _ = F.host_index(data, sizes)
        d_buf, nbytes = _upload(data)
        ix = d.index_device(d_buf, nbytes, sizes)
        assert ix.fallback == fallback
        want = d.decode(F._arr(data), h_st, h_en)
        got = d.decode_image(F._arr(data), sizes)
        _assert_same(got, want)
        assert len(got) == h_st.size
        mode = "u32_ends" if not fallback and F.tiled_of(h_st, h_en) else "u64"
        assert d.last_image_mode == mode
        return got, mode, ix
    finally:
        d.close()


@pytest.fixture(scope="module")
def c1_pair():
    return [synth.framed(synth.c1_payloads(40, offset=k))[0].tobytes() for k in (0, 40)]


EDGES = [p for p in F.GOLDEN if p.stem.startswith("edge_")]


@pytest.mark.parametrize("path", EDGES, ids=lambda p: p.stem)
def test_decode_image_edge_files(c1_pair, path):
    assert len(EDGES) == 5
    edge = path.read_bytes()
    modes = []
    for blobs in ([edge], [*c1_pair, edge], [edge, *c1_pair]):
        assert all(F.walk_terminates(b, 64 + len(b)) for b in blobs)
        modes.append(_image_vs_host_index(b"".join(blobs), [len(b) for b in blobs])[1])
    # trailing bytes, a cut header or an overrunning end leave a gap before the next piece's first
    # record: only a piece that ends on a record's end keeps the batch tiled
    h_st, h_en, _ = F.host_index(edge)
    gap = bool(h_st.size) and int(h_en[-1]) != len(edge)
    assert modes == ["u32_ends", "u32_ends", "u64" if gap else "u32_ends"]


@pytest.mark.parametrize("placed", ("alone", "middle"))
def test_decode_image_falls_back_to_the_host_index(c1_pair, placed):
    img = F.interleaved(F.ROUNDS + 3, chunk=4096)
    assert F.walk_terminates(img, 64)
    blobs = [img] if placed == "alone" else [c1_pair[0], img, c1_pair[1]]
    got, mode, _ = _image_vs_host_index(b"".join(blobs), [len(b) for b in blobs], fallback=F.FB_ROUNDS)
    assert mode == "u64"
    assert len(got) == F.ROUNDS + 4 + 80 * (placed == "middle")


def test_more_records_than_the_first_cap(dec):
    """606 records of which 600 are 15 bytes long, 15 bytes apart: index_device runs twice, and the
    tiled index drives the decode from u32 ends whose records are shorter than a frame."""
    data = F.ff_run()
    assert F.walk_terminates(data, 4 * len(data))
    h_st, h_en, _ = F.host_index(data)
    assert h_st.size == 606 > len(data) // 16 + 2 and (h_en - h_st == 15).sum() == 600
    ix = _check(dec, data)
    assert (ix.fallback, ix.n, ix.tiled, ix.repair_rounds) == (0, 606, 1, 2) and ix.start.numel() == 606
    assert _check(dec, data, None, 64).fallback == F.FB_ROUNDS
    got, mode, _ = _image_vs_host_index(data)
    assert mode == "u32_ends" and len(got) == 606


@pytest.mark.parametrize("name", sorted(F.SHORT_SEEKS))
def test_short_forward_seeks(dec, name):
    data = F.length_edge(F.SHORT_SEEKS[name])
    assert F.walk_terminates(data, 64)
    for chunk in (64, 0):
        assert _check(dec, data, None, chunk).fallback == 0
    assert _image_vs_host_index(data)[1] == ("u64" if name == "seek1" else "u32_ends")
