"""The chunked framing index on the CPU (csrc/tfrg_frame_host.cpp: tfrg_index_device's algorithm run
phase by phase through csrc/tfrg_frame.h) against the host walk, tfrg_index_split per piece. Every
comparison is exact equality."""

import numpy as np
import pytest

from tests import _frame_images as F
from tfr_reader import synth

CHUNKS = (64, 256, 4096)


def _check_exact(data, sizes=None, chunk=0):
    info, st, en, pr = F.chunked(data, sizes, chunk)
    h_st, h_en, h_cnt = F.host_index(data, sizes)
    assert info.fallback == 0
    assert info.n_records == h_st.size
    assert np.array_equal(st, h_st) and np.array_equal(en, h_en)
    assert np.array_equal(pr, h_cnt)
    assert info.tiled == F.tiled_of(h_st, h_en)
    if h_st.size:
        assert info.first_start == int(h_st[0])
    return info


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("path", F.GOLDEN, ids=lambda p: p.stem)
def test_golden_file(path, chunk):
    _check_exact(path.read_bytes(), None, chunk)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_golden_files_packed_as_pieces(chunk):
    assert len(F.GOLDEN) == 11
    blobs = [p.read_bytes() for p in F.GOLDEN]
    info = _check_exact(b"".join(blobs), [len(b) for b in blobs], chunk)
    assert info.n_records > 0


@pytest.fixture(scope="module")
def c1_files():
    pay = synth.c1_payloads(3000)
    return {crc: synth.framed(pay, crc=crc)[0] for crc in (True, False)}


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("crc", (True, False), ids=("spec", "zero_crc"))
def test_c1_file(c1_files, crc, chunk):
    info = _check_exact(c1_files[crc], None, chunk)
    assert info.n_records == 3000 and info.tiled == 1
    if chunk == 4096:  # the default chunk: every guess of a plain file is right
        assert info.repaired_chunks == 0 and info.repair_rounds == 0


def test_default_chunk_is_4096(c1_files):
    assert F.info_tuple(F.chunked(c1_files[True], None, 0)[0]) == F.info_tuple(F.chunked(c1_files[True], None, 4096)[0])


@pytest.mark.parametrize("chunk", CHUNKS)
def test_records_spanning_many_chunks(chunk):
    buf = synth.framed(synth.c2_payloads(6, scale=1.0))[0]
    info = _check_exact(buf, None, chunk)
    assert info.n_records == 6 and info.n_chunks > 6 * 4
    if chunk == 4096:
        assert info.repaired_chunks == 0


@pytest.mark.parametrize("chunk", CHUNKS)
def test_c3_records(chunk):
    info = _check_exact(synth.framed(synth.c3_payloads(64))[0], None, chunk)
    if chunk == 4096:
        assert info.repaired_chunks == 0


@pytest.mark.parametrize("chunk", CHUNKS)
def test_nested_records_are_repaired(chunk):
    data = F.nested(chunk)
    assert F.nested_false_chunks(data, chunk) > F.ROUNDS, "several chunks with a false header first"
    info = _check_exact(data, None, chunk)
    assert info.repaired_chunks > 0


@pytest.mark.parametrize("m", (1, 2, F.ROUNDS))
def test_interleaved_chains_within_the_bound(m):
    info = _check_exact(F.interleaved(m), None, 128)
    # (the chunk after a repaired one was judged by its stale exit as well: at least m repairs)
    assert info.repaired_chunks >= m and info.repair_rounds == m


def test_interleaved_chains_past_the_bound():
    info, *_ = F.chunked(F.interleaved(F.ROUNDS + 3), None, 128)
    assert info.fallback == F.FB_ROUNDS


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", sorted(F.LENGTH_EDGES))
def test_length_edges(name, chunk):
    data = F.length_edge(F.LENGTH_EDGES[name])
    assert F.walk_terminates(data, 64)
    info = _check_exact(data, None, chunk)
    # the edge header is a record; the wrap seeks on, the overflow and the negative seeks end the piece
    assert info.n_records == (4 if name != "wrap15" else info.n_records) and info.n_records >= 4


@pytest.mark.parametrize("chunk", CHUNKS)
def test_backward_seek_is_reported(chunk):
    data = F.length_edge(F.SEEK_BACK)
    assert not F.walk_terminates(data, 10_000)
    info, *_ = F.chunked(data, None, chunk)
    assert info.fallback == F.FB_SEEK


def test_cap_smaller_than_the_count(c1_files):
    h_st, h_en, _ = F.host_index(c1_files[True])
    info, st, en, pr = F.chunked(c1_files[True], None, 256, cap=100)  # (chunked() checks the row after cap)
    assert info.n_records == 3000 and int(pr[0]) == 3000 and info.fallback == 0
    assert np.array_equal(st, h_st[:100]) and np.array_equal(en, h_en[:100])


def test_argument_errors():
    L = F.lib()
    import ctypes as C

    from tfr_reader import _native as N

    info = N.TfrgIndexInfo()
    buf = np.zeros(64, np.uint8)
    one = np.array([63], np.uint64)
    assert L.tfrg_index_chunked_host(buf.ctypes.data, 64, N.ptr(one, N.u64p), 1, 64, None, None, 0, None,
                                     C.byref(info)) == -1  # sizes do not sum to nbytes
    one[0] = 64
    assert L.tfrg_index_chunked_host(buf.ctypes.data, 64, N.ptr(one, N.u64p), 1, 64, None, None, 0, None, None) == -1
    assert L.tfrg_index_chunked_host(buf.ctypes.data, 64, N.ptr(one, N.u64p), 1, 96, None, None, 0, None,
                                     C.byref(info)) == -1  # not a power of two
    assert L.tfrg_index_chunked_host(buf.ctypes.data, 0, N.ptr(one, N.u64p), 0, 64, None, None, 0, None,
                                     C.byref(info)) == 0
    assert info.n_records == 0 and info.fallback == 0


FUZZ_SEED = F.FUZZ_SEED  # images FUZZ_SEED .. FUZZ_SEED + 199


def test_random_images_are_exact_or_fall_back():
    fallbacks = ran = 0
    for i in range(200):
        data = F.fuzz_image(FUZZ_SEED + i)
        if not F.walk_terminates(data, 4 * len(data)):
            continue
        ran += 1
        h_st, h_en, h_cnt = F.host_index(data)
        fb = False
        for chunk in (64, 256):
            info, st, en, pr = F.chunked(data, None, chunk)
            if info.fallback:
                fb = True
                continue
            assert info.n_records == h_st.size, (i, chunk)
            assert np.array_equal(st, h_st) and np.array_equal(en, h_en) and np.array_equal(pr, h_cnt), (i, chunk)
            assert info.tiled == F.tiled_of(h_st, h_en), (i, chunk)
        fallbacks += fb
    assert ran >= 150
    assert fallbacks <= 10, fallbacks  # at most 5 % of the 200


def test_random_images_packed_as_pieces():
    """25 fuzzed images to a call: every piece but the first has neighbours and an unaligned base."""
    imgs = F.fuzz_images()
    assert all(F.walk_terminates(d, 4 * len(d)) for d in imgs)  # (before any host walk)
    for g in range(0, len(imgs), F.FUZZ_PACK):
        pack = imgs[g : g + F.FUZZ_PACK]
        sizes = [len(b) for b in pack]
        assert any(sum(sizes[:i]) % 64 for i in range(1, len(sizes)))
        for chunk in CHUNKS:
            info = _check_exact(b"".join(pack), sizes, chunk)
            assert info.repaired_chunks > 0, (g, chunk)


# ------------------------------------------------------------------- past the single-iteration sizes
def _check_rows(data, sizes, chunk, host):
    """_check_exact with the host walk's count as the cap, naming the first differing row"""
    h_st, h_en, h_cnt = host
    info, st, en, pr = F.chunked(data, sizes, chunk, cap=int(h_st.size))
    shift = (chunk or 4096).bit_length() - 1
    assert info.fallback == 0 and info.n_records == h_st.size
    for got, want, what in ((st, h_st, "start"), (en, h_en, "end")):
        msg = F.first_difference(got, want, h_st, shift, what)
        assert msg is None, msg
    assert np.array_equal(pr, h_cnt)
    assert info.tiled == F.tiled_of(h_st, h_en)
    return info


def test_scale_image_coverage():
    F.assert_scale_coverage(64)


@pytest.mark.parametrize("chunk", (64, 0), ids=("chunk64", "default"))
def test_scale_image(chunk):
    c = F.scale_case()
    info = _check_rows(c["data"], None, chunk, c["one"])
    assert info.repaired_chunks > 0 and info.tiled == 1
    info = _check_rows(c["data"], c["sizes"], chunk, c["cut"])
    assert info.repaired_chunks > 0 and info.tiled == 0
    if chunk:
        assert info.n_chunks > F.SCALE_BLOCKS * 256


# ------------------------------------------------------------------ records shorter than their frame
def test_ff_run_needs_more_rows_than_bytes_over_16():
    data = F.ff_run()
    assert F.walk_terminates(data, 4 * len(data))
    h_st, h_en, _ = F.host_index(data)
    assert h_st.size == 606 > len(data) // 16 + 2  # (index_device's first cap for one piece)
    assert (h_en - h_st == 15).sum() == 600
    info = _check_exact(data)
    assert info.tiled == 1 and info.repair_rounds == 2
    assert F.chunked(data, None, 64)[0].fallback == F.FB_ROUNDS


@pytest.mark.parametrize("name", sorted(F.SHORT_SEEKS))
def test_short_forward_seeks(name):
    data = F.length_edge(F.SHORT_SEEKS[name])
    assert F.walk_terminates(data, 64)
    h_st, h_en, _ = F.host_index(data)
    assert int(h_en[3] - h_st[3]) == {"seek12": 12, "seek10": 10, "seek1": 1}[name]
    for chunk in CHUNKS:
        _check_exact(data, None, chunk)


# ---------------------------------------------------------------- zero-CRC images with zero bytes
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("kind", ("zeros", "zeros90", "lists"))
def test_zero_crc_images_with_zero_runs(kind, chunk):
    fallbacks = 0
    for data in F.zero_images(kind, chunk):
        assert F.walk_terminates(data, 4 * len(data))
        assert 40 * chunk <= len(data) < 43 * chunk + 16
        info, *_ = F.chunked(data, None, chunk)
        if info.fallback:
            assert info.fallback == F.FB_ROUNDS
            fallbacks += 1
        else:
            _check_exact(data, None, chunk)
    assert fallbacks == F.ZERO_FALLBACKS[kind, chunk]
    if kind == "lists":
        assert fallbacks == 0
    elif kind == "zeros":
        assert 0 < fallbacks < F.ZERO_IMAGES  # both outcomes


# ------------------------------------------------------------------- two proposals to one chunk
@pytest.mark.parametrize("low_first", (True, False))
def test_the_lowest_of_two_proposals_is_kept(low_first):
    """F.two_proposals: the chunks before an entry-less chunk propose its true entry and a false one
    8 bytes on. The lower one is kept whichever chunk proposes it, and saves a round; the false one
    alone costs the repair that no proposal costs."""
    both = (0, 8) if low_first else (8, 0)
    want = {both: (1, 1), (0, None): (1, 1), (None, 0): (1, 1),
            (8, None): (2, 2), (None, 8): (2, 2), (None, None): (2, 2)}
    for offs, counters in want.items():
        data = F.two_proposals(*offs)
        assert F.walk_terminates(data, 64)
        info = _check_exact(data, None, 256)
        assert (info.repaired_chunks, info.repair_rounds) == counters, offs
