"""The framing index on the device (tfrg_index_device, csrc/tfrg_frame.hip) against its CPU model
(tfrg_index_chunked_host) and the host walk (tfrg_index_split), then through the layers built on it:
HipDecoder.decode_image and StreamDecoder(device_index=True). Every comparison is exact equality."""

import ctypes as C

import numpy as np
import pytest
import torch

from tests import _frame_images as F
from tfr_reader import _native as N
from tfr_reader import hip, stream, synth, writer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    d = hip.HipDecoder(0)
    yield d
    d.close()


def _upload(data) -> tuple[torch.Tensor, int]:
    a = F._arr(data)
    pad = np.zeros(((a.size + 15) & ~15) + 32, np.uint8)
    pad[: a.size] = a
    return torch.from_numpy(pad).to("cuda:0"), int(a.size)


def _check(dec, data, sizes=None, chunk=0):
    """device == model on everything; model == host walk when it reports no fallback"""
    dec.set_index_chunk(chunk)
    try:
        d_buf, nbytes = _upload(data)
        ix = dec.index_device(d_buf, nbytes, sizes)
    finally:
        dec.set_index_chunk(0)
    info, m_st, m_en, m_pr = F.chunked(data, sizes, chunk)
    assert ix.fallback == info.fallback
    if info.fallback:
        return ix
    assert (ix.n, ix.tiled, ix.first_start, ix.n_chunks, ix.repaired_chunks, ix.repair_rounds) == (
        info.n_records, info.tiled, info.first_start, info.n_chunks, info.repaired_chunks, info.repair_rounds)
    st = ix.start.cpu().numpy().view(np.uint64)
    en = ix.end.cpu().numpy().view(np.uint64)
    e32 = ix.end32.cpu().numpy().view(np.uint32)
    assert np.array_equal(st, m_st) and np.array_equal(en, m_en)
    assert np.array_equal(e32, (m_en & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    assert np.array_equal(ix.piece_records, m_pr.astype(np.int64))
    h_st, h_en, h_cnt = F.host_index(data, sizes)
    assert np.array_equal(st, h_st) and np.array_equal(en, h_en) and np.array_equal(ix.piece_records, h_cnt.astype(np.int64))
    return ix


@pytest.mark.parametrize("chunk", (64, 256))
def test_golden_files_and_packed_pieces(dec, chunk):
    blobs = [p.read_bytes() for p in F.GOLDEN]
    for b in blobs:
        _check(dec, b, None, chunk)
    ix = _check(dec, b"".join(blobs), [len(b) for b in blobs], chunk)
    assert ix.n > 2000 and ix.fallback == 0


@pytest.mark.parametrize("chunk", (64, 256))
def test_hostile_images(dec, chunk):
    ix = _check(dec, F.nested(chunk), None, chunk)
    assert ix.fallback == 0 and ix.repaired_chunks > 0
    for name in sorted(F.LENGTH_EDGES):
        assert _check(dec, F.length_edge(F.LENGTH_EDGES[name]), None, chunk).fallback == 0
    assert _check(dec, F.length_edge(F.SEEK_BACK), None, chunk).fallback == F.FB_SEEK


def test_interleaved_chains(dec):
    for m in (1, F.ROUNDS):
        ix = _check(dec, F.interleaved(m), None, 128)
        assert ix.fallback == 0 and ix.repair_rounds == m
    assert _check(dec, F.interleaved(F.ROUNDS + 3), None, 128).fallback == F.FB_ROUNDS


@pytest.mark.parametrize("crc", (True, False), ids=("spec", "zero_crc"))
def test_c1_file_at_the_default_chunk(dec, crc):
    ix = _check(dec, synth.framed(synth.c1_payloads(3000), crc=crc)[0])
    assert ix.n == 3000 and ix.tiled == 1 and ix.repaired_chunks == 0 and ix.n_chunks > 40


def test_cap_and_device_bytes(dec):
    data = synth.framed(synth.c1_payloads(500))[0]
    d_buf, nbytes = _upload(data)
    st = torch.full((101,), -1, dtype=torch.int64, device="cuda:0")
    sizes = np.array([nbytes], np.uint64)
    info = N.TfrgIndexInfo()
    torch.cuda.synchronize()
    N.check(dec._lib.tfrg_index_device(dec._ctx, C.c_void_p(d_buf.data_ptr()), nbytes, N.ptr(sizes, N.u64p), 1,
                                       C.c_void_p(st.data_ptr()), None, None, 100, None, None, C.byref(info)),
            "tfrg_index_device")
    assert info.n_records == 500 and info.fallback == 0
    h_st, _, _ = F.host_index(data)
    got = st.cpu().numpy()
    assert np.array_equal(got[:100].view(np.uint64), h_st[:100]) and got[100] == -1
    assert dec.device_bytes()[0] > 0


def test_argument_errors_and_empty_input(dec):
    L, ctx = dec._lib, dec._ctx
    d_buf, nbytes = _upload(b"\0" * 64)
    info = N.TfrgIndexInfo()
    p = C.c_void_p(d_buf.data_ptr())
    big = np.array([1 << 32], np.uint64)
    assert L.tfrg_index_device(ctx, p, 1 << 32, N.ptr(big, N.u64p), 1, None, None, None, 0, None, None,
                               C.byref(info)) == -1
    short = np.array([32, 31], np.uint64)
    assert L.tfrg_index_device(ctx, p, 64, N.ptr(short, N.u64p), 2, None, None, None, 0, None, None,
                               C.byref(info)) == -1
    ok = np.array([64], np.uint64)
    assert L.tfrg_index_device(ctx, p, 64, N.ptr(ok, N.u64p), 1, None, None, None, 0, None, None, None) == -1
    assert L.tfrg_ctx_set_index_chunk(ctx, 96) == -1 and L.tfrg_ctx_set_index_chunk(ctx, 32) == -1
    # nothing to index: no pieces, and only empty pieces
    pr = np.full(3, 7, np.uint64)
    assert L.tfrg_index_device(ctx, p, 0, N.ptr(ok, N.u64p), 0, None, None, None, 0, None, None, C.byref(info)) == 0
    assert (info.n_records, info.fallback) == (0, 0)
    empty = np.zeros(3, np.uint64)
    assert L.tfrg_index_device(ctx, p, 0, N.ptr(empty, N.u64p), 3, None, None, None, 0, N.ptr(pr, N.u64p), None,
                               C.byref(info)) == 0
    assert (info.n_records, info.fallback) == (0, 0) and not pr.any()


# ------------------------------------------------------------------------------------ decode_image
def _assert_same(a: hip.BatchResult, b: hip.BatchResult):
    for name in ("starts", "ends", "status", "verdict", "order", "row_splits", "slot_base", "i64", "f32", "bytes_off",
                 "bytes_len"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape and np.array_equal(x, y), name
    bad = a.status != 0
    assert np.array_equal(a.aux[bad], b.aux[bad])
    assert a.slot_key == b.slot_key and a.slot_kind == b.slot_kind
    for name in ("bytes_data", "bytes_offsets"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), name


def _image_vs_host_index(data, sizes, crc=True):
    d = hip.HipDecoder(0)
    try:
        h_st, h_en, _ = F.host_index(data, sizes)
        want = d.decode(F._arr(data), h_st, h_en, crc=crc)
        got = d.decode_image(F._arr(data), sizes, crc=crc)
        _assert_same(got, want)
        return got, d.last_image_mode
    finally:
        d.close()


@pytest.mark.parametrize("stem", ("c0_mini", "c0_mini_crc", "c3_mini_crc"))
def test_decode_image_golden(stem):
    data = next(p for p in F.GOLDEN if p.stem == stem).read_bytes()
    got, mode = _image_vs_host_index(data, None)
    assert len(got) > 0 and mode == "u32_ends"  # (a file image is tiled)


def test_decode_image_three_files(tmp_path):
    paths = synth.write_c4_dir(tmp_path, 3, "c1", base=1500)
    blobs = [open(p, "rb").read() for p in paths]
    got, mode = _image_vs_host_index(b"".join(blobs), [len(b) for b in blobs])
    assert len(got) > 2000 and mode == "u32_ends" and not got.status.any()
    # a piece with trailing bytes breaks the tiling: the u64 columns drive the decode
    blobs[0] += b"\x01\x02\x03"
    got, mode = _image_vs_host_index(b"".join(blobs), [len(b) for b in blobs])
    assert mode == "u64" and not got.status.any()


# ------------------------------------------------------------------------------------------ stream
@pytest.fixture(scope="module")
def stream_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame_stream")
    paths = []
    for f in range(3):
        p = d / f"a{f}.tfrecord"
        synth.c4_file(f, "c1", base=1500).tofile(p)
        paths.append(str(p))
    p = d / "b.tfrecord.gz"
    writer.write_tfrecord(p, synth.c3_payloads(200, seed=8, max_len=6), compression="GZIP")
    paths.append(str(p))
    p = d / "c-partial-header.tfrecord"  # 10 trailing bytes: a header cut short is a record
    p.write_bytes(writer.frame_records(synth.c1_payloads(300, offset=7)) + b"\x03" + b"\0" * 7 + b"\x01\x02")
    paths.append(str(p))
    return paths


def _batches(paths, device_index, extra=None):
    sd = stream.StreamDecoder(0, batch_bytes=1 << 17, copy_threads=2, device_index=device_index)
    try:
        out = [(b.piece_records, b.result) for b in sd.batches(paths)]
        if extra is not None:  # one more batch: a memory piece
            pieces = [("mem", 0, None, 0, int(extra.size), extra)]
            sd._submit(0, 0, pieces)
            b = sd._finish(0, 0, pieces)
            out.append((b.piece_records, b.result))
        return out
    finally:
        sd.close()


def test_stream_device_index_equals_host_index(dec, stream_dir):
    # the interleaved chains at the default chunk: the device index falls back (checked below), the
    # stream indexes that batch on the host
    extra = np.frombuffer(F.interleaved(F.ROUNDS + 3, chunk=4096), np.uint8)
    d_buf, nbytes = _upload(extra)
    assert dec.index_device(d_buf, nbytes).fallback == F.FB_ROUNDS
    off = _batches(stream_dir, False, extra)
    on = _batches(stream_dir, True, extra)
    assert len(on) == len(off) > 3
    for (pr_on, r_on), (pr_off, r_off) in zip(on, off):
        assert pr_on == pr_off
        _assert_same(r_on, r_off)
    assert sum(len(r) for _, r in on) > 4000
