"""Images and call wrappers shared by the framing-index tests (tests/test_frame_index_*.py): the
chunked index on the host (tfrg_index_chunked_host), the host walk it must equal (tfrg_index_split per
piece) and the hostile images both are run on."""

from __future__ import annotations

import ctypes as C
import struct
from pathlib import Path

import numpy as np

from tfr_reader import _native as N

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = sorted((ROOT / "tests" / "golden" / "files").glob("*.tfrecord"))
ROUNDS = 4  # kIndexRepairRounds (csrc/tfrg_frame.h)
FB_ROUNDS, FB_SEEK = N.INDEX_FB_ROUNDS, N.INDEX_FB_SEEK
U64 = (1 << 64) - 1


def lib():
    L = N.lib()
    L.tfrg_index_chunked_host.restype = C.c_int
    L.tfrg_index_chunked_host.argtypes = [C.c_void_p, C.c_uint64, N.u64p, C.c_uint32, C.c_uint32, C.c_void_p,
                                          C.c_void_p, C.c_uint64, N.u64p, C.POINTER(N.TfrgIndexInfo)]
    L.tfrg_index_split.restype = C.c_int64
    L.tfrg_index_split.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64]
    return L


def _arr(data) -> np.ndarray:
    a = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
    return a if a.size else np.zeros(1, np.uint8)[:0]


def host_index(data, sizes=None):
    """(starts, ends, records per piece) of tfrg_index_split over every piece, shifted by its offset."""
    a = _arr(data)
    sizes = [a.size] if sizes is None else list(sizes)
    L = lib()
    st, en, cnt, base = [], [], [], 0
    pad = np.concatenate([a, np.zeros(8, np.uint8)])  # (a valid pointer for empty pieces)
    for sz in sizes:
        p = pad[base:].ctypes.data
        n = L.tfrg_index_split(p, sz, base, None, None, 0)
        s, e = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
        assert L.tfrg_index_split(p, sz, base, N.ptr(s), N.ptr(e), n) == n
        st.append(s[:n])
        en.append(e[:n])
        cnt.append(n)
        base += sz
    return np.concatenate(st), np.concatenate(en), np.array(cnt, np.uint64)


def walk_terminates(data: bytes, max_steps: int) -> bool:
    """Does the host walk (index_walk) end within max_steps records?"""
    pos, size = 0, len(data)
    for _ in range(max_steps):
        if pos + 8 > size:
            return True
        length = struct.unpack_from("<Q", data, pos)[0]
        off = (length + 4) & U64
        if off >= 1 << 63:
            off -= 1 << 64
        np_ = pos + 12 + off
        if np_ >= 1 << 63 or np_ < 0:
            return True
        pos = np_
    return False


def tiled_of(starts: np.ndarray, ends: np.ndarray) -> int:
    """tfrg_index_info.tiled by its definition."""
    return int(bool((ends < (1 << 32)).all()) and bool((starts[1:] == ends[:-1]).all()))


def chunked(data, sizes=None, chunk: int = 0, cap: int | None = None):
    """tfrg_index_chunked_host -> (info, starts[:rows], ends[:rows], piece_records)."""
    a = _arr(data)
    sizes = np.array([a.size] if sizes is None else list(sizes), np.uint64)
    rows = a.size + 1 if cap is None else cap
    st, en = np.full(rows + 1, 0xAA, np.uint64), np.full(rows + 1, 0xAA, np.uint64)
    pr = np.zeros(max(sizes.size, 1), np.uint64)
    info = N.TfrgIndexInfo()
    pad = np.concatenate([a, np.zeros(8, np.uint8)])
    rc = lib().tfrg_index_chunked_host(pad.ctypes.data, a.size, N.ptr(sizes, N.u64p), sizes.size, chunk, N.ptr(st),
                                       N.ptr(en), rows, N.ptr(pr, N.u64p), C.byref(info))
    assert rc == 0, rc
    assert st[rows] == 0xAA and en[rows] == 0xAA, "wrote past cap"
    k = min(rows, int(info.n_records))
    return info, st[:k], en[:k], pr[: sizes.size]


def info_tuple(info) -> tuple:
    return (int(info.n_records), int(info.fallback), int(info.tiled), int(info.first_start), int(info.n_chunks),
            int(info.repaired_chunks), int(info.repair_rounds))


# ---------------------------------------------------------------------------------- images
def mcrc(b: bytes) -> int:
    return int(N.lib().tfrg_masked_crc32c(b, len(b)))


def header(length: int) -> bytes:
    """The 12 header bytes of a spec-framed record."""
    h = struct.pack("<Q", length & U64)
    return h + struct.pack("<I", mcrc(h))


def record(payload: bytes) -> bytes:
    return header(len(payload)) + payload + struct.pack("<I", mcrc(payload))


def filler(rng, n: int) -> bytes:
    """Random bytes without zeros: nothing in them passes for a header."""
    return rng.integers(1, 256, n, dtype=np.uint8).tobytes()


def nested(chunk: int, n: int = 12, seed: int = 5) -> bytes:
    """Records whose payload ends in two complete spec-framed records. Every other record is sized to
    end 8 bytes before a chunk boundary, so the nested headers and the next true start share a chunk
    that no other record starts in: that chunk's guess is the first nested header."""
    rng = np.random.default_rng(seed)
    inner = record(b"nested-1") + record(b"nested-2")
    out = bytearray()
    for i in range(n):
        fill = int(rng.integers(2 * chunk, 3 * chunk))
        if i % 2 == 0:
            fill += (chunk - 8 - (len(out) + 16 + fill + len(inner))) % chunk
        out += record(filler(rng, fill) + inner)
    return bytes(out)


def nested_false_chunks(data: bytes, chunk: int) -> int:
    """Chunks of a nested() image in which a nested header precedes the true start."""
    st, en, _ = host_index(data)
    return sum(1 for e in en[:-1].tolist() if (e - 52) // chunk == e // chunk)


def interleaved(m: int, chunk: int = 128, seed: int = 9) -> bytes:
    """Two interleaved chains. True records of one chunk each, the first one and a half, so a true
    record starts in the middle of every chunk after the first; chunks 1..m hold, 16 bytes in, a
    valid header inside the previous record's payload whose length leads to the same place of the
    next chunk. The guesses of chunks 1..m therefore form a second consistent chain, and each repair
    moves the mismatch one chunk on."""
    rng = np.random.default_rng(seed)
    emb = header(chunk - 16)
    out = bytearray()
    for i in range(m + 1):
        size = chunk + chunk // 2 if i == 0 else chunk
        pay = bytearray(filler(rng, size - 16))
        if i < m:  # the embedded header of chunk i + 1, at chunk * (i + 1) + 16
            at = chunk * (i + 1) + 16 - len(out) - 12
            pay[at : at + 12] = emb
        out += record(bytes(pay))
    return bytes(out)


def length_edge(length: int, seed: int = 3) -> bytes:
    """Three plain records, a header with the given length field, four more plain records."""
    rng = np.random.default_rng(seed)
    plain = [record(filler(rng, 40)) for _ in range(7)]
    if length == U64:  # a forward seek of 15: the next record starts inside this header's frame
        edge = struct.pack("<Q", length) + filler(rng, 7)
    else:
        edge = header(length)
    return b"".join(plain[:3]) + edge + b"".join(plain[3:])


LENGTH_EDGES = {"wrap15": U64, "overflow": (1 << 63) - 5, "negative": (1 << 63) - 4, "negative2": 1 << 63}
SEEK_BACK = (1 << 64) - 16  # pos + 12 + (len + 4) == pos


def fuzz_image(seed: int) -> bytes:
    """Random records, a randomly truncated tail, random byte flips in headers; at most 8 KiB."""
    rng = np.random.default_rng(seed)
    out, heads = bytearray(), []
    target = int(rng.integers(64, 8192))
    while len(out) < target:
        n = int(rng.choice([0, 1, 7, 30, 59, 200, 700]))
        heads.append(len(out))
        out += record(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    out = out[:target] if rng.random() < 0.5 else out[:8192]
    for _ in range(int(rng.integers(0, 3))):
        h = heads[int(rng.integers(0, len(heads)))] + int(rng.integers(0, 12))
        if h < len(out):
            out[h] ^= 1 << int(rng.integers(0, 8))
    return bytes(out)
