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


def first_difference(got: np.ndarray, want: np.ndarray, want_start: np.ndarray, shift: int, what: str) -> str | None:
    """None when the columns are equal; else the first differing row, its chunk (start >> shift) and
    its block of kFrBlock chunks, for an assertion message."""
    if got.shape == want.shape and np.array_equal(got, want):
        return None
    k = min(got.size, want.size)
    ne = np.flatnonzero(got[:k] != want[:k])
    if not ne.size:
        return f"{what}: {got.size} rows, expected {want.size}"
    i = int(ne[0])
    chunk = int(want_start[i]) >> shift
    return (f"{what}: first difference at row {i} of {want.size} (chunk {chunk}, block {chunk // 256}): "
            f"{int(got[i])} != {int(want[i])}; {ne.size} rows differ")


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


FUZZ_SEED = 20240  # images FUZZ_SEED .. FUZZ_SEED + 199
FUZZ_PACK = 25     # images per packed call


def fuzz_images() -> list[bytes]:
    return [fuzz_image(FUZZ_SEED + i) for i in range(200)]


# ------------------------------------------------------------------------------ one image at scale
SCALE_BLOCKS = 1024  # blocks of 256 chunks that k_fr_scan ranks in one iteration


def scale_image(chunk: int = 64, seed: int = 77) -> tuple[bytes, dict]:
    """Just over SCALE_BLOCKS x 256 chunks of spec-framed records (one payload, so one pair of CRCs, per
    distinct length): lengths 0-700 throughout, a stretch of empty records (four starts per chunk),
    records longer than a block of 256 chunks (blocks without a start) and, past the first
    SCALE_BLOCKS blocks, a record with a damaged length CRC and a record that ends in two nested ones
    (nested()'s construction). -> (image, {"damaged": start, "nested": start of the record after it})."""
    rng = np.random.default_rng(seed)
    block = 256 * chunk
    cache: dict[int, bytes] = {}
    parts: list[bytes] = []
    size = 0

    def add(b: bytes) -> None:
        nonlocal size
        parts.append(b)
        size += len(b)

    def rec(n: int) -> bytes:
        r = cache.get(n)
        if r is None:
            r = cache[n] = record(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        return r

    def plain(upto: int) -> None:
        while size < upto:
            add(rec(int(rng.integers(0, 701))))

    plain(190 * block)
    for _ in range(4096):
        add(rec(0))
    plain(400 * block)
    for n in (2 * block + 100, block + 1, 3 * block + 7):
        add(rec(n))
        plain(size + 5 * block)
    plain(SCALE_BLOCKS * block + 5000)
    where = {"damaged": size}
    good = rec(300)
    add(good[:8] + struct.pack("<I", struct.unpack_from("<I", good, 8)[0] ^ 0x10) + good[12:])
    plain(size + 6000)
    inner = record(b"nested-1") + record(b"nested-2")
    fill = int(rng.integers(2 * chunk, 3 * chunk))
    fill += (chunk - 8 - (size + 16 + fill + len(inner))) % chunk
    add(record(filler(rng, fill) + inner))
    where["nested"] = size
    plain(SCALE_BLOCKS * block + 50_000)
    return b"".join(parts), where


def uneven_pieces(starts: np.ndarray, nbytes: int, seed: int = 78) -> tuple[list[int], dict]:
    """A few hundred uneven piece sizes over an image whose records start at `starts`: cuts on record
    starts and inside records, pieces shorter than 12 bytes, empty pieces (an empty first and last
    piece, and runs of two). -> (sizes, {"on": cuts on a start, "inside": cuts elsewhere})."""
    rng = np.random.default_rng(seed)
    inner = starts[1:].astype(np.int64)
    cuts = rng.choice(inner, 180, replace=False).tolist()
    cuts += rng.integers(1, nbytes, 90).tolist()
    for s in rng.choice(inner, 8, replace=False).tolist():  # 5 bytes of a header, then the rest of it
        cuts += [s, s + 5]
    for s in rng.choice(inner, 4, replace=False).tolist():  # one empty piece
        cuts += [s, s]
    for s in rng.choice(inner, 3, replace=False).tolist():  # two empty pieces in a row
        cuts += [s, s, s]
    cuts += [0, nbytes - 7, nbytes]  # an empty first piece, a 7-byte piece, an empty last piece
    cuts = np.sort(np.array(cuts, np.int64))
    sizes = np.diff(np.concatenate([[0], cuts, [nbytes]]))
    on = np.isin(cuts, inner)
    return sizes.tolist(), {"on": int(on.sum()), "inside": int((~on & (cuts > 0) & (cuts < nbytes)).sum())}


def ff_run(n: int = 9000, seed: int = 3) -> bytes:
    """Three plain records, n bytes of 0xFF, three plain records. Every position of the run reads
    length 2^64 - 1: a forward seek of 15, so records 15 bytes long that start 15 bytes apart."""
    rng = np.random.default_rng(seed)
    plain = [record(filler(rng, 40)) for _ in range(6)]
    return b"".join(plain[:3]) + b"\xff" * n + b"".join(plain[3:])


SHORT_SEEKS = {"seek12": U64 - 3, "seek10": U64 - 5, "seek1": U64 - 14}  # 2^64 - 4, - 6, - 15


# --------------------------------------------------------------------- zero-CRC images with zero bytes
ZERO_SEED = 4100  # images ZERO_SEED .. ZERO_SEED + ZERO_IMAGES - 1 of each kind
ZERO_IMAGES = 40


def zrecord(payload: bytes) -> bytes:
    """A record framed with both CRCs left 0."""
    return struct.pack("<QI", len(payload), 0) + payload + b"\0\0\0\0"


def _varint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def zero_filled(seed: int, chunk: int, zero_fraction: float = 1.0) -> bytes:
    """About 40 chunks of zero-CRC records of up to 3 chunks whose payload bytes are zero (all of
    them, or the given fraction)."""
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < 40 * chunk:
        n = int(rng.integers(0, 3 * chunk))
        pay = np.zeros(n, np.uint8)
        if zero_fraction < 1.0:
            keep = rng.random(n) >= zero_fraction
            pay[keep] = rng.integers(1, 256, int(keep.sum()), dtype=np.uint8)
        out += zrecord(pay.tobytes())
    return bytes(out)


def zero_lists(seed: int, chunk: int) -> bytes:
    """About 40 chunks of zero-CRC records whose payload is protobuf-shaped: a tagged length-delimited
    entry holding a run of 0x00 of up to 3 chunks (a packed int64 list of zeros), then a short
    non-zero entry."""
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < 40 * chunk:
        run = int(rng.integers(0, 3 * chunk))
        tail = filler(rng, int(rng.integers(1, 9)))
        out += zrecord(b"\x0a" + _varint(run) + b"\0" * run + b"\x12" + _varint(len(tail)) + tail)
    return bytes(out)


_SCALE: dict = {}


def scale_case() -> dict:
    """scale_image(), its uneven pieces and the host walk of both, built once and left unchanged."""
    if not _SCALE:
        data, where = scale_image()
        one = host_index(data)
        sizes, cuts = uneven_pieces(one[0], len(data))
        cut = host_index(data, sizes)
        for a in one + cut:
            a.setflags(write=False)
        _SCALE.update(data=data, where=where, one=one, sizes=sizes, cuts=cuts, cut=cut)
    return _SCALE


def assert_scale_coverage(chunk: int = 64, num_cus: int = 0) -> None:
    """What scale_case() is for, from its host walk: k_fr_scan's second iteration, k_fr_guess's
    stride (4 chunks per workgroup, num_cus x 32 workgroups), blocks with and without record starts,
    the repairs past the first SCALE_BLOCKS blocks, and the pieces' edge cases."""
    c = scale_case()
    shift = chunk.bit_length() - 1
    nbytes = len(c["data"])
    n_chunks = (nbytes + chunk - 1) >> shift
    assert n_chunks > SCALE_BLOCKS * 256
    assert n_chunks > 4 * 32 * num_cus
    assert (n_chunks - 1).bit_length() >= 19  # FrTab.jumps of the one-piece run (fr_layout)
    st = c["one"][0]
    per_block = np.bincount((st >> np.uint64(shift + 8)).astype(np.int64), minlength=(n_chunks + 255) // 256)
    assert per_block.size == (n_chunks + 255) // 256 and (per_block == 0).any() and per_block[-1] > 0
    assert np.unique(per_block).size > 10 and (np.diff(per_block) != 0).mean() > 0.5, "the blocks' counts differ"
    assert np.bincount((st >> np.uint64(shift)).astype(np.int64)).max() == 4, "four empty records in a chunk"
    for key in ("damaged", "nested"):
        assert c["where"][key] >> shift >= SCALE_BLOCKS * 256 and c["where"][key] in st
    s = np.array(c["sizes"])
    assert 200 < s.size < 1000 and int(s.sum()) == nbytes
    assert c["cuts"]["on"] > 50 and c["cuts"]["inside"] > 50
    assert (s == 0).sum() >= 5 and ((s > 0) & (s < 12)).sum() >= 5 and ((s[1:] == 0) & (s[:-1] == 0)).sum() >= 2
    assert s[0] == 0 and s[-1] == 0
    assert int(((s + chunk - 1) >> shift).sum()) > SCALE_BLOCKS * 256


def zero_images(kind: str, chunk: int):
    """The ZERO_IMAGES images of a kind: "zeros", "zeros90" (zero_filled) or "lists" (zero_lists)."""
    for i in range(ZERO_IMAGES):
        seed = ZERO_SEED + i
        if kind == "lists":
            yield zero_lists(seed, chunk)
        else:
            yield zero_filled(seed, chunk, {"zeros": 1.0, "zeros90": 0.9}[kind])


# images of ZERO_IMAGES that fall back (always to FB_ROUNDS), as the model gives them: a change in the
# guess's quality shows here ("Hint quality")
ZERO_FALLBACKS = {("zeros", 64): 24, ("zeros", 256): 34, ("zeros", 4096): 32,
                  ("zeros90", 64): 24, ("zeros90", 256): 40, ("zeros90", 4096): 40,
                  ("lists", 64): 0, ("lists", 256): 0, ("lists", 4096): 0}


def two_proposals(first: int | None, second: int | None, chunk: int = 256, seed: int = 11) -> bytes:
    """Two chunks off the chain propose different entries to one chunk without a recognisable header
    (fr_detect's fr_min). Record R starts in chunk 1 and ends in chunk 4 at x1, where a record with a
    damaged length CRC fills the rest of chunk 4: chunk 4 finds no entry. Chunk 1's guess is a header
    nested just before R's start whose length leads to a true start in chunk 5, so in round 0 the
    links skip chunks 2-4, chunk 1 is a mismatch, and chunks 2 and 3, whose guesses are headers
    embedded in R's payload that lead to x1 + first and x1 + second (None: no header), propose those
    to chunk 4. Round 1 reaches chunk 4 at x1: an entry of x1 ends the rounds there, any other entry
    is one more mismatch and one more round."""
    rng = np.random.default_rng(seed)
    s_r, x1, d_end = chunk + 100, 4 * chunk + 40, 5 * chunk + 30
    out = bytearray(record(filler(rng, 100)))
    f = s_r - 16  # the nested header: its record would end at d_end
    out += record(filler(rng, f - len(out) - 12) + header(d_end - f - 16))
    assert len(out) == s_r
    pay = bytearray(filler(rng, x1 - 4 - (s_r + 12)))
    for k, off in ((2, first), (3, second)):
        if off is not None:
            p = k * chunk + 16
            pay[p - (s_r + 12) : p - s_r] = header(x1 + off - p - 16)
    out += record(bytes(pay))
    assert len(out) == x1
    bad = bytearray(record(filler(rng, d_end - x1 - 16)))
    bad[8] ^= 0x10
    out += bad
    while len(out) < 8 * chunk:
        out += record(filler(rng, 40))
    return bytes(out)
