"""Frame classes of the record-shape templates (csrc/tfrg_internal.h kLtFrame), on the host: what
tfrg_learn_templates_host keeps for spec-framed, zero-CRC ("unchecked") and mixed samples, and
k_tpl_lane's hit rule per class restated in numpy (csrc/tfrg_tpl.hip):

* spec template, CRCs on: mask match and masked(K ^ lin) == the stored data CRC (as ever);
* unchecked template, CRCs on: mask match (which proves both stored CRC fields 0) and
  masked(K ^ lin) != 0 -- a record whose true masked payload CRC is 0 keeps its DATA_CRC verdict bit
  by missing;
* CRCs off: the mask match alone.

No GPU: the kernel runs the same rule in tests/test_unchecked_frames_gpu.py.
"""

import numpy as np

from oracle import oracle as O
from tfr_reader import _native as N
from tfr_reader import synth, writer

# tfrg_internal.h layout
K_L, K_NE, K_CRCW, K_CHAIN, K_K, K_ABSENT, K_FRAME, K_ENT = 0, 1, 2, 3, 4, 5, 6, 8
K_WIN = K_ENT + 4 * 16
K_SLOT = K_WIN + 3 * 64
K_WORDS = K_SLOT + 3 * 16
KEYS, SLOTS = [b"label", b"id"], [(0, 3), (1, 1)]


def _tables() -> np.ndarray:
    t0 = np.zeros(256, np.uint64)
    for v in range(256):
        c = v
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
        t0[v] = c
    T = np.zeros((32, 256), np.uint64)
    x = t0.copy()
    for d in range(32):
        T[d] = x
        x = (x >> np.uint64(8)) ^ t0[(x & np.uint64(0xFF)).astype(np.int64)]
    return T.astype(np.uint32)


TABS = _tables()


def _mask_crc(c: int) -> int:
    return ((((c >> 15) | (c << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF


def _learn(buf, st, en, keys=KEYS, slots=SLOTS):
    blob = b"".join(keys)
    offs = np.zeros(len(keys) + 1, np.uint64)
    offs[1:] = np.cumsum([len(k) for k in keys])
    sk = np.array([s[0] for s in slots], np.uint32)
    sd = np.array([s[1] for s in slots], np.uint8)
    out = np.zeros(32 * K_WORDS, np.uint32)
    W = np.zeros(1, np.uint32)
    b = np.frombuffer(blob, np.uint8)
    nt = N.lib().tfrg_learn_templates_host(len(keys), N.ptr(b), N.ptr(offs), None, len(slots), N.ptr(sk), N.ptr(sd),
                                           N.ptr(buf), buf.size, N.ptr(st), N.ptr(en), st.size, 0, N.ptr(out),
                                           out.size, N.ptr(W))
    assert nt >= 1
    return out[: nt * K_WORDS].reshape(nt, K_WORDS), int(W[0])


def _hit(tpls, W, buf, s, e, nocrc=False, strict=False):
    """k_tpl_lane's match for one record: (template index or -1, hit verdict)."""
    if e < 4 * W or e > buf.size:
        return -1, 0
    win = buf[e - 4 * W : e].view("<u4").astype(np.uint32)
    for t, tp in enumerate(tpls):
        L, frame = int(tp[K_L]), int(tp[K_FRAME])
        if e - s != L + 16:
            continue
        B, M, Cm = tp[K_WIN : K_WIN + W], tp[K_WIN + W : K_WIN + 2 * W], tp[K_WIN + 2 * W : K_WIN + 3 * W]
        if ((win ^ B) & M).any():  # (every word: the unchecked class masks word W - 1 too)
            continue
        if nocrc:
            return t, 1
        lin, c = 0, 0
        for i in range(int(tp[K_CHAIN]), W - 9):
            x = int(win[i] & Cm[i]) ^ c
            c = int(TABS[3][x & 255] ^ TABS[2][(x >> 8) & 255] ^ TABS[1][(x >> 16) & 255] ^ TABS[0][x >> 24])
        for j in range(8):
            if not (int(tp[K_CRCW]) >> j) & 1:
                continue
            x = int(win[W - 9 + j] & Cm[W - 9 + j]) ^ (c if j == 0 else 0)
            for b in range(4):
                lin ^= int(TABS[28 - 4 * j + 3 - b][(x >> (8 * b)) & 255])
        mc = _mask_crc(lin ^ int(tp[K_K]))
        if frame:
            if mc != 0 and not strict:
                return t, 1
        elif mc == int(win[W - 1]):
            return t, 7
    return -1, 0


def _put32(buf, at, v):
    buf[at : at + 4] = np.frombuffer(int(v).to_bytes(4, "little"), np.uint8)


def crc_zero_payload() -> bytes:
    """A C1 record whose masked payload CRC-32C is exactly 0: the CRC is affine in the 32 free bits of
    the id b"img-" + 4 bytes + b"abcd", so they solve a 32 x 32 system over GF(2)."""
    def pl(x):
        return writer.encode_example([("label", "int64_list", [5]),
                                      ("id", "bytes_list", [b"img-" + x.to_bytes(4, "little") + b"abcd"])])
    # masked(c) == 0  <=>  rotr15(c) == -0xA282EAD8
    r = (-0xA282EAD8) & 0xFFFFFFFF
    target = ((r << 15) | (r >> 17)) & 0xFFFFFFFF
    base = O.crc32c(pl(0))
    cols = [O.crc32c(pl(1 << k)) ^ base for k in range(32)]
    # Gaussian elimination: rows are the columns' images with the bit of x they stand for
    rows = [(cols[k], 1 << k) for k in range(32)]
    want, x = target ^ base, 0
    for bit in range(32):
        piv = next((i for i, (v, _) in enumerate(rows) if (v >> bit) & 1), None)
        assert piv is not None, "the 32 free bits do not span the CRC"
        pv, px = rows.pop(piv)
        rows = [((v ^ pv, m ^ px) if (v >> bit) & 1 else (v, m)) for v, m in rows]
        if (want >> bit) & 1:
            want ^= pv
            x ^= px
    assert want == 0
    return pl(x)


def _frames(tpls):
    return sorted(int(t[K_FRAME]) for t in tpls)


def test_spec_sample_keeps_spec_templates_as_before():
    buf, st, en = synth.framed(synth.c1_payloads(3000))
    tpls, W = _learn(buf, st, en)
    assert len(tpls) == 2 and W == 16 and _frames(tpls) == [0, 0]
    for tp in tpls:  # the spec layout: the length CRC fixed, the data CRC word unmasked
        L = int(tp[K_L])
        off = 4 * W - (L + 16)
        Bm = tp[K_WIN : K_WIN + W].tobytes()
        Mm = tp[K_WIN + W : K_WIN + 2 * W].tobytes()
        assert int.from_bytes(Bm[off + 8 : off + 12], "little") == O.masked_crc32c(L.to_bytes(8, "little"))
        assert Mm[off + 8 : off + 12] == b"\xff" * 4 and int(tp[K_WIN + 2 * W - 1]) == 0
    for i in range(3000):
        t, v = _hit(tpls, W, buf, int(st[i]), int(en[i]))
        assert (t >= 0 and v == 7) or int(en[i]) < 64, i


def test_zero_crc_sample_keeps_unchecked_templates():
    n = 3000
    buf, st, en = synth.framed(synth.c1_payloads(n), crc=False)
    buf = buf.copy()
    tpls, W = _learn(buf, st, en)
    assert len(tpls) == 2 and W == 16 and _frames(tpls) == [1, 1]
    spec, _ = _learn(*synth.framed(synth.c1_payloads(n)))
    for tp in tpls:  # the spec template of the shape but for the two CRC fields
        sp = next(s for s in spec if int(s[K_L]) == int(tp[K_L]))
        L = int(tp[K_L])
        off = 4 * W - (L + 16)
        d = np.flatnonzero(tp != sp).tolist()
        assert set(d) <= {K_FRAME, K_WIN + (off + 8) // 4, K_WIN + (off + 8) // 4 + 1, K_WIN + 2 * W - 1}, d
        Bm = tp[K_WIN : K_WIN + W].tobytes()
        Mm = tp[K_WIN + W : K_WIN + 2 * W].tobytes()
        assert Bm[off + 8 : off + 12] == b"\0" * 4 and Mm[off + 8 : off + 12] == b"\xff" * 4
        assert int(tp[K_WIN + W - 1]) == 0 and int(tp[K_WIN + 2 * W - 1]) == 0xFFFFFFFF
    for i in range(n):
        s, e = int(st[i]), int(en[i])
        t, v = _hit(tpls, W, buf, s, e)
        assert (t >= 0 and v == 1) or e < 64, i
        assert _hit(tpls, W, buf, s, e, strict=True)[0] == -1
        assert _hit(tpls, W, buf, s, e, nocrc=True)[0] == t
    # a record that carries a true CRC is no unchecked-frame record: the canonical walk's
    s, e = int(st[300]), int(en[300])
    b2 = buf.copy()
    _put32(b2, e - 4, O.masked_crc32c(bytes(buf[s + 12 : e - 4])))
    assert _hit(tpls, W, b2, s, e)[0] == -1
    s, e = int(st[200]), int(en[200])
    b2 = buf.copy()
    _put32(b2, s + 8, O.masked_crc32c(bytes(buf[s : s + 8])))
    assert _hit(tpls, W, b2, s, e)[0] == -1


def _mixed(n, run=200):
    pl = synth.c1_payloads(n)
    a, st, en = synth.framed(pl)
    z, _, _ = synth.framed(pl, crc=False)
    buf = a.copy()
    zero = (np.arange(n) // run) % 2 == 1
    for i in np.flatnonzero(zero):
        buf[int(st[i]) : int(en[i])] = z[int(st[i]) : int(en[i])]
    return buf, st, en, zero


def test_mixed_sample_keeps_a_shape_once_per_class():
    n = 3000
    buf, st, en, zero = _mixed(n)
    tpls, W = _learn(buf, st, en)
    assert len(tpls) == 4 and _frames(tpls) == [0, 0, 1, 1]
    for i in range(n):
        s, e = int(st[i]), int(en[i])
        if e < 64:
            continue
        t, v = _hit(tpls, W, buf, s, e)
        assert t >= 0 and int(tpls[t][K_FRAME]) == int(zero[i]) and v == (1 if zero[i] else 7), i
        # without CRCs either class of template may take it: the first of its length that matches
        assert _hit(tpls, W, buf, s, e, nocrc=True) == (t, 1), i


def test_masked_payload_crc_of_zero_misses():
    p0 = crc_zero_payload()
    assert O.masked_crc32c(p0) == 0 and len(p0) == len(synth.c1_payloads(1, 5)[0])
    pl = synth.c1_payloads(600)
    pl[400] = p0
    buf, st, en = synth.framed(pl, crc=False)
    tpls, W = _learn(buf, st, en)
    assert _frames(tpls) == [1, 1]
    s, e = int(st[400]), int(en[400])
    assert _hit(tpls, W, buf, s, e)[0] == -1  # (its verdict is LEN_MATCH | DATA_CRC: k_lane_count's)
    assert _hit(tpls, W, buf, s, e, nocrc=True)[0] >= 0
    assert all(_hit(tpls, W, buf, int(st[i]), int(en[i]))[0] >= 0 for i in (399, 401))
