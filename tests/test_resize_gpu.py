"""Resized raw images on the device (tfrg_result_raw_resize: k_resize). Records hold an image as raw bytes
next to its height and width; the expectation never comes from ``tfr_reader.raw``: bilinear rows are
compared with torch's float64 ``interpolate`` within the bound derived in tests/test_resize_host.py,
identity resizes (f == 0 everywhere) and nearest rows bit for bit. Outputs lie inside 0xA5-poisoned
buffers: guards, skipped rows and refused calls keep the poison."""

import ctypes as C

import numpy as np
import pytest

from tests.test_resize_host import BIAS, IMAGES, SCALE, as_float, ref64, tolerance
from tfr_reader import _native as N
from tfr_reader import hip, shard, synth, writer
from tfr_reader import raw as W

pytestmark = pytest.mark.gpu

POISON, GUARD, POISON32 = 0xA5, 256, -1515870811
BAND = N.RESIZE_BAND
SHAPES = [(h, w) for h, w, _, _ in IMAGES] + [(3, 5), (2, 21), (6, 6), (4, 3), (11, 2), (1, 40), (8, 9)]  # 17 records


@pytest.fixture(scope="module")
def dec():
    d = hip.HipDecoder(0)
    yield d
    d.close()


def dev():
    import torch

    return torch.device("cuda", 0)


def make(src, C, shapes=SHAPES, seed=0):
    rng = np.random.default_rng(seed)
    dt = W.SRC[src][1]
    if np.dtype(dt).kind == "f":
        return [rng.uniform(-8, 8, (h, w, C)).astype(dt) for h, w in shapes]
    return [rng.integers(*{"uint8": (0, 256), "int16": (-32768, 32768)}[src], (h, w, C)).astype(dt) for h, w in shapes]


def feats(a, **over):
    """The features of one record, the image last; ``over``: height / width / image values, None: no key."""
    f = {"height": [a.shape[0]], "width": [a.shape[1]], "image": [a.tobytes()], **over}
    return [(k, "bytes_list" if k == "image" else "int64_list", v) for k, v in f.items() if v is not None]


def write(records):
    """Framed records; a pad feature puts record i's image (the payload's last bytes) at byte i mod 16."""
    payloads, pos = [], 0
    for i, f in enumerate(records):
        img = f[-1][2][0] if f[-1][0] == "image" and f[-1][2] else b""
        for p in range(16):
            payload = writer.encode_example([("pre", "bytes_list", [b"p" * p])] + f)
            if (pos + 12 + len(payload) - len(img)) % 16 == i % 16:
                break
        payloads.append(payload)
        pos += len(payload) + 16
    return synth.framed(payloads)


def run(call, sp, m, shift=0, **kw):
    """One call over poisoned outputs: (the batch, the output's bits as [m, OH, OW, C], written shapes)."""
    import torch

    osz, nb = W.ITEMSIZE[sp.out_type], m * sp.count * W.ITEMSIZE[sp.out_type]
    lo = GUARD + shift * osz
    big = torch.full((lo + nb + GUARD,), POISON, dtype=torch.uint8, device=dev())
    view = big[lo : lo + nb].view(W._torch_dtype(sp)).view(m, *sp.out_shape)
    shp = torch.full((m, 2), POISON32, dtype=torch.int32, device=dev())
    got = call([sp], out={sp.out_name: (view, shp) if sp.shapes else view},
               **{k: (torch.from_numpy(np.asarray(v)).to(dev()) if v is not None else None) for k, v in kw.items()})
    host = big.cpu().numpy()
    assert (host[:lo] == POISON).all() and (host[lo + nb :] == POISON).all()
    body = host[lo : lo + nb].view({1: np.uint8, 2: np.uint16, 4: np.uint32}[osz]).reshape(m, *sp.out_shape)
    return got, (body.transpose(0, 2, 3, 1) if sp.planar else body), shp.cpu().numpy()


def values(bits, out):
    return as_float(bits.view({"float32": np.float32, "float16": np.float16}.get(out, np.uint16)), out)


def close(img, box, flip, sp, bits):
    want = ref64(img, box, flip, sp.size, sp.scale, sp.bias)
    err = np.abs(values(bits, sp.out) - want)
    assert (err <= tolerance(img, box, want, sp.out, sp.scale, sp.bias)).all(), err.max()


@pytest.mark.parametrize("out", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("src", ["uint8", "int16", "float32"])
def test_identity_is_bit_exact(dec, src, out):
    for C in (1, 3, 4):
        imgs = make(src, C, [(9, 11)] * 3)
        dec.decode(*write([feats(a) for a in imgs]))
        for planar in (False, True):
            sp = W.Resize("image", size=(9, 11), src=src, out=out, channels=C, planar=planar, scale=SCALE[:C], bias=BIAS[:C])
            _, bits, _ = run(dec.resize, sp, 3, shift=1)
            y = (np.stack(imgs).astype(np.float64) * np.asarray(sp.scale) + np.asarray(sp.bias)).astype(np.float32)
            want = y.view(np.uint32) if out == "float32" else y.astype(np.float16).view(np.uint16) if out == "float16" else W.bf16_bits(y).reshape(y.shape)
            assert np.array_equal(bits, want)


ROWS = [5, 5, 0, 16, 1, -1, 2, 3, 4, 17, 6, 7, 8, 9, 10, 1 << 40, 11, 12, 13, 14, 15]


@pytest.mark.parametrize("src,out,C,planar", [("uint8", "float32", 3, True), ("uint8", "bfloat16", 4, True), ("int16", "float16", 1, False),
                                              ("float32", "float32", 3, False)])
@pytest.mark.parametrize("size", [(16, 12), (8, 8), (1, 13), (13, 1)])
def test_mixed_shapes_boxes_flips_and_row_lists(dec, src, out, C, planar, size):
    imgs = make(src, C)
    res = dec.decode(*write([feats(a) for a in imgs]))
    s = list(res.slot_key).index("image")
    off = {int(res.bytes_off[int(res.slot_base[s]) + int(res.row_splits[s][g])]) % 16 for g in range(len(imgs))}
    assert len(off) == 16  # the image starts at every residue
    sp = W.Resize("image", size=size, src=src, out=out, channels=C, planar=planar, scale=SCALE[:C], bias=BIAS[:C], shapes=True)
    geo = [((0, 0, *SHAPES[g]), 0) if g >= len(IMAGES) else (IMAGES[g][2] or (0, 0, *SHAPES[g]), IMAGES[g][3])
           for g in (r if 0 <= r < 17 else 0 for r in ROWS)]
    geo[1] = ((12, 0, 8, 31), 1)  # record 5 drawn twice: another crop, mirrored
    got, bits, shp = run(dec.resize, sp, len(ROWS), rows=np.array(ROWS, np.int64), boxes=np.array([b for b, _ in geo], np.int32),
                         flip=np.array([f for _, f in geo], np.uint8))
    for k, r in enumerate(ROWS):
        if not 0 <= r < 17:
            assert (np.ascontiguousarray(bits[k]).view(np.uint8) == POISON).all() and (shp[k] == POISON32).all()
            continue
        close(imgs[r], geo[k][0], geo[k][1], sp, bits[k])
        assert shp[k].tolist() == list(SHAPES[r])
    assert got.stats["image"].tolist() == [0, 0, 0, 0] and got.skipped == 3 and list(got.shapes) == ["image"]


@pytest.mark.parametrize("oh", [1, BAND, BAND + 1, 2 * BAND + 1])
def test_band_seams(dec, oh):
    imgs = make("uint8", 3, [(37, 53), (5, 7), (2 * BAND + 1, 20)], seed=oh)
    dec.decode(*write([feats(a) for a in imgs]))
    sp = W.Resize.normalize("image", [120.0, 110.0, 100.0], [60.0, 61.0, 62.0], size=(oh, 19), channels=3, out="bfloat16", planar=True)
    _, bits, _ = run(dec.resize, sp, 3)
    for k, a in enumerate(imgs):
        close(a, (0, 0, *a.shape[:2]), 0, sp, bits[k])


def test_crop_row_limit_and_largest_output(dec):
    """A crop row of exactly TFRG_RESIZE_MAX_ROW_BYTES works; one element over is a bad box. out_w *
    channels == 4096 takes the largest LDS a launch asks for."""
    a = make("int16", 1, [(2, 8193)])[0]
    dec.decode(*write([feats(a)]))
    sp = W.Resize("image", size=(3, 4096), src="int16", scale=SCALE[0], bias=BIAS[0], fill=-7)
    got, bits, _ = run(dec.resize, sp, 2, rows=np.array([0, 0]), boxes=np.array([[0, 1, 2, 8192], [0, 0, 2, 8193]], np.int32))
    close(a, (0, 1, 2, 8192), 0, sp, bits[0])
    assert (bits[1] == np.float32(-7).view(np.uint32)).all() and got.stats["image"].tolist() == [0, 1, 0, 0]


def test_bad_rows_are_fill_and_counted(dec):
    a = make("uint8", 3, [(6, 5)])[0]
    b = a.tobytes()
    recs = [feats(a), feats(a, height=None), feats(a, height=[0]), feats(a, width=[16385]), feats(a, image=[b[:-1]]),
            feats(a), feats(a, image=[]), feats(a, width=[]), feats(a, image=[b + b"xy"])]
    dec.decode(*write(recs))
    sp = W.Resize("image", size=(4, 4), channels=3, out="float16", fill=2.5, shapes=True)
    boxes = np.array([[0, 0, 6, 5]] * 5 + [[2, 2, 4, 4]] + [[0, 0, 6, 5]] * 3, np.int32)
    got, bits, shp = run(dec.resize, sp, 9, boxes=boxes)
    good = [0, 8]
    assert all((bits[k] == np.float16(2.5).view(np.uint16)).all() for k in range(9) if k not in good)
    for k in good:
        close(a, (0, 0, 6, 5), 0, sp, bits[k])
    assert got.stats["image"].tolist() == [6, 1, 1, 1]
    assert shp.tolist() == [[6, 5], [0, 5], [0, 5], [6, 16385], [6, 5], [6, 5], [6, 5], [6, 0], [6, 5]]


@pytest.mark.parametrize("out", ["same", "float32", "bfloat16"])
def test_constant_extents_nearest_mask(dec, out):
    """Nearest with constant extents: the source bits ("same"), or the taken element normalised (float
    outputs; exact in float64 with these scale and bias, so bits are compared)."""
    masks = make("uint8", 1, [(10, 14)] * 4, seed=3)
    dec.decode(*write([feats(a, height=None, width=None) for a in masks]))
    sp = W.Resize("image", size=(7, 5), height=10, width=14, out=out, interp="nearest", fill=9, scale=SCALE[0], bias=BIAS[0])
    flip = np.array([0, 1, 0, 1], np.uint8)
    _, bits, _ = run(dec.resize, sp, 4, boxes=np.array([[0, 0, 10, 14], [0, 0, 10, 14], [1, 2, 9, 11], [3, 3, 1, 1]], np.int32), flip=flip)
    for k, (t, l, h, w) in enumerate([(0, 0, 10, 14), (0, 0, 10, 14), (1, 2, 9, 11), (3, 3, 1, 1)]):
        iy = np.minimum(((2 * np.arange(7) + 1) * h) // 14, h - 1)
        ox = 4 - np.arange(5) if flip[k] else np.arange(5)
        take = masks[k][t : t + h, l : l + w][iy][:, np.minimum(((2 * ox + 1) * w) // 10, w - 1)]
        y = (take.astype(np.float64) * sp.scale[0] + sp.bias[0]).astype(np.float32)
        assert np.array_equal(bits[k], take if out == "same" else y.view(np.uint32) if out == "float32" else W.bf16_bits(y).reshape(y.shape))


def test_a_decoder_that_never_saw_the_height_key():
    """The image is there, its height key has no column: fill rows that count as bad shapes only, on the
    device (which has no extent to report) and on the host (which reads the width)."""
    imgs = make("uint8", 1, [(4, 4)] * 3)
    fresh = hip.HipDecoder(0)
    try:
        res = fresh.decode(*write([feats(a, height=None) for a in imgs]))
        sp = W.Resize("image", size=(2, 2), fill=3, shapes=True)
        got, bits, shp = run(fresh.resize, sp, 3)
        host = res.resize([sp])
        assert (bits.view(np.float32) == 3).all() and not shp.any() and got.stats["image"].tolist() == [3, 0, 0, 0]
        assert (host["image"] == 3).all() and host.shapes["image"].tolist() == [[0, 4]] * 3 and host.stats["image"].tolist() == [3, 0, 0, 0]
    finally:
        fresh.close()


def test_shard_decoder_two_batches():
    import torch

    imgs = make("uint8", 3, [(7 + i % 2, 6 - i % 2) for i in range(48)], seed=5)
    buf, st, en = write([feats(a) for a in imgs])
    sd = shard.ShardDecoder(0, int(buf.size) // 2 + 256, 2, balanced=False)
    try:
        plan = sd.plan(st, en, int(buf.size))
        assert len(plan) == 2
        rst, ren = sd.rebase(plan, st, en)
        d_bytes = torch.zeros(((buf.size + 15) // 16) * 16 + 16, dtype=torch.uint8, device=dev())
        d_bytes[: buf.size].copy_(torch.from_numpy(buf.copy()))
        d_st, d_en = torch.from_numpy(rst.view(np.int64)).to(dev()), torch.from_numpy(ren.view(np.int64)).to(dev())
        sd.learn(plan, buf, st, en)
        sd.decode_device(plan, d_bytes.data_ptr(), d_st.data_ptr(), d_en.data_ptr())
        sp = W.Resize("image", size=(6, 6), channels=3, out="bfloat16", planar=True, scale=SCALE[:3], bias=BIAS[:3])
        rows = np.random.default_rng(0).permutation(48)[:30].tolist() + [48]
        got, bits, _ = run(lambda specs, **kw: sd.resize(plan, specs, **kw), sp, 31, rows=np.array(rows), flip=np.arange(31, dtype=np.uint8) % 2)
        for k, r in enumerate(rows[:-1]):
            close(imgs[r], (0, 0, *imgs[r].shape[:2]), k % 2, sp, bits[k])
        assert (np.ascontiguousarray(bits[30]).view(np.uint8) == POISON).all() and got.skipped == 1 and got.stats["image"].tolist() == [0, 0, 0, 0]
    finally:
        sd.close()


def test_refusals_leave_the_outputs_alone(dec):
    import torch

    a = make("uint8", 1, [(4, 4)])[0]
    dec.decode(*write([feats(a)] * 4))
    good = W.Resize("image", size=(4, 4))
    big = torch.full((1024,), POISON, dtype=torch.uint8, device=dev())
    slot, hs, ws = W._resize_slots(dec, good)

    def call(n_specs=1, rows_dtype=N.ROWS_I64, m=4, **over):
        arr = (N.TfrgResizeSpec * 17)()
        for s in arr:
            s.slot, s.src, s.out, s.channels, s.h_slot, s.w_slot, s.out_h, s.out_w = slot, N.RAW_U8, N.RAW_OUT_F32, 1, hs, ws, 4, 4
            s.out_ptr = big.data_ptr() + 256
            for k, v in over.items():
                setattr(s, k, v)
        rc = dec._lib.tfrg_result_raw_resize(dec._ctx, arr, n_specs, C.c_void_p(big.data_ptr()), rows_dtype, m, 0, None, None, None, None, None)
        assert rc == -1 and b"tfrg_result_raw_resize" in dec._lib.tfrg_last_error()

    for kw in (dict(n_specs=0), dict(n_specs=17), dict(slot=hs), dict(slot=1 << 20), dict(src=8), dict(out=4), dict(h_slot=slot),
               dict(w_slot=1 << 20), dict(h_slot=N.RESIZE_CONST, src_h=0), dict(w_slot=N.RESIZE_CONST, src_w=16385), dict(out_h=0),
               dict(out_w=4097), dict(out_w=2048, channels=3), dict(channels=0), dict(channels=5), dict(interp=2),
               dict(out=N.RAW_OUT_SAME), dict(out_ptr=None), dict(out_ptr=big.data_ptr() + 2), dict(reserved=1), dict(rows_dtype=2),
               dict(m=1 << 31)):
        call(**kw)
    torch.cuda.synchronize()
    assert (big.cpu().numpy() == POISON).all()
