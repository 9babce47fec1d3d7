"""Antialiased resize on the device (tfrg_result_raw_resize with TFRG_RESIZE_ANTIALIAS: k_resize_aa) against
the float64 weight-matrix reference and the bound of tests/test_resize_aa_host.py. Outputs lie inside
0xA5-poisoned buffers with guards, and the images start at every 16-byte residue (``run`` and ``write`` of
tests/test_resize_gpu.py)."""

import ctypes as C

import numpy as np
import pytest

from tests.test_resize_aa_host import close_aa
from tests.test_resize_gpu import POISON, POISON32, ROWS, SHAPES, dec, dev, feats, make, run, write  # noqa: F401
from tests.test_resize_host import BIAS, IMAGES, SCALE
from tfr_reader import _native as N
from tfr_reader import raw as W
from tfr_reader import shard

pytestmark = pytest.mark.gpu

B, G = N.RESIZE_AA_BAND, N.RESIZE_AA_GROUP
GEO = [((0, 0, *SHAPES[g]), 0) if g >= len(IMAGES) else (IMAGES[g][2] or (0, 0, *SHAPES[g]), IMAGES[g][3])
       for g in (r if 0 <= r < 17 else 0 for r in ROWS)]
GEO[1] = ((12, 0, 8, 31), 1)  # record 5 drawn twice: another crop, mirrored


@pytest.mark.parametrize("src,out,C,planar", [("uint8", "float32", 3, True), ("uint8", "bfloat16", 4, True), ("int16", "float16", 1, False),
                                              ("float32", "float32", 3, False)])
@pytest.mark.parametrize("size", [(16, 12), (8, 8), (1, 13), (13, 1), (3, 3)])
def test_mixed_shapes_boxes_flips_and_row_lists(dec, src, out, C, planar, size):
    imgs = make(src, C)
    dec.decode(*write([feats(a) for a in imgs]))
    sp = W.Resize("image", size=size, src=src, out=out, channels=C, planar=planar, scale=SCALE[:C], bias=BIAS[:C], shapes=True,
                  antialias=True)
    got, bits, shp = run(dec.resize, sp, len(ROWS), rows=np.array(ROWS, np.int64), boxes=np.array([b for b, _ in GEO], np.int32),
                         flip=np.array([f for _, f in GEO], np.uint8))
    for k, r in enumerate(ROWS):
        if not 0 <= r < 17:
            assert (np.ascontiguousarray(bits[k]).view(np.uint8) == POISON).all() and (shp[k] == POISON32).all()
            continue
        close_aa(imgs[r], GEO[k][0], GEO[k][1], sp, bits[k].view({"float32": np.float32, "float16": np.float16}.get(out, np.uint16)))
        assert shp[k].tolist() == list(SHAPES[r])
    assert got.stats["image"].tolist() == [0, 0, 0, 0] and got.skipped == 3


@pytest.mark.parametrize("oh", [1, B, B + 1, 2 * B + 1])
def test_band_and_group_seams(dec, oh):
    """Windows that straddle a band seam, a group seam and more than one group, at vertical ratios from an
    upscale to 5x."""
    heights = [G - 1, G, G + 1, 2 * G + 1, 5 * oh + 3, (23 * oh) // 10 + 1]
    imgs = make("uint8", 3, [(h, 20 + i) for i, h in enumerate(heights)], seed=oh)
    dec.decode(*write([feats(a) for a in imgs]))
    sp = W.Resize.normalize("image", [120.0, 110.0, 100.0], [60.0, 61.0, 62.0], size=(oh, 19), channels=3, out="bfloat16", planar=True,
                            antialias=True)
    _, bits, _ = run(dec.resize, sp, len(imgs))
    for k, a in enumerate(imgs):
        close_aa(a, (0, 0, *a.shape[:2]), 0, sp, bits[k])


@pytest.mark.parametrize("shape,size,boxes", [
    ((2, 8193), (3, 3), [(0, 1, 2, 8192), (0, 0, 2, 8193)]),     # a crop row of the limit: windows of thousands of taps
    ((2, 8193), (3, 4096), [(0, 1, 2, 8192), (0, 0, 2, 8193)]),  # the largest LDS, two or three taps
    ((100, 7), (3, 20), [(0, 0, 100, 7), (0, 0, 100, 8)]),       # a window taller than a group while x upscales
])
def test_limits(dec, shape, size, boxes):
    """The second box is one element too wide: a bad box, ``fill``, counted."""
    a = make("int16", 1, [shape])[0]
    dec.decode(*write([feats(a)]))
    sp = W.Resize("image", size=size, src="int16", scale=SCALE[0], bias=BIAS[0], fill=-7, antialias=True)
    got, bits, _ = run(dec.resize, sp, 2, rows=np.array([0, 0]), boxes=np.array(boxes, np.int32))
    close_aa(a, boxes[0], 0, sp, bits[0].view(np.float32))
    assert (bits[1] == np.float32(-7).view(np.uint32)).all() and got.stats["image"].tolist() == [0, 1, 0, 0]


def test_bad_rows_are_fill_and_counted(dec):
    a = make("uint8", 3, [(6, 5)])[0]
    b = a.tobytes()
    recs = [feats(a), feats(a, height=None), feats(a, height=[0]), feats(a, width=[16385]), feats(a, image=[b[:-1]]),
            feats(a), feats(a, image=[]), feats(a, width=[]), feats(a, image=[b + b"xy"])]
    dec.decode(*write(recs))
    sp = W.Resize("image", size=(4, 4), channels=3, out="float16", fill=2.5, shapes=True, antialias=True)
    boxes = np.array([[0, 0, 6, 5]] * 5 + [[2, 2, 4, 4]] + [[0, 0, 6, 5]] * 3, np.int32)
    got, bits, shp = run(dec.resize, sp, 9, boxes=boxes)
    assert all((bits[k] == np.float16(2.5).view(np.uint16)).all() for k in range(9) if k not in (0, 8))
    for k in (0, 8):
        close_aa(a, (0, 0, 6, 5), 0, sp, bits[k].view(np.float16))
    assert got.stats["image"].tolist() == [6, 1, 1, 1]
    assert shp.tolist() == [[6, 5], [0, 5], [0, 5], [6, 16385], [6, 5], [6, 5], [6, 5], [6, 0], [6, 5]]


@pytest.mark.parametrize("kw", [dict(interp=0x101), dict(interp=0x102), dict(interp=0x200), dict(interp=0x100, out=N.RAW_OUT_SAME)])
def test_refused_flags_leave_the_outputs_alone(dec, kw):
    import torch

    dec.decode(*write([feats(make("uint8", 1, [(4, 4)])[0])] * 4))
    slot, hs, ws = W._resize_slots(dec, W.Resize("image", size=(4, 4)))
    big = torch.full((1024,), POISON, dtype=torch.uint8, device=dev())
    s = N.TfrgResizeSpec(slot=slot, src=N.RAW_U8, out=N.RAW_OUT_F32, channels=1, h_slot=hs, w_slot=ws, out_h=4, out_w=4,
                         out_ptr=big.data_ptr() + 256)
    for k, v in kw.items():
        setattr(s, k, v)
    rc = dec._lib.tfrg_result_raw_resize(dec._ctx, C.byref(s), 1, None, 0, 4, 0, None, None, None, None, None)
    assert rc == -1 and b"tfrg_result_raw_resize" in dec._lib.tfrg_last_error()
    torch.cuda.synchronize()
    assert (big.cpu().numpy() == POISON).all()
    s.interp, s.out = N.RESIZE_BILINEAR | N.RESIZE_ANTIALIAS, N.RAW_OUT_F32  # (the accepted value writes)
    assert dec._lib.tfrg_result_raw_resize(dec._ctx, C.byref(s), 1, None, 0, 4, 0, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert (big[256:512].cpu().numpy() != POISON).any()


@pytest.mark.parametrize("via", ["decoder", "shard"])
def test_antialiased_and_plain_specs_share_a_call(dec, via):
    """Both kernels in one call, over the same slot, boxes and flips: the plain spec's bits are those of a
    call of its own; the antialiased one meets the reference. ``shard``: over two decoded batches."""
    import torch

    imgs = make("uint8", 3, [(17 + i % 5, 23 - i % 3) for i in range(48)], seed=7)
    buf, st, en = write([feats(a) for a in imgs])
    sd = None
    if via == "decoder":
        dec.decode(buf, st, en)
        call = dec.resize
    else:
        sd = shard.ShardDecoder(0, int(buf.size) // 2 + 256, 2, balanced=False)
        plan = sd.plan(st, en, int(buf.size))
        assert len(plan) == 2
        rst, ren = sd.rebase(plan, st, en)
        d_bytes = torch.zeros(((buf.size + 15) // 16) * 16 + 16, dtype=torch.uint8, device=dev())
        d_bytes[: buf.size].copy_(torch.from_numpy(buf.copy()))
        d_st, d_en = torch.from_numpy(rst.view(np.int64)).to(dev()), torch.from_numpy(ren.view(np.int64)).to(dev())
        sd.learn(plan, buf, st, en)
        sd.decode_device(plan, d_bytes.data_ptr(), d_st.data_ptr(), d_en.data_ptr())
        call = lambda specs, **kw: sd.resize(plan, specs, **kw)  # noqa: E731
    try:
        kw = dict(size=(6, 7), channels=3, out="bfloat16", planar=True, scale=SCALE[:3], bias=BIAS[:3])
        aa, plain = W.Resize("image", name="aa", antialias=True, **kw), W.Resize("image", name="plain", **kw)
        rows = np.random.default_rng(0).permutation(48)[:30]
        boxes = np.array([(1, 2, imgs[r].shape[0] - 2, imgs[r].shape[1] - 3) for r in rows], np.int32)
        geo = dict(rows=torch.from_numpy(rows).to(dev()), boxes=torch.from_numpy(boxes).to(dev()),
                   flip=torch.from_numpy(np.arange(30, dtype=np.uint8) % 2).to(dev()))
        both, alone = call([aa, plain], **geo), call([plain], **geo)
        assert torch.equal(both["plain"].view(torch.int16), alone["plain"].view(torch.int16))
        assert both.stats["aa"].tolist() == both.stats["plain"].tolist() == [0, 0, 0, 0] and both.skipped == 0
        have = both["aa"].view(torch.int16).cpu().numpy().view(np.uint16).transpose(0, 2, 3, 1)
        for k, r in enumerate(rows):
            close_aa(imgs[r], tuple(boxes[k]), k % 2, aa, have[k])
    finally:
        if sd is not None:
            sd.close()
