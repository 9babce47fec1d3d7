"""Resized raw images without a GPU: ``Resize``'s validation, and ``BatchResult.resize`` (the numpy host
path, over a host decode) against references that use no code of ``tfr_reader.raw``: for bilinear,
``torch.nn.functional.interpolate`` in float64 on the cropped array, mirrored after the resize for a
flipped row, then ``* scale + bias`` in float64; for nearest, a numpy index take.

The float32 bound. Let A be the largest ``|v|`` of the row's crop window and u = 2^-24 (half an ulp,
relative). The kernel's arithmetic (include/tfrg.h) rounds fx and fy once each (u relative, on a weight
that multiplies a difference of at most 2A), the two lerp fused multiply-adds once each (results of at most
A: u A each), ``h1 - h0`` once, and ``v[i1] - v[i0]`` once for float sources (integers below 2^24 subtract
exactly; differences of at most 2A: 2 u A each, weighted by f < 1). That is at most (2 + 2 + 1 + 1 + 2 + 2)
u A = 10 u A = 1.25 * 2^-21 * A before the normalise, which scales it by |scale| and whose own fma adds
u (A |scale| + |bias|): 11 u A |scale| + u |bias| in all, below 1.4 * 2^-21 * (A |scale| + |bias|). The
asserted 2^-20 * (A |scale[c]| + |bias[c]|) is about 1.45 times that worst case. float16 / bfloat16 add
one ulp of the output type at the value's magnitude: a perturbed value may round to the neighbour."""

import numpy as np
import pytest

from tests import _columns
from tfr_reader import raw as W
from tfr_reader import synth, writer

SCALE, BIAS = (3 / 256, 1.25, -0.5, 0.75), (-0.5, 0.25, 1.5, -2.0)
ULP = {"float16": 2.0 ** -10, "bfloat16": 2.0 ** -7}
# (H, W, box or None, flip): upscale, a downscale that skips rows, 1x1, single rows and columns, boxes that
# touch the edges, a 1-pixel box
IMAGES = [(5, 7, None, 0), (37, 53, None, 1), (1, 1, None, 0), (1, 9, None, 1), (9, 1, None, 0), (20, 31, (3, 4, 11, 13), 1),
          (20, 31, (0, 0, 20, 5), 0), (20, 31, (15, 26, 5, 5), 1), (20, 31, (7, 30, 1, 1), 0), (16, 12, None, 0)]


def ref64(img, box, flip, size, scale, bias):
    """The bilinear reference, float64 ``[OH, OW, C]``."""
    import torch

    t, l, h, w = box
    x = torch.from_numpy(np.ascontiguousarray(img[t : t + h, l : l + w].astype(np.float64))).permute(2, 0, 1)[None]
    y = torch.nn.functional.interpolate(x, size=size, mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()
    return (y[:, ::-1] if flip else y) * np.asarray(scale, np.float64) + np.asarray(bias, np.float64)


def tolerance(img, box, want, out, scale, bias):
    """The bound of the module's docstring, per element of ``want``; A is taken over the crop window."""
    t, l, h, w = box
    a = float(np.abs(img[t : t + h, l : l + w].astype(np.float64)).max())
    tol = 2.0 ** -20 * (a * np.abs(np.asarray(scale, np.float64)) + np.abs(np.asarray(bias, np.float64))) + 0 * want
    return tol if out == "float32" else tol + ULP[out] * 2.0 ** np.floor(np.log2(np.maximum(np.abs(want), 2.0 ** -14)))


def as_float(bits, out):
    """Output values as float64 (bfloat16 comes as its uint16 bits)."""
    if out == "bfloat16":
        return (np.asarray(bits).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return np.asarray(bits).astype(np.float64)


def images(src, C, seed=0):
    rng = np.random.default_rng(seed)
    dt = W.SRC[src][1]
    if np.dtype(dt).kind == "f":
        return [rng.uniform(-8, 8, (h, w, C)).astype(dt) for h, w, _, _ in IMAGES]
    lo, hi = {"uint8": (0, 256), "int16": (-32768, 32768)}[src]
    return [rng.integers(lo, hi, (h, w, C)).astype(dt) for h, w, _, _ in IMAGES]


def payloads(imgs, pad=lambda i: i):
    return [writer.encode_example([("pre", "bytes_list", [b"p" * pad(i)]), ("image", "bytes_list", [a.tobytes()]),
                                   ("height", "int64_list", [a.shape[0]]), ("width", "int64_list", [a.shape[1]])])
            for i, a in enumerate(imgs)]


@pytest.mark.parametrize("kw,exc", [
    (dict(src="uint4"), ValueError), (dict(out="int8"), ValueError), (dict(size=(0, 4)), ValueError), (dict(size=(4,)), ValueError),
    (dict(size=(4, 4097)), ValueError), (dict(size=(4, 2048), channels=3), ValueError), (dict(channels=5), ValueError),
    (dict(channels=0), ValueError), (dict(height=0), ValueError), (dict(width=16385), ValueError), (dict(height=1.5), TypeError),
    (dict(interp="bicubic"), ValueError), (dict(out="same"), ValueError), (dict(out="same", interp="nearest", fill=256), ValueError),
    (dict(channels=3, scale=(1, 2)), ValueError), (dict(bias=float("inf")), ValueError), (dict(key=b"image"), TypeError),
])
def test_resize_validation(kw, exc):
    with pytest.raises(exc):
        W.Resize(**{"key": "image", "size": (4, 4), **kw})


def test_normalize_and_shapes():
    sp = W.Resize.normalize("image", [0.5, 0.25], [0.25, 0.5], size=(3, 5), channels=2, planar=True, height=7, width="w")
    assert sp.scale == (4.0, 2.0) and sp.bias == (-2.0, -0.5) and sp.out_shape == (2, 3, 5) and sp.height == 7
    assert W.Resize("image", size=(3, 5), channels=2).out_shape == (3, 5, 2)


@pytest.mark.parametrize("src,out,C,planar,size", [("uint8", "float32", 3, True, (16, 12)), ("int16", "bfloat16", 1, False, (8, 8)),
                                                   ("float32", "float16", 4, False, (1, 5)), ("uint8", "float32", 3, False, (7, 1))])
def test_batch_resize_bilinear_against_torch(src, out, C, planar, size):
    imgs = images(src, C)
    res = _columns.batch_from_oracle(*synth.framed(payloads(imgs)))
    sp = W.Resize("image", size=size, src=src, out=out, channels=C, planar=planar, scale=SCALE[:C], bias=BIAS[:C], shapes=True)
    boxes = [b or (0, 0, h, w) for h, w, b, _ in IMAGES]
    got = res.resize([sp], boxes=boxes, flip=[f for *_, f in IMAGES])
    assert got.stats["image"].tolist() == [0, 0, 0, 0] and got.shapes["image"].tolist() == [[h, w] for h, w, _, _ in IMAGES]
    for k, (img, box) in enumerate(zip(imgs, boxes)):
        want = ref64(img, box, IMAGES[k][3], size, SCALE[:C], BIAS[:C])
        have = as_float(got["image"][k], out)
        have = have.transpose(1, 2, 0) if planar else have
        err = np.abs(have - want)
        assert (err <= tolerance(img, box, want, out, SCALE[:C], BIAS[:C])).all(), (k, err.max())


def test_batch_resize_nearest_and_bad_rows():
    imgs = images("uint8", 2, 3)
    pl = payloads(imgs)
    pl[2] = writer.encode_example([("image", "bytes_list", [imgs[2].tobytes()]), ("width", "int64_list", [1])])  # no height
    pl[3] = writer.encode_example([("image", "bytes_list", [imgs[3].tobytes()[:-1]]), ("height", "int64_list", [1]),
                                   ("width", "int64_list", [9])])  # one byte short
    pl[4] = writer.encode_example([("image", "bytes_list", [imgs[4].tobytes() + b"x"]), ("height", "int64_list", [9]),
                                   ("width", "int64_list", [1])])  # longer: decodes
    res = _columns.batch_from_oracle(*synth.framed(pl))
    sp = W.Resize("image", size=(6, 5), channels=2, out="same", interp="nearest", fill=7)
    rows = [0, 1, 2, 3, 4, 5, 5]
    boxes = [(0, 0, 5, 7), (1, 2, 30, 40), (0, 0, 1, 1), (0, 0, 1, 9), (0, 0, 9, 1), (3, 4, 11, 13), (3, 4, 11, 28)]
    flip = [0, 1, 0, 0, 0, 1, 0]
    got = res.resize([sp], rows=rows, boxes=boxes, flip=flip)
    assert got.stats["image"].tolist() == [2, 1, 0, 1]
    for k, g in enumerate(rows):
        if k in (2, 3, 6):
            assert (got["image"][k] == 7).all()
            continue
        t, l, h, w = boxes[k]
        oy, ox = np.arange(6), np.arange(5)
        iy = np.minimum(((2 * oy + 1) * h) // 12, h - 1)
        ix = np.minimum(((2 * (4 - ox if flip[k] else ox) + 1) * w) // 10, w - 1)
        assert np.array_equal(got["image"][k], imgs[g][t : t + h, l : l + w][iy][:, ix])


@pytest.mark.parametrize("out", ["float32", "bfloat16"])
def test_batch_resize_nearest_to_float(out):
    """Nearest with a float output: the taken element, normalised in float64 and rounded once."""
    imgs = images("int16", 3, 4)
    res = _columns.batch_from_oracle(*synth.framed(payloads(imgs)))
    sp = W.Resize("image", size=(6, 5), src="int16", out=out, channels=3, interp="nearest", scale=SCALE[:3], bias=BIAS[:3])
    boxes = [b or (0, 0, h, w) for h, w, b, _ in IMAGES]
    got = res.resize([sp], boxes=boxes, flip=[f for *_, f in IMAGES])
    for k, (img, (t, l, h, w)) in enumerate(zip(imgs, boxes)):
        ox = 4 - np.arange(5) if IMAGES[k][3] else np.arange(5)
        take = img[t : t + h, l : l + w][np.minimum(((2 * np.arange(6) + 1) * h) // 12, h - 1)][:, np.minimum(((2 * ox + 1) * w) // 10, w - 1)]
        y = (take.astype(np.float64) * np.asarray(sp.scale) + np.asarray(sp.bias)).astype(np.float32)
        assert np.array_equal(got["image"][k], y if out == "float32" else W.bf16_bits(y).reshape(y.shape))


def test_spec_mirror_size():
    import ctypes

    from tfr_reader import _native as N

    assert ctypes.sizeof(N.TfrgResizeSpec) == 104
