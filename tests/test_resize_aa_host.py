"""Antialiased resize (``Resize(antialias=True)``, TFRG_RESIZE_ANTIALIAS) without a GPU: the validation, and
``BatchResult.resize`` (the numpy host path) against a reference that uses no code of ``tfr_reader.raw``: two
dense float64 weight matrices from the formula of include/tfrg.h, ``want = (Wy / Sy) @ crop @ (Wx / Sx).T``
per channel, mirrored after the resize for a flipped row, then ``* scale + bias`` in float64. The reference
itself is pinned to torch's float64 ``interpolate(antialias=True)``.

The float32 bound. Let Th, Tv be the largest tap counts of the row's two axes, A the largest ``|v|`` of the
crop window and u = 2^-24. The weights are exact in float32 and positive, so an accumulation of T terms
``fmaf(w, v, acc)``, in any order, errs by at most T u A after the division by S; ``1 / (float)S`` and the
product add 2 u A per axis; float sources add u A per axis for nothing (``w v`` is fused); the normalise adds
u (A |scale| + |bias|). That is below (Th + Tv + 6) u (A |scale[c]| + |bias[c]|). Asserted: 2^-23 (Th + Tv +
8) (A |scale[c]| + |bias[c]|), twice the worst case, plus one ulp of float16 / bfloat16 at the value's
magnitude, as ``tests/test_resize_host.py`` adds it."""

import numpy as np
import pytest

from tests import _columns
from tests.test_resize_host import BIAS, IMAGES, SCALE, ULP, as_float, images, payloads
from tfr_reader import raw as W
from tfr_reader import synth


def weights(n, size):
    """(the normalised [size, n] float64 weights of an axis, its largest tap count)."""
    o, j = np.arange(size, dtype=np.int64)[:, None], np.arange(n, dtype=np.int64)[None, :]
    w = np.maximum(0, 2 * max(n, size) - np.abs((2 * j + 1) * size - (2 * o + 1) * n))
    return w / w.sum(1, keepdims=True), int((w > 0).sum(1).max())


def ref_aa(img, box, flip, size, scale, bias):
    """(the reference, float64 ``[OH, OW, C]``; Th + Tv)."""
    t, l, h, w = box
    (wy, tv), (wx, th) = weights(h, size[0]), weights(w, size[1])
    y = np.einsum("oy,yxc->oxc", wy, img[t : t + h, l : l + w].astype(np.float64))
    y = np.einsum("px,oxc->opc", wx, y)
    return (y[:, ::-1] if flip else y) * np.asarray(scale, np.float64) + np.asarray(bias, np.float64), th + tv


def tol_aa(img, box, want, taps, out, scale, bias):
    """The bound of the module's docstring, per element of ``want``."""
    t, l, h, w = box
    a = float(np.abs(img[t : t + h, l : l + w].astype(np.float64)).max())
    tol = 2.0 ** -23 * (taps + 8) * (a * np.abs(np.asarray(scale, np.float64)) + np.abs(np.asarray(bias, np.float64))) + 0 * want
    return tol if out == "float32" else tol + ULP[out] * 2.0 ** np.floor(np.log2(np.maximum(np.abs(want), 2.0 ** -14)))


def close_aa(img, box, flip, sp, have):
    """``have``: the output's values ``[OH, OW, C]`` (bfloat16 as bits)."""
    want, taps = ref_aa(img, box, flip, sp.size, sp.scale, sp.bias)
    err = np.abs(as_float(have, sp.out) - want)
    assert (err <= tol_aa(img, box, want, taps, sp.out, sp.scale, sp.bias)).all(), err.max()


@pytest.mark.parametrize("kw", [dict(interp="nearest"), dict(out="same"), dict(out="same", interp="nearest")])
def test_antialias_validation(kw):
    with pytest.raises(ValueError):
        W.Resize("image", size=(4, 4), antialias=True, **kw)
    assert W.Resize("image", size=(4, 4), antialias=1).antialias is True and not W.Resize("image", size=(4, 4)).antialias


@pytest.mark.parametrize("src,out,C,planar,size", [("uint8", "float32", 3, True, (16, 12)), ("int16", "bfloat16", 1, False, (8, 8)),
                                                   ("float32", "float16", 4, False, (1, 5)), ("uint8", "float32", 3, False, (7, 1))])
def test_batch_resize_antialias_against_the_formula(src, out, C, planar, size):
    imgs = images(src, C)
    res = _columns.batch_from_oracle(*synth.framed(payloads(imgs)))
    sp = W.Resize("image", size=size, src=src, out=out, channels=C, planar=planar, scale=SCALE[:C], bias=BIAS[:C], antialias=True)
    boxes = [b or (0, 0, h, w) for h, w, b, _ in IMAGES]
    got = res.resize([sp], boxes=boxes, flip=[f for *_, f in IMAGES])
    assert got.stats["image"].tolist() == [0, 0, 0, 0]
    for k, (img, box) in enumerate(zip(imgs, boxes)):
        close_aa(img, box, IMAGES[k][3], sp, got["image"][k].transpose(1, 2, 0) if planar else got["image"][k])


@pytest.mark.parametrize("size", [(16, 12), (8, 8), (1, 13), (3, 3)])
def test_the_formula_is_torchs_antialias(size):
    """out_w >= 2 only: torch's CPU antialias kernel deviates at out_w == 1, even from its own plain bilinear
    on a pure upscale, where the formula agrees with plain bilinear."""
    import torch

    for img, (h, w, box, _) in zip(images("uint8", 2, 1), IMAGES):
        t, l, bh, bw = box or (0, 0, h, w)
        x = torch.from_numpy(img[t : t + bh, l : l + bw].astype(np.float64)).permute(2, 0, 1)[None]
        y = torch.nn.functional.interpolate(x, size=size, mode="bilinear", align_corners=False, antialias=True)
        want, _ = ref_aa(img, (t, l, bh, bw), 0, size, 1.0, 0.0)
        assert np.abs(y[0].permute(1, 2, 0).numpy() - want).max() <= 1e-12 * 255
