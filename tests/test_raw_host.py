"""Raw tensors from bytes features without a GPU: ``Raw``'s validation, ``BatchResult.raw`` (the numpy
host path, over a host decode) against an expectation computed from the test's own arrays, and the ctypes
mirror of tfrg_raw_spec against the header's layout."""

import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tfr_reader import _native as N
from tests import _columns
from tfr_reader import synth, writer
from tfr_reader import raw as W

INCLUDE = Path(__file__).resolve().parents[1] / "include"


@pytest.mark.parametrize("kw,exc", [
    (dict(src="uint4"), ValueError), (dict(out="int8"), ValueError), (dict(shape=()), ValueError),
    (dict(shape=(0, 3)), ValueError), (dict(shape=(1 << 24, 2)), ValueError), (dict(channels=0), ValueError),
    (dict(channels=17, shape=(17,)), ValueError), (dict(shape=(5, 7), channels=3), ValueError),
    (dict(shape=(6, 2), channels=3, planar=True), ValueError), (dict(shape=(4, 3), channels=3, scale=(1, 2)), ValueError),
    (dict(bias=float("nan")), ValueError), (dict(out="same", fill=256), ValueError), (dict(key=b"t"), TypeError),
])
def test_raw_validation(kw, exc):
    with pytest.raises(exc):
        W.Raw(**{"key": "t", **kw})


def test_normalize_rounds_once():
    sp = W.Raw.normalize("t", [0.485, 0.456, 0.406], [0.229, 0.224, 0.225], shape=(2, 2, 3), channels=3, planar=True)
    assert sp.scale == tuple(float(np.float32(1 / s)) for s in (0.229, 0.224, 0.225))
    assert sp.bias == tuple(float(np.float32(-m / s)) for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)))
    assert sp.out_shape == (3, 2, 2) and sp.count == 12


@pytest.mark.parametrize("src,out,shape,C,planar", [
    ("uint8", "float32", (5, 7, 3), 3, True), ("int16", "float16", (40,), 1, False), ("float32", "bfloat16", (6, 4), 4, False)])
def test_batch_raw_against_the_arrays(src, out, shape, C, planar):
    rng = np.random.default_rng(1)
    count = int(np.prod(shape))
    arrs = [rng.integers(1, 100, count).astype(W.SRC[src][1]) for _ in range(6)]
    elems = [[a.tobytes()] for a in arrs]
    elems[1], elems[2], elems[3] = [elems[1][0][:-3]], [], [elems[3][0] + b"xyz", b"more"]
    payloads = [writer.encode_example([("t", "bytes_list", e), ("label", "int64_list", [i])]) for i, e in enumerate(elems)]
    payloads[4] = writer.encode_example([("label", "int64_list", [4])])
    buf, st, en = synth.framed(payloads)
    res = _columns.batch_from_oracle(buf, st, en)
    scale, bias = (3 / 256, 1.25, -0.5, 0.75)[:C], (-0.5, 0.25, 1.5, -2.0)[:C]
    sp = W.Raw("t", src=src, out=out, shape=shape, channels=C, planar=planar, scale=scale, bias=bias, fill=9, lengths=True)
    rows = [5, 0, 1, 1, 2, 3, 4]
    got = res.raw([sp], rows=rows)
    esz = W.ITEMSIZE[src]
    want = np.full((len(rows), count), 9.0, np.float64)
    lens = []
    for k, g in enumerate(rows):
        b = b"" if g == 4 or not elems[g] else elems[g][0]
        lens.append(len(b))
        a = np.frombuffer(b[: min(len(b) // esz, count) * esz], W.SRC[src][1]).astype(np.float64)
        ch = np.arange(a.size) % C
        want[k, : a.size] = (a * np.asarray(scale)[ch] + np.asarray(bias)[ch]).astype(np.float32)
    if planar:
        want = want.reshape(len(rows), -1, C).transpose(0, 2, 1)
    want = want.reshape(len(rows), *sp.out_shape).astype(np.float32)
    bits = got["t"]
    if out == "bfloat16":
        assert bits.dtype == np.uint16
        b32 = want.view(np.uint32).astype(np.uint64)
        assert np.array_equal(bits, ((b32 + 0x7FFF + ((b32 >> 16) & 1)) >> 16).astype(np.uint16).reshape(bits.shape))
    else:
        assert np.array_equal(bits, want.astype(bits.dtype))
    assert got.lengths["t"].tolist() == lens
    assert got.stats["t"].tolist() == [1, 4, 2, 1]  # (rows 1, 1, 2 and 4 are short)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_raw_spec_layout_matches_the_header(tmp_path):
    py = N.TfrgRawSpec
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "tfrg.h"', "int main(void) {",
             '  printf("%zu\\n", sizeof(tfrg_raw_spec));']
    lines += [f'  printf("%zu %zu\\n", offsetof(tfrg_raw_spec, {f}), sizeof(((tfrg_raw_spec*)0)->{f}));' for f, _ in py._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    subprocess.run(["gcc", "-I", str(INCLUDE), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == C.sizeof(py) == 176
    for line, (f, _) in zip(out[1:], py._fields_):
        assert tuple(int(x) for x in line.split()) == (getattr(py, f).offset, getattr(py, f).size), f
    assert (N.RAW_MAX_SPECS, N.RAW_MAX_COUNT, N.RAW_MAX_CHANNELS) == (16, 1 << 24, 16)


def test_python_tile_constants_are_the_kernels():
    """``tfr_reader.raw.tile_elems`` and the narrow-row threshold, from which the GPU tests pick their edge
    shapes, are the constants csrc/tfrg_raw.h builds k_raw with."""
    import re

    hdr = (INCLUDE.parent / "tfrecords-reader_amd" / "csrc" / "tfrg_raw.h").read_text()
    assert int(re.search(r"kRawTile = (\d+);", hdr).group(1)) == N.RAW_TILE
    assert int(re.search(r"kRawNarrow = (\d+);", hdr).group(1)) == N.RAW_NARROW
    assert "return (kRawTile / channels) & ~15u;" in hdr
    assert [W.tile_elems(c) for c in (1, 3, 4, 16)] == [4096, 4080, 4096, 4096]
