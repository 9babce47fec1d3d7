"""Raw tensors from bytes features: ``tf.io.decode_raw`` + ``tf.cast`` + a per-channel normalise + an
HWC -> CHW transpose, for a list of rows of a decoded batch.

A ``Raw`` spec names a ``bytes_list`` key whose first element is a tensor stored as bytes
(``image.tobytes()``, int16 PCM, a float16 feature map): its source element type, the output type, the
shape, ``scale`` / ``bias`` per channel and whether the output is planar. Then

* ``HipDecoder.raw`` / ``ShardDecoder.raw`` write ``[m, *shape]`` (planar: ``[m, channels,
  *shape[:-1]]``) torch tensors on the device with one kernel per decoded batch (``tfrg_result_raw_rows``):
  one read of the element, one write of the output;
* ``BatchResult.raw`` computes the same function with numpy from fetched columns (the host path).

Per output: ``lengths[k]`` is the element's byte length (0: the list is empty or absent) and ``stats`` the
four counters of ``tfr_reader.dense`` with ``count * itemsize`` in the place of the width. Elements the
record does not have (a short or missing element; a trailing partial element counts as missing) are
``fill``, which is not transformed.

A ``Resize`` spec is for images whose size differs from record to record: the key's first element is an
``[H, W, channels]`` image, H and W are int64 features of the same record, and a crop box and a flip per
output row are resampled to one fixed size (``HipDecoder.resize`` / ``ShardDecoder.resize``: one
``tfrg_result_raw_resize`` launch per decoded batch; ``BatchResult.resize``: the host path).
"""

from __future__ import annotations

from collections.abc import Mapping, Sequence
from dataclasses import dataclass

import numpy as np

from tfr_reader import _native as N
from tfr_reader import dense as D

#: source type name -> (TFRG_RAW_* id, numpy dtype; None: bfloat16, which numpy does not have)
SRC = {
    "uint8": (N.RAW_U8, np.uint8), "int8": (N.RAW_I8, np.int8), "uint16": (N.RAW_U16, np.uint16),
    "int16": (N.RAW_I16, np.int16), "int32": (N.RAW_I32, np.int32), "float16": (N.RAW_F16, np.float16),
    "bfloat16": (N.RAW_BF16, None), "float32": (N.RAW_F32, np.float32),
}
ITEMSIZE = {"uint8": 1, "int8": 1, "uint16": 2, "int16": 2, "int32": 4, "float16": 2, "bfloat16": 2, "float32": 4}
#: output type name -> TFRG_RAW_OUT_* id
OUT = {"float32": N.RAW_OUT_F32, "float16": N.RAW_OUT_F16, "bfloat16": N.RAW_OUT_BF16, "same": N.RAW_OUT_SAME}


def tile_elems(channels: int = 1) -> int:
    """The elements of a row that one tile of the kernel covers (csrc/tfrg_raw.h)."""
    return ((N.RAW_TILE // channels) & ~15) * channels


def bf16_bits(a: np.ndarray) -> np.ndarray:
    """float32 -> bfloat16 bits (uint16), round to nearest even."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


@dataclass(frozen=True)
class Raw:
    """One raw-tensor output: element 0 of ``key``'s ``bytes_list`` as ``prod(shape)`` little-endian
    elements of ``src`` ("uint8", "int8", "uint16", "int16", "int32", "float16", "bfloat16", "float32"),
    each written as ``out`` ("float32", "float16", "bfloat16": ``x * scale[c] + bias[c]`` with one
    rounding, ``c`` the index along the last axis modulo ``channels``; "same": the source bits). The
    result is ``[m, *shape]``, or ``[m, channels, *shape[:-1]]`` with ``planar`` (then ``shape[-1]`` must
    be ``channels``). ``scale`` / ``bias``: a number or ``channels`` numbers. ``fill``: the value of the
    elements a record does not have, in the output type. ``lengths``: also return the byte lengths.
    ``name``: the output's name in the result (default: the key)."""

    key: str
    src: str = "uint8"
    out: str = "float32"
    shape: tuple = (1,)
    channels: int = 1
    scale: float | Sequence[float] = 1.0
    bias: float | Sequence[float] = 0.0
    planar: bool = False
    fill: float | int = 0
    lengths: bool = False
    name: str | None = None

    dtype = "uint8"  # (the slot kind, as ``Dense.dtype`` selects it)

    def __post_init__(self) -> None:
        if not isinstance(self.key, str):
            raise TypeError(f"Raw key must be a str, not {type(self.key).__name__}")
        if self.src not in SRC:
            raise ValueError(f"Raw({self.key!r}): src must be one of {sorted(SRC)}, not {self.src!r}")
        if self.out not in OUT:
            raise ValueError(f"Raw({self.key!r}): out must be one of {sorted(OUT)}, not {self.out!r}")
        shape = (self.shape,) if isinstance(self.shape, (int, np.integer)) else tuple(self.shape)
        if not shape or any(not isinstance(d, (int, np.integer)) or d < 1 for d in shape):
            raise ValueError(f"Raw({self.key!r}): shape must be a tuple of positive integers, not {self.shape!r}")
        object.__setattr__(self, "shape", tuple(int(d) for d in shape))
        if not 1 <= self.count <= N.RAW_MAX_COUNT:
            raise ValueError(f"Raw({self.key!r}): shape must hold 1..{N.RAW_MAX_COUNT} elements, not {self.count}")
        c = self.channels
        if not isinstance(c, (int, np.integer)) or not 1 <= int(c) <= N.RAW_MAX_CHANNELS:
            raise ValueError(f"Raw({self.key!r}): channels must be in 1..{N.RAW_MAX_CHANNELS}, not {c!r}")
        if self.count % int(c):
            raise ValueError(f"Raw({self.key!r}): {self.count} elements are not a multiple of {c} channels")
        if self.planar and self.shape[-1] != int(c):
            raise ValueError(f"Raw({self.key!r}): planar needs shape[-1] == channels, not {self.shape[-1]} and {c}")
        for what in ("scale", "bias"):
            object.__setattr__(self, what, channel_values(f"Raw({self.key!r})", what, getattr(self, what), int(c)))
        self.fill_bits  # noqa: B018 (validates the fill)

    @classmethod
    def normalize(cls, key: str, mean, std, **kw) -> Raw:
        """``(x - mean) / std`` per channel as ``scale = 1 / std``, ``bias = -mean / std``, computed in
        float64 and rounded once to float32."""
        mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
        return cls(key, scale=tuple((1.0 / std).reshape(-1)), bias=tuple((-mean / std).reshape(-1)), **kw)

    @property
    def out_name(self) -> str:
        return self.name if self.name is not None else self.key

    @property
    def count(self) -> int:
        return int(np.prod(self.shape, dtype=np.int64))

    @property
    def out_type(self) -> str:
        """The output's type name (``out``, or ``src`` for "same")."""
        return self.src if self.out == "same" else self.out

    @property
    def out_shape(self) -> tuple:
        return (int(self.channels), *self.shape[:-1]) if self.planar else self.shape

    @property
    def fill_bits(self) -> int:
        """The pad value's raw bits in the output type, as ``tfrg_raw_spec.fill`` takes them."""
        return fill_bits_of(f"Raw({self.key!r})", self.out_type, self.fill)


def fill_bits_of(who: str, t: str, fill) -> int:
    """``fill``'s raw bits in the output type named ``t`` (ValueError, naming ``who``, for an integer that
    does not fit)."""
    if t == "bfloat16":
        return int(bf16_bits(np.array([fill], np.float32))[0])
    dt = SRC[t][1]
    if np.dtype(dt).kind == "f":
        return int(np.array(fill, dt).view({2: np.uint16, 4: np.uint32}[np.dtype(dt).itemsize]))
    v, bits = int(fill), 8 * np.dtype(dt).itemsize
    if not -(1 << (bits - 1)) <= v < (1 << bits):
        raise ValueError(f"{who}: fill {v} does not fit {t}")
    return v & ((1 << bits) - 1)


def channel_values(who: str, what: str, v, c: int) -> tuple:
    """``scale`` / ``bias``: a number or ``c`` finite numbers, as ``c`` float32 values."""
    v = np.asarray(v, np.float64).reshape(-1)
    if v.size not in (1, c) or not np.isfinite(v).all():
        raise ValueError(f"{who}: {what} must be a number or {c} finite numbers")
    return tuple(float(x) for x in np.broadcast_to(v, (c,)).astype(np.float32))


def check_specs(specs: Sequence[Raw]) -> list[Raw]:
    specs = list(specs)
    if not 1 <= len(specs) <= N.RAW_MAX_SPECS:
        raise ValueError(f"between 1 and {N.RAW_MAX_SPECS} Raw specs per call, not {len(specs)}")
    seen = set()
    for s in specs:
        if not isinstance(s, Raw):
            raise TypeError(f"specs must be Raw objects, not {type(s).__name__}")
        if s.out_name in seen:
            raise ValueError(f"two Raw specs are named {s.out_name!r}: give one of them name=")
        seen.add(s.out_name)
    return specs


# ---------------------------------------------------------------------- host path (numpy)
def _np_out(sp: Raw):
    """(numpy dtype of the output's bits, numpy dtype it is returned as)."""
    t = sp.out_type
    if t == "bfloat16":
        return np.uint16, np.uint16  # (numpy has no bfloat16: the bits)
    return {1: np.uint8, 2: np.uint16, 4: np.uint32}[ITEMSIZE[t]], SRC[t][1]


def convert(sp: Raw, elem: np.ndarray) -> np.ndarray:
    """The output bits of the whole source elements of ``elem`` (uint8), at most ``count`` of them, in
    source order."""
    esz, ubits = ITEMSIZE[sp.src], _np_out(sp)[0]
    k = min(elem.size // esz, sp.count)
    b = np.ascontiguousarray(elem[: k * esz])
    if sp.out == "same":
        return b.view(ubits)
    if sp.src == "bfloat16":
        v = (b.view(np.uint16).astype(np.uint32) << 16).view(np.float32)
    else:
        v = b.view(np.dtype(SRC[sp.src][1]).newbyteorder("<")).astype(np.float32)
    c = np.arange(k) % int(sp.channels)
    # (one rounding, as fmaf: the float64 product of two float32 is exact, the sum rounds once more only
    # at a float32 rounding boundary)
    with np.errstate(all="ignore"):
        y = (v.astype(np.float64) * np.asarray(sp.scale, np.float64)[c] + np.asarray(sp.bias, np.float64)[c]).astype(np.float32)
        if sp.out == "float32":
            return y.view(np.uint32)
        return y.astype(np.float16).view(np.uint16) if sp.out == "float16" else bf16_bits(y)


def element0(res, base: int, rs: np.ndarray, g: int) -> tuple:
    """(the elements of record ``g``'s list, element 0's bytes: empty without one) from a fetched result."""
    lo, c = base + int(rs[g]), int(rs[g + 1] - rs[g])
    if not c:
        return 0, np.zeros(0, np.uint8)
    if res.bytes_data is not None:
        return c, res.bytes_data[int(res.bytes_offsets[lo]) : int(res.bytes_offsets[lo + 1])]
    o, ln = int(res.bytes_off[lo]), int(res.bytes_len[lo])
    elem = np.zeros(ln, np.uint8)  # (a view past the input reads zeros)
    got = res.buf[o : o + ln]
    elem[: got.size] = got
    return c, elem


def batch_raw(res, specs: Sequence[Raw], rows=None) -> D.DenseBatch:
    """``BatchResult.raw``: the outputs of ``specs`` from a fetched result's columns, record by record. A
    key without a slot gives all-``fill`` outputs. bfloat16 outputs are returned as their uint16 bits."""
    specs = check_specs(specs)
    n = len(res)
    picked = list(range(n)) if rows is None else D.host_rows(rows, n).tolist()
    m = len(picked)
    values, lengths, stats = {}, {}, {}
    for sp in specs:
        ubits, dt = _np_out(sp)
        count, C, width = sp.count, int(sp.channels), sp.count * ITEMSIZE[sp.src]
        out = np.full((m, count), sp.fill_bits, ubits)
        lens, st = np.zeros(m, np.int32), np.zeros(4, np.uint32)
        s = D.find_slot(res.slot_key, res.slot_kind, sp.key, 1)
        if s is None:
            st[1] = st[2] = m
        else:
            base, rs = int(res.slot_base[s]), np.asarray(res.row_splits[s]).astype(np.int64)
            for k, g in enumerate(picked):
                c, elem = element0(res, base, rs, g)
                ln = int(elem.size)
                if c:
                    v = convert(sp, elem)
                    out[k, : v.size] = v
                lens[k] = ln
                st += np.array([ln > width, ln < width, c == 0, c > 1], np.uint32)
        if sp.planar:
            out = out.reshape(m, count // C, C).transpose(0, 2, 1)
        values[sp.out_name] = np.ascontiguousarray(out).view(dt).reshape(m, *sp.out_shape)
        if sp.lengths:
            lengths[sp.out_name] = lens
        stats[sp.out_name] = st
    return D.DenseBatch(values, lengths, stats)


# ---------------------------------------------------------------------- resized images
INTERP = {"bilinear": N.RESIZE_BILINEAR, "nearest": N.RESIZE_NEAREST}
RESIZE_STAT_NAMES = ("bad_shape", "bad_box", "empty", "longer")


@dataclass(frozen=True)
class Resize:
    """One resized-image output: element 0 of ``key``'s ``bytes_list`` is an ``[H, W, channels]`` image of
    ``src`` elements whose H and W are value 0 of the int64 features ``height`` / ``width`` (a str: the
    key; an int: the same extent for every record). A per-row crop box, optionally mirrored left-right, is
    resampled to ``size = (OH, OW)`` (``interp``: "bilinear", half-pixel centres without antialiasing, or
    "nearest"), then ``x * scale[c] + bias[c]`` and one rounding to ``out``, as ``Raw``. The result is
    ``[m, OH, OW, channels]``, or ``[m, channels, OH, OW]`` with ``planar``. A record whose shape or box
    is unusable gives a row of ``fill``. ``shapes``: also return ``[m, 2]`` int32, each record's (H, W).
    ``out="same"`` (the source bits) goes with "nearest" only. ``antialias`` (with "bilinear" only): the
    triangle filter of include/tfrg.h on both axes, which filters a downscale instead of skipping samples
    (``F.interpolate(antialias=True)``, torchvision's ``Resize``, PIL's ``BILINEAR``); an upscaled axis then
    agrees with plain bilinear within rounding, not bit for bit."""

    key: str
    size: tuple = (1, 1)
    height: str | int = "height"
    width: str | int = "width"
    src: str = "uint8"
    out: str = "float32"
    channels: int = 1
    scale: float | Sequence[float] = 1.0
    bias: float | Sequence[float] = 0.0
    interp: str = "bilinear"
    planar: bool = False
    fill: float | int = 0
    shapes: bool = False
    name: str | None = None
    antialias: bool = False

    dtype = "uint8"  # (the slot kind, as ``Dense.dtype`` selects it)

    def __post_init__(self) -> None:
        who = f"Resize({self.key!r})"
        if not isinstance(self.key, str):
            raise TypeError(f"Resize key must be a str, not {type(self.key).__name__}")
        if self.src not in SRC:
            raise ValueError(f"{who}: src must be one of {sorted(SRC)}, not {self.src!r}")
        if self.out not in OUT:
            raise ValueError(f"{who}: out must be one of {sorted(OUT)}, not {self.out!r}")
        if self.interp not in INTERP:
            raise ValueError(f"{who}: interp must be one of {sorted(INTERP)}, not {self.interp!r}")
        if self.out == "same" and self.interp != "nearest":
            raise ValueError(f"{who}: out='same' copies bits and goes with interp='nearest' only")
        if self.antialias and self.interp != "bilinear":
            raise ValueError(f"{who}: antialias filters and goes with interp='bilinear' only")
        object.__setattr__(self, "antialias", bool(self.antialias))
        c = self.channels
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 1 <= int(c) <= N.RESIZE_MAX_CHANNELS:
            raise ValueError(f"{who}: channels must be in 1..{N.RESIZE_MAX_CHANNELS}, not {c!r}")
        object.__setattr__(self, "channels", int(c))
        size = tuple(self.size) if isinstance(self.size, (tuple, list)) else ()
        if len(size) != 2 or any(not isinstance(d, (int, np.integer)) or not 1 <= d <= N.RESIZE_MAX_OUT for d in size):
            raise ValueError(f"{who}: size must be (OH, OW) with both in 1..{N.RESIZE_MAX_OUT}, not {self.size!r}")
        if int(size[1]) * int(c) > N.RESIZE_MAX_OUT:
            raise ValueError(f"{who}: OW * channels must be at most {N.RESIZE_MAX_OUT}, not {int(size[1]) * int(c)}")
        object.__setattr__(self, "size", (int(size[0]), int(size[1])))
        for what in ("height", "width"):
            v = getattr(self, what)
            if isinstance(v, bool) or not isinstance(v, (str, int, np.integer)):
                raise TypeError(f"{who}: {what} must be a key (str) or an int, not {type(v).__name__}")
            if not isinstance(v, str):
                if not 1 <= int(v) <= N.RESIZE_MAX_SRC:
                    raise ValueError(f"{who}: a constant {what} must be in 1..{N.RESIZE_MAX_SRC}, not {v}")
                object.__setattr__(self, what, int(v))
        for what in ("scale", "bias"):
            object.__setattr__(self, what, channel_values(who, what, getattr(self, what), int(c)))
        self.fill_bits  # noqa: B018 (validates the fill)

    @classmethod
    def normalize(cls, key: str, mean, std, **kw) -> Resize:
        """``(x - mean) / std`` per channel, as ``Raw.normalize``."""
        mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
        return cls(key, scale=tuple((1.0 / std).reshape(-1)), bias=tuple((-mean / std).reshape(-1)), **kw)

    @property
    def out_name(self) -> str:
        return self.name if self.name is not None else self.key

    @property
    def out_type(self) -> str:
        return self.src if self.out == "same" else self.out

    @property
    def out_shape(self) -> tuple:
        (oh, ow), c = self.size, self.channels
        return (c, oh, ow) if self.planar else (oh, ow, c)

    @property
    def count(self) -> int:
        return self.size[0] * self.size[1] * self.channels

    @property
    def fill_bits(self) -> int:
        return fill_bits_of(f"Resize({self.key!r})", self.out_type, self.fill)


def axis_coords(n: int, size: int, interp: str, flip: bool = False) -> tuple:
    """(i0, i1, f) of the ``size`` output positions along a source axis of ``n`` samples, in the integers
    of include/tfrg.h (tfrg_result_raw_resize): half-pixel centres; ``flip``: position o reads as size - 1 - o."""
    o = np.arange(size, dtype=np.int64)
    if flip:
        o = size - 1 - o
    if interp == "nearest":
        i = np.minimum(((2 * o + 1) * n) // (2 * size), n - 1)
        return i, i, np.zeros(size, np.float32)
    num, den = (2 * o + 1) * n - size, 2 * size
    neg = num < 0
    i0 = np.where(neg, 0, num // den)
    f = np.where(neg, np.float32(0), (num % den).astype(np.float32) / np.float32(den)).astype(np.float32)
    edge = i0 >= n - 1
    i0 = np.where(edge, n - 1, i0)
    return i0, np.where(edge, n - 1, i0 + 1), np.where(edge, np.float32(0), f).astype(np.float32)


def _fma32(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """fmaf on float32 arrays (the float64 product of two float32 is exact; see ``convert``)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def axis_windows(n: int, size: int, flip: bool = False) -> tuple:
    """(j0, cnt, d0, inv) of the ``size`` antialiased output positions along a source axis of ``n`` samples,
    in the integers of include/tfrg.h: the window's first tap and tap count, d = (2 j0 + 1) N - (2 o + 1) n
    of the first tap (the next tap's is 2N more; a tap's weight is 2M - |d|) and float32 1 / (float32)S."""
    o = np.arange(size, dtype=np.int64)
    if flip:
        o = size - 1 - o
    big, c = max(n, size), (2 * o + 1) * n
    j0 = np.maximum((c - 2 * big - size) // (2 * size) + 1, 0)
    j1 = np.minimum((c + 2 * big - size - 1) // (2 * size), n - 1)
    d0 = (2 * j0 + 1) * size - c
    tot = [int((2 * big - np.abs(d + 2 * size * np.arange(k))).sum()) for d, k in zip(d0, j1 - j0 + 1)]
    return j0, j1 - j0 + 1, d0, np.float32(1) / np.array(tot, np.int64).astype(np.float32)


def _filter_axis(v: np.ndarray, n: int, size: int, flip: bool) -> np.ndarray:
    """float32 ``v`` ``[n, ...]`` filtered along axis 0 to ``[size, ...]``: per output a sequential float32
    accumulation of fmaf(w, v, acc) over the window, times 1 / S."""
    j0, cnt, d0, inv = axis_windows(n, size, flip)
    out = np.zeros((size, *v.shape[1:]), np.float32)
    big = 2 * max(n, size)
    for o in range(size):
        acc = np.zeros(v.shape[1:], np.float32)
        for j in range(int(cnt[o])):
            w = np.float32(big - abs(int(d0[o]) + 2 * size * j))
            acc = _fma32(np.broadcast_to(w, acc.shape), v[int(j0[o]) + j], acc)
        out[o] = acc * inv[o]
    return out


def resample(sp: Resize, img: np.ndarray, box: tuple, flip: bool) -> np.ndarray:
    """The output bits ``[OH, OW, channels]`` of the crop ``box`` = (top, left, height, width) of ``img``
    (``[H, W, channels]`` of the source type; bfloat16 as uint16 bits), in the kernel's arithmetic."""
    (oh, ow), ubits = sp.size, _np_out(sp)[0]
    top, left, ch, cw = box
    y0, y1, fy = axis_coords(ch, oh, sp.interp)
    x0, x1, fx = axis_coords(cw, ow, sp.interp, flip)
    crop = img[top : top + ch, left : left + cw]
    if sp.out == "same":
        return crop[y0][:, x0].view(ubits)
    v = (crop.astype(np.uint32) << 16).view(np.float32) if sp.src == "bfloat16" else crop.astype(np.float32)
    with np.errstate(all="ignore"):
        if sp.antialias:
            h = _filter_axis(np.ascontiguousarray(v.transpose(1, 0, 2)), cw, ow, flip)  # ([OW, ch, C])
            r = _filter_axis(np.ascontiguousarray(h.transpose(1, 0, 2)), ch, oh, False)
        elif sp.interp == "nearest":
            r = v[y0][:, x0]
        else:
            a, b = v[:, x0], v[:, x1]
            h = _fma32(fx[None, :, None], b - a, a)  # (every crop row; the kernel visits the tapped ones)
            r = _fma32(fy[:, None, None], h[y1] - h[y0], h[y0])
        y = _fma32(r, np.asarray(sp.scale, np.float32), np.asarray(sp.bias, np.float32))
        if sp.out == "float32":
            return y.view(np.uint32)
        return y.astype(np.float16).view(np.uint16) if sp.out == "float16" else bf16_bits(y).reshape(y.shape)


def _extent(res, what, g: int):
    """Record ``g``'s height or width: the constant, or value 0 of the int64 key (None: no value)."""
    if not isinstance(what, str):
        return int(what)
    s = D.find_slot(res.slot_key, res.slot_kind, what, 3)
    if s is None:
        return None
    rs = np.asarray(res.row_splits[s]).astype(np.int64)
    return int(res.i64[int(res.slot_base[s]) + int(rs[g])]) if rs[g + 1] > rs[g] else None


def check_resize_specs(specs: Sequence[Resize]) -> list[Resize]:
    specs = list(specs)
    if not 1 <= len(specs) <= N.RESIZE_MAX_SPECS:
        raise ValueError(f"between 1 and {N.RESIZE_MAX_SPECS} Resize specs per call, not {len(specs)}")
    seen = set()
    for s in specs:
        if not isinstance(s, Resize):
            raise TypeError(f"specs must be Resize objects, not {type(s).__name__}")
        if s.out_name in seen:
            raise ValueError(f"two Resize specs are named {s.out_name!r}: give one of them name=")
        seen.add(s.out_name)
    return specs


def batch_resize(res, specs: Sequence[Resize], rows=None, boxes=None, flip=None) -> D.DenseBatch:
    """``BatchResult.resize``: the outputs of ``specs`` from a fetched result's columns, row by row, with the
    integer coordinates and float32 arithmetic of the kernel. ``boxes``: ``[m, 4]`` (top, left, height,
    width) per output row; ``flip``: ``[m]``. ``.stats[name]``: ``RESIZE_STAT_NAMES``; ``.shapes[name]``
    where asked. bfloat16 outputs are returned as their uint16 bits."""
    specs = check_resize_specs(specs)
    n = len(res)
    picked = list(range(n)) if rows is None else D.host_rows(rows, n).tolist()
    m = len(picked)
    boxes = None if boxes is None else np.asarray(boxes, np.int64).reshape(m, 4)
    flip = None if flip is None else np.asarray(flip).reshape(m) != 0
    values, shapes, stats = {}, {}, {}
    for sp in specs:
        ubits, dt = _np_out(sp)
        (oh, ow), C, esz = sp.size, sp.channels, ITEMSIZE[sp.src]
        out = np.full((m, oh, ow, C), sp.fill_bits, ubits)
        shp, st = np.zeros((m, 2), np.int32), np.zeros(4, np.uint32)
        s = D.find_slot(res.slot_key, res.slot_kind, sp.key, 1)
        base = int(res.slot_base[s]) if s is not None else 0
        rs = np.asarray(res.row_splits[s]).astype(np.int64) if s is not None else None
        for k, g in enumerate(picked):
            c, elem = element0(res, base, rs, g) if s is not None else (0, np.zeros(0, np.uint8))
            H, W = _extent(res, sp.height, g), _extent(res, sp.width, g)
            shp[k] = [np.clip(v or 0, -(1 << 31), (1 << 31) - 1) for v in (H, W)]
            st[2] += c == 0
            sized = H is not None and W is not None and 1 <= H <= N.RESIZE_MAX_SRC and 1 <= W <= N.RESIZE_MAX_SRC
            st[3] += bool(sized and elem.size > H * W * C * esz)
            if not sized or H * W * C * esz > elem.size:
                st[0] += 1
                continue
            top, left, ch, cw = (0, 0, H, W) if boxes is None else (int(v) for v in boxes[k])
            if (ch <= 0 or cw <= 0 or top < 0 or left < 0 or top + ch > H or left + cw > W
                    or cw * C * esz > N.RESIZE_MAX_ROW_BYTES):
                st[1] += 1
                continue
            src_dt = np.uint16 if sp.src == "bfloat16" else np.dtype(SRC[sp.src][1]).newbyteorder("<")
            img = np.ascontiguousarray(elem[: H * W * C * esz]).view(src_dt).reshape(H, W, C)
            out[k] = resample(sp, img, (top, left, ch, cw), bool(flip is not None and flip[k]))
        if sp.planar:
            out = out.transpose(0, 3, 1, 2)
        values[sp.out_name] = np.ascontiguousarray(out).view(dt)
        if sp.shapes:
            shapes[sp.out_name] = shp
        stats[sp.out_name] = st
    return D.DenseBatch(values, {}, stats, shapes=shapes)


# ---------------------------------------------------------------------- device path
def launch(dec, items: Sequence[tuple], rows: tuple | None, m: int, row0: int, stats_ptr: int | None,
           skipped_ptr: int | None, consumer: int | None) -> None:
    """One ``tfrg_result_raw_rows`` call: items are (spec, slot, out pointer, lengths pointer or None);
    ``rows``: (device pointer, TFRG_ROWS_* id) or None."""
    arr = (N.TfrgRawSpec * len(items))()
    for a, (sp, slot, out, lens) in zip(arr, items):
        a.slot, a.src, a.out, a.count, a.channels = slot, SRC[sp.src][0], OUT[sp.out], sp.count, int(sp.channels)
        a.planar, a.fill, a.reserved, a.out_ptr, a.lengths = int(bool(sp.planar)), sp.fill_bits, 0, out, lens
        a.scale[: len(sp.scale)] = sp.scale
        a.bias[: len(sp.bias)] = sp.bias
    ptr, rdt = rows if rows is not None else (None, 0)
    N.check(dec._lib.tfrg_result_raw_rows(dec._ctx, arr, len(items), D.vp(ptr), rdt, m, row0, D.vp(stats_ptr),
                                          D.vp(skipped_ptr), D.vp(consumer)), "tfrg_result_raw_rows")


def launch_resize(dec, items: Sequence[tuple], rows: tuple | None, m: int, row0: int, stats_ptr: int | None,
                  skipped_ptr: int | None, consumer: int | None, boxes: int | None = None,
                  flip: int | None = None) -> None:
    """One ``tfrg_result_raw_resize`` call: items are (spec, (image slot, h_slot, w_slot), out pointer, shapes
    pointer or None); ``boxes``, ``flip``: device pointers, or None."""
    arr = (N.TfrgResizeSpec * len(items))()
    for a, (sp, (slot, hs, ws), out, shapes) in zip(arr, items):
        a.slot, a.src, a.out, a.channels, a.interp = slot, SRC[sp.src][0], OUT[sp.out], sp.channels, INTERP[sp.interp]
        a.interp |= N.RESIZE_ANTIALIAS if sp.antialias else 0
        a.h_slot, a.src_h = (N.RESIZE_CONST, sp.height) if hs is None else (hs, 0)
        a.w_slot, a.src_w = (N.RESIZE_CONST, sp.width) if ws is None else (ws, 0)
        (a.out_h, a.out_w), a.planar, a.fill, a.reserved = sp.size, int(bool(sp.planar)), sp.fill_bits, 0
        a.out_ptr, a.shapes = out, shapes
        a.scale[: len(sp.scale)] = sp.scale
        a.bias[: len(sp.bias)] = sp.bias
    ptr, rdt = rows if rows is not None else (None, 0)
    N.check(dec._lib.tfrg_result_raw_resize(dec._ctx, arr, len(items), D.vp(ptr), rdt, m, row0, D.vp(boxes), D.vp(flip),
                                            D.vp(stats_ptr), D.vp(skipped_ptr), D.vp(consumer)), "tfrg_result_raw_resize")


def _resize_slots(dec, sp: Resize):
    """(image slot, h_slot, w_slot) on ``dec``, a constant extent's slot being None; None: a key is missing."""
    slots = [D.resolve_slot(dec, sp)]
    for what in (sp.height, sp.width):
        slots.append(D.resolve_slot(dec, D.Dense(what, "int64")) if isinstance(what, str) else None)
        if isinstance(what, str) and slots[-1] is None:
            return None
    return None if slots[0] is None else tuple(slots)


@dataclass(frozen=True)
class _Kind:
    """What ``_run`` drives: its specs' check, whether a spec returns its per-row int32 side output (of
    shape ``[m, *aux_shape]``), a spec's columns on a decoder (None: the batch does not have them), the
    launch, and ``missing(dec, spec)``: the counters that the rows of a batch without the spec's keys add to."""

    check: object
    wants_aux: object
    aux_name: str
    aux_shape: tuple
    resolve: object
    launch: object
    missing: tuple


# (a batch without the key: its rows are padded and empty; without the image key: bad shapes and empty;
# with the image but without its height or width key: bad shapes)
RAW_KIND = _Kind(check_specs, lambda sp: sp.lengths, "lengths", (), D.resolve_slot, launch, lambda dec, sp: (1, 2))
RESIZE_KIND = _Kind(check_resize_specs, lambda sp: sp.shapes, "shapes", (2,), _resize_slots, launch_resize,
                    lambda dec, sp: (0, 2) if D.resolve_slot(dec, sp) is None else (0,))


def _torch_dtype(sp: Raw):
    import torch  # noqa: PLC0415

    return {"uint8": torch.uint8, "int8": torch.int8, "uint16": torch.uint16, "int16": torch.int16, "int32": torch.int32,
            "float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}[sp.out_type]


def _fill(t, bits: int, mine) -> None:
    """``bits`` into every element of the rows of ``t`` where ``mine`` is set, whatever its type."""
    import torch  # noqa: PLC0415

    esz = t.element_size()
    if esz > 1 and bits >= 1 << (8 * esz - 1):
        bits -= 1 << (8 * esz)
    t.view(t.shape[0], -1).view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[esz]).masked_fill_(mine[:, None], bits)


def _run(batches: Sequence[tuple], n: int, device: int, specs: Sequence[Raw], rows, out: Mapping | None,
         stream: int | None, strict: bool, kind: _Kind = RAW_KIND, extra: tuple = ()) -> D.DenseBatch:
    """``batches``: (decoder, r0, r1) per decoded batch, which holds rows [r0, r1) of the n. Every batch
    takes the whole row list with ``row0 = r0`` and writes the rows whose record it holds.

    The driver follows ``dense._Collator`` (whose specs are ``Dense``'s: a width and a dtype per slot kind)
    and shares ``device_rows``, ``rows_arg``, ``resolve_slot``, ``ConsumerStream`` and ``DenseBatch`` with
    it. As there, the rows of a batch that does not have a spec's key are ``fill``, with length 0, and
    count as padded and empty (``kind.missing``); and nothing is written on the current torch stream between the
    allocations and the end of the call: the fills run on the consumer stream, like the kernels' fences.
    Unlike dense, rows that no batch holds are ``fill`` too where the call allocated the output (with
    ``out=`` they keep what they held). ``kind``: Raw specs and their lengths, or Resize specs and their
    shapes (the batch's ``shapes``; (0, 0) for the rows of a batch whose decoder does not know a key); ``extra``: further
    arguments of its launch."""
    import torch  # noqa: PLC0415

    specs = kind.check(specs)
    dev = torch.device("cuda", device)
    rows_t, m = (None, n) if rows is None else D.device_rows(rows, n, device)
    values, lengths, own = {}, {}, set()
    with torch.cuda.device(dev):
        cur = torch.cuda.current_stream(dev)
        for sp in specs:
            given = (out or {}).get(sp.out_name)
            lens = None
            if isinstance(given, tuple):
                given, lens = given
            shape, tdt = (m, *sp.out_shape), _torch_dtype(sp)
            if given is None:
                given = torch.empty(shape, dtype=tdt, device=dev)
                own.add(sp.out_name)
            elif tuple(given.shape) != shape or given.dtype != tdt or given.device != dev or not given.is_contiguous():
                raise ValueError(f"out[{sp.out_name!r}] must be a contiguous {tdt} tensor of shape {shape} on {dev}")
            if kind.wants_aux(sp):
                ashape = (m, *kind.aux_shape)
                if lens is None:
                    lens = torch.empty(ashape, dtype=torch.int32, device=dev)
                    own.add(sp.out_name + " lengths")
                elif tuple(lens.shape) != ashape or lens.dtype != torch.int32 or lens.device != dev or not lens.is_contiguous():
                    raise ValueError(f"out[{sp.out_name!r}] {kind.aux_name} must be a contiguous int32 tensor of shape "
                                     f"{ashape} on {dev}")
                lengths[sp.out_name] = lens
            values[sp.out_name] = given
        k = len(specs)
        # (the library zeroes the counters of every call, and only those are read back)
        counters = torch.empty((max(len(batches), 1), k * 5), dtype=torch.int32, device=dev)
        consumer = D.ConsumerStream(cur, stream)
        consumer.begin()
        # the torch stream that is the consumer stream: what is filled here is ordered like the kernels
        fs = consumer.side if consumer.side is not None else (torch.cuda.ExternalStream(stream, device=dev) if stream else cur)
        calls, masks, ran = [], [], 0
        with torch.cuda.stream(fs):

            def fill_rows(sp: Raw, mine) -> None:
                _fill(values[sp.out_name], sp.fill_bits, mine)
                if sp.out_name in lengths:
                    lengths[sp.out_name].view(m, -1).masked_fill_(mine[:, None], 0)

            for b, (dec, r0, r1) in enumerate(batches):
                if not m:  # (no row: nothing to write, and an empty tensor has no address to give)
                    break
                ran += 1
                items, idx = [], []
                for i, sp in enumerate(specs):
                    slot = kind.resolve(dec, sp) if r1 > r0 else None
                    if slot is None:
                        if strict and r1 > r0:
                            raise KeyError(sp.key)
                        entries = rows_t if rows_t is not None else torch.arange(m, device=dev)
                        mine = (entries >= r0) & (entries < r1)  # (none of an empty batch)
                        fill_rows(sp, mine)
                        masks.append((i, mine.sum(), kind.missing(dec, sp) if r1 > r0 else ()))
                        continue
                    lens = lengths.get(sp.out_name)
                    items.append((sp, slot, values[sp.out_name].data_ptr(), lens.data_ptr() if lens is not None else None))
                    idx.append(i)
                if items:
                    kind.launch(dec, items, D.rows_arg(rows_t) if rows_t is not None else None, m, r0,
                                counters[b].data_ptr(), counters[b, 4 * k :].data_ptr(), consumer.handle, *extra)
                    calls.append((b, idx))
            if m and rows_t is not None and own:
                outside = (rows_t < 0) | (rows_t >= n)
                for sp in specs:
                    if sp.out_name in own:
                        _fill(values[sp.out_name], sp.fill_bits, outside)
                    if sp.out_name + " lengths" in own:
                        lengths[sp.out_name].view(m, -1).masked_fill_(outside[:, None], 0)
        consumer.end()

    def stats() -> dict:
        got = counters.cpu().numpy().view(np.uint32)
        tot = np.zeros((k, 4), np.int64)
        for b, idx in calls:
            tot[idx] += got[b, : 4 * len(idx)].reshape(-1, 4)
        for i, cnt, which in masks:  # (a batch without the spec's keys: ``kind.missing``)
            tot[i, list(which)] += int(cnt)
        return {sp.out_name: tot[i].astype(np.uint32) for i, sp in enumerate(specs)}

    def skipped() -> int:
        # Every batch skips what is not its own: for the first spec the sum over the batches is the
        # entries in no batch plus (batches - 1) * m. (A batch without its key counts through its mask.)
        if not m:
            return 0
        if not ran:
            return m
        got = counters.cpu().numpy().view(np.uint32).astype(np.int64)
        tot = sum(int(got[b, 4 * k]) for b, idx in calls if idx[0] == 0)
        tot += sum(m - int(cnt) for i, cnt, _ in masks if i == 0)
        return tot - (ran - 1) * m

    if kind.aux_name == "shapes":
        return D.DenseBatch(values, {}, stats, skipped, shapes=lengths)
    return D.DenseBatch(values, lengths, stats, skipped)


def decoder_raw(dec, specs: Sequence[Raw], *, rows=None, out: Mapping | None = None, stream: int | None = None,
                strict: bool = False) -> D.DenseBatch:
    """``HipDecoder.raw``: the raw-tensor outputs of the decoder's last decode, as torch tensors on its
    device: name -> ``[m, *shape]`` (planar: ``[m, channels, *shape[:-1]]``), with ``.lengths``,
    ``.stats`` and ``.skipped`` as ``HipDecoder.dense`` gives them.

    ``rows``: as ``decoder_dense``'s (what ``select`` and ``torch.randperm`` give, unchanged); None:
    every record in order. ``out``: name -> a preallocated tensor, or ``(tensor, lengths tensor)``;
    rows the call skips keep what they held. ``stream``: a HIP stream handle to order the call with,
    instead of the current torch stream. ``strict``: KeyError for a key the batch does not have,
    ValueError when a row is truncated, padded or holds several elements, IndexError for a skipped row."""
    b = _run([(dec, 0, D.last_n(dec))], D.last_n(dec), dec.device, specs, rows, out, stream, strict)
    return _strict(b, specs) if strict else b


def shard_raw(sd, plan: np.ndarray, specs: Sequence[Raw], *, rows=None, out: Mapping | None = None,
              stream: int | None = None, strict: bool = False) -> D.DenseBatch:
    """``ShardDecoder.raw``: one output per spec over the plan of the last ``decode_device`` /
    ``decode_device32``; every batch's context takes the row list (None: the plan's rows in order) with
    ``row0 = plan[k, 0]`` and writes the rows whose record it holds."""
    n = int(plan[-1, 1]) if len(plan) else 0
    b = _run([(sd.decs[k], r0, r1) for k, (r0, r1, _, _) in enumerate(plan.tolist())], n, sd.device, specs, rows, out,
             stream, strict)
    return _strict(b, specs) if strict else b


def _geometry(boxes, flip, m: int, device: int):
    """The device pointers of ``boxes`` (int32 ``[m, 4]``) and ``flip`` (uint8 / bool ``[m]``), each or both None."""
    import torch  # noqa: PLC0415

    dev = torch.device("cuda", device)
    for what, t, shape, dts in (("boxes", boxes, (m, 4), (torch.int32,)), ("flip", flip, (m,), (torch.uint8, torch.bool))):
        if t is not None and not (isinstance(t, torch.Tensor) and tuple(t.shape) == shape and t.dtype in dts
                                  and t.device == dev and t.is_contiguous()):
            raise ValueError(f"{what} must be a contiguous {dts[0]} tensor of shape {shape} on {dev}")
    return (boxes.data_ptr() if boxes is not None and m else None, flip.data_ptr() if flip is not None and m else None)


def _strict_resize(b: D.DenseBatch, specs: Sequence[Resize], strict: bool) -> D.DenseBatch:
    if strict:
        for s in specs:
            bs, bb, _, _ = (int(x) for x in b.stats[s.out_name])
            if bs or bb:
                raise ValueError(f"Resize({s.key!r}): {bs} rows with a bad shape, {bb} with a bad box")
        if b.skipped:
            raise IndexError(f"{b.skipped} rows of the list are outside the decoded records")
    return b


def _list_len(rows, n: int) -> int:
    return n if rows is None else len(rows)


def decoder_resize(dec, specs: Sequence[Resize], *, rows=None, boxes=None, flip=None, out: Mapping | None = None,
                   stream: int | None = None, strict: bool = False) -> D.DenseBatch:
    """``HipDecoder.resize``: the resized-image outputs of the decoder's last decode, as torch tensors on its
    device: name -> ``[m, OH, OW, C]`` (planar: ``[m, C, OH, OW]``), with ``.stats`` (``RESIZE_STAT_NAMES``),
    ``.skipped`` and ``.shapes`` (name -> ``[m, 2]`` int32, for the specs that ask). ``rows``, ``out`` (name
    -> a tensor, or ``(tensor, shapes tensor)``) and ``stream`` as ``decoder_raw``'s. ``boxes``: an int32
    ``[m, 4]`` device tensor (top, left, height, width) per entry of the row list, None: whole images;
    ``flip``: a uint8 / bool ``[m]`` device tensor, None: no mirror. Both are read on the call's stream.
    A key that the decoder's key table does not hold (no batch so far had it) has no column to read: the
    rows are ``fill`` and bad shapes (and empty, if it is the image key), and their shapes are (0, 0), where
    the kernel and the host path report each extent they can read and 0 for the other.
    ``strict``: KeyError for a missing key, ValueError for a row with a bad shape or box, IndexError for a
    skipped row."""
    n = D.last_n(dec)
    extra = _geometry(boxes, flip, _list_len(rows, n), dec.device)
    return _strict_resize(_run([(dec, 0, n)], n, dec.device, specs, rows, out, stream, strict, RESIZE_KIND, extra), specs, strict)


def shard_resize(sd, plan: np.ndarray, specs: Sequence[Resize], *, rows=None, boxes=None, flip=None,
                 out: Mapping | None = None, stream: int | None = None, strict: bool = False) -> D.DenseBatch:
    """``ShardDecoder.resize``: as ``shard_raw``, every batch's context taking the row list, the boxes and the
    flips of the whole call."""
    n = int(plan[-1, 1]) if len(plan) else 0
    extra = _geometry(boxes, flip, _list_len(rows, n), sd.device)
    b = _run([(sd.decs[k], r0, r1) for k, (r0, r1, _, _) in enumerate(plan.tolist())], n, sd.device, specs, rows, out,
             stream, strict, RESIZE_KIND, extra)
    return _strict_resize(b, specs, strict)


def _strict(b: D.DenseBatch, specs: Sequence[Raw]) -> D.DenseBatch:
    for s in specs:
        t, p, _, mu = (int(x) for x in b.stats[s.out_name])
        if t or p or mu:
            raise ValueError(f"Raw({s.key!r}, {s.src!r}, shape={s.shape}): {t} rows truncated, {p} padded, "
                             f"{mu} with more than one element")
    if b.skipped:
        raise IndexError(f"{b.skipped} rows of the list are outside the decoded records")
    return b
