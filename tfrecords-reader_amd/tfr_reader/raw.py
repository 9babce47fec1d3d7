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
            v = np.asarray(getattr(self, what), np.float64).reshape(-1)
            if v.size not in (1, int(c)) or not np.isfinite(v).all():
                raise ValueError(f"Raw({self.key!r}): {what} must be a number or {c} finite numbers")
            object.__setattr__(self, what, tuple(float(x) for x in np.broadcast_to(v, (int(c),)).astype(np.float32)))
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
        t = self.out_type
        if t == "bfloat16":
            return int(bf16_bits(np.array([self.fill], np.float32))[0])
        dt = SRC[t][1]
        if np.dtype(dt).kind == "f":
            return int(np.array(self.fill, dt).view({2: np.uint16, 4: np.uint32}[np.dtype(dt).itemsize]))
        v, bits = int(self.fill), 8 * np.dtype(dt).itemsize
        if not -(1 << (bits - 1)) <= v < (1 << bits):
            raise ValueError(f"Raw({self.key!r}): fill {v} does not fit {t}")
        return v & ((1 << bits) - 1)


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
                lo, c = base + int(rs[g]), int(rs[g + 1] - rs[g])
                ln = 0
                if c:
                    if res.bytes_data is not None:
                        elem = res.bytes_data[int(res.bytes_offsets[lo]) : int(res.bytes_offsets[lo + 1])]
                        ln = int(elem.size)
                    else:
                        o, ln = int(res.bytes_off[lo]), int(res.bytes_len[lo])
                        elem = np.zeros(ln, np.uint8)  # (a view past the input reads zeros)
                        got = res.buf[o : o + ln]
                        elem[: got.size] = got
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
         stream: int | None, strict: bool) -> D.DenseBatch:
    """``batches``: (decoder, r0, r1) per decoded batch, which holds rows [r0, r1) of the n. Every batch
    takes the whole row list with ``row0 = r0`` and writes the rows whose record it holds.

    The driver follows ``dense._Collator`` (whose specs are ``Dense``'s: a width and a dtype per slot kind)
    and shares ``device_rows``, ``rows_arg``, ``resolve_slot``, ``ConsumerStream`` and ``DenseBatch`` with
    it. As there, the rows of a batch that does not have a spec's key are ``fill``, with length 0, and
    count as padded and empty; and nothing is written on the current torch stream between the
    allocations and the end of the call: the fills run on the consumer stream, like the kernels' fences.
    Unlike dense, rows that no batch holds are ``fill`` too where the call allocated the output (with
    ``out=`` they keep what they held)."""
    import torch  # noqa: PLC0415

    specs = check_specs(specs)
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
            if sp.lengths:
                if lens is None:
                    lens = torch.empty((m,), dtype=torch.int32, device=dev)
                    own.add(sp.out_name + " lengths")
                elif tuple(lens.shape) != (m,) or lens.dtype != torch.int32 or lens.device != dev or not lens.is_contiguous():
                    raise ValueError(f"out[{sp.out_name!r}] lengths must be a contiguous int32 tensor of shape {(m,)} on {dev}")
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
                    lengths[sp.out_name].masked_fill_(mine, 0)

            for b, (dec, r0, r1) in enumerate(batches):
                if not m:  # (no row: nothing to write, and an empty tensor has no address to give)
                    break
                ran += 1
                items, idx = [], []
                for i, sp in enumerate(specs):
                    slot = D.resolve_slot(dec, sp) if r1 > r0 else None
                    if slot is None:
                        if strict and r1 > r0:
                            raise KeyError(sp.key)
                        entries = rows_t if rows_t is not None else torch.arange(m, device=dev)
                        mine = (entries >= r0) & (entries < r1)  # (none of an empty batch)
                        fill_rows(sp, mine)
                        masks.append((i, mine.sum()))
                        continue
                    lens = lengths.get(sp.out_name)
                    items.append((sp, slot, values[sp.out_name].data_ptr(), lens.data_ptr() if lens is not None else None))
                    idx.append(i)
                if items:
                    launch(dec, items, D.rows_arg(rows_t) if rows_t is not None else None, m, r0,
                           counters[b].data_ptr(), counters[b, 4 * k :].data_ptr(), consumer.handle)
                    calls.append((b, idx))
            if m and rows_t is not None and own:
                outside = (rows_t < 0) | (rows_t >= n)
                for sp in specs:
                    if sp.out_name in own:
                        _fill(values[sp.out_name], sp.fill_bits, outside)
                    if sp.out_name + " lengths" in own:
                        lengths[sp.out_name].masked_fill_(outside, 0)
        consumer.end()

    def stats() -> dict:
        got = counters.cpu().numpy().view(np.uint32)
        tot = np.zeros((k, 4), np.int64)
        for b, idx in calls:
            tot[idx] += got[b, : 4 * len(idx)].reshape(-1, 4)
        for i, cnt in masks:  # (a key without a slot: its rows are padded and empty)
            tot[i, 1:3] += int(cnt)
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
        tot += sum(m - int(cnt) for i, cnt in masks if i == 0)
        return tot - (ran - 1) * m

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


def _strict(b: D.DenseBatch, specs: Sequence[Raw]) -> D.DenseBatch:
    for s in specs:
        t, p, _, mu = (int(x) for x in b.stats[s.out_name])
        if t or p or mu:
            raise ValueError(f"Raw({s.key!r}, {s.src!r}, shape={s.shape}): {t} rows truncated, {p} padded, "
                             f"{mu} with more than one element")
    if b.skipped:
        raise IndexError(f"{b.skipped} rows of the list are outside the decoded records")
    return b
