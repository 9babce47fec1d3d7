"""Dense tensors from decoded batches: the ``tf.io.parse_example`` step (FixedLenFeature / padded
VarLenFeature) that the reference's users run after its decoder, here on the device.

A decode ends as ragged columns (``BatchResult`` on the host, ``tfrg_result_device`` on the device).
``Dense`` specs name the fixed-shape outputs a training loop takes -- ``[n, width]`` per key, padded
with ``fill`` or truncated, in the dtype the model wants -- and

* ``HipDecoder.dense`` / ``ShardDecoder.dense`` / ``TFRecordDatasetReader.load_tensors`` collate
  them on the device with one kernel per decoded batch (``tfrg_result_dense``), into torch tensors
  ordered with the caller's stream;
* ``BatchResult.dense`` / ``densify`` compute the same function with numpy from fetched columns (the
  host path, and the reference the device path is tested against).

Row lists: every entry point takes ``rows=``, and then output row k is record ``rows[k]`` of the
decode -- a shuffled, sampled or filtered minibatch. On the device that is one launch per decoded
batch over columns that stay where the decode left them (``tfrg_result_dense_rows``), so a shard is
decoded once and ``minibatches`` draws an epoch of batches from it. The columns an optimistic decode
left implicit are not written for it: a bytes output whose ``bytes_off`` words are implicit
(``info().implicit_off_slots``) is gathered from the decode's u32 record ends, which therefore stay in
place, like the input bytes, while the decode is read.

Per output: ``lengths[r]`` is the record's untruncated value count (bytes: the byte length of the
list's first element, 0 if the list is empty or absent) and ``stats`` the four counters
``(truncated, padded, empty, multi)``: records whose count (bytes: length) is above / below the
width, records without a value, and (bytes) records with more than one element.
"""

from __future__ import annotations

import contextlib
import ctypes as C
import functools
from collections.abc import Mapping, Sequence
from dataclasses import dataclass

import numpy as np

from tfr_reader import _native as N
from tfr_reader import _status as S

#: dtype name -> (TFRG_DENSE_* id, slot kind, numpy dtype, unsigned dtype of the same size)
DTYPES = {
    "int64": (N.DENSE_I64, 3, np.int64, np.uint64),
    "int32": (N.DENSE_I32, 3, np.int32, np.uint32),
    "float32": (N.DENSE_F32, 2, np.float32, np.uint32),
    "uint8": (N.DENSE_U8, 1, np.uint8, np.uint8),
}
STAT_NAMES = ("truncated", "padded", "empty", "multi")


@dataclass(frozen=True)
class Dense:
    """One dense output: ``key``'s values as ``[n, width]`` of ``dtype`` ("int64", "int32",
    "float32", "uint8"). The dtype selects the slot kind (int64_list, float_list, bytes_list), so a
    key that occurs with several kinds is unambiguous. ``fill`` pads short records (a float for
    float32). ``lengths``: also return the per-record lengths. ``name``: the output's name in the
    result (default: the key; needed when one key is asked for twice)."""

    key: str
    dtype: str
    width: int = 1
    fill: float | int = 0
    lengths: bool = False
    name: str | None = None

    def __post_init__(self) -> None:
        if self.dtype not in DTYPES:
            raise ValueError(f"Dense({self.key!r}): dtype must be one of {sorted(DTYPES)}, not {self.dtype!r}")
        if not isinstance(self.width, (int, np.integer)) or not 1 <= int(self.width) <= N.DENSE_MAX_WIDTH:
            raise ValueError(f"Dense({self.key!r}): width must be in 1..{N.DENSE_MAX_WIDTH}, not {self.width!r}")
        if not isinstance(self.key, str):
            raise TypeError(f"Dense key must be a str, not {type(self.key).__name__}")
        self.fill_bits  # noqa: B018 (validates the fill)

    @property
    def out_name(self) -> str:
        return self.name if self.name is not None else self.key

    @property
    def fill_bits(self) -> int:
        """The pad value's raw bits, as ``tfrg_dense_spec.fill`` takes them."""
        if self.dtype == "float32":
            return int(np.array(self.fill, np.float32).view(np.uint32))
        v = int(self.fill)
        if self.dtype == "uint8":
            if not 0 <= v <= 255:
                raise ValueError(f"Dense({self.key!r}): a uint8 fill must be in 0..255, not {v}")
            return v
        bits = 64 if self.dtype == "int64" else 32
        if not -(1 << (bits - 1)) <= v < (1 << bits):
            raise ValueError(f"Dense({self.key!r}): fill {v} does not fit {self.dtype}")
        return v & ((1 << bits) - 1)


def check_specs(specs: Sequence[Dense]) -> list[Dense]:
    specs = list(specs)
    if not 1 <= len(specs) <= N.DENSE_MAX_SPECS:
        raise ValueError(f"between 1 and {N.DENSE_MAX_SPECS} Dense specs per call, not {len(specs)}")
    seen = set()
    for s in specs:
        if not isinstance(s, Dense):
            raise TypeError(f"specs must be Dense objects, not {type(s).__name__}")
        if s.out_name in seen:
            raise ValueError(f"two Dense specs are named {s.out_name!r}: give one of them name=")
        seen.add(s.out_name)
    return specs


class DenseBatch(dict):
    """name -> ``[n, width]`` array (torch tensors on the decoder's device, numpy arrays on the host
    path); ``lengths[name]`` for the specs that asked for them; ``stats[name]`` the four counters
    ``STAT_NAMES`` as a uint32 array (read back from the device on first access); ``skipped``: how
    many entries of a device row list were out of range, their output rows left unwritten (read back
    on first access too)."""

    def __init__(self, values: Mapping, lengths: Mapping, stats, skipped=0) -> None:
        super().__init__(values)
        self.lengths = dict(lengths)
        self._stats = stats  # a dict, or a function returning it
        self._skipped = skipped  # an int, or a function returning it

    @property
    def skipped(self) -> int:
        if callable(self._skipped):
            self._skipped = int(self._skipped())
        return self._skipped

    @property
    def stats(self) -> dict[str, np.ndarray]:
        if callable(self._stats):
            self._stats = self._stats()
        return self._stats


def check_strict(specs: Sequence[Dense], stats: Mapping[str, np.ndarray]) -> None:
    """The FixedLenFeature contract: every record has exactly ``width`` values (bytes: one element of
    ``width`` bytes)."""
    for s in specs:
        t, p, _, m = (int(x) for x in stats[s.out_name])
        if t or p or m:
            raise ValueError(f"Dense({s.key!r}, {s.dtype!r}, width={s.width}): {t} records truncated, {p} padded, "
                             f"{m} with more than one element")


def host_rows(rows, n: int) -> np.ndarray:
    """A host row list as a 1-D int64 array, range-checked against ``n`` records (ValueError for
    anything but a 1-D integer sequence, IndexError naming the first index outside [0, n))."""
    a = np.asarray(rows)
    if a.ndim != 1:
        raise ValueError(f"rows must be one-dimensional, not of shape {a.shape}")
    if a.size == 0:
        return np.zeros(0, np.int64)
    if a.dtype.kind not in "iu":
        raise ValueError(f"rows must be integers, not {a.dtype}")
    bad = (a < 0) | (a >= n)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise IndexError(f"rows[{k}] = {int(a[k])} is out of range for {n} records")
    return np.ascontiguousarray(a, np.int64)


# ---------------------------------------------------------------------- host path (numpy)
def find_slot(slot_key: Sequence[str | None], slot_kind: Sequence[int], key: str, kind: int) -> int | None:
    for s, (k, kd) in enumerate(zip(slot_key, slot_kind)):
        if k == key and kd == kind:
            return s
    return None


def densify(specs: Sequence[Dense], *, n: int, slot_key: Sequence[str | None], slot_kind: Sequence[int],
            row_splits: np.ndarray, slot_base: np.ndarray, i64: np.ndarray, f32: np.ndarray,
            bytes_off: np.ndarray | None = None, bytes_len: np.ndarray | None = None, buf: np.ndarray | None = None,
            bytes_data: np.ndarray | None = None, bytes_offsets: np.ndarray | None = None,
            strict: bool = False, rows=None) -> DenseBatch:
    """The dense outputs of ``specs`` from plain result columns (``BatchResult``'s: ``row_splits``
    ``[n_slots][n + 1]``, ``slot_base``, the value arrays; bytes as ``(bytes_off, bytes_len)`` views
    into ``buf``, or ``bytes_data`` / ``bytes_offsets``), record by record. A key without a slot
    gives an all-``fill`` output (``strict``: KeyError). ``rows``: output row k is record
    ``rows[k]`` (any order, repeats allowed; IndexError for one outside [0, n)), and the lengths and
    counters are those of the output's rows."""
    specs = check_specs(specs)
    values, lengths, stats = {}, {}, {}
    picked = list(range(n)) if rows is None else host_rows(rows, n).tolist()
    n = len(picked)  # (from here on: the output's rows)
    for sp in specs:
        _, kind, dt, udt = DTYPES[sp.dtype]
        W = int(sp.width)
        out = np.full((n, W), sp.fill_bits, udt)
        lens = np.zeros(n, np.int32)
        st = np.zeros(4, np.uint32)
        s = find_slot(slot_key, slot_kind, sp.key, kind)
        if s is None:
            if strict:
                raise KeyError(sp.key)
            st[1] = st[2] = n
        else:
            base = int(slot_base[s])
            rs = np.asarray(row_splits[s]).astype(np.int64)
            for r, g in enumerate(picked):
                lo, c = base + int(rs[g]), int(rs[g + 1] - rs[g])
                if kind == 1:
                    ln = 0
                    if c:
                        if bytes_data is not None:
                            elem = bytes_data[int(bytes_offsets[lo]) : int(bytes_offsets[lo + 1])]
                            ln = int(elem.size)
                        else:
                            o, ln = int(bytes_off[lo]), int(bytes_len[lo])
                            elem = buf[o : o + ln]
                        m = min(ln, W, int(elem.size))  # (a view past the input reads zeros)
                        out[r, :m] = elem[:m]
                        out[r, m : min(ln, W)] = 0
                    st[3] += c > 1
                else:
                    ln = c
                    m = min(c, W)
                    src = f32 if kind == 2 else i64
                    out[r, :m] = np.asarray(src[lo : lo + m]).view(np.uint32 if kind == 2 else np.uint64).astype(udt)
                lens[r] = ln
                st[0] += ln > W
                st[1] += ln < W
                st[2] += c == 0
        values[sp.out_name] = out.view(dt)
        if sp.lengths:
            lengths[sp.out_name] = lens
        stats[sp.out_name] = st
    if strict:
        check_strict(specs, stats)
    return DenseBatch(values, lengths, stats)


def batch_dense(res, specs: Sequence[Dense], strict: bool = False, rows=None) -> DenseBatch:
    """``BatchResult.dense``: ``densify`` over a fetched result's columns."""
    if strict and res.status.any():
        res.raise_for(int(np.flatnonzero(res.status)[0]))
    return densify(specs, n=len(res), slot_key=res.slot_key, slot_kind=res.slot_kind, row_splits=res.row_splits,
                   slot_base=res.slot_base, i64=res.i64, f32=res.f32, bytes_off=res.bytes_off,
                   bytes_len=res.bytes_len, buf=res.buf, bytes_data=res.bytes_data, bytes_offsets=res.bytes_offsets,
                   strict=strict, rows=rows)


# ---------------------------------------------------------------------- device path
def resolve_slot(dec, sp: Dense) -> int | None:
    """The device column of a spec on ``dec`` (None: the key / kind is not in its key table)."""
    kt = dec.keys
    kid = kt.key_ids.get(sp.key.encode("utf-8"))
    if kid is None:
        return None
    s = kt.slots.get((kid, DTYPES[sp.dtype][1]))
    if s is None or s >= getattr(dec, "_pushed_slots", 0):
        return None
    return s


def vp(p: int | None):
    return C.c_void_p(p) if p else None


def launch(dec, items: Sequence[tuple], stats_ptr: int | None, consumer: int | None, rows: tuple | None = None,
           row0: int = 0, skipped_ptr: int | None = None) -> None:
    """One ``tfrg_result_dense`` call: items are (slot, TFRG_DENSE_* id, width, fill bits, out
    pointer, lengths pointer or None). ``rows``: (device pointer, m, TFRG_ROWS_* id), and the call is
    ``tfrg_result_dense_rows`` with ``row0`` and the ``[len(items)]`` skipped counters."""
    arr = (N.TfrgDenseSpec * len(items))()
    for a, (slot, dt, width, fill, out, lens) in zip(arr, items):
        a.slot, a.dtype, a.width, a.reserved, a.fill, a.out, a.lengths = slot, dt, width, 0, fill, out, lens
    if rows is None:
        N.check(dec._lib.tfrg_result_dense(dec._ctx, arr, len(items), vp(stats_ptr), vp(consumer)), "tfrg_result_dense")
        return
    ptr, m, rdt = rows
    N.check(dec._lib.tfrg_result_dense_rows(dec._ctx, arr, len(items), vp(ptr), rdt, m, row0, vp(stats_ptr),
                                            vp(skipped_ptr), vp(consumer)), "tfrg_result_dense_rows")


ROW_DTYPES = {"int32": N.ROWS_I32, "int64": N.ROWS_I64}


def device_rows(rows, n: int, device: int):
    """A row list for the device path, as (torch tensor, m). A 1-D contiguous int32 / int64 tensor on
    ``cuda:device`` is used where it is (no copy, no synchronisation: entries out of range are
    skipped and counted by the kernel). A host sequence is range-checked against ``n`` (IndexError)
    and uploaded as int64 on the current stream."""
    import torch  # noqa: PLC0415

    dev = torch.device("cuda", device)
    if isinstance(rows, torch.Tensor):
        if rows.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"rows must be an int32 or int64 tensor, not {rows.dtype}")
        if rows.device != dev:
            raise ValueError(f"rows is on {rows.device}, the decoder on {dev}")
        if rows.dim() != 1 or not rows.is_contiguous():
            raise ValueError(f"rows must be one-dimensional and contiguous, not of shape {tuple(rows.shape)} "
                             f"with strides {tuple(rows.stride())}")
        if rows.numel() >= 1 << 31:
            raise ValueError("rows must hold fewer than 2^31 entries")
        return rows, int(rows.numel())
    a = host_rows(rows, n)
    with torch.cuda.device(dev):
        return torch.from_numpy(a).to(dev, non_blocking=True), int(a.size)


def rows_arg(rows) -> tuple[int, int]:
    """(device pointer, TFRG_ROWS_* id) of a row tensor that ``device_rows`` returned."""
    return rows.data_ptr(), N.ROWS_I64 if rows.element_size() == 8 else N.ROWS_I32


@functools.cache
def torch_dtypes() -> dict:
    """dtype name (``DTYPES``) -> torch dtype (one table, made on first use)."""
    import torch  # noqa: PLC0415

    return {"int64": torch.int64, "int32": torch.int32, "float32": torch.float32, "uint8": torch.uint8}


def last_n(dec) -> int:
    """The records of ``dec``'s last decode (from ``dec.info()`` where the decoder did not note them)."""
    n = getattr(dec, "_last_n", None)
    return int(dec.info().n_records) if n is None else n


class ConsumerStream:
    """The consumer stream of library calls made for the torch stream ``cur``; the calls are given
    ``handle``. The legacy default stream (handle 0, which NULL would not name) is stood in for by one
    side stream per device: ``begin`` orders it after ``cur``, ``end`` orders ``cur`` after it, and
    the caller chooses how many calls lie between the two. ``handle=``: a raw HIP stream handle to
    use instead of ``cur``'s: dense's ``stream=``, whose tensors are allocated on the current torch
    stream. Ragged and select make their ``stream=`` the current torch stream (``wrapping``), so
    their allocations run on it too. The two differ observably and stay as they are."""

    __slots__ = ("cur", "side", "handle")
    _side: dict = {}

    def __init__(self, cur, handle: int | None = None) -> None:
        self.cur, self.side = cur, None
        self.handle = int(cur.cuda_stream) if handle is None else handle
        if not self.handle:
            import torch  # noqa: PLC0415

            self.side = self._side.get(cur.device.index)
            if self.side is None:
                self.side = self._side[cur.device.index] = torch.cuda.Stream(cur.device)
            self.handle = int(self.side.cuda_stream)

    @classmethod
    def wrapping(cls, stream: int | None, dev) -> ConsumerStream:
        """For ``stream`` (a HIP stream handle) as a torch stream, or the current one of ``dev``."""
        import torch  # noqa: PLC0415

        with torch.cuda.device(dev):
            return cls(torch.cuda.ExternalStream(stream, device=dev) if stream else torch.cuda.current_stream(dev))

    def begin(self) -> None:
        if self.side is not None:
            self.side.wait_stream(self.cur)

    def end(self) -> None:
        if self.side is not None:
            self.cur.wait_stream(self.side)


class _Collator:
    """Torch outputs of ``specs`` for ``n`` rows on ``device``, written batch by batch: batch k of
    ``n_batches`` fills rows [r0, r1) from its decoder's last result. Tensors come from
    ``torch.empty`` on the current torch stream, which is handed to the library as the consumer
    stream: the collate kernels start after the work queued on it so far and the stream waits for
    them, so the tensors are used like any other torch result."""

    def __init__(self, specs: Sequence[Dense], n: int, device: int, n_batches: int, out: Mapping | None = None,
                 stream: int | None = None, rows=None) -> None:
        import torch  # noqa: PLC0415

        self.torch = torch
        self.specs = check_specs(specs)
        self.dev = torch.device("cuda", device)
        # with a row list (``rows``: over the n rows of all batches) the outputs have its m rows, and
        # every batch gets the whole list: batch k writes the rows whose record is its own
        self.rows = None
        self.n_records = n
        if rows is not None:
            self.rows, n = device_rows(rows, n, device)
        self.n = n
        tdt = torch_dtypes()
        self.values, self.lengths = {}, {}
        with torch.cuda.device(self.dev):
            self.cur = torch.cuda.current_stream(self.dev)
            for sp in self.specs:
                given = (out or {}).get(sp.out_name)
                lens = None
                if isinstance(given, tuple):
                    given, lens = given
                shape = (n, int(sp.width))
                if given is None:
                    given = torch.empty(shape, dtype=tdt[sp.dtype], device=self.dev)
                self._check(given, shape, tdt[sp.dtype], sp.out_name)
                if sp.lengths:
                    if lens is None:
                        lens = torch.empty((n,), dtype=torch.int32, device=self.dev)
                    self._check(lens, (n,), torch.int32, sp.out_name + " lengths")
                    self.lengths[sp.out_name] = lens
                self.values[sp.out_name] = given
            self.k = len(self.specs)
            # (the library zeroes the counters of every call, and only those are read back. With a row
            # list, batch b's [k][4] counters are followed by its [k] skipped counters -- the entries
            # of the list that are not the batch's -- so that one memset clears both)
            per = 5 if self.rows is not None else 4
            counters = torch.empty((max(n_batches, 1), self.k * per), dtype=torch.int32, device=self.dev)
            self.stats = counters[:, : self.k * 4]
            self.skips = counters[:, self.k * 4 :] if self.rows is not None else None
            self.ran = 0  # batches that took the row list
            self.masks: list = []  # (spec index, how many rows of the list an absent slot's batch holds)
            self.absent = np.zeros((self.k, 4), np.int64)  # counters of the (batch, spec) pairs without a slot
            self.calls: list = []  # (batch, spec indices of the call's counters)
            self.consumer = ConsumerStream(self.cur, stream)  # (once per collator: finish() ends it)
            self.consumer.begin()

    def _check(self, t, shape, dtype, what: str) -> None:
        if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != self.dev or not t.is_contiguous():
            raise ValueError(f"out[{what!r}] must be a contiguous {dtype} tensor of shape {tuple(shape)} on {self.dev}")

    def _fill(self, t, sp: Dense, mine=None) -> None:
        """The spec's fill into ``t``, or into its rows where ``mine`` is set."""
        torch = self.torch
        bits = sp.fill_bits
        if sp.dtype == "int64":
            bits = bits - (1 << 64) if bits >= 1 << 63 else bits
        elif sp.dtype != "uint8":
            t = t.view(torch.int32)
            bits = bits - (1 << 32) if bits >= 1 << 31 else bits
        if mine is None:
            t.fill_(bits)
        else:
            t.masked_fill_(mine[:, None], bits)

    def run(self, dec, r0: int, r1: int, k: int, strict: bool = False) -> None:
        """Rows [r0, r1) from ``dec``'s last decode (r1 - r0 records), as batch k."""
        by_rows = self.rows is not None
        if (not self.n) if by_rows else (r1 <= r0):  # (an empty batch still skips every row of a list)
            return
        self.ran += by_rows
        items, rows = [], []
        for i, sp in enumerate(self.specs):
            t = self.values[sp.out_name]
            lens = self.lengths.get(sp.out_name)
            slot = resolve_slot(dec, sp) if r1 > r0 else None
            if slot is None:
                if strict and r1 > r0:
                    raise KeyError(sp.key)
                side = self.consumer.side
                with self.torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
                    if by_rows:
                        # the rows of the list that are this batch's (none of an empty batch)
                        mine = (self.rows >= r0) & (self.rows < r1)
                        self._fill(t, sp, mine)
                        if lens is not None:
                            lens.masked_fill_(mine, 0)
                        self.masks.append((i, mine.sum()))
                    else:
                        self._fill(t[r0:r1], sp)
                        if lens is not None:
                            lens[r0:r1].zero_()
                if not by_rows:
                    self.absent[i, 1] += r1 - r0
                    self.absent[i, 2] += r1 - r0
                continue
            rows.append(i)
            at = 0 if by_rows else r0
            items.append((slot, DTYPES[sp.dtype][0], int(sp.width), sp.fill_bits,
                          t.data_ptr() + at * t.stride(0) * t.element_size(),
                          lens.data_ptr() + 4 * at if lens is not None else None))
        if items:
            # (the library's counters are per spec of the call: its rows map back on the host)
            if by_rows:
                ptr, rdt = rows_arg(self.rows)
                launch(dec, items, self.stats[k].data_ptr(), self.consumer.handle, (ptr, self.n, rdt), r0,
                       self.skips[k].data_ptr())
            else:
                launch(dec, items, self.stats[k].data_ptr(), self.consumer.handle)
            self.calls.append((k, rows))

    def finish(self, strict: bool = False) -> DenseBatch:
        self.consumer.end()
        specs, stats_t, absent, calls = self.specs, self.stats, self.absent, self.calls
        skips_t, masks, m, ran = self.skips, self.masks, self.n, self.ran

        def stats() -> dict:
            got = stats_t.cpu().numpy().view(np.uint32).reshape(len(stats_t), -1)
            tot = absent.copy()
            for k, rows in calls:
                tot[rows] += got[k, : 4 * len(rows)].reshape(-1, 4)
            for i, cnt in masks:  # (a key without a slot: its rows are padded and empty)
                tot[i, 1:3] += int(cnt)
            return {sp.out_name: tot[i].astype(np.uint32) for i, sp in enumerate(specs)}

        def skipped() -> int:
            # Every batch skips what is not its own: per spec the sum over the batches is the entries
            # in no batch plus (batches - 1) * m. (A batch without the key, or without a launch,
            # counts through its mask; the specs agree, the first one answers.)
            if skips_t is None or not m:
                return 0
            if not ran:  # (a plan without a batch holds no row)
                return m
            got = skips_t.cpu().numpy().view(np.uint32).astype(np.int64)
            tot = np.zeros(len(specs), np.int64)
            for k, rows in calls:
                tot[rows] += got[k, : len(rows)]
            for i, cnt in masks:
                tot[i] += m - int(cnt)
            return int(tot[0]) - (ran - 1) * m

        b = DenseBatch(self.values, self.lengths, stats, skipped)
        if strict:
            check_strict(specs, b.stats)
            if b.skipped:
                raise IndexError(f"{b.skipped} of the {m} rows are outside the {self.n_records} records")
        return b


def _raise_first_error(dec, info) -> None:
    """Raises the exception of the last decode's first failing record (``strict``)."""
    n = int(info.n_records)
    status, aux = np.empty(n, np.int32), np.empty(n, np.int64)
    cols = N.TfrgColumns()
    cols.status, cols.aux = N.ptr(status, N.i32p), N.ptr(aux, N.i64p)
    N.check(dec._lib.tfrg_result_fetch(dec._ctx, C.byref(cols)), "tfrg_result_fetch")
    r = int(info.first_error)
    st, ax = int(status[r]), int(aux[r])
    key = None
    host = getattr(dec, "_last_host", None)
    if st == S.ERR_KEY_UTF8 and host is not None:
        buf, starts, payload_only = host
        a = ax & 0xFFFFFFFFFFFFFFFF
        p = int(starts[r]) + (0 if payload_only else 12) + (a >> 32)
        key = bytes(buf[p : p + (a & 0xFFFFFFFF)])
    raise S.exception_for(st, ax, key)


def decoder_dense(dec, specs: Sequence[Dense], *, strict: bool = False, out: Mapping | None = None,
                  stream: int | None = None, rows=None) -> DenseBatch:
    """``HipDecoder.dense``: the dense outputs of the decoder's last decode (``decode``,
    ``decode_device`` or ``decode_device32``), as torch tensors on its device.

    ``out``: name -> a preallocated tensor, or ``(tensor, lengths tensor)``; for callers without
    torch, name -> a raw device pointer or ``(pointer, lengths pointer)`` for every spec (then the
    result holds the pointers, no counters are kept and ``stream`` -- a HIP stream handle, default
    the decode's own stream -- is the consumer stream). ``strict``: ValueError naming the key when a
    record is truncated, padded or holds several bytes elements (FixedLenFeature), KeyError for a key
    the batch does not have, and the first failing record's exception when a record failed.

    ``rows``: the outputs have one row per entry, output row k holding record ``rows[k]`` -- a 1-D
    contiguous int32 / int64 tensor on the device, used where it is and ordered with the current
    stream (an entry out of range leaves its row unwritten and counts in ``.skipped``; ``strict``:
    IndexError), or a host sequence, range-checked here (IndexError) and uploaded. With raw pointers
    as ``out=`` it is ``(device pointer, m, "int32" | "int64")``."""
    specs = check_specs(specs)
    info = dec.info() if strict else None
    n = int(info.n_records) if strict else last_n(dec)
    if strict and info.n_errors:
        _raise_first_error(dec, info)
    raw = bool(out) and all(isinstance(v, (int, np.integer)) or (isinstance(v, tuple) and isinstance(v[0], (int, np.integer)))
                            for v in out.values())
    if raw:
        if strict:
            raise ValueError("strict needs the counters: pass torch tensors (or none) as out=")
        items, values, lengths = [], {}, {}
        for sp in specs:
            v = out[sp.out_name]
            ptr, lens = (v if isinstance(v, tuple) else (v, None))
            slot = resolve_slot(dec, sp)
            if slot is None:
                raise KeyError(sp.key)
            items.append((slot, DTYPES[sp.dtype][0], int(sp.width), sp.fill_bits, int(ptr), int(lens) if lens else None))
            values[sp.out_name] = int(ptr)
            if lens:
                lengths[sp.out_name] = int(lens)
        if rows is not None:
            if not (isinstance(rows, tuple) and len(rows) == 3 and isinstance(rows[0], (int, np.integer))):
                raise TypeError('with raw pointers as out=, rows is (device pointer, m, "int32" | "int64")')
            if rows[2] not in ROW_DTYPES:
                raise ValueError(f"rows dtype must be one of {sorted(ROW_DTYPES)}, not {rows[2]!r}")
            launch(dec, items, None, stream, (int(rows[0]), int(rows[1]), ROW_DTYPES[rows[2]]))
        elif n:
            launch(dec, items, None, stream)
        return DenseBatch(values, lengths, {})
    col = _Collator(specs, n, dec.device, 1, out, stream, rows)
    col.run(dec, 0, n, 0, strict)
    return col.finish(strict)


def shard_dense(sd, plan: np.ndarray, specs: Sequence[Dense], *, strict: bool = False, out: Mapping | None = None,
                stream: int | None = None, rows=None) -> DenseBatch:
    """``ShardDecoder.dense``: one output per spec over the whole plan of the last
    ``decode_device`` / ``decode_device32``; batch k's context writes rows [plan[k, 0], plan[k, 1])
    on its own stream. ``rows`` (as ``decoder_dense``'s, numbering the plan's rows): every context
    takes the whole list with ``row0 = plan[k, 0]`` and writes the rows whose record it holds."""
    n = int(plan[-1, 1]) if len(plan) else 0
    col = _Collator(specs, n, sd.device, len(plan), out, stream, rows)
    for k, (r0, r1, _, _) in enumerate(plan.tolist()):
        d = sd.decs[k]
        if strict:
            info = d.info()
            if info.n_errors:
                _raise_first_error(d, info)
        col.run(d, r0, r1, k, strict)
    return col.finish(strict)


def minibatches(dec, specs: Sequence[Dense], batch_size: int, *, plan: np.ndarray | None = None, seed: int = 0,
                drop_last: bool = False, where=None):
    """One epoch of shuffled minibatches over the last decode of ``dec`` (a ``HipDecoder``, or a
    ``ShardDecoder`` with its ``plan``): yields one ``DenseBatch`` of ``batch_size`` rows per step
    (the last one shorter, or left out with ``drop_last``). The order is a ``torch.randperm`` on the
    device from a generator seeded with ``seed``; every step is one launch per decoded batch over the
    columns where the decode left them, with no host synchronisation after the first. ``where``
    (``tfr_reader.select`` terms): the epoch covers the records that pass, each once -- one select and
    one read-back of its count, then the selected rows permuted with the seeded generator."""
    import torch  # noqa: PLC0415

    if not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise ValueError(f"batch_size must be a positive integer, not {batch_size!r}")
    specs = check_specs(specs)
    if plan is not None:
        n = int(plan[-1, 1]) if len(plan) else 0
    else:
        n = last_n(dec)
    dev = torch.device("cuda", dec.device)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    if where is None:
        perm = torch.randperm(n, generator=gen, device=dev)
    else:
        from tfr_reader import select as SEL  # noqa: PLC0415

        perm = SEL.selected_permutation(dec, where, plan, seed)
        n = int(perm.numel())
    for lo in range(0, n, int(batch_size)):
        hi = min(lo + int(batch_size), n)
        if drop_last and hi - lo < batch_size:
            return
        rows = perm[lo:hi]
        yield shard_dense(dec, plan, specs, rows=rows) if plan is not None else decoder_dense(dec, specs, rows=rows)


def load_tensors(reader, selection, specs: Sequence[Dense], device: int | None = None) -> DenseBatch:
    """``TFRecordDatasetReader.load_tensors``: the records of an index selection as dense tensors
    with rows in selection order. The records are staged back to back in that order
    (tfrg_gather_ranges), decoded in batches below the per-call cap with their CRC verdicts and
    collated on the device. Raises the first failing record's exception, as ``load_records``."""
    from tfr_reader import _frame as F  # noqa: PLC0415
    from tfr_reader import _io, hip  # noqa: PLC0415
    from tfr_reader import reader as R  # noqa: PLC0415

    specs = check_specs(specs)
    cols = F.columns(selection, ["tfrecord_filename", "tfrecord_start", "tfrecord_end"])
    names = list(cols["tfrecord_filename"])
    starts = np.asarray(cols["tfrecord_start"], np.uint64).reshape(-1)
    ends = np.asarray(cols["tfrecord_end"], np.uint64).reshape(-1)
    n = len(names)
    dev = 0 if device is None else int(device)
    dec = hip.default_decoder(dev)
    images: dict = {}
    for i, name in enumerate(names):
        img = images.get(name)
        if img is None:
            path = R.join_path(reader.dataset_dir, name)
            R._check_path(path)
            img = images[name] = _io.file_image(path)
        if int(starts[i]) >= img.size or ends[i] <= starts[i] or int(ends[i]) > img.size:
            raise OSError(f"Failed to read data from {(int(starts[i]), int(ends[i]))}!")
    lens = ends - starts
    # batches of whole records below the per-call cap
    cuts = [0]
    acc = 0
    for i in range(n):
        if acc and acc + int(lens[i]) > R.MAX_BATCH_BYTES:
            cuts.append(i)
            acc = 0
        acc += int(lens[i])
    cuts.append(n)
    col = _Collator(specs, n, dev, len(cuts) - 1)
    lib = N.lib()
    for k in range(len(cuts) - 1):
        r0, r1 = cuts[k], cuts[k + 1]
        if r1 <= r0:
            continue
        b_en = np.cumsum(lens[r0:r1], dtype=np.uint64)
        b_st = b_en - lens[r0:r1]
        buf = np.empty(int(b_en[-1]), np.uint8)
        i = r0
        while i < r1:  # one gather per run of records of one file
            j = i + 1
            while j < r1 and names[j] == names[i]:
                j += 1
            st, en = np.ascontiguousarray(starts[i:j]), np.ascontiguousarray(ends[i:j])
            lib.tfrg_gather_ranges(N.ptr(images[names[i]]), N.ptr(st, N.u64p), N.ptr(en, N.u64p), j - i,
                                   N.ptr(buf[int(b_st[i - r0]):]))
            i = j
        res = dec.decode(buf, b_st, b_en)
        if res.status.any():
            res.raise_for(int(np.flatnonzero(res.status)[0]))
        col.run(dec, r0, r1, k)
    return col.finish()
