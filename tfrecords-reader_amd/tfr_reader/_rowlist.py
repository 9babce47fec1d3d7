"""What the per-spec outputs over a list of rows share (``tfr_reader.ragged``: ``Ragged`` and
``RaggedElements``; ``tfr_reader.ids``: ``ElementIds``): the spec's derived properties and the check
of a list of specs, the result class, the numpy walk over the elements of a ``bytes_list``, and the
driver of the device path. An output is a tuple of tensors, the last one the ``m + 1`` offsets of the
rows; an ``OutputKind`` says what the others are and how the library is called for them."""

from __future__ import annotations

from collections.abc import Callable, Mapping, Sequence
from dataclasses import dataclass
from typing import Any, NamedTuple

import numpy as np

from tfr_reader import dense as D


# ---------------------------------------------------------------------- specs
class NamedSpec:
    """The derived properties of a spec dataclass with ``key`` / ``name`` and, where it has them,
    ``max_len`` / ``max_elems``."""

    @property
    def out_name(self) -> str:
        return self.name if self.name is not None else self.key

    @property
    def limit(self) -> int:
        """The C spec's ``max_len`` (0: all of it)."""
        return int(self.max_len) if self.max_len is not None else 0

    @property
    def elems_limit(self) -> int:
        """The C spec's ``max_elems`` (0: every element)."""
        return int(self.max_elems) if self.max_elems is not None else 0


def check_named_specs(specs: Sequence, cls: type, limit: int) -> list:
    specs = list(specs)
    what = cls.__name__
    if not 1 <= len(specs) <= limit:
        raise ValueError(f"between 1 and {limit} {what} specs per call, not {len(specs)}")
    seen = set()
    for s in specs:
        if not isinstance(s, cls):
            raise TypeError(f"specs must be {what} objects, not {type(s).__name__}")
        if s.out_name in seen:
            raise ValueError(f"two {what} specs are named {s.out_name!r}: give one of them name=")
        seen.add(s.out_name)
    return specs


# ---------------------------------------------------------------------- results
class RowListBatch(dict):
    """name -> the output's arrays, with ``capacity``, ``totals``, ``stats`` and ``overflowed`` per
    name. ``totals`` and ``stats`` may be given as functions: the device path reads them back on
    first access."""

    def __init__(self, outputs: Mapping, capacity: Mapping, totals, stats) -> None:
        super().__init__(outputs)
        self.capacity = dict(capacity)
        self._totals = totals  # a dict, or a function returning it
        self._stats = stats

    @property
    def totals(self) -> dict:
        if callable(self._totals):
            self._totals = self._totals()
        return self._totals

    @property
    def stats(self) -> dict[str, np.ndarray]:
        if callable(self._stats):
            self._stats = self._stats()
        return self._stats

    @property
    def overflowed(self) -> dict[str, bool]:
        return {k: t > self.capacity[k] for k, t in self.totals.items()}


# ---------------------------------------------------------------------- host path (numpy)
@dataclass
class BytesColumns:
    """The columns of a fetched result that hold its bytes features: bytes as ``(bytes_off,
    bytes_len)`` views into ``buf``, or ``bytes_data`` / ``bytes_offsets``."""

    slot_key: Sequence[str | None]
    slot_kind: Sequence[int]
    row_splits: np.ndarray
    slot_base: np.ndarray
    bytes_off: np.ndarray | None = None
    bytes_len: np.ndarray | None = None
    buf: np.ndarray | None = None
    bytes_data: np.ndarray | None = None
    bytes_offsets: np.ndarray | None = None

    def element(self, e: int) -> np.ndarray:
        """The bytes of element ``e`` of the bytes columns."""
        if self.bytes_data is not None:
            return np.asarray(self.bytes_data[int(self.bytes_offsets[e]) : int(self.bytes_offsets[e + 1])], np.uint8)
        o, ln = int(self.bytes_off[e]), int(self.bytes_len[e])
        view = np.asarray(self.buf[o : o + ln], np.uint8)
        elem = np.zeros(ln, np.uint8)  # (a view past the input reads zeros)
        elem[: view.size] = view
        return elem

    def rows(self, key: str, max_elems: int | None, picked: Sequence[int]):
        """Per output row k (record ``picked[k]``): ``(k, the record's element count under key, its
        first max_elems elements)``. A key without a slot gives all-empty rows."""
        s = D.find_slot(self.slot_key, self.slot_kind, key, 1)
        if s is None:
            yield from ((k, 0, []) for k in range(len(picked)))
            return
        base = int(self.slot_base[s])
        rs = np.asarray(self.row_splits[s]).astype(np.int64)
        for k, g in enumerate(picked):
            lo, c = base + int(rs[g]), int(rs[g + 1] - rs[g])
            cnt = c if max_elems is None else min(c, int(max_elems))
            yield k, c, [self.element(e) for e in range(lo, lo + cnt)]


# ---------------------------------------------------------------------- device path
class Part(NamedTuple):
    """One tensor of an output whose size follows from the capacity."""

    name: str
    dtype: Any  # torch dtype
    size: Callable  # capacity -> entries
    wants: str  # in the refusal of an out= tensor
    least: int = 0  # entries an out= tensor must have
    zero_head: bool = False  # entry 0 is 0 in an output without an element


class OutputKind(NamedTuple):
    parts: Callable  # spec -> its Parts (the tensors before the rows' offsets)
    offsets: str  # the name of the [m + 1] tensor
    capacity: Callable  # (capacity= value, "capacity") -> its checked form, or None
    cap_of: Callable  # the out= tensors of the parts -> the capacity they give
    no_cap: Any  # the capacity, and the totals, of nothing
    item: Callable  # (spec, slot, the parts' tensors or Nones, offsets tensor) -> launch's item
    launch: Callable
    width: int  # totals words per output
    empty_stat: int  # the counter of rows without an element
    batch: type


def numel(t) -> int:
    return int(t.numel()) if t is not None else 0


def ptr(t) -> int | None:
    return t.data_ptr() if t is not None and t.numel() else None


def run(dec, specs: Sequence, kind: OutputKind, *, rows, capacity, out: Mapping | None, stream: int | None) -> RowListBatch:
    """The device path of the checked ``specs`` over the decoder's last decode. With every capacity
    known (``capacity=`` or ``out=``) one call of the library and no host synchronisation; else a
    sizing call without the parts, one read-back of its totals, exact allocations, and the storing
    call. A spec whose key has no slot, and every spec of a decode without records, is not launched:
    its rows are empty, and offsets the caller provides are zeroed."""
    import torch  # noqa: PLC0415

    n = D.last_n(dec)
    dev = torch.device("cuda", dec.device)
    consumer = D.ConsumerStream.wrapping(stream, dev)
    with torch.cuda.device(dev), torch.cuda.stream(consumer.cur):
        d_rows, m = (None, n) if rows is None else D.device_rows(rows, n, dec.device)
        rw = D.rows_arg(d_rows) if d_rows is not None else None

        def call(items, totals_t, stats_t) -> None:  # (the consumer is ordered around each call)
            consumer.begin()
            kind.launch(dec, items, rw, m, 0, totals_t.data_ptr(), stats_t.data_ptr() if stats_t is not None else None,
                        consumer.handle)
            consumer.end()

        def fits(t, dtype, size: int | None = None, least: int = 0) -> bool:
            return (t.dim() == 1 and t.dtype == dtype and t.device == dev and t.is_contiguous()
                    and (size is None or t.numel() == size) and t.numel() >= least)

        caps: dict = {}
        sized: dict[str, list] = {}  # name -> the parts' tensors (None: allocated once the capacity is known)
        offs: dict = {}
        present: list[tuple] = []  # the specs the library is called for, with their slots
        absent: list = []  # key or kind not in the key table, or no record: all-empty rows, no launch
        for sp in specs:
            k, parts = sp.out_name, kind.parts(sp)
            given = (out or {}).get(k)
            ts, o = [None] * len(parts), None
            if given is not None:
                *ts, o = given
                for p, t in zip(parts, ts, strict=True):
                    if not fits(t, p.dtype, None, p.least):
                        raise ValueError(f"out[{k!r}] {p.name} must be a contiguous {p.wants} on {dev}")
                if not fits(o, torch.int64, m + 1):
                    raise ValueError(f"out[{k!r}] {kind.offsets} must be a contiguous int64 tensor of shape ({m + 1},) on {dev}")
                caps[k] = kind.cap_of(*ts)
            else:
                caps[k] = kind.capacity(capacity.get(k) if isinstance(capacity, Mapping) else capacity, "capacity")
            slot = D.resolve_slot(dec, sp) if n else None
            if slot is None:
                absent.append(sp)
                caps[k] = caps[k] or kind.no_cap
                for i, p in enumerate(parts):
                    if ts[i] is None:
                        ts[i] = (torch.zeros if p.zero_head else torch.empty)(p.size(caps[k]), dtype=p.dtype, device=dev)
                    elif p.zero_head:
                        ts[i][:1].zero_()
                if o is None:
                    o = torch.zeros(m + 1, dtype=torch.int64, device=dev)
                else:
                    o.zero_()
            else:
                present.append((sp, slot))
                if o is None:
                    o = torch.empty(m + 1, dtype=torch.int64, device=dev)
            sized[k], offs[k] = ts, o
        # the skipped rows of a spec without a launch: every row of an empty decode, else the entries
        # of a device row list outside [0, n) (a host list was checked)
        absent_skipped = m if not n else 0
        if absent and n and isinstance(rows, torch.Tensor):
            absent_skipped = ((d_rows < 0) | (d_rows >= n)).sum()

        def total(row: list):
            return int(row[0]) if kind.width == 1 else tuple(int(t) for t in row)

        kp = len(present)
        host_totals = None
        totals_t = stats_t = None
        if kp:
            totals_t = torch.empty((kp, kind.width), dtype=torch.int64, device=dev)
            stats_t = torch.empty((kp, 4), dtype=torch.int32, device=dev)

            def items(stored: bool) -> list:
                return [kind.item(sp, slot, sized[sp.out_name] if stored else [None] * len(sized[sp.out_name]),
                                  offs[sp.out_name]) for sp, slot in present]

            if any(caps[sp.out_name] is None for sp, _ in present):
                call(items(False), totals_t, None)
                host_totals = [total(row) for row in totals_t.cpu().tolist()]  # the step's one synchronisation
                for (sp, _), t in zip(present, host_totals):
                    if caps[sp.out_name] is None:
                        caps[sp.out_name] = t
            for sp, _ in present:
                k = sp.out_name
                for i, p in enumerate(kind.parts(sp)):
                    if sized[k][i] is None:
                        sized[k][i] = torch.empty(p.size(caps[k]), dtype=p.dtype, device=dev)
            call(items(True), totals_t, stats_t)

    names = [sp.out_name for sp, _ in present]

    def totals() -> dict:
        got = {sp.out_name: kind.no_cap for sp in absent}
        if kp:
            host = host_totals if host_totals is not None else [total(row) for row in totals_t.cpu().tolist()]
            got.update(zip(names, host))
        return {sp.out_name: got[sp.out_name] for sp in specs}

    def stats() -> dict:
        got = {}
        if absent:
            bad = int(absent_skipped)
            st = np.zeros(4, np.uint32)
            st[kind.empty_stat], st[3] = m - bad, bad
            got = {sp.out_name: st.copy() for sp in absent}
        if kp:
            host = stats_t.cpu().numpy().view(np.uint32)
            got.update({k: host[i].copy() for i, k in enumerate(names)})
        return {sp.out_name: got[sp.out_name] for sp in specs}

    return kind.batch({sp.out_name: (*sized[sp.out_name], offs[sp.out_name]) for sp in specs}, caps, totals, stats)
