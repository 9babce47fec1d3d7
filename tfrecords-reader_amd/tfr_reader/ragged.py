"""Ragged minibatches from decoded batches: the ``tf.io.parse_example`` ``VarLenFeature`` /
``RaggedTensor`` side, next to the ``FixedLenFeature`` side of ``tfr_reader.dense``.

``Ragged`` specs name variable-length outputs -- per key one packed ``values`` array with the rows
back to back, and ``m + 1`` ``offsets`` (``cu_seqlens``: row k is ``values[offsets[k]:offsets[k + 1]]``)
-- the form varlen attention, ``torch.nested`` / jagged tensors and ``EmbeddingBag`` take. No row is
padded, and a row may be longer than ``dense``'s widest output.

* ``HipDecoder.ragged`` gathers them on the device for every record in order or for a list of rows
  (``rows=``: shuffled, sampled, filtered), in three launches over the columns where the decode left
  them (``tfrg_result_ragged_rows``), and ``HipDecoder.ragged_minibatches`` draws an epoch from one
  decode; implicit columns are not written for it, and a bytes output whose ``bytes_off`` words are
  implicit (``info().implicit_off_slots``) is gathered from the decode's u32 record ends, which stay
  in place like the input bytes while the decode is read;
* ``BatchResult.ragged`` / ``raggedify`` compute the same function with numpy from fetched columns
  (the host path, and the reference the device path is tested against).

Per output: ``totals[name]`` is ``offsets[m]``, ``stats[name]`` the four counters ``(truncated,
empty, multi, skipped)``: rows longer than ``max_len``, rows without a value, (bytes) rows with more
than one element -- only element 0 is taken, as ``dense`` does -- and rows whose entry in a device row
list is out of range (they are empty rows here, and count in ``skipped`` alone).
"""

from __future__ import annotations

from collections.abc import Mapping, Sequence
from dataclasses import dataclass

import numpy as np

from tfr_reader import _native as N
from tfr_reader import dense as D

STAT_NAMES = ("truncated", "empty", "multi", "skipped")


@dataclass(frozen=True)
class Ragged:
    """One ragged output: ``key``'s values of ``dtype`` ("int64", "int32", "float32", "uint8"; the
    dtype selects the slot kind as for ``Dense``). ``max_len``: a row contributes at most that many
    elements (None: whole rows). ``name``: the output's name in the result (default: the key)."""

    key: str
    dtype: str
    max_len: int | None = None
    name: str | None = None

    def __post_init__(self) -> None:
        if self.dtype not in D.DTYPES:
            raise ValueError(f"Ragged({self.key!r}): dtype must be one of {sorted(D.DTYPES)}, not {self.dtype!r}")
        if self.max_len is not None and (not isinstance(self.max_len, (int, np.integer))
                                         or not 1 <= int(self.max_len) < 1 << 32):
            raise ValueError(f"Ragged({self.key!r}): max_len must be None or in 1..2^32 - 1, not {self.max_len!r}")
        if not isinstance(self.key, str):
            raise TypeError(f"Ragged key must be a str, not {type(self.key).__name__}")

    @property
    def out_name(self) -> str:
        return self.name if self.name is not None else self.key

    @property
    def limit(self) -> int:
        """``tfrg_ragged_spec.max_len`` (0: whole rows)."""
        return int(self.max_len) if self.max_len is not None else 0


def check_specs(specs: Sequence[Ragged]) -> list[Ragged]:
    specs = list(specs)
    if not 1 <= len(specs) <= N.RAGGED_MAX_SPECS:
        raise ValueError(f"between 1 and {N.RAGGED_MAX_SPECS} Ragged specs per call, not {len(specs)}")
    seen = set()
    for s in specs:
        if not isinstance(s, Ragged):
            raise TypeError(f"specs must be Ragged objects, not {type(s).__name__}")
        if s.out_name in seen:
            raise ValueError(f"two Ragged specs are named {s.out_name!r}: give one of them name=")
        seen.add(s.out_name)
    return specs


class RaggedBatch(dict):
    """name -> ``(values, offsets)`` (torch tensors on the decoder's device, numpy arrays on the host
    path). ``values`` holds ``capacity`` elements, of which the first ``offsets[-1]`` (at most) are
    rows. ``totals[name]``: ``offsets[m]``; ``stats[name]``: the four counters ``STAT_NAMES`` as a
    uint32 array; ``overflowed[name]``: the total is above the capacity (the stored prefix is still
    right, the offsets complete). All three are read back from the device on first access."""

    def __init__(self, outputs: Mapping, capacity: Mapping, totals, stats) -> None:
        super().__init__(outputs)
        self.capacity = dict(capacity)
        self._totals = totals  # a dict, or a function returning it
        self._stats = stats

    @property
    def totals(self) -> dict[str, int]:
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
def raggedify(specs: Sequence[Ragged], *, n: int, slot_key: Sequence[str | None], slot_kind: Sequence[int],
              row_splits: np.ndarray, slot_base: np.ndarray, i64: np.ndarray, f32: np.ndarray,
              bytes_off: np.ndarray | None = None, bytes_len: np.ndarray | None = None, buf: np.ndarray | None = None,
              bytes_data: np.ndarray | None = None, bytes_offsets: np.ndarray | None = None, rows=None) -> RaggedBatch:
    """The ragged outputs of ``specs`` from plain result columns (as ``dense.densify`` takes them),
    record by record. A key without a slot gives all-empty rows. ``rows``: output row k is record
    ``rows[k]`` (any order, repeats allowed; IndexError for one outside [0, n))."""
    specs = check_specs(specs)
    picked = list(range(n)) if rows is None else D.host_rows(rows, n).tolist()
    m = len(picked)
    outputs, totals, stats = {}, {}, {}
    for sp in specs:
        _, kind, dt, udt = D.DTYPES[sp.dtype]
        parts = []
        offsets = np.zeros(m + 1, np.int64)
        st = np.zeros(4, np.uint32)
        s = D.find_slot(slot_key, slot_kind, sp.key, kind)
        if s is None:
            st[1] = m
        else:
            base = int(slot_base[s])
            rs = np.asarray(row_splits[s]).astype(np.int64)
            for k, g in enumerate(picked):
                lo, c = base + int(rs[g]), int(rs[g + 1] - rs[g])
                if kind == 1:
                    row = np.zeros(0, np.uint8)
                    if c:
                        if bytes_data is not None:
                            row = np.asarray(bytes_data[int(bytes_offsets[lo]) : int(bytes_offsets[lo + 1])], np.uint8)
                        else:
                            o, ln = int(bytes_off[lo]), int(bytes_len[lo])
                            elem = np.asarray(buf[o : o + ln], np.uint8)
                            row = np.zeros(ln, np.uint8)  # (a view past the input reads zeros)
                            row[: elem.size] = elem
                    st[2] += c > 1
                else:
                    src = f32 if kind == 2 else i64
                    row = np.asarray(src[lo : lo + c]).view(np.uint32 if kind == 2 else np.uint64).astype(udt)
                full = int(row.size)
                if sp.max_len is not None and full > sp.max_len:
                    row = row[: int(sp.max_len)]
                    st[0] += 1
                st[1] += c == 0
                parts.append(row)
                offsets[k + 1] = offsets[k] + row.size
        values = np.concatenate(parts).astype(udt) if parts else np.zeros(0, udt)
        outputs[sp.out_name] = (values.view(dt), offsets)
        totals[sp.out_name] = int(offsets[m])
        stats[sp.out_name] = st
    return RaggedBatch(outputs, dict(totals), totals, stats)


def batch_ragged(res, specs: Sequence[Ragged], rows=None) -> RaggedBatch:
    """``BatchResult.ragged``: ``raggedify`` over a fetched result's columns."""
    return raggedify(specs, n=len(res), slot_key=res.slot_key, slot_kind=res.slot_kind, row_splits=res.row_splits,
                     slot_base=res.slot_base, i64=res.i64, f32=res.f32, bytes_off=res.bytes_off,
                     bytes_len=res.bytes_len, buf=res.buf, bytes_data=res.bytes_data, bytes_offsets=res.bytes_offsets,
                     rows=rows)


# ---------------------------------------------------------------------- device path
def launch(dec, items: Sequence[tuple], rows: tuple | None, m: int, row0: int, totals_ptr: int | None,
           stats_ptr: int | None, consumer: int | None) -> None:
    """One ``tfrg_result_ragged_rows`` call: items are (slot, TFRG_DENSE_* id, max_len, cap, values
    pointer or None, offsets pointer); ``rows``: (device pointer, TFRG_ROWS_* id) or None."""
    arr = (N.TfrgRaggedSpec * len(items))()
    for a, (slot, dt, max_len, cap, values, offsets) in zip(arr, items):
        a.slot, a.dtype, a.max_len, a.reserved, a.cap, a.values, a.offsets = slot, dt, max_len, 0, cap, values, offsets
    ptr, rdt = rows if rows is not None else (None, 0)
    N.check(dec._lib.tfrg_result_ragged_rows(dec._ctx, arr, len(items), D.vp(ptr), rdt, m, row0, D.vp(totals_ptr),
                                             D.vp(stats_ptr), D.vp(consumer)), "tfrg_result_ragged_rows")


def decoder_ragged(dec, specs: Sequence[Ragged], *, rows=None, capacity=None, out: Mapping | None = None,
                   stream: int | None = None) -> RaggedBatch:
    """``HipDecoder.ragged``: the ragged outputs of the decoder's last decode, as torch tensors on
    its device: name -> ``(values, offsets)``.

    ``rows``: as ``dense(rows=)`` -- a 1-D contiguous int32 / int64 tensor on the device, used where
    it is (an entry out of range is an empty row and counts in ``skipped``), or a host sequence,
    range-checked here (IndexError) and uploaded; None: every record in order.

    ``capacity``: elements per ``values`` tensor, an int or name -> int. With it the call enqueues
    its work and returns without a host synchronisation; ``.overflowed`` tells (on first access)
    whether a total was above it, in which case ``values`` holds the prefix that fits and the offsets
    are still complete. Without it the call runs twice: offsets only, one device-to-host copy of the
    totals (the step's single synchronisation), exact allocations, then the gather.

    ``out``: name -> ``(values tensor, offsets tensor)`` to write into (``values`` 1-D of the spec's
    dtype, its size the capacity; ``offsets`` int64 ``[m + 1]``). ``stream``: a HIP stream handle as
    the consumer stream (default: the current torch stream)."""
    import torch  # noqa: PLC0415

    specs = check_specs(specs)
    n = D.last_n(dec)
    dev = torch.device("cuda", dec.device)
    tdt = D.torch_dtypes()
    consumer = D.ConsumerStream.wrapping(stream, dev)
    with torch.cuda.device(dev), torch.cuda.stream(consumer.cur):
        d_rows, m = (None, n) if rows is None else D.device_rows(rows, n, dec.device)
        rw = D.rows_arg(d_rows) if d_rows is not None else None

        def call(items, totals_t, stats_t) -> None:  # (the consumer is ordered around each call)
            consumer.begin()
            launch(dec, items, rw, m, 0, totals_t.data_ptr(), stats_t.data_ptr() if stats_t is not None else None,
                   consumer.handle)
            consumer.end()

        caps: dict[str, int | None] = {}
        values: dict = {}
        offsets: dict = {}
        present: list[tuple[Ragged, int]] = []  # the specs the library is called for, with their slots
        absent: list[Ragged] = []  # key or kind not in the key table, or no record: all-empty rows, no launch
        for sp in specs:
            k = sp.out_name
            given = (out or {}).get(k)
            v = o = None
            if given is not None:
                v, o = given
                if v.dim() != 1 or v.dtype != tdt[sp.dtype] or v.device != dev or not v.is_contiguous():
                    raise ValueError(f"out[{k!r}] values must be a contiguous 1-D {tdt[sp.dtype]} tensor on {dev}")
                if tuple(o.shape) != (m + 1,) or o.dtype != torch.int64 or o.device != dev or not o.is_contiguous():
                    raise ValueError(f"out[{k!r}] offsets must be a contiguous int64 tensor of shape ({m + 1},) on {dev}")
                caps[k] = int(v.numel())
            else:
                cap = capacity.get(k) if isinstance(capacity, Mapping) else capacity
                if cap is not None and (not isinstance(cap, (int, np.integer)) or cap < 0):
                    raise ValueError(f"capacity must be a non-negative integer, not {cap!r}")
                caps[k] = None if cap is None else int(cap)
            slot = D.resolve_slot(dec, sp) if n else None
            if slot is None:
                absent.append(sp)
                caps[k] = caps[k] or 0
                if v is None:
                    v = torch.empty(caps[k], dtype=tdt[sp.dtype], device=dev)
                if o is None:
                    o = torch.zeros(m + 1, dtype=torch.int64, device=dev)
                else:
                    o.zero_()
            else:
                present.append((sp, slot))
                if o is None:
                    o = torch.empty(m + 1, dtype=torch.int64, device=dev)
            values[k], offsets[k] = v, o
        # the skipped rows of a spec without a launch: every row of an empty decode, else the entries
        # of a device row list outside [0, n) (a host list was checked)
        absent_skipped = m if not n else 0
        if absent and n and isinstance(rows, torch.Tensor):
            absent_skipped = ((d_rows < 0) | (d_rows >= n)).sum()

        kp = len(present)
        host_totals = None
        totals_t = stats_t = None
        if kp:
            totals_t = torch.empty(kp, dtype=torch.int64, device=dev)
            stats_t = torch.empty((kp, 4), dtype=torch.int32, device=dev)

            def items(with_values: bool) -> list:
                got = []
                for sp, slot in present:
                    v = values[sp.out_name] if with_values else None
                    got.append((slot, D.DTYPES[sp.dtype][0], sp.limit, int(v.numel()) if v is not None else 0,
                                v.data_ptr() if v is not None and v.numel() else None, offsets[sp.out_name].data_ptr()))
                return got

            if any(caps[sp.out_name] is None for sp, _ in present):
                call(items(False), totals_t, None)
                host_totals = [int(t) for t in totals_t.cpu().tolist()]  # the step's one synchronisation
                for (sp, _), t in zip(present, host_totals):
                    if caps[sp.out_name] is None:
                        caps[sp.out_name] = t
            for sp, _ in present:
                if values[sp.out_name] is None:
                    values[sp.out_name] = torch.empty(caps[sp.out_name], dtype=tdt[sp.dtype], device=dev)
            call(items(True), totals_t, stats_t)

    names = [sp.out_name for sp, _ in present]

    def totals() -> dict:
        got = {sp.out_name: 0 for sp in absent}
        if kp:
            host = host_totals if host_totals is not None else totals_t.cpu().tolist()
            got.update({k: int(t) for k, t in zip(names, host)})
        return {sp.out_name: got[sp.out_name] for sp in specs}

    def stats() -> dict:
        got = {}
        if absent:
            bad = int(absent_skipped)
            for sp in absent:
                got[sp.out_name] = np.array([0, m - bad, 0, bad], np.uint32)
        if kp:
            host = stats_t.cpu().numpy().view(np.uint32)
            got.update({k: host[i].copy() for i, k in enumerate(names)})
        return {sp.out_name: got[sp.out_name] for sp in specs}

    return RaggedBatch({sp.out_name: (values[sp.out_name], offsets[sp.out_name]) for sp in specs}, caps, totals, stats)


def ragged_minibatches(dec, specs: Sequence[Ragged], batch_size: int, *, seed: int = 0, drop_last: bool = False,
                       capacity=None, where=None):
    """One epoch of shuffled ragged minibatches over the last decode of ``dec``: yields one
    ``RaggedBatch`` of ``batch_size`` rows per step (the last one shorter, or left out with
    ``drop_last``), in the order of a ``torch.randperm`` on the device seeded with ``seed``, as
    ``dense.minibatches``. With ``capacity`` no step synchronises with the host. ``where``
    (``tfr_reader.select`` terms): the epoch covers the records that pass, each once (one select and
    one read-back of its count before the first step)."""
    import torch  # noqa: PLC0415

    if not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise ValueError(f"batch_size must be a positive integer, not {batch_size!r}")
    specs = check_specs(specs)
    n = D.last_n(dec)
    dev = torch.device("cuda", dec.device)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    if where is None:
        perm = torch.randperm(n, generator=gen, device=dev)
    else:
        from tfr_reader import select as SEL  # noqa: PLC0415

        perm = SEL.selected_permutation(dec, where, None, seed)
        n = int(perm.numel())
    for lo in range(0, n, int(batch_size)):
        hi = min(lo + int(batch_size), n)
        if drop_last and hi - lo < batch_size:
            return
        yield decoder_ragged(dec, specs, rows=perm[lo:hi], capacity=capacity)


# ====================================================================== two-level ragged outputs
# Every element of a ``bytes_list`` (``Ragged(key, "uint8")`` takes element 0 alone): per output a list
# (rows) of lists (elements) of byte strings as three flat arrays -- ``values`` (the elements' bytes
# back to back), ``elem_offsets`` (element e is ``values[elem_offsets[e]:elem_offsets[e + 1]]``) and
# ``row_offsets`` (row k holds elements ``row_offsets[k]`` up to ``row_offsets[k + 1]``).
ELEM_STAT_NAMES = ("rows_truncated", "elems_truncated", "empty", "skipped")


@dataclass(frozen=True)
class RaggedElements:
    """One two-level ragged output: every element of ``key``'s ``bytes_list``. ``max_elems``: a row
    contributes at most its first that many elements; ``max_len``: an element at most its first that
    many bytes (None: all of them). ``name``: the output's name in the result (default: the key)."""

    key: str
    max_len: int | None = None
    max_elems: int | None = None
    name: str | None = None

    dtype = "uint8"  # (the slot kind, as ``Ragged.dtype`` selects it)

    def __post_init__(self) -> None:
        for what, v in (("max_len", self.max_len), ("max_elems", self.max_elems)):
            if v is not None and (not isinstance(v, (int, np.integer)) or not 1 <= int(v) < 1 << 32):
                raise ValueError(f"RaggedElements({self.key!r}): {what} must be None or in 1..2^32 - 1, not {v!r}")
        if not isinstance(self.key, str):
            raise TypeError(f"RaggedElements key must be a str, not {type(self.key).__name__}")

    @property
    def out_name(self) -> str:
        return self.name if self.name is not None else self.key

    @property
    def limit(self) -> int:
        """``tfrg_elems_spec.max_len`` (0: whole elements)."""
        return int(self.max_len) if self.max_len is not None else 0

    @property
    def elems_limit(self) -> int:
        """``tfrg_elems_spec.max_elems`` (0: every element)."""
        return int(self.max_elems) if self.max_elems is not None else 0


def check_elem_specs(specs: Sequence[RaggedElements]) -> list[RaggedElements]:
    specs = list(specs)
    if not 1 <= len(specs) <= N.ELEMS_MAX_SPECS:
        raise ValueError(f"between 1 and {N.ELEMS_MAX_SPECS} RaggedElements specs per call, not {len(specs)}")
    seen = set()
    for s in specs:
        if not isinstance(s, RaggedElements):
            raise TypeError(f"specs must be RaggedElements objects, not {type(s).__name__}")
        if s.out_name in seen:
            raise ValueError(f"two RaggedElements specs are named {s.out_name!r}: give one of them name=")
        seen.add(s.out_name)
    return specs


class ElementsBatch(dict):
    """name -> ``(values, elem_offsets, row_offsets)`` (torch tensors on the decoder's device, numpy
    arrays on the host path). ``capacity[name]``: the ``(elements, bytes)`` the arrays can describe
    and hold; ``totals[name]``: ``(E, B)``, the elements and bytes of the rows; ``stats[name]``: the
    four counters ``ELEM_STAT_NAMES`` as a uint32 array; ``overflowed[name]``: a total is above its
    capacity (the stored prefixes are still right, the row offsets complete). The last three are read
    back from the device on first access."""

    def __init__(self, outputs: Mapping, capacity: Mapping, totals, stats) -> None:
        super().__init__(outputs)
        self.capacity = dict(capacity)
        self._totals = totals  # a dict, or a function returning it
        self._stats = stats

    @property
    def totals(self) -> dict[str, tuple[int, int]]:
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
        return {k: t[0] > self.capacity[k][0] or t[1] > self.capacity[k][1] for k, t in self.totals.items()}


def elementify(specs: Sequence[RaggedElements], *, n: int, slot_key: Sequence[str | None], slot_kind: Sequence[int],
               row_splits: np.ndarray, slot_base: np.ndarray, bytes_off: np.ndarray | None = None,
               bytes_len: np.ndarray | None = None, buf: np.ndarray | None = None, bytes_data: np.ndarray | None = None,
               bytes_offsets: np.ndarray | None = None, rows=None) -> ElementsBatch:
    """The two-level ragged outputs of ``specs`` from plain result columns (as ``raggedify`` takes
    them: bytes as ``(bytes_off, bytes_len)`` views into ``buf``, or ``bytes_data`` / ``bytes_offsets``),
    record by record. A key without a slot gives all-empty rows. ``rows``: output row k is record
    ``rows[k]`` (any order, repeats allowed; IndexError for one outside [0, n))."""
    specs = check_elem_specs(specs)
    picked = list(range(n)) if rows is None else D.host_rows(rows, n).tolist()
    m = len(picked)
    outputs, totals, stats, caps = {}, {}, {}, {}
    for sp in specs:
        parts: list[np.ndarray] = []
        lens: list[int] = []
        row_offsets = np.zeros(m + 1, np.int64)
        st = np.zeros(4, np.uint32)
        s = D.find_slot(slot_key, slot_kind, sp.key, 1)
        if s is None:
            st[2] = m
        else:
            base = int(slot_base[s])
            rs = np.asarray(row_splits[s]).astype(np.int64)
            for k, g in enumerate(picked):
                lo, c = base + int(rs[g]), int(rs[g + 1] - rs[g])
                st[2] += c == 0
                cnt = c
                if sp.max_elems is not None and c > sp.max_elems:
                    cnt = int(sp.max_elems)
                    st[0] += 1
                for e in range(lo, lo + cnt):
                    if bytes_data is not None:
                        elem = np.asarray(bytes_data[int(bytes_offsets[e]) : int(bytes_offsets[e + 1])], np.uint8)
                    else:
                        o, ln = int(bytes_off[e]), int(bytes_len[e])
                        view = np.asarray(buf[o : o + ln], np.uint8)
                        elem = np.zeros(ln, np.uint8)  # (a view past the input reads zeros)
                        elem[: view.size] = view
                    if sp.max_len is not None and elem.size > sp.max_len:
                        elem = elem[: int(sp.max_len)]
                        st[1] += 1
                    parts.append(elem)
                    lens.append(int(elem.size))
                row_offsets[k + 1] = row_offsets[k] + cnt
        values = np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, np.uint8)
        elem_offsets = np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int64)
        k = sp.out_name
        outputs[k] = (values, elem_offsets, row_offsets)
        totals[k] = caps[k] = (len(lens), int(values.size))
        stats[k] = st
    return ElementsBatch(outputs, caps, totals, stats)


def batch_ragged_elements(res, specs: Sequence[RaggedElements], rows=None) -> ElementsBatch:
    """``BatchResult.ragged_elements``: ``elementify`` over a fetched result's columns."""
    return elementify(specs, n=len(res), slot_key=res.slot_key, slot_kind=res.slot_kind, row_splits=res.row_splits,
                      slot_base=res.slot_base, bytes_off=res.bytes_off, bytes_len=res.bytes_len, buf=res.buf,
                      bytes_data=res.bytes_data, bytes_offsets=res.bytes_offsets, rows=rows)


def launch_elems(dec, items: Sequence[tuple], rows: tuple | None, m: int, row0: int, totals_ptr: int | None,
                 stats_ptr: int | None, consumer: int | None) -> None:
    """One ``tfrg_result_ragged_elems`` call: items are (slot, max_elems, max_len, elem_cap, cap, values
    pointer or None, elem_offsets pointer or None, row_offsets pointer); ``rows``: (device pointer,
    TFRG_ROWS_* id) or None."""
    arr = (N.TfrgElemsSpec * len(items))()
    for a, (slot, max_elems, max_len, elem_cap, cap, values, elem_offsets, row_offsets) in zip(arr, items):
        a.slot, a.max_elems, a.max_len, a.reserved, a.elem_cap, a.cap = slot, max_elems, max_len, 0, elem_cap, cap
        a.values, a.elem_offsets, a.row_offsets = values, elem_offsets, row_offsets
    ptr, rdt = rows if rows is not None else (None, 0)
    N.check(dec._lib.tfrg_result_ragged_elems(dec._ctx, arr, len(items), D.vp(ptr), rdt, m, row0, D.vp(totals_ptr),
                                              D.vp(stats_ptr), D.vp(consumer)), "tfrg_result_ragged_elems")


def _capacity_pair(cap, what: str) -> tuple[int, int] | None:
    if cap is None:
        return None
    ok = isinstance(cap, (tuple, list)) and len(cap) == 2 and all(
        isinstance(c, (int, np.integer)) and c >= 0 for c in cap)
    if not ok:
        raise ValueError(f"{what} must be an (elements, bytes) pair of non-negative integers, not {cap!r}")
    return int(cap[0]), int(cap[1])


def decoder_ragged_elements(dec, specs: Sequence[RaggedElements], *, rows=None, capacity=None,
                            out: Mapping | None = None, stream: int | None = None) -> ElementsBatch:
    """``HipDecoder.ragged_elements``: the two-level ragged outputs of the decoder's last decode, as
    torch tensors on its device: name -> ``(values, elem_offsets, row_offsets)``.

    ``rows``: as ``ragged(rows=)`` -- a device int32 / int64 tensor used where it is (an entry out of
    range, a ``Selection.rows`` tail of -1 included, is an empty row and counts in ``skipped``), a
    host sequence (range-checked, IndexError), or None: every record in order.

    ``capacity``: an ``(elements, bytes)`` pair, or name -> pair. With it the call enqueues its work
    and returns without a host synchronisation; ``.overflowed`` tells (on first access) whether a
    total was above it: the stored prefixes are right and the row offsets complete. Entries of
    ``elem_offsets`` past ``E + 1`` and of ``values`` past ``B`` are unspecified. Without it the call
    runs twice: totals only, one device-to-host copy (the step's single synchronisation), exact
    allocations, then the gather.

    ``out``: name -> ``(values, elem_offsets, row_offsets)`` to write into (uint8 ``[bytes]``, int64
    ``[elements + 1]``, int64 ``[m + 1]``). ``stream``: a HIP stream handle as the consumer stream
    (default: the current torch stream)."""
    import torch  # noqa: PLC0415

    specs = check_elem_specs(specs)
    n = D.last_n(dec)
    dev = torch.device("cuda", dec.device)
    consumer = D.ConsumerStream.wrapping(stream, dev)
    with torch.cuda.device(dev), torch.cuda.stream(consumer.cur):
        d_rows, m = (None, n) if rows is None else D.device_rows(rows, n, dec.device)
        rw = D.rows_arg(d_rows) if d_rows is not None else None

        def call(items, totals_t, stats_t) -> None:  # (the consumer is ordered around each call)
            consumer.begin()
            launch_elems(dec, items, rw, m, 0, totals_t.data_ptr(), stats_t.data_ptr() if stats_t is not None else None,
                         consumer.handle)
            consumer.end()

        def i64_ok(t, shape0: int | None) -> bool:
            return (t.dim() == 1 and t.dtype == torch.int64 and t.device == dev and t.is_contiguous()
                    and (shape0 is None or t.numel() == shape0))

        caps: dict[str, tuple[int, int] | None] = {}
        values: dict = {}
        eoffs: dict = {}
        roffs: dict = {}
        present: list[tuple[RaggedElements, int]] = []
        absent: list[RaggedElements] = []  # key not in the key table, or no record: all-empty rows, no launch
        for sp in specs:
            k = sp.out_name
            given = (out or {}).get(k)
            v = e = r = None
            if given is not None:
                v, e, r = given
                if v.dim() != 1 or v.dtype != torch.uint8 or v.device != dev or not v.is_contiguous():
                    raise ValueError(f"out[{k!r}] values must be a contiguous 1-D torch.uint8 tensor on {dev}")
                if not i64_ok(e, None) or e.numel() < 1:
                    raise ValueError(f"out[{k!r}] elem_offsets must be a contiguous 1-D int64 tensor of at least "
                                     f"one entry on {dev}")
                if not i64_ok(r, m + 1):
                    raise ValueError(f"out[{k!r}] row_offsets must be a contiguous int64 tensor of shape ({m + 1},) on {dev}")
                caps[k] = (int(e.numel()) - 1, int(v.numel()))
            else:
                cap = capacity.get(k) if isinstance(capacity, Mapping) else capacity
                caps[k] = _capacity_pair(cap, "capacity")
            slot = D.resolve_slot(dec, sp) if n else None
            if slot is None:
                absent.append(sp)
                caps[k] = caps[k] or (0, 0)
                if v is None:
                    v = torch.empty(caps[k][1], dtype=torch.uint8, device=dev)
                if e is None:
                    e = torch.zeros(caps[k][0] + 1, dtype=torch.int64, device=dev)
                else:
                    e[:1].zero_()
                if r is None:
                    r = torch.zeros(m + 1, dtype=torch.int64, device=dev)
                else:
                    r.zero_()
            else:
                present.append((sp, slot))
                if r is None:
                    r = torch.empty(m + 1, dtype=torch.int64, device=dev)
            values[k], eoffs[k], roffs[k] = v, e, r
        # the skipped rows of a spec without a launch (as decoder_ragged)
        absent_skipped = m if not n else 0
        if absent and n and isinstance(rows, torch.Tensor):
            absent_skipped = ((d_rows < 0) | (d_rows >= n)).sum()

        kp = len(present)
        host_totals = None
        totals_t = stats_t = None
        if kp:
            totals_t = torch.empty((kp, 2), dtype=torch.int64, device=dev)
            stats_t = torch.empty((kp, 4), dtype=torch.int32, device=dev)

            def items(with_values: bool) -> list:
                got = []
                for sp, slot in present:
                    k = sp.out_name
                    v, e = (values[k], eoffs[k]) if with_values else (None, None)
                    got.append((slot, sp.elems_limit, sp.limit, int(e.numel()) - 1 if e is not None else 0,
                                int(v.numel()) if v is not None else 0,
                                v.data_ptr() if v is not None and v.numel() else None,
                                e.data_ptr() if e is not None else None, roffs[k].data_ptr()))
                return got

            if any(caps[sp.out_name] is None for sp, _ in present):
                call(items(False), totals_t, None)
                host_totals = [(int(a), int(b)) for a, b in totals_t.cpu().tolist()]  # the step's one synchronisation
                for (sp, _), t in zip(present, host_totals):
                    if caps[sp.out_name] is None:
                        caps[sp.out_name] = t
            for sp, _ in present:
                k = sp.out_name
                if values[k] is None:
                    values[k] = torch.empty(caps[k][1], dtype=torch.uint8, device=dev)
                if eoffs[k] is None:
                    eoffs[k] = torch.empty(caps[k][0] + 1, dtype=torch.int64, device=dev)
            call(items(True), totals_t, stats_t)

    names = [sp.out_name for sp, _ in present]

    def totals() -> dict:
        got = {sp.out_name: (0, 0) for sp in absent}
        if kp:
            host = host_totals if host_totals is not None else totals_t.cpu().tolist()
            got.update({k: (int(t[0]), int(t[1])) for k, t in zip(names, host)})
        return {sp.out_name: got[sp.out_name] for sp in specs}

    def stats() -> dict:
        got = {}
        if absent:
            bad = int(absent_skipped)
            for sp in absent:
                got[sp.out_name] = np.array([0, 0, m - bad, bad], np.uint32)
        if kp:
            host = stats_t.cpu().numpy().view(np.uint32)
            got.update({k: host[i].copy() for i, k in enumerate(names)})
        return {sp.out_name: got[sp.out_name] for sp in specs}

    return ElementsBatch({sp.out_name: (values[sp.out_name], eoffs[sp.out_name], roffs[sp.out_name]) for sp in specs},
                         caps, totals, stats)
