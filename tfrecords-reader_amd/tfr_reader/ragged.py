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
from tfr_reader import _rowlist as RL
from tfr_reader import dense as D

STAT_NAMES = ("truncated", "empty", "multi", "skipped")


@dataclass(frozen=True)
class Ragged(RL.NamedSpec):
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


def check_specs(specs: Sequence[Ragged]) -> list[Ragged]:
    return RL.check_named_specs(specs, Ragged, N.RAGGED_MAX_SPECS)


class RaggedBatch(RL.RowListBatch):
    """name -> ``(values, offsets)`` (torch tensors on the decoder's device, numpy arrays on the host
    path). ``values`` holds ``capacity`` elements, of which the first ``offsets[-1]`` (at most) are
    rows. ``totals[name]``: ``offsets[m]``; ``stats[name]``: the four counters ``STAT_NAMES`` as a
    uint32 array; ``overflowed[name]``: the total is above the capacity (the stored prefix is still
    right, the offsets complete). All three are read back from the device on first access."""


# ---------------------------------------------------------------------- host path (numpy)
def raggedify(specs: Sequence[Ragged], *, n: int, slot_key: Sequence[str | None], slot_kind: Sequence[int],
              row_splits: np.ndarray, slot_base: np.ndarray, i64: np.ndarray, f32: np.ndarray,
              bytes_off: np.ndarray | None = None, bytes_len: np.ndarray | None = None, buf: np.ndarray | None = None,
              bytes_data: np.ndarray | None = None, bytes_offsets: np.ndarray | None = None, rows=None) -> RaggedBatch:
    """The ragged outputs of ``specs`` from plain result columns (as ``dense.densify`` takes them),
    record by record. A key without a slot gives all-empty rows. ``rows``: output row k is record
    ``rows[k]`` (any order, repeats allowed; IndexError for one outside [0, n))."""
    specs = check_specs(specs)
    cols = RL.BytesColumns(slot_key, slot_kind, row_splits, slot_base, bytes_off, bytes_len, buf, bytes_data, bytes_offsets)
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
                    row = cols.element(lo) if c else np.zeros(0, np.uint8)
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


def _capacity(cap, what: str) -> int | None:
    if cap is not None and (not isinstance(cap, (int, np.integer)) or cap < 0):
        raise ValueError(f"{what} must be a non-negative integer, not {cap!r}")
    return None if cap is None else int(cap)


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
    tdt = D.torch_dtypes()
    kind = RL.OutputKind(
        parts=lambda sp: (RL.Part("values", tdt[sp.dtype], lambda cap: cap, f"1-D {tdt[sp.dtype]} tensor"),),
        offsets="offsets", capacity=_capacity, cap_of=lambda v: int(v.numel()), no_cap=0,
        item=lambda sp, slot, ts, o: (slot, D.DTYPES[sp.dtype][0], sp.limit, RL.numel(ts[0]), RL.ptr(ts[0]), o.data_ptr()),
        launch=launch, width=1, empty_stat=1, batch=RaggedBatch)
    return RL.run(dec, check_specs(specs), kind, rows=rows, capacity=capacity, out=out, stream=stream)


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
class RaggedElements(RL.NamedSpec):
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


def check_elem_specs(specs: Sequence[RaggedElements]) -> list[RaggedElements]:
    return RL.check_named_specs(specs, RaggedElements, N.ELEMS_MAX_SPECS)


class ElementsBatch(RL.RowListBatch):
    """name -> ``(values, elem_offsets, row_offsets)`` (torch tensors on the decoder's device, numpy
    arrays on the host path). ``capacity[name]``: the ``(elements, bytes)`` the arrays can describe
    and hold; ``totals[name]``: ``(E, B)``, the elements and bytes of the rows; ``stats[name]``: the
    four counters ``ELEM_STAT_NAMES`` as a uint32 array; ``overflowed[name]``: a total is above its
    capacity (the stored prefixes are still right, the row offsets complete). The last three are read
    back from the device on first access."""

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
    cols = RL.BytesColumns(slot_key, slot_kind, row_splits, slot_base, bytes_off, bytes_len, buf, bytes_data, bytes_offsets)
    picked = list(range(n)) if rows is None else D.host_rows(rows, n).tolist()
    m = len(picked)
    outputs, totals, stats, caps = {}, {}, {}, {}
    for sp in specs:
        parts: list[np.ndarray] = []
        lens: list[int] = []
        row_offsets = np.zeros(m + 1, np.int64)
        st = np.zeros(4, np.uint32)
        for k, c, elems in cols.rows(sp.key, sp.max_elems, picked):
            st[0] += c > len(elems)
            st[2] += c == 0
            for elem in elems:
                if sp.max_len is not None and elem.size > sp.max_len:
                    elem = elem[: int(sp.max_len)]
                    st[1] += 1
                parts.append(elem)
                lens.append(int(elem.size))
            row_offsets[k + 1] = row_offsets[k] + len(elems)
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

    kind = RL.OutputKind(
        parts=lambda sp: (RL.Part("values", torch.uint8, lambda cap: cap[1], "1-D torch.uint8 tensor"),
                          RL.Part("elem_offsets", torch.int64, lambda cap: cap[0] + 1, "1-D int64 tensor of at least one entry",
                                  least=1, zero_head=True)),
        offsets="row_offsets", capacity=_capacity_pair, cap_of=lambda v, e: (int(e.numel()) - 1, int(v.numel())), no_cap=(0, 0),
        item=lambda sp, slot, ts, r: (slot, sp.elems_limit, sp.limit, max(RL.numel(ts[1]) - 1, 0), RL.numel(ts[0]), RL.ptr(ts[0]),
                                      RL.ptr(ts[1]), r.data_ptr()),
        launch=launch_elems, width=2, empty_stat=2, batch=ElementsBatch)
    return RL.run(dec, check_elem_specs(specs), kind, rows=rows, capacity=capacity, out=out, stream=stream)
