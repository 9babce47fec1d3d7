"""Filtered row lists from decoded batches: the WHERE clause of the reference's ``select`` / ``query``,
over the decoded columns instead of an index frame, and on the device.

A ``where`` is a list whose items are ANDed; an item is a ``Term`` / ``Status``, or a list of them (an
OR group; ``is_in`` builds one). A ``Term`` compares one thing about a record's feature ``key`` with
an operand:

* ``subject="value"``: value ``index`` of the list (false, whatever the op, for a record that has no
  such value);
* ``subject="any"``: true iff some value of the list satisfies the op;
* ``subject="count"``: the number of values (0 for an absent key);
* ``subject="bytes_len"``: the byte length of the first element of a bytes list (0 if empty or absent).

Integers compare as signed 64-bit, float32 values by value (NaN is false under every op but ``!=``,
``-0.0 == 0.0``, denormals are not flushed). ``Status(op, operand)`` compares the record's decode status.

A ``BytesTerm`` compares an element of a bytes list with a byte string -- ``name == b"cat"``,
``path.startswith(b"train/")``, ``b"rose" in name`` -- by Python's own ``bytes`` semantics, for element
``index`` (``subject="value"``) or for any element (``subject="any"``); ``bytes_in`` builds the OR group
of ``id IN (...)``.

* ``HipDecoder.select`` / ``ShardDecoder.select`` evaluate a ``where`` on the device over the columns
  where the decode left them (``tfrg_result_select_rows``; with a ``BytesTerm``,
  ``tfrg_result_select_match``) and return a ``Selection`` whose ``.rows``
  -- a device tensor -- is ``rows=`` of ``dense`` / ``ragged`` / ``minibatches`` as it is; with
  ``capacity=`` nothing synchronises with the host;
* ``BatchResult.select`` / ``selectify`` compute the same function with numpy from fetched columns,
  record by record (the host path, and the reference the device path is tested against).
"""

from __future__ import annotations

import operator
from collections.abc import Sequence
from dataclasses import dataclass

import numpy as np

from tfr_reader import _native as N
from tfr_reader import dense as D

OPS = {"==": N.SEL_EQ, "!=": N.SEL_NE, "<": N.SEL_LT, "<=": N.SEL_LE, ">": N.SEL_GT, ">=": N.SEL_GE}
SUBJECTS = {"value": N.SEL_VALUE, "any": N.SEL_ANY, "count": N.SEL_COUNT, "bytes_len": N.SEL_BYTES_LEN}
_PY_OPS = {"==": operator.eq, "!=": operator.ne, "<": operator.lt, "<=": operator.le, ">": operator.gt,
           ">=": operator.ge}
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _int_operand(what: str, v) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{what}: the operand must be an integer, not {v!r}")
    if not I64_MIN <= int(v) <= I64_MAX:
        raise ValueError(f"{what}: the operand {v} does not fit int64")
    return int(v)


@dataclass(frozen=True)
class Term:
    """``key``'s feature of ``dtype`` ("int64", "int32", "float32", "uint8": it selects the slot kind
    as for ``Dense``; int32 compares the whole int64 too) under ``op`` ("==", "!=", "<", "<=", ">",
    ">=") against ``operand``. ``subject``: "value" (value ``index`` of the list), "any", "count" or
    "bytes_len" (uint8 only; "value" and "any" take the other dtypes)."""

    key: str
    dtype: str
    op: str
    operand: float | int
    subject: str = "value"
    index: int = 0

    def __post_init__(self) -> None:
        what = f"Term({self.key!r})"
        if not isinstance(self.key, str):
            raise TypeError(f"Term key must be a str, not {type(self.key).__name__}")
        if self.dtype not in D.DTYPES:
            raise ValueError(f"{what}: dtype must be one of {sorted(D.DTYPES)}, not {self.dtype!r}")
        if self.op not in OPS:
            raise ValueError(f"{what}: op must be one of {list(OPS)}, not {self.op!r}")
        if self.subject not in SUBJECTS:
            raise ValueError(f"{what}: subject must be one of {list(SUBJECTS)}, not {self.subject!r}")
        if self.subject in ("value", "any") and self.dtype == "uint8":
            raise ValueError(f"{what}: subject {self.subject!r} needs an int64 or float32 feature, not bytes")
        if self.subject == "bytes_len" and self.dtype != "uint8":
            raise ValueError(f"{what}: subject 'bytes_len' needs dtype 'uint8', not {self.dtype!r}")
        if isinstance(self.index, (bool, np.bool_)) or not isinstance(self.index, (int, np.integer)) \
                or not 0 <= int(self.index) < 1 << 32:
            raise ValueError(f"{what}: index must be in 0..2^32 - 1, not {self.index!r}")
        if self.index and self.subject != "value":
            raise ValueError(f"{what}: index is for subject 'value' alone")
        if self.is_float:
            if isinstance(self.operand, (bool, np.bool_)) or not isinstance(self.operand, (int, float, np.integer, np.floating)):
                raise TypeError(f"{what}: the operand must be a number, not {self.operand!r}")
        else:
            _int_operand(what, self.operand)

    @property
    def is_float(self) -> bool:
        return self.dtype == "float32" and self.subject in ("value", "any")

    @property
    def kind(self) -> int:
        return D.DTYPES[self.dtype][1]

    @property
    def operand_bits(self) -> int:
        """``tfrg_select_term.operand``."""
        if self.is_float:
            with np.errstate(over="ignore"):
                return int(np.array(self.operand, np.float32).view(np.uint32))
        return int(self.operand) & 0xFFFFFFFFFFFFFFFF

    @property
    def rhs(self):
        """The operand as the host path compares it."""
        if self.is_float:
            with np.errstate(over="ignore"):
                return float(np.float32(self.operand))
        return int(self.operand)


@dataclass(frozen=True)
class Status:
    """The record's decode status (0: decoded) under ``op`` against ``operand``."""

    op: str
    operand: int

    def __post_init__(self) -> None:
        if self.op not in OPS:
            raise ValueError(f"Status: op must be one of {list(OPS)}, not {self.op!r}")
        _int_operand("Status", self.operand)


def is_in(key: str, dtype: str, values: Sequence) -> list[Term]:
    """An OR group: ``key``'s first value is one of ``values``."""
    return [Term(key, dtype, "==", v) for v in values]


BYTES_OPS = {**OPS, "startswith": N.SEL_PREFIX, "endswith": N.SEL_SUFFIX, "contains": N.SEL_CONTAINS}
BYTES_SUBJECTS = {"value": N.SEL_BYTES, "any": N.SEL_BYTES_ANY}
# element op operand, as Python's own bytes objects have it
_PY_BYTES_OPS = {**_PY_OPS, "startswith": bytes.startswith, "endswith": bytes.endswith,
                 "contains": lambda element, operand: operand in element}


@dataclass(frozen=True)
class BytesTerm:
    """An element of ``key``'s bytes list under ``op`` against the byte string ``operand`` (``bytes``,
    or a ``str``, which is encoded as UTF-8; at most ``N.SEL_MAX_PATTERN`` bytes). ``op``: "==", "!=",
    "<", "<=", ">", ">=" compare as ``bytes`` objects do (unsigned bytes, the first difference decides,
    a proper prefix is less); "startswith", "endswith", "contains" as the ``bytes`` methods and ``in``
    do. ``subject``: "value" -- element ``index`` of the list, false whatever the op for a record that
    has no such element; "any" -- true iff some element of the list satisfies the op."""

    key: str
    op: str
    operand: bytes | str
    subject: str = "value"
    index: int = 0

    dtype = "uint8"  # (the slot kind, as for ``Dense`` and ``Term``)

    def __post_init__(self) -> None:
        what = f"BytesTerm({self.key!r})"
        if not isinstance(self.key, str):
            raise TypeError(f"BytesTerm key must be a str, not {type(self.key).__name__}")
        if self.op not in BYTES_OPS:
            raise ValueError(f"{what}: op must be one of {list(BYTES_OPS)}, not {self.op!r}")
        if self.subject not in BYTES_SUBJECTS:
            raise ValueError(f"{what}: subject must be one of {list(BYTES_SUBJECTS)}, not {self.subject!r}")
        if isinstance(self.index, (bool, np.bool_)) or not isinstance(self.index, (int, np.integer)) \
                or not 0 <= int(self.index) < 1 << 32:
            raise ValueError(f"{what}: index must be in 0..2^32 - 1, not {self.index!r}")
        if self.index and self.subject != "value":
            raise ValueError(f"{what}: index is for subject 'value' alone")
        if isinstance(self.operand, str):
            object.__setattr__(self, "operand", self.operand.encode("utf-8"))
        elif isinstance(self.operand, (bytes, bytearray)):
            object.__setattr__(self, "operand", bytes(self.operand))
        else:
            raise TypeError(f"{what}: the operand must be bytes or str, not {self.operand!r}")
        if len(self.operand) > N.SEL_MAX_PATTERN:
            raise ValueError(f"{what}: the operand has {len(self.operand)} bytes, more than {N.SEL_MAX_PATTERN}")

    @property
    def kind(self) -> int:
        return D.DTYPES[self.dtype][1]


def bytes_in(key: str, values: Sequence) -> list[BytesTerm]:
    """An OR group: ``key``'s first element is one of ``values``."""
    return [BytesTerm(key, "==", v) for v in values]


def pack_pattern(offset: int, length: int) -> int:
    """``tfrg_select_term.operand`` of a bytes term: the pattern's range in the call's patterns."""
    return offset | (length << 32)


_TERMS = (Term, Status, BytesTerm)


def check_where(where) -> list[list]:
    """``where`` as a list of OR groups (lists of ``Term`` / ``BytesTerm`` / ``Status``), validated:
    at most ``N.SEL_MAX_TERMS`` terms in at most 32 groups."""
    if isinstance(where, _TERMS) or not isinstance(where, Sequence) or isinstance(where, (str, bytes)):
        raise TypeError("where must be a list of Terms (ANDed) and lists of Terms (OR groups)")
    groups = []
    for item in where:
        if isinstance(item, _TERMS):
            groups.append([item])
        elif isinstance(item, Sequence) and not isinstance(item, (str, bytes)):
            for t in item:
                if not isinstance(t, _TERMS):
                    raise TypeError(f"an OR group holds Terms, not {type(t).__name__}")
            groups.append(list(item))
        else:
            raise TypeError(f"where items must be Terms or lists of Terms, not {type(item).__name__}")
    if len(groups) > 32:
        raise ValueError(f"at most 32 groups per where, not {len(groups)}")
    if sum(len(g) for g in groups) > N.SEL_MAX_TERMS:
        raise ValueError(f"at most {N.SEL_MAX_TERMS} terms per where, not {sum(len(g) for g in groups)}")
    return groups


# ---------------------------------------------------------------------- host path (numpy)
def select_mask(where, *, n: int, slot_key: Sequence[str | None], slot_kind: Sequence[int], row_splits: np.ndarray,
                slot_base: np.ndarray, i64: np.ndarray, f32: np.ndarray, status: np.ndarray,
                bytes_len: np.ndarray | None = None, bytes_offsets: np.ndarray | None = None,
                bytes_off: np.ndarray | None = None, buf: np.ndarray | None = None,
                bytes_data: np.ndarray | None = None) -> np.ndarray:
    """Which of the n records pass ``where`` (bool ``[n]``), from plain result columns, record by
    record and term by term. A key without a slot is absent from every record. A ``BytesTerm`` reads
    its elements as ``bytes``: from ``bytes_data`` / ``bytes_offsets`` where the bytes are
    materialized, else from the ``(bytes_off, bytes_len)`` views into ``buf``."""
    groups = check_where(where)
    cols = {}

    def element(e: int) -> bytes:
        if bytes_data is not None:
            return bytes_data[int(bytes_offsets[e]) : int(bytes_offsets[e + 1])].tobytes()
        return buf[int(bytes_off[e]) : int(bytes_off[e]) + int(bytes_len[e])].tobytes()

    def column(t):
        s = D.find_slot(slot_key, slot_kind, t.key, t.kind)
        if s is None:
            return None
        if s not in cols:
            cols[s] = (int(slot_base[s]), np.asarray(row_splits[s]).astype(np.int64).tolist())
        return cols[s]

    f32v = np.asarray(f32).view(np.float32)

    def true_for(t, g: int) -> bool:
        cmp = _PY_BYTES_OPS[t.op]
        if isinstance(t, Status):
            return cmp(int(status[g]), int(t.operand))
        col = column(t)
        lo, c = 0, 0
        if col is not None:
            base, rs = col
            lo, c = base + rs[g], rs[g + 1] - rs[g]
        if isinstance(t, BytesTerm):
            if t.subject == "value":
                return c > t.index and bool(cmp(element(lo + int(t.index)), t.operand))
            return any(cmp(element(lo + j), t.operand) for j in range(c))
        if t.subject == "count":
            return cmp(c, t.rhs)
        if t.subject == "bytes_len":
            ln = 0
            if c:
                ln = int(bytes_offsets[lo + 1]) - int(bytes_offsets[lo]) if bytes_offsets is not None else int(bytes_len[lo])
            return cmp(ln, t.rhs)
        src = f32v if t.is_float else i64
        conv = float if t.is_float else int
        if t.subject == "value":
            return c > t.index and bool(cmp(conv(src[lo + int(t.index)]), t.rhs))
        return any(cmp(conv(v), t.rhs) for v in src[lo : lo + c])

    mask = np.zeros(n, bool)
    for g in range(n):
        mask[g] = all(any(true_for(t, g) for t in grp) for grp in groups)
    return mask


def apply_mask(mask: np.ndarray, rows=None, row0: int = 0) -> tuple[np.ndarray, tuple[int, int]]:
    """The selection of a candidate list from the records' verdicts: (the entries of the passing
    candidates in candidate order as int64, (selected, skipped)). ``rows``: any integers (None: every
    record in order, entry k being k); candidate k is record ``rows[k] - row0``, skipped where that is
    outside the records."""
    n = len(mask)
    entries = list(range(n)) if rows is None else [int(v) for v in np.asarray(rows, object).reshape(-1)]
    got, skipped = [], 0
    for v in entries:
        if not row0 <= v < row0 + n:
            skipped += 1
        elif mask[v - row0]:
            got.append(v)
    return np.array(got, np.int64), (len(got), skipped)


def selectify(where, *, rows=None, row0: int = 0, **columns) -> tuple[np.ndarray, tuple[int, int]]:
    """``select_mask`` over the columns, then ``apply_mask``."""
    return apply_mask(select_mask(where, **columns), rows, row0)


def batch_columns(res) -> dict:
    return dict(n=len(res), slot_key=res.slot_key, slot_kind=res.slot_kind, row_splits=res.row_splits,
                slot_base=res.slot_base, i64=res.i64, f32=res.f32, status=res.status, bytes_len=res.bytes_len,
                bytes_offsets=res.bytes_offsets if res.bytes_data is not None else None, bytes_off=res.bytes_off,
                buf=res.buf, bytes_data=res.bytes_data)


def batch_select(res, where, rows=None, row0: int = 0) -> tuple[np.ndarray, tuple[int, int]]:
    """``BatchResult.select``: ``selectify`` over a fetched result's columns."""
    return selectify(where, rows=rows, row0=row0, **batch_columns(res))


# ---------------------------------------------------------------------- device path
def launch(dec, terms: Sequence[tuple], rows: tuple | None, m: int, row0: int, out: tuple | None, cap: int,
           count_ptr: int, stats_ptr: int | None, flags: int, consumer: int | None) -> None:
    """One select call: terms are (slot, subject, op, group, index, operand bits); ``rows``: (device
    pointer, TFRG_ROWS_* id) or None; ``out``: (device pointer or None, TFRG_ROWS_* id). A table with a
    bytes term (``fold``'s ``TermTable``, whose ``patterns`` its operands index) goes through
    ``tfrg_result_select_match``, any other through ``tfrg_result_select_rows``."""
    arr = (N.TfrgSelectTerm * max(len(terms), 1))()
    for a, (slot, subject, op, group, index, operand) in zip(arr, terms):
        a.slot, a.subject, a.op, a.group, a.index, a.reserved, a.operand = slot, subject, op, group, index, 0, operand
    ptr, rdt = rows if rows is not None else (None, 0)
    optr, odt = out if out is not None else (None, N.ROWS_I64)
    tail = (D.vp(ptr), rdt, m, row0, D.vp(optr), odt, cap, D.vp(count_ptr), D.vp(stats_ptr), flags, D.vp(consumer))
    if any(t[1] in (N.SEL_BYTES, N.SEL_BYTES_ANY) for t in terms):
        patterns = bytes(getattr(terms, "patterns", b""))
        N.check(dec._lib.tfrg_result_select_match(dec._ctx, arr, len(terms), patterns, len(patterns), *tail),
                "tfrg_result_select_match")
        return
    N.check(dec._lib.tfrg_result_select_rows(dec._ctx, arr, len(terms), *tail), "tfrg_result_select_rows")


class TermTable(list):
    """``fold``'s term table: a list of (slot, subject, op, group, index, operand bits), and the byte
    strings its bytes terms index (``patterns``: the operands back to back, each stored once)."""

    def __init__(self, terms=(), patterns: bytes = b"") -> None:
        super().__init__(terms)
        self.patterns = patterns


def fold(dec, groups: Sequence[Sequence]) -> TermTable | None:
    """The term table of ``groups`` on ``dec``. A key or kind that is not in its key table is absent
    from every record, so its terms are constants: value / any terms (bytes terms included) are false,
    count / bytes_len terms compare 0. A false term leaves its group, a true one removes its group;
    None: a group was emptied, nothing can pass. The operands of the bytes terms that are kept go into
    the table's ``patterns``, equal ones once (ValueError above ``N.SEL_MAX_PATTERN_BYTES``)."""
    terms = []
    blob = bytearray()
    g = 0
    for grp in groups:
        kept, true = [], False
        for t in grp:
            if isinstance(t, Status):
                kept.append((0, N.SEL_STATUS, OPS[t.op], 0, int(t.operand) & 0xFFFFFFFFFFFFFFFF))
                continue
            slot = D.resolve_slot(dec, t)
            if isinstance(t, BytesTerm):
                if slot is not None:
                    kept.append((slot, BYTES_SUBJECTS[t.subject], BYTES_OPS[t.op], int(t.index), t.operand))
                continue
            if slot is None:
                true |= t.subject in ("count", "bytes_len") and bool(_PY_OPS[t.op](0, t.rhs))
                continue
            kept.append((slot, SUBJECTS[t.subject], OPS[t.op], int(t.index), t.operand_bits))
        if true:
            continue
        if not kept:
            return None
        for slot, subject, op, index, bits in kept:
            if isinstance(bits, bytes):
                at = blob.find(bits)  # (an operand that is already there, as a whole or inside another)
                if at < 0:
                    at = len(blob)
                    blob += bits
                bits = pack_pattern(at, len(bits))
            terms.append((slot, subject, op, g, index, bits))
        g += 1
    if len(blob) > N.SEL_MAX_PATTERN_BYTES:
        raise ValueError(f"the byte-string operands of a where take at most {N.SEL_MAX_PATTERN_BYTES} bytes, "
                         f"not {len(blob)}")
    return TermTable(terms, bytes(blob))


class Selection:
    """A selected row list on the device. ``rows``: the entries of the passing candidates in
    candidate order -- with a capacity, a tensor of that length whose tail past ``count`` is -1 (``dense``
    and ``ragged`` skip such entries); without one, exactly ``count`` entries. ``count`` (it may exceed
    the capacity: ``overflowed``) and ``stats`` = (selected, skipped) are read back on first access."""

    def __init__(self, rows, capacity: int, count, stats) -> None:
        self.rows = rows
        self.capacity = capacity
        self._count = count  # an int, or a function returning it
        self._stats = stats

    @property
    def count(self) -> int:
        if callable(self._count):
            self._count = int(self._count())
        return self._count

    @property
    def stats(self) -> tuple[int, int]:
        if callable(self._stats):
            self._stats = tuple(int(x) for x in self._stats())
        return self._stats

    @property
    def overflowed(self) -> bool:
        return self.count > self.capacity


def _select(decs: Sequence, spans: Sequence[tuple[int, int]], n: int, device: int, where, *, rows=None, capacity=None,
            dtype: str = "int64", out=None, stream: int | None = None) -> Selection:
    """The selection over the contexts ``decs``, context k holding rows ``spans[k]`` = [r0, r1) of the
    n rows: one call per context in order, all into one list and one count."""
    import torch  # noqa: PLC0415

    groups = check_where(where)
    if dtype not in D.ROW_DTYPES:
        raise ValueError(f"dtype must be one of {sorted(D.ROW_DTYPES)}, not {dtype!r}")
    if capacity is not None and (isinstance(capacity, (bool, np.bool_)) or not isinstance(capacity, (int, np.integer))
                                 or capacity < 0):
        raise ValueError(f"capacity must be a non-negative integer, not {capacity!r}")
    dev = torch.device("cuda", device)
    tdt = D.torch_dtypes()
    consumer = D.ConsumerStream.wrapping(stream, dev)
    with torch.cuda.device(dev), torch.cuda.stream(consumer.cur):
        d_rows, m = (None, n) if rows is None else D.device_rows(rows, n, device)
        exact = capacity is None and out is None
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dim() != 1 or out.dtype not in (torch.int32, torch.int64) \
                    or out.device != dev or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous 1-D int32 or int64 tensor on {dev}")
            cap = int(out.numel())
        else:
            cap = m if exact else int(capacity)
            # (the tail past the count stays -1: an entry that every consumer of a row list skips)
            out = torch.empty(cap, dtype=tdt[dtype], device=dev) if exact else \
                torch.full((cap,), -1, dtype=tdt[dtype], device=dev)
        odt = N.ROWS_I64 if out.dtype == torch.int64 else N.ROWS_I32
        count_t = torch.zeros(1, dtype=torch.int64, device=dev)
        stats_t = torch.zeros((max(len(decs), 1), 2), dtype=torch.int32, device=dev)
        consumer.begin()  # (once around the loop over the contexts)
        rw = D.rows_arg(d_rows) if d_rows is not None else None
        ran = 0
        unlaunched = []  # per context without a launch: how many candidates it skips
        for k, (dec, (r0, r1)) in enumerate(zip(decs, spans)):
            terms = fold(dec, groups) if r1 > r0 else None
            if terms is None:
                # nothing of this context can pass: no launch, and its candidates count on the host side
                if d_rows is None:
                    unlaunched.append(m - max(0, min(r1, m) - min(r0, m)))
                elif isinstance(rows, torch.Tensor):
                    unlaunched.append(m - ((d_rows >= r0) & (d_rows < r1)).sum())
                else:
                    a = np.asarray(rows, np.int64)
                    unlaunched.append(m - int(((a >= r0) & (a < r1)).sum()))
                continue
            launch(dec, terms, rw, m, r0, (out.data_ptr() if cap else None, odt), cap, count_t.data_ptr(),
                   stats_t[k].data_ptr(), N.SEL_APPEND if ran else 0, consumer.handle)
            ran += 1
        consumer.end()
        n_ctx = len(decs)

        def stats() -> tuple[int, int]:
            # every context skips the candidates that are not its own: over the contexts that is the
            # candidates in no context plus (contexts - 1) * m
            host = stats_t.cpu().numpy().view(np.uint32).astype(np.int64)
            skipped = int(host[:, 1].sum()) + sum(int(x) for x in unlaunched)
            if not n_ctx:
                return 0, m
            return int(host[:, 0].sum()), skipped - (n_ctx - 1) * m

        if exact:
            total = int(count_t.cpu()[0])  # the step's one synchronisation
            return Selection(out[:total], total, total, stats)
    return Selection(out, cap, lambda: int(count_t.cpu()[0]), stats)


def decoder_select(dec, where, *, rows=None, capacity=None, dtype: str = "int64", out=None,
                   stream: int | None = None) -> Selection:
    """``HipDecoder.select``: the rows of the decoder's last decode that pass ``where``, as a device
    row list in candidate order.

    ``rows``: the candidates, as ``dense(rows=)`` -- a 1-D contiguous int32 / int64 tensor on the
    device, used where it is (an entry out of range is skipped and counted), or a host sequence,
    range-checked here (IndexError) and uploaded; None: every record in order.

    ``capacity``: the length of ``.rows``, which is prefilled with -1. With it the call enqueues its
    work and returns without a host synchronisation; ``.overflowed`` tells (on first access) whether
    more rows passed, in which case ``.rows`` holds the first ``capacity`` of them. Without it the
    count is read back once and ``.rows`` is exact. ``dtype``: "int64" or "int32".

    ``out``: a 1-D int32 / int64 tensor to write into instead (its length is the capacity; nothing
    past the stored rows is written). ``stream``: a HIP stream handle as the consumer stream
    (default: the current torch stream)."""
    n = D.last_n(dec)
    return _select([dec], [(0, n)], n, dec.device, where, rows=rows, capacity=capacity, dtype=dtype, out=out,
                   stream=stream)


def shard_select(sd, plan: np.ndarray, where, *, rows=None, capacity=None, dtype: str = "int64", out=None,
                 stream: int | None = None) -> Selection:
    """``ShardDecoder.select``: ``decoder_select`` over the whole plan of the last ``decode_device`` /
    ``decode_device32``. Every batch context takes the same candidates with ``row0 = plan[k, 0]`` and
    appends what it holds of them to one list, in plan order: with ``rows=None`` the list ascends."""
    n = int(plan[-1, 1]) if len(plan) else 0
    spans = [(int(r0), int(r1)) for r0, r1, _, _ in plan.tolist()]
    return _select(sd.decs[: len(plan)], spans, n, sd.device, where, rows=rows, capacity=capacity, dtype=dtype, out=out,
                   stream=stream)


def selected_permutation(dec, where, plan, seed: int):
    """The rows that pass ``where`` (one select, one read-back of the count), permuted on the device
    by a generator seeded with ``seed``: the epoch order of ``minibatches(where=)``."""
    import torch  # noqa: PLC0415

    sel = shard_select(dec, plan, where) if plan is not None else decoder_select(dec, where)
    dev = torch.device("cuda", dec.device)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    return sel.rows[torch.randperm(sel.count, generator=gen, device=dev)]
