"""Element ids: the elements of a ``bytes_list`` feature as the integers a model takes -- an exact lookup
in a vocabulary, a hash into N buckets, or both (``tf.strings.to_hash_bucket_fast`` /
``StaticVocabularyTable``, Keras ``StringLookup`` / ``Hashing``; the bucket numbers are this library's
own, ``hash64``, not FarmHash's).

``HipDecoder.element_ids`` computes them on the device from the last decode (tfrg_result_elem_ids:
one int64 per element that ``ragged_elements`` would describe, in its order, with its row offsets);
``BatchResult.element_ids`` / ``idsify`` are the numpy path over fetched columns, with a pure-Python
table.

    vocab = Vocabulary([b"cat", b"dog"], device=0)
    got = dec.element_ids([ElementIds("image/object/class/text", vocab, num_oov_buckets=8)])
    ids, row_offsets = got["image/object/class/text"]      # torch.nn.EmbeddingBag(ids, row_offsets[:-1])
"""

from __future__ import annotations

import ctypes as C
from collections.abc import Mapping, Sequence
from dataclasses import dataclass

import numpy as np

from tfr_reader import _native as N
from tfr_reader import _rowlist as RL
from tfr_reader import dense as D

IDS_STAT_NAMES = ("rows_truncated", "unmatched", "empty", "skipped")
_M64 = (1 << 64) - 1


def hash64_py(b: bytes) -> int:
    """``tfrg_hash64`` restated (include/tfrg.h): what ``idsify`` buckets with."""
    h = 0xCBF29CE484222325
    for i in range(0, len(b), 8):
        h = ((h ^ int.from_bytes(b[i : i + 8], "little")) * 0x100000001B3) & _M64
    h ^= len(b)
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & _M64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & _M64
    return h ^ (h >> 33)


def hash64(b: bytes) -> int:
    """``tfrg_hash64`` of a byte string, by the library."""
    b = bytes(b)
    return int(N.lib().tfrg_hash64(b, len(b)))


def _as_bytes(w) -> bytes:
    if isinstance(w, str):
        return w.encode("utf-8")
    if isinstance(w, (bytes, bytearray, memoryview, np.bytes_)):
        return bytes(w)
    raise TypeError(f"a word must be bytes or str, not {type(w).__name__}")


class Vocabulary:
    """Distinct words (bytes; a str is its UTF-8 bytes) with int64 ids (default: a word's position).
    Owns a ``tfrg_vocab``: ``device=None`` builds the host table alone, ``device=k`` also uploads it
    to GPU k for ``HipDecoder.element_ids`` of a decoder on that device. ``lookup`` is the library's
    host lookup; ``id_of`` the pure-Python one (a dict) the numpy path uses. Keep the object until
    the device work that uses it has been queued; ``close`` (or collection) synchronises that device."""

    def __init__(self, words: Sequence, ids: Sequence[int] | None = None, device: int | None = None) -> None:
        self.words = [_as_bytes(w) for w in words]
        n = len(self.words)
        if ids is not None and len(ids) != n:
            raise ValueError(f"{len(ids)} ids for {n} words")
        self.ids = np.arange(n, dtype=np.int64) if ids is None else np.ascontiguousarray(ids, np.int64)
        self._dict = {w: int(i) for w, i in zip(self.words, self.ids)}
        if len(self._dict) != n:
            raise ValueError("a word occurs twice in the vocabulary")
        self.device = device
        offs = np.zeros(n + 1, np.uint64)
        np.cumsum([len(w) for w in self.words], out=offs[1:])
        self._lib = N.lib()
        self._ptr = C.c_void_p()
        N.check(self._lib.tfrg_vocab_create(-1 if device is None else int(device), b"".join(self.words), N.ptr(offs, N.u64p),
                                            n, N.ptr(self.ids, N.i64p) if ids is not None else None, C.byref(self._ptr)),
                "tfrg_vocab_create")

    def __len__(self) -> int:
        return len(self.words)

    @property
    def info(self) -> dict[str, int]:
        """``n_words``, ``capacity`` and ``max_probe`` of the table, ``device_bytes`` of its upload."""
        nw, cap, db = C.c_uint64(), C.c_uint64(), C.c_uint64()
        mp = C.c_uint32()
        N.check(self._lib.tfrg_vocab_info(self._handle(), C.byref(nw), C.byref(cap), C.byref(mp), C.byref(db)), "tfrg_vocab_info")
        return {"n_words": nw.value, "capacity": cap.value, "max_probe": mp.value, "device_bytes": db.value}

    def _handle(self) -> C.c_void_p:
        if not self._ptr:
            raise ValueError("the vocabulary is closed")
        return self._ptr

    def lookup(self, b, missing: int = -1) -> int:
        b = _as_bytes(b)
        return int(self._lib.tfrg_vocab_lookup_host(self._handle(), b, len(b), missing))

    def id_of(self, b: bytes, missing: int = -1) -> int:
        return self._dict.get(b, missing)

    def close(self) -> None:
        if getattr(self, "_ptr", None):
            p, self._ptr = self._ptr, C.c_void_p()
            N.check(self._lib.tfrg_vocab_destroy(p), "tfrg_vocab_destroy")

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:  # noqa: BLE001 (interpreter shutdown)
            pass


@dataclass(frozen=True, eq=False)
class ElementIds(RL.NamedSpec):
    """One id output: every element of ``key``'s ``bytes_list`` as an int64. An element equal to a word
    of ``vocab`` gets the word's id; else, with ``num_oov_buckets``, ``oov_base + hash64(element) %
    num_oov_buckets`` (``oov_base`` default: ``len(vocab)``, or 0 without a vocabulary); else
    ``default_id``. ``max_elems``: a row contributes at most its first that many elements. ``name``: the
    output's name in the result (default: the key)."""

    key: str
    vocab: Vocabulary | None = None
    num_oov_buckets: int = 0
    oov_base: int | None = None
    default_id: int = -1
    max_elems: int | None = None
    name: str | None = None

    dtype = "uint8"  # (the slot kind, as ``Ragged.dtype`` selects it)

    def __post_init__(self) -> None:
        if not isinstance(self.key, str):
            raise TypeError(f"ElementIds key must be a str, not {type(self.key).__name__}")
        if self.vocab is not None and not isinstance(self.vocab, Vocabulary):
            raise TypeError(f"ElementIds({self.key!r}): vocab must be a Vocabulary, not {type(self.vocab).__name__}")
        nb = self.num_oov_buckets
        if not isinstance(nb, (int, np.integer)) or not 0 <= int(nb) < 1 << 64:
            raise ValueError(f"ElementIds({self.key!r}): num_oov_buckets must be in 0..2^64 - 1, not {nb!r}")
        if self.vocab is None and not nb:
            raise ValueError(f"ElementIds({self.key!r}): give a vocab, num_oov_buckets, or both")
        me = self.max_elems
        if me is not None and (not isinstance(me, (int, np.integer)) or not 1 <= int(me) < 1 << 32):
            raise ValueError(f"ElementIds({self.key!r}): max_elems must be None or in 1..2^32 - 1, not {me!r}")
        for what, v in (("oov_base", self.base), ("default_id", self.default_id)):
            if not -(1 << 63) <= int(v) < 1 << 63:
                raise ValueError(f"ElementIds({self.key!r}): {what} must be an int64, not {v!r}")

    @property
    def base(self) -> int:
        """``tfrg_ids_spec.oov_base``."""
        if self.oov_base is not None:
            return int(self.oov_base)
        return len(self.vocab) if self.vocab is not None else 0

    def id_of(self, b: bytes) -> tuple[int, bool]:
        """(the id of an element with bytes ``b``, whether a word matched it), in pure Python."""
        if self.vocab is not None:
            i = self.vocab._dict.get(b)
            if i is not None:
                return i, True
        if self.num_oov_buckets:
            v = self.base + hash64_py(b) % int(self.num_oov_buckets)
            return (v + (1 << 63)) % (1 << 64) - (1 << 63), False  # (int64 arithmetic wraps)
        return int(self.default_id), False


def check_specs(specs: Sequence[ElementIds]) -> list[ElementIds]:
    return RL.check_named_specs(specs, ElementIds, N.IDS_MAX_SPECS)


class IdsBatch(RL.RowListBatch):
    """name -> ``(ids, row_offsets)`` (torch tensors on the decoder's device, numpy arrays on the host
    path). ``capacity[name]``: the elements ``ids`` can hold; ``totals[name]``: E, the elements of the
    rows; ``stats[name]``: the four counters ``IDS_STAT_NAMES`` as a uint32 array; ``overflowed[name]``:
    E is above the capacity (the stored prefix is still right, the row offsets complete). The last
    three are read back from the device on first access."""


# ---------------------------------------------------------------------- host path (numpy)
def idsify(specs: Sequence[ElementIds], *, n: int, slot_key: Sequence[str | None], slot_kind: Sequence[int],
           row_splits: np.ndarray, slot_base: np.ndarray, bytes_off: np.ndarray | None = None,
           bytes_len: np.ndarray | None = None, buf: np.ndarray | None = None, bytes_data: np.ndarray | None = None,
           bytes_offsets: np.ndarray | None = None, rows=None) -> IdsBatch:
    """The id outputs of ``specs`` from plain result columns (as ``ragged.elementify`` takes them),
    element by element in Python: a dict for the vocabulary, ``hash64_py`` for the buckets. A key
    without a slot gives all-empty rows. ``rows``: output row k is record ``rows[k]`` (any order,
    repeats allowed; IndexError for one outside [0, n))."""
    specs = check_specs(specs)
    cols = RL.BytesColumns(slot_key, slot_kind, row_splits, slot_base, bytes_off, bytes_len, buf, bytes_data, bytes_offsets)
    picked = list(range(n)) if rows is None else D.host_rows(rows, n).tolist()
    m = len(picked)
    outputs, totals, stats = {}, {}, {}
    for sp in specs:
        ids: list[int] = []
        row_offsets = np.zeros(m + 1, np.int64)
        st = np.zeros(4, np.uint32)
        for k, c, elems in cols.rows(sp.key, sp.max_elems, picked):
            st[0] += c > len(elems)
            st[2] += c == 0
            for elem in elems:
                i, hit = sp.id_of(elem.tobytes())
                st[1] += not hit
                ids.append(i)
            row_offsets[k + 1] = row_offsets[k] + len(elems)
        k = sp.out_name
        outputs[k] = (np.asarray(ids, np.int64).reshape(-1), row_offsets)
        totals[k] = len(ids)
        stats[k] = st
    return IdsBatch(outputs, dict(totals), totals, stats)


def batch_element_ids(res, specs: Sequence[ElementIds], rows=None) -> IdsBatch:
    """``BatchResult.element_ids``: ``idsify`` over a fetched result's columns."""
    return idsify(specs, n=len(res), slot_key=res.slot_key, slot_kind=res.slot_kind, row_splits=res.row_splits,
                  slot_base=res.slot_base, bytes_off=res.bytes_off, bytes_len=res.bytes_len, buf=res.buf,
                  bytes_data=res.bytes_data, bytes_offsets=res.bytes_offsets, rows=rows)


# ---------------------------------------------------------------------- device path
def launch_ids(dec, items: Sequence[tuple], rows: tuple | None, m: int, row0: int, totals_ptr: int | None,
               stats_ptr: int | None, consumer: int | None) -> None:
    """One ``tfrg_result_elem_ids`` call: items are (slot, max_elems, vocab handle or None,
    num_oov_buckets, oov_base, default_id, elem_cap, ids pointer or None, row_offsets pointer); ``rows``:
    (device pointer, TFRG_ROWS_* id) or None."""
    arr = (N.TfrgIdsSpec * len(items))()
    for a, (slot, max_elems, vocab, nb, base, default, elem_cap, ids, row_offsets) in zip(arr, items):
        a.slot, a.max_elems, a.reserved0, a.reserved1, a.vocab = slot, max_elems, 0, 0, vocab
        a.num_oov_buckets, a.oov_base, a.default_id, a.elem_cap = nb, base, default, elem_cap
        a.ids, a.row_offsets = ids, row_offsets
    ptr, rdt = rows if rows is not None else (None, 0)
    N.check(dec._lib.tfrg_result_elem_ids(dec._ctx, arr, len(items), D.vp(ptr), rdt, m, row0, D.vp(totals_ptr),
                                          D.vp(stats_ptr), D.vp(consumer)), "tfrg_result_elem_ids")


def _capacity(cap, what: str) -> int | None:
    if cap is None:
        return None
    if not isinstance(cap, (int, np.integer)) or isinstance(cap, bool) or cap < 0:
        raise ValueError(f"{what} must be a non-negative integer (elements), not {cap!r}")
    return int(cap)


def decoder_element_ids(dec, specs: Sequence[ElementIds], *, rows=None, capacity=None, out: Mapping | None = None,
                        stream: int | None = None) -> IdsBatch:
    """``HipDecoder.element_ids``: the id outputs of the decoder's last decode, as torch tensors on its
    device: name -> ``(ids, row_offsets)``.

    ``rows``, ``stream``: as ``ragged_elements``. ``capacity``: the elements an ``ids`` tensor holds,
    or name -> that. With it the call enqueues its work and returns without a host synchronisation;
    ``.overflowed`` tells (on first access) whether E was above it: the stored prefix is right and
    the row offsets complete. Entries of ``ids`` past E are unspecified. Without it the call runs
    twice: row offsets and E only (no element is read), one device-to-host copy (the step's single
    synchronisation), exact allocations, then the ids.

    ``out``: name -> ``(ids, row_offsets)`` to write into (int64 ``[elements]``, int64 ``[m + 1]``).
    A spec's vocabulary must have been made with ``device=`` this decoder's."""
    import torch  # noqa: PLC0415

    specs = check_specs(specs)
    for sp in specs:
        if sp.vocab is not None and sp.vocab.device != dec.device:
            raise ValueError(f"ElementIds({sp.key!r}): its vocabulary was made with device={sp.vocab.device}, "
                             f"the decoder is on device {dec.device}")
    kind = RL.OutputKind(
        parts=lambda sp: (RL.Part("ids", torch.int64, lambda cap: cap, "1-D int64 tensor"),),
        offsets="row_offsets", capacity=_capacity, cap_of=lambda v: int(v.numel()), no_cap=0,
        item=lambda sp, slot, ts, r: (slot, sp.elems_limit, sp.vocab._handle().value if sp.vocab is not None else None,
                                      int(sp.num_oov_buckets), sp.base, int(sp.default_id), RL.numel(ts[0]), RL.ptr(ts[0]),
                                      r.data_ptr()),
        launch=launch_ids, width=1, empty_stat=2, batch=IdsBatch)
    return RL.run(dec, specs, kind, rows=rows, capacity=capacity, out=out, stream=stream)
