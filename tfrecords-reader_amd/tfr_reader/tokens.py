"""Token ids: a text feature (one sentence per ``bytes_list`` element) as one integer per word --
``tf.strings.split`` + ``StringLookup`` / ``Hashing``, or Keras ``TextVectorization(split="whitespace",
standardize="lower")``. The elements are split at ASCII delimiter bytes, optionally lower-cased, and each
token gets its id by the rule of ``tfr_reader.ids`` (a vocabulary word, a hash bucket, or a default).

``HipDecoder.token_ids`` computes them on the device from the last decode (tfrg_result_token_ids);
``BatchResult.token_ids`` / ``tokenize`` are the numpy path over fetched columns, with a pure-Python table.

    vocab = Vocabulary([b"the", b"cat"], device=0)
    got = dec.token_ids([TokenIds("title", vocab, num_oov_buckets=8, lower=True)])
    ids, row_offsets = got["title"]                        # torch.nn.EmbeddingBag(ids, row_offsets[:-1])
"""

from __future__ import annotations

from collections.abc import Mapping, Sequence
from dataclasses import dataclass

import numpy as np

from tfr_reader import _native as N
from tfr_reader import _rowlist as RL
from tfr_reader import dense as D
from tfr_reader import ids as I  # noqa: N812

TOK_STAT_NAMES = ("rows_truncated", "unmatched", "empty", "skipped")
WHITESPACE = b" \t\n\r\x0b\x0c"  # what bytes.split() splits on


@dataclass(frozen=True, eq=False)
class TokenIds(RL.NamedSpec):
    """One id output: every token of ``key``'s ``bytes_list`` elements as an int64. A token is a maximal
    run of bytes outside ``delimiters`` (ASCII bytes) inside one element; with ``lower`` its ``A``..``Z``
    become ``a``..``z`` first. Its id is ``ElementIds``'s: a word of ``vocab`` equal to it gives the word's
    id; else, with ``num_oov_buckets``, ``oov_base + hash64(token) % num_oov_buckets`` (``oov_base``
    default: ``len(vocab)``, or 0 without a vocabulary); else ``default_id``. ``max_tokens``: a row
    contributes at most its first that many tokens; ``max_elems``: of its first that many elements.
    ``name``: the output's name in the result (default: the key)."""

    key: str
    vocab: I.Vocabulary | None = None
    num_oov_buckets: int = 0
    lower: bool = False
    delimiters: bytes = WHITESPACE
    max_tokens: int | None = None
    max_elems: int | None = None
    oov_base: int | None = None
    default_id: int = -1
    name: str | None = None

    dtype = "uint8"  # (the slot kind, as ``Ragged.dtype`` selects it)

    def __post_init__(self) -> None:
        what = f"TokenIds({self.key!r})"
        if not isinstance(self.key, str):
            raise TypeError(f"TokenIds key must be a str, not {type(self.key).__name__}")
        if self.vocab is not None and not isinstance(self.vocab, I.Vocabulary):
            raise TypeError(f"{what}: vocab must be a Vocabulary, not {type(self.vocab).__name__}")
        nb = self.num_oov_buckets
        if not isinstance(nb, (int, np.integer)) or not 0 <= int(nb) < 1 << 64:
            raise ValueError(f"{what}: num_oov_buckets must be in 0..2^64 - 1, not {nb!r}")
        if self.vocab is None and not nb:
            raise ValueError(f"{what}: give a vocab, num_oov_buckets, or both")
        if not isinstance(self.delimiters, (bytes, bytearray)) or not self.delimiters:
            raise TypeError(f"{what}: delimiters must be a non-empty bytes object")
        if max(self.delimiters) >= 0x80:
            raise ValueError(f"{what}: a delimiter must be an ASCII byte (< 0x80), not 0x{max(self.delimiters):02x}")
        for field in ("max_tokens", "max_elems"):
            v = getattr(self, field)
            if v is not None and (not isinstance(v, (int, np.integer)) or not 1 <= int(v) < 1 << 32):
                raise ValueError(f"{what}: {field} must be None or in 1..2^32 - 1, not {v!r}")
        for field, v in (("oov_base", self.base), ("default_id", self.default_id)):
            if not -(1 << 63) <= int(v) < 1 << 63:
                raise ValueError(f"{what}: {field} must be an int64, not {v!r}")

    @property
    def base(self) -> int:
        """``tfrg_tok_spec.oov_base``."""
        if self.oov_base is not None:
            return int(self.oov_base)
        return len(self.vocab) if self.vocab is not None else 0

    @property
    def tokens_limit(self) -> int:
        """``tfrg_tok_spec.max_tokens`` (0: every token)."""
        return int(self.max_tokens) if self.max_tokens is not None else 0

    @property
    def delim_words(self) -> tuple[int, int]:
        """``tfrg_tok_spec.delims``: bit b of the 128 is set for a delimiter byte b."""
        bits = sum(1 << b for b in set(self.delimiters))
        return bits & ((1 << 64) - 1), bits >> 64

    def split(self, elem: bytes) -> list[bytes]:
        """The tokens of one element, lower-cased if asked."""
        d = bytes(self.delimiters)
        toks = elem.translate(bytes.maketrans(d, d[:1] * len(d))).split(d[:1])
        return [t.lower() if self.lower else t for t in toks if t]

    id_of = I.ElementIds.id_of


def check_specs(specs: Sequence[TokenIds]) -> list[TokenIds]:
    return RL.check_named_specs(specs, TokenIds, N.TOK_MAX_SPECS)


class TokensBatch(I.IdsBatch):
    """``IdsBatch`` whose totals count tokens: name -> ``(ids, row_offsets)``, with ``capacity``, ``totals``
    (T), ``stats`` (``TOK_STAT_NAMES``) and ``overflowed``."""


# ---------------------------------------------------------------------- host path (numpy)
def tokenize(specs: Sequence[TokenIds], *, n: int, slot_key: Sequence[str | None], slot_kind: Sequence[int],
             row_splits: np.ndarray, slot_base: np.ndarray, bytes_off: np.ndarray | None = None,
             bytes_len: np.ndarray | None = None, buf: np.ndarray | None = None, bytes_data: np.ndarray | None = None,
             bytes_offsets: np.ndarray | None = None, rows=None) -> TokensBatch:
    """The token outputs of ``specs`` from plain result columns (as ``ids.idsify`` takes them), token by
    token in Python. A key without a slot gives all-empty rows. ``rows``: output row k is record
    ``rows[k]`` (any order, repeats allowed; IndexError for one outside [0, n))."""
    specs = check_specs(specs)
    cols = RL.BytesColumns(slot_key, slot_kind, row_splits, slot_base, bytes_off, bytes_len, buf, bytes_data, bytes_offsets)
    picked = list(range(n)) if rows is None else D.host_rows(rows, n).tolist()
    m = len(picked)
    outputs, totals, stats = {}, {}, {}
    for sp in specs:
        ids: list[int] = []
        row_offsets = np.zeros(m + 1, np.int64)
        st = np.zeros(4, np.uint32)
        for k, _, elems in cols.rows(sp.key, sp.max_elems, picked):
            toks = [t for elem in elems for t in sp.split(elem.tobytes())]
            if sp.max_tokens is not None and len(toks) > sp.max_tokens:
                st[0] += 1
                toks = toks[: sp.max_tokens]
            st[2] += not toks
            for t in toks:
                i, hit = sp.id_of(t)
                st[1] += not hit
                ids.append(i)
            row_offsets[k + 1] = row_offsets[k] + len(toks)
        k = sp.out_name
        outputs[k] = (np.asarray(ids, np.int64).reshape(-1), row_offsets)
        totals[k] = len(ids)
        stats[k] = st
    return TokensBatch(outputs, dict(totals), totals, stats)


def batch_token_ids(res, specs: Sequence[TokenIds], rows=None) -> TokensBatch:
    """``BatchResult.token_ids``: ``tokenize`` over a fetched result's columns."""
    return tokenize(specs, n=len(res), slot_key=res.slot_key, slot_kind=res.slot_kind, row_splits=res.row_splits,
                    slot_base=res.slot_base, bytes_off=res.bytes_off, bytes_len=res.bytes_len, buf=res.buf,
                    bytes_data=res.bytes_data, bytes_offsets=res.bytes_offsets, rows=rows)


# ---------------------------------------------------------------------- device path
def launch_tokens(dec, items: Sequence[tuple], rows: tuple | None, m: int, row0: int, totals_ptr: int | None,
                  stats_ptr: int | None, consumer: int | None) -> None:
    """One ``tfrg_result_token_ids`` call: items are (slot, max_elems, max_tokens, flags, (delims lo, hi),
    vocab handle or None, num_oov_buckets, oov_base, default_id, tok_cap, ids pointer or None, row_offsets
    pointer); ``rows``: (device pointer, TFRG_ROWS_* id) or None."""
    arr = (N.TfrgTokSpec * len(items))()
    for a, (slot, max_elems, max_tokens, flags, delims, vocab, nb, base, default, tok_cap, ids, row_offsets) in zip(arr, items):
        a.slot, a.max_elems, a.max_tokens, a.flags, a.vocab = slot, max_elems, max_tokens, flags, vocab
        a.delims[0], a.delims[1] = delims
        a.num_oov_buckets, a.oov_base, a.default_id, a.tok_cap = nb, base, default, tok_cap
        a.ids, a.row_offsets = ids, row_offsets
    ptr, rdt = rows if rows is not None else (None, 0)
    N.check(dec._lib.tfrg_result_token_ids(dec._ctx, arr, len(items), D.vp(ptr), rdt, m, row0, D.vp(totals_ptr),
                                           D.vp(stats_ptr), D.vp(consumer)), "tfrg_result_token_ids")


def decoder_token_ids(dec, specs: Sequence[TokenIds], *, rows=None, capacity=None, out: Mapping | None = None,
                      stream: int | None = None) -> TokensBatch:
    """``HipDecoder.token_ids``: the token outputs of the decoder's last decode, as torch tensors on its
    device: name -> ``(ids, row_offsets)``. ``rows``, ``capacity``, ``out`` and ``stream`` are
    ``decoder_element_ids``'s, counted in tokens: with every capacity known the call enqueues its work
    and returns without a host synchronisation; without it the call runs twice (one sweep that counts,
    one device-to-host copy of T, exact allocations, then the ids). A spec's vocabulary must have been
    made with ``device=`` this decoder's."""
    import torch  # noqa: PLC0415

    specs = check_specs(specs)
    for sp in specs:
        if sp.vocab is not None and sp.vocab.device != dec.device:
            raise ValueError(f"TokenIds({sp.key!r}): its vocabulary was made with device={sp.vocab.device}, "
                             f"the decoder is on device {dec.device}")
    kind = RL.OutputKind(
        parts=lambda sp: (RL.Part("ids", torch.int64, lambda cap: cap, "1-D int64 tensor"),),
        offsets="row_offsets", capacity=I._capacity, cap_of=lambda v: int(v.numel()), no_cap=0,
        item=lambda sp, slot, ts, r: (slot, sp.elems_limit, sp.tokens_limit, N.TOK_LOWER_ASCII if sp.lower else 0, sp.delim_words,
                                      sp.vocab._handle().value if sp.vocab is not None else None, int(sp.num_oov_buckets),
                                      sp.base, int(sp.default_id), RL.numel(ts[0]), RL.ptr(ts[0]), r.data_ptr()),
        launch=launch_tokens, width=1, empty_stat=2, batch=TokensBatch)
    return RL.run(dec, specs, kind, rows=rows, capacity=capacity, out=out, stream=stream)
