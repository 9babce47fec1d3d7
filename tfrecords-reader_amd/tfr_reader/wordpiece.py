"""WordPiece ids: a text feature as the subword ids that BERT-family encoders take. The elements are
split at ASCII delimiters, ASCII punctuation is split off as words of its own, every word is cut greedily
into the longest pieces of a ``vocab.txt``-style vocabulary (continuation pieces carry a prefix, ``##ing``),
a word that cannot be covered becomes ``[UNK]``, and a row may be bracketed by ``[CLS]`` ... ``[SEP]``.

``HipDecoder.wordpiece_ids`` computes them on the device from the last decode (tfrg_result_wordpiece_ids);
``BatchResult.wordpiece_ids`` / ``wordpiece`` are the numpy path over fetched columns, in pure Python.

    vocab = WordPieceVocab(open("vocab.txt", "rb").read().split(b"\\n"), device=0)
    got = dec.wordpiece_ids([WordPieceIds("title", vocab, max_pieces=128, special=True)])
    ids, row_offsets = got["title"]

Not done (include/tfrg.h says the same): Unicode normalisation, accent stripping, CJK splitting,
non-ASCII punctuation and whitespace; a piece-to-word map; BPE; a padded ``[m, max_pieces]`` output.
"""

from __future__ import annotations

from collections.abc import Mapping, Sequence
from dataclasses import dataclass

import numpy as np

from tfr_reader import _native as N
from tfr_reader import _rowlist as RL
from tfr_reader import dense as D
from tfr_reader import ids as I  # noqa: N812
from tfr_reader.tokens import WHITESPACE

WP_STAT_NAMES = ("rows_truncated", "unknown_words", "empty", "skipped")
ASCII_PUNCTUATION = bytes(b for b in range(33, 127) if not chr(b).isalnum())  # BERT's ASCII punctuation
DEFAULT_WORD_BYTES = 100


class WordPieceVocab:
    """One ``vocab.txt``-style list of words as the two vocabularies of the device path: ``first`` holds
    the words without ``prefix`` (they may begin a word), ``cont`` the words with it, stored WITHOUT the
    prefix. A word's id is its line number. ``unk_id``, ``cls_id`` and ``sep_id`` are looked up by name
    (``cls_id`` / ``sep_id`` are None where the list has no such word). ``device=k`` uploads both tables."""

    def __init__(self, words: Sequence, prefix: bytes = b"##", device: int | None = None, unk: bytes = b"[UNK]",
                 cls: bytes = b"[CLS]", sep: bytes = b"[SEP]") -> None:
        words = [I._as_bytes(w) for w in words]
        prefix = I._as_bytes(prefix)
        if not prefix:
            raise ValueError("the continuation prefix must not be empty")
        is_cont = [w.startswith(prefix) and len(w) > len(prefix) for w in words]
        table = {w: i for i, w in enumerate(words)}
        if unk not in table:
            raise ValueError(f"the vocabulary has no {unk!r}")
        self.prefix, self.device = prefix, device
        self.unk_id, self.cls_id, self.sep_id = table[unk], table.get(cls), table.get(sep)
        self.first = I.Vocabulary([w for w, c in zip(words, is_cont) if not c], [i for i, c in enumerate(is_cont) if not c], device)
        cont = [(w[len(prefix):], i) for i, (w, c) in enumerate(zip(words, is_cont)) if c]
        self.cont = I.Vocabulary([w for w, _ in cont], [i for _, i in cont], device) if cont else None
        self.n_words = len(words)

    def __len__(self) -> int:
        return self.n_words

    def close(self) -> None:
        self.first.close()
        if self.cont is not None:
            self.cont.close()


@dataclass(frozen=True, eq=False)
class WordPieceIds(RL.NamedSpec):
    """One id output: the WordPiece ids of ``key``'s ``bytes_list`` elements as int64. Words are maximal runs
    of bytes outside ``delimiters`` and ``isolate`` (ASCII bytes) inside one element; every byte of
    ``isolate`` is a word of its own; a byte in both is a delimiter. With ``lower`` a word's ``A``..``Z``
    become ``a``..``z`` first. A word longer than ``max_word_bytes`` is ``unk``; else it is cut from the left
    into the longest pieces of ``vocab`` (the first piece from ``vocab.first``, the others from
    ``vocab.cont``), and is ``unk`` as a whole if some position has no piece. ``max_pieces``: a row gives
    at most that many ids (``special``: ``cls`` and ``sep`` included, so at least 2). ``special``: every
    row that is not skipped is ``cls``, its pieces, ``sep``. ``max_elems``: of a row's first that many
    elements. ``name``: the output's name in the result (default: the key)."""

    key: str
    vocab: WordPieceVocab
    lower: bool = True
    isolate: bytes = ASCII_PUNCTUATION
    max_pieces: int | None = None
    special: bool = False
    max_word_bytes: int = DEFAULT_WORD_BYTES
    max_elems: int | None = None
    delimiters: bytes = WHITESPACE
    name: str | None = None

    dtype = "uint8"  # (the slot kind, as ``Ragged.dtype`` selects it)

    def __post_init__(self) -> None:
        what = f"WordPieceIds({self.key!r})"
        if not isinstance(self.key, str):
            raise TypeError(f"WordPieceIds key must be a str, not {type(self.key).__name__}")
        if not isinstance(self.vocab, WordPieceVocab):
            raise TypeError(f"{what}: vocab must be a WordPieceVocab, not {type(self.vocab).__name__}")
        for field, empty_ok in (("delimiters", False), ("isolate", True)):
            v = getattr(self, field)
            if not isinstance(v, (bytes, bytearray)) or not (v or empty_ok):
                raise TypeError(f"{what}: {field} must be a{'' if empty_ok else ' non-empty'} bytes object")
            if v and max(v) >= 0x80:
                raise ValueError(f"{what}: {field} must hold ASCII bytes (< 0x80), not 0x{max(v):02x}")
        for field, least in (("max_pieces", 2 if self.special else 1), ("max_elems", 1)):
            v = getattr(self, field)
            if v is not None and (not isinstance(v, (int, np.integer)) or not least <= int(v) < 1 << 32):
                raise ValueError(f"{what}: {field} must be None or in {least}..2^32 - 1, not {v!r}")
        if not isinstance(self.max_word_bytes, (int, np.integer)) or not 1 <= int(self.max_word_bytes) <= N.WP_MAX_WORD_BYTES:
            raise ValueError(f"{what}: max_word_bytes must be in 1..{N.WP_MAX_WORD_BYTES}, not {self.max_word_bytes!r}")
        if self.special and (self.vocab.cls_id is None or self.vocab.sep_id is None):
            raise ValueError(f"{what}: special=True needs [CLS] and [SEP] in the vocabulary")

    @property
    def flags(self) -> int:
        return (N.WP_LOWER_ASCII if self.lower else 0) | (N.WP_SPECIAL if self.special else 0)

    @property
    def pieces_limit(self) -> int:
        """``tfrg_wp_spec.max_pieces`` (0: every piece)."""
        return int(self.max_pieces) if self.max_pieces is not None else 0

    @staticmethod
    def _words(bits: int) -> tuple[int, int]:
        return bits & ((1 << 64) - 1), bits >> 64

    @property
    def delim_words(self) -> tuple[int, int]:
        return self._words(sum(1 << b for b in set(self.delimiters)))

    @property
    def isolate_words(self) -> tuple[int, int]:
        return self._words(sum(1 << b for b in set(self.isolate)))

    def split(self, elem: bytes) -> list[bytes]:
        """The words of one element, lower-cased if asked."""
        dl = set(self.delimiters)
        iso = set(self.isolate) - dl
        words, cur = [], bytearray()
        for b in elem:
            if b in dl or b in iso:
                if cur:
                    words.append(bytes(cur))
                    cur = bytearray()
                if b in iso:
                    words.append(bytes([b]))
            else:
                cur.append(b)
        if cur:
            words.append(bytes(cur))
        return [w.lower() if self.lower else w for w in words]

    def pieces(self, word: bytes) -> tuple[list[int], bool]:
        """The ids of one (lowered) word's pieces, and whether it became ``unk``."""
        v = self.vocab
        if len(word) > self.max_word_bytes:
            return [v.unk_id], True
        out, pos = [], 0
        while pos < len(word):
            table = v.first if pos == 0 else v.cont
            end = len(word)
            while end > pos and (table is None or word[pos:end] not in table._dict):
                end -= 1
            if end == pos:
                return [v.unk_id], True
            out.append(table._dict[word[pos:end]])
            pos = end
        return out, False


def check_specs(specs: Sequence[WordPieceIds]) -> list[WordPieceIds]:
    return RL.check_named_specs(specs, WordPieceIds, N.WP_MAX_SPECS)


class WordPieceBatch(I.IdsBatch):
    """``IdsBatch`` whose totals count pieces: name -> ``(ids, row_offsets)``, with ``capacity``, ``totals``
    (T), ``stats`` (``WP_STAT_NAMES``) and ``overflowed``."""


# ---------------------------------------------------------------------- host path (numpy)
def wordpiece(specs: Sequence[WordPieceIds], *, n: int, slot_key: Sequence[str | None], slot_kind: Sequence[int],
              row_splits: np.ndarray, slot_base: np.ndarray, bytes_off: np.ndarray | None = None,
              bytes_len: np.ndarray | None = None, buf: np.ndarray | None = None, bytes_data: np.ndarray | None = None,
              bytes_offsets: np.ndarray | None = None, rows=None) -> WordPieceBatch:
    """The WordPiece outputs of ``specs`` from plain result columns (as ``tokens.tokenize`` takes them), word
    by word in Python. A key without a slot gives rows without a word. ``rows``: output row k is record
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
        limit = None if sp.max_pieces is None else sp.max_pieces - 2 * sp.special
        for k, _, elems in cols.rows(sp.key, sp.max_elems, picked):
            row: list[int] = []
            words = [w for elem in elems for w in sp.split(elem.tobytes())]
            st[2] += not words
            for w in words:
                got, unk = sp.pieces(w)
                st[1] += unk and (limit is None or len(row) < limit)  # (counted over the taken pieces)
                row += got
            if limit is not None and len(row) > limit:
                st[0] += 1
                row = row[:limit]
            if sp.special:
                row = [sp.vocab.cls_id, *row, sp.vocab.sep_id]
            ids += row
            row_offsets[k + 1] = row_offsets[k] + len(row)
        k = sp.out_name
        outputs[k] = (np.asarray(ids, np.int64).reshape(-1), row_offsets)
        totals[k] = len(ids)
        stats[k] = st
    return WordPieceBatch(outputs, dict(totals), totals, stats)


def batch_wordpiece_ids(res, specs: Sequence[WordPieceIds], rows=None) -> WordPieceBatch:
    """``BatchResult.wordpiece_ids``: ``wordpiece`` over a fetched result's columns."""
    return wordpiece(specs, n=len(res), slot_key=res.slot_key, slot_kind=res.slot_kind, row_splits=res.row_splits,
                     slot_base=res.slot_base, bytes_off=res.bytes_off, bytes_len=res.bytes_len, buf=res.buf,
                     bytes_data=res.bytes_data, bytes_offsets=res.bytes_offsets, rows=rows)


# ---------------------------------------------------------------------- device path
def launch_wordpiece(dec, items: Sequence[tuple], rows: tuple | None, m: int, row0: int, totals_ptr: int | None,
                     stats_ptr: int | None, consumer: int | None) -> None:
    """One ``tfrg_result_wordpiece_ids`` call: items are (slot, the spec, tok_cap, ids pointer or None,
    row_offsets pointer); ``rows``: (device pointer, TFRG_ROWS_* id) or None."""
    arr = (N.TfrgWpSpec * len(items))()
    for a, (slot, sp, tok_cap, ids, row_offsets) in zip(arr, items):
        v = sp.vocab
        a.slot, a.max_elems, a.max_pieces, a.flags = slot, sp.elems_limit, sp.pieces_limit, sp.flags
        a.delims[0], a.delims[1] = sp.delim_words
        a.isolate[0], a.isolate[1] = sp.isolate_words
        a.vocab = v.first._handle().value
        a.vocab_cont = v.cont._handle().value if v.cont is not None else None
        a.unk_id, a.cls_id, a.sep_id = v.unk_id, v.cls_id or 0, v.sep_id or 0
        a.max_word_bytes, a.tok_cap, a.ids, a.row_offsets = int(sp.max_word_bytes), tok_cap, ids, row_offsets
    ptr, rdt = rows if rows is not None else (None, 0)
    N.check(dec._lib.tfrg_result_wordpiece_ids(dec._ctx, arr, len(items), D.vp(ptr), rdt, m, row0, D.vp(totals_ptr),
                                               D.vp(stats_ptr), D.vp(consumer)), "tfrg_result_wordpiece_ids")


def decoder_wordpiece_ids(dec, specs: Sequence[WordPieceIds], *, rows=None, capacity=None, out: Mapping | None = None,
                          stream: int | None = None) -> WordPieceBatch:
    """``HipDecoder.wordpiece_ids``: the WordPiece outputs of the decoder's last decode, as torch tensors on
    its device: name -> ``(ids, row_offsets)``. ``rows``, ``capacity``, ``out`` and ``stream`` are
    ``decoder_token_ids``'s, counted in pieces: with every capacity known the call enqueues its work and
    returns without a host synchronisation; with ``capacity=None`` it runs twice (a sizing call without
    ids, one device-to-host copy of T, exact allocations, then the ids). A spec's vocabulary must have
    been made with ``device=`` this decoder's. A spec whose key has no slot gives rows without a piece,
    ``special`` or not."""
    import torch  # noqa: PLC0415

    specs = check_specs(specs)
    for sp in specs:
        if sp.vocab.device != dec.device:
            raise ValueError(f"WordPieceIds({sp.key!r}): its vocabulary was made with device={sp.vocab.device}, "
                             f"the decoder is on device {dec.device}")
    kind = RL.OutputKind(
        parts=lambda sp: (RL.Part("ids", torch.int64, lambda cap: cap, "1-D int64 tensor"),),
        offsets="row_offsets", capacity=I._capacity, cap_of=lambda v: int(v.numel()), no_cap=0,
        item=lambda sp, slot, ts, r: (slot, sp, RL.numel(ts[0]), RL.ptr(ts[0]), r.data_ptr()),
        launch=launch_wordpiece, width=1, empty_stat=2, batch=WordPieceBatch)
    return RL.run(dec, specs, kind, rows=rows, capacity=capacity, out=out, stream=stream)
