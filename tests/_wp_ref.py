"""Reference of the WordPiece ids (``WordPieceIds``: tfrg_result_wordpiece_ids, ``wordpiece.wordpiece``), its
vocabulary and its batch, for tests/test_wordpiece_host.py and tests/test_wordpiece_gpu.py. No GPU.

The expected ids are built from the batch's own ``bytes`` objects with ``bytes.translate`` / ``replace`` /
``split`` / ``lower``, one dict per table and slicing. Nothing comes from a decode's columns or from
tfr_reader/wordpiece.py."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import _bytes_ref as B
from tests import _ids_ref as IR
from tests.golden.gen_golden import entry, i64

WHITESPACE = b" \t\n\r\x0b\x0c"
PUNCT = bytes(b for b in range(33, 127) if not chr(b).isalnum())
ALPHA = b"abcdefghijklmnopq"
# vocab.txt: a word's id is its line. No "aa", no "i", no piece with a "q" but the whole words of ALPHA.
VOCAB = [b"[PAD]", b"[UNK]", b"[CLS]", b"[SEP]", b"a", b"##a", b"abc", *(ALPHA[:n] for n in (7, 8, 9, 15, 16, 17)), b"##j", b"##z",
         b"##zz", b"cat", b"##ing", b"##s", b"play", b"hello", b"world", b"the", b"on", b"mat", b"sat", b"caf\xc3\xa9", b"na",
         b"##\xc3\xafve", b"\xe6\x97\xa5", b"##\xe6\x9c\xac", b",", b".", b"!", b"-", b"un", b"##believ", b"##able", b"x", b"b"]
UNK, CLS, SEP = 1, 2, 3
FIRST = {w: i for i, w in enumerate(VOCAB) if not (w.startswith(b"##") and len(w) > 2)}
CONT = {w[2:]: i for i, w in enumerate(VOCAB) if w.startswith(b"##") and len(w) > 2}
G = 8  # the lanes that probe one piece's ends together: candidate counts G - 1, G, G + 1 and 2 G + 1 below

# The words the cases are about (all lower-case unless the case is about case), each in some sentence
SPECIAL_WORDS = [
    *(ALPHA[:n] for n in (1, 7, 8, 9, 15, 16, 17)),  # whole words around the 8-byte hash groups
    *(b"a" + b"z" * (n - 1) for n in (G - 1, G, G + 1, 2 * G + 1)),  # matched by the LAST candidate end only, then ##zz ...
    *(b"q" * n for n in (G - 1, G, G + 1, 2 * G + 1)),  # no candidate matches
    ALPHA[:10],  # longest first piece abcdefghi (then ##j), shortest a
    b"abcq", b"a",  # pieces found (abc), then no continuation: one unk; the next word's index follows
    b"acat", b"ing", b"cats", b"playing", b"unbelievable",  # "cat" only begins a word, "ing" only continues one
    b"a" + b"z" * 99, b"a" + b"z" * 100,  # max_word_bytes and one more
    b"a" * 40,  # 40 one-byte pieces: past the stage
    b"Hello", b"WORLD", b"hello",  # match only when lowered
    b"caf\xc3\xa9", b"na\xc3\xafve", b"\xe6\x97\xa5\xe6\x9c\xac", b"\xe6\x97\xa5\xe6\x97\xa5",  # UTF-8; the last: no ##日
]
SENTENCES = [
    b",,,,,,,,", b",,,,,,,,,", b"a,,,,,,,,.b", b",hello.", b"!", b"hello,world!", b"the cat-sat on the mat.", b"a-b--c", b"x?x",
    b"", b"   ", b" \t\n", b"the  cat", b"playing cats, unbelievable!", b"abcq a abcq. a",
]
N_REC, LONG_REC = 200, 57


def text_batch() -> tuple[list[bytes], list[dict]]:
    """200 records of 0 to 3 short sentences under b"t" (every SPECIAL_WORDS word and every SENTENCES
    sentence among them), and record LONG_REC: one element of about 3 KiB in which a word lies across
    byte 512."""
    pool = [*SENTENCES, *(b" ".join(SPECIAL_WORDS[(i + j) % len(SPECIAL_WORDS)] for j in range(1 + i % 4)) + b"."[: i % 2]
                          for i in range(len(SPECIAL_WORDS)))]
    counts = [(1, 2, 0, 3)[r % 4] for r in range(N_REC)]
    payloads, items, at = [], [], 0
    for r, c in enumerate(counts):
        elems = [pool[(at + j) % len(pool)] for j in range(c)]
        at += c
        if r == LONG_REC:
            body = b" ".join(SPECIAL_WORDS[j % len(SPECIAL_WORDS)] for j in range(400) if len(SPECIAL_WORDS[j % len(SPECIAL_WORDS)]) < 20)
            pad = next(p for p in range(64) if b" " not in (b" " * p + body)[508:516])
            elems = [(b" " * pad + body)[:3100]]
        p, it = B.record({b"t": elems}, entry(b"n", i64(r)))
        payloads.append(p)
        items.append(it)
    assert at >= len(pool) and len(items[LONG_REC]["t"][0]) > 3000
    return payloads, items


@dataclass
class Rule:
    """One spec. ``delims`` must hold the whitespace bytes; ``cont`` False: no continuation vocabulary."""

    key: str = "t"
    lower: bool = True
    isolate: bytes = PUNCT
    delims: bytes = WHITESPACE
    max_pieces: int | None = None
    special: bool = False
    max_word_bytes: int = 100
    max_elems: int | None = None
    cont: bool = True


RULES = [
    Rule(), Rule(lower=False), Rule(cont=False), Rule(isolate=b""), Rule(isolate=PUNCT, delims=WHITESPACE + b"-,"),
    Rule(max_word_bytes=9), Rule(max_elems=1), Rule(max_pieces=3), Rule(max_pieces=5, special=True), Rule(max_pieces=2, special=True),
    Rule(special=True), Rule(max_pieces=1),
]


def words_of(elem: bytes, rule: Rule) -> list[bytes]:
    assert set(WHITESPACE) <= set(rule.delims)  # (split() below splits on these whatever the rule says)
    s = elem.translate(bytes.maketrans(rule.delims, b" " * len(rule.delims)))
    for b in set(rule.isolate) - set(rule.delims):
        s = s.replace(bytes([b]), b" %c " % b)
    return [w.lower() if rule.lower else w for w in s.split()]


def pieces_of(w: bytes, rule: Rule) -> tuple[list[int], bool]:
    if len(w) > rule.max_word_bytes:
        return [UNK], True
    out, pos = [], 0
    while pos < len(w):
        tab = FIRST if pos == 0 else CONT if rule.cont else {}
        end = next((e for e in range(len(w), pos, -1) if w[pos:e] in tab), None)
        if end is None:
            return [UNK], True
        out.append(tab[w[pos:end]])
        pos = end
    return out, False


def expect(items: list[dict], rule: Rule, rows=None, row0: int = 0) -> IR.Want:
    """What ``rule`` must give for the row list ``rows`` (None: every record): ids, row offsets, the four
    counters; ``Want.elems[t]`` is the word piece t came from."""
    n = len(items)
    rows = list(range(row0, row0 + n)) if rows is None else [int(v) for v in np.asarray(rows, object).reshape(-1)]
    limit = None if rule.max_pieces is None else rule.max_pieces - 2 * rule.special
    ids: list[int] = []
    src: list[bytes] = []
    ro = [0]
    st = [0, 0, 0, 0]
    for v in rows:
        g = v - row0
        if not 0 <= g < n:
            st[3] += 1
            ro.append(ro[-1])
            continue
        its = items[g].get(rule.key, [])
        words = [w for e in (its if rule.max_elems is None else its[: rule.max_elems]) for w in words_of(e, rule)]
        st[2] += not words
        row: list[tuple[int, bytes]] = []
        for w in words:
            got, unk = pieces_of(w, rule)
            st[1] += unk and (limit is None or len(row) < limit)
            row += [(i, w) for i in got]
        if limit is not None and len(row) > limit:
            st[0] += 1
            row = row[:limit]
        if rule.special:
            row = [(CLS, b"[CLS]"), *row, (SEP, b"[SEP]")]
        ids += [i for i, _ in row]
        src += [w for _, w in row]
        ro.append(ro[-1] + len(row))
    return IR.Want(ids, ro, st, src)
