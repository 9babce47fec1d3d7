"""Token ids on the host (no GPU): what ``TokenIds`` refuses, the layout of tfrg_tok_spec against the
header, and the numpy path (``BatchResult.token_ids`` / ``tokenize``) against tests/_tok_ref.py on the
batch tests/test_token_ids_gpu.py runs on the device. Every comparison is exact."""

import ctypes as C

import numpy as np
import pytest

from tests import _bytes_ref as B
from tests import _columns
from tests import _tok_ref as TR
from tests import test_elem_ids_host as EH
from tests.golden.gen_golden import entry, i64
from tests.test_dense_rows_host import row_lists
from tfr_reader import _native as N
from tfr_reader import ids as I
from tfr_reader import synth
from tfr_reader import tokens as T

LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 511, 512, 513, 1029, 4099]  # around the 8-byte word and the 512-byte round
PER = [0, 1, 2, 5]
N_REC = 200
LONG_REC, LONG_COUNT = 57, 1100
WORDS = [b"The", b"cat", b"SAT", b"on", b"a", b"Mat", b"zebra-crossing", b"I", b"x" * 23, b"caf\xc3\xa9", b"Hello,", b"world."]
PUNCT = TR.WHITESPACE + b",.-"


def contents(L: int, seed: int) -> list[bytes]:
    """One element of L bytes per kind of content."""
    rng = np.random.default_rng(seed)
    words = b" ".join(WORDS[i] for i in rng.integers(0, len(WORDS), L // 2 + 2))
    noisy = rng.integers(0, 256, L, dtype=np.uint8)
    noisy[rng.integers(0, max(L, 1), L // 3)] = 0  # zero bytes and bytes >= 0x80 among random ones
    return [
        (b" \t\n\r\x0b\x0c" * (L // 6 + 1))[:L],  # all delimiters
        (b"aBcDeFgHiJ" * (L // 10 + 1))[:L],  # no delimiter: one token across words and rounds
        (b"a b c d " * (L // 8 + 1))[:L],  # four ends in every word
        (b" " * (L // 3) + b"Q" * L)[:L],  # a token that ends exactly at the element's end
        (b" \n " + words)[: max(L - 3, 0)] + b" \t "[: min(L, 3)],  # leading and trailing runs
        noisy.tobytes(),
        words[:L],  # mixed case, punctuation, UTF-8
    ]


def text_batch() -> tuple[list[bytes], list[dict]]:
    """200 records of 0, 1, 2 or 5 elements under b"t" (one of 1100 two-byte elements), every length of
    LENGTHS with every kind of content; a short sentence under b"s"."""
    pool = [e for i, L in enumerate(LENGTHS) for e in contents(L, i)]
    counts = [PER[r % len(PER)] for r in range(N_REC)]
    counts[LONG_REC] = LONG_COUNT
    tiny = [(b"ab", b"c ", b" d", b"  ", b"E,")[j % 5] for j in range(LONG_COUNT)]
    payloads, items, at = [], [], 0
    for r, c in enumerate(counts):
        elems = tiny if r == LONG_REC else [pool[(at + j) % len(pool)] for j in range(c)]
        at += 0 if r == LONG_REC else c
        sentence = b" ".join(WORDS[(r + j) % len(WORDS)] for j in range(r % 9))
        p, it = B.record({b"s": [sentence], b"t": elems}, entry(b"n", i64(r)))
        payloads.append(p)
        items.append(it)
    assert at >= len(pool)  # (every element of the pool is in the batch)
    return payloads, items


def vocab_words(items) -> list[bytes]:
    """Lower-case words: every other distinct lowered whitespace token of at most 24 bytes."""
    toks = [t.lower() for it in items for k in ("t", "s") for e in it.get(k, []) for t in e.split() if len(t) <= 24]
    return list(dict.fromkeys(toks))[::2]


def rules(words: list[bytes]) -> list[TR.Rule]:
    """The rules of the cases, over one table of lower-case words (None where a rule has no vocabulary)."""
    t = {w: i for i, w in enumerate(words)}
    return [
        TR.Rule("t", None, 1024, 0), TR.Rule("t", None, 1000, 5, lower=True),  # buckets only
        TR.Rule("t", t, default=-7, lower=True), TR.Rule("t", t, default=-7),  # a vocabulary only
        TR.Rule("t", t, 7, len(words), lower=True),  # both
        TR.Rule("t", t, 7, 0, lower=True, delims=PUNCT), TR.Rule("s", t, default=-1, lower=True, delims=PUNCT),
        TR.Rule("t", t, 7, 0, lower=True, max_tokens=1), TR.Rule("t", None, 7, 0, max_tokens=3),
        TR.Rule("t", t, 7, 0, lower=True, max_elems=2), TR.Rule("t", t, 3, 0, max_elems=2, max_tokens=3),
    ]


def spec_of(rule: TR.Rule, vocab, name: str) -> T.TokenIds:
    return T.TokenIds(rule.key, vocab if rule.table is not None else None, num_oov_buckets=rule.buckets, lower=rule.lower,
                      delimiters=rule.delims, max_tokens=rule.max_tokens, max_elems=rule.max_elems, oov_base=rule.base,
                      default_id=rule.default, name=name)


def test_tokenize_gives_the_references_ids():
    payloads, items = text_batch()
    res = _columns.batch_from_oracle(*synth.framed(payloads))
    words = vocab_words(items)
    vocab = I.Vocabulary(words)
    pairs = [(r, spec_of(r, vocab, str(i))) for i, r in enumerate(rules(words))]
    pairs.append((TR.Rule("zz", {}, default=-1), T.TokenIds("zz", vocab, name="absent")))
    for rows in [None, *row_lists(len(items))[:2]]:
        got = res.token_ids([sp for _, sp in pairs], rows=rows)
        for rule, sp in pairs:
            want, k = TR.expect(items, rule, rows), sp.out_name
            assert np.array_equal(got[k][0], want.ids) and np.array_equal(got[k][1], want.row_offsets), rule
            assert got.stats[k].tolist() == want.stats and got.totals[k] == want.total == got.capacity[k], rule
            if rule.table and rows is None:
                assert 0 < want.matched < want.total, rule
    whole = [TR.expect(items, r) for r in rules(words)]
    assert whole[7].stats[0] > 0 and whole[8].stats[0] > 0 and whole[0].stats[2] > 0  # rows cut, rows without a token
    assert whole[2].matched > whole[3].matched > 0  # (lower-casing matches more of the lower-case words)
    assert whole[5].total > whole[4].total  # (punctuation splits further)


def test_specs_that_are_refused():
    v = I.Vocabulary([b"q"])
    with pytest.raises(ValueError):
        T.TokenIds("t")  # (no vocabulary and no buckets)
    for bad in (dict(delimiters=b" \x80"), dict(delimiters=b"\xff"), dict(num_oov_buckets=-1), dict(max_tokens=0),
                dict(max_tokens=1 << 32), dict(max_elems=0), dict(default_id=1 << 63), dict(oov_base=-(1 << 63) - 1)):
        with pytest.raises(ValueError):
            T.TokenIds("t", v, **bad)
    for bad in (dict(delimiters=b""), dict(delimiters=" "), dict(vocab={b"q": 0})):
        with pytest.raises(TypeError):
            T.TokenIds("t", **{"vocab": v, **bad})
    with pytest.raises(TypeError):
        T.TokenIds(b"t", v)
    sp = T.TokenIds("t", v, num_oov_buckets=3, lower=True)
    assert sp.base == 1 and sp.delim_words == (0x100003E00, 0) and sp.split(b" A b\tC ") == [b"a", b"b", b"c"]
    assert T.TokenIds("t", v, delimiters=b"a~").delim_words == (0, (1 << (ord("a") - 64)) | (1 << (ord("~") - 64)))
    with pytest.raises(ValueError):
        T.check_specs([T.TokenIds("t", v, name=str(i)) for i in range(N.TOK_MAX_SPECS + 1)])


def test_tok_spec_matches_the_header(tmp_path, monkeypatch):
    monkeypatch.setattr(EH, "STRUCTS", {"tfrg_tok_spec": N.TfrgTokSpec})
    monkeypatch.setattr(EH, "CONSTANTS", {"TFRG_TOK_MAX_SPECS": N.TOK_MAX_SPECS, "TFRG_TOK_LOWER_ASCII": N.TOK_LOWER_ASCII})
    c = EH._c_layout(tmp_path)
    assert c[("tfrg_tok_spec", "__size__")] == C.sizeof(N.TfrgTokSpec) == 88
    for fname, _ in N.TfrgTokSpec._fields_:
        f = getattr(N.TfrgTokSpec, fname)
        assert c[("tfrg_tok_spec", fname)] == (f.offset, f.size), fname
    assert c[("const", "TFRG_TOK_MAX_SPECS")][0] == 16 and c[("const", "TFRG_TOK_LOWER_ASCII")][0] == 1
    lib = N.lib()
    spec = N.TfrgTokSpec(slot=0, num_oov_buckets=4, row_offsets=16)
    assert lib.tfrg_result_token_ids(None, C.byref(spec), 1, None, N.ROWS_I64, 1, 0, None, None, None) == -1
    assert lib.tfrg_last_error().startswith(b"tfrg_result_token_ids: ")
