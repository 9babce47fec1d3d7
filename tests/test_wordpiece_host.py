"""WordPiece ids on the host (no GPU): the batch has the inputs the cases are about, the numpy path
(``BatchResult.wordpiece_ids``) equals tests/_wp_ref.py on the batch tests/test_wordpiece_gpu.py runs on the
device, what ``WordPieceIds`` refuses, and the layout of tfrg_wp_spec against the header."""

import ctypes as C

import numpy as np
import pytest

from tests import _columns
from tests import _wp_ref as WR
from tests import test_elem_ids_host as EH
from tests.test_dense_rows_host import row_lists
from tfr_reader import _native as N
from tfr_reader import synth
from tfr_reader import wordpiece as W


def spec_of(rule: WR.Rule, vocab: W.WordPieceVocab, name: str) -> W.WordPieceIds:
    return W.WordPieceIds(rule.key, vocab, lower=rule.lower, isolate=rule.isolate, max_pieces=rule.max_pieces, special=rule.special,
                          max_word_bytes=rule.max_word_bytes, max_elems=rule.max_elems, delimiters=rule.delims, name=name)


def test_the_reference_on_known_words_and_the_batch():
    r = WR.Rule()
    by_word = {w: WR.pieces_of(w, r)[0] for w in (b"playing", b"abcdefghij", b"abcq", b"acat", b"ing", b"a" * 40, b"na\xc3\xafve")}
    v = WR.VOCAB.index
    assert by_word[b"playing"] == [v(b"play"), v(b"##ing")] and by_word[b"abcdefghij"] == [v(b"abcdefghi"), v(b"##j")]
    assert by_word[b"abcq"] == by_word[b"acat"] == by_word[b"ing"] == [WR.UNK] and by_word[b"a" * 40] == [v(b"a")] + [v(b"##a")] * 39
    assert by_word[b"na\xc3\xafve"] == [v(b"na"), v(b"##\xc3\xafve")]
    assert WR.words_of(b",Hello.a-b", r) == [b",", b"hello", b".", b"a", b"-", b"b"]
    assert WR.words_of(b"a-b,c", WR.RULES[4]) == [b"a", b"b", b"c"]  # (a byte in both sets is a delimiter)
    _, items = WR.text_batch()
    text = [e for it in items for e in it["t"]]
    words = {w for e in text for w in e.split()}
    assert words >= set(WR.SPECIAL_WORDS) - {b""} and set(text) >= set(WR.SENTENCES)
    whole = [WR.expect(items, rule) for rule in WR.RULES]
    assert all(w.stats[2] > 0 and (w.stats[1] > 0) == (i != 9) for i, w in enumerate(whole))  # (rule 9 takes no piece)
    assert whole[7].stats[0] > 0 and whole[8].stats[0] > 0
    assert whole[1].stats[1] > whole[0].stats[1] and whole[2].stats[1] > whole[0].stats[1] and whole[5].stats[1] > whole[0].stats[1]
    assert whole[10].total == whole[0].total + 2 * len(items)


def test_the_numpy_path_gives_the_references_ids():
    payloads, items = WR.text_batch()
    res = _columns.batch_from_oracle(*synth.framed(payloads))
    full, no_cont = W.WordPieceVocab(WR.VOCAB), W.WordPieceVocab([w for w in WR.VOCAB if not w.startswith(b"##")])
    assert (full.unk_id, full.cls_id, full.sep_id) == (WR.UNK, WR.CLS, WR.SEP) and no_cont.cont is None
    # (without the ## lines the ids of the first pieces change: that table is compared through its own reference below)
    pairs = [(r, spec_of(r, full, str(i))) for i, r in enumerate(WR.RULES) if r.cont]
    pairs.append((WR.Rule(key="zz"), W.WordPieceIds("zz", full, name="absent")))
    for rows in [None, *row_lists(len(items))[:2]]:
        got = res.wordpiece_ids([sp for _, sp in pairs], rows=rows)
        for rule, sp in pairs:
            want, k = WR.expect(items, rule, rows), sp.out_name
            if k == "absent":  # (a key without a slot: rows without a word, special or not)
                assert got.totals[k] == 0
                continue
            assert np.array_equal(got[k][0], want.ids) and np.array_equal(got[k][1], want.row_offsets), rule
            assert got.stats[k].tolist() == want.stats and got.totals[k] == want.total == got.capacity[k], rule
    sp = W.WordPieceIds("t", no_cont)
    assert sp.pieces(b"cats") == ([no_cont.unk_id], True) and sp.pieces(b"cat") == ([no_cont.first.id_of(b"cat")], False)


def test_specs_that_are_refused():
    v = W.WordPieceVocab(WR.VOCAB)
    for bad in (dict(isolate=b"\x80"), dict(delimiters=b" \xff"), dict(max_pieces=0), dict(max_pieces=1, special=True),
                dict(max_pieces=1 << 32), dict(max_elems=0), dict(max_word_bytes=0), dict(max_word_bytes=1025)):
        with pytest.raises(ValueError):
            W.WordPieceIds("t", v, **bad)
    for bad in (dict(delimiters=b""), dict(isolate=","), dict(vocab={b"a": 0})):
        with pytest.raises(TypeError):
            W.WordPieceIds("t", **{"vocab": v, **bad})
    with pytest.raises(ValueError):
        W.WordPieceVocab([b"a", b"##a"])  # (no [UNK])
    with pytest.raises(ValueError):
        W.WordPieceIds("t", W.WordPieceVocab([b"[UNK]", b"a"]), special=True)  # (no [CLS] / [SEP])
    sp = W.WordPieceIds("t", v, special=True, max_pieces=4)
    assert sp.flags == 3 and sp.delim_words == (0x100003E00, 0) and sp.split(b"Hi,a b") == [b"hi", b",", b"a", b"b"]
    with pytest.raises(ValueError):
        W.check_specs([W.WordPieceIds("t", v, name=str(i)) for i in range(N.WP_MAX_SPECS + 1)])


def test_wp_spec_matches_the_header(tmp_path, monkeypatch):
    monkeypatch.setattr(EH, "STRUCTS", {"tfrg_wp_spec": N.TfrgWpSpec})
    monkeypatch.setattr(EH, "CONSTANTS", {"TFRG_WP_MAX_SPECS": N.WP_MAX_SPECS, "TFRG_WP_LOWER_ASCII": N.WP_LOWER_ASCII,
                                          "TFRG_WP_SPECIAL": N.WP_SPECIAL, "TFRG_WP_MAX_WORD_BYTES": N.WP_MAX_WORD_BYTES})
    c = EH._c_layout(tmp_path)
    assert c[("tfrg_wp_spec", "__size__")] == C.sizeof(N.TfrgWpSpec) == 120
    for fname, _ in N.TfrgWpSpec._fields_:
        f = getattr(N.TfrgWpSpec, fname)
        assert c[("tfrg_wp_spec", fname)] == (f.offset, f.size), fname
    assert [c[("const", k)][0] for k in EH.CONSTANTS] == [16, 1, 2, 1024]
    spec = N.TfrgWpSpec(slot=0, row_offsets=16)
    assert N.lib().tfrg_result_wordpiece_ids(None, C.byref(spec), 1, None, N.ROWS_I64, 1, 0, None, None, None) == -1
    assert N.lib().tfrg_last_error().startswith(b"tfrg_result_wordpiece_ids: ")
