"""WordPiece ids on the device (tfrg_result_wordpiece_ids: k_wp_count / k_wp_scan / k_wp_write): every case
is a raw call of the C entry point whose ids, row offsets, totals and counters must equal tests/_wp_ref.py
exactly -- the batch's own bytes, bytes.split(), a dict per table and slicing. Every case runs with the
split knob at 8 (every row above 8 bytes by a wave), 0 (the default) and 65536 (every row by a lane). Every
output lies inside a larger buffer prefilled with 0xA5: the guards and everything past the stored prefix
keep the poison. The batch and the vocabulary are tests/_wp_ref.py's, the tile is 64."""

import ctypes as C

import numpy as np
import pytest

from tests import _wp_ref as WR
from tests.test_elem_ids_gpu import BAD32, BAD64, TILE, Outs, payload_input, slot_of, with_bad
from tests.test_elem_ids_host import RawVocab
from tests.test_ragged_gpu import I64_MAX, I64_MIN, dev, new_decoder, to_dev
from tests.test_wordpiece_host import spec_of
from tfr_reader import _native as N
from tfr_reader import wordpiece as W

pytestmark = pytest.mark.gpu

SPLITS = (8, 0, 65536)
N_REC, LONG_REC = WR.N_REC, WR.LONG_REC


def call_c(dec, rules, voc, outs, rows_ptr, rdt, m, row0, totals, stats, **over) -> int:
    """One raw call: ``voc`` is (the vocabulary of first pieces, the continuation vocabulary)."""
    arr = (N.TfrgWpSpec * len(rules))()
    for a, rule, o in zip(arr, rules, outs):
        a.slot, a.max_elems, a.max_pieces = slot_of(dec, rule.key), rule.max_elems or 0, rule.max_pieces or 0
        a.flags = (N.WP_LOWER_ASCII if rule.lower else 0) | (N.WP_SPECIAL if rule.special else 0)
        for field, chars in ((a.delims, b"" if rule.delims == WR.WHITESPACE else rule.delims), (a.isolate, rule.isolate)):
            bits = sum(1 << b for b in set(chars))  # (no delimiter bit: the default set)
            field[0], field[1] = bits & ((1 << 64) - 1), bits >> 64
        a.vocab, a.vocab_cont = voc[0].ptr.value, voc[1].ptr.value if rule.cont else None
        a.unk_id, a.cls_id, a.sep_id = WR.UNK, WR.CLS, WR.SEP
        a.max_word_bytes = 0 if rule.max_word_bytes == 100 else rule.max_word_bytes
        a.tok_cap = o.cap or 0
        a.ids = o.ids.data_ptr() if o.ids is not None and o.cap else None
        a.row_offsets = o.ro.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
    return dec._lib.tfrg_result_wordpiece_ids(dec._ctx, arr, len(rules), C.c_void_p(rows_ptr) if rows_ptr else None, rdt, m, row0,
                                              C.c_void_p(totals.data_ptr()) if totals is not None else None,
                                              C.c_void_p(stats.data_ptr()) if stats is not None else None, None)


def run_c(dec, items, rules, voc, rows=None, rdt=N.ROWS_I64, row0: int = 0, caps=None, with_stats: bool = True):
    """The call over poisoned outputs (capacity: T + 3, or ``caps[i]`` as a function of T; None: a NULL
    ids) in every split mode, checked against the reference, which is computed once."""
    import torch

    m = len(items) if rows is None else len(rows)
    wants = [WR.expect(items, rule, rows, row0) for rule in rules]
    caps = [w.total + 3 for w in wants] if caps is None else [c(w.total) if callable(c) else c for c, w in zip(caps, wants)]
    d_rows = None if rows is None else to_dev(rows, np.int64 if rdt == N.ROWS_I64 else np.int32)
    for split in SPLITS:
        dec.set_token_split(split)
        outs = [Outs(m, c) for c in caps]
        totals = torch.full((len(rules),), -1, dtype=torch.int64, device=dev())
        stats = torch.full((len(rules), 4), 77, dtype=torch.int32, device=dev()) if with_stats else None
        torch.cuda.synchronize()  # (the poison is in place before the library's own stream writes)
        rc = call_c(dec, rules, voc, outs, d_rows.data_ptr() if d_rows is not None else None, rdt, m, row0, totals, stats)
        assert rc == 0, dec._lib.tfrg_last_error()
        torch.cuda.synchronize()
        for o, w in zip(outs, wants):
            o.check(w)
        assert totals.cpu().tolist() == [w.total for w in wants], split
        if with_stats:
            assert stats.cpu().numpy().view(np.uint32).tolist() == [w.stats for w in wants], split
    return wants


def vocabs():
    voc = (RawVocab(list(WR.FIRST), list(WR.FIRST.values()), device=0), RawVocab(list(WR.CONT), list(WR.CONT.values()), device=0))
    assert voc[0].rc == 0 and voc[1].rc == 0, N.lib().tfrg_last_error()
    return voc


@pytest.fixture(scope="module")
def main():
    d = new_decoder()
    payloads, items = WR.text_batch()
    res = d.decode(*payload_input(payloads), payload_only=True)
    assert len(res) == N_REC and int(res.status.max()) == 0
    d.set_ragged_tile(TILE)
    voc = vocabs()
    yield d, res, items, voc
    for v in voc:
        v.close()
    d.close()


@pytest.mark.parametrize("i", range(len(WR.RULES)))
def test_rules(main, i):
    """Every rule of the reference beside a second spec in the same call, over every record: every word
    and sentence the cases are about, the long record included."""
    d, _, items, voc = main
    run_c(d, items, [WR.RULES[i], WR.Rule(lower=False, max_pieces=4)], voc)


ROW0 = 1 << 40
ROW_LISTS = {
    "a permutation": (np.random.default_rng(1).permutation(N_REC), N.ROWS_I64, 0),
    "repeats, int32": ([LONG_REC, 3, LONG_REC, 3, 3, 7, LONG_REC, *range(60, 125)], N.ROWS_I32, 0),
    "out of range, int64": (with_bad(BAD64, 327), N.ROWS_I64, 0),
    "out of range, int32": (with_bad(BAD32, 130), N.ROWS_I32, 0),
    "only skipped rows": ([I64_MAX, -1, I64_MIN, N_REC], N.ROWS_I64, 0),
    "row0": ([ROW0 + (7 * k) % N_REC for k in range(150)] + [ROW0 - 1, ROW0 + N_REC, 5, I64_MIN], N.ROWS_I64, ROW0),
}


@pytest.mark.parametrize("name", list(ROW_LISTS))
def test_row_lists(main, name):
    d, _, items, voc = main
    rows, rdt, row0 = ROW_LISTS[name]
    run_c(d, items, [WR.Rule(special=True, max_pieces=6), WR.Rule()], voc, rows, rdt, row0)


@pytest.mark.parametrize("cap", ["T", "T // 2", "0", "NULL"])
def test_capacities_with_and_without_counters(main, cap):
    d, _, items, voc = main
    caps = {"T": lambda t: t, "T // 2": lambda t: t // 2, "0": 0, "NULL": None}
    rows = np.random.default_rng(3).integers(0, N_REC, 150).tolist() + [LONG_REC]
    for with_stats in (True, False):
        run_c(d, items, [WR.Rule(special=True), WR.Rule()], voc, rows, caps=[caps[cap], lambda t: t + 3], with_stats=with_stats)


def test_refusals_leave_the_poison_and_empty_cases(main):
    import torch

    d, res, items, voc = main
    lib = N.lib()
    host_only = RawVocab([b"q"])
    rule = WR.Rule()
    tot = torch.full((1,), -1, dtype=torch.int64, device=dev())
    st = torch.full((1, 4), 77, dtype=torch.int32, device=dev())
    outs = Outs(3, 16)
    s_n = next(s for s in range(len(res.slot_key)) if res.slot_key[s] == "n")

    def call(k=1, rdt=N.ROWS_I64, m=3, **kw):
        torch.cuda.synchronize()
        if k != 1:
            return lib.tfrg_result_wordpiece_ids(d._ctx, (N.TfrgWpSpec * 17)(), k, None, rdt, m, 0, None, None, None)
        return call_c(d, [rule], voc, [outs], None, rdt, m, 0, tot, st, **kw)

    try:
        ro_ptr, id_ptr = outs.ro.data_ptr(), outs.ids.data_ptr()
        for bad in (dict(k=0), dict(k=N.WP_MAX_SPECS + 1), dict(slot=len(res.slot_key)), dict(slot=s_n), dict(row_offsets=None),
                    dict(row_offsets=ro_ptr + 4), dict(ids=id_ptr + 4), dict(flags=4), dict(flags=1 << 31), dict(reserved=1),
                    dict(vocab=None), dict(vocab=host_only.ptr.value), dict(vocab_cont=host_only.ptr.value),
                    dict(max_word_bytes=1025), dict(flags=N.WP_SPECIAL, max_pieces=1), dict(m=1 << 31)):
            assert call(**bad) == -1, bad
            assert lib.tfrg_last_error().startswith(b"tfrg_result_wordpiece_ids: "), bad
            torch.cuda.synchronize()
            outs.untouched()
            assert tot.cpu().tolist() == [-1] and st.cpu().tolist() == [[77] * 4], bad
        # m == 0: row_offsets[0] = 0, totals 0, no kernel
        assert call(m=0) == 0
        torch.cuda.synchronize()
        assert outs.ro.cpu().tolist()[0] == 0 and bool((outs.id_buf == 0xA5).all()) and tot.cpu().tolist() == [0]
        assert st.cpu().tolist() == [[0] * 4]
    finally:
        host_only.close()


def test_materialized_column():
    d = new_decoder()
    payloads, items = WR.text_batch()
    voc = vocabs()
    try:
        res = d.decode(*payload_input(payloads), payload_only=True, materialize_bytes=True)
        assert res.bytes_data is not None
        d.set_ragged_tile(TILE)
        run_c(d, items, [WR.Rule(), WR.Rule(special=True, max_pieces=7, max_elems=2)], voc, with_bad(BAD64, 200))
    finally:
        for v in voc:
            v.close()
        d.close()


def test_python_device_path_against_the_reference(main):
    d, res, items, _ = main
    vocab = W.WordPieceVocab(WR.VOCAB, device=0)
    try:
        d.set_token_split(0)
        rs = [r for r in WR.RULES if r.cont][:9]
        specs = [spec_of(r, vocab, str(i)) for i, r in enumerate(rs)]
        rows = [0, N_REC, -1, 5, LONG_REC, 3, 3, *range(20, 90)]
        for r in (None, rows):
            got = d.wordpiece_ids(specs, rows=None if r is None else to_dev(r))  # no capacity: the sizing call, exact tensors
            for sp, rule in zip(specs, rs):
                k, want = sp.out_name, WR.expect(items, rule, r)
                ids, ro = got[k]
                assert ids.numel() == want.total == got.capacity[k] == got.totals[k] and not got.overflowed[k], rule
                assert np.array_equal(ids.cpu().numpy(), want.ids) and np.array_equal(ro.cpu().numpy(), want.row_offsets), rule
                assert got.stats[k].tolist() == want.stats, rule
        want = WR.expect(items, rs[0], rows)
        got = d.wordpiece_ids(specs[:1], rows=to_dev(rows), capacity=want.total - 5)
        assert got.overflowed["0"] and np.array_equal(got["0"][0].cpu().numpy(), want.ids[:-5])
        with pytest.raises(ValueError, match="device"):
            d.wordpiece_ids([W.WordPieceIds("t", W.WordPieceVocab(WR.VOCAB))])
    finally:
        vocab.close()
