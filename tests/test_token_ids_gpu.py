"""Token ids on the device (tfrg_result_token_ids: k_tok_count / k_tok_scan / k_tok_write): every case is
a raw call of the C entry point whose ids and row offsets must equal tests/_tok_ref.py -- the generator's
own items, bytes.split(), a Python dict and the Python restatement of tfrg_hash64. Every case runs with
the split knob at 8 (every row above 8 bytes by a wave), 0 (the default) and 65536 (every row by a lane).
Every output lies inside a larger buffer prefilled with 0xA5: the guards and everything past the stored
prefix keep the poison. The batch is tests/test_token_ids_host.py's, the tile is 64."""

import ctypes as C

import numpy as np
import pytest

from tests import _tok_ref as TR
from tests import test_implicit_off_gpu as IO
from tests import test_token_ids_host as TH
from tests.test_elem_ids_gpu import BAD32, BAD64, TILE, Outs, payload_input, slot_of, with_bad
from tests.test_elem_ids_host import RawVocab
from tests.test_ragged_gpu import I64_MAX, I64_MIN, dev, new_decoder, to_dev
from tfr_reader import _native as N
from tfr_reader import ids as I
from tfr_reader import synth
from tfr_reader import tokens as T

pytestmark = pytest.mark.gpu

SPLITS = (8, 0, 65536)
N_REC, LONG_REC = TH.N_REC, TH.LONG_REC


def call_c(dec, rules, voc, outs, rows_ptr, rdt, m, row0, totals, stats, **over) -> int:
    arr = (N.TfrgTokSpec * len(rules))()
    for a, rule, o in zip(arr, rules, outs):
        a.slot, a.max_elems, a.max_tokens = slot_of(dec, rule.key), rule.max_elems or 0, rule.max_tokens or 0
        a.flags = N.TOK_LOWER_ASCII if rule.lower else 0
        bits = 0 if rule.delims == TR.WHITESPACE else sum(1 << b for b in set(rule.delims))  # (0: the default set)
        a.delims[0], a.delims[1] = bits & ((1 << 64) - 1), bits >> 64
        a.vocab = voc.ptr.value if rule.table is not None else None
        a.num_oov_buckets, a.oov_base, a.default_id = rule.buckets, rule.base, rule.default
        a.tok_cap = o.cap or 0
        a.ids = o.ids.data_ptr() if o.ids is not None and o.cap else None
        a.row_offsets = o.ro.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
    return dec._lib.tfrg_result_token_ids(dec._ctx, arr, len(rules), C.c_void_p(rows_ptr) if rows_ptr else None, rdt, m, row0,
                                          C.c_void_p(totals.data_ptr()) if totals is not None else None,
                                          C.c_void_p(stats.data_ptr()) if stats is not None else None, None)


def run_c(dec, items, rules, voc, rows=None, rdt=N.ROWS_I64, row0: int = 0, caps=None, with_stats: bool = True, splits=SPLITS):
    """The call over poisoned outputs (capacity: T + 3, or ``caps[i]`` as a function of T; None: a NULL
    ids) in every split mode, checked against the reference, which is computed once."""
    import torch

    m = len(items) if rows is None else len(rows)
    wants = [TR.expect(items, rule, rows, row0) for rule in rules]
    caps = [w.total + 3 for w in wants] if caps is None else [c(w.total) if callable(c) else c for c, w in zip(caps, wants)]
    d_rows = None if rows is None else to_dev(rows, np.int64 if rdt == N.ROWS_I64 else np.int32)
    for split in splits:
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
    return wants, outs


@pytest.fixture(scope="module")
def main():
    d = new_decoder()
    payloads, items = TH.text_batch()
    res = d.decode(*payload_input(payloads), payload_only=True)
    assert len(res) == N_REC and int(res.status.max()) == 0
    d.set_ragged_tile(TILE)
    words = TH.vocab_words(items)
    v = RawVocab(words, device=0)
    assert v.rc == 0, N.lib().tfrg_last_error()
    yield d, res, items, words, v
    v.close()
    d.close()


ROW0 = 1 << 40
ROW_LISTS = {
    "every record": (None, N.ROWS_I64, 0),
    "a permutation": (np.random.default_rng(1).permutation(N_REC), N.ROWS_I64, 0),
    "repeats, int32": ([LONG_REC, 3, LONG_REC, 3, 3, 7, LONG_REC, *range(60, 125)], N.ROWS_I32, 0),
    "out of range, int64": (with_bad(BAD64, 327), N.ROWS_I64, 0),
    "out of range, int32": (with_bad(BAD32, 130), N.ROWS_I32, 0),
    "only skipped rows": ([I64_MAX, -1, I64_MIN, N_REC], N.ROWS_I64, 0),
    "row0": ([ROW0 + (7 * k) % N_REC for k in range(150)] + [ROW0 - 1, ROW0 + N_REC, 5, I64_MIN], N.ROWS_I64, ROW0),
}


@pytest.mark.parametrize("name", list(ROW_LISTS))
def test_row_lists(main, name):
    d, _, items, words, v = main
    rows, rdt, row0 = ROW_LISTS[name]
    both = TH.rules(words)[4]
    wants, _ = run_c(d, items, [both, TR.Rule("t", None, 1024, 0)], v, rows, rdt, row0)
    if name != "only skipped rows":
        assert 0 < wants[0].matched < wants[0].total and wants[0].total == wants[1].total


@pytest.mark.parametrize("i", range(len(TH.rules([]))))
def test_rules(main, i):
    """Buckets, a vocabulary, both, lower on and off, punctuation, max_tokens and max_elems, each beside
    a second spec in the same call; over every record, so over every length and kind of content."""
    d, _, items, words, v = main
    rule = TH.rules(words)[i]
    wants, _ = run_c(d, items, [rule, TR.Rule("s", None, 1000, 0, lower=True)], v)
    if rule.table:
        assert 0 < wants[0].matched < wants[0].total, rule


@pytest.mark.parametrize("cap", ["T + 3", "T", "T // 2", "0", "NULL"])
def test_capacities_with_and_without_counters(main, cap):
    d, _, items, words, v = main
    caps = {"T + 3": lambda t: t + 3, "T": lambda t: t, "T // 2": lambda t: t // 2, "0": 0, "NULL": None}
    rows = np.random.default_rng(3).integers(0, N_REC, 150).tolist() + [LONG_REC]
    rule = TH.rules(words)[4]
    for with_stats in (True, False):
        run_c(d, items, [rule, rule], v, rows, caps=[caps[cap], lambda t: t + 3], with_stats=with_stats)


def test_refusals_leave_the_poison_and_empty_cases(main):
    import torch

    d, res, items, words, v = main
    lib = N.lib()
    fresh = new_decoder()
    host_only = RawVocab([b"q"])
    try:
        rule = TR.Rule("t", {}, default=-1)
        tot = torch.full((1,), -1, dtype=torch.int64, device=dev())
        st = torch.full((1, 4), 77, dtype=torch.int32, device=dev())
        outs = Outs(3, 16)
        s_n = next(s for s in range(len(res.slot_key)) if res.slot_key[s] == "n")

        def call(dec=d, k=1, rdt=N.ROWS_I64, m=3, voc=v, **kw):
            torch.cuda.synchronize()
            return call_c(dec, [rule] * k, voc, [outs] * max(k, 1), None, rdt, m, 0, tot, st, **kw) if k == 1 else \
                dec._lib.tfrg_result_token_ids(dec._ctx, (N.TfrgTokSpec * 17)(), k, None, rdt, m, 0, None, None, None)

        ro_ptr, id_ptr = outs.ro.data_ptr(), outs.ids.data_ptr()
        for bad in (dict(k=0), dict(k=N.TOK_MAX_SPECS + 1), dict(slot=len(res.slot_key)), dict(slot=s_n), dict(row_offsets=None),
                    dict(row_offsets=ro_ptr + 4), dict(ids=id_ptr + 4), dict(flags=2), dict(flags=1 << 31), dict(vocab=None),
                    dict(voc=host_only), dict(m=1 << 31)):
            assert call(**bad) == -1, bad
            assert lib.tfrg_last_error().startswith(b"tfrg_result_token_ids: "), bad
            torch.cuda.synchronize()
            outs.untouched()
            assert tot.cpu().tolist() == [-1] and st.cpu().tolist() == [[77] * 4], bad
        assert lib.tfrg_ctx_set_token_split(d._ctx, 7) == -1 and lib.tfrg_ctx_set_token_split(d._ctx, 65537) == -1
        # m == 0: row_offsets[0] = 0, totals 0, no kernel
        assert call(m=0) == 0
        torch.cuda.synchronize()
        assert outs.ro.cpu().tolist()[0] == 0 and bool((outs.id_buf == 0xA5).all()) and tot.cpu().tolist() == [0]
        assert st.cpu().tolist() == [[0] * 4]
        # n == 0: every row is skipped
        buf, s0, e0 = payload_input(TH.text_batch()[0])
        assert len(fresh.decode(buf[: int(e0[4])], s0[:5], e0[:5], payload_only=True)) == 5  # (the keys get their slots)
        assert len(fresh.decode(buf[:0], s0[:0], e0[:0], payload_only=True)) == 0
        outs = Outs(3, 16)
        assert call(dec=fresh, slot=slot_of(fresh, "t")) == 0
        torch.cuda.synchronize()
        assert outs.ro.cpu().tolist() == [0, 0, 0, 0] and bool((outs.id_buf == 0xA5).all())
        assert tot.cpu().tolist() == [0] and st.cpu().tolist() == [[0, 0, 0, 3]]
    finally:
        host_only.close()
        fresh.close()


def test_materialized_column():
    d = new_decoder()
    payloads, items = TH.text_batch()
    words = TH.vocab_words(items)
    v = RawVocab(words, device=0)
    try:
        res = d.decode(*payload_input(payloads), payload_only=True, materialize_bytes=True)
        assert res.bytes_data is not None and v.rc == 0
        d.set_ragged_tile(TILE)
        rs = TH.rules(words)
        wants, _ = run_c(d, items, [rs[4], rs[8], rs[6]], v, with_bad(BAD64, 200))
        assert 0 < wants[0].matched < wants[0].total
    finally:
        v.close()
        d.close()


def test_optimistic_decode_with_implicit_offsets():
    """A device-resident optimistic decode whose ``id`` slot's bytes_off words are not stored (the column
    is poisoned before the decode): every byte comes from the end-relative view, the first call confirms
    the decode itself, and the poison in the unwritten column survives the calls."""
    n1 = 2000
    items = [{"id": [b"img-%08d" % i]} for i in range(n1)]
    fr = synth.framed(synth.c1_payloads(n1))
    d = IO.new_decoder(fr)
    words = [b"%08d" % i for i in range(0, n1, 3)] + [b"img"]
    v = RawVocab(words, device=0)
    try:
        assert v.rc == 0
        run = IO.Run(d, *fr, "u32")  # (no info, fetch or view before the calls)
        d.set_ragged_tile(TILE)
        dash = TR.WHITESPACE + b"-"
        rules = [TR.Rule("id", {w: i for i, w in enumerate(words)}, 11, len(words), delims=dash), TR.Rule("id", None, 1 << 20, 0)]
        wants, _ = run_c(d, items, rules, v)
        assert 0 < wants[0].matched < wants[0].total == 2 * n1 and wants[1].total == n1
        sid = slot_of(d, "id")
        assert int(run.info().implicit_off_slots) == 1 << sid and run.reruns() == 0
        run_c(d, items, rules, v, np.random.default_rng(4).integers(-3, n1 + 3, 700), N.ROWS_I32)
        fresh = IO.new_decoder(fr, optimistic="0")
        try:
            want = IO.Run(fresh, *fr, "u32").fetch()
        finally:
            fresh.close()
        run.assert_raw(want, 1 << sid)  # (poison still: the calls neither read nor wrote the column)
    finally:
        v.close()
        d.close()


def test_python_device_path_against_the_reference_and_the_numpy_path(main):
    d, res, items, words, _ = main
    vocab = I.Vocabulary(words, device=0)
    try:
        d.set_token_split(0)
        rs = [*TH.rules(words)[4:9], TR.Rule("zz", {}, default=-1)]
        specs = [TH.spec_of(r, vocab, str(i)) for i, r in enumerate(rs)]
        rows = [0, N_REC, -1, 5, LONG_REC, 3, 3, *range(20, 90)]
        for r in (None, rows):
            got = d.token_ids(specs, rows=None if r is None else to_dev(r))  # no capacity: exact tensors
            host = res.token_ids(specs, rows=None if r is None else [g for g in r if 0 <= g < N_REC])
            for sp, rule in zip(specs, rs):
                k, want = sp.out_name, TR.expect(items, rule, r)
                ids, ro = got[k]
                assert ids.numel() == want.total == got.capacity[k] == got.totals[k] and not got.overflowed[k], rule
                assert np.array_equal(ids.cpu().numpy(), want.ids) and np.array_equal(ro.cpu().numpy(), want.row_offsets), rule
                assert got.stats[k].tolist() == want.stats and np.array_equal(host[k][0], want.ids), rule
        want = TR.expect(items, rs[0], rows)
        got = d.token_ids(specs[:1], rows=to_dev(rows), capacity=want.total - 5)
        assert got.overflowed["0"] and np.array_equal(got["0"][0].cpu().numpy(), want.ids[:-5])
        with pytest.raises(ValueError, match="device"):
            d.token_ids([T.TokenIds("t", I.Vocabulary([b"q"]))])
    finally:
        vocab.close()
