"""One context through every kind of decode in turn, and a re-learn between a decode and its readers.

The context keeps what it knows about the last decode in one record that is replaced as a whole
(DESIGN.md "The context"): nothing of an earlier decode (implicit columns, implicit bytes_off words,
a materialized column, a pending confirmation, a value hint) may show in a later one, and nothing a
later tfrg_learn_templates learns may show in an earlier decode's columns.

Input: 321 C1 records (five 64-record groups and one lane, two 256-record tiles, two record shapes).
Every result is compared column by column, fetched and through the device view copied back, with a
fresh TFRG_OPTIMISTIC=0 context that decoded that input alone (every pass, every word stored) and with
the oracle; never with the context under test."""

import ctypes as C
import types

import numpy as np
import pytest

from tests._columns import batch_from_oracle
from tests.test_dense_gpu import d2h
from tests.test_implicit_off_gpu import (Run, _dense_host, _ragged_host, _written, assert_equal_columns, c1_input,
                                         new_decoder, slot_of)
from tests.test_tpl_stage_gpu import COLS
from tfr_reader import _native as N
from tfr_reader import dense as D
from tfr_reader import ragged as R

pytestmark = pytest.mark.gpu

NREC = 321
ALL = COLS + ("aux",)
LT_SLOT, LT_WORDS = 8 + 4 * 16 + 3 * 64, 8 + 4 * 16 + 3 * 64 + 3 * 16  # (tfrg_layout.h: kLtSlot, kLtWords)


@pytest.fixture(scope="module")
def sample():
    return c1_input(NREC)


@pytest.fixture(scope="module")
def oracle(sample):
    return batch_from_oracle(*sample)


def device_view(dec, like):
    """The columns of ``dec.device_columns()`` copied back, sized as the result `like`."""
    cols = dec.device_columns()
    v = types.SimpleNamespace(info=like.info)
    for name in ALL:
        want = np.asarray(getattr(like, name))
        got = d2h(getattr(cols, name), want.size, want.dtype) if want.size else np.zeros(0, want.dtype)
        setattr(v, name, got.reshape(want.shape))
    return v


def assert_columns(got, want, skip=()):
    """(aux is a failed record's error detail: a full decode leaves the word of an OK record unwritten)"""
    failed = np.asarray(want.status) != 0
    for k in ALL:
        if k not in skip:
            g, w = np.asarray(getattr(got, k)), np.asarray(getattr(want, k))
            assert np.array_equal(g[failed], w[failed]) if k == "aux" else np.array_equal(g, w), k


def truth_of(sample, inp, mode, count=None, **flags):
    """The fetched result of `inp` on a fresh context that runs every pass and stores every word."""
    d = new_decoder(sample, optimistic="0")
    try:
        t = Run(d, *inp, mode, count=count, **flags).fetch()
        assert int(t.info.implicit_cols) == 0 and int(t.info.implicit_off_slots) == 0
        return t
    finally:
        d.close()


def check(run, truth, orc, skip_oracle=(), optimistic=False):
    """The run's fetched result and its device view, each against the truth context and the oracle.
    `optimistic`: no record failed and the decode stored no aux word, so both hand out zeros."""
    got = run.fetch()
    assert_equal_columns(got, truth)
    view = device_view(run.dec, truth)
    for r in (got, view):
        assert_columns(r, truth)
        assert_columns(r, orc, skip_oracle)
        assert not (optimistic and np.asarray(r.aux).any())
    return got


# ------------------------------------------------------------------ 1. one context, many kinds of decode
def test_one_context_through_every_kind_of_decode(sample, oracle):
    buf, st, en = sample
    dec = new_decoder(sample)
    try:
        t_clean = truth_of(sample, sample, "ends")
        sid = slot_of(t_clean, "id", 1)

        def clean_optimistic():  # steps a and g
            run = Run(dec, buf, st, en, "ends")
            info = run.info()
            assert int(info.implicit_off_slots) == 1 << sid and int(info.implicit_cols) == 7 and run.reruns() == 0
            assert int(info.n_records) == NREC
            run.assert_raw(t_clean, 1 << sid)
            check(run, t_clean, oracle, optimistic=True)

        clean_optimistic()  # a

        # b: u64 offsets, the first 65 records: every bytes_off word stored
        t_b = truth_of(sample, sample, "u64", count=65)
        run = Run(dec, buf, st, en, "u64", count=65)
        info = run.info()
        assert int(info.implicit_off_slots) == 0 and int(info.n_records) == 65 and run.reruns() == 0
        run.assert_raw(t_b, 0)
        check(run, t_b, batch_from_oracle(buf, st[:65], en[:65]))

        # c: the materialized byte column
        t_c = truth_of(sample, sample, "ends", materialize_bytes=True)
        run = Run(dec, buf, st, en, "ends", materialize_bytes=True)
        info = run.info()
        assert int(info.implicit_off_slots) == 0 and run.reruns() == 0
        got = check(run, t_c, oracle)
        ids = b"".join(b"img-%08d" % (7 + i) for i in range(NREC))
        assert got.bytes_data.tobytes() == t_c.bytes_data.tobytes() == ids
        assert got.bytes_offsets.tobytes() == t_c.bytes_offsets.tobytes()
        assert got.bytes_offsets.tolist() == list(range(0, 12 * NREC + 1, 12))

        # d: an empty batch
        t_d = truth_of(sample, sample, "ends", count=0)
        run = Run(dec, buf, st, en, "ends", count=0)
        info = run.info()
        assert int(info.n_records) == 0 and int(info.implicit_cols) == 0 and int(info.implicit_off_slots) == 0
        assert list(info.kind_totals) == [0, 0, 0, 0] and list(t_d.info.kind_totals) == [0, 0, 0, 0]
        dec.device_columns()
        got = run.fetch()
        assert_equal_columns(got, t_d)
        assert not np.asarray(got.row_splits).any() and got.i64.size == 0 and got.bytes_off.size == 0

        # e: one payload byte of record 130 flipped (a byte of its id): one re-run, nothing implicit
        bad = buf.copy()
        bad[int(en[130]) - 6] ^= 0x01
        assert batch_from_oracle(bad, st, en).bytes_off.tobytes() == oracle.bytes_off.tobytes()  # (still parses)
        t_e = truth_of(sample, (bad, st, en), "ends")
        run = Run(dec, bad, st, en, "ends")
        info = run.info()
        assert run.reruns() == 1 and int(info.implicit_cols) == 0 and int(info.implicit_off_slots) == 0
        run.assert_raw(t_e, 0)
        got = check(run, t_e, oracle, skip_oracle=("verdict",))  # (the oracle checks no CRC)
        v = np.array(got.verdict)
        assert np.flatnonzero(v != 7).tolist() == [130] and int(v[130]) == 3

        # f: a value hint far too small: re-run at the worst case
        dec.set_value_caps(bytes_values=8)
        try:
            run = Run(dec, buf, st, en, "ends")
            info = run.info()
            print("step f: reruns", run.reruns(), "implicit_cols", int(info.implicit_cols))
            assert run.reruns() >= 1 and int(info.implicit_cols) == 0 and int(info.implicit_off_slots) == 0
            check(run, t_clean, oracle)
        finally:
            dec.set_value_caps()

        clean_optimistic()  # g: as a, nothing left of b - f
    finally:
        dec.close()


# ------------------------------------------------------------------ 2. a re-learn between a decode and its readers
DENSE = [D.Dense("id", "uint8", 12, lengths=True)]
RAGGED = [R.Ragged("id", "uint8")]


def slot_words(dec, n_slots):
    """Per slot (order word, element length) of the first learned template (tfrg_template_words)."""
    w = np.zeros(LT_WORDS, np.uint32)
    assert N.lib().tfrg_template_words(dec._ctx, N.ptr(w), LT_WORDS, None) >= 1
    return [(int(w[LT_SLOT + 3 * k]) >> 16, (int(w[LT_SLOT + 3 * k]) >> 8) & 0xFF) for k in range(n_slots)]


@pytest.fixture(scope="module")
def other_sample():
    """The same two keys, the id first and 8 bytes long: other order words, another constant length."""
    return _written(lambda i: [("id", "bytes_list", [b"i%07d" % i]), ("label", "int64_list", [100 + i % 200])], NREC)


@pytest.fixture(scope="module")
def relearn_truth(sample):
    """A context that never saw the second sample: the fetched columns, dense and ragged of the id."""
    d = new_decoder(sample, optimistic="0")
    try:
        run = Run(d, *sample, "ends")
        return run.fetch(), _dense_host(d.dense(DENSE)), _ragged_host(d.ragged(RAGGED))
    finally:
        d.close()


@pytest.mark.parametrize("first", ["info", "fetch", "device_columns", "dense", "ragged"])
def test_relearn_between_a_decode_and_its_readers(sample, other_sample, oracle, relearn_truth, first):
    buf, st, en = sample
    truth, want_dense, want_ragged = relearn_truth
    ids = b"".join(b"img-%08d" % (7 + i) for i in range(NREC))
    assert want_dense[0]["id"] == ids and want_ragged[0]["id"][0] == ids  # (the writer's bytes)
    sid, n_slots = slot_of(truth, "id", 1), len(truth.slot_kind)
    dec = new_decoder(sample)
    try:
        run = Run(dec, buf, st, en, "ends")  # (no info: the decode is unconfirmed, its columns implicit)
        before = slot_words(dec, n_slots)
        assert dec.learn_templates(*other_sample) >= 1
        after = slot_words(dec, n_slots)
        assert before[sid][1] == 12 and after[sid][1] == 8
        assert all(b[0] != a[0] for b, a in zip(before, after)), (before, after)
        delta = C.c_int32(0)  # (tfrg_ctx_rel_off answers from the live shapes: the id is no longer end-relative)
        assert N.lib().tfrg_ctx_rel_off(dec._ctx, sid, C.byref(delta)) != 0

        def fetched():
            got = dec._fetch(buf, run.st, run.en, truth.info, False)  # (sized by the truth's info: no info() first)
            import torch

            torch.cuda.synchronize()
            assert_columns(got, truth)
            assert_columns(got, oracle)
            assert not np.asarray(got.aux).any()

        def viewed():
            view = device_view(dec, truth)
            assert_columns(view, truth)
            assert_columns(view, oracle)
            assert not np.asarray(view.aux).any()

        def info():
            i = run.info()
            assert int(i.implicit_cols) == 7 and int(i.implicit_off_slots) == 1 << sid and run.reruns() == 0
            assert list(i.kind_totals) == list(truth.info.kind_totals)

        readers = {"info": info, "fetch": fetched, "device_columns": viewed,
                   "dense": lambda: _assert_same(_dense_host(dec.dense(DENSE)), want_dense),
                   "ragged": lambda: _assert_same(_ragged_host(dec.ragged(RAGGED)), want_ragged)}
        readers[first]()
        for name, reader in readers.items():
            if name != first:
                reader()
    finally:
        dec.close()


def _assert_same(got, want):
    assert got == want
