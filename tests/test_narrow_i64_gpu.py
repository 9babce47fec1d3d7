"""Narrowed int64 columns (tfrg_info.i64_width): an optimistic decode whose learned record shapes hold
every int64 slot as one varint of at most 2 / 4 bytes stores the column in elements of 2 / 4 bytes, in a
buffer of its own. tfrg_result_fetch and tfrg_result_device still give a true int64 column (one
widening kernel per decode); dense / dense_rows / ragged / select read the narrow column as it is;
tfrg_result_i64_narrow hands it out.

The truth of every case is a second context created with TFRG_NARROW_I64=0 (the same decode, every value
stored as 8 bytes) decoding the same input through the same entry point, and for the fetched values also
the oracle's column (tests/_columns.py). All comparisons are exact.

Learning the shapes decodes the sample on the same context, and contexts are reused, so a column could
already hold the expected values when the decode under test stores nothing there. Every decode here is
therefore preceded by a poisoning of both the int64 and the narrow column with 0xa5 bytes
(``Run.__init__``), and the raw columns are read back before any view is taken: the narrow one holds the
values, the int64 one still the poison.

Inputs are 5,000 records at most. TFRG_TPL_STAGE=2 with TFRG_TPL_GPW=8 runs the staged group loop of
the headline launch at that size, TFRG_TPL_STAGE=0 the per-lane kernel (tests/test_tpl_dma_gpu.py)."""

import ctypes as C

import numpy as np
import pytest

from tests._columns import batch_from_oracle
from tests.test_dense_gpu import d2h
from tests.test_tpl_stage_gpu import COLS
from tests.test_unchecked_frames_gpu import _launch, _upload
from tfr_reader import dense as D
from tfr_reader import hip, ragged as R, select as S, synth, writer

pytestmark = pytest.mark.gpu

N1 = 5000
SIZES = [1, 63, 64, 65, 257, N1]  # a lone lane, the edges of a 64-record group, of a 256-record tile, many groups
NP_OF = {2: np.uint16, 4: np.uint32, 8: np.uint64}


def host_rule(values) -> int:
    """The width the learner's rule gives int64 slots holding `values`: 7 value bits per varint byte."""
    if min(values) < 0 or max(values) >= 1 << 28:
        return 8
    return 2 if max(values) < 1 << 14 else 4


def _ids(i):
    return f"img-{i:08d}".encode()


def labelled(labels, n=N1):
    """C1-shaped framed records whose labels cycle through `labels`."""
    return synth.framed([writer.encode_example([("label", "int64_list", [int(labels[i % len(labels)])]),
                                                ("id", "bytes_list", [_ids(i)])]) for i in range(n)])


def _hip_memset(ptr, nbytes):
    import torch

    torch.cuda.synchronize()
    rt = C.CDLL("libamdhip64.so")
    assert rt.hipMemset(C.c_void_p(ptr), 0xA5, C.c_size_t(nbytes)) == 0
    assert rt.hipDeviceSynchronize() == 0


def new_decoder(sample, *, narrow=None, stage="2", optimistic="1"):
    """A fresh context (the switches are read at its creation) that learned `sample`'s shapes. A context
    that narrows then decodes the whole sample once from device memory: its narrow column is allocated
    at the size of every later decode here (each is of that sample or a part of it), so its address is
    known before the decodes under test and can be poisoned."""
    mp = pytest.MonkeyPatch()
    mp.setenv("TFRG_OPTIMISTIC", optimistic)
    mp.setenv("TFRG_TEMPLATES", "1")
    mp.setenv("TFRG_TPL_STAGE", stage)
    mp.setenv("TFRG_TPL_GPW", "8")
    mp.delenv("TFRG_IMPLICIT_OFF", raising=False)
    mp.delenv("TFRG_NARROW_I64", raising=False)
    if narrow is not None:
        mp.setenv("TFRG_NARROW_I64", narrow)
    try:
        d = hip.HipDecoder(0)
    finally:
        mp.undo()
    res = d.decode(*sample)
    assert d.template_count() >= 1
    d._sample_i64 = int(res.info.kind_totals[3])
    buf, st, en = sample
    bufs = _upload(buf, st, en, "ends")
    _launch(d, bufs, buf, st, en, "ends")
    d._warm_width = int(d.info().i64_width)
    d._narrow_ptr = d.i64_narrow()[0] if d._warm_width < 8 else 0
    return d


class Run:
    """One device-resident decode, both value columns poisoned first; the uploaded bytes and offsets
    stay in place while it is read."""

    def __init__(self, dec, buf, st, en, mode, count=None):
        n = len(st) if count is None else count
        self.dec, self.buf, self.n = dec, buf, n
        self.st, self.en = np.ascontiguousarray(st[:n]), np.ascontiguousarray(en[:n])
        self.bufs = _upload(buf, self.st, self.en, mode)
        # (the view of the previous decode: the address of the context's int64 column)
        self.wide_ptr = C.cast(dec.device_columns().i64, C.c_void_p).value
        _hip_memset(self.wide_ptr, 8 * dec._sample_i64)
        if dec._narrow_ptr:
            _hip_memset(dec._narrow_ptr, dec._warm_width * dec._sample_i64)
        self.before = dec.device_bytes()[1]
        _launch(dec, self.bufs, buf, self.st, self.en, mode)

    def info(self):
        return self.dec.info()

    def reruns(self):
        return self.dec.device_bytes()[1] - self.before

    def fetch(self):
        import torch

        r = self.dec._fetch(self.buf, self.st, self.en, self.dec.info(), False)
        torch.cuda.synchronize()
        return r

    def raw_wide(self, count):
        """The int64 column as the decode left it: no view, no fetch (after the confirmation)."""
        return d2h(C.c_void_p(self.wide_ptr), count, np.uint64)

    def narrow(self, count):
        """(the stored column of tfrg_result_i64_narrow, its width)"""
        ptr, width = self.dec.i64_narrow()
        return d2h(C.c_void_p(ptr), count, NP_OF[width]), width, ptr

    def device_i64(self, count):
        cols = self.dec.device_columns()
        assert C.cast(cols.i64, C.c_void_p).value == self.wide_ptr  # (the column that was poisoned)
        return d2h(cols.i64, count, np.int64)


def assert_equal_columns(got, truth):
    for k in COLS:
        assert np.array_equal(np.array(getattr(got, k)), np.array(getattr(truth, k))), k
    assert list(got.info.kind_totals) == list(truth.info.kind_totals)


def assert_stored_narrow(run, truth_i64, width):
    """After a narrowed decode, before any view: the narrow column holds the values and the int64
    column still the poison -- the kernel stored narrow and nothing widened early."""
    info = run.info()
    assert int(info.i64_width) == width and run.reruns() == 0 and int(info.tpl_groups_missed) == 0
    got, w, ptr = run.narrow(truth_i64.size)
    assert w == width and ptr == run.dec._narrow_ptr
    assert got.dtype.itemsize == width and np.array_equal(got.astype(np.int64), truth_i64)
    assert (run.raw_wide(truth_i64.size) == 0xA5A5A5A5A5A5A5A5).all()


# ------------------------------------------------------------------ consumers
DENSE_SPECS = [D.Dense("label", "int64", lengths=True), D.Dense("label", "int32", lengths=True, name="label32"),
               D.Dense("id", "uint8", 12, lengths=True)]
RAGGED_SPECS = [R.Ragged("label", "int64"), R.Ragged("label", "int32", name="label32"), R.Ragged("id", "uint8")]


def _dense_host(got):
    return ({k: v.cpu().numpy().tobytes() for k, v in got.items()},
            {k: v.cpu().numpy().tobytes() for k, v in got.lengths.items()},
            {k: v.tolist() for k, v in got.stats.items()}, got.skipped)


def _ragged_host(got):
    tot = got.totals
    return ({k: (v[: tot[k]].cpu().numpy().tobytes(), o.cpu().numpy().tobytes()) for k, (v, o) in got.items()},
            tot, {k: v.tolist() for k, v in got.stats.items()})


def _select_host(dec, where, rows=None):
    sel = dec.select(where, rows=rows)
    return sel.rows[: sel.count].cpu().numpy().tolist(), sel.stats


def _consumers(dec, rows, pivot, key="label"):
    import torch

    d_rows = torch.from_numpy(rows).to(torch.device("cuda", 0))
    where = [S.Term(key, "int64", "<", pivot)]
    return (_dense_host(dec.dense(DENSE_SPECS)), _dense_host(dec.dense(DENSE_SPECS, rows=d_rows)),
            _ragged_host(dec.ragged(RAGGED_SPECS, rows=d_rows)), _ragged_host(dec.ragged(RAGGED_SPECS)),
            _select_host(dec, where), _select_host(dec, [S.Term(key, "int64", ">=", pivot)], rows=d_rows))


def _rows(n, seed=5):
    rng = np.random.default_rng(seed)
    rows = np.concatenate([rng.permutation(n)[: min(n, 700)], rng.integers(0, n, 300), [0, n - 1, 0, n - 1]]).astype(np.int64)
    return rows


# ------------------------------------------------------------------ 1. C1: width 2, every kernel path
@pytest.fixture(scope="module")
def c1():
    blob, offs = synth.c1_blob(N1, 100, 7)  # (labels 100 .. 999 and 0 .. 99 again: 1- and 2-byte varints, two shapes)
    buf = synth.frame_blob(blob, offs)
    en = (offs[1:] + 16 * np.arange(1, N1 + 1)).astype(np.uint64)
    st = np.concatenate([[0], en[:-1]]).astype(np.uint64)
    assert len(set((en - st).tolist())) == 2
    return buf, st, en


@pytest.fixture(scope="module")
def c1_oracle(c1):
    """The oracle's int64 column of the C1 input (one int64 slot: record r's label is row r)."""
    r = batch_from_oracle(*c1)
    assert r.i64.shape == (N1,) and host_rule(r.i64.tolist()) == 2 and int(r.i64.max()) > 127
    return r.i64


@pytest.fixture(scope="module")
def c1_truth(c1):
    d = new_decoder(c1, narrow="0")
    assert d._warm_width == 8
    yield d
    d.close()


@pytest.fixture(scope="module", params=["2", "0"], ids=["staged", "per_lane"])
def c1_new(request, c1):
    d = new_decoder(c1, stage=request.param)
    assert d._warm_width == 2 and d._narrow_ptr
    yield d
    d.close()


@pytest.mark.parametrize("mode", ["ends", "u32", "u64"])
@pytest.mark.parametrize("n", SIZES)
def test_c1_stored_narrow_then_fetch_and_device_view(c1, c1_new, c1_truth, c1_oracle, n, mode):
    buf, st, en = c1
    truth = Run(c1_truth, buf, st, en, mode, count=n).fetch()
    assert int(truth.info.i64_width) == 8
    run = Run(c1_new, buf, st, en, mode, count=n)
    assert_stored_narrow(run, c1_oracle[:n], 2)
    got = run.fetch()
    assert got.i64.dtype == np.int64 and got.i64.tobytes() == c1_oracle[:n].tobytes()
    assert_equal_columns(got, truth)
    for _ in range(2):  # (the widening runs once per decode: the second view hands out the same column)
        assert run.device_i64(n).tobytes() == c1_oracle[:n].tobytes()
    assert run.narrow(n)[0].astype(np.int64).tobytes() == c1_oracle[:n].tobytes()  # (and the narrow one stays)


def test_device_view_before_any_fetch(c1, c1_new, c1_oracle):
    buf, st, en = c1
    run = Run(c1_new, buf, st, en, "ends")
    assert run.device_i64(N1).tobytes() == c1_oracle.tobytes()
    assert run.raw_wide(N1).view(np.int64).tobytes() == c1_oracle.tobytes()  # (the view wrote the column itself)
    assert run.fetch().i64.tobytes() == c1_oracle.tobytes()


@pytest.mark.parametrize("mode", ["ends", "u64"])
@pytest.mark.parametrize("n", [65, 257, N1])
def test_consumers_read_the_narrow_column(c1, c1_new, c1_truth, c1_oracle, n, mode):
    buf, st, en = c1
    rows = _rows(n)
    t_run = Run(c1_truth, buf, st, en, mode, count=n)  # (kept: the consumers read its uploaded input)
    want = _consumers(c1_truth, rows, 128)
    assert int(t_run.info().i64_width) == 8
    run = Run(c1_new, buf, st, en, mode, count=n)  # (no info, fetch or view before the consumers: they confirm the decode)
    got = _consumers(c1_new, rows, 128)
    assert got == want
    labels = np.frombuffer(got[0][0]["label"], np.int64)
    assert labels.tobytes() == c1_oracle[:n].tobytes()  # (and against the oracle)
    assert np.frombuffer(got[0][0]["label32"], np.int32).tolist() == c1_oracle[:n].tolist()
    assert got[4][0] == np.flatnonzero(c1_oracle[:n] < 128).tolist()
    # nothing the consumers gave came from the int64 column, and none of them widened it
    assert_stored_narrow(run, c1_oracle[:n], 2)
    assert run.device_i64(n).tobytes() == c1_oracle[:n].tobytes()
    assert _consumers(c1_new, rows, 128) == want


def test_switch_off_stores_eight_bytes(c1, c1_truth, c1_oracle):
    buf, st, en = c1
    run = Run(c1_truth, buf, st, en, "ends")
    info = run.info()
    assert int(info.i64_width) == 8 and int(info.implicit_cols) == 7 and run.reruns() == 0  # (optimistic all the same)
    got, width, ptr = run.narrow(N1)
    assert width == 8 and ptr == run.wide_ptr and got.view(np.int64).tobytes() == c1_oracle.tobytes()
    assert run.raw_wide(N1).view(np.int64).tobytes() == c1_oracle.tobytes()  # (stored by the decode over the poison)


def test_a_decode_that_is_not_optimistic_stores_eight_bytes(c1, c1_oracle):
    buf, st, en = c1
    d = new_decoder(c1, optimistic="0")
    try:
        assert d._warm_width == 8
        run = Run(d, buf, st, en, "ends")
        assert int(run.info().i64_width) == 8
        assert run.raw_wide(N1).view(np.int64).tobytes() == c1_oracle.tobytes()
        assert run.fetch().i64.tobytes() == c1_oracle.tobytes()
    finally:
        d.close()


@pytest.mark.parametrize("n", [65, N1])
def test_a_host_decode_stores_eight_bytes(c1, c1_new, c1_oracle, n):
    """tfrg_decode_host on a context whose device decodes narrow: the int64
    column stored by the decode itself as 8-byte values -- the narrow column is not written, and nothing
    is widened for the fetch that follows it."""
    buf, st, en = c1
    wide_ptr = C.cast(c1_new.device_columns().i64, C.c_void_p).value
    _hip_memset(wide_ptr, 8 * c1_new._sample_i64)
    _hip_memset(c1_new._narrow_ptr, 2 * c1_new._sample_i64)
    before = c1_new.device_bytes()[1]
    res = c1_new.decode(buf, st[:n], en[:n])
    assert int(res.info.i64_width) == 8 and c1_new.device_bytes()[1] == before  # (no re-run)
    assert res.i64.tobytes() == c1_oracle[:n].tobytes()
    ptr, width = c1_new.i64_narrow()
    assert (ptr, width) == (wide_ptr, 8)
    assert d2h(C.c_void_p(wide_ptr), n, np.int64).tobytes() == c1_oracle[:n].tobytes()
    assert (d2h(C.c_void_p(c1_new._narrow_ptr), n, np.uint16) == 0xA5A5).all()  # (the narrow column: untouched)
    # and the device decode after it narrows again
    run = Run(c1_new, buf, st, en, "ends", count=n)
    assert_stored_narrow(run, c1_oracle[:n], 2)


# ------------------------------------------------------------------ 2. value boundaries
def _check_sample(sample, values, stage="2", modes=("ends", "u64"), sizes=(N1,)):
    """`sample` on a fresh context and on the TFRG_NARROW_I64=0 one: the width the host rule predicts for
    `values`, the raw columns, the fetch, the device view against the oracle's column."""
    buf, st, en = sample
    width = host_rule(values)
    orc = batch_from_oracle(*sample)
    new, tr = new_decoder(sample, stage=stage), new_decoder(sample, narrow="0", stage=stage)
    try:
        assert new._warm_width == width and tr._warm_width == 8
        for mode in modes:
            for n in sizes:
                truth = Run(tr, buf, st, en, mode, count=n).fetch()
                want = truth.i64
                if n == N1:
                    assert want.tobytes() == orc.i64.tobytes()
                run = Run(new, buf, st, en, mode, count=n)
                assert_stored_narrow(run, want, width)
                assert_equal_columns(run.fetch(), truth)
                assert run.device_i64(want.size).tobytes() == want.tobytes()
    finally:
        new.close()
        tr.close()
    return orc


@pytest.mark.parametrize("stage", ["2", "0"], ids=["staged", "per_lane"])
def test_the_boundaries_of_one_and_two_byte_varints(stage):
    values = [0, 127, 128, 16383]
    orc = _check_sample(labelled(values), values, stage=stage)
    assert sorted(set(orc.i64.tolist())) == values


@pytest.mark.parametrize("stage", ["2", "0"], ids=["staged", "per_lane"])
def test_three_and_four_byte_varints_store_four_bytes(stage):
    values = [16384, (1 << 28) - 1, 5, 16383, (1 << 21) - 1, 1 << 21]
    orc = _check_sample(labelled(values), values, stage=stage, sizes=(63, 65, N1))
    assert sorted(set(orc.i64.tolist())) == sorted(values)


# ------------------------------------------------------------------ 3. two int64 slots
def test_two_int64_slots_share_one_width_and_keep_their_bases():
    """a (<= 2 bytes) and b (3 bytes): width 4 for both; and both <= 2 bytes: width 2, b's narrow rows
    starting at byte 2 n, which is no multiple of a 128-byte line for any n here."""
    for b_of, vals in ((lambda i: 20000 + i % 100, [999, 20099]), (lambda i: 300 + i % 50, [999, 349])):
        sample = synth.framed([writer.encode_example([("a", "int64_list", [i % 1000]), ("b", "int64_list", [b_of(i)]),
                                                      ("id", "bytes_list", [_ids(i)])]) for i in range(N1)])
        assert (host_rule(vals) * N1) % 128 != 0 and (host_rule(vals) * 257) % 128 != 0
        orc = _check_sample(sample, vals, modes=("ends",), sizes=(257, N1))
        assert orc.i64[:N1].tolist() == [i % 1000 for i in range(N1)]
        assert orc.i64[N1:].tolist() == [b_of(i) for i in range(N1)]
    # the consumers over the second slot, against the TFRG_NARROW_I64=0 context
    buf, st, en = sample
    new, tr = new_decoder(sample), new_decoder(sample, narrow="0")
    try:
        specs = [D.Dense("b", "int64", lengths=True), D.Dense("a", "int32", lengths=True)]
        rag = [R.Ragged("b", "int32"), R.Ragged("a", "int64")]
        rows = _rows(N1, 9)
        outs = []
        for d in (tr, new):
            import torch

            run = Run(d, buf, st, en, "ends")
            d_rows = torch.from_numpy(rows).to(torch.device("cuda", 0))
            outs.append((_dense_host(d.dense(specs)), _dense_host(d.dense(specs, rows=d_rows)),
                         _ragged_host(d.ragged(rag, rows=d_rows)), _select_host(d, [S.Term("b", "int64", ">", 320)])))
        assert outs[0] == outs[1]
        assert np.frombuffer(outs[1][0][0]["b"], np.int64).tolist() == orc.i64[N1:].tolist()
        assert_stored_narrow(run, orc.i64, 2)
    finally:
        new.close()
        tr.close()


# ------------------------------------------------------------------ 4. a miss re-runs with 8-byte values
@pytest.mark.parametrize("mode", ["ends", "u64"])
def test_an_unseen_shape_reruns_in_full(c1, c1_new, mode):
    """One record with a negative label (a 10-byte varint: no learned shape): the decode is re-run with
    every pass, which stores 8-byte values."""
    n, at = 1000, 517
    payloads = [writer.encode_example([("label", "int64_list", [-3 if i == at else (100 + i) % 1000]),
                                       ("id", "bytes_list", [_ids(i)])]) for i in range(n)]
    buf, st, en = synth.framed(payloads)
    orc = batch_from_oracle(buf, st, en)
    assert int(orc.i64[at]) == -3
    run = Run(c1_new, buf, st, en, mode)
    info = run.info()
    assert run.reruns() == 1 and int(info.i64_width) == 8 and int(info.implicit_cols) == 0
    got, width, ptr = run.narrow(n)
    assert width == 8 and ptr == run.wide_ptr and got.view(np.int64).tobytes() == orc.i64.tobytes()
    res = run.fetch()
    assert res.i64.tobytes() == orc.i64.tobytes()
    assert run.device_i64(n).tobytes() == orc.i64.tobytes()
    rows = _rows(n)
    lab = np.frombuffer(_consumers(c1_new, rows, 128)[0][0]["label"], np.int64)
    assert lab.tobytes() == orc.i64.tobytes()


# ------------------------------------------------------------------ 5. value-capacity hints
@pytest.mark.parametrize("stage", ["2", "0"], ids=["staged", "per_lane"])
def test_value_capacity_hints(c1, c1_oracle, stage):
    """A hint that holds every value: narrowed, within the hinted capacity. A hint below n: the rows past
    it are not stored (r < lim), the overflow is reported, and the re-run at the worst case runs every
    pass: 8-byte values."""
    buf, st, en = c1
    d = new_decoder(c1, stage=stage)
    try:
        d.set_value_caps(N1, 0, N1)
        run = Run(d, buf, st, en, "ends")
        assert_stored_narrow(run, c1_oracle, 2)
        assert run.fetch().i64.tobytes() == c1_oracle.tobytes()
        d.set_value_caps(N1 // 2, 0, N1)
        run = Run(d, buf, st, en, "ends")
        info = run.info()
        assert run.reruns() == 1 and int(info.i64_width) == 8
        got, width, ptr = run.narrow(N1)
        assert width == 8 and ptr == run.wide_ptr and got.view(np.int64).tobytes() == c1_oracle.tobytes()
        assert run.fetch().i64.tobytes() == c1_oracle.tobytes()
        assert run.device_i64(N1).tobytes() == c1_oracle.tobytes()
    finally:
        d.close()


# ------------------------------------------------------------------ 6. a re-learn between decode and fetch
def test_a_relearn_between_decode_and_fetch_leaves_the_result(c1, c1_oracle):
    buf, st, en = c1
    wide = labelled([5, 1 << 20], n=400)  # (shapes of width 4)
    none = synth.framed([writer.encode_example([("other", "int64_list", [1])]) for _ in range(8)])
    d = new_decoder(c1)
    try:
        for sample in (wide, none):
            run = Run(d, buf, st, en, "ends")
            d.learn_templates(*sample)
            assert_stored_narrow(run, c1_oracle, 2)  # (the decode's width, not the context's new one)
            assert run.fetch().i64.tobytes() == c1_oracle.tobytes()
            assert run.device_i64(N1).tobytes() == c1_oracle.tobytes()
            d.learn_templates(buf, st, en)
    finally:
        d.close()
