"""Implicit end-relative bytes_off words (tfrg_info.implicit_off_slots): an optimistic decode with u32
offsets does not store the bytes_off words of a bytes slot that lies at one distance from the record's
end in every learned shape; tfrg_result_fetch and tfrg_result_device fill them from the caller's u32
ends, and dense / dense_rows / ragged read the ends instead of the column.

The truth of every case is a second context created with TFRG_OPTIMISTIC=0 (every pass, every word
stored) decoding the same input through the same entry point, and for the fetched offsets also the
oracle's columns (tests/_columns.py). Nothing is compared against the path under test.

Learning the shapes decodes the sample on the same context (a host decode: u64 offsets, every word
stored), and contexts are reused, so the device column would already hold the expected words when the
decode under test skips its store. Every decode here is therefore preceded by a poisoning of the
context's whole bytes_off column (``poison_bytes_off``): a fill that did nothing, or a consumer that
read the column, gives 0xa5a5a5a5 offsets. The raw column is also read back without a view
(``Run.raw_off``): still poisoned where the mask says "not stored", the truth where it says "stored".

Inputs are 5,000 records at most. TFRG_TPL_STAGE=2 with TFRG_TPL_GPW=8 runs the staged group loop of
the headline launch at that size, TFRG_TPL_STAGE=0 the per-lane kernel (tests/test_tpl_dma_gpu.py)."""

import ctypes as C

import numpy as np
import pytest

from tests._columns import batch_from_oracle
from tests.test_dense_gpu import d2h
from tests.test_tpl_stage_gpu import COLS
from tests.test_unchecked_frames_gpu import _launch, _upload
from tfr_reader import _native as N
from tfr_reader import dense as D
from tfr_reader import hip, ragged as R, synth, writer

pytestmark = pytest.mark.gpu

N1 = 5000
POISON = 0xA5A5A5A5


def poison_bytes_off(dec):
    """Overwrites the whole bytes_off column of `dec`'s context (as large as its learning sample needs:
    every decode here is of that sample or a part of it) with 0xa5 bytes. Returns the column's address."""
    import torch

    ptr = C.cast(dec.device_columns().bytes_off, C.c_void_p).value
    torch.cuda.synchronize()
    rt = C.CDLL("libamdhip64.so")
    assert rt.hipMemset(C.c_void_p(ptr), 0xA5, C.c_size_t(4 * dec._sample_bytes_elements)) == 0
    assert rt.hipDeviceSynchronize() == 0
    return ptr


def new_decoder(sample, *, optimistic="1", stage="2", implicit_off=None, **flags):
    """A fresh context (the switches are read at its creation) that learned `sample`'s shapes."""
    mp = pytest.MonkeyPatch()
    mp.setenv("TFRG_OPTIMISTIC", optimistic)
    mp.setenv("TFRG_TEMPLATES", "1")
    mp.setenv("TFRG_TPL_STAGE", stage)
    mp.setenv("TFRG_TPL_GPW", "8")
    mp.delenv("TFRG_IMPLICIT_OFF", raising=False)
    if implicit_off is not None:
        mp.setenv("TFRG_IMPLICIT_OFF", implicit_off)
    try:
        d = hip.HipDecoder(0)
    finally:
        mp.undo()
    res = d.decode(*sample, **flags)
    assert d.template_count() >= 1
    d._sample_bytes_elements = int(res.info.kind_totals[1])
    return d


class Run:
    """One device-resident decode; the uploaded bytes and offsets stay in place while it is read."""

    def __init__(self, dec, buf, st, en, mode, count=None, **flags):
        n = len(st) if count is None else count
        self.dec, self.buf = dec, buf
        self.st, self.en = np.ascontiguousarray(st[:n]), np.ascontiguousarray(en[:n])
        self.n, self.mat = n, bool(flags.get("materialize_bytes"))
        self.bufs = _upload(buf, self.st, self.en, mode)
        self.raw_ptr = poison_bytes_off(dec)
        self.before = dec.device_bytes()[1]
        _launch(dec, self.bufs, buf, self.st, self.en, mode, **flags)

    def info(self):
        return self.dec.info()

    def reruns(self):
        return self.dec.device_bytes()[1] - self.before

    def fetch(self):
        import torch

        r = self.dec._fetch(self.buf, self.st, self.en, self.dec.info(), False, self.mat)
        torch.cuda.synchronize()
        return r

    def device_off(self, count):
        cols = self.dec.device_columns()
        assert C.cast(cols.bytes_off, C.c_void_p).value == self.raw_ptr  # (the column that was poisoned)
        return d2h(cols.bytes_off, count, np.uint32)

    def raw_off(self, count):
        """The column as the decode left it: no view, no fetch, no fill (after the confirmation)."""
        return d2h(C.c_void_p(self.raw_ptr), count, np.uint32)

    def assert_raw(self, truth, mask):
        """Per bytes slot: rows still poisoned where `mask` has the slot's bit, the truth's elsewhere."""
        n, raw = self.n, self.raw_off(int(truth.info.kind_totals[1]))
        rank = 0
        for s, kind in enumerate(truth.slot_kind):
            if kind != 1:
                continue
            rows = raw[rank * n : (rank + 1) * n]
            if (mask >> s) & 1:
                assert rows.size == n and (rows == POISON).all(), s
            else:
                assert rows.tobytes() == truth.bytes_off[rank * n : (rank + 1) * n].tobytes(), s
            rank += 1


def slot_of(res, key, kind):
    return next(s for s in range(len(res.slot_key)) if res.slot_key[s] == key and res.slot_kind[s] == kind)


def mask_of(run):
    return int(run.info().implicit_off_slots)


def assert_equal_columns(got, truth):
    for k in COLS:
        assert np.array_equal(np.array(getattr(got, k)), np.array(getattr(truth, k))), k
    assert list(got.info.kind_totals) == list(truth.info.kind_totals)


def c1_input(n=N1, crc=True):
    blob, offs = synth.c1_blob(n, 100, 7)  # (58- and 59-byte records mixed: two shapes)
    buf = synth.frame_blob(blob, offs, crc)
    en = (offs[1:] + 16 * np.arange(1, n + 1)).astype(np.uint64)
    st = np.concatenate([[0], en[:-1]]).astype(np.uint64)
    assert len(set((en - st).tolist())) == 2
    return buf, st, en


@pytest.fixture(scope="module")
def c1():
    return c1_input()


@pytest.fixture(scope="module")
def c1_oracle_off(c1):
    """The oracle's bytes_off column of the C1 input (one bytes slot: record r's element is row r)."""
    r = batch_from_oracle(*c1)
    assert r.bytes_off.shape == (N1,)
    return r.bytes_off


@pytest.fixture(scope="module")
def c1_truth(c1):
    d = new_decoder(c1, optimistic="0")
    yield d
    d.close()


@pytest.fixture(scope="module", params=["2", "0"], ids=["staged", "per_lane"])
def c1_new(request, c1):
    d = new_decoder(c1, stage=request.param)
    yield d
    d.close()


# ------------------------------------------------------------------ 1. fetch and the device view
@pytest.mark.parametrize("mode", ["ends", "u32"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, N1])
def test_c1_fetch_and_device_view(c1, c1_new, c1_truth, c1_oracle_off, n, mode):
    buf, st, en = c1
    truth = Run(c1_truth, buf, st, en, mode, count=n).fetch()
    assert int(truth.info.implicit_cols) == 0 and int(truth.info.implicit_off_slots) == 0
    run = Run(c1_new, buf, st, en, mode, count=n)
    info = run.info()
    sid = slot_of(truth, "id", 1)
    assert int(info.implicit_cols) == 7 and int(info.implicit_off_slots) == 1 << sid and run.reruns() == 0
    run.assert_raw(truth, 1 << sid)  # (not stored: the fetch below has to compute every word)
    got = run.fetch()
    assert got.bytes_off.dtype == np.uint32 and got.bytes_off.tobytes() == truth.bytes_off.tobytes()
    assert got.bytes_off.tobytes() == c1_oracle_off[:n].tobytes()
    assert_equal_columns(got, truth)
    for _ in range(2):  # (the fill runs once per decode: the second view hands out the same column)
        assert run.device_off(n).tobytes() == truth.bytes_off.tobytes()
    assert run.fetch().bytes_off.tobytes() == truth.bytes_off.tobytes()


def test_device_view_before_any_fetch(c1, c1_new, c1_truth):
    buf, st, en = c1
    truth = Run(c1_truth, buf, st, en, "ends").fetch()
    run = Run(c1_new, buf, st, en, "ends")
    assert run.device_off(N1).tobytes() == truth.bytes_off.tobytes()
    assert run.device_off(N1).tobytes() == truth.bytes_off.tobytes()
    assert run.raw_off(N1).tobytes() == truth.bytes_off.tobytes()  # (the view wrote the column itself)
    assert_equal_columns(run.fetch(), truth)


def test_rel_off_accessor(c1, c1_new, c1_truth):
    buf, st, en = c1
    truth = Run(c1_truth, buf, st, en, "ends").fetch()
    delta = C.c_int32(0)
    lib = N.lib()
    assert lib.tfrg_ctx_rel_off(c1_new._ctx, slot_of(truth, "id", 1), C.byref(delta)) == 0
    assert delta.value == -16  # (12 id bytes and the 4-byte data CRC before the record's end)
    assert lib.tfrg_ctx_rel_off(c1_new._ctx, slot_of(truth, "label", 3), C.byref(delta)) != 0
    assert lib.tfrg_ctx_rel_off(c1_new._ctx, 64, C.byref(delta)) != 0


# ------------------------------------------------------------------ 2. consumers that read no column
DENSE_SPECS = [D.Dense("id", "uint8", 12, lengths=True), D.Dense("id", "uint8", 5, lengths=True, name="id5"),
               D.Dense("id", "uint8", 16, fill=0x20, lengths=True, name="id16"), D.Dense("label", "int64", lengths=True)]
RAGGED_SPECS = [R.Ragged("id", "uint8"), R.Ragged("id", "uint8", max_len=5, name="id5"), R.Ragged("label", "int64")]


def _dense_host(got):
    return ({k: v.cpu().numpy().tobytes() for k, v in got.items()},
            {k: v.cpu().numpy().tobytes() for k, v in got.lengths.items()},
            {k: v.tolist() for k, v in got.stats.items()}, got.skipped)


def _ragged_host(got):
    tot = got.totals
    return ({k: (v[: tot[k]].cpu().numpy().tobytes(), o.cpu().numpy().tobytes()) for k, (v, o) in got.items()},
            tot, {k: v.tolist() for k, v in got.stats.items()})


def _consumers(dec, rows):
    import torch

    d_rows = torch.from_numpy(rows).to(torch.device("cuda", 0))
    return (_dense_host(dec.dense(DENSE_SPECS)), _dense_host(dec.dense(DENSE_SPECS, rows=d_rows)),
            _ragged_host(dec.ragged(RAGGED_SPECS, rows=d_rows)), _ragged_host(dec.ragged(RAGGED_SPECS)))


@pytest.mark.parametrize("mode", ["ends", "u32"])
def test_dense_dense_rows_and_ragged_before_any_view(c1, c1_new, c1_truth, mode):
    buf, st, en = c1
    rng = np.random.default_rng(5)
    rows = np.concatenate([rng.permutation(N1)[:700], rng.integers(0, N1, 300), [0, N1 - 1, 0, N1 - 1]]).astype(np.int64)
    assert len(set(rows.tolist())) < rows.size  # (repeats)
    t_run = Run(c1_truth, buf, st, en, mode)
    want = _consumers(c1_truth, rows)
    truth = t_run.fetch()
    run = Run(c1_new, buf, st, en, mode)  # (no info, fetch or view before the consumers: they confirm the decode)
    got = _consumers(c1_new, rows)
    assert got == want
    ids = np.frombuffer(got[0][0]["id"], np.uint8).reshape(N1, 12)
    for i in (0, 63, 64, N1 - 1):  # (and against the writer's bytes: record i holds id 7 + i)
        assert bytes(ids[i]) == b"img-%08d" % (7 + i)
    assert mask_of(run) == 1 << slot_of(truth, "id", 1) and run.reruns() == 0
    run.assert_raw(truth, mask_of(run))  # (poison still: nothing the consumers gave came from the column)
    # the consumers wrote no column: the device view still fills it, and they read the same after it
    assert run.device_off(N1).tobytes() == truth.bytes_off.tobytes()
    assert _consumers(c1_new, rows) == want
    assert_equal_columns(run.fetch(), truth)


# ------------------------------------------------------------------ 3 - 5. decodes that store the column
def test_u64_offsets_store_the_column(c1, c1_new, c1_truth):
    buf, st, en = c1
    truth = Run(c1_truth, buf, st, en, "u64").fetch()
    run = Run(c1_new, buf, st, en, "u64")
    info = run.info()
    assert int(info.implicit_off_slots) == 0 and int(info.implicit_cols) == 7 and run.reruns() == 0
    run.assert_raw(truth, 0)  # (stored by the decode over the poison)
    assert_equal_columns(run.fetch(), truth)
    assert run.device_off(N1).tobytes() == truth.bytes_off.tobytes()


def test_materialized_bytes_store_the_column(c1, c1_new, c1_truth):
    buf, st, en = c1
    truth = Run(c1_truth, buf, st, en, "ends", materialize_bytes=True).fetch()
    run = Run(c1_new, buf, st, en, "ends", materialize_bytes=True)
    info = run.info()
    assert int(info.implicit_off_slots) == 0 and int(info.implicit_cols) == 3 and run.reruns() == 0
    run.assert_raw(truth, 0)
    got = run.fetch()
    assert_equal_columns(got, truth)
    assert got.bytes_data.tobytes() == truth.bytes_data.tobytes()
    assert got.bytes_offsets.tobytes() == truth.bytes_offsets.tobytes()
    assert bytes(got.bytes_data[:12]) == b"img-%08d" % 7


@pytest.mark.parametrize("stage", ["2", "0"])
def test_switch_off_stores_the_column(c1, c1_truth, stage):
    buf, st, en = c1
    truth = Run(c1_truth, buf, st, en, "ends").fetch()
    d = new_decoder(c1, stage=stage, implicit_off="0")
    try:
        run = Run(d, buf, st, en, "ends")
        info = run.info()
        assert int(info.implicit_off_slots) == 0 and int(info.implicit_cols) == 7 and run.reruns() == 0
        run.assert_raw(truth, 0)
        assert run.device_off(N1).tobytes() == truth.bytes_off.tobytes()
        assert_equal_columns(run.fetch(), truth)
    finally:
        d.close()


# ------------------------------------------------------------------ 6. a miss re-runs with every word stored
@pytest.mark.parametrize("mode", ["ends", "u32"])
def test_corrupted_payload_crc_reruns_in_full(c1, c1_new, c1_truth, mode):
    buf, st, en = c1
    bad = buf.copy()
    i = N1 // 2 + 11
    bad[int(en[i]) - 2] ^= 0x40  # (a byte of the stored payload CRC)
    truth = Run(c1_truth, bad, st, en, mode).fetch()
    run = Run(c1_new, bad, st, en, mode)
    info = run.info()
    assert run.reruns() == 1 and int(info.implicit_off_slots) == 0 and int(info.implicit_cols) == 0
    run.assert_raw(truth, 0)  # (the re-run stored every word)
    got = run.fetch()
    assert_equal_columns(got, truth)
    v = np.array(got.verdict)
    assert np.flatnonzero(v != 7).tolist() == [i] and int(v[i]) == 3
    assert run.device_off(N1).tobytes() == truth.bytes_off.tobytes()


# ------------------------------------------------------------------ 7. two-shape inputs of the writer
def _ids(i):
    return f"img-{i:08d}".encode()


def _written(features_of, n=N1, crc=True):
    return synth.framed([writer.encode_example(features_of(i)) for i in range(n)], crc)


def _check_against_truth(sample, modes=("ends", "u32"), **flags):
    """The decode of `sample` on a fresh staged context and on the truth context: equal columns and
    views. Returns (truth result, the masks reported per mode)."""
    buf, st, en = sample
    new, tr = new_decoder(sample, **flags), new_decoder(sample, optimistic="0", **flags)
    masks = []
    try:
        for mode in modes:
            truth = Run(tr, buf, st, en, mode, **flags).fetch()
            run = Run(new, buf, st, en, mode, **flags)
            masks.append(mask_of(run))
            assert run.reruns() == 0 and int(run.info().tpl_groups_missed) == 0
            run.assert_raw(truth, masks[-1])
            nb = int(truth.info.kind_totals[1])
            assert run.device_off(nb).tobytes() == truth.bytes_off.tobytes()
            assert_equal_columns(run.fetch(), truth)
    finally:
        new.close()
        tr.close()
    return truth, masks


def test_label_varint_lengths_with_the_id_last():
    sample = _written(lambda i: [("label", "int64_list", [100 + i % 200]), ("id", "bytes_list", [_ids(i)])])
    assert len(set((sample[2] - sample[1]).tolist())) == 2
    truth, masks = _check_against_truth(sample)
    assert masks == [1 << slot_of(truth, "id", 1)] * 2
    assert truth.bytes_off.tobytes() == batch_from_oracle(*sample).bytes_off.tobytes()


def test_id_before_a_label_of_varying_length():
    sample = _written(lambda i: [("id", "bytes_list", [_ids(i)]), ("label", "int64_list", [100 + i % 200])])
    assert len(set((sample[2] - sample[1]).tolist())) == 2
    truth, masks = _check_against_truth(sample)
    assert masks == [0, 0]
    assert truth.bytes_off.tobytes() == batch_from_oracle(*sample).bytes_off.tobytes()


def test_variable_length_ids():
    blob, offs = synth.c1v_blob(N1, 0, 11)
    buf = synth.frame_blob(blob, offs)
    en = (offs[1:] + 16 * np.arange(1, N1 + 1)).astype(np.uint64)
    st = np.concatenate([[0], en[:-1]]).astype(np.uint64)
    _check_against_truth((buf, st, en))  # (whatever the bit: the id's start moves with its length)


# ------------------------------------------------------------------ 8. the kernel that knows frame classes
@pytest.mark.parametrize("which", ["zero_crc_file", "crc_off_decode"])
def test_frame_class_kernel(c1, which):
    sample = c1_input(crc=False) if which == "zero_crc_file" else c1
    flags = {} if which == "zero_crc_file" else {"crc": False}
    truth, masks = _check_against_truth(sample, **flags)
    assert masks == [1 << slot_of(truth, "id", 1)] * 2  # (the same rule)
    assert (np.array(truth.verdict) == 1).all()


# ------------------------------------------------------------------ 9. two bytes slots
def test_two_bytes_slots_one_end_relative():
    """a (8 bytes) before a label of varying length, b (6 bytes) after it: only b's words are implicit,
    and both columns are right at their own bases (a's rows first, then b's)."""
    sample = _written(lambda i: [("a", "bytes_list", [f"a{i:07d}".encode()]), ("label", "int64_list", [100 + i % 200]),
                                 ("b", "bytes_list", [f"b{i:05d}".encode()])])
    buf, st, en = sample
    truth, masks = _check_against_truth(sample)
    sa, sb = slot_of(truth, "a", 1), slot_of(truth, "b", 1)
    assert masks == [1 << sb] * 2
    orc = batch_from_oracle(*sample)
    assert truth.bytes_off.tobytes() == orc.bytes_off.tobytes()
    base = truth.slot_base
    assert (int(base[sa]), int(base[sb])) == (0, N1)
    for i in (0, 64, N1 - 1):
        oa, ob = int(truth.bytes_off[i]), int(truth.bytes_off[N1 + i])
        assert bytes(buf[oa : oa + 8]) == f"a{i:07d}".encode() and bytes(buf[ob : ob + 6]) == f"b{i:05d}".encode()
    # dense over both slots before any view, against the truth context
    new, tr = new_decoder(sample), new_decoder(sample, optimistic="0")
    try:
        specs = [D.Dense("a", "uint8", 8, lengths=True), D.Dense("b", "uint8", 6, lengths=True)]
        t_run = Run(tr, buf, st, en, "ends")
        want = _dense_host(tr.dense(specs))
        run = Run(new, buf, st, en, "ends")
        assert _dense_host(new.dense(specs)) == want
        assert mask_of(run) == 1 << sb and mask_of(t_run) == 0
        run.assert_raw(truth, 1 << sb)  # (a's rows stored, b's still poison: dense read b from the ends)
        bs = np.frombuffer(want[0]["b"], np.uint8).reshape(N1, 6)
        assert bytes(bs[N1 - 1]) == f"b{N1 - 1:05d}".encode()
    finally:
        new.close()
        tr.close()
