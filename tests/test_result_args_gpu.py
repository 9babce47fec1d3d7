"""The argument checks of the four entry points over a decoded result -- tfrg_result_dense,
tfrg_result_dense_rows, tfrg_result_ragged_rows, tfrg_result_select_rows -- pinned to their exact
return code and ``tfrg_last_error()`` text, and, for a call with two defects, to the one that is
reported (the order of the checks). Every call here is refused before anything is launched: the
buffers keep their poison."""

import ctypes as C

import pytest

from tfr_reader import _native as N
from tfr_reader import hip, synth, writer

pytestmark = pytest.mark.gpu

E_ARG = -1
POISON = 0x5A
S_I, S_F, S_B = 0, 1, 2  # the slots of the three keys, in the order the records name them
KIND = {S_I: 3, S_F: 2, S_B: 1}  # TFRG_KIND_*
ROWS_ERR = "rows_dtype must be TFRG_ROWS_I32 or TFRG_ROWS_I64, not 7"


def vp(p):
    return C.c_void_p(p) if p else None


class Calls:
    """The four entry points on one decoder with valid defaults; every call returns
    (return code, error text)."""

    def __init__(self, dec) -> None:
        import torch

        self.dec, self.lib = dec, N.lib()
        dev = torch.device("cuda", 0)
        self.bufs = {k: torch.full((64,), POISON, dtype=torch.uint8, device=dev)
                     for k in ("out", "rows", "stats", "skipped", "values", "offsets", "totals", "count")}
        self.p = {k: t.data_ptr() for k, t in self.bufs.items()}

    def _done(self, rc: int):
        return rc, self.lib.tfrg_last_error().decode()

    def _dense_specs(self, k: int, kw: dict):
        f = dict(slot=S_I, dtype=N.DENSE_I64, width=1, reserved=0, fill=0, out=self.p["out"], lengths=None)
        f.update(kw)
        return (N.TfrgDenseSpec * max(k, 1))(*[N.TfrgDenseSpec(**f) for _ in range(max(k, 1))])

    def dense(self, k=1, ctx=True, **kw):
        return self._done(self.lib.tfrg_result_dense(self.dec._ctx if ctx else None, self._dense_specs(k, kw), k,
                                                     vp(self.p["stats"]), None))

    def dense_rows(self, k=1, ctx=True, rows=True, rdt=N.ROWS_I64, m=4, **kw):
        return self._done(self.lib.tfrg_result_dense_rows(
            self.dec._ctx if ctx else None, self._dense_specs(k, kw), k, vp(self.p["rows"]) if rows else None, rdt, m,
            0, vp(self.p["stats"]), vp(self.p["skipped"]), None))

    def ragged(self, k=1, ctx=True, rows=True, rdt=N.ROWS_I64, m=4, **kw):
        f = dict(slot=S_I, dtype=N.DENSE_I64, max_len=0, reserved=0, cap=4, values=self.p["values"],
                 offsets=self.p["offsets"])
        f.update(kw)
        arr = (N.TfrgRaggedSpec * max(k, 1))(*[N.TfrgRaggedSpec(**f) for _ in range(max(k, 1))])
        return self._done(self.lib.tfrg_result_ragged_rows(
            self.dec._ctx if ctx else None, arr, k, vp(self.p["rows"]) if rows else None, rdt, m, 0,
            vp(self.p["totals"]), vp(self.p["stats"]), None))

    def select(self, k=1, ctx=True, terms=True, rows=True, rdt=N.ROWS_I64, m=4, out=0, odt=N.ROWS_I64, count=0,
               flags=0, **kw):
        f = dict(slot=S_I, subject=N.SEL_VALUE, op=N.SEL_GE, group=0, index=0, reserved=0, operand=0)
        f.update(kw)
        arr = (N.TfrgSelectTerm * max(k, 1))(*[N.TfrgSelectTerm(**f) for _ in range(max(k, 1))])
        return self._done(self.lib.tfrg_result_select_rows(
            self.dec._ctx if ctx else None, arr if terms else None, k, vp(self.p["rows"]) if rows else None, rdt, m, 0,
            vp(self.p["out"] + out), odt, 4, vp(self.p["count"] + count) if count is not None else None,
            vp(self.p["stats"]), flags, None))

    def untouched(self) -> bool:
        import torch

        torch.cuda.synchronize()
        return all(bool((t == POISON).all()) for t in self.bufs.values())


@pytest.fixture
def calls():
    mp = pytest.MonkeyPatch()
    mp.setenv("TFRG_OPTIMISTIC", "1")  # (read at context creation; the suite may run with 0)
    mp.setenv("TFRG_TEMPLATES", "1")
    try:
        dec = hip.HipDecoder(0)
    finally:
        mp.undo()
    yield Calls(dec)
    dec.close()


def decode4(c: Calls) -> None:
    recs = [writer.encode_example([("a_int", "int64_list", [i]), ("b_float", "float_list", [0.5 * i]),
                                   ("c_bytes", "bytes_list", [b"xy"])]) for i in range(4)]
    res = c.dec.decode(*synth.framed(recs))
    assert res.slot_key == ["a_int", "b_float", "c_bytes"] and list(res.slot_kind) == [KIND[S_I], KIND[S_F], KIND[S_B]]


def test_no_result_before_a_decode(calls):
    c = calls
    assert c.dense() == (E_ARG, "tfrg_result_dense: no result (decode first)")
    assert c.dense_rows() == (E_ARG, "tfrg_result_dense_rows: no result (decode first)")
    assert c.ragged() == (E_ARG, "tfrg_result_ragged_rows: no result (decode first)")
    assert c.select() == (E_ARG, "tfrg_result_select_rows: no result (decode first)")
    # (two defects: the missing result is reported before the count, and before a NULL term table)
    assert c.dense(k=0) == (E_ARG, "tfrg_result_dense: no result (decode first)")
    assert c.dense_rows(k=65) == (E_ARG, "tfrg_result_dense_rows: no result (decode first)")
    assert c.ragged(k=0) == (E_ARG, "tfrg_result_ragged_rows: no result (decode first)")
    assert c.select(k=33) == (E_ARG, "tfrg_result_select_rows: no result (decode first)")
    assert c.select(terms=False) == (E_ARG, "tfrg_result_select_rows: no result (decode first)")
    assert c.untouched()


def test_dense_and_dense_rows_checks(calls):
    c = calls
    decode4(c)
    for fn, call in (("tfrg_result_dense", c.dense), ("tfrg_result_dense_rows", c.dense_rows)):
        def err(why: str, fn=fn):
            return E_ARG, f"{fn}: {why}"

        assert call(k=0) == err("n_specs must be 1..64")
        assert call(k=65) == err("n_specs must be 1..64")
        assert call(slot=3) == err("spec 0: slot 3 >= n_slots")
        assert call(slot=S_I, dtype=N.DENSE_F32) == err("spec 0: dtype 2 does not fit the slot's kind 3")
        assert call(slot=S_I, dtype=N.DENSE_U8) == err("spec 0: dtype 3 does not fit the slot's kind 3")
        assert call(slot=S_I, dtype=4) == err("spec 0: dtype 4 does not fit the slot's kind 3")
        assert call(slot=S_F, dtype=N.DENSE_I64) == err("spec 0: dtype 0 does not fit the slot's kind 2")
        assert call(slot=S_F, dtype=N.DENSE_I32) == err("spec 0: dtype 1 does not fit the slot's kind 2")
        assert call(slot=S_F, dtype=N.DENSE_U8) == err("spec 0: dtype 3 does not fit the slot's kind 2")
        assert call(slot=S_B, dtype=N.DENSE_I64) == err("spec 0: dtype 0 does not fit the slot's kind 1")
        assert call(slot=S_B, dtype=N.DENSE_I32) == err("spec 0: dtype 1 does not fit the slot's kind 1")
        assert call(slot=S_B, dtype=N.DENSE_F32) == err("spec 0: dtype 2 does not fit the slot's kind 1")
        assert call(width=0) == err("spec 0: width must be 1..4096")
        assert call(width=4097) == err("spec 0: width must be 1..4096")
        assert call(out=None) == err("spec 0: out is NULL")
        assert call(reserved=1) == err("spec 0: reserved must be 0")
        # two defects: slot, then dtype, then width, then out, then reserved
        assert call(slot=3, dtype=4, reserved=1) == err("spec 0: slot 3 >= n_slots")
        assert call(dtype=N.DENSE_F32, width=0) == err("spec 0: dtype 2 does not fit the slot's kind 3")
        assert call(width=0, out=None) == err("spec 0: width must be 1..4096")
        assert call(out=None, reserved=1) == err("spec 0: out is NULL")
        assert call(k=2, reserved=1) == err("spec 0: reserved must be 0")  # (the first bad spec)
        assert call(k=65, slot=3) == err("n_specs must be 1..64")
    # the row list of tfrg_result_dense_rows: its dtype is checked whether or not there is a list, and a
    # list of m > 0 rows must be given
    def err(why: str):
        return E_ARG, f"tfrg_result_dense_rows: {why}"

    assert c.dense_rows(rdt=7) == err(ROWS_ERR)
    assert c.dense_rows(rdt=7, rows=False) == err(ROWS_ERR)
    assert c.dense_rows(rdt=7, rows=False, m=0) == err(ROWS_ERR)
    assert c.dense_rows(m=1 << 31) == err("m must be below 2^31")
    assert c.dense_rows(m=1, rows=False) == err("d_rows is NULL")
    # two defects: the specs, then rows_dtype, then m, then d_rows
    assert c.dense_rows(reserved=1, rdt=7) == err("spec 0: reserved must be 0")
    assert c.dense_rows(rdt=7, m=1 << 31) == err(ROWS_ERR)
    assert c.dense_rows(m=1 << 31, rows=False) == err("m must be below 2^31")
    assert c.untouched()


def test_ragged_rows_checks(calls):
    c = calls
    decode4(c)

    def err(why: str):
        return E_ARG, f"tfrg_result_ragged_rows: {why}"

    assert c.ragged(k=0) == err("n_specs must be 1..64")
    assert c.ragged(k=65) == err("n_specs must be 1..64")
    assert c.ragged(slot=3) == err("spec 0: slot 3 >= n_slots")
    assert c.ragged(slot=S_I, dtype=N.DENSE_F32) == err("spec 0: dtype 2 does not fit the slot's kind 3")
    assert c.ragged(slot=S_I, dtype=N.DENSE_U8) == err("spec 0: dtype 3 does not fit the slot's kind 3")
    assert c.ragged(slot=S_I, dtype=4) == err("spec 0: dtype 4 does not fit the slot's kind 3")
    assert c.ragged(slot=S_F, dtype=N.DENSE_I64) == err("spec 0: dtype 0 does not fit the slot's kind 2")
    assert c.ragged(slot=S_F, dtype=N.DENSE_I32) == err("spec 0: dtype 1 does not fit the slot's kind 2")
    assert c.ragged(slot=S_F, dtype=N.DENSE_U8) == err("spec 0: dtype 3 does not fit the slot's kind 2")
    assert c.ragged(slot=S_B, dtype=N.DENSE_I64) == err("spec 0: dtype 0 does not fit the slot's kind 1")
    assert c.ragged(slot=S_B, dtype=N.DENSE_I32) == err("spec 0: dtype 1 does not fit the slot's kind 1")
    assert c.ragged(slot=S_B, dtype=N.DENSE_F32) == err("spec 0: dtype 2 does not fit the slot's kind 1")
    assert c.ragged(offsets=None) == err("spec 0: offsets is NULL")
    assert c.ragged(reserved=1) == err("spec 0: reserved must be 0")
    assert c.ragged(values=c.p["values"] + 4) == err("spec 0: values and offsets must be aligned to their element size")
    assert c.ragged(offsets=c.p["offsets"] + 4) == \
        err("spec 0: values and offsets must be aligned to their element size")
    # the row list: its dtype is checked only when there is a list (NULL: every record in order)
    assert c.ragged(rdt=7) == err(ROWS_ERR)
    assert c.ragged(m=1 << 31) == err("m must be below 2^31")
    assert c.ragged(m=1 << 31, rows=False) == err("m must be below 2^31")
    # two defects: slot, dtype, offsets, reserved, alignment; then the specs, rows_dtype, m
    assert c.ragged(slot=3, dtype=4) == err("spec 0: slot 3 >= n_slots")
    assert c.ragged(dtype=N.DENSE_F32, offsets=None) == err("spec 0: dtype 2 does not fit the slot's kind 3")
    assert c.ragged(offsets=None, reserved=1) == err("spec 0: offsets is NULL")
    assert c.ragged(reserved=1, values=c.p["values"] + 4) == err("spec 0: reserved must be 0")
    assert c.ragged(k=65, slot=3) == err("n_specs must be 1..64")
    assert c.ragged(reserved=1, rdt=7) == err("spec 0: reserved must be 0")
    assert c.ragged(rdt=7, m=1 << 31) == err(ROWS_ERR)
    assert c.ragged(rdt=7, m=1 << 31, rows=False) == err("m must be below 2^31")  # (no list: its dtype is not read)
    assert c.untouched()


def test_select_rows_checks(calls):
    c = calls
    decode4(c)

    def err(why: str):
        return E_ARG, f"tfrg_result_select_rows: {why}"

    assert c.select(k=33) == err("n_terms must be at most 32")
    assert c.select(terms=False) == err("terms is NULL")
    assert c.select(slot=3) == err("term 0: slot 3 >= n_slots")
    assert c.select(subject=5) == err("term 0: unknown subject 5")
    assert c.select(op=6) == err("term 0: unknown op 6")
    assert c.select(group=32) == err("term 0: group must be below 32")
    assert c.select(slot=S_B, subject=N.SEL_VALUE) == err("term 0: subject 0 does not fit slot 2 of kind 1")
    assert c.select(slot=S_B, subject=N.SEL_ANY) == err("term 0: subject 1 does not fit slot 2 of kind 1")
    assert c.select(slot=S_I, subject=N.SEL_BYTES_LEN) == err("term 0: subject 3 does not fit slot 0 of kind 3")
    assert c.select(slot=S_F, subject=N.SEL_BYTES_LEN) == err("term 0: subject 3 does not fit slot 1 of kind 2")
    assert c.select(slot=S_F, subject=N.SEL_STATUS) == err("term 0: subject 4 does not fit slot 1 of kind 2")
    assert c.select(subject=N.SEL_ANY, index=1) == err("term 0: index must be 0 outside TFRG_SEL_VALUE")
    assert c.select(reserved=1) == err("term 0: reserved must be 0")
    assert c.select(slot=S_F, operand=1 << 32) == err("term 0: a float operand has its high 32 bits set")
    # the candidates: their dtype is checked only when there is a list (NULL: every record in order)
    assert c.select(rdt=7) == err(ROWS_ERR)
    assert c.select(odt=7) == err("out_dtype must be TFRG_ROWS_I32 or TFRG_ROWS_I64, not 7")
    assert c.select(m=1 << 31) == err("m must be below 2^31")
    assert c.select(m=1 << 31, rows=False) == err("m must be below 2^31")
    assert c.select(count=None) == err("d_count is NULL")
    assert c.select(out=4) == err("d_out and d_count must be aligned to their element size")
    assert c.select(out=2, odt=N.ROWS_I32) == err("d_out and d_count must be aligned to their element size")
    assert c.select(count=4) == err("d_out and d_count must be aligned to their element size")
    assert c.select(flags=2) == err("unknown flag bits")
    # two defects: within a term slot, subject, op, group, fit, index, reserved; then the terms,
    # rows_dtype, out_dtype, m, d_count, alignment, flags
    assert c.select(k=33, slot=3) == err("n_terms must be at most 32")
    assert c.select(slot=3, subject=5) == err("term 0: slot 3 >= n_slots")
    assert c.select(subject=5, op=6) == err("term 0: unknown subject 5")
    assert c.select(op=6, group=32) == err("term 0: unknown op 6")
    assert c.select(group=32, slot=S_B) == err("term 0: group must be below 32")
    assert c.select(slot=S_B, subject=N.SEL_ANY, index=1) == err("term 0: subject 1 does not fit slot 2 of kind 1")
    assert c.select(subject=N.SEL_COUNT, index=1, reserved=1) == err("term 0: index must be 0 outside TFRG_SEL_VALUE")
    assert c.select(slot=S_F, reserved=1, operand=1 << 32) == err("term 0: reserved must be 0")
    assert c.select(reserved=1, rdt=7) == err("term 0: reserved must be 0")
    assert c.select(rdt=7, odt=7) == err(ROWS_ERR)
    assert c.select(rdt=7, odt=7, rows=False) == err("out_dtype must be TFRG_ROWS_I32 or TFRG_ROWS_I64, not 7")
    assert c.select(odt=7, m=1 << 31) == err("out_dtype must be TFRG_ROWS_I32 or TFRG_ROWS_I64, not 7")
    assert c.select(m=1 << 31, count=None) == err("m must be below 2^31")
    assert c.select(count=None, out=4) == err("d_count is NULL")
    assert c.select(out=4, flags=2) == err("d_out and d_count must be aligned to their element size")
    assert c.untouched()
