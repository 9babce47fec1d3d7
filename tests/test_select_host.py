"""Filtered row lists on the host (no GPU): ``BatchResult.select`` / ``selectify`` -- the numpy
reference the device path (tfrg_result_select_rows) is tested against -- must select exactly the
candidates whose record satisfies the predicate evaluated in plain Python over the ORACLE's value
lists; what ``Term`` / ``where`` refuse; and the C-ABI's argument check without a context. Every
predicate that is not an "all" or "none" case selects some candidates and not all of them."""

import ctypes as C
import math
import operator

import numpy as np
import pytest

from tests import _columns
from tests.test_dense_rows_host import mixed, row_lists
from tests.test_ragged_host import oracle_rows
from tfr_reader import _native as N
from tfr_reader import select as S
from tfr_reader import synth
from tfr_reader.select import Status, Term, is_in

PY = {"==": operator.eq, "!=": operator.ne, "<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge}
KINDS = {"int64": "int64_list", "int32": "int64_list", "float32": "float_list", "uint8": "bytes_list"}
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def values_of(rec: dict, key: str, dtype: str) -> list:
    """The oracle's list of a record (floats as Python floats of their float32 bits)."""
    vals = rec.get((key, KINDS[dtype]), [])
    if dtype == "float32":
        return [float(x) for x in np.array(vals, np.uint32).view(np.float32)]
    return list(vals)


def py_term(rec: dict, t) -> bool:
    """One term for one record, from the specification's words."""
    if isinstance(t, Status):
        return PY[t.op](0, t.operand)  # (every oracle record here decoded)
    vals = values_of(rec, t.key, t.dtype)
    cmp = PY[t.op]
    if t.subject == "count":
        return cmp(len(vals), t.operand)
    if t.subject == "bytes_len":
        return cmp(len(bytes(vals[0])) if vals else 0, t.operand)
    rhs = float(np.float32(t.operand)) if t.dtype == "float32" else t.operand
    if t.subject == "value":
        return len(vals) > t.index and cmp(vals[t.index], rhs)
    return any(cmp(v, rhs) for v in vals)


def py_select(recs: list[dict], where, rows=None, row0: int = 0):
    groups = [g if isinstance(g, list) else [g] for g in where]
    n = len(recs)
    entries = list(range(n)) if rows is None else [int(v) for v in np.asarray(rows, object).reshape(-1)]
    got, skipped = [], 0
    for v in entries:
        if not row0 <= v < row0 + n:
            skipped += 1
        elif all(any(py_term(recs[v - row0], t) for t in g) for g in groups):
            got.append(v)
    return got, (len(got), skipped)


def check(res, recs, where, rows=None, row0: int = 0, kind: str = "some"):
    want, wstats = py_select(recs, where, rows, row0)
    cands = len(recs) if rows is None else len(rows)
    if kind == "some":
        assert 0 < wstats[0] < cands - wstats[1], (where, wstats, cands)
    elif kind == "all":
        assert wstats[0] == cands - wstats[1] > 0
    elif kind == "none":
        assert wstats[0] == 0 and cands > 0
    got, stats = res.select(where, rows=rows, row0=row0)
    assert got.dtype == np.int64 and got.tolist() == want and tuple(stats) == wstats, where
    return got


@pytest.fixture(scope="module")
def c1():
    fr = synth.framed(synth.c1_payloads(200))
    return _columns.batch_from_oracle(*fr), oracle_rows(*fr)


C1_WHERES = [[Term("label", "int64", op, 77)] for op in PY] + [
    [Term("label", "int64", ">=", 10), Term("label", "int64", "<", 20)],
    [is_in("label", "int64", [1, 3, 150])],
    [[Term("label", "int64", "<", 5), Term("label", "int32", ">", 190)], Term("id", "uint8", "==", 12, "bytes_len")],
]


def test_c1_predicates_and_row_lists(c1):
    res, recs = c1
    for where in C1_WHERES:
        check(res, recs, where)
    for r in row_lists(200):
        check(res, recs, [Term("label", "int64", "<", 100)], r, kind="some" if len(r) > 5 else ("none" if len(r) else "empty"))
    check(res, recs, [Term("id", "uint8", "==", 12, "bytes_len")], kind="all")
    check(res, recs, [Term("id", "uint8", "!=", 12, "bytes_len")], kind="none")
    check(res, recs, [Term("label", "int64", "==", 1, "count"), Status("==", 0)], kind="all")
    check(res, recs, [Status("!=", 0)], kind="none")
    check(res, recs, [], kind="all")
    check(res, recs, [[]], kind="none")  # an empty OR group holds no true term
    # candidates out of range are skipped and counted, with and without a row0
    rows = [0, 200, -1, 15, I64_MAX, I64_MIN, 15, 199]
    got = check(res, recs, [Term("label", "int64", ">=", 15)], rows)
    assert got.tolist() == [15, 15, 199]
    row0 = 1 << 40
    rows = [row0 + 3, 3, row0 + 200, row0 - 1, row0 + 150, row0]
    got = check(res, recs, [Term("label", "int64", ">", 2)], rows, row0)
    assert got.tolist() == [row0 + 3, row0 + 150]
    check(res, recs, [Term("label", "int64", "<", 50)], [-3 + k for k in range(120)], -3)


def test_mixed_absent_keys_empty_lists_and_two_kinds():
    n = 600
    fr = synth.framed(mixed(n))
    res, recs = _columns.batch_from_oracle(*fr), oracle_rows(*fr)
    check(res, recs, [Term("half", "int64", "<", 0, index=1)])
    check(res, recs, [Term("empty", "float32", "==", 3.5, index=2)])
    check(res, recs, [Term("two", "int64", "==", 7)])
    check(res, recs, [Term("two", "float32", "==", 0.25)])
    check(res, recs, [[Term("two", "float32", "<", 1.0, "any"), Term("half", "int64", ">", 300, "any")]])
    for c in (0, 1, 2):
        check(res, recs, [Term("names", "uint8", "==", c, "count")])
    check(res, recs, [Term("names", "uint8", ">=", 4, "bytes_len")])
    check(res, recs, [Term("names", "uint8", "==", 0, "bytes_len")])
    # NE on a missing value is false: only the records that have the value can pass
    got = check(res, recs, [Term("half", "int64", "!=", 5)])
    assert all(g % 2 for g in got.tolist()) and 5 not in got.tolist()
    # an absent key: value / any are false, count / bytes_len compare 0
    for op in PY:
        check(res, recs, [Term("absent", "int64", op, 0)], kind="none")
        check(res, recs, [Term("absent", "float32", op, 0.0, "any")], kind="none")
        check(res, recs, [Term("absent", "int64", op, 0, "count")], kind="all" if PY[op](0, 0) else "none")
        check(res, recs, [Term("absent", "uint8", op, 0, "bytes_len")], kind="all" if PY[op](0, 0) else "none")
    check(res, recs, [[Term("absent", "int64", "==", 0), Term("half", "int64", ">", 100)]])
    for r in row_lists(n)[:3]:
        check(res, recs, [Term("half", "int64", ">", 300)], r, kind="some" if len(r) > 5 else "all")


def test_c3_any_and_late_values():
    fr = synth.framed(synth.c3_payloads(96))
    res, recs = _columns.batch_from_oracle(*fr), oracle_rows(*fr)
    check(res, recs, [Term("i0", "int64", "<", 0, "any")])
    check(res, recs, [Term("f0", "float32", ">", 2.0, "any")])
    check(res, recs, [[Term(f"i{j}", "int64", ">=", 0, index=63) for j in range(32)]])
    check(res, recs, [Term("f1", "float32", "<", 0.0, index=40)])
    check(res, recs, [Term(f"i{j}", "int64", ">", 1, "count") for j in range(32)])
    check(res, recs, [[Term(f"f{j}", "float32", "==", 0, "count") for j in range(32)]])
    for r in row_lists(96)[:3]:
        check(res, recs, [Term("i0", "int64", "<", 0, "any")], r, kind="some" if len(r) > 5 else "all")


def test_float_compares_are_on_values():
    """The reference's own float rules, on columns written by hand: NaN, signed zeros, denormals."""
    den = float(np.array(1, np.uint32).view(np.float32))
    vals = np.array([math.nan, 0.0, -0.0, math.inf, -math.inf, den, -den, 1.5, -1.5], np.float32)
    n = len(vals)
    cols = dict(n=n, slot_key=["x"], slot_kind=[2], row_splits=np.arange(n + 1, dtype=np.uint32)[None, :],
                slot_base=np.zeros(1, np.uint64), i64=np.zeros(0, np.int64), f32=vals.view(np.uint32),
                status=np.zeros(n, np.int32))
    for rhs in vals.tolist():
        for op in PY:
            got, _ = S.selectify([Term("x", "float32", op, rhs)], **cols)
            want = [g for g, v in enumerate(vals.tolist()) if PY[op](v, rhs)]
            assert got.tolist() == want, (op, rhs)
    assert S.selectify([Term("x", "float32", "==", 0.0)], **cols)[0].tolist() == [1, 2]
    assert S.selectify([Term("x", "float32", ">", 0.0)], **cols)[0].tolist() == [3, 5, 7]
    assert S.selectify([Term("x", "float32", "!=", math.nan)], **cols)[0].tolist() == list(range(n))
    assert S.selectify([Term("x", "float32", "==", math.nan)], **cols)[0].tolist() == []


def test_term_and_where_validation():
    for bad in (dict(dtype="int16"), dict(op="=<"), dict(subject="all"), dict(operand=1.5), dict(operand=1 << 63),
                dict(operand=True), dict(index=-1), dict(index=1 << 32), dict(subject="any", index=1),
                dict(subject="count", index=2), dict(subject="bytes_len"), dict(dtype="uint8"),
                dict(dtype="uint8", subject="any"), dict(key=b"label"), dict(operand="7"), dict(operand=None)):
        kw = dict(key="label", dtype="int64", op="==", operand=7)
        kw.update(bad)
        with pytest.raises((ValueError, TypeError)):
            Term(**kw)
    with pytest.raises(TypeError):
        Term("w", "float32", "<", "1.0")
    assert Term("w", "float32", "<", 1).operand_bits == 0x3F800000
    assert Term("x", "int64", "<", -1).operand_bits == (1 << 64) - 1
    assert Term("x", "int32", "<", I64_MIN).operand_bits == 1 << 63
    for bad in (dict(op="~"), dict(operand=0.5), dict(operand=1 << 64)):
        kw = dict(op="==", operand=0)
        kw.update(bad)
        with pytest.raises((ValueError, TypeError)):
            Status(**kw)
    t = Term("label", "int64", "==", 1)
    assert S.check_where([t, [t, Status("==", 0)]]) == [[t], [t, Status("==", 0)]]
    assert S.check_where([]) == []
    for bad in (t, "label", [["label"]], [3], [[t, [t]]], None):
        with pytest.raises(TypeError):
            S.check_where(bad)
    with pytest.raises(ValueError, match="32 groups"):
        S.check_where([t] * 33)
    with pytest.raises(ValueError, match="32 terms"):
        S.check_where([[t] * 33])
    assert len(S.check_where([[t] * 32])) == 1 and len(S.check_where([t] * 32)) == 32
    assert [x.operand for x in is_in("label", "int64", [1, 3])] == [1, 3]


def test_result_select_rows_without_a_context_is_an_argument_error():
    lib = N.lib()
    term = N.TfrgSelectTerm(slot=0, subject=N.SEL_VALUE, op=N.SEL_EQ, group=0, index=0, reserved=0, operand=1)
    rc = lib.tfrg_result_select_rows(None, C.byref(term), 1, None, N.ROWS_I64, 1, 0, C.c_void_p(16), N.ROWS_I64, 1,
                                     C.c_void_p(16), None, 0, None)
    assert rc == -1
    assert lib.tfrg_last_error().startswith(b"tfrg_result_select_rows: ")
    assert lib.tfrg_ctx_set_select_tile(None, 64) == -1
    assert (N.SEL_VALUE, N.SEL_ANY, N.SEL_COUNT, N.SEL_BYTES_LEN, N.SEL_STATUS) == (0, 1, 2, 3, 4)
    assert (N.SEL_EQ, N.SEL_NE, N.SEL_LT, N.SEL_LE, N.SEL_GT, N.SEL_GE) == (0, 1, 2, 3, 4, 5)


def test_no_context_is_reported_first_and_in_the_same_words_by_every_result_entry_point():
    """The exact text, and that a missing context is reported before any other defect of the call
    (a count of 0, a NULL spec table); tests/test_result_args_gpu.py pins the checks that need a
    context."""
    lib = N.lib()
    dense = N.TfrgDenseSpec(slot=0, dtype=N.DENSE_I64, width=1, reserved=0, fill=0, out=16, lengths=None)
    ragged = N.TfrgRaggedSpec(slot=0, dtype=N.DENSE_I64, max_len=0, reserved=0, cap=0, values=None, offsets=16)
    term = N.TfrgSelectTerm(slot=0, subject=N.SEL_VALUE, op=N.SEL_EQ, group=0, index=0, reserved=0, operand=1)
    for n, d, r, t in ((1, C.byref(dense), C.byref(ragged), C.byref(term)), (0, None, None, None)):
        assert lib.tfrg_result_dense(None, d, n, None, None) == -1
        assert lib.tfrg_last_error() == b"tfrg_result_dense: no context"
        assert lib.tfrg_result_dense_rows(None, d, n, C.c_void_p(16), 7, 1 << 31, 0, None, None, None) == -1
        assert lib.tfrg_last_error() == b"tfrg_result_dense_rows: no context"
        assert lib.tfrg_result_ragged_rows(None, r, n, C.c_void_p(16), 7, 1 << 31, 0, None, None, None) == -1
        assert lib.tfrg_last_error() == b"tfrg_result_ragged_rows: no context"
        rc = lib.tfrg_result_select_rows(None, t, 33 if n == 0 else 1, C.c_void_p(16), 7, 1 << 31, 0, None, 7, 1, None,
                                         None, 2, None)
        assert rc == -1
        assert lib.tfrg_last_error() == b"tfrg_result_select_rows: no context"
