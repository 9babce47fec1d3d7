"""Two-level ragged outputs on the host (no GPU): ``BatchResult.ragged_elements`` / ``elementify`` -- the
numpy reference the device path (tfrg_result_ragged_elems) is tested against -- must give, for row k,
EVERY element of record ``rows[k]``'s bytes_list as the generator made it and as the oracle decodes it,
element offsets and row offsets that are the cumulative lengths and counts, and the four counters; what
it refuses; and the C-ABI's layout and its argument check without a context. Every comparison is exact."""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _bytes_ref as B
from tests import _columns
from tests._elems_ref import expect
from tests.golden.gen_golden import entry, i64
from tests.test_dense_rows_host import row_lists
from tests.test_ragged_host import oracle_rows
from tfr_reader import _native as N
from tfr_reader import ragged as R
from tfr_reader import synth

HEADER = Path(__file__).resolve().parents[1] / "include" / "tfrg.h"
LENGTHS = [0, 1, 3, 4, 15, 16, 17, 31, 33, 40]
PER_RECORD = [0, 1, 2, 3, 7]


def batch() -> tuple[list[bytes], list[dict]]:
    """Records of 0, 1, 2, 3 and 7 elements (some of 0 bytes) under b"b", every ninth without the key."""
    payloads, items = B.pack(B.random_elems([LENGTHS[i % len(LENGTHS)] for i in range(300)], 21), PER_RECORD)
    for i in range(0, len(payloads), 9):
        payloads[i], items[i] = B.record({}, entry(b"n", i64(i)))
    return payloads, items


@pytest.fixture(scope="module")
def decoded():
    payloads, items = batch()
    fr = synth.framed(payloads)
    return _columns.batch_from_oracle(*fr), items, oracle_rows(*fr)


def specs_all() -> list:
    out = [R.RaggedElements("b"), R.RaggedElements("zz", name="absent")]
    out += [R.RaggedElements("b", max_elems=me, name=f"e{me}") for me in (1, 2, 5)]
    out += [R.RaggedElements("b", max_len=ml, name=f"l{ml}") for ml in (1, 3, 16, 17)]
    out += [R.RaggedElements("b", max_len=ml, max_elems=me, name=f"l{ml}e{me}") for ml, me in ((3, 2), (16, 5), (1, 1))]
    return out


def check(got, items, specs, rows) -> None:
    for sp in specs:
        k = sp.out_name
        want = expect(items, sp, rows)
        values, eo, ro = got[k]
        assert values.dtype == np.uint8 and eo.dtype == np.int64 and ro.dtype == np.int64, k
        assert np.array_equal(ro, want.row_offsets) and np.array_equal(eo, want.elem_offsets), k
        assert np.array_equal(values, want.values), k
        assert got.stats[k].tolist() == want.stats and got.totals[k] == want.totals, k
        assert got.capacity[k] == want.totals and got.overflowed[k] is False, k


def test_rows_hold_the_generators_items(decoded):
    res, items, _ = decoded
    n = len(items)
    counts = {len(it.get("b", [])) for it in items}
    assert counts >= {0, 1, 2, 3, 7} and any("b" not in it for it in items)
    assert any(len(e) == 0 for it in items for e in it.get("b", []))
    specs = specs_all()
    for rows in [None, *row_lists(n)]:
        check(res.ragged_elements(specs, rows=rows), items, specs, rows)
    got = res.ragged_elements([R.RaggedElements("b", max_len=3, max_elems=2)], rows=[4, 4, 0, 1])
    want = expect(items, R.RaggedElements("b", max_len=3, max_elems=2), [4, 4, 0, 1])
    assert got.stats["b"].tolist() == want.stats and want.stats[0] == 2  # a record drawn twice counts twice
    assert R.ELEM_STAT_NAMES == ("rows_truncated", "elems_truncated", "empty", "skipped")


def test_rows_hold_the_oracles_elements(decoded):
    res, _, recs = decoded
    got = res.ragged_elements([R.RaggedElements("b")])
    values, eo, ro = got["b"]
    for g, rec in enumerate(recs):
        vals = rec.get(("b", "bytes_list"), [])
        assert int(ro[g + 1] - ro[g]) == len(vals), g
        for j, v in enumerate(vals):
            e = int(ro[g]) + j
            assert bytes(values[int(eo[e]) : int(eo[e + 1])]) == bytes(v), (g, j)


def test_materialized_source_and_plain_columns(decoded):
    res, items, _ = decoded
    col = B.expected(items, res.slot_key, res.slot_kind, res.slot_base, res.row_splits)  # (the generator's column)
    specs = specs_all()
    rows = row_lists(len(items))[1]
    got = R.elementify(specs, n=len(res), slot_key=res.slot_key, slot_kind=res.slot_kind, row_splits=res.row_splits,
                       slot_base=res.slot_base, bytes_data=col.data, bytes_offsets=col.offsets, rows=rows)
    check(got, items, specs, rows)
    views = R.elementify(specs, n=len(res), slot_key=res.slot_key, slot_kind=res.slot_kind, row_splits=res.row_splits,
                         slot_base=res.slot_base, bytes_off=res.bytes_off, bytes_len=res.bytes_len, buf=res.buf, rows=rows)
    check(views, items, specs, rows)


def test_single_element_lists_agree_with_ragged():
    res = _columns.batch_from_oracle(*synth.framed(synth.c1_payloads(50)))
    rows = [49, 0, 0, 7]
    el = res.ragged_elements([R.RaggedElements("id")], rows=rows)
    rg = res.ragged([R.Ragged("id", "uint8")], rows=rows)
    values, eo, ro = el["id"]
    assert np.array_equal(values, rg["id"][0]) and el.totals["id"] == (4, rg.totals["id"])
    assert np.array_equal(eo[ro[:-1]], rg["id"][1][:-1]) and ro.tolist() == [0, 1, 2, 3, 4]
    assert bytes(values) == b"".join(b"img-%08d" % i for i in rows)


def test_rows_and_specs_that_are_refused(decoded):
    res = decoded[0]
    n = len(res)
    sp = [R.RaggedElements("b")]
    with pytest.raises(IndexError, match=r"rows\[1\] = -1 "):
        res.ragged_elements(sp, rows=[0, -1, n])
    with pytest.raises(IndexError, match=rf"rows\[2\] = {n} "):
        res.ragged_elements(sp, rows=[0, n - 1, n])
    with pytest.raises(ValueError, match="one-dimensional"):
        res.ragged_elements(sp, rows=[[0, 1], [2, 3]])
    empty = res.ragged_elements(sp, rows=[])
    assert empty["b"][0].shape == (0,) and empty["b"][1].tolist() == [0] and empty["b"][2].tolist() == [0]
    for bad in (dict(max_len=0), dict(max_elems=0), dict(max_len=1 << 32), dict(max_elems=-1), dict(max_len=1.5)):
        with pytest.raises(ValueError):
            R.RaggedElements("b", **bad)
    with pytest.raises(TypeError):
        R.RaggedElements(b"b")
    with pytest.raises(ValueError):
        res.ragged_elements([R.RaggedElements("b"), R.RaggedElements("b", max_len=3)])  # (two outputs of one name)
    with pytest.raises(ValueError):
        res.ragged_elements([])
    with pytest.raises(ValueError):
        res.ragged_elements([R.RaggedElements("b", name=str(i)) for i in range(N.ELEMS_MAX_SPECS + 1)])
    with pytest.raises(TypeError):
        res.ragged_elements([R.Ragged("b", "uint8")])


def test_result_ragged_elems_without_a_context_is_an_argument_error():
    lib = N.lib()
    spec = N.TfrgElemsSpec(slot=0, max_elems=0, max_len=0, reserved=0, elem_cap=0, cap=0, values=None, elem_offsets=None,
                           row_offsets=16)
    assert lib.tfrg_result_ragged_elems(None, C.byref(spec), 1, None, N.ROWS_I64, 1, 0, None, None, None) == -1
    assert lib.tfrg_last_error().startswith(b"tfrg_result_ragged_elems: ")


def test_spec_layout_and_limit_match_the_header():
    text = HEADER.read_text()
    assert int(re.search(r"#define TFRG_ELEMS_MAX_SPECS (\d+)", text).group(1)) == N.ELEMS_MAX_SPECS
    body = re.search(r"typedef struct tfrg_elems_spec \{(.*?)\} tfrg_elems_spec;", text, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|uint64_t|uint8_t\*|int64_t\*)\s+(\w+);", body, re.M)
    assert [f for _, f in fields] == [f for f, _ in N.TfrgElemsSpec._fields_]
    at = 0
    for ctype, name in fields:
        size = 4 if ctype == "uint32_t" else 8
        at = (at + size - 1) // size * size
        assert getattr(N.TfrgElemsSpec, name).offset == at and getattr(N.TfrgElemsSpec, name).size == size, name
        at += size
    assert C.sizeof(N.TfrgElemsSpec) == at == 56
