"""Bytes predicates on the device (tfrg_result_select_match: the bytes instantiation of k_sel_eval).
The oracle of every test is Python's own ``bytes`` semantics (``==``, ``<``, ``startswith``,
``endswith``, ``in``) applied to the lists the test wrote into the file (tests/test_select_bytes_host.py
``py_mask``): neither the host path nor the device path has a part in it. Raw calls go over poisoned
outputs (tests/test_select_gpu.py ``run``): the list, the count, the two counters, and nothing written
before ``d_out``, after the stored prefix or past ``cap``. Every case that is not named "all" or "none"
selects, by the oracle alone, at least one candidate and rejects at least one."""

import ctypes as C

import numpy as np
import pytest

from tests import _columns
from tests.test_implicit_off_gpu import Run, c1_input, slot_of
from tests.test_implicit_off_gpu import new_decoder as learned_decoder
from tests.test_select_bytes_host import OPS, mixed_bytes, py_mask
from tests.test_select_gpu import I64_MAX, I64_MIN, dev, new_decoder, run, to_dev
from tfr_reader import _native as N
from tfr_reader import dense as D
from tfr_reader import select as S
from tfr_reader import shard, synth, writer
from tfr_reader.select import BytesTerm, Status, Term, bytes_in

pytestmark = pytest.mark.gpu


def expect(recs, where, rows=None, row0: int = 0, kind: str = "some", failed=()):
    """(entries of the passing candidates, (selected, skipped)) by the oracle; ``kind`` is asserted on it."""
    mask = py_mask(recs, where, failed)
    n = len(recs)
    entries = list(range(n)) if rows is None else [int(v) for v in rows]
    want, skipped = [], 0
    for v in entries:
        if not row0 <= v < row0 + n:
            skipped += 1
        elif mask[v - row0]:
            want.append(v)
    cands = len(entries) - skipped
    if kind == "some":
        assert 0 < len(want) < cands, (where, len(want), cands)
    elif kind == "all":
        assert len(want) == cands > 0, where
    elif kind == "none":
        assert not want and cands > 0, where
    return np.array(want, np.int64), (len(want), skipped)


@pytest.fixture
def dec():
    d = new_decoder()
    yield d
    d.close()


# ------------------------------------------------------------------------------------ 1. every op, both subjects
LENS = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000]
PLENS = [0, 1, 3, 4, 5, 16, 255, 256]
# the patterns are prefixes of BASE (every third byte >= 0x80, the first one too); FILL never holds BASE[0]
BASE = bytes(((i * 37 + 139) % 256) | (0x80 if i % 3 == 0 else 0) for i in range(1000))
FILL = bytes(0x20 + (i * 7) % 0x50 for i in range(1000))
assert BASE[0] >= 0x80 and BASE[0] not in FILL and max(FILL) < 0x80


def op_elements() -> list[bytes]:
    """Elements of every length of LENS: BASE's prefix (equal to the pattern of that length, a proper
    prefix of the longer patterns, an extension of the shorter ones), the same with its last byte's top
    bit flipped (smaller or larger only as unsigned bytes), and for every pattern that fits an element
    that ends with it and one that holds it in the middle."""
    out = []
    for ln in LENS:
        out.append(BASE[:ln])
        if ln:
            out.append(BASE[: ln - 1] + bytes([BASE[ln - 1] ^ 0x80]))
        for k in PLENS:
            if 0 < k <= ln:
                out.append(FILL[: ln - k] + BASE[:k])
            if 0 < k <= ln - 2:
                out.append(FILL[:1] + BASE[:k] + FILL[1 : ln - k])
    assert {len(e) for e in out} == set(LENS)
    return out


def op_records() -> tuple[list[bytes], list[dict]]:
    """Records with 1 and 3 elements over ``op_elements``, with an empty list and without the key, shuffled."""
    el = op_elements()
    # (every element stands first, second and third in some triple)
    triples = [[el[(i + j) % len(el)] for j in range(3)] for i in range(len(el))]
    lists = [[e] for e in el] + triples + [[]] * 8 + [None] * 8
    order = np.random.default_rng(11).permutation(len(lists)).tolist()
    payloads, recs = [], []
    for g, k in enumerate(order):
        rec, feats = {"label": [g]}, [("label", "int64_list", [g])]
        if lists[k] is not None:
            rec["blob"] = list(lists[k])
            feats.append(("blob", "bytes_list", rec["blob"]))
        payloads.append(writer.encode_example(feats))
        recs.append(rec)
    return payloads, recs


@pytest.fixture(scope="module")
def ops_file():
    d = new_decoder()
    payloads, recs = op_records()
    res = d.decode(*synth.framed(payloads))
    assert len(res) == len(recs) <= 4000 and not res.status.any()
    # element starts at every alignment mod 4, for the short and for the long elements
    for lo, hi in ((0, 16), (16, 2000)):
        pick = (res.bytes_len >= lo) & (res.bytes_len < hi)
        assert set((res.bytes_off[pick] % 4).tolist()) == {0, 1, 2, 3}
    assert {len(r.get("blob") or []) for r in recs} == {0, 1, 3}
    yield d, recs
    d.close()


@pytest.mark.parametrize("plen", PLENS)
def test_every_op_and_both_subjects(ops_file, plen):
    d, recs = ops_file
    pattern = BASE[:plen]
    for op in OPS:
        for subject in ("value", "any"):
            # (nothing is smaller than the empty string: the one "none" case)
            kind = "none" if (op == "<" and plen == 0) else "some"
            where = [BytesTerm("blob", op, pattern, subject)]
            run(d, where, *expect(recs, where, kind=kind))
    for index in (1, 2):
        for op in ("==", "!=", "<", ">=", "endswith", "contains"):
            where = [BytesTerm("blob", op, pattern, index=index)]
            want, wstats = expect(recs, where, kind="none" if (op == "<" and plen == 0) else "some")
            run(d, where, want, wstats)
            assert all(len(recs[g]["blob"]) == 3 for g in want.tolist())
    # NE on a record without the element is false, whatever the pattern
    where = [BytesTerm("blob", "!=", (pattern + b"\x00")[-256:], index=1)]
    want, wstats = expect(recs, where)
    assert want.tolist() == [g for g, r in enumerate(recs) if len(r.get("blob") or []) == 3]
    run(d, where, want, wstats)


def test_compare_edges_are_the_ones_python_has(ops_file):
    """What the rules say, spelled out on known elements: unsigned bytes, proper prefixes, last bytes."""
    d, recs = ops_file
    first = {g: r["blob"][0] for g, r in enumerate(recs) if r.get("blob")}

    def rows_of(where):
        want, wstats = expect(recs, where)
        run(d, where, want, wstats)
        return want.tolist()

    p = BASE[:16]
    flipped = p[:15] + bytes([p[15] ^ 0x80])
    assert flipped in first.values() and p in first.values() and BASE[:15] in first.values() and BASE[:17] in first.values()
    lt = rows_of([BytesTerm("blob", "<", p)])
    assert all(first[g] < p for g in lt) and any(first[g] == BASE[:15] for g in lt)  # (a proper prefix is less)
    assert not any(first[g] in (p, BASE[:17]) for g in lt)
    # the flipped last byte sorts by its unsigned value: a signed compare would put it on the other side
    assert (flipped in [first[g] for g in lt]) == (flipped[15] < p[15]) and (flipped[15] >= 0x80) != (p[15] >= 0x80)
    ge = rows_of([BytesTerm("blob", ">=", p)])
    assert sorted(lt + ge) == sorted(first)
    eq = rows_of([BytesTerm("blob", "==", p)])
    assert eq and all(first[g] == p for g in eq)
    # every element that is present starts with, ends with and contains the empty pattern
    for op in ("startswith", "endswith", "contains"):
        assert rows_of([BytesTerm("blob", op, b"")]) == sorted(first)
    assert [first[g] for g in rows_of([BytesTerm("blob", "==", b"")])] == [b""] * len([v for v in first.values() if v == b""])
    assert rows_of([bytes_in("blob", [BASE[:4], BASE[:255], FILL[:1] + BASE[:3], b"nothing"])])


# ------------------------------------------------------------------------------------ 2. the wave scan
SCAN_CHUNK = 2048  # bytes per chunk of the wave scan, from the 16-byte boundary at or before the element


def scan_pattern(ln: int) -> bytes:
    """0xaa, then bytes of 0x80..0xa9: the first byte occurs once, so a pattern cannot overlap itself."""
    return bytes([0xAA]) + bytes(0x80 + (i * 5 + ln) % 0x2A for i in range(1, ln))


SCAN_PLENS = [3, 5, 17, 256]
SCAN_PATTERNS = {ln: scan_pattern(ln) for ln in SCAN_PLENS}


def near(p: bytes) -> bytes:
    """The pattern but for its last byte."""
    return p[:-1] + bytes([p[-1] ^ 1])


def scan_specs() -> list[list[tuple[int, object]]]:
    """Per record a list of elements (length, plant), plant(boundaries) -> [(position, bytes)]: what is
    written over the filler once the element's boundaries (element-relative) are known."""
    recs = []

    def one(ln, plant):
        recs.append([(ln, plant)])

    for L in (3, 5, 17):
        p = SCAN_PATTERNS[L]
        for b in (0, 1):  # both boundaries inside a 4400-byte element, every overlap 0..L
            for j in range(L + 1):
                one(4400, lambda bd, b=b, j=j, p=p: [(bd[b] - j, p)])
                one(4400, lambda bd, b=b, j=j, p=p: [(bd[b] - j, near(p))])
    p = SCAN_PATTERNS[256]
    for j in range(257):
        one(2400, lambda bd, j=j, p=p: [(bd[0] - j, p)])
        if j % 16 == 0 or j > 250:
            one(2400, lambda bd, j=j, p=p: [(bd[0] - j, near(p))])
    for L in SCAN_PLENS:
        p = SCAN_PATTERNS[L]
        for ln in (L, L + 1, 300, SCAN_CHUNK + 40, 2 * SCAN_CHUNK + 300):
            one(ln, lambda bd, p=p: [(0, p)])  # at offset 0
            one(ln, lambda bd, p=p, ln=ln: [(ln - len(p), p)])  # at the very end
            one(ln, lambda bd, p=p, ln=ln: [(ln - len(p), near(p))])
            one(ln, lambda bd: [])
    big = 200 * 1024
    p5 = SCAN_PATTERNS[5]
    one(big, lambda bd: [(big - 5, p5)])  # the only match in its last bytes
    one(big, lambda bd: [(big - 5, near(p5)), (big // 2, p5[:4])])
    # short and tiny elements beside the long ones: the lane's path at the smallest knob, or just above it
    p3 = SCAN_PATTERNS[3]
    for ln in (3, 4, 5, 9, 16, 17):
        for at in (0, ln - 3):
            one(ln, lambda bd, at=at: [(at, p3)])
            one(ln, lambda bd, at=at: [(at, near(p3))])
    one(0, lambda bd: [])
    one(1, lambda bd: [])
    # three elements, the match in the last one only, in the middle one only, in none
    recs.append([(300, lambda bd: []), (5, lambda bd: []), (4400, lambda bd: [(bd[1] - 2, p5)])])
    recs.append([(300, lambda bd: []), (5, lambda bd: [(0, p5)]), (4400, lambda bd: [(bd[0] - 2, near(p5))])])
    recs.append([(4400, lambda bd: [(bd[0] - 3, near(p3))]), (4, lambda bd: []), (2400, lambda bd: [])])
    recs.append([(4400, lambda bd: []), (3, lambda bd: [(0, p3)]), (2400, lambda bd: [(bd[0] - 100, SCAN_PATTERNS[256])])])
    order = np.random.default_rng(12).permutation(len(recs)).tolist()
    return [recs[k] for k in order]


def scan_records() -> tuple[list[bytes], list[dict], np.ndarray]:
    """(payloads, what was written, the elements' byte offsets in the framed file). Two passes: the
    offsets of the elements (the oracle decoder's, on the CPU) do not depend on their contents."""
    specs = scan_specs()
    rng = np.random.default_rng(13)
    fill = [[rng.integers(0, 0x80, ln, dtype=np.uint8).tobytes() for ln, _ in rec] for rec in specs]

    def encode(lists):
        return [writer.encode_example([("blob", "bytes_list", els)]) for els in lists]

    offs = _columns.batch_from_oracle(*synth.framed(encode(fill))).bytes_off.astype(np.int64)
    lists, e = [], 0
    for rec, fl in zip(specs, fill):
        els = []
        for (ln, plant), raw in zip(rec, fl):
            off = int(offs[e])
            first = (off & ~15) + SCAN_CHUNK - off  # the element's first chunk boundary
            buf = bytearray(raw)
            for at, what in plant((first, first + SCAN_CHUNK)):
                assert 0 <= at and at + len(what) <= ln, (ln, at)
                buf[at : at + len(what)] = what
            els.append(bytes(buf))
            e += 1
        lists.append(els)
    assert e == len(offs)
    return encode(lists), [{"blob": els} for els in lists], offs


@pytest.fixture(scope="module")
def scan_file():
    d = new_decoder()
    payloads, recs, offs = scan_records()
    res = d.decode(*synth.framed(payloads))
    assert len(res) == len(recs) <= 4000 and not res.status.any()
    assert np.array_equal(res.bytes_off.astype(np.int64), offs)  # (the boundaries are where the plants assumed)
    yield d, recs
    d.set_select_scan(0)
    d.close()


@pytest.mark.parametrize("knob", [N.SEL_SCAN_MIN, N.SEL_SCAN_MAX, 0], ids=["smallest", "largest", "default"])
def test_contains_by_lane_and_by_wave(scan_file, knob):
    d, recs = scan_file
    assert N.SEL_SCAN_MIN <= 16 and max(len(e) for r in recs for e in r["blob"]) > N.SEL_SCAN_MAX
    d.set_select_scan(knob)
    for L in SCAN_PLENS:
        for subject in ("value", "any"):
            where = [BytesTerm("blob", "contains", SCAN_PATTERNS[L], subject)]
            run(d, where, *expect(recs, where))
    # a near match alone is no match; the 200 KiB element is found by its last bytes alone
    big = [g for g, r in enumerate(recs) if len(r["blob"][0]) == 200 * 1024]
    want, wstats = expect(recs, [BytesTerm("blob", "contains", SCAN_PATTERNS[5])])
    assert len(big) == 2 and len(set(big) & set(want.tolist())) == 1
    rows = big + [g for g in range(len(recs)) if g % 7 == 0] + big
    where = [BytesTerm("blob", "contains", SCAN_PATTERNS[5])]
    run(d, where, *expect(recs, where, rows), rows)
    # the other ops read no more than the pattern's length of these elements, and agree with Python too
    for op in ("startswith", "endswith", "==", ">"):
        where = [BytesTerm("blob", op, SCAN_PATTERNS[17], "any")]
        run(d, where, *expect(recs, where))


def test_the_knob_has_a_range(dec):
    for bad in (1, 3, N.SEL_SCAN_MAX + 1, 1 << 31):
        with pytest.raises(N.NativeError):
            dec.set_select_scan(bad)
    for ok in (N.SEL_SCAN_MIN, 16, 1000, N.SEL_SCAN_MAX, 0):
        dec.set_select_scan(ok)


def test_two_equal_calls_write_equal_bytes(scan_file):
    import torch

    d, recs = scan_file
    d.set_select_scan(N.SEL_SCAN_MIN)
    where = [[BytesTerm("blob", "contains", SCAN_PATTERNS[3], "any"), BytesTerm("blob", "endswith", SCAN_PATTERNS[17])]]
    want, wstats = expect(recs, where)
    a = d.select(where, capacity=len(recs))
    b = d.select(where, capacity=len(recs))
    assert torch.equal(a.rows, b.rows) and a.count == b.count == len(want) and a.stats == b.stats == wstats
    assert a.rows.cpu().tolist() == want.tolist() + [-1] * (len(recs) - len(want))


# ------------------------------------------------------------------------------------ 3. the three byte sources
def test_views_implicit_offsets_and_the_materialized_column_agree():
    buf, st, en = c1 = c1_input()
    n = len(st)
    ids = [b"img-%08d" % (7 + i) for i in range(n)]  # (what c1_input wrote: record i holds id 7 + i)
    recs = [{"id": [v]} for v in ids]
    wheres = [[BytesTerm("id", "==", ids[123])], [bytes_in("id", [ids[0], ids[64], ids[n - 1], b"img-"])],
              [BytesTerm("id", "startswith", b"img-0000010")], [BytesTerm("id", "endswith", b"77")],
              [BytesTerm("id", "contains", b"99", "any")], [BytesTerm("id", ">=", ids[n // 2])],
              [BytesTerm("id", "<", b"img-00001"), BytesTerm("id", "!=", ids[5])]]
    wants = [expect(recs, w) for w in wheres]

    def selections(d):
        return [d.select(w).rows.cpu().tolist() for w in wheres] + [d.select(w, rows=to_dev([n - 1, 5, -1, 123, 123])).stats for w in wheres]

    got = {}
    # the implicit end-relative offsets and the constant length: nothing of bytes_off / bytes_len is read
    d = learned_decoder(c1)
    try:
        r = Run(d, buf, st, en, "ends")
        got["implicit"] = selections(d)
        info = r.info()
        sid = slot_of(r.fetch(), "id", 1)
        assert int(info.implicit_off_slots) == 1 << sid and int(info.implicit_cols) & 4 and r.reruns() == 0
        # the materialized column
        r = Run(d, buf, st, en, "ends", materialize_bytes=True)
        got["materialized"] = selections(d)
        assert int(r.info().implicit_off_slots) == 0 and int(r.info().bytes_data_len) == 12 * n
    finally:
        d.close()
    # the same decode with the offsets stored, and with every column stored
    for name, kw in (("stored offsets", dict(implicit_off="0")), ("stored", dict(optimistic="0"))):
        d = learned_decoder(c1, **kw)
        try:
            r = Run(d, buf, st, en, "ends")
            got[name] = selections(d)
            assert int(r.info().implicit_off_slots) == 0
            assert (int(r.info().implicit_cols) & 4 != 0) == (name == "stored offsets")
        finally:
            d.close()
    for name, sel in got.items():
        assert sel == got["implicit"], name
        assert sel[: len(wheres)] == [w.tolist() for w, _ in wants], name


# ------------------------------------------------------------------------------------ 4. the end of the buffer
@pytest.mark.parametrize("tail_len", [9, 300, 5000])
@pytest.mark.parametrize("rem", [1, 7, 15])
def test_the_last_element_ends_where_the_buffer_ends(dec, rem, tail_len):
    """Bare payloads whose bytes feature comes last: the last record's element ends at nbytes, and
    nbytes is no multiple of 16. Its last bytes decide every verdict here."""
    p = SCAN_PATTERNS[5]
    rng = np.random.default_rng(rem)
    lists = [[rng.integers(0, 0x80, 20 + g, dtype=np.uint8).tobytes()] for g in range(70)]
    lists[3] = [lists[3][0][:-5] + p]
    lists.append([rng.integers(0, 0x80, tail_len - 5, dtype=np.uint8).tobytes() + p])

    def encode():
        return [writer.encode_example([("blob", "bytes_list", els)]) for els in lists]

    lists[0] = [lists[0][0] + b"\x01" * ((rem - sum(len(x) for x in encode())) % 16)]
    payloads = encode()
    buf = np.frombuffer(b"".join(payloads), np.uint8)
    en = np.cumsum([len(x) for x in payloads]).astype(np.uint64)
    st = np.concatenate([[0], en[:-1]]).astype(np.uint64)
    assert buf.size % 16 == rem and payloads[-1].endswith(p)
    res = dec.decode(buf, st, en, payload_only=True)
    assert not res.status.any() and int(res.bytes_off[-1]) + int(res.bytes_len[-1]) == buf.size
    recs = [{"blob": els} for els in lists]
    last, tail = len(recs) - 1, lists[-1][0]
    for knob in (N.SEL_SCAN_MIN, 0):
        dec.set_select_scan(knob)
        short = tail_len <= 256
        for where, kind, has_last in (
                ([BytesTerm("blob", "endswith", p)], "some", True), ([BytesTerm("blob", "contains", p)], "some", True),
                ([BytesTerm("blob", "endswith", near(p))], "none", False), ([BytesTerm("blob", "contains", near(p))], "none", False),
                ([BytesTerm("blob", "==", tail[-256:])], "some" if short else "none", short),
                ([BytesTerm("blob", "endswith", tail[-256:])], "some", True),
                ([BytesTerm("blob", ">", b"\x40")], "some", tail > b"\x40"),
                ([BytesTerm("blob", "<=", tail[:256])], "some", short)):
            want, wstats = expect(recs, where, kind=kind)
            run(dec, where, want, wstats)
            assert (last in want.tolist()) == has_last, where


# ------------------------------------------------------------------------------------ 5. candidates
def test_candidate_lists_row0_dtypes_and_small_tiles(ops_file):
    d, recs = ops_file
    n = len(recs)
    rng = np.random.default_rng(5)
    bad64 = [-1, n, n + 1, (1 << 31) - 1, I64_MIN, I64_MAX, -n, 1 << 32, (1 << 32) + 5]
    bad32 = [-1, n, n + 1, (1 << 31) - 1, -(1 << 31), -n]
    wheres = [[BytesTerm("blob", "contains", BASE[:4], "any")], [BytesTerm("blob", "<", BASE[:16])],
              [BytesTerm("blob", "endswith", BASE[:255], "any")]]
    d.set_select_tile(64)
    try:
        assert n > 3 * 64  # (several tiles)
        for j, where in enumerate(wheres):
            for i, (rows, rdt) in enumerate([(rng.permutation(n), np.int64), (rng.integers(0, n, 2 * n + 3), np.int32),
                                             ([bad64[k % 9] if k % 3 == 1 else (5 * k) % n for k in range(400)], np.int64),
                                             ([bad32[k % 6] if k % 3 == 1 else (7 * k) % n for k in range(400)], np.int32)]):
                odt = N.ROWS_I32 if (i + j) % 2 else N.ROWS_I64
                run(d, where, *expect(recs, where, rows), rows, rdt, odt=odt)
            run(d, where, *expect(recs, where, list(range(n + 70))), None, m=n + 70)  # (rows NULL, m above n)
            row0 = 1 << 40
            rows = [row0 + (7 * k) % n for k in range(500)]
            rows[3], rows[10], rows[11], rows[40] = row0 - 1, row0 + n, 5, I64_MIN
            run(d, where, *expect(recs, where, rows, row0), rows, np.int64, row0)
            rows = [-3 + k for k in range(n + 9)]
            run(d, where, *expect(recs, where, rows, -3), rows, np.int32, -3, odt=N.ROWS_I32)
        # every candidate out of range; capacities below the count, the count alone, appending
        where = wheres[0]
        assert expect(recs, where, bad64, kind=None)[1] == (0, len(bad64))
        run(d, where, *expect(recs, where, bad64, kind=None), bad64)
        want, wstats = expect(recs, where)
        for cap in (len(want), len(want) - 1, 1, 0):
            run(d, where, want, wstats, cap=cap)
        run(d, where, want, wstats, null_out=True)
        run(d, where, want, wstats, base=17)
        run(d, where, want, wstats, base=17, cap=17 + len(want) - 5)
    finally:
        d.set_select_tile(0)


@pytest.fixture(scope="module")
def sharded():
    """Three C1 files decoded by a ShardDecoder in at least 3 batches on 2 streams (the method of
    tests/test_select_gpu.py): (decoder, plan, the ids that were written)."""
    import torch

    base = 1200
    imgs = [synth.c4_file(f, "c1", base=base) for f in range(3)]
    counts = synth.c4_counts(3, base).tolist()
    ids = [b"img-%08d" % ((f * 1_000_003 + i) % 10**8) for f in range(3) for i in range(counts[f])]
    sb = shard.ShardBatch([synth.c4_file_name(f) for f in range(3)], imgs)
    assert len(sb.starts) == len(ids) <= 6000
    sd = shard.ShardDecoder(0, batch_bytes=sb.nbytes // 3 + 4096, n_streams=2)
    plan = sd.plan(sb.starts, sb.ends, sb.nbytes)
    assert len(plan) >= 3
    d_bytes = torch.zeros(((sb.nbytes + 15) // 16) * 16 + 16, dtype=torch.uint8, device=dev())
    d_bytes[: sb.nbytes].copy_(torch.from_numpy(sb.buf))
    rst, ren, firsts = sd.rebase32(plan, sb.starts, sb.ends)
    assert rst is None
    d_en = torch.from_numpy(ren.view(np.int32)).to(dev())
    sd.learn(plan, sb.buf, sb.starts, sb.ends)
    streams = [torch.cuda.Stream(dev()), torch.cuda.Stream(dev())]
    torch.cuda.synchronize(dev())
    sd.decode_device32(plan, d_bytes.data_ptr(), None, d_en.data_ptr(), firsts, streams=[s.cuda_stream for s in streams])
    yield sd, plan, ids, (d_bytes, d_en, streams)
    sd.close()


def test_select_appends_across_the_contexts_of_a_plan(sharded):
    sd, plan, ids, _ = sharded
    n = len(ids)
    assert int(plan[-1, 1]) == n
    recs = [{"id": [v]} for v in ids]
    for where in ([BytesTerm("id", "endswith", b"7")], [bytes_in("id", [ids[3], ids[n // 2], ids[n - 1], b"img-nobody"])],
                  [BytesTerm("id", "contains", b"0031", "any"), BytesTerm("id", ">", ids[n // 3])]):
        want, wstats = expect(recs, where)
        sel = sd.select(plan, where)
        assert sel.rows.cpu().tolist() == want.tolist() and sel.count == len(want) and sel.stats == wstats
    # the contexts append in plan order: with a list that crosses the batches, each its own part
    where = [BytesTerm("id", "endswith", b"7")]
    want, _ = expect(recs, where)
    assert want[0] < plan[1, 0] <= plan[2, 0] <= want[-1]  # (rows of every batch)
    rows = np.random.default_rng(8).integers(0, n, 3000).tolist()
    for k, v in zip((1, 2, 500, 2999), (-1, n, I64_MAX, I64_MIN)):
        rows[k] = v
    want, wstats = expect(recs, where, rows)
    got = sd.select(plan, where, rows=to_dev(rows), dtype="int32")
    parts = [[v for v in want.tolist() if r0 <= v < r1] for r0, r1, _, _ in plan.tolist()]
    assert got.rows.cpu().tolist() == [v for p in parts for v in p] and got.stats == wstats and wstats[1] == 4
    # an overflowing capacity keeps the prefix and the whole count
    want, _ = expect(recs, where)
    short = sd.select(plan, where, capacity=len(want) - 3)
    assert short.overflowed and short.count == len(want) and short.rows.cpu().tolist() == want.tolist()[:-3]


# ------------------------------------------------------------------------------------ 6. failed records, mixed terms
def test_failed_records_have_no_bytes(dec):
    n = 300
    payloads = synth.c1_payloads(n)
    bad = [5, 64, 65, 299]
    for g in bad:
        payloads[g] = b"\xff" * 10
    res = dec.decode(*synth.framed(payloads))
    assert np.flatnonzero(res.status).tolist() == bad
    recs = [{"id": [b"img-%08d" % i], "label": [i % 1000]} for i in range(n)]
    good = [g for g in range(n) if g not in bad]
    for where in ([BytesTerm("id", "!=", b"zzz")], [BytesTerm("id", ">=", b"", "any")], [BytesTerm("id", "startswith", b"")],
                  [BytesTerm("id", "contains", b"")]):
        want, wstats = expect(recs, where, failed=bad)
        assert want.tolist() == good
        run(dec, where, want, wstats)
    where = [[BytesTerm("id", "startswith", b"img-000000"), Status("!=", 0)]]
    want, wstats = expect(recs, where, failed=bad)
    assert want.tolist() == sorted(set(range(100)) | set(bad))
    run(dec, where, want, wstats)


def test_bytes_and_integer_terms_in_one_where(dec):
    payloads, recs = mixed_bytes(600)
    res = dec.decode(*synth.framed(payloads))
    assert not res.status.any()
    rows = np.random.default_rng(6).integers(-2, 602, 900)
    for where in ([BytesTerm("names", "contains", b"cat", "any"), Term("label", "int64", "<", 400)],
                  [[BytesTerm("names", "endswith", b"cat"), Term("label", "int64", ">=", 550)], Status("==", 0)],
                  [Term("names", "uint8", "==", 3, "count"), BytesTerm("names", "<", b"cat", index=2)],
                  [Term("names", "uint8", ">=", 5, "bytes_len"), BytesTerm("names", "startswith", "c")],
                  [bytes_in("names", [b"cat", b"", b"\xff"]), Term("label", "int32", ">", 100)],
                  [[BytesTerm("absent", "==", b"cat"), BytesTerm("names", "==", b"cat")]]):
        run(dec, where, *expect(recs, where))
        want, wstats = expect(recs, where, rows)
        run(dec, where, want, wstats, rows, np.int32, odt=N.ROWS_I32)
        sel = dec.select(where, rows=to_dev(rows))
        assert sel.rows.cpu().tolist() == want.tolist() and sel.stats == wstats
        # the host path computes the same function
        got, stats = res.select(where, rows=rows)
        assert got.tolist() == want.tolist() and tuple(stats) == wstats
    # a where that nothing can pass is not launched
    assert S.fold(dec, S.check_where([BytesTerm("absent", "contains", b"")])) is None
    sel = dec.select([BytesTerm("absent", "contains", b"")])
    assert sel.rows.numel() == 0 and sel.count == 0 and sel.stats == (0, 0)


def test_minibatches_over_the_records_a_bytes_term_selects(dec):
    n = 1500
    dec.decode(*synth.framed(synth.c1_payloads(n)))
    recs = [{"id": [b"img-%08d" % i]} for i in range(n)]
    where = [BytesTerm("id", "startswith", b"img-000001"), BytesTerm("id", "!=", b"img-00000150")]
    chosen = expect(recs, where)[0].tolist()
    assert chosen == [i for i in range(100, 200) if i != 150]
    specs = [D.Dense("id", "uint8", 12), D.Dense("label", "int64")]
    drawn = []
    for b in dec.minibatches(specs, 32, seed=3, where=where):
        drawn += [int(bytes(x)[4:]) for x in b["id"].cpu().numpy()]
        assert b.skipped == 0
    assert sorted(drawn) == chosen and drawn != chosen
    assert list(dec.minibatches(specs, 32, where=[BytesTerm("id", "==", b"img-")])) == []


# ------------------------------------------------------------------------------------ 7. the C level
def test_c_level_argument_errors(dec):
    import torch

    lib = N.lib()
    out = torch.full((64,), -1, dtype=torch.int64, device=dev())
    cnt = torch.full((2,), -1, dtype=torch.int64, device=dev())
    st = torch.full((2,), 77, dtype=torch.int32, device=dev())
    d_rows = to_dev([0, 1, 2])
    blob = b"img-00000001" + bytes(2036)
    assert len(blob) == N.SEL_MAX_PATTERN_BYTES

    def call(fn="tfrg_result_select_match", k=1, patterns=blob, plen=None, rows_ptr=d_rows.data_ptr(), rdt=N.ROWS_I64, m=3,
             row0=0, out_ptr=out.data_ptr(), odt=N.ROWS_I64, cap=64, cnt_ptr=cnt.data_ptr(), flags=0, **kw):
        f = dict(slot=0, subject=N.SEL_BYTES, op=N.SEL_EQ, group=0, index=0, reserved=0, operand=S.pack_pattern(0, 12))
        f.update(kw)
        arr = (N.TfrgSelectTerm * max(k, 1))(*[N.TfrgSelectTerm(**f) for _ in range(max(k, 1))])
        tail = (C.c_void_p(rows_ptr) if rows_ptr else None, rdt, m, row0, C.c_void_p(out_ptr) if out_ptr else None, odt,
                cap, C.c_void_p(cnt_ptr) if cnt_ptr else None, C.c_void_p(st.data_ptr()), flags, None)
        if fn == "tfrg_result_select_rows":
            return lib.tfrg_result_select_rows(dec._ctx, arr, k, *tail)
        return lib.tfrg_result_select_match(dec._ctx, arr, k, patterns, len(patterns or b"") if plen is None else plen, *tail)

    assert call() == -1 and lib.tfrg_last_error() == b"tfrg_result_select_match: no result (decode first)"
    res = dec.decode(*synth.framed(synth.c1_payloads(10)))
    s_label, s_id = res.slot_key.index("label"), res.slot_key.index("id")
    ok = dict(slot=s_id)
    value = dict(slot=s_label, subject=N.SEL_VALUE, operand=0)
    for bad in (
            # what tfrg_result_select_rows refuses, with the limits at 6 and 8
            dict(ok, k=33), dict(ok, slot=len(res.slot_key)), dict(ok, subject=7), dict(ok, op=9), dict(ok, group=32),
            dict(ok, reserved=1), dict(slot=s_id, subject=N.SEL_VALUE), dict(slot=s_label, subject=N.SEL_BYTES_LEN),
            dict(value, subject=N.SEL_ANY, index=1), dict(value, subject=N.SEL_COUNT, index=1), dict(ok, rdt=2), dict(ok, odt=2),
            dict(ok, m=1 << 31), dict(ok, cnt_ptr=None), dict(ok, cnt_ptr=cnt.data_ptr() + 4), dict(ok, out_ptr=out.data_ptr() + 4),
            dict(ok, odt=N.ROWS_I32, row0=(1 << 31) - 9), dict(ok, flags=2),
            # a bytes subject on a slot of another kind
            dict(slot=s_label), dict(slot=s_label, subject=N.SEL_BYTES_ANY),
            # PREFIX / SUFFIX / CONTAINS with another subject
            dict(value, op=N.SEL_PREFIX), dict(value, op=N.SEL_SUFFIX), dict(value, subject=N.SEL_ANY, op=N.SEL_CONTAINS),
            dict(slot=s_id, subject=N.SEL_BYTES_LEN, op=N.SEL_CONTAINS, operand=1), dict(slot=s_id, subject=N.SEL_COUNT, op=N.SEL_PREFIX),
            dict(slot=0, subject=N.SEL_STATUS, op=N.SEL_SUFFIX),
            # index != 0 outside VALUE and BYTES
            dict(ok, subject=N.SEL_BYTES_ANY, index=1),
            # a pattern longer than TFRG_SEL_MAX_PATTERN, patterns_len above TFRG_SEL_MAX_PATTERN_BYTES
            dict(ok, operand=S.pack_pattern(0, 257)), dict(ok, patterns=blob + b"x"), dict(ok, plen=1 << 40),
            # a pattern range outside patterns
            dict(ok, operand=S.pack_pattern(2048 - 255, 256)), dict(ok, operand=S.pack_pattern(2049, 0)),
            dict(ok, operand=S.pack_pattern(0xFFFFFFFF, 1)), dict(ok, patterns=b"img", operand=S.pack_pattern(0, 4)),
            dict(ok, patterns=b"", operand=S.pack_pattern(0, 1)), dict(ok, patterns=None, plen=0, operand=S.pack_pattern(0, 1)),
            # patterns == NULL with patterns_len > 0
            dict(ok, patterns=None, plen=12), dict(value, patterns=None, plen=1)):
        assert call(**bad) == -1, bad
        assert lib.tfrg_last_error().startswith(b"tfrg_result_select_match: "), bad
    # the old call still refuses the new subjects and ops, under its own name
    for bad in (dict(slot=s_id, subject=5), dict(slot=s_id, subject=6), dict(value, op=6), dict(value, op=7), dict(value, op=8),
                dict(slot=s_id, subject=5, op=8)):
        assert call("tfrg_result_select_rows", **bad) == -1, bad
        assert lib.tfrg_last_error().startswith(b"tfrg_result_select_rows: "), bad
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [-1] * 64 and cnt.cpu().tolist() == [-1, -1] and st.cpu().tolist() == [77, 77]
    # what is allowed: the limits themselves, NULL patterns when every pattern is empty, index with BYTES,
    # the old subjects through the new call, shared and overlapping patterns
    assert call(**ok) == 0
    torch.cuda.synchronize()
    assert out.cpu().tolist()[:2] == [1, -1] and cnt.cpu().tolist() == [1, -1] and st.cpu().tolist() == [1, 0]
    for good in (dict(ok, operand=S.pack_pattern(2048 - 256, 256)), dict(ok, operand=S.pack_pattern(2048, 0)),
                 dict(ok, patterns=None, plen=0, operand=0, op=N.SEL_CONTAINS), dict(ok, index=3), dict(value),
                 dict(value, patterns=None, plen=0), dict(ok, k=32, op=N.SEL_CONTAINS, subject=N.SEL_BYTES_ANY),
                 dict(ok, cap=0), dict(ok, out_ptr=None), dict(ok, rows_ptr=None, rdt=9, m=14)):
        assert call(**good) == 0, good
    # nothing is written past cap: two records pass, one fits
    out.fill_(-1)
    assert call(slot=s_id, op=N.SEL_PREFIX, operand=S.pack_pattern(0, 4), cap=1) == 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0] + [-1] * 63 and cnt.cpu().tolist() == [3, -1] and st.cpu().tolist() == [3, 0]
    # m == 0 and n == 0 are as for the old call
    cnt.fill_(41)
    assert call(**ok, m=0, rows_ptr=None) == 0 and call(**ok, m=0, rows_ptr=None, flags=N.SEL_APPEND) == 0
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [0, 41]
    fr = synth.framed(synth.c1_payloads(10))
    assert len(dec.decode(fr[0][:0], fr[1][:0], fr[2][:0])) == 0
    assert call(**ok) == 0
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [0, 41] and st.cpu().tolist() == [0, 3]
