"""The decode on wide schemas (tests/_wide.py): past the lane kernel's LDS dicts, past 64 slots
(MaskSink -> the global-column dict, the second 64-slot loop of the staged gather, the 64-bit placed
mask), past 256 slots (the spine's column-base passes) and past 256 keys (the key table leaves LDS:
every record takes the exact walker), on both sides of each boundary.

Every case ends in ``_wide.compare``: every record against the oracle (status, aux, entries in key
order, values, both CRC verdict bits), every slot's row splits in full, the kind totals. Each batch
holds three corrupted records and a few malformed ones. Unless it says otherwise a case decodes on a
fresh ``HipDecoder``; the lane mode is not exposed, so every case asserts the size of the decoder's
key table and takes the mode from ``_wide.expected_mode`` (pinned by tests/test_wide_host.py).

Which kernel gathers a record's lists is decided by its size (``_wide.wave_route``, a port of the
test in ``k_lane_count``): up to ``lane_max`` the lane kernels, above it ``role_stage_gather`` when
the record spans at most min(wave_stage, kWStage = 12 KiB) and ``role_wave_gather`` otherwise.
``tfrg_info.n_big`` counts both sorts of large records and nothing the decode returns tells them
apart, so each case asserts the route that the sizes of its batch imply, and three batches per
schema are sized for the routes:

* the large dense records (every key, lists of 0 to 200 values; 7 KB and up, from 64 slots on all
  above kWStage): lane records walked from HBM (``lane``: lane_max 1 MiB, which stands in for the
  default lane_max, where every one of them is a large record) and ``role_wave_gather``'s
  (``huge``: lane_max 0);
* the stageable dense records (every key, real lists of 2, 5 and 12 values of every kind in every
  slot, all within kWStage): ``role_stage_gather``, whose second loop takes slots 64 and up
  (``staged``: lane_max 0), the same records through ``role_wave_gather`` (``wave``: wave_stage 0),
  as lane records, and at the default lane_max (lane records up to 29 slots, staged ones beyond);
* the sparse records (1 to 4 keys: 64 of them fit the lane kernel's 4 KiB stage): the lane
  kernel's staged fast walk, and both wave gathers.

Beside the sweep: spec (64-bit) varints on a mode-2 schema against the values as encoded; bytes,
float and int64 slots at indices 64 to 129, each slot's value column as one array; a speculative
placement learned on a narrow schema, then the key table grown past 64 slots; strict CRC on a
mode-2 batch; one context across schema growth and batch sizes (the scan words are not cleared
between decodes); 300 records with a key of their own each, holding lists.
"""

import numpy as np
import pytest

from oracle import oracle as O
from tests import _golden as G
from tests import _wide as W
from tfr_reader import _status as S
from tfr_reader import hip

pytestmark = pytest.mark.gpu

CASES = W.sweep_cases()
N = W.N_RECORDS

#: path -> (lane_max, wave_stage); None: the decoder's default
PATHS = {"default": (None, None), "lane": (1 << 20, None), "staged": (0, None), "huge": (0, None), "wave": (0, 0)}


@pytest.fixture(scope="module")
def orc():
    return O.Oracle()


def _decoder(path="default", slots=None, **kw) -> hip.HipDecoder:
    d = hip.HipDecoder(0, **kw)
    lane_max, wave_stage = PATHS[path]
    if lane_max is not None:
        d.set_lane_max(lane_max)
    if wave_stage is not None:
        d.set_wave_stage(wave_stage)
    for key, kind in slots or ():  # (a sparse batch does not hold every key: the whole schema up front)
        d.keys.intern(key, kind)
    return d


def _decode(b: W.Batch, path="default", slots=None, **kw):
    d = _decoder(path, slots)
    try:
        r = d.decode(b.buf, b.st, b.en, **kw)
        return r, len(d.keys.keys), len(d.keys.slot_key)
    finally:
        d.close()


def _check(r, b: W.Batch, orc, **kw) -> None:
    bad = W.compare(r, b.buf, b.st, b.en, orc, ref=b.ref, **kw)
    assert not bad, "\n".join(bad)


def _route(b: W.Batch, path: str) -> tuple[int, int, int]:
    """(lane, staged, huge) records of the batch on the path, by their sizes."""
    lane_max, wave_stage = PATHS[path]
    return W.wave_route(b.st, b.en, hip.DEFAULT_LANE_MAX if lane_max is None else lane_max, wave_stage)


# ------------------------------------------------------------------------------------ schema sweep
@pytest.fixture(scope="module", params=CASES, ids=[f"{k}keys-{s}slots" for k, s, _ in CASES])
def case(request):
    """One schema of the sweep with its three batches (and their oracle outcomes), shared by the
    paths and dropped before the next schema."""
    n_keys, n_slots, mode = request.param
    _, slots = W.schema_for(n_keys, n_slots)
    return {"keys": n_keys, "slots": n_slots, "mode": mode, "schema": slots, "dense": W.dense_batch(slots),
            "stage": W.stage_batch(slots), "sparse": W.sparse_batch(slots)}


def _sweep(case, orc, shape: str, path: str, want_route):
    b = case[shape]
    assert _route(b, path) == want_route  # (the sizes send the records where the case means them to go)
    r, nk, ns = _decode(b, path, case["schema"] if shape == "sparse" else None)
    assert (nk, ns) == (case["keys"], case["slots"]) and W.expected_mode(nk, ns) == case["mode"]
    assert int(r.info.n_big) == want_route[1] + want_route[2]
    assert not r.info.placed_slots
    _check(r, b, orc)
    return r


@pytest.mark.parametrize("path", ["lane", "huge"])
def test_sweep_dense(case, orc, path):
    """The large dense records: lane records walked from HBM, or large ones; from 64 slots on
    ``role_wave_gather`` takes every one of them whatever wave_stage says (below, 2 in 3 are staged)."""
    b = case["dense"]
    if path == "lane":
        want = (N, 0, 0)
    else:
        want = _route(b, path)
        assert want[0] == 0 and (want[1] == 0 if case["slots"] >= 64 else want[1] > 0 and want[2] > 0)
    _sweep(case, orc, "dense", path, want)


@pytest.mark.parametrize("path", ["default", "lane", "staged", "wave"])
def test_sweep_stage(case, orc, path):
    """The stageable dense records: every one staged by ``role_stage_gather`` (lane_max 0), streamed
    by ``role_wave_gather`` (wave_stage 0: the same records, the other route), a lane record, or
    what the default lane_max makes of it (a lane record up to 29 slots, a staged one from 64 on)."""
    small = case["slots"] < 64
    want = {"default": (N, 0, 0) if small else (0, N, 0), "lane": (N, 0, 0), "staged": (0, N, 0), "wave": (0, 0, N)}
    _sweep(case, orc, "stage", path, want[path])


@pytest.mark.parametrize("path", ["default", "staged", "wave"])
def test_sweep_sparse(case, orc, path):
    want = {"default": (N, 0, 0), "staged": (0, N, 0), "wave": (0, 0, N)}
    _sweep(case, orc, "sparse", path, want[path])


@pytest.mark.parametrize("shape,path", [("stage", "staged"), ("stage", "wave"), ("dense", "huge")])
def test_spec_varints_mode2(orc, shape, path):
    """A 70-slot schema decoded with spec (64-bit) varints, every record a large one, staged
    (``role_stage_gather``) or not: the int64 lists are the values as encoded; keys, order, floats
    and bytes are the oracle's (whose int64 lists are the reference's int-width ones, so they are
    not compared)."""
    _, slots = W.schema(70)
    b = (W.stage_batch if shape == "stage" else W.dense_batch)(slots, seed=9, corrupt=False)
    assert _route(b, path) == {"staged": (0, len(b), 0)}.get(path, (0, 0, len(b)))
    d = _decoder(path, spec_varint=True)
    try:
        r = d.decode(b.buf, b.st, b.en)
        assert len(d.keys.slot_key) == 70 and W.expected_mode(70, 70) == 2
    finally:
        d.close()
    assert int(r.info.n_big) == len(b)
    wide = 0
    for i in range(len(b)):
        if i in b.malformed:
            continue
        assert int(r.status[i]) == 0, i
        want = [(k, kind, b.int_values[i][k] if kind == "int64_list" else v) for k, kind, v in b.ref[i][2]]
        assert G.canon_entries(W.raw_entries(r, i)) == want, i
        wide += sum(1 for k, kind, v in b.ref[i][2] if kind == "int64_list" and v != b.int_values[i][k])
    assert wide > 100  # (the two varint modes do differ on these values)
    assert [int(r.status[i]) for i in b.malformed if i % 107 == 5] == [S.ERR_VARINT_TOO_MANY] * 3


# ----------------------------------------------------------------------------- kinds at high slots
def _quiet(a: np.ndarray) -> np.ndarray:
    a = a.astype(np.uint32)
    nan = ((a & 0x7F800000) == 0x7F800000) & ((a & 0x7FFFFF) != 0)
    return np.where(nan, a | 0x400000, a)


@pytest.mark.parametrize("shape,path", [("stage", "staged"), ("stage", "wave"), ("dense", "huge")])
def test_value_columns_of_slots_64_to_129(orc, shape, path):
    """130 slots, slots 64 to 129 bytes, float and int64 in turn. ``stage-staged``: every record
    spans less than kWStage and is gathered by ``role_stage_gather``, slots 64 to 129 by its second
    loop (lists of 2, 5 and 12 values of each kind). ``stage-wave`` and ``dense-huge``: the same
    through ``role_wave_gather``'s slot stride. Beside the record-by-record comparison, each of
    these slots' value columns, sliced by slot_base and row_splits, equals the oracle's values of
    that (key, kind) concatenated over the records, as one array."""
    _, slots = W.kinds_high_schema()
    b = (W.stage_batch if shape == "stage" else W.dense_batch)(slots, seed=3)
    assert _route(b, path) == {"staged": (0, len(b), 0)}.get(path, (0, 0, len(b)))
    r, nk, ns = _decode(b, path)
    assert (nk, ns) == (130, 130) and int(r.info.n_big) == len(b)
    # the first record holds the keys in schema order: so are the slots numbered
    assert [(k.encode(), kd) for k, kd in zip(r.slot_key, r.slot_kind)] == slots
    assert [r.slot_kind[64:].count(kd) for kd in (1, 2, 3)] == [22, 22, 22]
    want, lists = {}, {}
    for ost, _, ent, _, _ in b.ref:
        for key, kind, vals in ent or ():
            want.setdefault((key, W.KIND_ID[kind]), []).extend(vals)
            lists[key, W.KIND_ID[kind]] = lists.get((key, W.KIND_ID[kind]), 0) + (len(vals) > 1)
    raw = r.buf
    for s in range(64, 130):
        key, kd = slots[s]
        rs = r.row_splits[s].astype(np.int64)
        lo, hi = int(r.slot_base[s]) + int(rs[0]), int(r.slot_base[s]) + int(rs[-1])
        w = want[key, kd]
        assert hi - lo == len(w) > 400 and lists[key, kd] > 60, (s, key)  # (out-of-line lists: the gathers' work)
        if kd == 3:
            assert np.array_equal(r.i64[lo:hi], np.array(w, np.int64)), f"int64 slot {s} {key}: column differs"
        elif kd == 2:
            assert np.array_equal(_quiet(r.f32[lo:hi]), _quiet(np.array(w, np.uint32))), f"float slot {s} {key}"
        else:
            off, ln = r.bytes_off[lo:hi], r.bytes_len[lo:hi]
            assert np.array_equal(ln, np.array([len(x) for x in w], np.uint32)), f"bytes slot {s} {key}: lengths"
            got = b"".join(raw[o : o + n].tobytes() for o, n in zip(off.tolist(), ln.tolist()))
            assert got == b"".join(w), f"bytes slot {s} {key}: contents"
    # the slots' runs tile each kind's column without gap or overlap
    for kd in (1, 2, 3):
        runs = sorted((int(r.slot_base[s]), int(r.row_splits[s, -1])) for s in range(130) if r.slot_kind[s] == kd)
        at = 0
        for base, cnt in runs:
            assert base == at, (kd, base, at)
            at += cnt
        assert at == int(r.info.kind_totals[kd])
    _check(r, b, orc)


# --------------------------------------------------------------- placed slots beside a wide schema
def test_placed_slots_then_wide_schema(orc):
    """16 single-value slots are placed speculatively (placed_slots != 0); a batch of 60 more keys
    takes the same decoder's key table to 76 slots (mode 2, past the 64 bits of the placed mask):
    nothing is placed any more, every slot's row splits are stored and exact, and the narrow
    records decode to what they decoded to at first, column by column."""
    narrow = W.narrow_batch(600, W.kernel_constants()["kLeanMaxSlots"])
    _, wide_slots = W.schema(60)
    wide = W.dense_batch(wide_slots, seed=11)
    d = hip.HipDecoder(0)
    try:
        r1 = d.decode(narrow.buf, narrow.st, narrow.en)
        assert len(d.keys.slot_key) == 16 and W.expected_mode(16, 16, spec=True) == 0
        assert r1.info.placed_slots != 0
        _check(r1, narrow, orc)
        r2 = d.decode(wide.buf, wide.st, wide.en)
        assert len(d.keys.slot_key) == 76 and W.expected_mode(76, 76) == 2
        assert r2.info.placed_slots == 0
        _check(r2, wide, orc)
        r3 = d.decode(narrow.buf, narrow.st, narrow.en)
        assert len(d.keys.slot_key) == 76 and r3.info.placed_slots == 0
        _check(r3, narrow, orc)
    finally:
        d.close()
    for s in range(16):
        assert np.array_equal(r3.row_splits[s], np.arange(len(narrow) + 1)), s
    assert not r3.row_splits[16:].any() and not r3.order[16:].any()
    assert not W.columns_differ(r1, r3)


# -------------------------------------------------------------------------------------- strict CRC
@pytest.mark.parametrize("shape,path", [("dense", "lane"), ("stage", "staged"), ("dense", "huge")])
def test_strict_crc_mode2(orc, shape, path):
    """strict_crc on a 65-slot dense batch, as lane records, staged large records and huge ones: the
    three corrupted records fail with ERR_CRC and hold nothing (``strict_reject`` /
    ``withdraw_record`` go over all 65 slots, the tile sums included: the row splits behind them
    close up), every other record is the loose decode's."""
    _, slots = W.schema(65)
    b = (W.stage_batch if shape == "stage" else W.dense_batch)(slots, seed=13)
    n = len(b)
    assert _route(b, path) == {"lane": (n, 0, 0), "staged": (0, n, 0), "huge": (0, 0, n)}[path]
    d = _decoder(path)
    try:
        loose = d.decode(b.buf, b.st, b.en)
        strict = d.decode(b.buf, b.st, b.en, strict_crc=True)
        assert len(d.keys.slot_key) == 65
    finally:
        d.close()
    _check(loose, b, orc)
    _check(strict, b, orc, strict=True)
    hit = sorted(b.corrupted.values())
    for i in range(len(b)):
        if i in hit:
            want = b.ref[i][0] or S.ERR_CRC
            assert int(strict.status[i]) == want and not strict.order[:, i].any(), i
            assert want != S.ERR_CRC or int(strict.aux[i]) == int(loose.verdict[i]), i
        else:
            assert int(strict.status[i]) == int(loose.status[i]), i
            assert W.raw_entries(strict, i) == W.raw_entries(loose, i), i
    assert int((strict.status == S.ERR_CRC).sum()) >= 2


# ------------------------------------------------------ one context across schemas and batch sizes
def test_one_context_across_schema_growth_and_batch_sizes(orc):
    """The scan words (tile sums | look-back words | irr, laid out [S][tile_stride], [S][n_chunks],
    [S] in one buffer) are cleared only when the buffer grows: each decode must leave every word it
    dirtied at zero for the next, whose S and tile_stride differ. One decoder takes 1,100 narrow
    records, 321 dense ones of 65 slots, 2,900 sparse ones over 300 slots, 70 dense ones of 257 keys,
    one record, an empty batch and the first batch again (tile_stride 8, 4, 12, 4, 4, 8 while S
    grows): every result equals the oracle and a fresh decoder's, the last one the first."""
    steps = W.reuse_steps()
    d = hip.HipDecoder(0)
    try:
        first = None
        for k, b in enumerate(steps + (steps[0],)):
            r = d.decode(b.buf, b.st, b.en)
            if not len(b):
                assert int(r.info.n_records) == 0 and int(r.info.n_errors) == 0 and len(r.status) == 0, k
            bad = W.compare(r, b.buf, b.st, b.en, orc, ref=b.ref)
            assert not bad, f"step {k + 1}:\n" + "\n".join(bad)
            f = hip.HipDecoder(0)
            try:
                fresh = f.decode(b.buf, b.st, b.en)
            finally:
                f.close()
            bad = W.columns_differ(r, fresh)
            assert not bad, f"step {k + 1} vs a fresh decoder: {bad[:10]}"
            first, last = (r if first is None else first), r
        bad = W.columns_differ(first, last)
        assert not bad, f"step 7 vs step 1: {bad[:10]}"
        assert len(d.keys.keys) > W.kernel_constants()["kLdsMaxKeys"]
    finally:
        d.close()


def test_scan_words_between_layouts_without_growth(orc):
    """The same invariant where no clearing can help: in the sequence above the scan buffer grows
    (and is cleared) at steps 2 and 3. Here 1,100 narrow records (slots 0 to 7), 321 dense ones of
    65 slots (slots 8 to 72) and 2,900 sparse ones over 300 slots bring the buffer to its final size;
    then the dense batch (tile_stride 4, every tile sum non-zero), the narrow one (tile_stride 8),
    and both again follow in a buffer that no longer grows. Tile 1 of dense slot 8 (word 4 * 8 + 1)
    is tile 1 of narrow slot 4 (word 8 * 4 + 1), and so for slots 10 and 5, 12 and 6, 14 and 7: a
    tile sum left behind by one decode is a tile prefix of the next."""
    narrow, dense, sparse = W.narrow_batch(1100, 8), W.reuse_steps()[1], W.reuse_steps()[2]
    d = hip.HipDecoder(0)
    try:
        for k, b in enumerate((narrow, dense, sparse, dense, narrow, dense, narrow)):
            r = d.decode(b.buf, b.st, b.en)
            assert len(d.keys.slot_key) == (8, 73, 308)[min(k, 2)]
            bad = W.compare(r, b.buf, b.st, b.en, orc, ref=b.ref)
            assert not bad, f"decode {k + 1}:\n" + "\n".join(bad)
        assert r.slot_key[:8] == [f"nar{j}" for j in range(8)]
        assert [(x.encode(), kd) for x, kd in zip(r.slot_key[8:73], r.slot_kind[8:73])] == W.schema(65)[1]
    finally:
        d.close()
    strides = [W.tile_stride(len(b)) for b in (sparse, narrow, dense)]
    assert strides == [12, 8, 4]  # (the sparse decode's scan words hold the later ones)


# ------------------------------------------------------------------ high-cardinality keys, dense
def test_high_cardinality_keys_with_lists(orc):
    """300 records with a key of their own each (302 keys: the key table is past LDS, every record
    takes the exact walker), each holding a list of 0 to 40 int64 values, a float list and a bytes
    list under shared keys: all 300 records against the oracle."""
    b = W.high_cardinality_batch(300)
    r, nk, ns = _decode(b)
    assert (nk, ns) == (302, 302) and not W.schema_in_lds(nk)
    _check(r, b, orc)
