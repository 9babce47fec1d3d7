"""Host-side checks of the wide-schema cases (tests/_wide.py; no GPU): the constants the case
table was laid out for are the ones the sources build with, the table reaches the lane modes and
key-table regimes it claims, the colliding key names really share their hash, and every generated
batch is what tests/test_wide_schema_gpu.py takes it for: decodable by the oracle but for the few
records malformed on purpose, decoded alike by the host walker, dense records too large for the
lane kernel's LDS stage and sparse ones small enough for it."""

import numpy as np
import pytest

from tests import _wide as W
from tfr_reader import _status as S
from tfr_reader import hip, host

CASES = W.sweep_cases()
IDS = [f"{k}keys-{s}slots" for k, s, _ in CASES]


def test_pinned_constants():
    """A retune of any of these moves the boundaries the wide-schema cases sit on: revisit the case
    table of tests/_wide.py (``sweep_cases``, ``reuse_steps``) with it, then ``PINNED``."""
    assert W.kernel_constants() == W.PINNED


def test_case_table_reaches_the_lane_modes():
    m0 = W.largest_mode0()
    assert W.expected_mode(m0, m0) == 0 and W.expected_mode(m0 + 1, m0 + 1) == 1
    assert 16 < m0 < 63  # both sides of the switch are schemas of MODE 0 / MODE 1 size
    assert [m for _, _, m in CASES] == [W.expected_mode(k, s) for k, s, _ in CASES]
    assert {(k, s): m for k, s, m in CASES} == {
        (m0, m0): 0, (m0 + 1, m0 + 1): 1, (64, 64): 1, (65, 65): 2, (128, 128): 2, (129, 129): 2, (100, 300): 2,
        (256, 256): 2, (256, 257): 2, (257, 257): 2, (300, 300): 2}
    # a speculative placement takes LDS of its own: the switch can only come earlier with it
    assert W.expected_mode(m0 + 1, m0 + 1, spec=True) == 1
    assert W.expected_mode(8, 8, spec=True) == 0 and W.expected_mode(16, 16, spec=True) == 0


def test_key_table_leaves_lds_past_256_keys():
    c = W.kernel_constants()
    assert W.schema_in_lds(256) and not W.schema_in_lds(257)
    assert W.schema_in_lds(100)  # 100 keys x 3 kinds: 300 slots with the key table still in LDS
    # the table-size half of the condition cannot fail on its own: kLdsMaxKeys keys give a table of
    # exactly kLdsMaxHt entries, so the key count alone decides
    assert W.ht_size(c["kLdsMaxKeys"]) == c["kLdsMaxHt"]
    assert all(W.ht_size(k) <= c["kLdsMaxHt"] for k in range(c["kLdsMaxKeys"] + 1))


def test_tile_strides_of_the_reuse_steps():
    steps = W.reuse_steps()
    assert [len(b) for b in steps] == [1100, 321, 2900, 70, 1, 0]
    assert [W.tile_stride(len(b)) for b in steps if len(b)] + [W.tile_stride(1100)] == [8, 4, 12, 4, 4, 8]


@pytest.mark.parametrize("n_keys", [28, 65, 300])
def test_key_names_mix_and_collide(n_keys):
    names, slots = W.schema(n_keys)
    kind = dict(slots)
    assert any(len(nm) <= 4 for nm in names) and any(len(nm) > 8 for nm in names)
    assert n_keys < 9 or any(len(nm) == 8 for nm in names)
    groups = W.colliding_groups(names)
    assert len(groups) >= 8
    for g in groups:
        assert len({W.key_hash_words(nm) for nm in g}) == 1, g
        assert len(set(g)) == len(g) and len({kind[nm] for nm in g}) == len(g), g
    # and the hash is not constant: names outside a group spread
    assert len({W.key_hash_words(nm) for nm in names}) >= len(names) - sum(len(g) - 1 for g in groups) - 2


def test_slot_count_apart_from_key_count():
    names, slots = W.schema(100, 3)
    assert len(names) == 100 and len(slots) == 300 and len(set(slots)) == 300
    names, slots = W.schema_for(256, 257)
    assert len(names) == 256 and len(slots) == 257 and len(W.key_kinds(slots)[names[0]]) == 2
    _, slots = W.kinds_high_schema()
    assert [kd for _, kd in slots[64:70]] == [2, 3, 1, 2, 3, 1]


def _check_batch(b: W.Batch, label: str) -> None:
    """The oracle decodes every record but the malformed ones (and perhaps the one whose payload byte
    was flipped) with status 0, at most 5 % of the batch fails, and the host walker agrees with the
    oracle record by record."""
    n = len(b)
    ref = b.ref
    may_fail = set(b.malformed) | ({b.corrupted["payload"]} if b.corrupted else set())
    failed = [i for i, x in enumerate(ref) if x[0]]
    assert set(failed) <= may_fail, (label, failed)
    assert 0 not in failed and 0 not in b.malformed
    assert len(b.malformed) <= 0.05 * n, (label, b.malformed)
    raw = b.buf.tobytes()
    for i in range(n):
        payload = raw[int(b.st[i]) + 12 : int(b.en[i]) - 4]
        st, aux, ent = host.decode_raw(payload)
        ost, oaux, oent, _, _ = ref[i]
        assert st == ost, (label, i, st, ost)
        if st:
            assert W.G.status_exception(st, aux, payload) == W.G.status_exception(ost, oaux, payload), (label, i)
        else:
            assert W.G.canon_entries(ent) == oent, (label, i)
    if b.corrupted:
        for what, i in b.corrupted.items():
            assert (ref[i][3], ref[i][4]) == {"length_crc": (False, True), "payload": (True, False),
                                              "data_crc": (True, False)}[what], (label, what)
        assert sum(1 for x in ref if not (x[3] and x[4])) == 3


@pytest.mark.parametrize("n_keys,n_slots,mode", CASES, ids=IDS)
def test_sweep_batches(n_keys, n_slots, mode):
    c = W.kernel_constants()
    names, slots = W.schema_for(n_keys, n_slots)
    dense, stage, sparse = W.dense_batch(slots), W.stage_batch(slots), W.sparse_batch(slots)
    assert len(dense) == len(stage) == len(sparse) == W.N_RECORDS
    _check_batch(dense, "dense")
    _check_batch(stage, "stage")
    _check_batch(sparse, "sparse")
    # every (key, kind) slot of the schema occurs, in both batches together with what the oracle saw
    lens = W.oracle_lengths(dense.ref, len(dense))
    assert set(lens) == set(slots)
    for sl in slots:  # and every list length of the cycle, in every slot
        assert set(W.CYCLE) <= set(lens[sl].tolist()), sl
    # the malformed records are of the three kinds: the 11-byte varint fails as the reference's does
    assert [dense.ref[i][0] for i in dense.malformed if i % 107 == 5] == [S.ERR_VARINT_TOO_MANY] * 3
    assert len(dense.malformed) == len(stage.malformed) == len(sparse.malformed) == 9
    # the stageable batch: every slot, of every kind, holds out-of-line lists of 2, 5 and 12 values
    # (what the wave gathers write; single values are inline and k_down_gather's), in many records
    slens = W.oracle_lengths(stage.ref, len(stage))
    assert set(slens) == set(slots)
    for sl in slots:
        got = slens[sl].tolist()
        assert set(W.STAGE_LISTS) | {0, 1} == set(got) and sum(1 for x in got if x > 1) >= 15, sl
    # the routes by size (k_lane_count): above lane_max a record spanning at most kWStage is
    # role_stage_gather's, a larger one role_wave_gather's. Every stageable record is within kWStage;
    # from 64 slots on every large dense record is beyond it, whatever wave_stage is set to
    n, kw = W.N_RECORDS, c["kWStage"]
    span = lambda b: (b.en.astype(np.int64) - (b.st.astype(np.int64) & ~15))  # noqa: E731
    assert span(stage).max() <= kw and span(sparse).max() <= kw
    assert W.wave_route(stage.st, stage.en, 0) == (0, n, 0) and W.wave_route(stage.st, stage.en, 0, 0) == (0, 0, n)
    assert W.wave_route(stage.st, stage.en, 1 << 20) == (n, 0, 0)
    assert W.wave_route(stage.st, stage.en, hip.DEFAULT_LANE_MAX) == ((n, 0, 0) if n_slots < 64 else (0, n, 0))
    assert W.wave_route(sparse.st, sparse.en, 0) == (0, n, 0) and W.wave_route(sparse.st, sparse.en, 0, 0) == (0, 0, n)
    if n_slots >= 64:
        assert span(dense).min() > kw and W.wave_route(dense.st, dense.en, 0) == (0, 0, n)
    else:
        _, staged, huge = W.wave_route(dense.st, dense.en, 0)
        assert staged > 0 and huge > 0
    # record sizes: dense records are large records at the default lane_max, lane records at 1 MiB,
    # and never fit a wave's LDS stage; 64 sparse records do
    size = (dense.en - dense.st).astype(np.int64)
    assert size.min() > hip.DEFAULT_LANE_MAX and size.max() < (1 << 20)
    assert size.min() > c["kStageBytes"] // 64
    assert W.wave_spans(dense.st, dense.en).min() > c["kStageBytes"]
    ssize = (sparse.en - sparse.st).astype(np.int64)
    assert ssize.max() <= hip.DEFAULT_LANE_MAX
    assert W.wave_spans(sparse.st, sparse.en).max() <= c["kStageBytes"]
    assert np.median(ssize) < c["kStageBytes"] // 64


def test_other_batches():
    _, slots = W.kinds_high_schema()
    _check_batch(W.dense_batch(slots, seed=3), "kinds at high slots")
    b = W.stage_batch(slots, seed=3)
    _check_batch(b, "kinds at high slots, stageable")
    assert W.wave_route(b.st, b.en, 0) == (0, len(b), 0)
    for seed, n_keys in ((9, 70), (13, 65)):  # (the spec-varint and strict-CRC batches)
        b = W.stage_batch(W.schema(n_keys)[1], seed=seed)
        _check_batch(b, f"stageable, {n_keys} slots")
        assert W.wave_route(b.st, b.en, 0) == (0, len(b), 0)
        b = W.dense_batch(W.schema(n_keys)[1], seed=seed)
        assert W.wave_route(b.st, b.en, 0) == (0, 0, len(b))
    _check_batch(W.high_cardinality_batch(), "high cardinality")
    for k, b in enumerate(W.reuse_steps()):
        _check_batch(b, f"reuse step {k + 1}")
    b = W.narrow_batch(600, 16)
    _check_batch(b, "narrow")
    assert all(len(vals) == 1 for x in b.ref for _, _, vals in x[2])
    _check_batch(W.dense_batch(W.schema(70)[1], seed=9, corrupt=False), "spec varint")
