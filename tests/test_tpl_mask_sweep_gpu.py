"""k_tpl_lane's mask-only hits (csrc/tfrg_tpl.hip) against the canonical walk and the oracle, on the
one-byte mutants of tests/_mutants.py: the shapes S16 / S32 / S64 (W = 16 / 32 / 64 window words, S16
with two templates on one length chain), every byte of one framed record per template set to each of
{b ^ 0x01, b ^ 0x80, 0x00, 0xFF}. tests/test_tpl_mask_sweep_host.py has held the learner's mask and
the numpy restatement `_hit` of the kernel's rule to the oracle; here the kernel runs the batches.

Contexts: the trio of tests/test_unchecked_frames_gpu.py (staged windows, per-lane windows, no
templates as the yardstick), taught by one decode of the shape's clean sample in the frame class.
Decode modes: (A) zero-CRC frames with CRCs on and (C) with crc=False, (B) spec frames with
crc=False -- in these three the mask is a hit's only guard -- and (D) spec frames with CRCs on as
the control, where every mutant misses. Offsets: ends for every shape, u64 and u32 as well for S16.

Per batch and mode every column equals the yardstick's, and the mutated records and their
neighbours the oracle's. The benign batch takes templates throughout (no re-run, no group missed,
the clean sample's implicit columns: the values come from k_tpl_lane's stores, read from mutated
bytes); the hostile batch misses exactly the groups `_hit` predicts. The key mutants run last: each
one that still decodes adds a key to the contexts' schemas.

Only S16 decodes optimistically (every slot one inline value); S32 and S64 have list slots, so their
decodes launch every pass, a missed record costs no re-run and no column is implicit.
"""

import numpy as np
import pytest

from oracle import oracle as O
from tests import _mutants as M
from tests.test_tpl_mask_sweep_host import SAMPLE_N, batches, learned, predict
from tests.test_unchecked_frames_gpu import COLS, _all, _close, _device, _oracle, _trio
from tests.test_unchecked_templates_host import K_FRAME, K_L, _hit
from tfr_reader import synth

pytestmark = pytest.mark.gpu

LEN_MATCH = 1  # TFRG_V_LEN_MATCH
MAX_SLOTS = 16  # kLeanMaxSlots: k_tpl_lane runs for schemas of at most this many slots
assert COLS and _device  # (the trio's helpers: _all decodes through _device and compares COLS)


@pytest.fixture(scope="module")
def orc():
    return O.Oracle()


def _near(idx, n) -> list[int]:
    """Every mutated record and both its neighbours."""
    return sorted({j for i in idx.tolist() for j in (i - 1, i, i + 1) if 0 <= j < n})


def _groups(n: int) -> int:
    return (n + 63) // 64


def _share_keys(trio, sample, buf, st, en, crc, n_tpl) -> None:
    """A device decode interns no keys: a record with a key outside the schema (a mutated key, a key
    cut short by a mutated length) ends as ST_SCHEMA_MISS. So the yardstick context decodes the batch
    from the host first, which interns what the batch misses, in the order the device reports it; the
    template contexts take the yardstick's key table entry by entry (the columns are compared slot by
    slot) and, their templates dropped with the old schema, learn the clean sample again."""
    yard = trio[2]
    before = yard.keys.version
    yard.decode(buf, st, en, crc=crc)
    if yard.keys.version == before:
        return
    kt = yard.keys
    for d in trio[:2]:
        for key in kt.keys:
            d.keys.intern(key, 0)
        for kid, kind in zip(kt.slot_key, kt.slot_kind):
            d.keys.intern(kt.keys[kid], kind)
        assert d.keys.keys == kt.keys and (d.keys.slot_key, d.keys.slot_kind) == (kt.slot_key, kt.slot_kind)
        d.decode(*sample)
        assert d.template_count() == n_tpl


@pytest.mark.parametrize("frames", ["spec", "zero"])
@pytest.mark.parametrize("name", ["S16", "S32", "S64"])
def test_mutants_take_templates_exactly_when_the_mask_allows(monkeypatch, orc, name, frames):
    spec = frames == "spec"
    shape = M.SHAPES[name]
    sample = synth.framed(shape.clean(SAMPLE_N), spec)
    tpls, _ = learned(name, spec)
    optimistic = name == "S16"
    parts = batches(name, spec)
    modes = (("D", True), ("B", False)) if spec else (("A", True), ("C", False))
    trio = _trio(monkeypatch, sample)
    try:
        frames_bits = int(np.bitwise_or.reduce([1 << int(t[K_FRAME]) for t in tpls]))
        assert frames_bits == (1 if spec else 2)
        for d in trio[:2]:  # the host learner's answer for the same sample
            assert d.template_count() == len(tpls) and d.template_frames() == frames_bits
        for mode, crc in modes:
            for om in ("ends", "u64", "u32") if name == "S16" else ("ends",):
                r, reruns, _ = _all(trio, *sample, om, crc=crc)
                clean_implicit = int(r.info.implicit_cols)
                assert reruns == 0 and int(r.info.tpl_groups_missed) == 0 and bool(clean_implicit) == optimistic

                buf, st, en, idx, _ = parts["benign"]
                _share_keys(trio, sample, buf, st, en, crc, len(tpls))
                r, reruns, _ = _all(trio, buf, st, en, om, crc=crc)
                _oracle(r, orc, buf, _near(idx, len(st)), check_crc=crc)
                assert not np.array(r.status).any()
                if mode == "D":  # every benign mutant fails its data CRC
                    assert reruns == (1 if optimistic else 0)
                    assert int(r.info.tpl_groups_missed) == len(M.groups_of(idx))
                else:
                    assert reruns == 0 and int(r.info.tpl_groups_missed) == 0
                    assert (np.array(r.verdict) == LEN_MATCH).all()
                    assert int(r.info.implicit_cols) == clean_implicit

                buf, st, en, idx, _ = parts["hostile"]
                pred = predict(name, spec, "hostile", nocrc=not crc)
                assert mode != "D" or (pred < 0).all()
                missed = M.groups_of(idx[pred < 0])
                _share_keys(trio, sample, buf, st, en, crc, len(tpls))
                r, reruns, _ = _all(trio, buf, st, en, om, crc=crc)
                _oracle(r, orc, buf, _near(idx, len(st)), check_crc=crc)
                assert int(r.info.tpl_groups_missed) == len(missed)
                assert 2 * len(missed) > _groups(len(st)) and len(missed) < _groups(len(st))
                assert trio[0].template_count() >= 1 and reruns == (1 if optimistic else 0)
        buf, st, en, idx, _ = parts["keys"]
        for mode, crc in modes:
            _share_keys(trio, sample, buf, st, en, crc, len(tpls))
            r, _, _ = _all(trio, buf, st, en, "ends", crc=crc)
            _oracle(r, orc, buf, _near(idx, len(st)), check_crc=crc)
            # the mutated keys that are still UTF-8 joined the schema; past kLeanMaxSlots slots the
            # template pass does not run for the batch, so it misses nothing
            assert int(r.info.n_slots) > len(shape.slots)
            if int(r.info.n_slots) > MAX_SLOTS:
                assert int(r.info.tpl_groups_missed) == 0
    finally:
        _close(trio)


def test_second_template_of_a_length_chain(monkeypatch, orc):
    """S16's two templates of payload length 42: records of each whose value bytes look like the
    other's structure at the same window position. Each matches its own template -- for one of the
    two the second on the chain -- and neither is taken by the other's."""
    shape = M.S16
    sample = synth.framed(shape.clean(SAMPLE_N), False)
    recs, dressed = M.chain_records(shape)
    _, buf, st, en = M.place(shape, recs, synth.framed, False)
    idx = M.mutant_index(len(recs))
    tpls, W = learned("S16", False)
    chain = [t for t in range(len(tpls)) if int(tpls[t][K_L]) == 42]
    hits = {_hit(tpls, W, buf, int(st[j]), int(en[j]), nocrc=nocrc)[0] for j in idx.tolist() for nocrc in (False, True)}
    assert len(chain) == 2 and hits == set(chain) and dressed >= 1
    trio = _trio(monkeypatch, sample)
    try:
        for crc in (True, False):
            r, reruns, _ = _all(trio, buf, st, en, "ends", crc=crc)
            assert reruns == 0 and int(r.info.tpl_groups_missed) == 0 and not np.array(r.status).any()
            assert (np.array(r.verdict) == LEN_MATCH).all() and int(r.info.implicit_cols) != 0
            _oracle(r, orc, buf, range(len(st)), check_crc=crc)
    finally:
        _close(trio)
