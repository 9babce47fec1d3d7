"""The learner's template mask (tpl_derive, csrc/tfrg_learn.cpp) against the oracle, byte by byte, in
the modes where the mask is a hit's only guard: unchecked-frame templates (zero-CRC files; the hit
rule is the mask match and masked(K ^ lin) != 0) and crc=False decodes (the mask match alone). No GPU:
k_tpl_lane's rule is tests/test_unchecked_templates_host.py's numpy restatement `_hit`, which
tests/test_tpl_mask_sweep_gpu.py then holds the kernel to.

For the shapes S16 / S32 / S64 of tests/_mutants.py (W = 16 / 32 / 64; S16 with two templates on one
length chain) and both frame classes, every one-byte mutant of one record per template -- each value
of {b ^ 0x01, b ^ 0x80, 0x00, 0xFF} at each of the L + 16 framed positions -- is run through `_hit`:

* a hit implies the template's dict: the oracle's status of the mutated payload is 0 and its entries
  are the template's entries read at the window positions (inline int64 by the 7-bit regrouping,
  float bits, the bytes element's offset / length, list locations decoded from the payload), in key
  order. This is what makes the mask sufficient;
* benign implies a hit: a mutant inside a bytes element or a float, or of the low 7 bits of a varint
  byte, hits the template its clean record hits. This is what keeps the mask no stricter than needed;
* structural implies a miss: every other payload mutant, and every mutant of the length field or the
  length CRC, misses every template;
* with spec templates and CRCs on (the guarded mode, as a control) every mutant misses.

EXCEPTIONS lists the benign mutants that must not hit by the first statement: none was found. The
oracle takes the low 7 bits of every varint byte, the 10th byte of a negative int64 included, as
value bits only (decode_varint ends on bit 7 and fails on the 11th byte alone), which is the claim
the mask 0x80 makes.

Run with -s for the counts per shape and frame class.
"""

import functools
import struct

import numpy as np
import pytest

from oracle import oracle as O
from tests import _mutants as M
from tests.test_unchecked_templates_host import K_ENT, K_FRAME, K_L, K_NE, _hit, _learn
from tfr_reader import synth

SAMPLE_N = 600  # clean records the templates are learned from (>= 256: a shape needs two records)
KIND_NAME = {1: "bytes_list", 2: "float_list", 3: "int64_list"}
INLINE_COUNT = 1 | 0x80000000

# benign mutants that must not hit: {shape name: ((variant, framed position, value), ...)} with the
# oracle's verdict beside each. The sweep found none.
EXCEPTIONS: dict = {"S16": (), "S32": (), "S64": ()}

# (name, _hit's nocrc) per frame class of the sample: spec frames (crc=True), zero-CRC frames
MODES = (("nocrc", True), ("crc", False))


@functools.lru_cache(maxsize=None)
def learned(name: str, crc: bool):
    """(templates, W) of the shape's clean sample framed with spec (crc) or zero CRCs."""
    shape = M.SHAPES[name]
    buf, st, en = synth.framed(shape.clean(SAMPLE_N), crc)
    return _learn(buf, st, en, list(shape.keys), list(shape.slots))


@functools.lru_cache(maxsize=None)
def batches(name: str, crc: bool):
    """{part: (image, starts, ends, mutant records, mutants)} for benign / hostile / keys."""
    shape = M.SHAPES[name]
    parts = M.split(M.all_mutants(shape, synth.framed, crc), EXCEPTIONS[name])
    return {k: M.batch(shape, v, synth.framed, crc) + (v,) for k, v in parts.items()}


def predict(name: str, crc: bool, part: str, nocrc: bool) -> np.ndarray:
    """`_hit`'s template (or -1) of every mutant of a batch."""
    tpls, W = learned(name, crc)
    buf, st, en, idx, _ = batches(name, crc)[part]
    return np.array([_hit(tpls, W, buf, int(st[j]), int(en[j]), nocrc=nocrc)[0] for j in idx.tolist()], np.int64)


def _compat_varint(bs: bytes) -> int:
    """The reference's varint (oracle/tfrg_oracle.c decode_varint): each group shifted as a C int."""
    r = 0
    for k, b in enumerate(bs):
        t = ((b & 0x7F) << ((7 * k) & 31)) & 0xFFFFFFFF
        r |= t - (1 << 32) if t & 0x80000000 else t
    return r


def _list_values(payload: bytes, lo: int, ln: int, kind: int) -> list:
    """The values of a list location: packed chunks (tag 0x0a, length, body) in [lo, lo + ln)."""
    out, q = [], lo
    while q < lo + ln:
        assert payload[q] == 0x0A
        q, n, k = q + 1, 0, 0
        while True:
            b = payload[q]
            q, n, k = q + 1, n | (b & 0x7F) << (7 * k), k + 1
            if not b & 0x80:
                break
        body, q = payload[q : q + n], q + n
        if kind == 2:
            out += list(struct.unpack(f"<{n // 4}I", body))
        else:
            a = 0
            for z, b in enumerate(body):
                if not b & 0x80:
                    out.append(_compat_varint(body[a : z + 1]))
                    a = z + 1
            assert a == len(body)
    assert q == lo + ln
    return out


def template_dict(shape, tp, W, buf, s, e) -> list:
    """The entries k_tpl_lane stores for a record that hit `tp`, in the oracle's form (bytes values as
    (payload offset, length) views): tests/test_templates_host.py::_emulate's arithmetic."""
    payload = bytes(buf[s + 12 : e - 4])
    ents = []
    for k in range(int(tp[K_NE])):
        e0, rank, cw, pos = (int(v) for v in tp[K_ENT + 4 * k : K_ENT + 4 * k + 4])
        slot, mode, ln = e0 & 0xFF, (e0 >> 8) & 0xF, e0 >> 16
        key, kind = shape.keys[shape.slots[slot][0]], shape.slots[slot][1]
        if mode in (1, 2):
            x = int.from_bytes(bytes(buf[e - 4 * W + pos : e - 4 * W + pos + 4]), "little")
            if mode == 1:
                x &= (1 << (8 * ln)) - 1 if ln < 4 else 0xFFFFFFFF
                x = (x & 0x7F) | ((x >> 1) & 0x3F80) | ((x >> 2) & 0x1FC000) | ((x >> 3) & 0xFE00000)
            vals = [x]
        elif mode == 3:
            vals = [(((e + pos) & 0xFFFFFFFF) - (s + 12), ln)]
        else:
            vals = _list_values(payload, pos, ln, kind)
        assert cw == (INLINE_COUNT if mode else len(vals))
        ents.append((rank, (key, KIND_NAME[kind], vals)))
    ents.sort()
    assert [r for r, _ in ents] == list(range(1, len(ents) + 1))
    return [x for _, x in ents]


def _dict_or_none(shape, tp, W, buf, s, e):
    """template_dict, or None where the template's entries do not even fit the bytes (a wrong hit)."""
    try:
        return template_dict(shape, tp, W, buf, s, e)
    except (AssertionError, IndexError, struct.error):
        return None


def _homes(shape, tpls, W, crc) -> list[int]:
    """The template each variant's clean base record hits."""
    out = []
    for v in range(shape.variants):
        _, buf, st, en = M.place(shape, [shape.payload(v, M.BASE_I)], synth.framed, crc)
        j = int(M.mutant_index(1)[0])
        t = _hit(tpls, W, buf, int(st[j]), int(en[j]), nocrc=True)[0]
        assert t >= 0 and int(tpls[t][K_L]) == shape.lengths[v] and _hit(tpls, W, buf, int(st[j]), int(en[j]))[0] == t
        out.append(t)
    assert len(set(out)) == shape.variants
    return out


@pytest.mark.parametrize("crc", [True, False], ids=["spec", "zero"])
@pytest.mark.parametrize("name", ["S16", "S32", "S64"])
def test_mask_sweep(name, crc):
    shape = M.SHAPES[name]
    M.check_shape(shape)
    tpls, W = learned(name, crc)
    assert W == shape.W and len(tpls) == shape.variants
    assert [int(t[K_FRAME]) for t in tpls] == [0 if crc else 1] * len(tpls)
    if name == "S16":  # at least 3 templates, two of them on one length chain
        assert len(tpls) >= 3 and sorted(int(t[K_L]) for t in tpls) == [41, 42, 42, 43]
    home = _homes(shape, tpls, W, crc)
    orc = O.Oracle()
    moved = set(EXCEPTIONS[name])
    n_kind, n_hit = {}, {m: 0 for m, _ in MODES}
    wrong_dict, missed_benign, hit_structural, zero_crc = [], [], [], []
    total = 0
    for part, (buf, st, en, idx, muts) in batches(name, crc).items():
        total += len(muts)
        # the clean records of the batch all hit (from the first whose window lies in the batch)
        if part == "benign":
            for j in sorted(set(range(len(st))) - set(idx.tolist())):
                if int(en[j]) >= 4 * W:
                    assert _hit(tpls, W, buf, int(st[j]), int(en[j]), nocrc=True)[0] >= 0, j
        for j, m in zip(idx.tolist(), muts):
            s, e = int(st[j]), int(en[j])
            assert e >= 4 * W
            payload = bytes(buf[s + 12 : e - 4])
            ost, _, oent = orc.decode(payload, views=True)
            n_kind[m.kind] = n_kind.get(m.kind, 0) + 1
            n_kind["keys"] = n_kind.get("keys", 0) + m.is_key
            tag = (name, m.variant, m.pos, hex(m.value), m.role)
            for mode, nocrc in MODES:
                t = _hit(tpls, W, buf, s, e, nocrc=nocrc)[0]
                n_hit[mode] += t >= 0
                if crc and not nocrc:  # the guarded mode: the payload CRC, or the frame's own bytes
                    assert t == -1, tag
                    continue
                if t >= 0 and (ost != 0 or oent != _dict_or_none(shape, tpls[t], W, buf, s, e)):
                    wrong_dict.append(tag + (mode, f"oracle status {ost}"))
                if m.kind == M.BENIGN and (m.variant, m.pos, m.value) not in moved:
                    if not nocrc and O.masked_crc32c(payload) == 0:
                        zero_crc.append(tag)  # (the hit rule leaves such a record to the walk)
                    elif t != home[m.variant]:
                        missed_benign.append(tag + (mode, t))
                if (m.kind == M.STRUCTURAL or m.in_length_field or m.role == "lcrc") and t != -1:
                    hit_structural.append(tag + (mode, t))
    assert total == sum(len(M.values_at(b)) for v in range(shape.variants)
                        for b in _framed_base(shape, v, crc)), "no mutant left out"
    print(f"\n{name} {'spec' if crc else 'zero-CRC'} frames: W {W}, {len(tpls)} templates, {total} mutants: "
          f"{n_kind.get(M.BENIGN, 0)} benign, {n_kind.get(M.STRUCTURAL, 0)} structural "
          f"({n_kind.get('keys', 0)} in keys), {n_kind.get(M.FRAME, 0)} frame; hits "
          + ", ".join(f"{m} {n_hit[m]}" for m, _ in MODES) + f"; exceptions {list(EXCEPTIONS[name])}")
    assert not wrong_dict, f"a hit whose dict is not the oracle's: {wrong_dict[:12]}"
    assert not zero_crc, zero_crc
    assert not missed_benign, f"benign mutants that miss: {missed_benign[:12]}"
    assert not hit_structural, f"structural mutants that hit: {hit_structural[:12]}"


def _framed_base(shape, v, crc) -> bytes:
    buf, st, en = synth.framed([shape.payload(v, M.BASE_I)], crc)
    return bytes(buf[int(st[0]) : int(en[0])])


ROLES = {"S16": {"inline-varint", "bytes"},
         "S32": {"inline-varint", "list-varint-1", "list-varint-2", "list-varint-10", "inline-float", "bytes"},
         "S64": {"inline-varint", "list-varint-1", "list-varint-2", "list-varint-5", "list-varint-10", "inline-float",
                 "list-float", "bytes"}}


@pytest.mark.parametrize("name", ["S16", "S32", "S64"])
def test_sweep_is_not_vacuous(name):
    """On the byte maps and the oracle alone: every class of mutant occurs, benign ones in every kind
    of value, and the oracle tells benign from structural."""
    shape = M.SHAPES[name]
    orc = O.Oracle()
    muts = M.all_mutants(shape, synth.framed, False)
    by = {k: [m for m in muts if m.kind == k] for k in (M.BENIGN, M.STRUCTURAL, M.FRAME)}
    assert all(by.values()) and any(m.is_key for m in by[M.STRUCTURAL])
    assert {m.role for m in by[M.BENIGN]} == ROLES[name]
    tenth = [m for m in by[M.BENIGN] if m.role == "list-varint-10" and m.was == 0x01]
    assert name == "S16" or (tenth and all(m.value == 0x00 for m in tenth))  # (the negative value's last byte)

    def status(m):
        p = bytearray(shape.payload(m.variant, M.BASE_I))
        p[m.pos - 12] = m.value
        return orc.decode(bytes(p))[0]

    ok = sum(status(m) == 0 for m in by[M.BENIGN])
    assert ok == len(by[M.BENIGN])  # (every one: at least half is what the sweep needs)
    assert sum(status(m) != 0 for m in by[M.STRUCTURAL]) >= 1


@pytest.mark.parametrize("crc", [True, False], ids=["spec", "zero"])
def test_chain_records_hit_their_own_template(crc):
    """S16's two templates of payload length 42: a record of one whose value bytes are the other's
    structure bytes at the same window position hits its own template -- for one of the two the second
    on the length chain -- and its dict is the oracle's."""
    shape = M.S16
    tpls, W = learned("S16", crc)
    chain = [t for t in range(len(tpls)) if int(tpls[t][K_L]) == 42]
    recs, dressed = M.chain_records(shape)
    _, buf, st, en = M.place(shape, recs, synth.framed, crc)
    orc = O.Oracle()
    hits = set()
    for j in M.mutant_index(len(recs)).tolist():
        s, e = int(st[j]), int(en[j])
        for _, nocrc in MODES:
            t = _hit(tpls, W, buf, s, e, nocrc=nocrc)[0]
            assert t in chain, j
            ost, _, oent = orc.decode(bytes(buf[s + 12 : e - 4]), views=True)
            assert ost == 0 and oent == template_dict(shape, tpls[t], W, buf, s, e), j
            hits.add(t)
    assert len(chain) == 2 and hits == set(chain) and dressed >= 1
