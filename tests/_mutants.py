"""Record shapes and one-byte mutants for the mask-only template sweeps
(tests/test_tpl_mask_sweep_host.py, tests/test_tpl_mask_sweep_gpu.py). No GPU and no native code:
payloads come from the tests.golden.gen_golden builders, the framing from the caller (synth.framed).

Shapes (tfrg_layout.h picks the window W from the longest payload L: W = 16 for L <= 48, 32 for
L <= 112, 64 for L <= 240):

* S16: C1-like, `label` one int64 of 1 or 2 varint bytes (127 / 128), `id` one bytes value of 11 or
  12 bytes: four variants with payloads of 41, 42, 42 and 43 bytes, so two templates share the
  length chain of 42.
* S32: `n` inline int64 (1 or 2 bytes), `w` inline float, `v` an int64 list of a 1-byte, a 2-byte and
  a negative (10-byte) varint, `id` one bytes value of 5 or 8 bytes: two variants.
* S64: S32 plus `e`, a float list of 16, and `g`, an int64 list of one 5-byte varint (too long for
  the inline mode: a list location): two variants.

Every payload byte has a role, written down by the encoder below beside the byte itself (and the
bytes are asserted equal to the gen_golden builders'): the class of a role is `content` (inside a
bytes element or a float), `varint-low` (a packed or inline int64 byte) or `structure` (tags, lengths,
keys). The 16 frame bytes have the roles `len`, `lcrc` and `dcrc`.

Mutants: for each variant one base record (record index BASE_I of the variant); for every position p
of its framed bytes [0, L + 16) the values {b ^ 0x01, b ^ 0x80, 0x00, 0xFF} that differ from the
byte b there. A payload mutant is benign where the role's class is content, or varint-low with bit 7
unchanged; every other payload mutant is structural; the mutants of the 16 frame bytes are frame
mutants. Key bytes are structural; they are kept apart (`keys`), since each one that still decodes
adds a key to the decoder's schema.

A batch holds the mutant of list index k as record 5 k + 2 -- the variant's base record with that
one byte changed in the framed image, after the frame's CRCs were computed -- among clean records
whose values differ from record to record; 130 clean records follow the last mutant. starts / ends
are those of the clean image.
"""

from __future__ import annotations

import struct
from dataclasses import dataclass

import numpy as np

from tests.golden.gen_golden import byt, enc, entry, example, f32, i64

CONTENT, VARINT, STRUCTURE = "content", "varint-low", "structure"
BENIGN, STRUCTURAL, FRAME = "benign", "structural", "frame"
BASE_I = 77
STRIDE, OFFSET, TAIL = 5, 2, 130


def role_class(role: str) -> str:
    if role in ("bytes", "inline-float", "list-float"):
        return CONTENT
    if role == "inline-varint" or role.startswith("list-varint-"):
        return VARINT
    assert role in ("tag", "key"), role
    return STRUCTURE


# ---------------------------------------------------------------------------------------------------
# the encoder with roles: [(byte, role)]
# ---------------------------------------------------------------------------------------------------
def _tagged(fn: int, body: list) -> list:
    return [(b, "tag") for b in enc((fn << 3) | 2) + enc(len(body))] + body


def _feature(kind: str, vals: list) -> list:
    if kind == "bytes":
        return _tagged(1, [x for v in vals for x in _tagged(1, [(b, "bytes") for b in v])])
    if kind == "float":  # values are float32 bit patterns
        role = "inline-float" if len(vals) == 1 else "list-float"
        return _tagged(2, _tagged(1, [(b, role) for v in vals for b in struct.pack("<I", v)]))
    body = []
    for v in vals:
        e = enc(v)
        role = "inline-varint" if len(vals) == 1 and len(e) <= 4 else f"list-varint-{len(e)}"
        body += [(b, role) for b in e]
    return _tagged(3, _tagged(1, body))


def encode(feats: list) -> tuple[bytes, list[str]]:
    """[(key, kind, values)] -> (payload, role of every byte); the payload is gen_golden's."""
    ents = [_tagged(1, _tagged(1, [(b, "key") for b in key]) + _tagged(2, _feature(kind, vals)))
            for key, kind, vals in feats]
    pairs = _tagged(1, [x for e in ents for x in e])
    payload = bytes(b for b, _ in pairs)

    def feat(kind, vals):
        if kind == "bytes":
            return byt(*vals)
        if kind == "float":
            return f32(*[struct.unpack("<f", struct.pack("<I", v))[0] for v in vals])
        return i64(*vals)

    assert payload == example(*[entry(key, feat(kind, vals)) for key, kind, vals in feats])
    return payload, [r for _, r in pairs]


# ---------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------
def _fbits(i: int, k: int = 0) -> int:
    """A normal float32 in [0.5, 1) whose mantissa depends on (i, k)."""
    return 0x3F000000 | ((i * 2654435761 + k * 40503 + 12345) & 0x7FFFFF)


def _s16(v: int, i: int) -> list:
    label = 128 + i % 872 if v & 1 else 1 + i % 127
    ident = (b"img-%08d" if v & 2 else b"im-%08d") % (i % 10**8)
    return [(b"label", "int64", [label]), (b"id", "bytes", [ident])]


def _s32(v: int, i: int) -> list:
    n = 130 + i % 800 if v else 3 + i % 120
    ident = (b"r%07d" if v else b"r%04d") % (i % 10**4)
    return [(b"n", "int64", [n]), (b"w", "float", [_fbits(i)]),
            (b"v", "int64", [1 + i % 126, 128 + i % 900, -(1 + i % 8)]), (b"id", "bytes", [ident])]


def _s64(v: int, i: int) -> list:
    return _s32(v, i) + [(b"e", "float", [_fbits(i, 1 + k) for k in range(16)]),
                         (b"g", "int64", [(1 << 28) + (i * 7919) % (1 << 30)])]


@dataclass(frozen=True)
class Shape:
    name: str
    W: int
    variants: int
    lengths: tuple  # the payload length of each variant
    keys: tuple  # key bytes in record order
    slots: tuple  # (key index, kind code 1 bytes / 2 float / 3 int64) per slot
    feats: object

    def record(self, v: int, i: int) -> tuple[bytes, list[str]]:
        return encode(self.feats(v, i))

    def payload(self, v: int, i: int) -> bytes:
        return self.record(v, i)[0]

    def clean(self, n: int) -> list[bytes]:
        """n clean records: record j is of variant j % variants, with the values of index j."""
        return [self.payload(j % self.variants, j) for j in range(n)]


S16 = Shape("S16", 16, 4, (41, 42, 42, 43), (b"label", b"id"), ((0, 3), (1, 1)), _s16)
S32 = Shape("S32", 32, 2, (70, 74), (b"n", b"w", b"v", b"id"), ((0, 3), (1, 2), (2, 3), (3, 1)), _s32)
S64 = Shape("S64", 64, 2, (162, 166), (b"n", b"w", b"v", b"id", b"e", b"g"),
            ((0, 3), (1, 2), (2, 3), (3, 1), (4, 2), (5, 3)), _s64)
SHAPES = {s.name: s for s in (S16, S32, S64)}


def check_shape(shape: Shape) -> None:
    """The lengths, windows and byte maps the sweeps rely on (asserted, not assumed)."""
    lo, hi = {16: (0, 48), 32: (48, 112), 64: (112, 240)}[shape.W]
    for v in range(shape.variants):
        maps = set()
        for i in (0, 1, BASE_I, 500, 4999):
            p, roles = shape.record(v, i)
            assert len(p) == shape.lengths[v] == len(roles) and lo < len(p) <= hi, (shape.name, v, len(p))
            maps.add(tuple(roles))
        assert len(maps) == 1, "a variant's records share one byte map"
    if shape is S16:
        assert shape.lengths[1] == shape.lengths[2] and len(set(shape.lengths)) == 3


# ---------------------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Mutant:
    variant: int
    pos: int  # byte of the framed record: [0, 8) length, [8, 12) length CRC, payload, 4 bytes data CRC
    was: int
    value: int
    role: str
    kind: str  # BENIGN / STRUCTURAL / FRAME

    @property
    def is_key(self) -> bool:
        return self.role == "key"

    @property
    def in_length_field(self) -> bool:
        return self.role == "len"


def values_at(b: int) -> list[int]:
    out = []
    for x in (b ^ 0x01, b ^ 0x80, 0x00, 0xFF):
        if x != b and x not in out:
            out.append(x)
    return out


def frame_roles(roles: list[str]) -> list[str]:
    return ["len"] * 8 + ["lcrc"] * 4 + list(roles) + ["dcrc"] * 4


def mutant_set(shape: Shape, variant: int, framed_record: bytes) -> list[Mutant]:
    """Every (position, value) mutant of the variant's base record, whose framed bytes the caller passes."""
    payload, roles = shape.record(variant, BASE_I)
    assert framed_record[12:-4] == payload and len(framed_record) == len(payload) + 16
    assert int.from_bytes(framed_record[:8], "little") == len(payload)
    out = []
    for p, (b, role) in enumerate(zip(framed_record, frame_roles(roles))):
        for x in values_at(b):
            if role in ("len", "lcrc", "dcrc"):
                kind = FRAME
            elif role_class(role) == CONTENT or (role_class(role) == VARINT and not (x ^ b) & 0x80):
                kind = BENIGN
            else:
                kind = STRUCTURAL
            out.append(Mutant(variant, p, b, x, role, kind))
    assert len(out) == sum(len(values_at(b)) for b in framed_record)
    return out


def all_mutants(shape: Shape, framed, crc: bool) -> list[Mutant]:
    """The mutant sets of every variant; framed(payloads, crc) -> (image, starts, ends)."""
    out = []
    for v in range(shape.variants):
        buf, st, en = framed([shape.payload(v, BASE_I)], crc)
        out += mutant_set(shape, v, bytes(buf[int(st[0]) : int(en[0])]))
    return out


def split(muts: list[Mutant], moved: tuple = ()) -> dict[str, list[Mutant]]:
    """benign / hostile / keys; `moved`: benign mutants (variant, pos, value) that go to hostile."""
    out = {"benign": [], "hostile": [], "keys": []}
    for m in muts:
        if m.is_key:
            out["keys"].append(m)
        elif m.kind == BENIGN and (m.variant, m.pos, m.value) not in moved:
            out["benign"].append(m)
        else:
            out["hostile"].append(m)
    assert sum(len(v) for v in out.values()) == len(muts)
    return out


def batch_len(n_mutants: int) -> int:
    return (STRIDE * (n_mutants - 1) + OFFSET + 1 if n_mutants else 0) + TAIL


def mutant_index(n_mutants: int) -> np.ndarray:
    return STRIDE * np.arange(n_mutants, dtype=np.int64) + OFFSET


def place(shape: Shape, records: list[bytes], framed, crc: bool):
    """records[k] (a whole payload) as record 5 k + 2 among clean ones: (payloads, image, starts, ends)."""
    n = batch_len(len(records))
    payloads = shape.clean(n)
    for j, p in zip(mutant_index(len(records)).tolist(), records):
        payloads[j] = p
    buf, st, en = framed(payloads, crc)
    return payloads, buf.copy(), st, en


def batch(shape: Shape, muts: list[Mutant], framed, crc: bool):
    """The batch of `muts`: (image, starts, ends, record index of every mutant)."""
    base = [shape.payload(v, BASE_I) for v in range(shape.variants)]
    _, buf, st, en = place(shape, [base[m.variant] for m in muts], framed, crc)
    idx = mutant_index(len(muts))
    for j, m in zip(idx.tolist(), muts):
        s, e = int(st[j]), int(en[j])
        assert e - s == shape.lengths[m.variant] + 16 and int(buf[s + m.pos]) == m.was != m.value
        buf[s + m.pos] = m.value
    assert len(st) == batch_len(len(muts)) and int(en[-1]) == buf.size
    return buf, st, en, idx


def groups_of(idx) -> set[int]:
    """The 64-record groups (k_tpl_lane's wavefronts) that hold the records idx."""
    return {int(j) >> 6 for j in idx}


# ---------------------------------------------------------------------------------------------------
# the chain case (S16): records of one template of the shared length dressed as the other
# ---------------------------------------------------------------------------------------------------
def chain_records(shape: Shape, n_each: int = 40) -> tuple[list[bytes], int]:
    """For each ordered pair (a, b) of variants of one payload length: records of a whose bytes take
    b's base bytes wherever the position is content or varint-low in a and structure in b (a varint
    byte keeps its own bit 7: that bit is a's structure). Returns (payloads, positions dressed)."""
    out, dressed = [], 0
    pairs = [(a, b) for a in range(shape.variants) for b in range(shape.variants)
             if a != b and shape.lengths[a] == shape.lengths[b]]
    assert pairs
    for a, b in pairs:
        other, roles_b = shape.record(b, BASE_I)
        for i in range(n_each):
            p, roles_a = shape.record(a, 1000 + 37 * i)
            q = bytearray(p)
            n = 0
            for k, (ra, rb) in enumerate(zip(roles_a, roles_b)):
                if role_class(ra) != STRUCTURE and role_class(rb) == STRUCTURE:
                    q[k] = other[k] if role_class(ra) == CONTENT else (p[k] & 0x80) | (other[k] & 0x7F)
                    n += 1
            assert n >= 1, "the two templates of the chain differ in where their structure lies"
            dressed = max(dressed, n)
            out.append(bytes(q))
    return out, dressed
