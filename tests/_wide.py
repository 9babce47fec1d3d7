"""Wide schemas (past 64 slots, 256 slots and 256 keys): generators, the pinned kernel constants and
the full comparison, for tests/test_wide_host.py and tests/test_wide_schema_gpu.py. Test
infrastructure: no GPU.

The decode changes path with the size of the key table: the lane kernel's dictionary
(``lane_count_mode`` in csrc/tfrg_kernels.hip: 0 per-lane dicts in LDS, 1 MaskSink up to 64 slots,
2 the global columns), the LDS key table (``schema_in_lds``: up to ``kLdsMaxKeys`` keys), the
second 64-slot loop of the staged gather, the 256-slot passes of the spine. Which wave gather takes
a record above lane_max is decided by its size against kWStage (``wave_route``), so the dense
records come in two sizes: ``dense_batch`` (beyond kWStage from 64 slots on: ``role_wave_gather``)
and ``stage_batch`` (within it at every width: ``role_stage_gather``). The mode is not exposed:
``expected_mode`` is a port of the host code that picks it, over constants read from the sources,
and ``PINNED`` holds the values the case table was laid out for, so that a retune fails
``test_wide_host.py::test_pinned_constants`` by name instead of moving the cases off their
boundaries.
"""

from __future__ import annotations

import re
import struct
from functools import lru_cache
from pathlib import Path

import numpy as np

from oracle import oracle as O
from tests import _golden as G
from tests.golden.gen_golden import byt, enc, entry, example, i64, ld
from tfr_reader import _status as S
from tfr_reader import synth

CSRC = Path(__file__).resolve().parents[1] / "tfrecords-reader_amd" / "csrc"

KIND = {1: "bytes_list", 2: "float_list", 3: "int64_list"}
KIND_ID = {v: k for k, v in KIND.items()}

#: list lengths of the dense records, cycled per slot and per record: empty, an inline single value,
#: short lists, and 200 values (past the wave-cooperative threshold of the int64 gathers)
CYCLE = (0, 1, 2, 5, 40, 200)
#: lengths of the bytes elements
BYTES_LENS = (0, 1, 127, 128, 300)
#: records of every sweep batch: two tiles, a ragged last 64-record group, a ragged last tile
N_RECORDS = 321

#: the values the case table was laid out for (test_pinned_constants)
PINNED = {
    "kLdsMaxKeys": 256, "kLdsMaxHt": 1024, "kLaneLdsBudget": 65536, "kLaneCountBlock": 256,
    "kStageBytes": 4096, "kStageStride": 4160, "kLaneSlice": 4, "kLaneRep": 1, "kKrWords": 8,
    "kSpecTgtWords": 8, "kSpineBlock": 256, "kLeanMaxSlots": 16, "kWStage": 12288,
}


# ------------------------------------------------------------------------------- pinned constants
@lru_cache(maxsize=None)
def kernel_constants() -> dict[str, int]:
    """The constants as the sources build with them, read by regex (tests/_bytes_ref.py does the
    same for the bytes column), and the two host formulas ``expected_mode`` ports, checked to still
    be spelled the way they were ported."""
    kern = (CSRC / "tfrg_kernels.hip").read_text()
    intr = (CSRC / "tfrg_internal.h").read_text()
    scan = (CSRC / "tfrg_scan.hip").read_text()
    lay = (CSRC / "tfrg_layout.h").read_text()
    capi = (CSRC / "tfrg_capi.cpp").read_text()

    def const(text: str, name: str) -> int:
        m = re.search(rf"\b{name} = (\d+)(?: \* (\d+))?;", text)
        assert m, f"{name} is no longer a literal"
        return int(m.group(1)) * int(m.group(2) or 1)

    c = {name: const(intr, name) for name in ("kLdsMaxKeys", "kLdsMaxHt")}
    for name in ("kLaneLdsBudget", "kLaneCountBlock", "kStageBytes", "kLaneSlice", "kLaneRep", "kSpecTgtWords",
                 "kWStage"):
        c[name] = const(kern, name)
    m = re.search(r"\bkStageStride = kStageBytes \+ (\d+);", kern)
    assert m, "kStageStride is no longer kStageBytes + slack"
    c["kStageStride"] = c["kStageBytes"] + int(m.group(1))
    m = re.search(r"enum KeyRec : uint32_t \{([^}]*)\}", intr)
    assert m, "enum KeyRec moved"
    names = [x.split("=")[0].strip() for x in m.group(1).split(",")]
    c["kKrWords"] = names.index("kKrWords")  # (the enumerators count from 0: the last one is their number)
    c["kSpineBlock"] = const(scan, "kSpineBlock")
    c["kLeanMaxSlots"] = const(lay, "kLeanMaxSlots")
    # the code expected_mode / ht_size / schema_in_lds port
    for text, line in (
        (kern, "return tab_lds + lane_count_lds(sc, 0) <= kLaneLdsBudget ? 0 : sc.n_slots <= 64 ? 1 : 2;"),
        (kern, "const size_t tab_lds = 256ull * kLaneSlice * kLaneRep * 4;"),
        (kern, "const size_t dict = mode == 0 ? S * kLaneCountBlock * 4 + r16(S * kLaneCountBlock * 2) : 0;"),
        (kern, "const size_t stage = (size_t)kStageStride * (kLaneCountBlock / 64);"),
        (kern, "const size_t keys = fast_ok ? (((size_t)sc.ht_mask + 4) / 4 * 4 + (size_t)sc.n_keys * kKrWords) * 4 : 0;"),
        (kern, "const size_t spec = mode == 0 && fast_ok && sc.spec ? ((S + 7) & ~(size_t)7) * 4 + S * kSpecTgtWords * 4 : 0;"),
        (intr, "return sc.n_keys <= kLdsMaxKeys && sc.ht_mask + 1 <= kLdsMaxHt;"),
        (capi, "while (hsz < 2 * n_keys + 2) hsz <<= 1;"),
        # wave_route: which wave gather takes a record above lane_max
        (kern, "big = v.status == TFRG_OK && v.e - v.st > lane_max;"),
        (kern, "if (v.e - (v.st & ~15ull) <= wave_stage) {"),
        (kern, "cfg.wave_stage < kWStage ? cfg.wave_stage : kWStage, defer_big ? 1u : 0u);"),
    ):
        assert line in text, f"ported host code changed: {line}"
    return c


def ht_size(n_keys: int) -> int:
    """Entries of the open-addressing key table (tfrg_set_schema)."""
    hsz = 16
    while hsz < 2 * n_keys + 2:
        hsz <<= 1
    return hsz


def schema_in_lds(n_keys: int) -> bool:
    c = kernel_constants()
    return n_keys <= c["kLdsMaxKeys"] and ht_size(n_keys) <= c["kLdsMaxHt"]


def lane_count_lds(n_keys: int, n_slots: int, spec: bool, mode: int) -> int:
    c = kernel_constants()
    blk = c["kLaneCountBlock"]
    fast_ok = schema_in_lds(n_keys)
    r16 = lambda x: (x + 15) & ~15  # noqa: E731
    dict_ = n_slots * blk * 4 + r16(n_slots * blk * 2) if mode == 0 else 0
    stage = c["kStageStride"] * (blk // 64)
    keys = ((ht_size(n_keys) - 1 + 4) // 4 * 4 + n_keys * c["kKrWords"]) * 4 if fast_ok else 0
    tsl = (blk // 64) * 64 * 4 if mode == 1 else 0
    sp = ((n_slots + 7) & ~7) * 4 + n_slots * c["kSpecTgtWords"] * 4 if mode == 0 and fast_ok and spec else 0
    return dict_ + stage + keys + tsl + sp


def expected_mode(n_keys: int, n_slots: int, spec: bool = False) -> int:
    """``lane_count_mode`` of a key table with ``n_keys`` keys and ``n_slots`` slots (``spec``: the
    context holds a speculative placement, DevSchema::spec)."""
    c = kernel_constants()
    tab = 256 * c["kLaneSlice"] * c["kLaneRep"] * 4
    if tab + lane_count_lds(n_keys, n_slots, spec, 0) <= c["kLaneLdsBudget"]:
        return 0
    return 1 if n_slots <= 64 else 2


def wave_route(st, en, lane_max: int, wave_stage: int | None = None) -> tuple[int, int, int]:
    """(lane records, staged records, huge records) of a batch of well-framed records, as
    ``k_lane_count`` routes them: a record above ``lane_max`` is a large one (tfrg_info.n_big counts
    both sorts); one spanning at most min(``wave_stage``, kWStage) bytes from the 16-byte boundary
    below its start is listed for ``role_stage_gather``, a larger one for ``role_wave_gather``
    (a large record whose values are all inline is listed for neither). ``wave_stage`` None: the
    context's default, no limit of its own."""
    lim = kernel_constants()["kWStage"]
    if wave_stage is not None:
        lim = min(lim, wave_stage)
    st, en = np.asarray(st, np.int64), np.asarray(en, np.int64)
    big = (en - st) > lane_max
    staged = big & ((en - (st & ~15)) <= lim)
    return int((~big).sum()), int(staged.sum()), int((big & ~staged).sum())


def largest_mode0() -> int:
    """The largest one-kind-per-key schema the lane kernel still decodes with per-lane dicts in LDS
    (no speculative placement), found by search."""
    m = 1
    while expected_mode(m + 1, m + 1) == 0:
        m += 1
    return m


def sweep_cases() -> list[tuple[int, int, int]]:
    """(keys, slots, lane mode) of the schema sweep."""
    m0 = largest_mode0()
    return [(m0, m0, 0), (m0 + 1, m0 + 1, 1), (64, 64, 1), (65, 65, 2), (128, 128, 2), (129, 129, 2),
            (100, 300, 2), (256, 256, 2), (256, 257, 2), (257, 257, 2), (300, 300, 2)]


def key_hash_words(key: bytes) -> int:
    """The host branch of ``key_hash_words`` (csrc/tfrg_internal.h) over ``key_words`` of the key."""
    n = len(key)
    w0 = int.from_bytes(key[:4], "little")
    w1 = int.from_bytes(key[n - 4 :], "little") if n > 4 else 0
    a = (w0 ^ (w0 >> 11) ^ (n << 17)) & 0xFFFFFF
    b = (w1 ^ (w1 >> 13) ^ (n << 7)) & 0xFFFFFF
    h = ((a * 0x9E3779) & 0xFFFFFFFF) ^ ((b * 0x85EBCB) & 0xFFFFFFFF)
    return h ^ (h >> 15)


# ---------------------------------------------------------------------------------------- schemas
def key_name(j: int) -> bytes:
    """Key j of a schema. Of every 8 names one is short (at most 8 bytes: the hash triple is the key
    itself; every other one of them exactly 8 bytes), one long, and six form three pairs that share
    length, first 4 and last 4 bytes (identical ``key_hash_words``: only the byte compare of the key
    table tells them apart)."""
    q, r = divmod(j, 8)
    if r == 0:
        return f"k{j:07d}".encode() if q % 2 else f"s{j}".encode()
    if r == 1:
        return f"long_key_{j:04d}_x".encode()
    g = 3 * q + (r - 2) // 2
    return f"feat_{'AAAA' if r % 2 == 0 else 'BBBB'}_{g:04d}".encode()


def schema(n_keys: int, kinds_per_key=1) -> tuple[list[bytes], list[tuple[bytes, int]]]:
    """Key names and (key, kind) slots. ``kinds_per_key`` (an int, or one int per key) is the number
    of kinds, 1 to 3, a key holds in different records: the slot count is controlled apart from the
    key count. Key j's first kind is 1 + j % 3, so the kinds interleave and the two names of a
    colliding pair (consecutive j) never share one."""
    per = [kinds_per_key] * n_keys if isinstance(kinds_per_key, int) else list(kinds_per_key)
    assert len(per) == n_keys and all(1 <= p <= 3 for p in per)
    names = [key_name(j) for j in range(n_keys)]
    assert len(set(names)) == n_keys
    slots = [(names[j], 1 + (j + t) % 3) for j in range(n_keys) for t in range(per[j])]
    return names, slots


def schema_for(n_keys: int, n_slots: int):
    """A schema of ``n_keys`` keys and ``n_slots`` slots: the extra slots dealt to the first keys."""
    per = [1] * n_keys
    for e in range(n_slots - n_keys):
        per[e % n_keys] += 1
    return schema(n_keys, per)


def key_kinds(slots) -> dict[bytes, list[int]]:
    out: dict[bytes, list[int]] = {}
    for key, kind in slots:
        out.setdefault(key, []).append(kind)
    return out


def colliding_groups(names) -> list[list[bytes]]:
    """Groups of at least two names longer than 8 bytes with equal length, first 4 and last 4 bytes."""
    by: dict[tuple, list[bytes]] = {}
    for nm in names:
        if len(nm) > 8:
            by.setdefault((len(nm), nm[:4], nm[-4:]), []).append(nm)
    return [g for g in by.values() if len(g) > 1]


# ------------------------------------------------------------------------------------ value pools
_VARIANTS = 16
_FLOAT_SPECIALS = (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FC12345, 0x7FA00000, 0xFFC00001,
                   0x00000001, 0x807FFFFF, 0x007FFFFF, 0x3F800000)


def f32_bits(bits) -> bytes:
    """A packed float_list of raw bit patterns."""
    return ld(2, ld(1, struct.pack(f"<{len(bits)}I", *bits)))


def _int_values(rng, m: int) -> list[int]:
    """Mixed varint widths (1 to 10 bytes), negatives included."""
    bits = rng.integers(1, 64, m)
    v = [int(x) for x in (rng.random(m) * (2.0**bits)).astype(np.uint64) % (1 << 63)]
    return [-x - 1 if rng.random() < 0.15 else x for x in v]


#: element lengths of the stageable batch's bytes lists
SMALL_BYTES_LENS = (0, 1, 2, 3, 9)


def _bytes_elems(rng, m: int, v: int, small: bool = False) -> list[bytes]:
    """Elements of the lengths BYTES_LENS. Lists of up to 5 elements cycle through all of them; in
    the long lists (40, 200) every 16th element is one of the three large lengths and the others are
    0 or 1 bytes, which keeps a 300-key record near 100 KB."""
    if small:
        lens = [SMALL_BYTES_LENS[(v + t) % 5] for t in range(m)]
    elif m <= 5:
        lens = [BYTES_LENS[(v + t) % 5] for t in range(m)]
    else:
        lens = [BYTES_LENS[2 + (v + t // 16) % 3] if t % 16 == v % 16 else (v + t) % 2 for t in range(m)]
    blob = rng.integers(0, 256, sum(lens) + 1, dtype=np.uint8).tobytes()
    out, at = [], 0
    for ln in lens:
        out.append(blob[at : at + ln])
        at += ln
    return out


@lru_cache(maxsize=None)
def pools(seed: int, cycle: tuple[int, ...], small_bytes: bool = False) -> dict:
    """(kind, list length) -> ``_VARIANTS`` encoded features, from a fixed seed; under ("values",
    list length) the int64 values themselves."""
    rng = np.random.default_rng(seed)
    out = {}
    for m in cycle:
        out["values", m] = [_int_values(rng, m) for _ in range(_VARIANTS)]  # (as encoded: 64-bit)
        out[3, m] = [i64(*v) for v in out["values", m]]
        fl = []
        for v in range(_VARIANTS):
            bits = [int(x) for x in rng.integers(0, 1 << 32, m, dtype=np.uint64)]
            for t in range(v % 3, m, 3):  # every third value a special: NaN payloads, -0.0, denormals
                bits[t] = _FLOAT_SPECIALS[(v + t) % len(_FLOAT_SPECIALS)]
            fl.append(f32_bits(bits))
        out[2, m] = fl
        out[1, m] = [byt(*_bytes_elems(rng, m, v, small_bytes)) for v in range(_VARIANTS)]
    return out


def _variant(s: int, i: int) -> int:
    return (s * 7 + i * 13) % _VARIANTS


# ---------------------------------------------------------------------------------------- batches
class Batch:
    """Framed records of one generated batch, three of them corrupted (a length CRC, a payload byte,
    a data CRC: ``corrupted``), a few malformed on purpose (``malformed``), and the oracle's outcome of
    every record (``ref``), computed once and shared by the tests that compare against it."""

    def __init__(self, payloads: list[bytes], malformed: list[int], corrupt: bool = True) -> None:
        self.payloads = payloads
        self.malformed = malformed
        n = len(payloads)
        if n:
            buf, self.st, self.en = synth.framed(payloads, crc=True)
            self.buf = buf.copy()
        else:  # an empty batch
            self.buf, self.st, self.en = np.zeros(16, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint64)
        # the three corrupted records: away from record 0 and from the malformed ones
        self.corrupted = {}
        if corrupt and n >= 40:
            for what, i in (("length_crc", n // 2 + 1), ("payload", n // 2 + 4), ("data_crc", n - 2)):
                while i in malformed:
                    i -= 1
                s, e = int(self.st[i]), int(self.en[i])
                if what == "length_crc":
                    self.buf[s + 8 + i % 4] ^= 0x10
                elif what == "payload":
                    self.buf[e - 5] ^= 0x01  # the record's last payload byte
                else:
                    self.buf[e - 4 + i % 4] ^= 0x80
                self.corrupted[what] = i
        self._ref = None

    def __len__(self) -> int:
        return len(self.payloads)

    @property
    def ref(self):
        if self._ref is None:
            self._ref = reference(self.buf, self.st, self.en, O.Oracle())
        return self._ref


def _malform(i: int, ents: list, keys: list[bytes], kinds: dict, pool: dict, small: bool) -> bool:
    """Records 5, 9 and 13 of every run of 107 records (never record 0) are malformed: an 11-byte
    varint in a packed int64 body (of a key at index 64 or above where the schema has one: every
    slot of such a key is numbered 64 or above), a duplicate key, a two-chunk packed list."""
    m = i % 107
    if i == 0 or m not in (5, 9, 13):
        return False
    if m == 5:
        hi = [k for k in keys[64:] if 3 in kinds[k]] or [k for k in keys if 3 in kinds[k]]
        if not hi:
            return False
        k = hi[i % len(hi)]
        body = enc(7) + enc(300) + b"\xff" * 10 + b"\x01" + (b"" if small else b"".join(enc(x) for x in range(90)))
        feat = ld(3, ld(1, body))
        pos = next((p for p, (kk, _) in enumerate(ents) if kk == k), None)
        if pos is None:
            ents.append((k, feat))
        else:
            ents[pos] = (k, feat)
    elif m == 9:
        k, _ = ents[0]
        ents.append((k, pool[kinds[k][0], 1][i % _VARIANTS]))
    else:
        ik = [k for k in keys if 3 in kinds[k]]
        if not ik:
            return False
        k = ik[i % len(ik)]
        a, b = (enc(1), enc(2)) if small else (b"".join(enc(x) for x in range(3)), b"".join(enc(-x) for x in range(70)))
        feat = ld(3, ld(1, a) + ld(1, b))
        pos = next((p for p, (kk, _) in enumerate(ents) if kk == k), None)
        if pos is None:
            ents.append((k, feat))
        else:
            ents[pos] = (k, feat)
    return True


def _keyed_batch(slots, n: int, seed: int, pool: dict, period: int, length_of, small: bool, malformed: bool,
                 corrupt: bool) -> Batch:
    """Every key present in every record, in schema order in the even records and shuffled in the odd
    ones. Key j carries kind ``kinds[j][(i // period + j) % len]`` in record i (one kind for ``period``
    records, so that every slot sees every list length); the list of slot s (schema order) in record
    i has ``length_of((s + i) % period)`` values, taken from the pools."""
    kinds = key_kinds(slots)
    keys = list(kinds)
    slot_ix = {sl: s for s, sl in enumerate(slots)}
    rng = np.random.default_rng(seed + 1000)
    out, bad, ints = [], [], []
    for i in range(n):
        ents, iv = [], {}
        for j, k in enumerate(keys):
            kd = kinds[k][(i // period + j) % len(kinds[k])]
            s = slot_ix[k, kd]
            m = length_of((s + i) % period)
            ents.append((k, pool[kd, m][_variant(s, i)]))
            if kd == 3:
                iv[k] = pool["values", m][_variant(s, i)]
        if malformed and _malform(i, ents, keys, kinds, pool, small):
            bad.append(i)
        if i % 2:
            ents = [ents[p] for p in rng.permutation(len(ents))]
        out.append(example(*[entry(k, f) for k, f in ents]))
        ints.append(iv)
    b = Batch(out, bad, corrupt)
    b.int_values = ints  # per record: int64 key -> the values as encoded (malformed records: not theirs)
    return b


def dense_batch(slots, n: int = N_RECORDS, seed: int = 1, long_len: int = 200, malformed: bool = True,
                corrupt: bool = True) -> Batch:
    """The large dense records: every key in every record (``_keyed_batch``), the list of slot s in
    record i ``CYCLE[(s + i) % 6]`` values long. From 64 slots on every record is larger than the
    wave kernels' LDS stage (kWStage): above ``lane_max`` these are ``role_wave_gather``'s records."""
    cyc = tuple(long_len if m == 200 else m for m in CYCLE)
    return _keyed_batch(slots, n, seed, pools(seed, cyc), len(cyc), lambda ph: cyc[ph], False, malformed, corrupt)


#: list lengths of the stageable dense records: real (out-of-line) lists of 2, 5 and 12 values
STAGE_LISTS = (2, 5, 12)


def stage_period(n_keys: int) -> int:
    """Records after which a slot's list lengths repeat in ``stage_batch``: 3 of them hold a real
    list, so about 3 keys in 6 (narrow schemas) down to 3 in ``n_keys // 10`` carry one per record."""
    return max(6, n_keys // 10)


def stage_batch(slots, n: int = N_RECORDS, seed: int = 4, malformed: bool = True, corrupt: bool = True) -> Batch:
    """Dense records that fit the wave kernels' LDS stage (kWStage bytes) however wide the schema:
    every key in every record (``_keyed_batch``), but only the phases 0, 1 and 2 of a slot's period
    (``stage_period``) hold a real list, of 2, 5 and 12 values; the other phases alternate between a
    single value (inline: ``k_down_gather`` writes it) and an empty list. Every slot of every kind,
    the slots at 64 and above included, thus holds out-of-line lists in some records, and above
    ``lane_max`` ``role_stage_gather`` gathers them. int64 values of every varint width, float bit
    patterns as in the large batch, bytes elements of 0 to 9 bytes."""
    period = stage_period(len(key_kinds(slots)))
    lens = (0, 1) + STAGE_LISTS
    pool = pools(seed, lens, small_bytes=True)
    return _keyed_batch(slots, n, seed, pool, period, lambda ph: STAGE_LISTS[ph] if ph < 3 else ph % 2, True,
                        malformed, corrupt)


#: keys per sparse record, cycled: 1 to 4, mostly 1, so that 64 records span less than the LDS stage
_SPARSE_COUNTS = (1, 1, 1, 2, 1, 1, 1, 3, 1, 1, 1, 2, 1, 1, 1, 4)


@lru_cache(maxsize=None)
def _sparse_pool(seed: int) -> dict:
    rng = np.random.default_rng(seed)
    out = {}
    for m in (0, 1, 2):
        out[3, m] = [i64(*[int(x) for x in rng.integers(0, 1 << 14, m)]) for _ in range(_VARIANTS)]
    for m in (0, 1):
        out[2, m] = [f32_bits([_FLOAT_SPECIALS[v % 12] if v % 2 else int(rng.integers(0, 1 << 32))] * m)
                     for v in range(_VARIANTS)]
        out[1, m] = [byt(*[bytes(rng.integers(0, 256, v % 4, dtype=np.uint8))] * m) for v in range(_VARIANTS)]
    return out


def sparse_batch(slots, n: int = N_RECORDS, seed: int = 2, malformed: bool = True, corrupt: bool = True) -> Batch:
    """Each record holds 1 to 4 random keys of the schema with lists of 0 to 2 small values: a
    wave's 64 records fit the lane kernel's LDS stage, the only way to the staged fast walk with a
    wide schema."""
    pool = _sparse_pool(seed)
    kinds = key_kinds(slots)
    keys = list(kinds)
    rng = np.random.default_rng(seed + 2000)
    out, bad = [], []
    for i in range(n):
        m = min(_SPARSE_COUNTS[i % len(_SPARSE_COUNTS)], len(keys))
        ents = []
        for j in rng.choice(len(keys), m, replace=False).tolist():
            k = keys[j]
            kd = kinds[k][int(rng.integers(0, len(kinds[k])))]
            ln = int(rng.integers(0, 3 if kd == 3 else 2))
            ents.append((k, pool[kd, ln][int(rng.integers(0, _VARIANTS))]))
        if malformed and _malform(i, ents, keys, kinds, {(kd, 1): pool[kd, 1] for kd in (1, 2, 3)}, True):
            bad.append(i)
        out.append(example(*[entry(k, f) for k, f in ents]))
    return Batch(out, bad, corrupt)


def narrow_batch(n: int, n_slots: int = 8, offset: int = 0) -> Batch:
    """Records of ``n_slots`` single-value slots (int64 below 2^28, float, short bytes, one kind
    per key, every key in every record, in one order): the shape whose values the decoder places
    speculatively. No malformed and no corrupted record."""
    out = []
    for i in range(offset, offset + n):
        ents = []
        for j in range(n_slots):
            kd = 1 + j % 3
            if kd == 3:
                f = i64((i * 31 + j) % (1 << 20))
            elif kd == 2:
                f = f32_bits([(0x3F800000 + i * 8 + j) & 0xFFFFFFFF])
            else:
                f = byt(f"n{i:06d}-{j}".encode())
            ents.append(entry(f"nar{j}".encode(), f))
        out.append(example(*ents))
    return Batch(out, [], corrupt=False)


def join(*batches: Batch) -> Batch:
    """The records of several batches as one (uncorrupted) batch."""
    return Batch([p for b in batches for p in b.payloads], [], corrupt=False)


def kinds_high_schema():
    """130 one-kind slots: slots 64 to 129 are bytes, float and int64 in turn (22 of each)."""
    names, slots = schema(130)
    assert [sum(1 for _, kd in slots[64:] if kd == k) for k in (1, 2, 3)] == [22, 22, 22]
    return names, slots


def high_cardinality_batch(n: int = 300) -> Batch:
    """Every record holds its own key ``k{i}`` with a list of 0 to 40 int64 values, beside a float
    list and a bytes list under two shared keys: ``n`` + 2 keys, past the LDS key table."""
    rng = np.random.default_rng(41)
    out = []
    for i in range(n):
        m = (0, 1, 7, 40, 3, 19)[i % 6]
        fl = [int(x) for x in rng.integers(0, 1 << 32, i % 9, dtype=np.uint64)]
        out.append(example(entry(f"k{i}".encode(), i64(*_int_values(rng, m))), entry(b"shared_f", f32_bits(fl)),
                           entry(b"shared_b", byt(*_bytes_elems(rng, i % 4, i)))))
    return Batch(out, [])


def tile_stride(n: int) -> int:
    """Words between two slots' tile sums in the scan buffer of an ``n``-record decode."""
    intr = (CSRC / "tfrg_internal.h").read_text()
    capi = (CSRC / "tfrg_capi.cpp").read_text()
    shift = int(re.search(r"\bkTileShift = (\d+);", intr).group(1))
    assert "const uint32_t tile_stride = (n_tiles + 3u) & ~3u;" in capi
    return (((n + (1 << shift) - 1) >> shift) + 3) & ~3


@lru_cache(maxsize=None)
def reuse_steps() -> tuple[Batch, ...]:
    """The batches one context decodes in turn while its key table grows and the batch size
    changes (the scan words' layout is [S][tile_stride], [S][n_chunks], [S] in one buffer that is
    not cleared between decodes): the first six; the seventh step decodes the first again."""
    s65 = schema(65)[1]
    s300 = schema(100, 3)[1]
    s257 = schema(257)[1]
    return (narrow_batch(1100, 8), dense_batch(s65, seed=5), sparse_batch(s300, 2900, seed=6),
            dense_batch(s257, 70, seed=7), dense_batch(s257, 1, seed=8, corrupt=False),
            Batch([], [], corrupt=False))


# ------------------------------------------------------------------------------------- comparison
def raw_entries(r, i: int):
    """[(key bytes, kind, values)] of record i straight from the columns (float values as raw bits)."""
    col = r.order[:, i]
    present = np.flatnonzero(col)
    present = present[np.argsort(col[present], kind="stable")]
    out = []
    for s in present.tolist():
        lo = int(r.slot_base[s] + r.row_splits[s, i])
        hi = int(r.slot_base[s] + r.row_splits[s, i + 1])
        kind = r.slot_kind[s]
        if kind == 3:
            vals = r.i64[lo:hi].tolist()
        elif kind == 2:
            vals = r.f32[lo:hi].tolist()
        else:
            vals = [r.buf[o : o + n].tobytes() for o, n in zip(r.bytes_off[lo:hi].tolist(), r.bytes_len[lo:hi].tolist())]
        out.append((r.slot_key[s].encode("utf-8"), KIND[kind], vals))
    return out


def reference(buf, st, en, orc) -> list[tuple]:
    """Per framed record: (oracle status, aux, canonical entries or None, length CRC ok, data CRC ok)."""
    raw = buf.tobytes()
    out = []
    for s, e in zip(np.asarray(st).tolist(), np.asarray(en).tolist()):
        payload = raw[s + 12 : e - 4]
        ost, aux, ent = orc.decode(payload)
        lc = O.masked_crc32c(raw[s : s + 8]) == struct.unpack("<I", raw[s + 8 : s + 12])[0]
        dc = O.masked_crc32c(payload) == struct.unpack("<I", raw[e - 4 : e])[0]
        out.append((ost, aux, G.canon_entries(ent) if ost == 0 else None, lc, dc))
    return out


#: statuses whose exception the reference defines (type and message, which for two of them hold aux)
_REF_ERRORS = frozenset(S.MESSAGES) | {S.ERR_WIRE_TYPE, S.ERR_KEY_UTF8, S.ERR_FEATURES_NONE}


def oracle_lengths(ref, n_records: int) -> dict[tuple[bytes, int], np.ndarray]:
    """(key, kind) -> the list length per record, from the oracle (a failed record holds nothing)."""
    out: dict[tuple[bytes, int], np.ndarray] = {}
    for i, (ost, _, ent, _, _) in enumerate(ref):
        if ost:
            continue
        for key, kind, vals in ent:
            a = out.get((key, KIND_ID[kind]))
            if a is None:
                a = out[key, KIND_ID[kind]] = np.zeros(n_records, np.int64)
            a[i] = len(vals)
    return out


def compare(r, buf, st, en, orc, ref=None, strict=False) -> list[str]:
    """Every record of result ``r`` against the oracle: status, aux (where the status is an error the
    reference defines), the entries in key order with their values, both CRC verdict bits; then per
    slot the row splits against the running sum of the oracle's list lengths, and the kind totals.
    ``ref``: ``reference(buf, st, en, orc)`` computed before. ``strict``: the decode ran with
    strict_crc, a record whose framing check fails carries ERR_CRC and holds nothing. Returns the
    mismatches (at most 20 of them)."""
    n = len(st)
    ref = reference(buf, st, en, orc) if ref is None else ref
    raw = None
    bad: list[str] = []
    if len(r) != n or int(r.info.n_records) != n:
        return [f"{len(r)} records, want {n}"]
    if strict:
        ref = [(ost or (0 if lc and dc else S.ERR_CRC), aux, ent if lc and dc else None, lc, dc)
               for ost, aux, ent, lc, dc in ref]
    for i, (ost, oaux, oent, lc, dc) in enumerate(ref):
        if len(bad) >= 20:
            break
        got = int(r.status[i])
        if got != ost:
            bad.append(f"record {i}: status {got} != oracle {ost}")
            continue
        if ost in _REF_ERRORS:
            if raw is None:
                raw = buf.tobytes()
            payload = raw[int(st[i]) + 12 : int(en[i]) - 4]
            if G.status_exception(got, int(r.aux[i]), payload) != G.status_exception(ost, oaux, payload):
                bad.append(f"record {i}: aux {int(r.aux[i])} != oracle {oaux} (status {ost})")
        if ost == 0:
            ent = G.canon_entries(raw_entries(r, i))
            if ent != oent:
                k = next((k for k, (a, b) in enumerate(zip(ent, oent)) if a != b), min(len(ent), len(oent)))
                what = f"entry {k} " + (f"{ent[k][:2]} vs {oent[k][:2]}" if k < min(len(ent), len(oent)) else "missing")
                bad.append(f"record {i}: values differ ({len(ent)} entries, oracle {len(oent)}; first: {what})")
        elif r.order[:, i].any():
            bad.append(f"record {i}: status {ost} but order column not cleared")
        v = int(r.verdict[i])
        if bool(v & 2) != lc or bool(v & 4) != dc:
            bad.append(f"record {i}: crc verdict {v:#x}, want length {lc} data {dc}")
    # row splits of every slot in full, and the kind totals
    want = oracle_lengths(ref, n)
    totals = {1: 0, 2: 0, 3: 0}
    seen = set()
    for s in range(len(r.slot_kind)):
        key = (r.slot_key[s].encode("utf-8"), r.slot_kind[s])
        seen.add(key)
        lens = want.get(key)
        rs = np.concatenate([[0], np.cumsum(lens)]) if lens is not None else np.zeros(n + 1, np.int64)
        totals[key[1]] += int(rs[-1])
        got_rs = r.row_splits[s].astype(np.int64)
        if not np.array_equal(got_rs, rs):
            k = int(np.flatnonzero(got_rs != rs)[0])
            bad.append(f"slot {s} {key}: row_splits[{k}] = {int(got_rs[k])}, want {int(rs[k])}")
    for key in want:
        if key not in seen:
            bad.append(f"no slot for {key}")
    for kd in (1, 2, 3):
        if int(r.info.kind_totals[kd]) != totals[kd]:
            bad.append(f"kind_totals[{kd}] = {int(r.info.kind_totals[kd])}, oracle {totals[kd]}")
    return bad[:20]


def slot_columns(r) -> dict:
    """(key, kind) -> (row splits, the slot's values as one array; bytes as offset and length arrays):
    the form in which two results that number their slots differently compare."""
    out = {}
    for s in range(len(r.slot_kind)):
        rs = r.row_splits[s].astype(np.int64)
        lo, hi = int(r.slot_base[s]) + int(rs[0]), int(r.slot_base[s]) + int(rs[-1])
        kd = r.slot_kind[s]
        if kd == 3:
            vals = (r.i64[lo:hi],)
        elif kd == 2:
            vals = (r.f32[lo:hi],)
        else:
            vals = (r.bytes_off[lo:hi], r.bytes_len[lo:hi])
        out[r.slot_key[s], kd] = (rs, r.order[s], vals)
    return out


def columns_differ(a, b) -> list[str]:
    """Differences of two results of one batch, per (key, kind): a slot only one of them knows must
    be empty in the other."""
    bad = []
    for name in ("status", "verdict"):
        if not np.array_equal(getattr(a, name), getattr(b, name)):
            bad.append(name)
    failed = a.status != 0  # (aux is the detail of an error: not stored for a record that decoded)
    if not bad and not np.array_equal(a.aux[failed], b.aux[failed]):
        bad.append("aux")
    ca, cb = slot_columns(a), slot_columns(b)
    for key in sorted(set(ca) | set(cb)):
        x, y = ca.get(key), cb.get(key)
        if x is None or y is None:
            rs, order, _ = x or y
            if rs[-1] != rs[0] or order.any():
                bad.append(f"{key}: values in one result only")
            continue
        if not np.array_equal(x[0] - x[0][0], y[0] - y[0][0]):
            bad.append(f"{key}: row_splits")
        elif not np.array_equal(x[1], y[1]):
            bad.append(f"{key}: order")
        elif not all(np.array_equal(p, q) for p, q in zip(x[2], y[2])):
            bad.append(f"{key}: values")
    return bad


def wave_spans(st, en) -> np.ndarray:
    """Bytes each aligned group of 64 records spans, from the 16-byte boundary below its first
    record (the lane kernel stages a wave's span when this is at most kStageBytes)."""
    st, en = np.asarray(st, np.int64), np.asarray(en, np.int64)
    return np.array([int(en[min(a + 64, len(st)) - 1]) - (int(st[a]) & ~15) for a in range(0, len(st), 64)], np.int64)
