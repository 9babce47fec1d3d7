"""Reference of the element ids (``ElementIds``: tfrg_result_elem_ids, ``ids.idsify``), for
tests/test_elem_ids_host.py and tests/test_elem_ids_gpu.py. Test infrastructure: no GPU.

The expected ids are built from the generator's own items -- ``items[i]`` maps a key to the list of
``bytes`` objects record i carries under it, as tests/_bytes_ref.py hands them out --, a Python dict and
the Python restatement of tfrg_hash64 below. Nothing comes from a decode's columns, from the C lookup
or from tfr_reader/ids.py."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

M64 = (1 << 64) - 1
EMPTY = 0xFFFFFFFF

# include/tfrg.h's known answers
KNOWN = [(b"", 0xEFD01F60BA992926), (b"a", 0x25AD9D1B70DE62D1), (b"a\0", 0x9A836725E1EC859F), (b"cat", 0xC88023524FE4125C),
         (b"12345678", 0x2AE6663AF2DE905B), (b"123456789", 0x2F09F696751E111E), (bytes(range(256)), 0x4DE6A3BA6810D417)]


def hash64(s: bytes) -> int:
    """tfrg_hash64 as include/tfrg.h states it."""
    h = 0xCBF29CE484222325
    for at in range(0, len(s), 8):
        w = int.from_bytes(s[at : at + 8].ljust(8, b"\0"), "little")
        h = ((h ^ w) * 0x100000001B3) % (1 << 64)
    h ^= len(s)
    h ^= h >> 33
    h = h * 0xFF51AFD7ED558CCD % (1 << 64)
    h ^= h >> 33
    h = h * 0xC4CEB9FE1A85EC53 % (1 << 64)
    h ^= h >> 33
    return h


class TableModel:
    """The vocabulary's open-addressing table as include/tfrg.h documents it: ``capacity``, ``slots``
    (word index or EMPTY), ``disp[i]`` (word i's displacement from its home slot), ``max_probe``."""

    def __init__(self, words: list[bytes]) -> None:
        cap = 16
        while cap < 2 * len(words):
            cap *= 2
        self.capacity = cap
        self.slots = [EMPTY] * cap
        self.disp = []
        for i, w in enumerate(words):
            s, d = hash64(w) & (cap - 1), 0
            while self.slots[s] != EMPTY:
                s, d = (s + 1) & (cap - 1), d + 1
            self.slots[s] = i
            self.disp.append(d)
        self.max_probe = max(self.disp, default=0)


def wrap64(v: int) -> int:
    return (v + (1 << 63)) % (1 << 64) - (1 << 63)


@dataclass
class Rule:
    """One spec: ``table`` maps a word to its id (None: no vocabulary)."""

    key: str
    table: dict | None = None
    buckets: int = 0
    base: int = 0
    default: int = -1
    max_elems: int | None = None

    def id_of(self, s: bytes) -> tuple[int, bool]:
        if self.table is not None and s in self.table:
            return self.table[s], True
        if self.buckets:
            return wrap64(self.base + hash64(s) % self.buckets), False
        return self.default, False


class Want:
    """``ids`` and ``row_offsets`` (int64), the four counters, E, and how many elements matched a word."""

    def __init__(self, ids: list[int], row_offsets: list[int], stats: list[int], elems: list[bytes]) -> None:
        self.ids = np.asarray(ids, np.int64).reshape(-1)
        self.row_offsets = np.asarray(row_offsets, np.int64)
        self.stats = stats
        self.total = len(ids)
        self.matched = len(ids) - stats[1]
        self.elems = elems


def expect(items: list[dict], rule: Rule, rows=None, row0: int = 0) -> Want:
    """What ``rule`` must give for the row list ``rows`` (None: every record; entries are Python ints
    or an array) over the records of ``items``: row k is record ``rows[k] - row0``, a skipped (empty)
    row where that is outside [0, n)."""
    n = len(items)
    rows = list(range(row0, row0 + n)) if rows is None else [int(v) for v in np.asarray(rows, object).reshape(-1)]
    ids: list[int] = []
    elems: list[bytes] = []
    ro = [0]
    st = [0, 0, 0, 0]
    for v in rows:
        g = v - row0
        if not 0 <= g < n:
            st[3] += 1
            ro.append(ro[-1])
            continue
        its = items[g].get(rule.key, [])
        st[2] += len(its) == 0
        if rule.max_elems is not None and len(its) > rule.max_elems:
            st[0] += 1
            its = its[: rule.max_elems]
        for e in its:
            i, hit = rule.id_of(e)
            st[1] += not hit
            ids.append(i)
            elems.append(e)
        ro.append(ro[-1] + len(its))
    return Want(ids, ro, st, elems)
