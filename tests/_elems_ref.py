"""Reference of the two-level ragged outputs (``RaggedElements``: tfrg_result_ragged_elems,
``ragged.elementify``), for tests/test_ragged_elems_host.py and tests/test_ragged_elems_gpu.py. Test
infrastructure: no GPU.

The expected arrays are built from the generator's own items -- ``items[i]`` maps a key to the list of
``bytes`` objects record i carries under it, as tests/_bytes_ref.py hands them out -- never from a
decode's columns."""

from __future__ import annotations

import numpy as np


class Want:
    """``values`` (uint8), ``elem_offsets`` and ``row_offsets`` (int64), the four counters, (E, B)."""

    def __init__(self, elems: list[bytes], row_offsets: list[int], stats: list[int]) -> None:
        self.elems = elems
        self.values = np.frombuffer(b"".join(elems), np.uint8)
        lens = np.fromiter((len(e) for e in elems), np.int64, len(elems))
        self.elem_offsets = np.concatenate([np.zeros(1, np.int64), np.cumsum(lens, dtype=np.int64)])
        self.row_offsets = np.asarray(row_offsets, np.int64)
        self.stats = stats
        self.totals = (len(elems), int(self.values.size))


def expect(items: list[dict], sp, rows=None, row0: int = 0) -> Want:
    """What spec ``sp`` (key, max_elems, max_len) must give for the row list ``rows`` (None: every
    record; entries are Python ints or an array) over the records of ``items``: row k is record
    ``rows[k] - row0``, a skipped (empty) row where that is outside [0, n)."""
    n = len(items)
    rows = list(range(row0, row0 + n)) if rows is None else [int(v) for v in np.asarray(rows, object).reshape(-1)]
    elems: list[bytes] = []
    ro = [0]
    st = [0, 0, 0, 0]
    for v in rows:
        g = v - row0
        if not 0 <= g < n:
            st[3] += 1
            ro.append(ro[-1])
            continue
        its = items[g].get(sp.key, [])
        st[2] += len(its) == 0
        if sp.max_elems is not None and len(its) > sp.max_elems:
            st[0] += 1
            its = its[: sp.max_elems]
        for e in its:
            if sp.max_len is not None and len(e) > sp.max_len:
                st[1] += 1
                e = e[: sp.max_len]
            elems.append(e)
        ro.append(ro[-1] + len(its))
    return Want(elems, ro, st)
