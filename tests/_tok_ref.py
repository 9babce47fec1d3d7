"""Reference of the token ids (``TokenIds``: tfrg_result_token_ids, ``tokens.tokenize``), for
tests/test_token_ids_host.py and tests/test_token_ids_gpu.py. Test infrastructure: no GPU.

The expected ids are built from the generator's own items (``items[i]`` maps a key to the list of
``bytes`` objects record i carries under it), ``bytes.translate`` / ``bytes.split`` / ``bytes.lower`` and
the rule of tests/_ids_ref.py. Nothing comes from a decode's columns or from tfr_reader/tokens.py."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import _ids_ref as IR

WHITESPACE = b" \t\n\r\x0b\x0c"  # what bytes.split() splits on


@dataclass
class Rule(IR.Rule):
    """One spec: tests/_ids_ref.py's rule plus the split. ``delims`` must hold the whitespace bytes."""

    delims: bytes = WHITESPACE
    lower: bool = False
    max_tokens: int | None = None


def expect(items: list[dict], rule: Rule, rows=None, row0: int = 0) -> IR.Want:
    """What ``rule`` must give for the row list ``rows`` (None: every record) over the records of
    ``items``: row k is record ``rows[k] - row0``, a skipped (empty) row where that is outside [0, n).
    ``Want.elems`` are the taken tokens."""
    assert set(WHITESPACE) <= set(rule.delims)  # (split() below splits on these whatever the rule says)
    to_space = bytes.maketrans(rule.delims, b" " * len(rule.delims))
    n = len(items)
    rows = list(range(row0, row0 + n)) if rows is None else [int(v) for v in np.asarray(rows, object).reshape(-1)]
    ids: list[int] = []
    taken: list[bytes] = []
    ro = [0]
    st = [0, 0, 0, 0]
    for v in rows:
        g = v - row0
        if not 0 <= g < n:
            st[3] += 1
            ro.append(ro[-1])
            continue
        its = items[g].get(rule.key, [])
        its = its if rule.max_elems is None else its[: rule.max_elems]
        toks = [t.lower() if rule.lower else t for s in its for t in s.translate(to_space).split()]
        if rule.max_tokens is not None and len(toks) > rule.max_tokens:
            st[0] += 1
            toks = toks[: rule.max_tokens]
        st[2] += not toks
        for t in toks:
            i, hit = rule.id_of(t)
            st[1] += not hit
            ids.append(i)
        taken += toks
        ro.append(ro[-1] + len(toks))
    return IR.Want(ids, ro, st, taken)
