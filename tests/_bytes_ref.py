"""Host reference of the materialized bytes column (TFRG_FLAG_MATERIALIZE_BYTES), for
tests/test_materialize_gpu.py. Test infrastructure: no GPU.

The expected column is built from the generator's own items -- the ``bytes`` objects handed to
``byt(...)`` -- never from the device's ``bytes_off`` / ``bytes_len``. The decode only decides the
order: bytes slots by ``slot_base``, inside a slot the records and their ``row_splits``; what every
element holds is the generator's. ``want_data`` is the items concatenated in that order and
``want_offsets`` the exclusive scan of their lengths.

A batch here is ``(payloads, items)``: ``items[i]`` maps a key to the list of bytes items record i
carries under it (bytes_list features only)."""

from __future__ import annotations

import re
from pathlib import Path

import numpy as np

from tests.golden.gen_golden import byt, entry, example, i64

BYTES_HIP = Path(__file__).resolve().parents[1] / "tfrecords-reader_amd" / "csrc" / "tfrg_bytes.hip"


def kernel_constants() -> dict[str, int]:
    """kBsTile (= kBsBlock * kBsItems) and kBigElem as csrc/tfrg_bytes.hip builds with them."""
    text = BYTES_HIP.read_text()

    def const(name: str) -> int:
        return int(re.search(rf"\b{name} = (\d+)", text).group(1))

    assert re.search(r"\bkBsTile = kBsBlock \* kBsItems;", text), "kBsTile is no longer kBsBlock * kBsItems"
    return {"tile": const("kBsBlock") * const("kBsItems"), "big": const("kBigElem")}


def record(items: dict[bytes, list[bytes]], *extra: bytes) -> tuple[bytes, dict[str, list[bytes]]]:
    """One Example payload with a bytes_list per key of ``items`` (after the ``extra`` entries), and
    its items under the keys as the decoder names them."""
    payload = example(*extra, *[entry(k, byt(*v)) for k, v in items.items()])
    return payload, {k.decode(): list(v) for k, v in items.items()}


def pack(elems: list[bytes], per_record: list[int], key: bytes = b"b") -> tuple[list[bytes], list[dict]]:
    """``elems`` dealt to records of ``per_record[k % len]`` elements each (the last one ragged),
    every record with an int64 entry so that none is empty."""
    payloads, items, at, k = [], [], 0, 0
    while at < len(elems) or not payloads:
        m = per_record[k % len(per_record)]
        p, it = record({key: elems[at : at + m]}, entry(b"n", i64(k)))
        payloads.append(p)
        items.append(it)
        at += m
        k += 1
    return payloads, items


def random_elems(lengths, seed: int) -> list[bytes]:
    """Elements of the given lengths cut from one random blob (fixed seed): a shifted or misplaced
    byte cannot compare equal by accident."""
    lengths = [int(x) for x in lengths]
    blob = np.random.default_rng(seed).integers(0, 256, sum(lengths) + 1, dtype=np.uint8).tobytes()
    out, at = [], 0
    for ln in lengths:
        out.append(blob[at : at + ln])
        at += ln
    return out


class Expected:
    """The column a batch must materialize to: ``elems`` in column order, ``lengths``, ``offsets``
    (uint64, one more than elements) and ``data`` (uint8)."""

    def __init__(self, elems: list[bytes]) -> None:
        self.elems = elems
        self.lengths = np.fromiter((len(e) for e in elems), np.uint64, len(elems))
        self.offsets = np.concatenate([np.zeros(1, np.uint64), np.cumsum(self.lengths, dtype=np.uint64)])
        self.data = np.frombuffer(b"".join(elems), np.uint8)


def expected(items: list[dict], slot_key, slot_kind, slot_base, row_splits) -> Expected:
    """The reference column of a batch whose decode laid its slots out as given (``BatchResult``'s
    ``slot_key``, ``slot_kind``, ``slot_base``, ``row_splits``). The element counts the decode
    reports must be the generator's: a record's row-split span is the number of items it carries."""
    n = len(items)
    row_splits = np.asarray(row_splits)
    slots = [s for s in range(len(slot_kind)) if slot_kind[s] == 1]
    slots.sort(key=lambda s: (int(slot_base[s]), int(row_splits[s][-1]) != int(row_splits[s][0])))
    elems: list[bytes] = []
    for s in slots:
        rs = row_splits[s].astype(np.int64)
        assert rs.shape[0] == n + 1
        key = slot_key[s]
        base = int(slot_base[s])
        for i in range(n):
            its = items[i].get(key, ())
            assert int(rs[i + 1] - rs[i]) == len(its), (key, i, int(rs[i + 1] - rs[i]), len(its))
            if its:
                assert base + int(rs[i]) == len(elems), (key, i, base, int(rs[i]), len(elems))
                elems.extend(its)
    return Expected(elems)


def first_difference(got_offsets, got_data, want: Expected, src=None) -> str | None:
    """None when the column equals the reference, else the first differing element: its index,
    length, ``dst & 15`` and ``src & 3`` (``src``: the elements' input offsets, when known), which
    name the copy path that produced it."""

    def where(e: int) -> str:
        e = min(e, want.lengths.size - 1)
        if e < 0:
            return "no elements"
        sa = "?" if src is None or e >= len(src) else str(int(src[e]) & 3)
        return (f"element {e}: length {int(want.lengths[e])}, dst & 15 = {int(want.offsets[e]) & 15}, "
                f"src & 3 = {sa}")

    go = np.asarray(got_offsets).astype(np.uint64).reshape(-1)
    if go.shape != want.offsets.shape:
        return f"{go.shape[0]} offsets, want {want.offsets.shape[0]}"
    bad = np.flatnonzero(go != want.offsets)
    if bad.size:
        i = int(bad[0])
        return f"offsets[{i}] = {int(go[i])}, want {int(want.offsets[i])} ({bad.size} differ); {where(i - 1)}"
    gd = np.asarray(got_data).astype(np.uint8).reshape(-1)
    if gd.shape != want.data.shape:
        return f"{gd.shape[0]} data bytes, want {want.data.shape[0]}"
    bad = np.flatnonzero(gd != want.data)
    if bad.size:
        p = int(bad[0])
        e = int(np.searchsorted(want.offsets, p, side="right")) - 1
        return (f"data[{p}] = {int(gd[p])}, want {int(want.data[p])} ({bad.size} bytes differ), byte "
                f"{p - int(want.offsets[e])} of {where(e)}")
    return None
