#!/usr/bin/env python3
"""Timing of bytes predicates on the device (tfrg_result_select_match) beside the integer select.

usage (GPU box): select_bytes_timing.py [--runs 5] [--steps 50] [--n1 1048576] [--n2 4096] [--out FILE] [--small]

Every workload is resident in HBM, decoded once and confirmed; a step is one ``select(where, out=)``
over every record, nothing synchronising with the host. A run is `--steps` steps of one variant between
two device events on the stream (the host clock around the same steps beside it); the variants
alternate run by run in one process, after a warm-up of every variant (tools/ragged_bench.py
``timed_runs``). Nothing is judged here; the figures are reported as they come.

1. C1-shaped records (`--n1` of them: int64 label + 12-byte id, decoded optimistically): the integer
   select ``100 <= label < 350`` of tools/select_bench.py, ``id == <one id>``, ``id`` starts with a
   prefix, ``id`` in a list of 8, and ``id`` contains 2 bytes (12-byte elements: the lane's path).
2. C2-shaped records (`--n2` of them: images of 4 KiB .. 512 KiB of random bytes): ``image`` contains a
   16-byte pattern that occurs nowhere, so every image is scanned to its end, with the default knob.
   Reported beside a ``bytes_len`` select over the same records (the step's fixed part: three launches
   and a memset that read no image): bytes scanned over the step's time and over the difference of the
   two, and their share of the 8 TB/s HBM peak.
3. The knob (tfrg_ctx_set_select_scan): records of one 64-, 256-, 1024- or 4096-byte element, ``contains`` of
   an absent 8-byte pattern, with the knob at 16, 64, 256, 1024, 4096 and 65536: which elements should go to
   their lane and which to their wave.
--small: a quick check of the tool itself on a fraction of the records.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
for p in (str(REPO / "tfrecords-reader_amd"), str(REPO), str(REPO / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402
from dense_bench import Resident  # noqa: E402
from ragged_bench import line, timed_runs  # noqa: E402
from select_bench import WHERE as INT_WHERE  # noqa: E402
from select_bench import c1_workload  # noqa: E402
from tfr_reader import dense as D  # noqa: E402
from tfr_reader import synth, writer  # noqa: E402
from tfr_reader.select import BytesTerm, Term, bytes_in  # noqa: E402

HBM_PEAK = 8e12  # bytes per second
KNOBS = [16, 64, 256, 1024, 4096, 65536]


def selects(a: Resident, wheres: dict, dev) -> tuple[dict, dict, dict]:
    """name -> step function, output tensor, last Selection."""
    outs = {k: torch.empty(a.n, dtype=torch.int64, device=dev) for k in wheres}
    keep: dict = {}

    def step(k):
        def f() -> None:
            keep[k] = a.dec.select(wheres[k], capacity=a.n, out=outs[k])
        return f

    return {k: step(k) for k in wheres}, outs, keep


def c1_part(say, n: int, dev, stream, runs: int, steps: int) -> None:
    a = Resident(c1_workload(n), dev, stream)
    info = a.decode()
    say(f"1. C1, {n} records (implicit_cols {int(info.implicit_cols)}, implicit_off_slots {int(info.implicit_off_slots):#x})")
    ids = [b"img-%08d" % ((n // 2 + 7919 * k) % n) for k in range(8)]
    wheres = {"int  100 <= label < 350": INT_WHERE,
              "id == one id": [BytesTerm("id", "==", ids[0])],
              "id startswith 9 bytes": [BytesTerm("id", "startswith", ids[0][:9])],
              "id in 8 ids": [bytes_in("id", ids)],
              "id contains 2 bytes": [BytesTerm("id", "contains", b"77")]}
    variants, outs, keep = selects(a, wheres, dev)
    ev, wall = timed_runs(stream, variants, runs, steps)
    torch.cuda.synchronize(dev)
    for k in wheres:
        say(line(f"  {k} ({keep[k].count} pass)", ev[k], wall[k]))
    # the bytes lists against torch, once
    idt = a.dec.dense([D.Dense("id", "uint8", 12)], stream=stream.cuda_stream)["id"]
    eq = (idt == torch.tensor(list(ids[0]), dtype=torch.uint8, device=dev)).all(1).nonzero()[:, 0]
    got = outs["id == one id"][: keep["id == one id"].count]
    say(f"  id == one id equals the torch compare of a dense id tensor: {torch.equal(got, eq)}")
    a.sd.close()


def c2_part(say, n: int, dev, stream, runs: int, steps: int) -> None:
    buf, st, en = synth.framed(synth.c2_payloads(n))
    a = Resident(bench.Workload(f"c2x{n}", f"{n} C2-shaped records", buf, st, en, [(0, n)]), dev, stream)
    a.decode()
    sizes = synth.c2_truth(n)[0]
    scanned = int(sizes.sum())
    say(f"2. C2, {n} records, images of {int(sizes.min())} .. {int(sizes.max())} bytes, {scanned} bytes in all; default knob")
    pattern = bytes(range(0xF0, 0x100))  # 16 bytes; the images are random: it does not occur
    wheres = {"image contains 16 bytes": [BytesTerm("image", "contains", pattern)],
              "image bytes_len > 0 (fixed part)": [Term("image", "uint8", ">", 0, "bytes_len")],
              "image == 16 bytes": [BytesTerm("image", "==", pattern)]}
    variants, _, keep = selects(a, wheres, dev)
    ev, wall = timed_runs(stream, variants, runs, steps)
    torch.cuda.synchronize(dev)
    for k in wheres:
        say(line(f"  {k} ({keep[k].count} pass)", ev[k], wall[k]))
    whole = statistics.median(ev["image contains 16 bytes"]) * 1e-3
    fixed = statistics.median(ev["image bytes_len > 0 (fixed part)"]) * 1e-3
    say(f"  contains: {scanned / whole / 1e12:.3f} TB/s over the whole step ({100 * scanned / whole / HBM_PEAK:.1f} % of the "
        f"8 TB/s peak); {scanned / max(whole - fixed, 1e-9) / 1e12:.3f} TB/s over the step minus the fixed part "
        f"({100 * scanned / max(whole - fixed, 1e-9) / HBM_PEAK:.1f} %)")
    a.sd.close()


def knob_part(say, n: int, dev, stream, runs: int, steps: int) -> None:
    say(f"3. the knob: {n} records of one element each, contains of an absent 8-byte pattern; ms per step by knob")
    rng = np.random.default_rng(21)
    pattern = bytes(range(0xF8, 0x100))
    for ln in (64, 256, 1024, 4096):
        recs = [writer.encode_example([("blob", "bytes_list", [rng.integers(0, 0x80, ln, dtype=np.uint8).tobytes()])])
                for _ in range(n)]
        buf, st, en = synth.framed(recs)
        a = Resident(bench.Workload(f"b{ln}", f"{n} records of {ln} bytes", buf, st, en, [(0, n)]), dev, stream)
        a.decode()
        where = [BytesTerm("blob", "contains", pattern)]
        out = torch.empty(n, dtype=torch.int64, device=dev)

        def step(knob):
            def f() -> None:
                a.dec.set_select_scan(knob)
                a.dec.select(where, capacity=n, out=out)
            return f

        ev, wall = timed_runs(stream, {k: step(k) for k in KNOBS}, runs, steps)
        torch.cuda.synchronize(dev)
        say(f"  elements of {ln} bytes ({n * ln} bytes scanned per step)")
        for k in KNOBS:
            path = "wave" if ln > k else "lane"
            say(line(f"    knob {k:>5} ({path})", ev[k], wall[k]))
        a.dec.set_select_scan(0)
        a.sd.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--n1", type=int, default=1 << 20)
    ap.add_argument("--n2", type=int, default=4096)
    ap.add_argument("--n3", type=int, default=16384)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    if args.small:
        args.n1, args.n2, args.n3 = 1 << 16, 256, 2048
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    lines: list[str] = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)
        if args.out:  # (kept up to date: a later part that fails loses nothing recorded so far)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")

    stream = torch.cuda.Stream(dev)
    say(f"device {torch.cuda.get_device_name(dev)}; {args.runs} alternated runs of {args.steps} steps per variant, "
        f"after a warm-up of 2 runs each")
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):
        c1_part(say, args.n1, dev, stream, args.runs, args.steps)
        c2_part(say, args.n2, dev, stream, args.runs, args.steps)
        knob_part(say, args.n3, dev, stream, args.runs, args.steps)
    say(f"total {time.perf_counter() - t0:.1f} s")


if __name__ == "__main__":
    main()
