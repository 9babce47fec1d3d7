#!/usr/bin/env python3
"""Paired timing of the device WHERE clause (tfrg_result_select_rows) against the route callers had
before it: a width-1 dense tensor of the predicate column, a torch compare and ``torch.nonzero``.

usage (GPU box): select_bench.py [--runs 5] [--steps 50] [--big 4194304] [--out profiles/select/paired_timings.txt] [--small]

Workloads, each resident in HBM, decoded once (optimistically) and confirmed: C1-shaped records
(int64 label + 12 B id), 65,536 of them (the default single-file workload) and ``--big`` of them.
The predicate is ``100 <= label < 350`` (a quarter of the records pass); the candidates are every
record in order. A step is:

  (a) select(where, capacity=n): verdicts, tile scan and write over the column where the decode left
      it; the row list stays on the device and nothing synchronises with the host;
  (b) dense([label], width 1) -> (t >= 100) & (t < 350) -> torch.nonzero: the same list through torch
      (``nonzero`` synchronises with the host to size its result).

A run is `--steps` steps of one variant between two device events on the stream, with the host clock
around the same steps up to the stream's synchronisation; the variants alternate run by run in one
process, after a warm-up of every variant. Reported per variant and size: the runs' per-step times
(device events, and wall), their median, minimum and maximum, and (a)'s algorithmic bytes.
The outputs of (a) and (b) are compared once per size. Nothing is judged here.
--small: 8,192 and 131,072 records, for a quick check of the tool itself.
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
from tfr_reader import dense as D  # noqa: E402
from tfr_reader import synth  # noqa: E402
from tfr_reader.select import Term  # noqa: E402

LO, HI = 100, 350
WHERE = [Term("label", "int64", ">=", LO), Term("label", "int64", "<", HI)]


def c1_workload(n: int) -> bench.Workload:
    blob, offs = synth.c1_blob(n)
    buf = synth.frame_blob(blob, offs)
    lens = np.diff(offs) + 16
    en = np.cumsum(lens, dtype=np.uint64)
    return bench.Workload(f"c1x{n}", f"{n} C1-shaped records", buf, en - lens, en, [(0, n)])


def measure(say, n: int, dev, stream, runs: int, steps: int) -> None:
    a = Resident(c1_workload(n), dev, stream)
    info = a.decode()
    say(f"workload C1, {n} records (implicit_cols {int(info.implicit_cols)}, placed_slots {int(info.placed_slots):#x})")
    spec = [D.Dense("label", "int64")]
    out_a = torch.empty(n, dtype=torch.int64, device=dev)
    keep: dict = {}

    def step_a() -> None:
        keep["a"] = a.dec.select(WHERE, capacity=n, out=out_a)

    def step_b() -> None:
        t = a.dec.dense(spec, stream=stream.cuda_stream)["label"][:, 0]
        keep["b"] = torch.nonzero((t >= LO) & (t < HI))[:, 0]

    ev, wall = timed_runs(stream, {"a": step_a, "b": step_b}, runs, steps)
    torch.cuda.synchronize(dev)
    count = keep["a"].count
    equal = count == int(keep["b"].numel()) and torch.equal(out_a[:count], keep["b"])
    # (a)'s algorithmic bytes per step: the label column read once, one verdict bit per candidate
    # written and read, the selected entries written (DESIGN.md "Filtered row lists")
    alg = n * 8 + 2 * ((n + 63) // 64) * 8 + count * 8
    say(f"n = {n}: {count} rows pass, {steps} steps per run; (b) equal to (a): {equal}")
    say(line("  (a) select(where, capacity=)", ev["a"], wall["a"]))
    say(line("  (b) dense -> compare -> nonzero", ev["b"], wall["b"]))
    med = statistics.median(ev["a"])
    say(f"      (a) moves {alg} algorithmic bytes per step: {alg / (med * 1e-3) / 1e9:.1f} GB/s at the median")
    a.sd.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--big", type=int, default=1 << 22)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    lines: list[str] = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)
        if args.out:  # (kept up to date: a later size that fails loses nothing recorded so far)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")

    stream = torch.cuda.Stream(dev)
    say(f"device {torch.cuda.get_device_name(dev)}; {args.runs} alternated runs of {args.steps} steps per variant; "
        f"where: {LO} <= label < {HI}")
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):
        for n in ((8192, 131072) if args.small else (65536, args.big)):
            measure(say, n, dev, stream, args.runs, args.steps)
    say(f"total {time.perf_counter() - t0:.1f} s")


if __name__ == "__main__":
    main()
