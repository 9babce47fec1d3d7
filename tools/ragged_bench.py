#!/usr/bin/env python3
"""Paired timing of ragged minibatches (tfrg_result_ragged_rows) against the route through the
padded dense tensor that existed before it.

usage (GPU box): ragged_bench.py [--runs 5] [--steps 50] [--out profiles/ragged/paired_timings.txt] [--small]

Workloads, each resident in HBM, decoded once and confirmed:
  C3 (131,072 records, 32 int64_list + 32 float_list of 0..64 values), one slot and all 64;
  tokens: 2,048 records of one int64_list with lengths uniform in 0..4096;
  C2 (8,189 records): the `image` bytes, which the padded route cannot take whole above 4096 bytes,
    so (a) runs alone there;
  short tokens (256 records of 0..64 values) and one record of 1,000,000 values: 4,096 short rows with
    and without that one row among them, for the cost of one very long row in an otherwise short list.
For m in 256, 4096, 65536 rows drawn at random with repeats (one list per m, on the device), a step is:

  (a) ragged(rows=, capacity=): lengths, tile scan and gather over the columns where the decode left
      them; no host synchronisation;
  (b) dense(rows=, width=max, lengths=True), a mask select of the padded tensor and a cumsum of the
      lengths: the same packed values and offsets through torch (the mask select synchronises with
      the host to size its result).

A run is `--steps` steps of one variant between two device events on the stream, with the host clock
around the same steps up to the stream's synchronisation; the variants alternate run by run in one
process, after a warm-up of every variant and shape. Reported per variant and m: the runs' per-step
times (device events, and wall), their median, minimum and maximum. The outputs of (a) and (b) are
compared once per m. Nothing is judged: the medians and ranges go to DESIGN.md.
--small: 1/8 of the C3 records and smaller m, for a quick check of the tool itself.
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
from tfr_reader import dense as D  # noqa: E402
from tfr_reader import ragged as R  # noqa: E402
from tfr_reader import synth, writer  # noqa: E402

TDT = {"int64": torch.int64, "int32": torch.int32, "float32": torch.float32, "uint8": torch.uint8}
LONG = 1_000_000


def line(name: str, ev: list[float], wall: list[float]) -> str:
    def part(v: list[float]) -> str:
        return (" ".join(f"{x:8.4f}" for x in v) +
                f" | median {statistics.median(v):8.4f} min {min(v):8.4f} max {max(v):8.4f}")

    return f"{name:<34} ms/step, device events: {part(ev)}\n{'':<34} ms/step, wall:          {part(wall)}"


def token_workload(n: int, max_len: int, long_row: int = 0) -> bench.Workload:
    """n records of one int64_list `tok` with lengths uniform in 0..max_len (then one of long_row values)."""
    rng = np.random.default_rng(12)
    lens = rng.integers(0, max_len + 1, n).tolist() + ([long_row] if long_row else [])
    recs = [writer.encode_example([("tok", "int64_list", rng.integers(0, 32000, ln).tolist())]) for ln in lens]
    buf, st, en = synth.framed(recs)
    return bench.Workload("tokens", f"{n} records of 0..{max_len} int64 tokens", buf, st, en, [(0, len(lens))])


def timed_runs(stream, variants: dict, runs: int, steps: int) -> tuple[dict, dict]:
    ev = {k: [] for k in variants}
    wall = {k: [] for k in variants}

    def run(k: str) -> None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        for _ in range(steps):
            variants[k]()
        e1.record(stream)
        e1.synchronize()
        wall[k].append((time.perf_counter() - t0) * 1e3 / steps)
        ev[k].append(e0.elapsed_time(e1) / steps)

    for _ in range(2):  # warm-up: allocator, kernels
        for k in variants:
            run(k)
    for k in variants:
        ev[k].clear()
        wall[k].clear()
    for _ in range(runs):
        for k in variants:
            run(k)
    return ev, wall


def measure(say, title: str, a: Resident, specs, rows_by_m: dict, dev, stream, runs: int, steps: int,
            width: int | None) -> None:
    """``width``: the padded route's width (the longest row); None: (a) alone."""
    say(f"{title}: {a.n} records, {len(specs)} outputs")
    for name, rows in rows_by_m.items():
        m = int(rows.numel())
        first = a.dec.ragged(specs, rows=rows)  # exact sizes, once, outside the steps
        caps = dict(first.totals)
        out_a = {k: (torch.empty(caps[k], dtype=v.dtype, device=dev), torch.empty(m + 1, dtype=torch.int64, device=dev))
                 for k, (v, _) in first.items()}
        out_b: dict = {}

        def step_a() -> None:
            a.dec.ragged(specs, rows=rows, out=out_a)

        dspecs = [D.Dense(s.key, s.dtype, width or 1, lengths=True, name=s.out_name) for s in specs]
        col = torch.arange(width or 1, device=dev)[None, :]

        def step_b() -> None:
            got = a.dec.dense(dspecs, rows=rows, stream=stream.cuda_stream)
            for k, t in got.items():
                lens = got.lengths[k]
                offs = torch.zeros(m + 1, dtype=torch.int64, device=dev)
                torch.cumsum(lens, 0, out=offs[1:])
                out_b[k] = (t[col < lens[:, None]], offs)

        variants = {"a": step_a}
        if width is not None:
            variants["b"] = step_b
        ev, wall = timed_runs(stream, variants, runs, steps)
        torch.cuda.synchronize(dev)
        equal = None
        if width is not None:
            equal = all(torch.equal(out_a[k][0].view(torch.uint8), out_b[k][0].view(torch.uint8)) and
                        torch.equal(out_a[k][1], out_b[k][1]) for k in out_a)
        written = sum(v.numel() * v.element_size() + o.numel() * 8 for v, o in out_a.values())
        say(f"{name}: m = {m}, {written} bytes written per step, {steps} steps per run; (b) equal to (a): {equal}")
        say(line("  (a) ragged(rows=, capacity=)", ev["a"], wall["a"]))
        if width is not None:
            padded = sum(m * width * torch.empty(0, dtype=TDT[s.dtype]).element_size() for s in specs)
            say(line("  (b) dense(rows=) + mask + cumsum", ev["b"], wall["b"]))
            say(f"      (b) keeps {padded} bytes of padded tensors per step")
        out_b.clear()
        del out_a


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    lines: list[str] = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)
        if args.out:  # (kept up to date: a later workload that fails loses nothing recorded so far)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")

    ms = (256, 1024) if args.small else (256, 4096, 65536)
    stream = torch.cuda.Stream(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    say(f"device {torch.cuda.get_device_name(dev)}; {args.runs} alternated runs of {args.steps} steps per variant")
    with torch.cuda.stream(stream):
        def draws(n: int, sizes=ms) -> dict:
            return {f"random rows, m = {m}": torch.randint(0, n, (m,), generator=gen, device=dev, dtype=torch.int64)
                    for m in sizes}

        # C3
        if args.small:
            w3 = bench.Workload("c3", "C3, 1/8", *synth.replicate(*synth.framed(synth.c3_payloads(2048, seed=3)), 8), [(0, 16384)])
        else:
            w3 = bench.single_workload("c3")
        a = Resident(w3, dev, stream)
        a.decode()
        kt = a.dec.keys
        keys = [(kt.key_str[k], "int64" if kd == 3 else "float32") for k, kd in zip(kt.slot_key, kt.slot_kind) if kd in (2, 3)]
        rows3 = draws(a.n)
        measure(say, "workload c3, one int64 slot", a, [R.Ragged(*keys[0])], rows3, dev, stream, args.runs, args.steps, 64)
        measure(say, "workload c3, all 64 slots", a, [R.Ragged(k, dt) for k, dt in keys[:64]], rows3, dev, stream, args.runs,
                args.steps, 64)
        a.sd.close()
        del w3, a
        # tokens
        nt = 256 if args.small else 2048
        wt = token_workload(nt, 4096)
        a = Resident(wt, dev, stream)
        a.decode()
        spec = [R.Ragged("tok", "int64")]
        measure(say, "workload tokens (lengths 0..4096)", a, spec, draws(nt), dev, stream, args.runs, args.steps, 4096)
        a.sd.close()
        del wt, a
        # C2 image bytes
        w2 = bench.single_workload("c2")
        a = Resident(w2, dev, stream)
        a.decode()
        measure(say, "workload c2, image bytes (a alone: the rows are wider than dense's 4096)", a, [R.Ragged("image", "uint8")],
                draws(a.n, ms[:2]), dev, stream, args.runs, args.steps, None)
        a.sd.close()
        del w2, a
        # one very long row in an otherwise short list
        wl = token_workload(256, 64, LONG)
        a = Resident(wl, dev, stream)
        a.decode()
        pick = torch.randint(0, 256, (4096,), generator=gen, device=dev, dtype=torch.int64)
        with_long = pick.clone()
        with_long[2048] = 256  # (the record of LONG values)
        measure(say, f"workload short tokens (lengths 0..64) and one record of {LONG} values (a alone)", a, spec,
                {"4096 rows of <= 64 values": pick, f"the same with one row of {LONG} values": with_long}, dev, stream,
                args.runs, args.steps, None)
        a.sd.close()


if __name__ == "__main__":
    main()
