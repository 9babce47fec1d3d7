#!/usr/bin/env python3
"""Paired timing of row-selected dense tensors (tfrg_result_dense_rows) against the two ways of
drawing a minibatch from a decoded shard that existed before it.

usage (GPU box): dense_rows_bench.py [--runs 5] [--steps 50] [--out profiles/dense_rows/paired_timings.txt]
                                     [--small] [--no-c3]

Workloads: the decode of tools/dense_bench.py -- rank 0's share of 8 of the 256-file C1 directory
(~16.8 M records), `label` int64 W = 1 and `id` uint8 W = 12 -- and C3 (131,072 records), all 64
slots at width 64. The shard is resident in HBM, decoded once and confirmed. For m in 256, 4096,
65536 rows drawn at random with repeats (one list per m, on the device), a step is:

  (a) dense(rows=): one tfrg_result_dense_rows launch over the columns where the decode left them;
  (b) torch.index_select per output from a full dense() made once before the loop (its outputs stay
      resident on top of the columns: the extra bytes are reported);
  (c) the selection decoded again: the rows' (start, end) offsets gathered on the device,
      tfrg_decode_device32 on a second context, then tfrg_result_dense -- CRCs, the walk and the host
      synchronisation that confirms the optimistic decode, every step. The decode is handed the
      rows in ascending order (sorted once, outside the timed steps), the order every other caller
      of the device decode gives it records in; its outputs are compared in that order.

A run is `--steps` steps of one variant between two device events on the stream, with the host
clock around the same steps up to the stream's synchronisation; the variants alternate run by run in
one process, after a warm-up of every variant and shape. Reported per variant and m: the runs'
per-step times (device events, and wall), their median, minimum and maximum. Outputs of the three
variants are compared once per m. Nothing is judged: the medians and ranges go to DESIGN.md.
--small: a 1/16 C1 share, for a quick check of the tool itself.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
for p in (str(REPO / "tfrecords-reader_amd"), str(REPO), str(REPO / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402
from dense_bench import Resident  # noqa: E402
from tfr_reader import dense as D  # noqa: E402

MS = (256, 4096, 65536)
TDT = {"int64": torch.int64, "int32": torch.int32, "float32": torch.float32, "uint8": torch.uint8}


def empty_outputs(specs, m: int, dev) -> dict:
    return {s.out_name: torch.empty((m, s.width), dtype=TDT[s.dtype], device=dev) for s in specs}


def line(name: str, ev: list[float], wall: list[float]) -> str:
    def part(v: list[float]) -> str:
        return (" ".join(f"{x:8.4f}" for x in v) +
                f" | median {statistics.median(v):8.4f} min {min(v):8.4f} max {max(v):8.4f}")

    return f"{name:<34} ms/step, device events: {part(ev)}\n{'':<34} ms/step, wall:          {part(wall)}"


def measure(say, title: str, w, specs, dev, stream, runs: int, steps: int, with_c: bool) -> None:
    n = w.n
    a = Resident(w, dev, stream)
    a.decode()
    full = a.dec.dense(specs, stream=stream.cuda_stream)  # (b)'s resident outputs
    extra = sum(t.numel() * t.element_size() for t in full.values())
    say(f"{title}: {n} records, {len(specs)} outputs; (b) keeps {extra} bytes resident on top of the columns")
    c = None
    if with_c:
        c = Resident(w, dev, stream, share=a)
        assert int(w.buf.size) < 1 << 31  # (the gathered offsets are int32 tensors)
        en_all = a.d_en
        if a.d_st is not None:
            st_all = a.d_st
        else:  # back-to-back records: record i starts where record i - 1 ends
            first = torch.tensor([int(a.firsts[0])], dtype=torch.int32, device=dev)
            st_all = torch.cat([first, en_all[:-1]])
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    for m in MS:
        rows = torch.randint(0, n, (m,), generator=gen, device=dev, dtype=torch.int64)
        out = {k: empty_outputs(specs, m, dev) for k in "abc"}
        rows_up, order = torch.sort(rows)

        def step_a() -> None:
            a.dec.dense(specs, rows=rows, out=out["a"], stream=stream.cuda_stream)

        def step_b() -> None:
            for k, t in full.items():
                torch.index_select(t, 0, rows, out=out["b"][k])

        def step_c() -> None:
            st, en = st_all[rows_up], en_all[rows_up]
            c.dec.decode_device32(c.d_bytes.data_ptr(), int(w.buf.size), st.data_ptr(), en.data_ptr(), 0, m,
                                  stream=stream.cuda_stream)
            c.dec.dense(specs, out=out["c"], stream=stream.cuda_stream)

        variants = {"a": step_a, "b": step_b}
        if c is not None:
            variants["c"] = step_c
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

        for _ in range(2):  # warm-up: allocator, kernels, the second context's templates
            for k in variants:
                run(k)
        for k in variants:
            ev[k].clear()
            wall[k].clear()
        for _ in range(runs):
            for k in variants:
                run(k)
        torch.cuda.synchronize(dev)
        want = {"b": out["a"], "c": {name: t[order] for name, t in out["a"].items()}}
        equal = {k: all(torch.equal(want[k][name].view(torch.uint8), out[k][name].view(torch.uint8)) for name in out["a"])
                 for k in variants if k != "a"}
        written = sum(t.numel() * t.element_size() for t in out["a"].values())
        say(f"m = {m}: {written} bytes written per step, {steps} steps per run; outputs equal to (a): {equal}")
        say(line("  (a) dense(rows=)", ev["a"], wall["a"]))
        say(line("  (b) index_select per output", ev["b"], wall["b"]))
        if c is not None:
            say(line("  (c) gather offsets + decode + dense", ev["c"], wall["c"]))
        del out
    a.sd.close()
    if c is not None:
        c.sd.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-c3", action="store_true")
    ap.add_argument("--no-redecode", action="store_true", help="leave variant (c) out")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    lines: list[str] = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    stream = torch.cuda.Stream(dev)
    say(f"device {torch.cuda.get_device_name(dev)}; {args.runs} alternated runs of {args.steps} steps per variant")
    with torch.cuda.stream(stream):
        w = bench.c4_workload("c1", 0, 8 * (16 if args.small else 1), 256, name="c4_c1_rank0of8")
        specs = [D.Dense("label", "int64", 1), D.Dense("id", "uint8", 12)]
        measure(say, f"workload {w.name}", w, specs, dev, stream, args.runs, args.steps, not args.no_redecode)
        del w
        if not args.no_c3:
            w3 = bench.single_workload("c3")
            probe = Resident(w3, dev, stream)
            kt = probe.dec.keys
            keys = [(kt.key_str[k], "int64" if kd == 3 else "float32") for k, kd in zip(kt.slot_key, kt.slot_kind)
                    if kd in (2, 3)]
            probe.sd.close()
            specs3 = [D.Dense(k, dt, 64, fill=-1) for k, dt in keys[:64]]
            measure(say, "workload c3 (all slots at width 64)", w3, specs3, dev, stream, args.runs, args.steps,
                    not args.no_redecode)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
