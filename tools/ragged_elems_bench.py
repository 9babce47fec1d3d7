#!/usr/bin/env python3
"""Paired timing of two-level ragged outputs (tfrg_result_ragged_elems) against the same three arrays
built from the columns of the device view with torch ops, the only route before it.

usage (GPU box): ragged_elems_bench.py [--runs 5] [--steps 20] [--out profiles/ragged_elems/paired_timings.txt] [--small]

Workloads, each resident in HBM, decoded once and confirmed:
  detection: 131,072 records of 1..20 class strings of 3..12 bytes, m in 256, 4096, 65536;
  frames: 2,048 records of 1..8 encoded frames of about 40 KB each, m in 256, 4096;
  long list: one record of 5,000 elements of 0..9 bytes and one of a single 300,000-byte element among
    38 records of 0..3 short elements, every record in order plus the two long ones again.
Rows are drawn at random with repeats (one list per m, on the device). A step is:

  (a) ragged_elements(rows=, out=) into preallocated outputs: four launches, no host synchronisation;
  (b) device_columns() (which materializes the columns an optimistic decode left implicit), then
      row_splits / bytes_off / bytes_len gathered with torch: two cumsums, two repeat_interleaves whose
      sizes are read back (two host synchronisations), and an index of the input bytes.

The outputs of (a) and (b) are compared first. A run is `--steps` steps of one variant between two
device events on the stream (fewer where one step moves hundreds of MB), with the host clock around the
same steps; the variants alternate run by run in one process, after a warm-up of both. Reported per
variant and m: the runs' per-step times, their median, minimum and maximum. Nothing is judged.
--small: fewer records and smaller m, for a quick check of the tool itself.
"""
import argparse
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
for p in (str(REPO / "tfrecords-reader_amd"), str(REPO), str(REPO / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402
from dense_bench import Resident, column  # noqa: E402
from ragged_bench import line, timed_runs  # noqa: E402
from tfr_reader import dense as D  # noqa: E402
from tfr_reader import ragged as R  # noqa: E402
from tfr_reader import synth, writer  # noqa: E402

KEY = "b"


def lists_workload(name: str, desc: str, counts, length_of, seed: int) -> bench.Workload:
    """Records of one bytes_list `b`: record r holds counts[r] elements of length_of(rng) bytes each."""
    rng = np.random.default_rng(seed)
    recs = []
    for c in counts:
        lens = [int(length_of(rng)) for _ in range(int(c))]
        blob = rng.integers(0, 256, sum(lens) + 1, dtype=np.uint8).tobytes()
        at, elems = 0, []
        for ln in lens:
            elems.append(blob[at : at + ln])
            at += ln
        recs.append(writer.encode_example([(KEY, "bytes_list", elems), ("n", "int64_list", [len(recs)])]))
    buf, st, en = synth.framed(recs)
    return bench.Workload(name, desc, buf, st, en, [(0, len(recs))])


class Torch:
    """Variant (b): the three arrays from the device view's columns."""

    def __init__(self, a: Resident, slot: int, dev) -> None:
        self.a, self.slot, self.dev = a, slot, dev

    def __call__(self, rows) -> tuple:
        a, dev, n = self.a, self.dev, self.a.n
        cols = a.dec.device_columns()  # fills the implicit columns on the decode's stream
        total = int(a.dec.info().kind_totals[1])
        rs_ptr = C.cast(cols.row_splits, C.c_void_p).value + 4 * self.slot * (n + 1)
        rs = column(C.c_void_p(rs_ptr), n + 1, "<i4", dev)
        base = column(cols.slot_base, self.slot + 1, "<i8", dev)[self.slot]
        b_off = column(cols.bytes_off, total, "<i4", dev)
        b_len = column(cols.bytes_len, total, "<i4", dev)
        m = int(rows.numel())
        lo = rs[rows].to(torch.int64)
        cnt = rs[rows + 1].to(torch.int64) - lo
        ro = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        torch.cumsum(cnt, 0, out=ro[1:])
        n_el = int(ro[-1])  # (a host synchronisation)
        row_of = torch.repeat_interleave(torch.arange(m, device=dev), cnt, output_size=n_el)
        es = base + lo[row_of] + (torch.arange(n_el, device=dev) - ro[row_of])
        ln = b_len[es].to(torch.int64)
        eo = torch.zeros(n_el + 1, dtype=torch.int64, device=dev)
        torch.cumsum(ln, 0, out=eo[1:])
        n_by = int(eo[-1])  # (a host synchronisation)
        el_of = torch.repeat_interleave(torch.arange(n_el, device=dev), ln, output_size=n_by)
        src = b_off[es].to(torch.int64)[el_of] + (torch.arange(n_by, device=dev) - eo[el_of])
        return a.d_bytes[src], eo, ro


def measure(say, title: str, a: Resident, rows_by_name: dict, dev, stream, runs: int, steps: int) -> None:
    spec = [R.RaggedElements(KEY)]
    slot = D.resolve_slot(a.dec, spec[0])
    assert slot is not None
    say(f"{title}: {a.n} records")
    via_torch = Torch(a, slot, dev)
    for name, rows in rows_by_name.items():
        m = int(rows.numel())
        first = a.dec.ragged_elements(spec, rows=rows)  # exact sizes, once, outside the steps
        n_el, n_by = first.totals[KEY]
        out_a = {KEY: (torch.empty(n_by, dtype=torch.uint8, device=dev), torch.empty(n_el + 1, dtype=torch.int64, device=dev),
                       torch.empty(m + 1, dtype=torch.int64, device=dev))}
        a.dec.ragged_elements(spec, rows=rows, out=out_a)
        got_b = via_torch(rows)
        torch.cuda.synchronize(dev)
        equal = all(torch.equal(x, y) for x, y in zip(out_a[KEY], got_b))
        del got_b
        keep: dict = {}

        def step_a() -> None:
            a.dec.ragged_elements(spec, rows=rows, out=out_a)

        def step_b() -> None:
            keep["b"] = via_torch(rows)

        n_steps = max(2, min(steps, int(4e9 // max(n_by, 1))))
        ev, wall = timed_runs(stream, {"a": step_a, "b": step_b}, runs, n_steps)
        torch.cuda.synchronize(dev)
        written = n_by + 8 * (n_el + 1) + 8 * (m + 1)
        say(f"{name}: m = {m}, E = {n_el} elements, B = {n_by} bytes, {written} bytes written per step, "
            f"{n_steps} steps per run; (b) equal to (a): {equal}")
        say(line("  (a) ragged_elements(rows=, out=)", ev["a"], wall["a"]))
        say(line("  (b) device_columns() + torch ops", ev["b"], wall["b"]))
        keep.clear()
        del out_a


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
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

    stream = torch.cuda.Stream(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    say(f"device {torch.cuda.get_device_name(dev)}; {args.runs} alternated runs per variant")
    with torch.cuda.stream(stream):
        def draws(n: int, sizes) -> dict:
            return {f"random rows, m = {m}": torch.randint(0, n, (m,), generator=gen, device=dev, dtype=torch.int64)
                    for m in sizes}

        rng = np.random.default_rng(1)
        nd = 4096 if args.small else 131072
        wd = lists_workload("detection", "class strings", rng.integers(1, 21, nd), lambda r: r.integers(3, 13), 2)
        a = Resident(wd, dev, stream)
        a.decode()
        measure(say, "workload detection (1..20 strings of 3..12 bytes)", a, draws(nd, (256, 1024) if args.small else (256, 4096, 65536)),
                dev, stream, args.runs, args.steps)
        a.sd.close()
        del wd, a
        nf = 128 if args.small else 2048
        wf = lists_workload("frames", "encoded frames", rng.integers(1, 9, nf),
                            lambda r: np.clip(r.normal(40960, 8192), 4096, 131072), 3)
        a = Resident(wf, dev, stream)
        a.decode()
        measure(say, "workload frames (1..8 elements of about 40 KB)", a, draws(nf, (64, 256) if args.small else (256, 4096)), dev,
                stream, args.runs, args.steps)
        a.sd.close()
        del wf, a
        counts = rng.integers(0, 4, 40)
        counts[11], counts[29] = 5000, 1
        recs = []  # (record 11: the long list; record 29: one element of 300,000 bytes)
        r2 = np.random.default_rng(5)
        for i, c in enumerate(counts.tolist()):
            lens = [300_000] if i == 29 else r2.integers(0, 10, c).tolist()
            recs.append(writer.encode_example([(KEY, "bytes_list", [r2.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in lens]),
                                               ("n", "int64_list", [i])]))
        buf, st, en = synth.framed(recs)
        wl = bench.Workload("long", "one list of 5,000 elements, one element of 300,000 bytes", buf, st, en, [(0, len(recs))])
        a = Resident(wl, dev, stream)
        a.decode()
        rows = torch.tensor([*range(40), 11, 29], dtype=torch.int64, device=dev)
        measure(say, "workload long list and long element", a, {"every record, the two long ones twice": rows}, dev, stream,
                args.runs, args.steps)
        a.sd.close()


if __name__ == "__main__":
    main()
