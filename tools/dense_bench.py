#!/usr/bin/env python3
"""Paired timing of the dense collate (tfrg_result_dense) against what a consumer had to do before it.

usage (GPU box): dense_bench.py [--runs 5] [--out profiles/dense/paired_timings.txt] [--small] [--no-c3]

Workload: rank 0's share of 8 of the 256-file C1 directory (bench.py's c4of8, ~16.8 M records),
resident in HBM and decoded as bench.py does (u32 ends, optimistic). Each run decodes the batch
afresh, confirms it (tfrg_result_info, outside the timed region) and then times, with device events
on the decode's stream around the collate only:

  (a) tfrg_result_dense for `label` int64 W = 1 and `id` uint8 W = 12, lengths off (default stores);
  (a-nt) the same from a context created with TFRG_DENSE_NT=1 (nontemporal output stores);
  (b) tfrg_result_device -- which writes the columns the optimistic decode left implicit, because the
      view needs them -- and then the same two tensors from torch ops over that view: the label
      column cloned, the ids gathered from the input at bytes_off[:, None] + arange(12);
  (copy) a device-to-device copy of as many bytes as (a) reads and writes, the box's copy rate.

The variants alternate inside one process on one device. (a) is accepted when every run of it is
faster than every run of (b) and the outputs are equal. C3 (64 outputs of width 64) is timed as a
second, unjudged data point. --small: a 1/16 share, for a quick check of the tool itself.
"""
import argparse
import os
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
for p in (str(REPO / "tfrecords-reader_amd"), str(REPO)):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402
from tfr_reader import dense as D  # noqa: E402
from tfr_reader import shard  # noqa: E402


class _DevArray:
    """A library-owned device column as a torch tensor (``torch.as_tensor`` of this)."""

    def __init__(self, ptr: int, n: int, typestr: str) -> None:
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def column(ptr, n: int, typestr: str, dev):
    import ctypes as C

    return torch.as_tensor(_DevArray(C.cast(ptr, C.c_void_p).value, n, typestr), device=dev)


class Resident:
    """A workload resident in HBM with one decode context (one batch), decoded on `stream`."""

    def __init__(self, w, dev, stream, env=None, share=None) -> None:
        for k, v in (env or {}).items():
            os.environ[k] = v
        self.sd = shard.ShardDecoder(dev.index, 1 << 31, 1)
        self.plan = self.sd.plan(w.starts, w.ends, int(w.buf.size))
        assert len(self.plan) == 1, "one batch expected"
        self.dec = self.sd._decoders(1)[0]
        for k in env or {}:
            del os.environ[k]
        self.w, self.dev, self.stream = w, dev, stream
        self.n = w.n
        nbytes = int(w.buf.size)
        rst, ren, self.firsts = self.sd.rebase32(self.plan, w.starts, w.ends)
        if share is not None:  # (one resident copy of the input)
            self.d_bytes, self.d_st, self.d_en = share.d_bytes, share.d_st, share.d_en
        else:
            self.d_bytes = torch.zeros(((nbytes + 15) // 16) * 16 + 16, dtype=torch.uint8, device=dev)
            self.d_bytes[:nbytes].copy_(torch.from_numpy(w.buf))
            self.d_st = torch.from_numpy(rst.view(np.int32)).to(dev) if rst is not None else None
            self.d_en = torch.from_numpy(ren.view(np.int32)).to(dev)
        self.sd.learn(self.plan, w.buf, w.starts, w.ends)
        self.dec.set_record_bound(w.max_record)

    def decode(self):
        self.sd.decode_device32(self.plan, self.d_bytes.data_ptr(),
                                self.d_st.data_ptr() if self.d_st is not None else None, self.d_en.data_ptr(), self.firsts,
                                streams=[self.stream.cuda_stream])
        info = self.dec.info()  # confirms the optimistic decode (synchronizes)
        assert info.n_errors == 0 and info.n_miss_records == 0
        return info


def timed(stream, fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(name: str, ms: list[float], nbytes: int | None = None) -> str:
    s = f"{name:<28} runs ms: " + " ".join(f"{x:8.4f}" for x in ms)
    s += f" | median {statistics.median(ms):8.4f} min {min(ms):8.4f} max {max(ms):8.4f}"
    if nbytes:
        s += f" | {nbytes / (statistics.median(ms) * 1e-3) / 1e9:8.1f} GB/s on {nbytes} algorithmic bytes"
    return s


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-c3", action="store_true", help="skip the C3 data point (counter runs: tools/pmc_traffic.py)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    lines: list[str] = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    stream = torch.cuda.Stream(dev)
    w = bench.c4_workload("c1", 0, 8 * (16 if args.small else 1), 256, name="c4_c1_rank0of8")
    n = w.n
    say(f"workload {w.name}: {n} records, {int(w.buf.size)} framed bytes, device {torch.cuda.get_device_name(dev)}")
    specs = [D.Dense("label", "int64", 1), D.Dense("id", "uint8", 12)]
    with torch.cuda.stream(stream):
        res = {"a": Resident(w, dev, stream)}
        res["a_nt"] = Resident(w, dev, stream, {"TFRG_DENSE_NT": "1"}, share=res["a"])
        assert int(w.buf.size) < 1 << 31  # (the baseline reads bytes_off as int32)
        out = {k: {"label": torch.empty((n, 1), dtype=torch.int64, device=dev),
                   "id": torch.empty((n, 12), dtype=torch.uint8, device=dev)} for k in ("a", "a_nt")}
        ar12 = torch.arange(12, device=dev, dtype=torch.int64)
        algo = n * (8 + 4 + 8 + 12)  # read label + bytes_off, written label + id; the ids' input lines on top
        src = torch.empty(algo // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        ms = {"a": [], "a_nt": [], "b": [], "copy": []}
        b_out = {}

        def run_a(k: str) -> None:
            r = res[k]
            info = r.decode()
            assert int(info.implicit_cols) == 7 and int(info.placed_slots) & 3 == 3, "not an optimistic decode"
            ms[k].append(timed(stream, lambda: r.dec.dense(specs, out=out[k], stream=stream.cuda_stream)))

        def run_b() -> None:
            r = res["a"]
            r.decode()

            def body() -> None:
                cols = r.dec.device_columns()  # fills the implicit columns on the decode's stream
                i64 = column(cols.i64, n, "<i8", dev)
                boff = column(cols.bytes_off, n, "<i4", dev)
                b_out["label"] = i64.clone().view(n, 1)
                idx = boff.to(torch.int64)[:, None] + ar12
                b_out["id"] = r.d_bytes[idx]

            ms["b"].append(timed(stream, body))

        for _ in range(2):  # warm-up: allocator, kernels, templates
            run_a("a")
            run_a("a_nt")
            run_b()
            dst.copy_(src)
        for k in ms:
            ms[k].clear()
        for _ in range(args.runs):
            run_a("a")
            run_a("a_nt")
            run_b()
            ms["copy"].append(timed(stream, lambda: dst.copy_(src)))
        torch.cuda.synchronize(dev)
        equal = all(torch.equal(out[k][name], b_out[name]) for k in ("a", "a_nt") for name in ("label", "id"))
        say(summary("(a) tfrg_result_dense", ms["a"], algo))
        say(summary("(a-nt) nontemporal stores", ms["a_nt"], algo))
        say(summary("(b) device view + torch ops", ms["b"]))
        say(summary("(copy) torch D2D copy", ms["copy"], algo))
        say(f"outputs equal: {equal}")
        accept = equal and max(ms["a"]) < min(ms["b"])
        say(f"accept (every run of (a) faster than every run of (b), outputs equal): {accept}")
        # the project's rule for a policy change: every run faster and medians apart by more than
        # twice the other's range
        rng = lambda v: max(v) - min(v)  # noqa: E731
        nt_wins = max(ms["a_nt"]) < min(ms["a"]) and \
            statistics.median(ms["a"]) - statistics.median(ms["a_nt"]) > 2 * rng(ms["a"])
        df_wins = max(ms["a"]) < min(ms["a_nt"]) and \
            statistics.median(ms["a_nt"]) - statistics.median(ms["a"]) > 2 * rng(ms["a_nt"])
        say(f"store policy: nt wins {nt_wins}, default wins {df_wins} (neither: the default stays)")
        say("input lines the ids touch: not part of this run (counters-only run: tools/pmc_traffic.py <outdir> dense)")
        for r in res.values():
            r.sd.close()
        del res, out, b_out, src, dst

        if args.no_c3:
            return
        # second data point, unjudged: C3, all 64 slots at width 64
        w3 = bench.single_workload("c3")
        r3 = Resident(w3, dev, stream)
        kt = r3.dec.keys
        keys = [(kt.key_str[k], "int64" if kd == 3 else "float32") for k, kd in zip(kt.slot_key, kt.slot_kind)
                if kd in (2, 3)]
        specs3 = [D.Dense(k, dt, 64, fill=-1) for k, dt in keys[:64]]
        out3 = {s.out_name: torch.empty((w3.n, 64), dtype=torch.int64 if s.dtype == "int64" else torch.float32,
                                        device=dev) for s in specs3}
        t3 = []
        for i in range(args.runs + 1):
            r3.decode()
            t = timed(stream, lambda: r3.dec.dense(specs3, out=out3, stream=stream.cuda_stream))
            if i:
                t3.append(t)
        written = sum(t.numel() * t.element_size() for t in out3.values())
        say(f"workload c3: {w3.n} records, {len(specs3)} outputs of width 64")
        say(summary("(c3) tfrg_result_dense", t3, written) + " (bytes written only)")
        r3.sd.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
