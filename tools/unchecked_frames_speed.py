#!/usr/bin/env python3
"""Decode speed of spec-framed and zero-CRC ("unchecked") files, with and without CRC verdicts.

The c4of8-shaped shard (files 0..31 of the C4 directory, C1 records) is built twice, with spec CRCs
and with both CRC fields 0 (synth.c4_file(f, "c1", crc=...)), kept resident in HBM and decoded as
bench.py's measure() does: ShardDecoder, decode_device32 on the u32 ends, batch_bytes 2^31, two
streams, the record bound set. Four cases: {spec file, zero file} x {crc=True, crc=False}.

A step is the decode of every batch AND its confirmation (ShardDecoder.infos, tfrg_result_info), as a
consumer runs it: an optimistic decode that left records is re-run in full inside the confirmation,
and that re-run is what a file without templates of its frame class pays per batch. Each case runs
`--repeats` timed runs of `--steps` steps between HIP events after `--warmup` steps; the figure is
the median run, with the fastest and slowest beside it (the box's spread). Re-runs are the growth of
device_bytes()[1] over all timed runs.

Uses only API older than the unchecked-frame templates, so the same file measures an older checkout
(copy it into that checkout's tools/): run both alternately in one job and compare case by case.

usage: unchecked_frames_speed.py [--steps N] [--warmup W] [--repeats R] [--files F] [--cache DIR]
                                  [--cases spec_file_crc_on,zero_file_crc_on,...] [--label TEXT]
Prints one JSON object.
"""
import argparse
import json
import statistics
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "tfrecords-reader_amd"), str(REPO)]

import torch  # noqa: E402

from tfr_reader import shard, synth  # noqa: E402


def build(files: int, crc: bool, cache: str | None):
    """(image, starts, ends) of the shard; cached as .npy under `cache` between runs of one job."""
    tag = Path(cache) / f"c4of8_{files}_{int(crc)}" if cache else None
    if tag and (tag.with_suffix(".buf.npy")).exists():
        return tuple(np.load(tag.with_suffix(f".{k}.npy")) for k in ("buf", "st", "en"))
    with ThreadPoolExecutor(16) as ex:
        imgs = list(ex.map(lambda f: synth.c4_file(f, "c1", crc=crc), range(files)))
    sb = shard.ShardBatch([synth.c4_file_name(f) for f in range(files)], imgs)
    out = (sb.buf, sb.starts, sb.ends)
    if tag:
        tag.parent.mkdir(parents=True, exist_ok=True)
        for k, a in zip(("buf", "st", "en"), out):
            np.save(tag.with_suffix(f".{k}.npy"), a)
    return out


def measure(dev, buf, starts, ends, crc: bool, steps: int, warmup: int, repeats: int) -> dict:
    sd = shard.ShardDecoder(dev.index, 1 << 31, 2)
    nbytes = int(buf.size)
    plan = sd.plan(starts, ends, nbytes)
    d_bytes = torch.zeros(((nbytes + 15) // 16) * 16 + 16, dtype=torch.uint8, device=dev)
    d_bytes[:nbytes].copy_(torch.from_numpy(buf))
    rst, ren, firsts = sd.rebase32(plan, starts, ends)
    assert rst is None, "the shard's records lie back to back"
    d_en = torch.from_numpy(ren.view(np.int32)).to(dev)
    sd.learn(plan, buf, starts, ends)
    bound = int((ends - starts).max())
    for d in sd._decoders(len(plan)):
        d.set_record_bound(bound)
    main = torch.cuda.current_stream(dev)
    side = [torch.cuda.Stream(dev) for _ in range(2)]
    handles = [s.cuda_stream for s in side]

    def step():
        sd.decode_device32(plan, d_bytes.data_ptr(), None, d_en.data_ptr(), firsts, streams=handles, crc=crc)
        return sd.infos(plan)

    for _ in range(max(1, warmup)):
        infos = step()
    torch.cuda.synchronize(dev)
    assert not any(i.n_miss_records or i.n_errors for i in infos)
    reruns0 = sd.device_bytes()[1]
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record(main)
        for s in side:
            s.wait_event(e0)
        for _ in range(steps):
            infos = step()
        for s in side:
            main.wait_stream(s)
        e1.record(main)
        torch.cuda.synchronize(dev)
        ms.append(e0.elapsed_time(e1) / steps)
    reruns = sd.device_bytes()[1] - reruns0
    framed = int((ends - starts).sum())
    med = statistics.median(ms)
    out = {
        "ms_per_step": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
        "GiB_s": round(framed / 2**30 / (med / 1e3), 1), "runs_ms": [round(x, 4) for x in ms],
        "reruns": int(reruns), "reruns_per_step": round(reruns / (steps * repeats * len(plan)), 3),
        "tpl_groups_missed": int(sum(i.tpl_groups_missed for i in infos)),
        "implicit_cols": [int(i.implicit_cols) for i in infos],
        "template_count": sd.decs[0].template_count(), "batches": len(plan), "records": int(starts.shape[0]),
        "framed_bytes": framed,
    }
    sd.close()
    del d_bytes, d_en
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--cache", default=None, help="directory for the generated shards (.npy), reused if present")
    ap.add_argument("--cases", default=None, help="comma-separated subset of the four cases (a profiler run)")
    ap.add_argument("--label", default="", help="copied into the output (which build this is)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    out = {"tool": "unchecked_frames_speed", "label": a.label, "steps": a.steps, "warmup": a.warmup,
           "repeats": a.repeats, "files": a.files, "device": torch.cuda.get_device_name(dev), "cases": {}}
    for file_kind, file_crc in (("spec", True), ("zero", False)):
        buf, st, en = build(a.files, file_crc, a.cache)
        for crc in (True, False):
            name = f"{file_kind}_file_crc_{'on' if crc else 'off'}"
            if a.cases is None or name in a.cases.split(","):
                out["cases"][name] = measure(dev, buf, st, en, crc, a.steps, a.warmup, a.repeats)
        del buf, st, en
    print(json.dumps(out))


if __name__ == "__main__":
    main()
