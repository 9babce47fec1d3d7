#!/usr/bin/env python3
"""Paired timing of raw tensors (tfrg_result_raw_rows) against what the row-list passes without it compose.

One decode, resident in HBM and confirmed: `--records` records with one 224 x 224 x 3 uint8 image each
(``image.tobytes()``), and one row list of `--rows` entries, a slice of a ``torch.randperm``, on the
device. The result wanted is ``[rows, 3, 224, 224]`` bfloat16, ImageNet-normalised. Three variants, in
this order:

  raw       HipDecoder.raw: one launch, into a preallocated output;
  composed  HipDecoder.ragged(rows=) as packed uint8 with the exact capacity, then torch ``view`` /
            ``permute`` / ``to(bfloat16)`` / ``sub`` / ``div`` (what can be written without raw);
  read      tfrg_stream_read (variant 0) over as many bytes as raw moves: the card's HBM read rate.

A run is `--steps` calls of one variant between two device events on the stream; the variants alternate
run by run in one process, after a warm-up of each. Per variant: the runs' ms per call, their median,
minimum and maximum, and GB/s as (element bytes read + output bytes written) / median. Nothing is judged.

usage (GPU box): raw_speed.py [--runs 7] [--steps 20] [--records 8192] [--rows 256] [--out FILE]
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "tfrecords-reader_amd"), str(REPO)]

from tfr_reader import _native as N  # noqa: E402
from tfr_reader import hip  # noqa: E402
from tfr_reader import ragged as R  # noqa: E402
from tfr_reader import raw as W  # noqa: E402
from tfr_reader import synth, writer  # noqa: E402

H, WID, CH = 224, 224, 3
MEAN, STD = np.array([0.485, 0.456, 0.406]) * 255, np.array([0.229, 0.224, 0.225]) * 255


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--records", type=int, default=8192)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines: list[str] = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(1)
    img = H * WID * CH
    recs = [writer.encode_example([("image", "bytes_list", [rng.integers(0, 256, img, dtype=np.uint8).tobytes()]),
                                   ("label", "int64_list", [i % 1000])]) for i in range(a.records)]
    dec = hip.HipDecoder(0)
    res = dec.decode(*synth.framed(recs))
    del recs
    assert int(res.status.max()) == 0
    m = a.rows
    rows = torch.randperm(a.records, device=dev)[:m].contiguous()
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    spec = W.Raw.normalize("image", MEAN, STD, out="bfloat16", shape=(H, WID, CH), channels=CH, planar=True)
    out = torch.empty((m, CH, H, WID), dtype=torch.bfloat16, device=dev)
    packed = torch.empty(m * img, dtype=torch.uint8, device=dev)
    offsets = torch.empty(m + 1, dtype=torch.int64, device=dev)
    mean = torch.tensor(MEAN, dtype=torch.bfloat16, device=dev).view(1, CH, 1, 1)
    std = torch.tensor(STD, dtype=torch.bfloat16, device=dev).view(1, CH, 1, 1)
    moved = m * img * 3  # (one byte read and two written per element)
    src = torch.empty((moved + 15) // 16 * 16, dtype=torch.uint8, device=dev)
    sink = torch.zeros(4, dtype=torch.int32, device=dev)
    lib = N.lib()

    def raw_step():
        return dec.raw([spec], rows=rows, out={"image": out})["image"]

    def composed_step():
        v, _ = dec.ragged([R.Ragged("image", "uint8")], rows=rows, out={"image": (packed, offsets)})["image"]
        return v.view(m, H, WID, CH).permute(0, 3, 1, 2).to(torch.bfloat16).sub(mean).div(std)

    def read_step():
        N.check(lib.tfrg_stream_read(src.data_ptr(), src.numel(), sink.data_ptr(), stream.cuda_stream, 0), "tfrg_stream_read")

    variants = {"raw": raw_step, "composed": composed_step, "read": read_step}
    for f in variants.values():  # warm-up
        for _ in range(3):
            f()
    torch.cuda.synchronize(dev)
    close = (raw_step().float() - composed_step().float()).abs().max().item()
    ms: dict[str, list[float]] = {k: [] for k in variants}
    for _ in range(a.runs):
        for name, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.steps):
                f()
            e1.record(stream)
            torch.cuda.synchronize(dev)
            ms[name].append(e0.elapsed_time(e1) / a.steps)
    say(f"tools/raw_speed.py on {torch.cuda.get_device_name(dev)}: {a.records} records of one {H}x{WID}x{CH} uint8 image, "
        f"m = {m} rows of a randperm -> [{m}, {CH}, {H}, {WID}] bfloat16, ImageNet normalise; {moved} bytes moved per call "
        f"(element bytes read + output bytes written); {a.runs} interleaved runs of {a.steps} calls, ms per call between two "
        f"device events; largest difference between the two results {close:.4f} (the composition rounds three times)")
    for name, v in ms.items():
        med = statistics.median(v)
        say(f"  {name:8s} median {med:.4f} ms = {moved / med / 1e6:8.1f} GB/s (min {min(v):.4f}, max {max(v):.4f})  runs: "
            + " ".join(f"{x:.4f}" for x in v))
    say(f"  composed / raw: {statistics.median(ms['composed']) / statistics.median(ms['raw']):.2f}")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    dec.close()


if __name__ == "__main__":
    main()
