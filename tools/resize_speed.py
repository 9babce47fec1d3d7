#!/usr/bin/env python3
"""Timing of resized raw images (tfrg_result_raw_resize) against per-record torch ops on the same device.

m uint8 RGB records of mixed sizes around 500 x 375, random crop boxes and flips, to [m, 3, 224, 224]
bfloat16 planar. Alternating in one process, timed by device events over windows of a third of a second
(`--iters` calls, `--torch-iters` passes). The kernel's own time comes from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/resize_speed.py --rounds 1`, which names k_resize:
  resize:  HipDecoder.resize into a preallocated output (the memsets of its counters included);
  torch:   per record, a view of the packed image bytes (what ragged() hands back) -> crop -> float ->
           F.interpolate(bilinear) -> flip -> normalise -> bfloat16 into the same output.
Algorithmic bytes: the source crop rows that some output row taps, once each, plus the output.
`--antialias`: the same records, boxes and flips with `antialias=True` on both sides (k_resize_aa;
F.interpolate(..., antialias=True)); every crop row of a box is tapped, so the bytes are all of them once.
Prints one JSON line."""

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "tfrecords-reader_amd"), str(ROOT)]


def main() -> None:
    import torch
    import torch.nn.functional as F  # noqa: N812

    from tfr_reader import hip, synth, writer
    from tfr_reader import raw as W

    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--iters", type=int, default=1000, help="resize calls per timed window")
    ap.add_argument("--torch-iters", type=int, default=30, help="passes of the torch composition per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--antialias", action="store_true", help="the triangle filter on both sides")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM rate the fraction is taken of")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    m, dev = a.m, torch.device("cuda", 0)
    shapes = [(int(rng.integers(330, 420)), int(rng.integers(440, 560))) for _ in range(m)]
    imgs = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    payloads = [writer.encode_example([("height", "int64_list", [h]), ("width", "int64_list", [w]), ("image", "bytes_list", [i.tobytes()])])
                for (h, w), i in zip(shapes, imgs)]
    dec = hip.HipDecoder(0)
    dec.decode(*synth.framed(payloads))
    rows = rng.permutation(m)
    boxes = np.zeros((m, 4), np.int32)  # (per list entry: entry k draws record rows[k])
    for k, g in enumerate(rows.tolist()):
        h, w = shapes[g]
        ch, cw = int(rng.integers(h // 2, h + 1)), int(rng.integers(w // 2, w + 1))
        boxes[k] = [rng.integers(0, h - ch + 1), rng.integers(0, w - cw + 1), ch, cw]
    flips = rng.integers(0, 2, m).astype(np.uint8)
    mean, std = np.array([0.485, 0.456, 0.406]) * 255, np.array([0.229, 0.224, 0.225]) * 255
    sp = W.Resize.normalize("image", mean, std, size=(224, 224), channels=3, out="bfloat16", planar=True, antialias=a.antialias)
    d_rows, d_boxes, d_flips = (torch.from_numpy(x).to(dev) for x in (rows.astype(np.int64), boxes, flips))
    out = torch.empty((m, 3, 224, 224), dtype=torch.bfloat16, device=dev)

    def ours():
        dec.resize([sp], rows=d_rows, boxes=d_boxes, flip=d_flips, out={"image": out})

    packed = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(dev)
    offs = np.concatenate([[0], np.cumsum([i.size for i in imgs])])
    sc, bi = (torch.tensor(v, dtype=torch.float32, device=dev).view(1, 3, 1, 1) for v in (sp.scale, sp.bias))

    def theirs():
        for k, g in enumerate(rows.tolist()):
            h, w = shapes[g]
            t, l, ch, cw = boxes[k].tolist()
            x = packed[offs[g] : offs[g + 1]].view(h, w, 3)[t : t + ch, l : l + cw].permute(2, 0, 1)[None].float()
            y = F.interpolate(x, size=(224, 224), mode="bilinear", align_corners=False, antialias=a.antialias)
            out[k] = ((y.flip(-1) if flips[k] else y) * sc + bi)[0].to(torch.bfloat16)

    def timed(fn, iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(iters):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / iters

    ours(), theirs()
    torch.cuda.synchronize()
    t_ours, t_theirs = [], []
    for _ in range(a.rounds):
        t_ours.append(timed(ours, a.iters))
        t_theirs.append(timed(theirs, a.torch_iters))
    tapped = 0
    for k in range(m):
        _, _, ch, cw = boxes[k].tolist()
        y0, y1, _ = W.axis_coords(ch, 224, "bilinear")
        tapped += (ch if a.antialias else len(set(y0.tolist()) | set(y1.tolist()))) * cw * 3
    nbytes = tapped + out.numel() * 2
    best = min(t_ours)
    print(json.dumps({"m": m, "antialias": a.antialias, "resize_ms": sorted(round(t, 4) for t in t_ours), "torch_ms": sorted(round(t, 3) for t in t_theirs),
                      "algorithmic_bytes": int(nbytes), "resize_gbs_best": round(nbytes / best / 1e6, 1),
                      "hbm_fraction_best": round(nbytes / best / 1e6 / a.hbm_gbs, 4), "device": torch.cuda.get_device_name(0)}))
    dec.close()


if __name__ == "__main__":
    main()
