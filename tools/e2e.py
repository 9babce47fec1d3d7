#!/usr/bin/env python3
"""End-to-end rate, measured in one timed run: TFRecord files on disk -> every value in host memory
(BASELINE.json north_star).

The directory is written first (C4 layout: file f of default_rng(1000 + f), C1 / C2 / C3 record
shapes), then ONE timed pass streams it through ``tfr_reader.stream.StreamDecoder``: mmap of each
file, native copy into pinned staging (worker threads), native framing index, H2D, device decode
(framing + CRC-32C + Example decode + columnar gather, bytes_list payloads gathered into a device
byte column), D2H of every column into numpy arrays. Two slots overlap staging/H2D of batch k+1
with the decode of batch k. The page cache is warm (the files were just written; dropping it needs
root): the rate is host memory -> values, not disk -> values. A second figure times turning a
batch of records into Python ``Feature`` objects with every ``.value`` read (the reference's
output form).

usage: e2e.py [--config c1|c2|c3] [--files N] [--batch-mib M] [--out PATH]
"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "tfrecords-reader_amd"), str(REPO)]

import numpy as np  # noqa: E402

from tfr_reader import stream, synth, writer  # noqa: E402


def write_dir(d: Path, config: str, n_files: int) -> list[str]:
    paths = []
    for f in range(n_files):
        p = d / f"part-{f:05d}.tfrecord"
        if config == "c1":
            synth.c4_file(f, "c1").tofile(p)
        elif config == "c2":
            synth.c4_file(f, "c2").tofile(p)
        else:
            writer.write_tfrecord(p, synth.c3_payloads(4096, seed=1000 + f))
        paths.append(str(p))
    return paths


def alternate(paths, a) -> dict:
    """a.alternate timed passes per index mode, host and device alternating: per mode the walls (s), the
    summed index stage (worker_ms[1]) and all four stages of every pass, and whether every device pass
    beat every host pass on wall and index stage (the only ground for calling it faster). With the
    device index the bytes' H2D is part of the index stage (the index waits for it) and no longer of
    the H2D + decode stage: compare the two stages' sum across modes."""
    sds = {m: stream.StreamDecoder(0, batch_bytes=a.batch_mib << 20, copy_threads=8, copy_results=a.copy,
                                   device_index=(m == "device")) for m in ("host", "device")}
    res = {m: {"wall_s": [], "index_ms": [], "stage_ms": [], "records": 0} for m in sds}
    for sd in sds.values():  # warm-up: contexts, keys, pinned buffers, index scratch
        for _ in range(2):
            for _b in sd.batches(paths):
                pass
    for _ in range(a.alternate):
        for m, sd in sds.items():
            t0 = time.perf_counter()
            ms = np.zeros(4)
            n = 0
            for b in sd.batches(paths):
                assert not b.result.status.any()
                ms += np.array(b.stage_ms)
                n += len(b.result)
            res[m]["wall_s"].append(round(time.perf_counter() - t0, 4))
            res[m]["index_ms"].append(round(float(ms[1]), 2))
            res[m]["stage_ms"].append(np.round(ms, 2).tolist())  # read+copy, index, H2D + decode, D2H
            res[m]["records"] = n
    for sd in sds.values():
        sd.close()
    assert res["host"]["records"] == res["device"]["records"]
    res["device_faster_every_run"] = bool(max(res["device"]["wall_s"]) < min(res["host"]["wall_s"]) and
                                          max(res["device"]["index_ms"]) < min(res["host"]["index_ms"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c1", choices=["c1", "c2", "c3"])
    ap.add_argument("--files", type=int, default=None)
    ap.add_argument("--batch-mib", type=int, default=256)
    ap.add_argument("--sample", type=int, default=0,
                    help="records of the last batch turned into Python Feature values (0: all of them: a "
                         "batch's columns become Python objects once, so a part of a batch pays for all of it)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--copy", action="store_true", help="copy each batch's columns out of the pinned buffers")
    ap.add_argument("--passes", type=int, default=7, help="timed passes over the directory (median reported)")
    ap.add_argument("--device-index", action="store_true",
                    help="build every batch's framing index on the device (StreamDecoder(device_index=True))")
    ap.add_argument("--alternate", type=int, default=0, metavar="N",
                    help="after the report: N timed passes of each index mode (host, device), alternating in this "
                         "process over the same directory; their walls and index stage times are reported side by side")
    a = ap.parse_args()
    n_files = a.files or {"c1": 16, "c2": 32, "c3": 16}[a.config]
    with tempfile.TemporaryDirectory(dir="/tmp") as td:
        paths = write_dir(Path(td), a.config, n_files)
        file_bytes = sum(Path(p).stat().st_size for p in paths)
        sd = stream.StreamDecoder(0, batch_bytes=a.batch_mib << 20, copy_threads=8, copy_results=a.copy,
                                  device_index=a.device_index)
        # warm-up pass over the whole directory, not timed: device contexts, key learning, and the
        # pinned result buffers of both slots grown to full batches (steady state)
        for _ in range(2):  # (the first pass learns the keys: its first batch's results are partial)
            for b in sd.batches(paths):
                pass
        walls, stages = [], []
        for p in range(max(1, a.passes)):
            sd.timing = {k: 0.0 for k in sd.timing}
            t0 = time.perf_counter()
            n_rec = n_vals = 0
            stage_ms = np.zeros(4)
            last = None
            for b in sd.batches(paths):
                r = b.result
                assert not r.status.any()
                n_rec += len(r)
                n_vals += int(r.i64.size + r.f32.size + r.bytes_len.size)
                stage_ms += np.array(b.stage_ms)
                last = r
            walls.append(time.perf_counter() - t0)
            stages.append(stage_ms)
            if p + 1 < a.passes:
                del r, last
        med = int(np.argsort(walls)[len(walls) // 2])
        wall, stage_ms = walls[med], stages[med]
        timing = {k: round(v, 4) for k, v in sd.timing.items()}
        # Python Feature objects with every value read, on a sample of the last batch (its columns
        # may be views of the stream's pinned buffers: before the stream is closed)
        k = len(last) if a.sample <= 0 else min(a.sample, len(last))
        t1 = time.perf_counter()
        feats = last.features(0, k)
        nv = 0
        for f in feats:
            for key in f.fields_names if hasattr(f, "fields_names") else list(f.feature):
                nv += len(f[key].value)
        py_s = time.perf_counter() - t1
        del feats, last
        sd.close()
        alt = alternate(paths, a) if a.alternate > 0 else None
    out = {
        "config": a.config,
        "files": n_files,
        "file_bytes": file_bytes,
        "records": n_rec,
        "values": n_vals,
        "batch_MiB": a.batch_mib,
        "wall_s": round(wall, 4),
        "passes": len(walls),
        "wall_s_min_max": [round(min(walls), 4), round(max(walls), 4)],
        "GiB_s": round(file_bytes / wall / 2**30, 3),
        "examples_per_s": round(n_rec / wall, 1),
        "worker_ms": dict(zip(["read_copy", "index", "h2d_decode", "d2h"], np.round(stage_ms, 2).tolist())),
        "consumer_wait_s": timing,
        "python_features": {"records": k, "values": nv, "s": round(py_s, 4),
                            "records_per_s": round(k / py_s, 1)},
        "copy_results": a.copy,
        "device_index": bool(a.device_index),
        **({"alternate": alt} if alt else {}),
        "note": "median of the timed passes (wall_s; worker_ms of that pass), files on disk in the warm page cache -> every value in host memory: numpy "
                "columns over the stream's pinned result buffers (copied out with --copy); bytes_list payloads "
                "gathered on the device and copied back",
    }
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
