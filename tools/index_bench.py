"""Device time of one tfrg_index_device next to a streaming read of the same bytes.

    python tools/index_bench.py [--runs 5] [--small] [--out profiles/frame_index/kernels.json]

Three images: C1 (rank 0 of 8's share of the 256-file C1 directory, its files as pieces), C2
(8,189 flower records, one piece) and C3 (8,192 wide records tiled 16 times, one piece). Per image:
HIP events around one ``tfrg_index_device`` on the context's stream (the call synchronises once,
so the event pair brackets every kernel and the summary's D2H), after one warm-up call, ``--runs``
times; ``tfrg_stream_read`` of the same bytes (variant 0) timed the same way; and the index checked
against the host walk of every piece. The ratio is reported, not gated.
"""

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tfrecords-reader_amd"))

from tfr_reader import _native as N  # noqa: E402
from tfr_reader import hip, shard, synth  # noqa: E402
from tfr_reader.cython import indexer as native  # noqa: E402


def images(small: bool):
    n_files = 16 if small else 256
    sizes = synth.c4_file_sizes(n_files, "c1", base=(1 << 14) if small else None)
    mine = shard.lpt_partition(sizes.tolist(), 8)[0]
    yield "c1_rank0of8", [synth.c4_file(f, "c1", base=(1 << 14) if small else None) for f in mine]
    yield "c2", [synth.framed(synth.c2_payloads(512 if small else 8189, seed=2))[0]]
    base = synth.framed(synth.c3_payloads(512 if small else 8192, seed=3))
    yield "c3_x16", [synth.replicate(*base, 16)[0]]


def host_walk(pieces):
    t0 = time.perf_counter()
    rows, base = [], 0
    for p in pieces:
        rows.append(native.index_buffer(p)[:, :2] + np.uint64(base))
        base += p.size
    return np.concatenate(rows), (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--chunk", type=int, default=0, help="tfrg_ctx_set_index_chunk (0: the default)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = N.lib()
    dec = hip.HipDecoder(0)
    dec.set_index_chunk(a.chunk)
    out = {"chunk": a.chunk or 4096, "runs": a.runs, "images": {}}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for name, pieces in images(a.small):
        sizes = np.array([p.size for p in pieces], np.uint64)
        nbytes = int(sizes.sum())
        pad = np.zeros(((nbytes + 15) & ~15) + 32, np.uint8)
        pad[:nbytes] = np.concatenate(pieces)
        d = torch.from_numpy(pad).cuda()
        want, host_ms = host_walk(pieces)
        ix = dec.index_device(d, nbytes, sizes)  # warm-up, and the result that is checked
        assert ix.fallback == 0 and ix.n == want.shape[0]
        assert np.array_equal(ix.start.cpu().numpy().view(np.uint64), want[:, 0])
        assert np.array_equal(ix.end.cpu().numpy().view(np.uint64), want[:, 1])
        st, en, e32 = ix.start, ix.end, ix.end32
        info = N.TfrgIndexInfo()
        s = torch.cuda.Stream()
        sink = torch.zeros(4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        idx_ms, read_ms = [], []
        with torch.cuda.stream(s):
            for _ in range(a.runs):
                ev[0].record(s)
                N.check(lib.tfrg_index_device(dec._ctx, C.c_void_p(d.data_ptr()), nbytes, N.ptr(sizes, N.u64p),
                                              sizes.size, C.c_void_p(st.data_ptr()), C.c_void_p(en.data_ptr()),
                                              C.c_void_p(e32.data_ptr()), ix.n, None, C.c_void_p(s.cuda_stream),
                                              C.byref(info)), "tfrg_index_device")
                ev[1].record(s)
                ev[1].synchronize()
                idx_ms.append(round(ev[0].elapsed_time(ev[1]), 4))
            for _ in range(a.runs + 1):
                ev[0].record(s)
                N.check(lib.tfrg_stream_read(C.c_void_p(d.data_ptr()), nbytes & ~15, C.c_void_p(sink.data_ptr()),
                                             C.c_void_p(s.cuda_stream), 0), "tfrg_stream_read")
                ev[1].record(s)
                ev[1].synchronize()
                read_ms.append(round(ev[0].elapsed_time(ev[1]), 4))
        read_ms = read_ms[1:]
        out["images"][name] = {
            "bytes": nbytes, "pieces": int(sizes.size), "records": ix.n, "n_chunks": ix.n_chunks,
            "repaired_chunks": ix.repaired_chunks, "repair_rounds": ix.repair_rounds, "tiled": ix.tiled,
            "index_device_ms": idx_ms, "stream_read_ms": read_ms,
            "index_over_read": round(float(np.median(idx_ms) / np.median(read_ms)), 2),
            "index_GBps": round(nbytes / np.median(idx_ms) / 1e6, 1),
            "host_walk_ms_one_thread": round(host_ms, 2),
        }
        print(name, json.dumps(out["images"][name]), flush=True)
        del d, st, en, e32, ix
    dec.close()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
