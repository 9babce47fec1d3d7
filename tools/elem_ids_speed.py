#!/usr/bin/env python3
"""Paired timing of element ids (tfrg_result_elem_ids) against tfrg_result_ragged_elems over the same rows.

One decode, resident in HBM and confirmed: `--records` records of 1..20 class strings of 10 bytes
("cls-%06d", drawn from 140,000 names), and one row list of `--rows` entries drawn at random with
repeats, on the device. Three calls, each into preallocated outputs of the exact size:

  hash    tfrg_result_elem_ids, vocab NULL, 1000 buckets (pure hashing);
  vocab   tfrg_result_elem_ids, a vocabulary of the first 100,000 names, 1000 OOV buckets after it;
  elems   tfrg_result_ragged_elems: the yardstick, which reads the same element bytes and writes them back.

A run is `--steps` calls of one variant between two device events on the stream; the three variants
alternate run by run in one process (hash, vocab, elems, hash, ...), after a warm-up of each. Per
variant: the runs' ms per call, their median, minimum and maximum; then the ratios of the medians to the
yardstick's. Nothing is judged.

usage (GPU box): elem_ids_speed.py [--runs 7] [--steps 50] [--records 65536] [--rows 65536] [--out FILE]
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "tfrecords-reader_amd"), str(REPO)]

from tfr_reader import dense as D  # noqa: E402
from tfr_reader import hip  # noqa: E402
from tfr_reader import ids as I  # noqa: E402, N812
from tfr_reader import ragged as R  # noqa: E402
from tfr_reader import synth, writer  # noqa: E402

KEY = "b"
NAMES, WORDS, BUCKETS = 140_000, 100_000, 1000


def workload(records: int, seed: int = 1):
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 21, records)
    draws = rng.integers(0, NAMES, int(counts.sum()))
    recs, at = [], 0
    for r, c in enumerate(counts.tolist()):
        recs.append(writer.encode_example([(KEY, "bytes_list", [b"cls-%06d" % i for i in draws[at : at + c]]),
                                           ("n", "int64_list", [r])]))
        at += c
    return synth.framed(recs)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines: list[str] = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    dec = hip.HipDecoder(0)
    res = dec.decode(*workload(a.records))
    assert int(res.status.max()) == 0
    slot = D.resolve_slot(dec, R.RaggedElements(KEY))
    vocab = I.Vocabulary([b"cls-%06d" % i for i in range(WORDS)], device=0)
    m = a.rows
    rows = torch.from_numpy(np.random.default_rng(2).integers(0, a.records, m)).to(dev)
    rw = D.rows_arg(rows)
    stream = torch.cuda.Stream(dev)  # the consumer stream of every call: the events on it bracket the calls' work
    torch.cuda.set_stream(stream)
    # exact sizes, once
    first = dec.ragged_elements([R.RaggedElements(KEY)], rows=rows)
    n_el, n_by = first.totals[KEY]
    ids = torch.empty(n_el, dtype=torch.int64, device=dev)
    ro = torch.empty(m + 1, dtype=torch.int64, device=dev)
    values = torch.empty(n_by, dtype=torch.uint8, device=dev)
    eo = torch.empty(n_el + 1, dtype=torch.int64, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    stats = torch.empty(4, dtype=torch.int32, device=dev)
    h = stream.cuda_stream

    def hash_step() -> None:
        I.launch_ids(dec, [(slot, 0, None, BUCKETS, 0, -1, n_el, ids.data_ptr(), ro.data_ptr())], rw, m, 0, totals.data_ptr(),
                     stats.data_ptr(), h)

    def vocab_step() -> None:
        I.launch_ids(dec, [(slot, 0, vocab._handle().value, BUCKETS, WORDS, -1, n_el, ids.data_ptr(), ro.data_ptr())], rw, m, 0,
                     totals.data_ptr(), stats.data_ptr(), h)

    def elems_step() -> None:
        R.launch_elems(dec, [(slot, 0, 0, n_el, n_by, values.data_ptr(), eo.data_ptr(), ro.data_ptr())], rw, m, 0,
                       totals.data_ptr(), stats.data_ptr(), h)

    variants = {"hash": hash_step, "vocab": vocab_step, "elems": elems_step}
    for f in variants.values():  # warm-up
        for _ in range(5):
            f()
    torch.cuda.synchronize(dev)
    vocab_step()
    torch.cuda.synchronize(dev)
    unmatched = int(stats.cpu().numpy().view(np.uint32)[1])
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
    say(f"tools/elem_ids_speed.py on {torch.cuda.get_device_name(dev)}: {a.records} records, m = {m} rows, E = {n_el} elements "
        f"of 10 bytes, B = {n_by} bytes; vocabulary of {WORDS} words (capacity {vocab.info['capacity']}, max_probe "
        f"{vocab.info['max_probe']}), {unmatched} of {n_el} elements out of vocabulary; {a.runs} interleaved runs of {a.steps} calls, "
        "ms per call between two device events")
    med = {}
    for name, v in ms.items():
        med[name] = statistics.median(v)
        say(f"  {name:5s} median {med[name]:.4f} (min {min(v):.4f}, max {max(v):.4f})  runs: " + " ".join(f"{x:.4f}" for x in v))
    say(f"  ratio to elems: hash {med['hash'] / med['elems']:.2f}, vocab {med['vocab'] / med['elems']:.2f}")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    vocab.close()
    dec.close()


if __name__ == "__main__":
    main()
