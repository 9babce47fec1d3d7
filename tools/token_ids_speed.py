#!/usr/bin/env python3
"""Paired timing of token ids (tfrg_result_token_ids) against two yardsticks over the same rows.

Two decodes, each resident in HBM and confirmed, and for each one row list drawn at random with repeats:

  sentences  `--records` records with one sentence of 30..300 bytes of 5-byte words ("%05x", drawn from
             140,000 names) under "t" and the same words, one element each, under "w";
  documents  `--docs` records with one document of 4 KiB of the same words under "t".

Calls, each into preallocated outputs of the exact size:

  tok-hash       tfrg_result_token_ids on "t", vocab NULL, 1000 buckets, the default split (256 bytes);
  tok-vocab      the same with a vocabulary of the first 100,000 names and 1000 OOV buckets after it;
  tok-hash-wave  tok-hash with the split at 8: every row by a wave;
  tok-hash-lane  tok-hash with the split at 65536: every row by a lane;
  tok-hash-t64   tok-hash with 64 rows a tile (tfrg_ctx_set_ragged_tile) instead of 1024: 16 times the workgroups;
  elems          tfrg_result_ragged_elems on "t": reads the same bytes once and writes them back;
  elem-ids       tfrg_result_elem_ids on "w" (sentences only): one element per word, pure hashing.

A run is `--steps` calls of one variant between two device events on the consumer stream; the variants of
a decode alternate run by run in one process, after a warm-up of each. Per variant: the runs' ms per
call, their median, minimum and maximum; then the ratios of the medians to both yardsticks. Nothing is judged.

usage (GPU box): token_ids_speed.py [--runs 7] [--steps 20] [--records 65536] [--docs 4096] [--out FILE]
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
from tfr_reader import tokens as T  # noqa: E402, N812

NAMES, WORDS, BUCKETS = 140_000, 100_000, 1000


def workload(records: int, lo: int, hi: int, per_word: bool, seed: int):
    """`records` records of one text of lo..hi bytes of 5-byte words (6 bytes with the space)."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(lo // 6, hi // 6 + 1, records)
    draws = rng.integers(0, NAMES, int(counts.sum()))
    recs, at = [], 0
    for r, c in enumerate(counts.tolist()):
        words = [b"%05x" % i for i in draws[at : at + c]]
        feats = [("t", "bytes_list", [b" ".join(words)]), ("n", "int64_list", [r])]
        if per_word:
            feats.append(("w", "bytes_list", words))
        recs.append(writer.encode_example(feats))
        at += c
    return synth.framed(recs)


def measure(say, dev, stream, title: str, records: int, lo: int, hi: int, per_word: bool, runs: int, steps: int, vocab) -> None:
    dec = hip.HipDecoder(0)
    res = dec.decode(*workload(records, lo, hi, per_word, 1))
    assert int(res.status.max()) == 0
    s_t = D.resolve_slot(dec, R.RaggedElements("t"))
    m = records
    rows = torch.from_numpy(np.random.default_rng(2).integers(0, records, m)).to(dev)
    rw = D.rows_arg(rows)
    h = stream.cuda_stream
    n_tok = dec.token_ids([T.TokenIds("t", num_oov_buckets=BUCKETS)], rows=rows).totals["t"]  # exact sizes, once
    n_el, n_by = dec.ragged_elements([R.RaggedElements("t")], rows=rows).totals["t"]
    ids = torch.empty(n_tok, dtype=torch.int64, device=dev)
    ro = torch.empty(m + 1, dtype=torch.int64, device=dev)
    values = torch.empty(n_by, dtype=torch.uint8, device=dev)
    eo = torch.empty(n_el + 1, dtype=torch.int64, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    stats = torch.empty(4, dtype=torch.int32, device=dev)

    def tok(split: int, voc, tile: int = 0):
        def step() -> None:
            dec.set_ragged_tile(tile)
            dec.set_token_split(split)
            T.launch_tokens(dec, [(s_t, 0, 0, 0, (0, 0), voc, BUCKETS, WORDS if voc else 0, -1, n_tok, ids.data_ptr(), ro.data_ptr())],
                            rw, m, 0, totals.data_ptr(), stats.data_ptr(), h)
        return step

    def elems_step() -> None:
        dec.set_ragged_tile(0)
        R.launch_elems(dec, [(s_t, 0, 0, n_el, n_by, values.data_ptr(), eo.data_ptr(), ro.data_ptr())], rw, m, 0,
                       totals.data_ptr(), stats.data_ptr(), h)

    variants = {"tok-hash": tok(0, None), "tok-vocab": tok(0, vocab._handle().value), "tok-hash-wave": tok(8, None),
                "tok-hash-lane": tok(65536, None), "tok-hash-t64": tok(0, None, 64), "elems": elems_step}
    if per_word:
        s_w = D.resolve_slot(dec, R.RaggedElements("w"))

        def elem_ids_step() -> None:
            dec.set_ragged_tile(0)
            I.launch_ids(dec, [(s_w, 0, None, BUCKETS, 0, -1, n_tok, ids.data_ptr(), ro.data_ptr())], rw, m, 0, totals.data_ptr(),
                         stats.data_ptr(), h)

        variants["elem-ids"] = elem_ids_step
    for f in variants.values():  # warm-up
        for _ in range(3):
            f()
    torch.cuda.synchronize(dev)
    variants["tok-vocab"]()
    torch.cuda.synchronize(dev)
    unmatched = int(stats.cpu().numpy().view(np.uint32)[1])
    ms: dict[str, list[float]] = {k: [] for k in variants}
    for _ in range(runs):
        for name, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(steps):
                f()
            e1.record(stream)
            torch.cuda.synchronize(dev)
            ms[name].append(e0.elapsed_time(e1) / steps)
    say(f"{title}: {records} records of {lo}..{hi} bytes, m = {m} rows, T = {n_tok} tokens in B = {n_by} bytes; {unmatched} of "
        f"{n_tok} tokens out of vocabulary; {runs} interleaved runs of {steps} calls, ms per call between two device events")
    med = {}
    for name, v in ms.items():
        med[name] = statistics.median(v)
        say(f"  {name:13s} median {med[name]:.4f} (min {min(v):.4f}, max {max(v):.4f})  runs: " + " ".join(f"{x:.4f}" for x in v))
    for y in ("elems", "elem-ids"):
        if y in med:
            say(f"  ratio to {y}: " + ", ".join(f"{k} {med[k] / med[y]:.2f}" for k in med if k.startswith("tok")))
    dec.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines: list[str] = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    stream = torch.cuda.Stream(dev)  # the consumer stream of every call: the events on it bracket the calls' work
    torch.cuda.set_stream(stream)
    vocab = I.Vocabulary([b"%05x" % i for i in range(WORDS)], device=0)
    say(f"tools/token_ids_speed.py on {torch.cuda.get_device_name(dev)}; vocabulary of {WORDS} words (capacity "
        f"{vocab.info['capacity']}, max_probe {vocab.info['max_probe']})")
    measure(say, dev, stream, "sentences", a.records, 30, 300, True, a.runs, a.steps, vocab)
    measure(say, dev, stream, "documents", a.docs, 4096, 4096, False, a.runs, a.steps, vocab)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    vocab.close()


if __name__ == "__main__":
    main()
