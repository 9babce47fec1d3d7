#!/usr/bin/env python3
"""Paired timing of WordPiece ids (tfrg_result_wordpiece_ids) against two yardsticks over the same rows.

The decodes, the row lists and the method are tools/token_ids_speed.py's: "sentences" (records of one
sentence of 30..300 bytes of 5-byte words "%05x" drawn from 140,000 names) and "documents" (records of one
4 KiB document), each resident in HBM and confirmed, one row list drawn at random with repeats, 64 rows a
tile for every variant. The WordPiece vocabulary holds the first 98,000 names whole (about 70 % of the
words), and the 16 hex digits as first and as continuation pieces, so that every other word is cut into
five one-byte pieces: the case in which a piece's candidate ends are tried one after the other.

Calls, each into preallocated outputs of the exact size:

  wp            tfrg_result_wordpiece_ids on "t", the default split;
  wp-special    the same with cls / sep and max_pieces 128;
  tok-vocab     tfrg_result_token_ids on "t" with a vocabulary of the first 100,000 names and 1000 buckets;
  elems         tfrg_result_ragged_elems on "t": reads the same bytes once and writes them back.

A run is `--steps` calls of one variant between two device events on the consumer stream; the variants
alternate run by run in one process, after a warm-up of each. Per variant: the runs' ms per call, their
median, minimum and maximum; then the ratios of the medians to both yardsticks. Nothing is judged.

The lanes per word of the match (kWpG in csrc/tfrg_wordpiece.h) are a build-time constant: to time G = 1,
build `make -C tfrecords-reader_amd/csrc WP_G=1 BUILD=build_g1 OUT=../tfr_reader/libtfrg_g1.so
../tfr_reader/libtfrg_g1.so` and run this tool a second time with TFRG_LIB set to that file; `--tag` names
the library in the output. The two processes are to be run alternately in one job.

usage (GPU box): wordpiece_speed.py [--runs 7] [--steps 20] [--records 65536] [--docs 4096] [--tag G8] [--out FILE]
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "tfrecords-reader_amd"), str(REPO)]

from token_ids_speed import BUCKETS, WORDS, workload  # noqa: E402
from tfr_reader import dense as D  # noqa: E402
from tfr_reader import hip  # noqa: E402
from tfr_reader import ids as I  # noqa: E402, N812
from tfr_reader import ragged as R  # noqa: E402
from tfr_reader import tokens as T  # noqa: E402, N812
from tfr_reader import wordpiece as W  # noqa: E402, N812

WHOLE, TILE = 98_000, 64
HEX = b"0123456789abcdef"


def measure(say, dev, stream, title: str, records: int, lo: int, hi: int, runs: int, steps: int, vocab, wpv) -> None:
    dec = hip.HipDecoder(0)
    res = dec.decode(*workload(records, lo, hi, False, 1))
    assert int(res.status.max()) == 0
    dec.set_ragged_tile(TILE)
    s_t = D.resolve_slot(dec, R.RaggedElements("t"))
    m = records
    rows = torch.from_numpy(np.random.default_rng(2).integers(0, records, m)).to(dev)
    rw = D.rows_arg(rows)
    h = stream.cuda_stream
    plain, special = W.WordPieceIds("t", wpv), W.WordPieceIds("t", wpv, special=True, max_pieces=128)
    sized = dec.wordpiece_ids([plain], rows=rows)  # exact sizes, once
    n_wp, unk = sized.totals["t"], int(sized.stats["t"][1])
    n_sp = dec.wordpiece_ids([special], rows=rows).totals["t"]
    n_tok = dec.token_ids([T.TokenIds("t", num_oov_buckets=BUCKETS)], rows=rows).totals["t"]
    n_el, n_by = dec.ragged_elements([R.RaggedElements("t")], rows=rows).totals["t"]
    ids = torch.empty(max(n_wp, n_sp, n_tok), dtype=torch.int64, device=dev)
    ro = torch.empty(m + 1, dtype=torch.int64, device=dev)
    values = torch.empty(n_by, dtype=torch.uint8, device=dev)
    eo = torch.empty(n_el + 1, dtype=torch.int64, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    stats = torch.empty(4, dtype=torch.int32, device=dev)

    def wp(sp, cap: int):
        def step() -> None:
            W.launch_wordpiece(dec, [(s_t, sp, cap, ids.data_ptr(), ro.data_ptr())], rw, m, 0, totals.data_ptr(), stats.data_ptr(), h)
        return step

    def tok_step() -> None:
        T.launch_tokens(dec, [(s_t, 0, 0, 0, (0, 0), vocab._handle().value, BUCKETS, WORDS, -1, n_tok, ids.data_ptr(), ro.data_ptr())],
                        rw, m, 0, totals.data_ptr(), stats.data_ptr(), h)

    def elems_step() -> None:
        R.launch_elems(dec, [(s_t, 0, 0, n_el, n_by, values.data_ptr(), eo.data_ptr(), ro.data_ptr())], rw, m, 0,
                       totals.data_ptr(), stats.data_ptr(), h)

    variants = {"wp": wp(plain, n_wp), "wp-special": wp(special, n_sp), "tok-vocab": tok_step, "elems": elems_step}
    for f in variants.values():  # warm-up
        for _ in range(3):
            f()
    torch.cuda.synchronize(dev)
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
    say(f"{title}: {records} records of {lo}..{hi} bytes, m = {m} rows, {n_tok} words in B = {n_by} bytes, T = {n_wp} pieces "
        f"({n_sp} with cls / sep and max_pieces 128), {unk} words unk; {runs} interleaved runs of {steps} calls, ms per call "
        f"between two device events, {TILE} rows a tile")
    med = {}
    for name, v in ms.items():
        med[name] = statistics.median(v)
        say(f"  {name:11s} median {med[name]:.4f} (min {min(v):.4f}, max {max(v):.4f})  runs: " + " ".join(f"{x:.4f}" for x in v))
    for y in ("tok-vocab", "elems"):
        say(f"  ratio to {y}: " + ", ".join(f"{k} {med[k] / med[y]:.2f}" for k in med if k.startswith("wp")))
    dec.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--tag", default="G8")
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
    digits = [bytes([c]) for c in HEX]
    wpv = W.WordPieceVocab([b"[UNK]", b"[CLS]", b"[SEP]", *digits, *(b"##" + d for d in digits), *(b"%05x" % i for i in range(WHOLE))],
                           device=0)
    say(f"tools/wordpiece_speed.py [{a.tag}] on {torch.cuda.get_device_name(dev)}; {WHOLE} whole words, 16 + 16 one-byte pieces")
    measure(say, dev, stream, "sentences", a.records, 30, 300, a.runs, a.steps, vocab, wpv)
    measure(say, dev, stream, "documents", a.docs, 4096, 4096, a.runs, a.steps, vocab, wpv)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with Path(a.out).open("a") as f:
            f.write("\n".join(lines) + "\n")
    vocab.close()
    wpv.close()


if __name__ == "__main__":
    main()
