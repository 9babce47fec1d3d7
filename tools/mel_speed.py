"""Paired timings of HipDecoder.mel against the torch composition on the same device tensors, for Whisper's
front end: 16 clips of 480,000 int16 samples, n_fft 400, hop 160, 3000 frames, 80 mels, log10.

The two run interleaved, round after round, each timed with device events after a warm-up that is not
counted; the medians, the quartiles and the extremes are printed, then the kernel's share of the float32
matrix peak from its useful FLOP count (2 n_fft 2 n_bins + 2 n_bins n_mels per frame).

    python tools/mel_speed.py [--rows 16] [--rounds 30] [--peak-tflops 157.3]
"""

import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "tfrecords-reader_amd"), str(ROOT)]


def main() -> None:
    import torch

    from tfr_reader import hip, synth, writer
    from tfr_reader import mel as M

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--peak-tflops", type=float, default=157.3, help="the device's float32 matrix peak")
    a = ap.parse_args()
    n_fft, hop, samples, frames, n_mels = 400, 160, 480000, 3000, 80
    rng = np.random.default_rng(0)
    pcm = rng.integers(-32768, 32768, (a.rows, samples)).astype(np.int16)
    dec = hip.HipDecoder(0)
    dec.decode(*synth.framed([writer.encode_example([("pcm", "bytes_list", [x.tobytes()])]) for x in pcm]))
    window, fb = M.hann(n_fft), M.mel_filters(16000, n_fft, n_mels, norm="slaney")
    bank = M.MelBank(n_fft, window, fb)
    sp = M.Mel("pcm", bank, samples, frames, hop)
    dev = torch.device("cuda", 0)
    out = torch.empty((a.rows, n_mels, frames), dtype=torch.float32, device=dev)
    d_pcm = torch.from_numpy(pcm).to(dev)
    d_win, d_fb = torch.from_numpy(window.astype(np.float32)).to(dev), torch.from_numpy(fb.astype(np.float32)).to(dev)

    def ours():
        dec.mel([sp], out={"pcm": out})

    def composed():
        X = torch.stft(d_pcm.float(), n_fft, hop, window=d_win, center=True, pad_mode="reflect", return_complex=True)[..., :frames]
        return torch.log10(torch.clamp(d_fb @ (X.abs() ** 2), min=1e-10))

    def timed(fn) -> float:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(5):
        ours()
        ref = composed()
    torch.cuda.synchronize()
    print(f"largest difference from the composition: {(out - ref).abs().max().item():.3e}")
    t = {"mel": [], "torch": []}
    for _ in range(a.rounds):
        t["mel"].append(timed(ours))
        t["torch"].append(timed(composed))
    for k, v in t.items():
        q = np.percentile(v, [0, 25, 50, 75, 100])
        print(f"{k:6s} ms: median {q[2]:.3f}  quartiles {q[1]:.3f} .. {q[3]:.3f}  range {q[0]:.3f} .. {q[4]:.3f}  ({a.rounds} rounds)")
    med = float(np.median(t["mel"]))
    flop = a.rows * frames * (2.0 * n_fft * 2 * (n_fft // 2 + 1) + 2.0 * (n_fft // 2 + 1) * n_mels)
    print(f"ratio torch / mel (medians): {np.median(t['torch']) / med:.2f}")
    print(f"mel: {flop / 1e9:.2f} GFLOP useful, {flop / med / 1e9:.1f} TFLOP/s, {100 * flop / med / 1e9 / a.peak_tflops:.1f} % of {a.peak_tflops} TFLOP/s")
    bank.close()
    dec.close()


if __name__ == "__main__":
    main()
