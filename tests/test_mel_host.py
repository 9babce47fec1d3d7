"""Log-mel spectrograms without a GPU: the float64 reference and the derived bound that the GPU tests share,
``BatchResult.mel`` (the numpy host path, over a host decode) against that reference, ``mel_filters`` against
closed forms, and the validation of ``Mel`` / ``MelBank``."""

import numpy as np
import pytest

from tests import _columns
from tests.test_resize_host import as_float
from tfr_reader import mel as M
from tfr_reader import synth, writer

U = 2.0 ** -23
LN = {"ln": 1.0, "log10": np.log(10.0)}


def ref_mel(s, bank, frames, hop, center=True, power=2, log="log10", floor=1e-10, scale=1.0, bias=0.0):
    """The definition in float64 from explicit frames of the fixed-length signal ``s``: a dict of the windowed
    frames F ``[frames, n_fft]``, X, P, and mel / v / out ``[n_mels, frames]``."""
    n_fft = bank.n_fft
    y = np.pad(np.asarray(s, np.float64), n_fft // 2, mode="reflect") if center else np.asarray(s, np.float64)
    F = np.stack([y[t * hop : t * hop + n_fft] for t in range(frames)]) * bank.window.astype(np.float64)
    X = np.fft.rfft(F, axis=1)
    P = np.abs(X) ** power
    mel = bank.filters.astype(np.float64) @ P.T
    v = mel if log is None else np.log(np.maximum(mel, floor)) / LN[log]
    return dict(F=F, X=X, P=P, mel=mel, v=v, out=v * scale + bias)


def tol_mel(r, bank, power, log, floor, scale, out_type):
    """The worst-case bound of a float32 evaluation in any summation order: dX from the n_fft-term sums
    of a frame, propagated through the power, the filterbank and the log, plus the output type's half-ulp."""
    n_fft, fb = bank.n_fft, np.abs(bank.filters.astype(np.float64))
    dX = U * (n_fft + 16) * np.abs(r["F"]).sum(axis=1, keepdims=True)
    dP = (2 * np.sqrt(2) * np.abs(r["X"]) * dX + 2 * dX ** 2 if power == 2 else np.sqrt(2) * dX) + 4 * U * r["P"]
    dmel = fb @ dP.T + U * (bank.n_bins + 8) * r["mel"]
    if log is None:
        tol = abs(scale) * dmel + 4 * U * np.abs(r["out"])
    else:
        tol = abs(scale) * dmel / np.maximum(r["mel"] - dmel, floor) / LN[log] + 4 * U * np.maximum(1, np.abs(r["v"])) * abs(scale)
    return tol + {"float32": 0.0, "float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}[out_type] * np.abs(r["out"]) + (out_type == "float16") * 2.0 ** -25


def f32_mel(s, bank, frames, hop, center=True, power=2, log="log10", floor=1e-10, scale=1.0, bias=0.0):
    """The same formula in float32 numpy, both sums accumulated four terms at a time: the yardstick of the
    GPU tests' RMS condition (its own error against ``ref_mel``); never compared with the kernel."""
    n_fft, f4 = bank.n_fft, np.float32
    y = np.pad(np.asarray(s, np.float64), n_fft // 2, mode="reflect") if center else np.asarray(s, np.float64)
    F = np.stack([y[t * hop : t * hop + n_fft] for t in range(frames)]).astype(f4)
    ang = 2 * np.pi * ((np.arange(n_fft)[:, None] * np.arange(bank.n_bins)[None, :]) % n_fft) / n_fft
    w = bank.window.astype(np.float64)[:, None]
    wc, ws = (w * np.cos(ang)).astype(f4), (w * np.sin(ang)).astype(f4)
    re, im = np.zeros((frames, bank.n_bins), f4), np.zeros((frames, bank.n_bins), f4)
    for k in range(0, n_fft, 4):
        re += F[:, k : k + 4] @ wc[k : k + 4]
        im += F[:, k : k + 4] @ ws[k : k + 4]
    P = re * re + im * im
    P = np.sqrt(P) if power == 1 else P
    mel = np.zeros((bank.n_mels, frames), f4)
    for b in range(0, bank.n_bins, 4):
        mel += bank.filters[:, b : b + 4] @ P.T[b : b + 4]
    v = mel if log is None else (np.log if log == "ln" else np.log10)(np.maximum(mel, f4(floor)))
    return (v * f4(scale) + f4(bias)).astype(f4)


def noise(n, seed=0):
    """int16-range noise with a quiet first third."""
    x = np.random.default_rng(seed).integers(-32768, 32768, n).astype(np.float64)
    x[: n // 3] = np.round(x[: n // 3] / 4096)
    return x.astype(np.int16)


def bank_of(n_fft, n_mels, sr=16000, **kw):
    return M.MelBank(n_fft, M.hann(n_fft), M.mel_filters(sr, n_fft, n_mels, norm="slaney", **kw))


@pytest.mark.parametrize("n_fft,hop,n_mels,frames", [(400, 160, 80, 40), (64, 16, 20, 33), (30, 7, 5, 33), (1024, 256, 128, 9)])
def test_the_float32_formula_is_far_inside_the_bound(n_fft, hop, n_mels, frames):
    bank = bank_of(n_fft, n_mels)
    s = noise((frames - 1) * hop + n_fft // 2 + 3, seed=n_fft).astype(np.float64)
    r = ref_mel(s, bank, frames, hop)
    used = np.abs(f32_mel(s, bank, frames, hop) - r["out"]) / tol_mel(r, bank, 2, "log10", 1e-10, 1.0, "float32")
    assert used.max() < 0.05, used.max()


@pytest.mark.parametrize("src,out,kw", [
    ("int16", "float32", dict(center=True, power=2, log="log10")), ("float32", "float16", dict(center=False, power=1, log="ln")),
    ("uint8", "bfloat16", dict(center=True, power=2, log=None, scale=2.0 ** -12)), ("bfloat16", "float32", dict(center=True, power=1, log=None))])
def test_batch_mel_against_the_reference(src, out, kw):
    from tfr_reader import raw as W

    bank, samples, frames, hop = bank_of(64, 20), 200, 9, 16
    x = noise(2 * 230, seed=7).reshape(230, 2)
    sigs = [x, x[:150], x[:0], x[:200]]
    if src == "bfloat16":
        enc = [(a.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16) for a in sigs]  # (the low bits dropped)
        vals = [(e.astype(np.uint32) << 16).view(np.float32).astype(np.float64) for e in enc]
    else:
        enc = [(a % 256 if src == "uint8" else a).astype(W.SRC[src][1]) for a in sigs]
        vals = [e.astype(np.float64) for e in enc]
    elems = [[e.tobytes()] for e in enc]
    elems[3] = [elems[3][0] + b"x", b"more"]  # (a partial trailing sample, and a second element)
    payloads = [writer.encode_example([("pcm", "bytes_list", e)]) for e in elems] + [writer.encode_example([("n", "int64_list", [1])])]
    res = _columns.batch_from_oracle(*synth.framed(payloads))
    sp = M.Mel("pcm", bank, samples, frames, hop, src=src, out=out, channels=2, channel=1, fill=3, lengths=True, bias=0.5, **kw)
    got = res.mel([sp], rows=[4, 0, 1, 2, 3])
    assert got["pcm"].shape == (5, 20, 9) and (as_float(got["pcm"][0], out) == 3).all()
    for k, v in enumerate(vals):
        s = np.zeros(samples)
        s[: min(len(v), samples)] = v[:samples, 1]
        r = ref_mel(s, bank, frames, hop, bias=0.5, **kw)
        half = {"float32": 2.0 ** -24, "float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}[out]
        assert (np.abs(as_float(got["pcm"][k + 1], out) - r["out"]) <= half * np.abs(r["out"]) * 1.01 + 1e-30).all()
    esz = W.ITEMSIZE[src]
    assert got.lengths["pcm"].tolist() == [0, 460 * esz, 300 * esz, 0, 400 * esz + 1] and got.stats["pcm"].tolist() == [2, 3, 1, 1]


def test_mel_filters_closed_forms():
    sr, n_fft, n = 16000, 512, 40
    for scale, inv in (("htk", lambda m: 700 * (10 ** (m / 2595) - 1)), ("slaney", None)):
        fb = M.mel_filters(sr, n_fft, n, fmin=20.0, fmax=7600.0, scale=scale)
        m0, m1 = (float(M.hz_to_mel(f, scale)) for f in (20.0, 7600.0))
        centres = [m0 + (m1 - m0) * (j + 1) / (n + 1) for j in range(n)]
        if scale == "htk":
            hz = np.array([inv(m) for m in centres])
        else:  # (linear below 15 mel = 1 kHz, a factor 6.4 per 27 mel above)
            hz = np.array([m * 200 / 3 if m < 15 else 1000 * 6.4 ** ((m - 15) / 27) for m in centres])
        f = np.arange(n_fft // 2 + 1) * sr / n_fft
        # a triangle's peak is its centre: the bins next to it bracket the closed-form frequency
        for j in range(n):
            b = int(np.argmax(fb[j]))
            assert abs(f[b] - hz[j]) <= sr / n_fft and (fb[j] >= 0).all() and fb[j].max() <= 1
    assert abs(float(M.hz_to_mel(1000.0, "htk")) - 2595 * np.log10(1 + 1000 / 700)) < 1e-9
    # Slaney-normalised rows integrate to 2 / bandwidth * bandwidth / 2 = 1 over frequency (fine bins: the sum is the integral)
    fine = M.mel_filters(sr, 1 << 11, 10, norm="slaney")  # (n_fft here only spaces the bins)
    assert np.allclose(fine.sum(axis=1) * sr / (1 << 11), 1.0, rtol=2e-2)
    pts = M.mel_to_hz(np.linspace(M.hz_to_mel(0.0), M.hz_to_mel(sr / 2), 12))
    plain = M.mel_filters(sr, 1 << 11, 10)
    assert np.allclose(fine, plain * (2 / (pts[2:] - pts[:-2]))[:, None])


@pytest.mark.parametrize("kw", [
    dict(src="int4"), dict(out="same"), dict(samples=0), dict(samples=(1 << 24) + 1), dict(frames=0), dict(hop=0), dict(hop=65),
    dict(channels=17), dict(channels=2, channel=2), dict(samples=32), dict(frames=14), dict(center=False, frames=10),
    dict(power=3), dict(log="log2"), dict(floor=0.0), dict(floor=-1.0), dict(scale=float("inf")), dict(bias=float("nan")),
    dict(key=7), dict(bank=None)])
def test_mel_validation(kw):
    base = dict(key="pcm", bank=bank_of(64, 8), samples=200, frames=13, hop=16)
    M.Mel(**base)
    with pytest.raises((ValueError, TypeError)):
        M.Mel(**{**base, **kw})


@pytest.mark.parametrize("args", [(63, 63, (4, 32)), (0, 0, (4, 1)), (4096, 4096, (4, 2049)), (64, 63, (4, 33)), (64, 64, (4, 32)),
                                  (64, 64, (0, 33)), (64, 64, (129, 33))])
def test_mel_bank_validation(args):
    n_fft, nw, fshape = args
    with pytest.raises(ValueError):
        M.MelBank(n_fft, np.ones(nw), np.ones(fshape))
