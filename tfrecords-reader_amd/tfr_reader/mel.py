"""Log-mel spectrograms from PCM bytes features: the ``tf.signal.stft`` + ``linear_to_mel_weight_matrix`` +
``log`` block of an audio input pipeline (``torch.stft`` + a matmul + a log), for a list of rows of a decoded
batch.

A ``MelBank`` owns the device tables of one transform (``tfrg_mel``: n_fft, the window, the filterbank); a
``Mel`` spec names a ``bytes_list`` key whose first element is a PCM signal, the bank, the fixed signal
length, the framing and what becomes of the mel energies. Then

* ``HipDecoder.mel`` / ``ShardDecoder.mel`` write ``[m, n_mels, frames]`` torch tensors on the device
  (``tfrg_result_mel``: k_mel, two matrix products on the MFMA units per tile of frames; nothing but the
  PCM is read and nothing but the output written), through the driver of ``tfr_reader.raw``;
* ``BatchResult.mel`` evaluates the definition (include/tfrg.h) in numpy float64 with ``np.fft.rfft``, rounded
  once to the output type (the host path; it does not mimic the kernel's summation order).

``hann`` and ``mel_filters`` build the usual window and filterbanks; any float32 arrays will do.
"""

from __future__ import annotations

import ctypes as C
from collections.abc import Sequence
from dataclasses import dataclass

import numpy as np

from tfr_reader import _native as N
from tfr_reader import dense as D
from tfr_reader import raw as W

LOG = {None: N.MEL_LINEAR, "ln": N.MEL_LN, "log10": N.MEL_LOG10}


def tile_frames(n_fft: int, hop: int) -> int:
    """The frames of one work item of k_mel for this n_fft and hop (csrc/tfrg_mel.h: 64, 32 or 16)."""
    return int(N.lib().tfrg_mel_tile_frames(int(n_fft), int(hop)))


def hann(n_fft: int, periodic: bool = True) -> np.ndarray:
    """The Hann window as float64 (``torch.hann_window``; ``periodic=False``: ``np.hanning``)."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / (n_fft if periodic else max(n_fft - 1, 1)))


def hz_to_mel(f, scale: str = "slaney"):
    f = np.asarray(f, np.float64)
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    # (Slaney's Auditory Toolbox: linear below 1 kHz, 27 steps per factor of 6.4 above)
    return np.where(f < 1000.0, f * 3.0 / 200.0, 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) * 27.0 / np.log(6.4))


def mel_to_hz(m, scale: str = "slaney"):
    m = np.asarray(m, np.float64)
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m < 15.0, m * 200.0 / 3.0, 1000.0 * np.exp((np.maximum(m, 15.0) - 15.0) * np.log(6.4) / 27.0))


def mel_filters(sr: float, n_fft: int, n_mels: int, fmin: float = 0.0, fmax: float | None = None, scale: str = "slaney",
                norm: str | None = None) -> np.ndarray:
    """``[n_mels, n_fft // 2 + 1]`` float64 triangular filters whose corners are equally spaced on the mel
    ``scale`` ("slaney" or "htk") between ``fmin`` and ``fmax`` (default ``sr / 2``); ``norm="slaney"``
    divides each by half its bandwidth in Hz (librosa's and Whisper's bank: scale and norm "slaney")."""
    if scale not in ("slaney", "htk"):
        raise ValueError(f"scale must be 'slaney' or 'htk', not {scale!r}")
    if norm not in (None, "slaney"):
        raise ValueError(f"norm must be None or 'slaney', not {norm!r}")
    fmax = sr / 2.0 if fmax is None else fmax
    if not 0 <= fmin < fmax:
        raise ValueError(f"0 <= fmin < fmax is needed, not {fmin} and {fmax}")
    pts = mel_to_hz(np.linspace(hz_to_mel(fmin, scale), hz_to_mel(fmax, scale), n_mels + 2), scale)
    f = np.arange(n_fft // 2 + 1) * (sr / n_fft)
    lo, c, hi = pts[:-2, None], pts[1:-1, None], pts[2:, None]
    fb = np.maximum(0.0, np.minimum((f - lo) / (c - lo), (hi - f) / (hi - c)))
    return fb * (2.0 / (hi - lo)) if norm == "slaney" else fb


class MelBank:
    """The tables of one transform: ``n_fft`` (even), ``window`` ``[n_fft]`` and ``filters`` ``[n_mels, n_fft //
    2 + 1]``, rounded to float32. Owns a ``tfrg_mel`` per device it has been used on (``handle(device)``
    makes it on first use; the host path needs none). Keep the object until the device work that uses it
    has been queued: ``close`` (or collection) synchronises those devices."""

    def __init__(self, n_fft: int, window, filters) -> None:
        if isinstance(n_fft, bool) or not isinstance(n_fft, (int, np.integer)) or not 2 <= n_fft <= N.MEL_MAX_FFT or n_fft % 2:
            raise ValueError(f"n_fft must be even and in 2..{N.MEL_MAX_FFT}, not {n_fft!r}")
        self.n_fft, self.n_bins = int(n_fft), int(n_fft) // 2 + 1
        self.window = np.ascontiguousarray(window, np.float32)
        self.filters = np.ascontiguousarray(filters, np.float32)
        if self.window.shape != (self.n_fft,):
            raise ValueError(f"window must hold {self.n_fft} values, not shape {self.window.shape}")
        if self.filters.ndim != 2 or self.filters.shape[1] != self.n_bins or not 1 <= self.filters.shape[0] <= N.MEL_MAX_MELS:
            raise ValueError(f"filters must be [1..{N.MEL_MAX_MELS}, {self.n_bins}], not shape {self.filters.shape}")
        if not (np.isfinite(self.window).all() and np.isfinite(self.filters).all()):
            raise ValueError("window and filters must be finite")
        self.n_mels = int(self.filters.shape[0])
        self._handles: dict[int, C.c_void_p] = {}

    def handle(self, device: int) -> C.c_void_p:
        """The ``tfrg_mel`` on GPU ``device`` (``tfrg_mel_create`` on first use)."""
        if device not in self._handles:
            p = C.c_void_p()
            N.check(N.lib().tfrg_mel_create(int(device), self.n_fft, N.ptr(self.window), self.n_mels, N.ptr(self.filters),
                                            C.byref(p)), "tfrg_mel_create")
            self._handles[device] = p
        return self._handles[device]

    def info(self, device: int) -> dict[str, int]:
        a, b, c, d = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        N.check(N.lib().tfrg_mel_info(self.handle(device), C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "tfrg_mel_info")
        return {"n_fft": a.value, "n_mels": b.value, "n_bins": c.value, "device_bytes": d.value}

    def close(self) -> None:
        for dev in list(getattr(self, "_handles", {})):
            N.check(N.lib().tfrg_mel_destroy(self._handles.pop(dev)), "tfrg_mel_destroy")

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:  # noqa: BLE001 (interpreter shutdown)
            pass


@dataclass(frozen=True, eq=False)
class Mel:
    """One spectrogram output: element 0 of ``key``'s ``bytes_list`` is a little-endian signal of ``src``
    elements, sample n being element ``n * channels + channel``. It is cut or zero-padded to ``samples``,
    cut into ``frames`` frames ``hop`` apart (``center``: frame t is centred on sample ``t * hop`` of the
    signal reflected at both ends, as ``torch.stft``), windowed and transformed by ``bank``, ``|X| ** power``
    (1 or 2), filtered, ``log`` ("log10", "ln" or None; the energy is first raised to ``floor``), times
    ``scale`` plus ``bias``, rounded once to ``out`` ("float32", "float16", "bfloat16"). The result is
    ``[m, n_mels, frames]``. A record without the element gives a row of ``fill``, untransformed.
    ``lengths``: also return the byte lengths. ``name``: the output's name in the result (default: the key)."""

    key: str
    bank: MelBank
    samples: int
    frames: int
    hop: int
    center: bool = True
    power: int = 2
    log: str | None = "log10"
    floor: float = 1e-10
    scale: float = 1.0
    bias: float = 0.0
    src: str = "int16"
    out: str = "float32"
    channels: int = 1
    channel: int = 0
    fill: float | int = 0
    lengths: bool = False
    name: str | None = None

    dtype = "uint8"  # (the slot kind, as ``Dense.dtype`` selects it)

    def __post_init__(self) -> None:
        who = f"Mel({self.key!r})"
        if not isinstance(self.key, str):
            raise TypeError(f"Mel key must be a str, not {type(self.key).__name__}")
        if not isinstance(self.bank, MelBank):
            raise TypeError(f"{who}: bank must be a MelBank, not {type(self.bank).__name__}")
        if self.src not in W.SRC:
            raise ValueError(f"{who}: src must be one of {sorted(W.SRC)}, not {self.src!r}")
        if self.out not in ("float32", "float16", "bfloat16"):
            raise ValueError(f"{who}: out must be 'float32', 'float16' or 'bfloat16', not {self.out!r}")
        lim = {"samples": N.MEL_MAX_SAMPLES, "frames": N.MEL_MAX_FRAMES, "hop": self.bank.n_fft, "channels": N.RAW_MAX_CHANNELS}
        for what, hi in lim.items():
            v = getattr(self, what)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= hi:
                raise ValueError(f"{who}: {what} must be in 1..{hi}, not {v!r}")
            object.__setattr__(self, what, int(v))
        if isinstance(self.channel, bool) or not isinstance(self.channel, (int, np.integer)) or not 0 <= self.channel < self.channels:
            raise ValueError(f"{who}: channel must be in 0..{self.channels - 1}, not {self.channel!r}")
        object.__setattr__(self, "center", bool(self.center))
        n_fft, last = self.bank.n_fft, (self.frames - 1) * self.hop
        if self.center and (self.samples <= n_fft // 2 or last > self.samples):
            raise ValueError(f"{who}: center needs samples > n_fft / 2 and (frames - 1) * hop <= samples")
        if not self.center and last + n_fft > self.samples:
            raise ValueError(f"{who}: the last frame ends at {last + n_fft}, past samples = {self.samples}")
        if self.power not in (1, 2):
            raise ValueError(f"{who}: power must be 1 or 2, not {self.power!r}")
        if self.log not in LOG:
            raise ValueError(f"{who}: log must be 'log10', 'ln' or None, not {self.log!r}")
        for what in ("floor", "scale", "bias"):
            v = np.float32(getattr(self, what))
            if not np.isfinite(v):
                raise ValueError(f"{who}: {what} must be finite")
            object.__setattr__(self, what, float(v))
        if self.log is not None and not self.floor > 0:
            raise ValueError(f"{who}: a log needs floor > 0 (as float32), not {self.floor!r}")
        self.fill_bits  # noqa: B018 (validates the fill)

    @property
    def out_name(self) -> str:
        return self.name if self.name is not None else self.key

    @property
    def out_type(self) -> str:
        return self.out

    @property
    def out_shape(self) -> tuple:
        return (self.bank.n_mels, self.frames)

    @property
    def fill_bits(self) -> int:
        return W.fill_bits_of(f"Mel({self.key!r})", self.out, self.fill)


def check_specs(specs: Sequence[Mel]) -> list[Mel]:
    specs = list(specs)
    if not 1 <= len(specs) <= N.RAW_MAX_SPECS:
        raise ValueError(f"between 1 and {N.RAW_MAX_SPECS} Mel specs per call, not {len(specs)}")
    seen = set()
    for s in specs:
        if not isinstance(s, Mel):
            raise TypeError(f"specs must be Mel objects, not {type(s).__name__}")
        if s.out_name in seen:
            raise ValueError(f"two Mel specs are named {s.out_name!r}: give one of them name=")
        seen.add(s.out_name)
    return specs


# ---------------------------------------------------------------------- host path (numpy)
def signal(sp: Mel, elem: np.ndarray) -> np.ndarray:
    """The fixed-length float64 signal of an element's bytes (uint8)."""
    esz = W.ITEMSIZE[sp.src]
    k = min(elem.size // esz // sp.channels, sp.samples)
    b = np.ascontiguousarray(elem[: k * sp.channels * esz])
    if sp.src == "bfloat16":
        v = (b.view(np.uint16).astype(np.uint32) << 16).view(np.float32)
    else:
        v = b.view(np.dtype(W.SRC[sp.src][1]).newbyteorder("<"))
    s = np.zeros(sp.samples, np.float64)
    s[:k] = v.reshape(k, sp.channels)[:, sp.channel]
    return s


def spectrogram(sp: Mel, s: np.ndarray) -> np.ndarray:
    """The output bits ``[n_mels, frames]`` of the signal ``s``, by the definition, in float64."""
    n_fft = sp.bank.n_fft
    y = np.pad(s, n_fft // 2, mode="reflect") if sp.center else s
    idx = np.arange(sp.frames)[:, None] * sp.hop + np.arange(n_fft)[None, :]
    X = np.fft.rfft(y[idx] * sp.bank.window.astype(np.float64), axis=1)
    P = np.abs(X) ** sp.power
    mel = sp.bank.filters.astype(np.float64) @ P.T
    with np.errstate(all="ignore"):
        if sp.log is not None:
            mel = (np.log if sp.log == "ln" else np.log10)(np.maximum(mel, sp.floor))
        v = (mel * sp.scale + sp.bias).astype(np.float32)
        if sp.out == "float32":
            return v.view(np.uint32)
        return v.astype(np.float16).view(np.uint16) if sp.out == "float16" else W.bf16_bits(v).reshape(v.shape)


def batch_mel(res, specs: Sequence[Mel], rows=None) -> D.DenseBatch:
    """``BatchResult.mel``: the outputs of ``specs`` from a fetched result's columns, record by record. A key
    without a slot gives all-``fill`` outputs. bfloat16 outputs are returned as their uint16 bits."""
    specs = check_specs(specs)
    n = len(res)
    picked = list(range(n)) if rows is None else D.host_rows(rows, n).tolist()
    m = len(picked)
    values, lengths, stats = {}, {}, {}
    for sp in specs:
        ubits, dt = W._np_out(sp)
        width = sp.samples * sp.channels * W.ITEMSIZE[sp.src]
        out = np.full((m, *sp.out_shape), sp.fill_bits, ubits)
        lens, st = np.zeros(m, np.int32), np.zeros(4, np.uint32)
        s = D.find_slot(res.slot_key, res.slot_kind, sp.key, 1)
        if s is None:
            st[1] = st[2] = m
        else:
            base, rs = int(res.slot_base[s]), np.asarray(res.row_splits[s]).astype(np.int64)
            for k, g in enumerate(picked):
                c, elem = W.element0(res, base, rs, g)
                ln = int(elem.size)
                if c:
                    out[k] = spectrogram(sp, signal(sp, elem))
                lens[k] = ln
                st += np.array([ln > width, ln < width, c == 0, c > 1], np.uint32)
        values[sp.out_name] = out.view(dt)
        if sp.lengths:
            lengths[sp.out_name] = lens
        stats[sp.out_name] = st
    return D.DenseBatch(values, lengths, stats)


# ---------------------------------------------------------------------- device path
def launch(dec, items: Sequence[tuple], rows: tuple | None, m: int, row0: int, stats_ptr: int | None,
           skipped_ptr: int | None, consumer: int | None) -> None:
    """One ``tfrg_result_mel`` call: items are (spec, slot, out pointer, lengths pointer or None); ``rows``:
    (device pointer, TFRG_ROWS_* id) or None."""
    arr = (N.TfrgMelSpec * len(items))()
    for a, (sp, slot, out, lens) in zip(arr, items):
        a.slot, a.src, a.out, a.channels, a.channel = slot, W.SRC[sp.src][0], W.OUT[sp.out], sp.channels, int(sp.channel)
        a.samples, a.frames, a.hop, a.center, a.power, a.log = sp.samples, sp.frames, sp.hop, int(sp.center), int(sp.power), LOG[sp.log]
        a.fill, a.floor, a.scale, a.bias, a.reserved = sp.fill_bits, sp.floor, sp.scale, sp.bias, 0
        a.mel, a.out_ptr, a.lengths = sp.bank.handle(dec.device), out, lens
    ptr, rdt = rows if rows is not None else (None, 0)
    N.check(dec._lib.tfrg_result_mel(dec._ctx, arr, len(items), D.vp(ptr), rdt, m, row0, D.vp(stats_ptr), D.vp(skipped_ptr),
                                     D.vp(consumer)), "tfrg_result_mel")


# (a batch without the key: its rows are padded and empty, as Raw's)
MEL_KIND = W._Kind(check_specs, lambda sp: sp.lengths, "lengths", (), D.resolve_slot, launch, lambda dec, sp: (1, 2))


def _strict(b: D.DenseBatch, specs: Sequence[Mel]) -> D.DenseBatch:
    for s in specs:
        t, p, _, mu = (int(x) for x in b.stats[s.out_name])
        if t or p or mu:
            raise ValueError(f"Mel({s.key!r}, {s.src!r}, samples={s.samples}): {t} rows truncated, {p} padded, "
                             f"{mu} with more than one element")
    if b.skipped:
        raise IndexError(f"{b.skipped} rows of the list are outside the decoded records")
    return b


def decoder_mel(dec, specs: Sequence[Mel], *, rows=None, out=None, stream: int | None = None, strict: bool = False) -> D.DenseBatch:
    """``HipDecoder.mel``: the spectrograms of the decoder's last decode as torch tensors on its device: name
    -> ``[m, n_mels, frames]``, with ``.lengths``, ``.stats`` and ``.skipped``. ``rows``, ``out`` (name -> a
    tensor, or ``(tensor, lengths tensor)``), ``stream`` and ``strict`` as ``tfr_reader.raw.decoder_raw``'s."""
    n = D.last_n(dec)
    b = W._run([(dec, 0, n)], n, dec.device, specs, rows, out, stream, strict, MEL_KIND)
    return _strict(b, specs) if strict else b


def shard_mel(sd, plan: np.ndarray, specs: Sequence[Mel], *, rows=None, out=None, stream: int | None = None,
              strict: bool = False) -> D.DenseBatch:
    """``ShardDecoder.mel``: as ``tfr_reader.raw.shard_raw``, every batch's context taking the row list."""
    n = int(plan[-1, 1]) if len(plan) else 0
    b = W._run([(sd.decs[k], r0, r1) for k, (r0, r1, _, _) in enumerate(plan.tolist())], n, sd.device, specs, rows, out,
               stream, strict, MEL_KIND)
    return _strict(b, specs) if strict else b
