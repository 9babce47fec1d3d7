"""Log-mel spectrograms on the device (tfrg_result_mel: k_mel). Records hold PCM as raw bytes; the expectation
is ``ref_mel`` of tests/test_mel_host.py (float64, explicit frames), never ``tfr_reader.mel``'s host path. Every
value must lie within the derived worst-case bound ``tol_mel``, and the RMS error of a call within 8 times
the RMS error of the float32 numpy evaluation ``f32_mel`` against the same reference. Outputs lie inside
0xA5-poisoned buffers: guards, skipped rows and refused calls keep the poison."""

import ctypes as C

import numpy as np
import pytest

from tests.test_mel_host import bank_of, f32_mel, noise, ref_mel, tol_mel
from tests.test_resize_gpu import GUARD, POISON, POISON32, dec, dev, values, write  # noqa: F401 (dec: the fixture)
from tfr_reader import _native as N
from tfr_reader import shard
from tfr_reader import mel as M
from tfr_reader import raw as W

pytestmark = pytest.mark.gpu

BANKS = {}


def bank(n_fft, n_mels):
    if (n_fft, n_mels) not in BANKS:
        BANKS[n_fft, n_mels] = bank_of(n_fft, n_mels)
    return BANKS[n_fft, n_mels]


def feats(b, n=1):
    """The features of one record, the signal (key "image": ``write`` puts it at every 16-byte residue) last."""
    return [("image", "bytes_list", [b] * n)]


def run(call, sp, m, **kw):
    """One call over a poisoned output: (the batch, the output's bits [m, n_mels, frames], written lengths)."""
    import torch

    osz = W.ITEMSIZE[sp.out]
    nb = m * sp.bank.n_mels * sp.frames * osz
    big = torch.full((GUARD + nb + GUARD,), POISON, dtype=torch.uint8, device=dev())
    view = big[GUARD : GUARD + nb].view(W._torch_dtype(sp)).view(m, *sp.out_shape)
    lens = torch.full((m,), POISON32, dtype=torch.int32, device=dev())
    got = call([sp], out={sp.out_name: (view, lens) if sp.lengths else view},
               **{k: torch.from_numpy(np.asarray(v)).to(dev()) for k, v in kw.items()})
    host = big.cpu().numpy()
    assert (host[:GUARD] == POISON).all() and (host[GUARD + nb :] == POISON).all()
    return got, host[GUARD : GUARD + nb].view({2: np.uint16, 4: np.uint32}[osz]).reshape(m, *sp.out_shape), lens.cpu().numpy()


def fixed(sp, x):
    """The fixed-length float64 signal of the source samples ``x`` (already the selected channel's)."""
    s = np.zeros(sp.samples)
    k = min(len(x), sp.samples)
    s[:k] = np.asarray(x, np.float64)[:k]
    return s


def close(sp, sigs, bits, label=None):
    """Rows ``bits[k]`` against the reference of ``sigs[k]``: the bound per value, the RMS condition per call."""
    kw = dict(center=sp.center, power=sp.power, log=sp.log, floor=sp.floor, scale=sp.scale, bias=sp.bias)
    e_gpu, e_f32 = [], []
    for k, x in enumerate(sigs):
        s = fixed(sp, x)
        r = ref_mel(s, sp.bank, sp.frames, sp.hop, **kw)
        err = np.abs(values(bits[k], sp.out) - r["out"])
        worst = (err / tol_mel(r, sp.bank, sp.power, sp.log, sp.floor, sp.scale, sp.out)).max()
        assert worst <= 1, (k, worst)
        e_gpu.append(err)
        e_f32.append(f32_mel(s, sp.bank, sp.frames, sp.hop, **kw).astype(np.float64) - r["out"])
    if sp.out == "float32":  # (a 16-bit output's rounding is not the yardstick's)
        rms = [float(np.sqrt(np.mean(np.square(np.stack(e))))) for e in (e_gpu, e_f32)]
        print(f"error ratio {label or sp.out_name}: gpu {rms[0]:.3e} f32 {rms[1]:.3e} ratio {rms[0] / rms[1] if rms[1] else 0:.2f}")
        assert rms[0] <= 8 * rms[1], rms


SHAPES = [(30, 7, 5), (64, 16, 20), (400, 160, 80), (1024, 256, 128), (2048, 1024, 8)]  # (the last: a span beyond 64 KiB of LDS)


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("tiles", ["TF-1", "TF", "TF+1", "2TF+1"])
@pytest.mark.parametrize("n_fft,hop,n_mels", SHAPES)
def test_tile_seams(dec, n_fft, hop, n_mels, tiles, center):
    tf = M.tile_frames(n_fft, hop)
    assert tf in (16, 32, 64)
    frames = {"TF-1": tf - 1, "TF": tf, "TF+1": tf + 1, "2TF+1": 2 * tf + 1}[tiles]
    samples = (frames - 1) * hop + (3 if center else n_fft)
    xs = [noise(samples, seed=frames + i) for i in range(2)]
    dec.decode(*write([feats(x.tobytes()) for x in xs]))
    sp = M.Mel("image", bank(n_fft, n_mels), samples, frames, hop, center=center, scale=0.5, bias=1.0)
    _, bits, _ = run(dec.mel, sp, 2)
    close(sp, xs, bits, f"{n_fft}/{hop}/{n_mels} frames {frames} center {int(center)}")


def test_signal_edges(dec):
    n_fft, hop, samples, frames = 64, 16, 200, 13
    x = noise(samples + 5, seed=3)
    sine = np.round(32767 * np.sin(2 * np.pi * 5 * np.arange(samples) / n_fft)).astype(np.int16)
    elems = [x[:L].tobytes() for L in (0, 1, n_fft // 2, n_fft // 2 + 1, samples - 1, samples, samples + 5)]
    elems += [x[:77].tobytes() + b"\x7f", np.zeros(samples, np.int16).tobytes(), sine.tobytes()]
    dec.decode(*write([feats(b) for b in elems]))
    sp = M.Mel("image", bank(n_fft, 20), samples, frames, hop, scale=0.5, bias=1.0, lengths=True)
    got, bits, lens = run(dec.mel, sp, len(elems))
    sigs = [np.frombuffer(b[: len(b) // 2 * 2], np.int16) for b in elems]
    close(sp, sigs, bits)
    silent = np.float32(np.log10(np.float64(np.float32(1e-10))) * 0.5 + 1.0)
    assert (bits[0].view(np.float32) == silent).all() and (bits[8].view(np.float32) == silent).all()
    r = ref_mel(sine, sp.bank, frames, hop)["mel"][:, 4]
    assert int(np.argmax(bits[9].view(np.float32)[:, 4])) == int(np.argmax(r))  # (bin 5 = 1250 Hz lands in its filter)
    assert lens.tolist() == [len(b) for b in elems] and got.stats["image"].tolist() == [1, 6, 0, 0]


KINDS = [(2, "log10"), (1, "ln"), (2, None), (1, None)]


@pytest.mark.parametrize("out", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("i,src", enumerate(["int16", "float32", "uint8", "bfloat16"]))
def test_types_powers_logs_and_stereo(dec, i, src, out):
    power, log = KINDS[(i + ["float32", "float16", "bfloat16"].index(out)) % 4]
    n_fft, hop, samples, frames = 64, 16, 300, 19
    x = noise(2 * samples * 3, seed=i).reshape(3, samples, 2)
    if src == "bfloat16":
        enc = (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        val = (enc.astype(np.uint32) << 16).view(np.float32)
    else:
        enc = val = (x % 256 if src == "uint8" else x).astype(W.SRC[src][1])
    dec.decode(*write([feats(e.tobytes()) for e in enc]))
    # (linear outputs scaled into float16's range; bias within 2 |scale|: see the bound's last term)
    scale = 0.5 if log else 2.0 ** (-26 if power == 2 else -12)
    sp = M.Mel("image", bank(n_fft, 20), samples, frames, hop, src=src, out=out, channels=2, channel=1, power=power, log=log,
               scale=scale, bias=scale * 2)
    _, bits, _ = run(dec.mel, sp, 3)
    close(sp, [v[:, 1] for v in val], bits, f"{src} power {power} log {log}")


def test_row_lists_and_bad_rows(dec):
    n_fft, hop, samples, frames = 64, 16, 200, 13
    xs = [noise(samples, seed=20 + i) for i in range(5)]
    recs = [feats(xs[0].tobytes()), [("image", "bytes_list", [])], feats(xs[2].tobytes(), n=2), [("other", "int64_list", [1])],
            feats(xs[4].tobytes())]
    dec.decode(*write(recs))
    sp = M.Mel("image", bank(n_fft, 20), samples, frames, hop, out="float16", fill=2.5, lengths=True)
    rows = [4, 4, 0, -1, 1, 5, 2, 3, 1 << 40, 0]
    got, bits, lens = run(dec.mel, sp, len(rows), rows=np.array(rows, np.int64))
    for k, g in enumerate(rows):
        if not 0 <= g < 5:
            assert (np.ascontiguousarray(bits[k]).view(np.uint8) == POISON).all() and lens[k] == POISON32
        elif g in (1, 3):  # (an empty list, a missing key: fill, untransformed)
            assert (bits[k] == np.float16(2.5).view(np.uint16)).all() and lens[k] == 0
        else:  # (a record with two elements gives element 0's spectrogram and counts as multi)
            close(sp, [xs[g]], bits[k : k + 1])
            assert lens[k] == 2 * samples
    assert got.stats["image"].tolist() == [0, 2, 2, 1] and got.skipped == 3


def test_two_banks_share_a_call_and_shard_decoder_two_batches():
    import torch

    xs = [noise(2000, seed=40 + i) for i in range(24)]
    buf, st, en = write([feats(x.tobytes()) for x in xs])
    sd = shard.ShardDecoder(0, int(buf.size) // 2 + 256, 2, balanced=False)
    try:
        plan = sd.plan(st, en, int(buf.size))
        assert len(plan) == 2
        rst, ren = sd.rebase(plan, st, en)
        d_bytes = torch.zeros(((buf.size + 15) // 16) * 16 + 16, dtype=torch.uint8, device=dev())
        d_bytes[: buf.size].copy_(torch.from_numpy(buf.copy()))
        d_st, d_en = torch.from_numpy(rst.view(np.int64)).to(dev()), torch.from_numpy(ren.view(np.int64)).to(dev())
        sd.learn(plan, buf, st, en)
        sd.decode_device(plan, d_bytes.data_ptr(), d_st.data_ptr(), d_en.data_ptr())
        # (tiles of 64 and of 32 frames: two launches behind one call)
        a = M.Mel("image", bank(64, 20), 2000, 70, 16, name="a", scale=0.5, bias=1.0)
        b = M.Mel("image", bank(1024, 128), 2000, 4, 256, name="b", center=False, log="ln")
        assert M.tile_frames(64, 16) != M.tile_frames(1024, 256)
        rows = np.random.default_rng(0).permutation(24)[:10].tolist() + [24]
        got = sd.mel(plan, [a, b], rows=torch.tensor(rows, device=dev()))
        for sp in (a, b):
            t = got[sp.name][:10].cpu().numpy().view(np.uint32)
            close(sp, [xs[r] for r in rows[:10]], t)
        assert got.skipped == 1 and got.stats["a"].tolist() == [0, 0, 0, 0] and got.stats["b"].tolist() == [0, 0, 0, 0]
    finally:
        sd.close()


def test_refusals_leave_the_outputs_alone(dec):
    import torch

    x = noise(200, seed=9)
    dec.decode(*write([feats(x.tobytes())] * 4))
    lib, bk = dec._lib, bank(64, 20)
    p = C.c_void_p()
    ones = np.ones(33 * 2, np.float32)
    for n_fft in (63, 0, 4096):  # (an odd n_fft, and the range)
        assert lib.tfrg_mel_create(0, n_fft, N.ptr(ones), 2, N.ptr(ones), C.byref(p)) == -1 and not p
        assert b"tfrg_mel_create: " in lib.tfrg_last_error()
    good = M.Mel("image", bk, 200, 13, 16, lengths=True)
    slot = W.D.resolve_slot(dec, good)
    big = torch.full((4096 * 4,), POISON, dtype=torch.uint8, device=dev())

    def call(n_specs=1, rows_dtype=N.ROWS_I64, m=1, **over):
        arr = (N.TfrgMelSpec * 17)()
        for s in arr:
            s.slot, s.src, s.out, s.channels, s.samples, s.frames, s.hop, s.center, s.power = slot, N.RAW_I16, 0, 1, 200, 13, 16, 1, 2
            s.log, s.floor, s.scale, s.mel, s.out_ptr = N.MEL_LOG10, 1e-10, 1.0, bk.handle(0), big.data_ptr() + 256
            for k, v in over.items():
                setattr(s, k, v)
        rc = lib.tfrg_result_mel(dec._ctx, arr, n_specs, C.c_void_p(big.data_ptr()), rows_dtype, m, 0, None, None, None)
        assert rc == -1 and lib.tfrg_last_error().startswith(b"tfrg_result_mel: ")

    class OtherDevice(C.Structure):  # (the head of the object behind the handle: its device ordinal)
        _fields_ = [("device", C.c_int)]

    for kw in (dict(n_specs=0), dict(n_specs=17), dict(slot=1 << 20), dict(src=8), dict(out=N.RAW_OUT_SAME), dict(floor=0.0),
               dict(frames=14), dict(center=0, frames=10), dict(samples=32), dict(hop=0), dict(hop=65), dict(power=3), dict(log=3),
               dict(channels=0), dict(channel=1), dict(mel=None), dict(out_ptr=None), dict(out_ptr=big.data_ptr() + 2),
               dict(reserved=1), dict(scale=float("nan")), dict(rows_dtype=2), dict(m=1 << 31)):
        call(**kw)
    other = C.cast(bk.handle(0), C.POINTER(OtherDevice))
    other[0].device = 1
    try:
        call()  # (a bank of another device)
    finally:
        other[0].device = 0
    torch.cuda.synchronize()
    assert (big.cpu().numpy() == POISON).all()
    _, bits, lens = run(dec.mel, good, 4)  # (then the accepted spec writes)
    close(good, [x] * 4, bits)
    assert lens.tolist() == [400] * 4
