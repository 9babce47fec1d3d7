"""The argument checks of the three fixed-shape row passes over a decoded result -- tfrg_result_raw_rows,
tfrg_result_raw_resize, tfrg_result_mel -- pinned to their exact return code and ``tfrg_last_error()``
text, and, for a call with two defects, to the one that is reported (the order of the checks). Every such
call is refused before anything is launched: the buffers keep their poison. (tests/test_result_args_gpu.py
does the same for dense, ragged and select.) One check is out of reach of a test on one device: a mel
spec whose tables are on another device than the context. The last test is the other side: the two calls
that succeed without a launch, over a result without records and with m == 0."""

import ctypes as C

import numpy as np
import pytest

from tfr_reader import _native as N
from tfr_reader import hip, synth, writer

pytestmark = pytest.mark.gpu

E_ARG = -1
POISON = 0x5A
S_I, S_F, S_B = 0, 1, 2  # the slots of the three keys, in the order the records name them
KIND = {S_I: 3, S_F: 2, S_B: 1}  # TFRG_KIND_*
ROWS_ERR = "rows_dtype must be TFRG_ROWS_I32 or TFRG_ROWS_I64, not 7"
N_FFT, N_MELS = 16, 2
INF = float("inf")


def vp(p):
    return C.c_void_p(p) if p else None


class Calls:
    """The three entry points on one decoder with valid defaults; every call returns
    (return code, error text)."""

    def __init__(self, dec) -> None:
        import torch

        self.dec, self.lib = dec, N.lib()
        dev = torch.device("cuda", 0)
        self.bufs = {k: torch.full((64,), POISON, dtype=torch.uint8, device=dev)
                     for k in ("out", "rows", "stats", "skipped", "boxes", "flips", "shapes", "lengths")}
        self.p = {k: t.data_ptr() for k, t in self.bufs.items()}
        window = (C.c_float * N_FFT)(*([1.0] * N_FFT))
        fb = (C.c_float * (N_MELS * (N_FFT // 2 + 1)))(*([0.5] * (N_MELS * (N_FFT // 2 + 1))))
        mel = C.c_void_p()
        N.check(self.lib.tfrg_mel_create(0, N_FFT, window, N_MELS, fb, C.byref(mel)), "tfrg_mel_create")
        self.mel = mel.value

    def close(self) -> None:
        N.check(self.lib.tfrg_mel_destroy(self.mel), "tfrg_mel_destroy")

    def _done(self, rc: int):
        return rc, self.lib.tfrg_last_error().decode()

    def _call(self, fn, cls, f, kw, extra=()):
        k, ctx, specs = kw.pop("k", 1), kw.pop("ctx", True), kw.pop("specs", True)
        rows, rdt, m = kw.pop("rows", True), kw.pop("rdt", N.ROWS_I64), kw.pop("m", 4)
        f.update(kw)
        arr = (cls * max(k, 1))(*[cls(**f) for _ in range(max(k, 1))])
        return self._done(getattr(self.lib, fn)(
            self.dec._ctx if ctx else None, arr if specs else None, k, vp(self.p["rows"]) if rows else None, rdt, m, 0,
            *extra, vp(self.p["stats"]), vp(self.p["skipped"]), None))

    def raw(self, **kw):
        f = dict(slot=S_B, src=N.RAW_U8, out=N.RAW_OUT_F32, count=4, channels=1, planar=0, fill=0, reserved=0,
                 out_ptr=self.p["out"], lengths=None)
        return self._call("tfrg_result_raw_rows", N.TfrgRawSpec, f, kw)

    def resize(self, boxes=0, **kw):
        f = dict(slot=S_B, src=N.RAW_U8, out=N.RAW_OUT_F32, channels=1, h_slot=N.RESIZE_CONST, w_slot=N.RESIZE_CONST,
                 src_h=2, src_w=2, out_h=2, out_w=2, interp=N.RESIZE_BILINEAR, planar=0, fill=0, reserved=0,
                 out_ptr=self.p["out"], shapes=None)
        extra = (vp(self.p["boxes"] + boxes) if boxes is not None else None, vp(self.p["flips"]))
        return self._call("tfrg_result_raw_resize", N.TfrgResizeSpec, f, kw, extra)

    def melspec(self, **kw):
        f = dict(slot=S_B, src=N.RAW_I16, out=N.RAW_OUT_F32, channels=1, channel=0, samples=N_FFT, frames=1, hop=8,
                 center=0, power=2, log=N.MEL_LINEAR, fill=0, floor=0.0, scale=1.0, bias=0.0, reserved=0, mel=self.mel,
                 out_ptr=self.p["out"], lengths=None)
        return self._call("tfrg_result_mel", N.TfrgMelSpec, f, kw)

    def host(self, name: str) -> list[int]:
        import torch

        torch.cuda.synchronize()
        return self.bufs[name].cpu().numpy().view(np.uint32).tolist()

    def untouched(self, but=()) -> bool:
        import torch

        torch.cuda.synchronize()
        return all(bool((t == POISON).all()) for k, t in self.bufs.items() if k not in but)


@pytest.fixture
def calls():
    mp = pytest.MonkeyPatch()
    mp.setenv("TFRG_OPTIMISTIC", "1")  # (read at context creation; the suite may run with 0)
    mp.setenv("TFRG_TEMPLATES", "1")
    try:
        dec = hip.HipDecoder(0)
    finally:
        mp.undo()
    c = Calls(dec)
    yield c
    c.close()
    dec.close()


def decode4(c: Calls, n: int = 4) -> None:
    """Four records (``n`` 0: a result without records, of the same schema); the bytes element holds one
    frame of N_FFT int16 samples."""
    recs = [writer.encode_example([("a_int", "int64_list", [i]), ("b_float", "float_list", [0.5 * i]),
                                   ("c_bytes", "bytes_list", [bytes(range(2 * N_FFT))])]) for i in range(4)]
    buf, st, en = synth.framed(recs)
    res = c.dec.decode(buf, st, en)
    assert res.slot_key == ["a_int", "b_float", "c_bytes"] and list(res.slot_kind) == [KIND[S_I], KIND[S_F], KIND[S_B]]
    if n == 0:
        assert len(c.dec.decode(buf[:0], st[:0], en[:0])) == 0


ENTRY = {"tfrg_result_raw_rows": Calls.raw, "tfrg_result_raw_resize": Calls.resize, "tfrg_result_mel": Calls.melspec}


def test_no_context_and_no_result_before_a_decode(calls):
    c = calls
    for fn, call in ENTRY.items():
        assert call(c, ctx=False) == (E_ARG, f"{fn}: no context")
        assert call(c, ctx=False, k=0) == (E_ARG, f"{fn}: no context")
        assert call(c) == (E_ARG, f"{fn}: no result (decode first)")
        # (two defects: the missing result is reported before the count, and before a NULL spec table)
        assert call(c, k=0) == (E_ARG, f"{fn}: no result (decode first)")
        assert call(c, k=17) == (E_ARG, f"{fn}: no result (decode first)")
        assert call(c, specs=False) == (E_ARG, f"{fn}: no result (decode first)")
    assert c.resize(boxes=2) == (E_ARG, "tfrg_result_raw_resize: no result (decode first)")
    assert c.untouched()


def rows_checks(call, err, bad_spec: dict, bad_spec_err: str) -> None:
    """The count and the row list, which the three check alike: rows_dtype only beside a list (NULL: every
    record in order), then m; the specs before both."""
    assert call(k=0) == err("n_specs must be 1..16")
    assert call(k=17) == err("n_specs must be 1..16")
    assert call(specs=False) == err("n_specs must be 1..16")
    assert call(k=17, **bad_spec) == err("n_specs must be 1..16")
    assert call(k=2, **bad_spec) == err(bad_spec_err)  # (the first bad spec)
    assert call(rdt=7) == err(ROWS_ERR)
    assert call(m=1 << 31) == err("m must be below 2^31")
    assert call(m=1 << 31, rows=False) == err("m must be below 2^31")
    assert call(rdt=7, **bad_spec) == err(bad_spec_err)
    assert call(rdt=7, m=1 << 31) == err(ROWS_ERR)
    assert call(rdt=7, m=1 << 31, rows=False) == err("m must be below 2^31")  # (no list: its dtype is not read)


def test_raw_rows_checks(calls):
    c = calls
    decode4(c)

    def err(why: str):
        return E_ARG, f"tfrg_result_raw_rows: {why}"

    assert c.raw(slot=3) == err("spec 0: slot 3 >= n_slots")
    assert c.raw(slot=S_I) == err("spec 0: slot 0 is not a bytes_list slot (kind 3)")
    assert c.raw(slot=S_F) == err("spec 0: slot 1 is not a bytes_list slot (kind 2)")
    assert c.raw(src=8) == err("spec 0: unknown src 8")
    assert c.raw(out=4) == err("spec 0: unknown out 4")
    assert c.raw(count=0) == err("spec 0: count must be 1..16777216")
    assert c.raw(count=(1 << 24) + 1) == err("spec 0: count must be 1..16777216")
    assert c.raw(channels=0) == err("spec 0: channels must be 1..16")
    assert c.raw(channels=17, count=34) == err("spec 0: channels must be 1..16")
    assert c.raw(channels=3) == err("spec 0: count must be a multiple of channels")
    assert c.raw(planar=2) == err("spec 0: planar must be 0 or 1")
    assert c.raw(out_ptr=None) == err("spec 0: out_ptr is NULL")
    assert c.raw(out_ptr=c.p["out"] + 2) == err("spec 0: out_ptr must be aligned to the output element size")
    assert c.raw(out_ptr=c.p["out"] + 1, out=N.RAW_OUT_BF16) == err("spec 0: out_ptr must be aligned to the output element size")
    assert c.raw(out_ptr=c.p["out"] + 1, out=N.RAW_OUT_SAME, src=N.RAW_I16) == \
        err("spec 0: out_ptr must be aligned to the output element size")
    assert c.raw(reserved=1) == err("spec 0: reserved must be 0")
    # two defects: slot, src, out, count, channels, their ratio, planar, out_ptr, its alignment, reserved
    assert c.raw(slot=3, src=8) == err("spec 0: slot 3 >= n_slots")
    assert c.raw(src=8, out=4) == err("spec 0: unknown src 8")
    assert c.raw(out=4, count=0) == err("spec 0: unknown out 4")
    assert c.raw(count=0, channels=0) == err("spec 0: count must be 1..16777216")
    assert c.raw(channels=17, count=35) == err("spec 0: channels must be 1..16")
    assert c.raw(channels=3, planar=2) == err("spec 0: count must be a multiple of channels")
    assert c.raw(planar=2, out_ptr=None) == err("spec 0: planar must be 0 or 1")
    assert c.raw(out_ptr=None, reserved=1) == err("spec 0: out_ptr is NULL")
    assert c.raw(out_ptr=c.p["out"] + 2, reserved=1) == err("spec 0: out_ptr must be aligned to the output element size")
    rows_checks(c.raw, err, dict(reserved=1), "spec 0: reserved must be 0")
    assert c.untouched()


def test_raw_resize_checks(calls):
    c = calls
    decode4(c)
    AA = N.RESIZE_ANTIALIAS

    def err(why: str):
        return E_ARG, f"tfrg_result_raw_resize: {why}"

    assert c.resize(slot=3) == err("spec 0: slot 3 >= n_slots")
    assert c.resize(slot=S_I) == err("spec 0: slot 0 is not a bytes_list slot (kind 3)")
    assert c.resize(src=8) == err("spec 0: unknown src 8")
    assert c.resize(out=4) == err("spec 0: unknown out 4")
    assert c.resize(interp=N.RESIZE_NEAREST | AA) == err("spec 0: TFRG_RESIZE_ANTIALIAS filters: it goes with TFRG_RESIZE_BILINEAR only")
    assert c.resize(interp=2) == err("spec 0: unknown interp 2")
    assert c.resize(interp=2 | AA) == err("spec 0: unknown interp 258")
    assert c.resize(out=N.RAW_OUT_SAME) == err("spec 0: TFRG_RAW_OUT_SAME copies bits: it goes with TFRG_RESIZE_NEAREST only")
    assert c.resize(out=N.RAW_OUT_SAME, interp=AA) == err("spec 0: TFRG_RAW_OUT_SAME copies bits: it goes with TFRG_RESIZE_NEAREST only")
    assert c.resize(channels=0) == err("spec 0: channels must be 1..4")
    assert c.resize(channels=5) == err("spec 0: channels must be 1..4")
    for kw in (dict(out_h=0), dict(out_h=4097), dict(out_w=0), dict(out_w=4097)):
        assert c.resize(**kw) == err("spec 0: out_h and out_w must be 1..4096")
    assert c.resize(out_w=2048, channels=3) == err("spec 0: out_w * channels must be at most 4096")
    for kw in (dict(src_h=0), dict(src_h=16385), dict(src_w=0), dict(src_w=16385)):
        assert c.resize(**kw) == err("spec 0: a constant extent must be 1..16384")
    assert c.resize(h_slot=3) == err("spec 0: h_slot 3 is not an int64_list slot")
    assert c.resize(h_slot=S_B) == err("spec 0: h_slot 2 is not an int64_list slot")
    assert c.resize(w_slot=S_F) == err("spec 0: w_slot 1 is not an int64_list slot")
    assert c.resize(planar=2) == err("spec 0: planar must be 0 or 1")
    assert c.resize(out_ptr=None) == err("spec 0: out_ptr is NULL")
    assert c.resize(out_ptr=c.p["out"] + 2) == err("spec 0: out_ptr must be aligned to the output element size")
    assert c.resize(shapes=c.p["shapes"] + 2) == err("spec 0: shapes must be 4-byte aligned")
    assert c.resize(reserved=1) == err("spec 0: reserved must be 0")
    assert c.resize(boxes=2) == err("d_boxes must be 4-byte aligned")
    # two defects: slot, src, out, the interp rules, channels, the output's extents, the source's (h before
    # w), planar, out_ptr, its alignment, shapes, reserved
    assert c.resize(slot=3, src=8) == err("spec 0: slot 3 >= n_slots")
    assert c.resize(src=8, out=4) == err("spec 0: unknown src 8")
    assert c.resize(out=4, interp=2) == err("spec 0: unknown out 4")
    assert c.resize(interp=N.RESIZE_NEAREST | AA, out=N.RAW_OUT_SAME) == \
        err("spec 0: TFRG_RESIZE_ANTIALIAS filters: it goes with TFRG_RESIZE_BILINEAR only")
    assert c.resize(interp=2, out=N.RAW_OUT_SAME) == err("spec 0: unknown interp 2")
    assert c.resize(out=N.RAW_OUT_SAME, channels=0) == err("spec 0: TFRG_RAW_OUT_SAME copies bits: it goes with TFRG_RESIZE_NEAREST only")
    assert c.resize(channels=5, out_h=0) == err("spec 0: channels must be 1..4")
    assert c.resize(out_h=0, out_w=2048, channels=3) == err("spec 0: out_h and out_w must be 1..4096")
    assert c.resize(out_w=2048, channels=3, src_h=0) == err("spec 0: out_w * channels must be at most 4096")
    assert c.resize(src_h=0, w_slot=S_F) == err("spec 0: a constant extent must be 1..16384")
    assert c.resize(h_slot=S_B, src_w=0) == err("spec 0: h_slot 2 is not an int64_list slot")
    assert c.resize(w_slot=S_F, planar=2) == err("spec 0: w_slot 1 is not an int64_list slot")
    assert c.resize(planar=2, out_ptr=None) == err("spec 0: planar must be 0 or 1")
    assert c.resize(out_ptr=None, shapes=c.p["shapes"] + 2) == err("spec 0: out_ptr is NULL")
    assert c.resize(out_ptr=c.p["out"] + 2, shapes=c.p["shapes"] + 2) == err("spec 0: out_ptr must be aligned to the output element size")
    assert c.resize(shapes=c.p["shapes"] + 2, reserved=1) == err("spec 0: shapes must be 4-byte aligned")
    rows_checks(c.resize, err, dict(reserved=1), "spec 0: reserved must be 0")
    # d_boxes comes last: after the specs, rows_dtype and m
    assert c.resize(boxes=2, reserved=1) == err("spec 0: reserved must be 0")
    assert c.resize(boxes=2, rdt=7) == err(ROWS_ERR)
    assert c.resize(boxes=2, m=1 << 31) == err("m must be below 2^31")
    assert c.resize(boxes=2, k=17) == err("n_specs must be 1..16")
    assert c.untouched()


def test_mel_checks(calls):
    c = calls
    decode4(c)

    def err(why: str):
        return E_ARG, f"tfrg_result_mel: {why}"

    assert c.melspec(slot=3) == err("spec 0: slot 3 >= n_slots")
    assert c.melspec(slot=S_I) == err("spec 0: slot 0 is not a bytes_list slot (kind 3)")
    assert c.melspec(src=8) == err("spec 0: unknown src 8")
    assert c.melspec(out=N.RAW_OUT_SAME) == err("spec 0: out must be TFRG_RAW_OUT_F32, _F16 or _BF16, not 3")
    assert c.melspec(out=4) == err("spec 0: out must be TFRG_RAW_OUT_F32, _F16 or _BF16, not 4")
    assert c.melspec(mel=None) == err("spec 0: mel is NULL")
    assert c.melspec(channels=0) == err("spec 0: channels must be 1..16")
    assert c.melspec(channels=17) == err("spec 0: channels must be 1..16")
    assert c.melspec(channel=1) == err("spec 0: channel must be below channels")
    assert c.melspec(samples=0) == err("spec 0: samples must be 1..16777216")
    assert c.melspec(samples=(1 << 24) + 1) == err("spec 0: samples must be 1..16777216")
    assert c.melspec(frames=0) == err("spec 0: frames must be 1..1048576")
    assert c.melspec(frames=(1 << 20) + 1) == err("spec 0: frames must be 1..1048576")
    assert c.melspec(hop=0) == err("spec 0: hop must be 1..n_fft")
    assert c.melspec(hop=N_FFT + 1) == err("spec 0: hop must be 1..n_fft")
    assert c.melspec(center=2) == err("spec 0: center must be 0 or 1")
    assert c.melspec(power=0) == err("spec 0: power must be 1 or 2")
    assert c.melspec(power=3) == err("spec 0: power must be 1 or 2")
    assert c.melspec(log=3) == err("spec 0: unknown log 3")
    assert c.melspec(log=N.MEL_LN) == err("spec 0: a log needs a finite floor > 0")
    assert c.melspec(log=N.MEL_LOG10, floor=INF) == err("spec 0: a log needs a finite floor > 0")
    assert c.melspec(log=N.MEL_LN, floor=float("nan")) == err("spec 0: a log needs a finite floor > 0")
    assert c.melspec(scale=INF) == err("spec 0: scale and bias must be finite")
    assert c.melspec(bias=float("nan")) == err("spec 0: scale and bias must be finite")
    assert c.melspec(center=1, samples=N_FFT // 2) == err("spec 0: center reflects: samples must exceed n_fft / 2")
    assert c.melspec(center=1, samples=9, frames=3) == err("spec 0: the last frame's centre lies past samples")
    assert c.melspec(frames=2) == err("spec 0: the last frame ends past samples")
    assert c.melspec(out_ptr=None) == err("spec 0: out_ptr is NULL")
    assert c.melspec(out_ptr=c.p["out"] + 2) == err("spec 0: out_ptr must be aligned to the output element size")
    assert c.melspec(out_ptr=c.p["out"] + 1, out=N.RAW_OUT_F16) == err("spec 0: out_ptr must be aligned to the output element size")
    assert c.melspec(lengths=c.p["lengths"] + 2) == err("spec 0: lengths must be 4-byte aligned")
    assert c.melspec(reserved=1) == err("spec 0: reserved must be 0")
    # two defects: slot, src, out, mel, channels, channel, samples, frames, hop, center, power, log, floor,
    # scale and bias, the framing, out_ptr, its alignment, lengths, reserved
    assert c.melspec(slot=3, src=8) == err("spec 0: slot 3 >= n_slots")
    assert c.melspec(src=8, out=3) == err("spec 0: unknown src 8")
    assert c.melspec(out=3, mel=None) == err("spec 0: out must be TFRG_RAW_OUT_F32, _F16 or _BF16, not 3")
    assert c.melspec(mel=None, channels=0) == err("spec 0: mel is NULL")
    assert c.melspec(channels=17, channel=17) == err("spec 0: channels must be 1..16")
    assert c.melspec(channel=1, samples=0) == err("spec 0: channel must be below channels")
    assert c.melspec(samples=0, frames=0) == err("spec 0: samples must be 1..16777216")
    assert c.melspec(frames=0, hop=0) == err("spec 0: frames must be 1..1048576")
    assert c.melspec(hop=0, center=2) == err("spec 0: hop must be 1..n_fft")
    assert c.melspec(center=2, power=3) == err("spec 0: center must be 0 or 1")
    assert c.melspec(power=3, log=3) == err("spec 0: power must be 1 or 2")
    assert c.melspec(log=3, scale=INF) == err("spec 0: unknown log 3")
    assert c.melspec(log=N.MEL_LN, scale=INF) == err("spec 0: a log needs a finite floor > 0")
    assert c.melspec(scale=INF, frames=2) == err("spec 0: scale and bias must be finite")
    assert c.melspec(frames=2, out_ptr=None) == err("spec 0: the last frame ends past samples")
    assert c.melspec(out_ptr=None, lengths=c.p["lengths"] + 2) == err("spec 0: out_ptr is NULL")
    assert c.melspec(out_ptr=c.p["out"] + 2, lengths=c.p["lengths"] + 2) == err("spec 0: out_ptr must be aligned to the output element size")
    assert c.melspec(lengths=c.p["lengths"] + 2, reserved=1) == err("spec 0: lengths must be 4-byte aligned")
    rows_checks(c.melspec, err, dict(reserved=1), "spec 0: reserved must be 0")
    assert c.untouched()


@pytest.mark.parametrize("fn", sorted(ENTRY))
def test_no_record_or_no_row_launches_nothing(calls, fn):
    """Over a result without records every row is skipped: m in each spec's skipped counter, the stats
    zeroed. With m == 0 over a result with records both are zeroed. Neither launches: the output and every
    other buffer keep their poison, and so do the counters' words past n_specs."""
    c = calls
    P32 = int.from_bytes(bytes([POISON] * 4), "little")
    for n, m, rows in ((0, 4, True), (0, 4, False), (4, 0, True), (4, 0, False)):
        for t in c.bufs.values():
            t.fill_(POISON)
        decode4(c, n)
        assert ENTRY[fn](c, k=2, m=m, rows=rows)[0] == 0
        assert c.host("stats") == [0] * 8 + [P32] * 8
        assert c.host("skipped") == [m if n == 0 else 0] * 2 + [P32] * 14
        assert c.untouched(but=("stats", "skipped"))
