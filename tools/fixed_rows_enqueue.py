"""Host cost of the three fixed-shape row passes (GPU box): tfrg_result_raw_rows, tfrg_result_raw_resize and
tfrg_result_mel as C calls, K = 200 back to back without a synchronize (the host side alone, while the GPU
runs behind), then one synchronize -- what tools/host_enqueue.py does for the decode call. One decode of
256 small records stays resident; the row counts are the smallest of tools/raw_speed.py, resize_speed.py
(256) and mel_speed.py (16), on small elements, so that the call and not the kernel is what is timed. The
library is the one TFRG_LIB names (tools/build_rev.sh builds a parent's). Prints one JSON line:
{entry point: [enqueue ms per call, total ms per call]}.   usage: fixed_rows_enqueue.py"""
import ctypes as C
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, "tfrecords-reader_amd")
sys.path.insert(0, ".")
from tfr_reader import _native as N  # noqa: E402
from tfr_reader import hip, synth, writer  # noqa: E402

K, RECORDS, SIDE, OUT, SAMPLES, N_FFT, HOP, N_MELS = 200, 256, 32, 16, 1024, 64, 32, 8
FRAMES = 1 + (SAMPLES - N_FFT) // HOP
dev = torch.device("cuda", 0)
rng = np.random.default_rng(0)
recs = [writer.encode_example([("image", "bytes_list", [rng.integers(0, 256, SIDE * SIDE * 3, dtype=np.uint8).tobytes()]),
                               ("pcm", "bytes_list", [rng.integers(-3000, 3000, SAMPLES, dtype=np.int16).tobytes()]),
                               ("label", "int64_list", [i])]) for i in range(RECORDS)]
dec = hip.HipDecoder(0)
res = dec.decode(*synth.framed(recs))
assert int(res.status.max()) == 0
image, pcm = res.slot_key.index("image"), res.slot_key.index("pcm")
lib, ctx = dec._lib, dec._ctx
ones = (C.c_float * 16)(*([1.0] * 16))


def ptr(t):
    return C.c_void_p(t.data_ptr())


def rows_of(m):
    return torch.randperm(RECORDS, device=dev)[:m].contiguous()


def counters():
    return torch.zeros(8, dtype=torch.int32, device=dev)


calls = {}
m, rows, out, cnt = 256, rows_of(256), torch.empty(256 * SIDE * SIDE * 3, dtype=torch.bfloat16, device=dev), counters()
raw = (N.TfrgRawSpec * 1)(N.TfrgRawSpec(slot=image, src=N.RAW_U8, out=N.RAW_OUT_BF16, count=SIDE * SIDE * 3, channels=3, planar=1,
                                        scale=ones, out_ptr=out.data_ptr()))
calls["tfrg_result_raw_rows"] = (lib.tfrg_result_raw_rows, (ctx, raw, 1, ptr(rows), N.ROWS_I64, m, 0, ptr(cnt), ptr(cnt[4:]), None),
                                 (rows, out, cnt))
out, cnt = torch.empty(256 * OUT * OUT * 3, dtype=torch.float32, device=dev), counters()
rsz = (N.TfrgResizeSpec * 1)(N.TfrgResizeSpec(slot=image, src=N.RAW_U8, out=N.RAW_OUT_F32, channels=3, h_slot=N.RESIZE_CONST,
                                              w_slot=N.RESIZE_CONST, src_h=SIDE, src_w=SIDE, out_h=OUT, out_w=OUT,
                                              interp=N.RESIZE_BILINEAR, scale=(C.c_float * 4)(1, 1, 1, 1), out_ptr=out.data_ptr()))
calls["tfrg_result_raw_resize"] = (lib.tfrg_result_raw_resize,
                                   (ctx, rsz, 1, ptr(rows), N.ROWS_I64, m, 0, None, None, ptr(cnt), ptr(cnt[4:]), None), (out, cnt))
m, rows16, out, cnt = 16, rows_of(16), torch.empty(16 * N_MELS * FRAMES, dtype=torch.float32, device=dev), counters()
bank = C.c_void_p()
N.check(lib.tfrg_mel_create(0, N_FFT, (C.c_float * N_FFT)(*np.hanning(N_FFT).tolist()), N_MELS,
                            (C.c_float * (N_MELS * (N_FFT // 2 + 1)))(*([0.25] * (N_MELS * (N_FFT // 2 + 1)))), C.byref(bank)),
        "tfrg_mel_create")
mel = (N.TfrgMelSpec * 1)(N.TfrgMelSpec(slot=pcm, src=N.RAW_I16, out=N.RAW_OUT_F32, channels=1, samples=SAMPLES, frames=FRAMES,
                                        hop=HOP, power=2, log=N.MEL_LINEAR, scale=1.0, mel=bank.value, out_ptr=out.data_ptr()))
calls["tfrg_result_mel"] = (lib.tfrg_result_mel, (ctx, mel, 1, ptr(rows16), N.ROWS_I64, m, 0, ptr(cnt), ptr(cnt[4:]), None),
                            (rows16, out, cnt))

result = {}
for name, (fn, args, _keep) in calls.items():
    for _ in range(20):
        assert fn(*args) == 0, lib.tfrg_last_error()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(K):
        fn(*args)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    result[name] = [round(1e3 * (t1 - t0) / K, 5), round(1e3 * (t2 - t0) / K, 5)]
print(json.dumps(result), flush=True)
N.check(lib.tfrg_mel_destroy(bank), "tfrg_mel_destroy")
dec.close()
