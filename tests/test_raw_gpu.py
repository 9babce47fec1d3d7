"""Raw tensors from bytes features on the device (tfrg_result_raw_rows: k_raw). Every test makes a numpy
array per record, stores ``arr.tobytes()`` in a bytes feature and decodes; the expectation is computed
from those arrays in float64 (``v * scale + bias``, rounded once to float32, then RNE to float16 /
bfloat16), never from ``BatchResult.raw`` or the decode's columns. With scale and bias of at most 12
significant bits and sources of at most 24 the float64 expression is exact, so it equals fmaf bit for
bit: bits are compared. The one case with ImageNet mean / std allows 1 ulp of the output type. Outputs
lie inside 0xA5-poisoned buffers: guards, skipped rows and refused calls keep the poison."""

import ctypes as C

import numpy as np
import pytest

from tfr_reader import _native as N
from tfr_reader import hip, shard, synth, writer
from tfr_reader import raw as W

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 256
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SCALE, BIAS = (3 / 256, 1.25, -0.5, 0.75), (-0.5, 0.25, 1.5, -2.0)
NP_SRC = {"uint8": np.uint8, "int8": np.int8, "uint16": np.uint16, "int16": np.int16, "int32": np.int32,
          "float16": np.float16, "bfloat16": np.uint16, "float32": np.float32}
T = W.tile_elems(1)


def dev():
    import torch

    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def dec():
    d = hip.HipDecoder(0)
    yield d
    d.close()


def arrays(src, count, n, seed=0):
    """n arrays of `count` elements of `src`, values whose results stay in the 16-bit types' normal range."""
    rng = np.random.default_rng(seed)
    if src in ("float16", "float32", "bfloat16"):
        v = (rng.uniform(0.5, 8.0, (n, count)) * rng.choice([-1.0, 1.0], (n, count))).astype(np.float32)
        if src == "bfloat16":
            return list((v.view(np.uint32) >> 16).astype(np.uint16))
        return list(v.astype(NP_SRC[src]))
    lo, hi = {"uint8": (0, 256), "int8": (-128, 128), "uint16": (0, 65536), "int16": (-32768, 32768),
              "int32": (-(1 << 20), 1 << 20)}[src]
    return list(rng.integers(lo, hi, (n, count)).astype(NP_SRC[src]))


def write(elems):
    """Records with the bytes feature "t" (`elems[i]`: its list of byte strings, None: no such key) after
    a string feature whose length is chosen so that record i's element starts at i mod 16."""
    payloads, pos = [], 0
    for i, e in enumerate(elems):
        label = ("label", "int64_list", [i])
        tail = len(writer.encode_example([label])) - 2 + sum(len(writer._ld(1, x)) for x in (e or [])[1:])
        for p in range(16):
            f = [("pre", "bytes_list", [b"p" * p])] + ([("t", "bytes_list", e)] if e is not None else [])
            payload = writer.encode_example(f + [label])
            if not e or (pos + 12 + len(payload) - tail - len(e[0])) % 16 == i % 16:
                break
        payloads.append(payload)
        pos += len(payload) + 16
    return synth.framed(payloads)


def expect(sp, elems, rows, row0=0):
    """(bits [m][count] in output order, written [m], lengths [m], stats, skipped) from the records' own
    bytes: element 0 of the list as whole source elements, in float64; per record once, then per row."""
    n, count, C, esz = len(elems), sp.count, int(sp.channels), W.ITEMSIZE[sp.src]
    ubits = {1: np.uint8, 2: np.uint16, 4: np.uint32}[W.ITEMSIZE[sp.out_type]]
    rec = np.full((n + 1, count), sp.fill_bits, ubits)  # (row n: a skipped row)
    rlen, flags = np.zeros(n + 1, np.int32), np.zeros((n + 1, 4), np.int64)
    for g, e in enumerate(elems):
        e = e or []
        b = bytes(e[0]) if e else b""
        rlen[g], flags[g] = len(b), (len(b) > count * esz, len(b) < count * esz, len(e) == 0, len(e) > 1)
        a = np.frombuffer(b[: min(len(b) // esz, count) * esz], NP_SRC[sp.src])
        if sp.out == "same":
            rec[g, : a.size] = a.view(ubits)
            continue
        x = (a.astype(np.uint32) << 16).view(np.float32) if sp.src == "bfloat16" else a
        ch = np.arange(a.size) % C
        y = (x.astype(np.float64) * np.asarray(sp.scale, np.float64)[ch] + np.asarray(sp.bias, np.float64)[ch]).astype(np.float32)
        if sp.out == "float32":
            rec[g, : a.size] = y.view(np.uint32)
        elif sp.out == "float16":
            rec[g, : a.size] = y.astype(np.float16).view(np.uint16)
        else:
            bits = y.view(np.uint32).astype(np.uint64)
            rec[g, : a.size] = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)
    if sp.planar:
        rec = np.ascontiguousarray(rec.reshape(n + 1, count // C, C).transpose(0, 2, 1)).reshape(n + 1, count)
    rows = [int(v) for v in (range(n) if rows is None else rows)]
    idx = np.array([v - row0 if row0 <= v < row0 + n else n for v in rows], np.int64)
    written = idx < n
    return rec[idx], written, rlen[idx], flags[idx].sum(0).tolist(), int((~written).sum())


def poisoned(sp, m, shift=0):
    """(the whole poisoned byte buffer, the [m, *out_shape] view `shift` elements past 16-byte alignment)."""
    import torch

    osz = W.ITEMSIZE[sp.out_type]
    big = torch.full((GUARD + shift * osz + m * sp.count * osz + GUARD,), POISON, dtype=torch.uint8, device=dev())
    lo = GUARD + shift * osz
    return big, big[lo : lo + m * sp.count * osz].view(W._torch_dtype(sp)).view(m, *sp.out_shape)


def check(dec, sp, elems, rows=None, row0=0, rows_dtype=np.int64, shift=0, ulp=0, run=None, stream=None):
    """One call over poisoned outputs against the expectation; `rows`: entries for a device list."""
    import torch

    m = len(elems) if rows is None else len(rows)
    big, view = poisoned(sp, m, shift)
    lens = torch.full((m + 8,), -1515870811, dtype=torch.int32, device=dev())  # (0xA5A5A5A5)
    d_rows = None if rows is None else torch.from_numpy(np.array(rows, rows_dtype)).to(dev())
    call = run or (lambda **kw: W._run([(dec, row0, row0 + len(elems))], row0 + len(elems), 0, [sp], **kw))
    got = call(rows=d_rows, out={sp.out_name: (view, lens[:m])}, stream=stream, strict=False)
    want, written, wl, st, skipped = expect(sp, elems, rows if rows is not None else range(row0, row0 + m), row0)
    osz = W.ITEMSIZE[sp.out_type]
    host = big.cpu().numpy()
    lo = GUARD + shift * osz
    assert (host[:lo] == POISON).all() and (host[lo + m * sp.count * osz :] == POISON).all()
    body = host[lo : lo + m * sp.count * osz].view(want.dtype).reshape(m, sp.count)
    assert (body[~written].view(np.uint8) == POISON).all()
    if ulp:
        w = 8 * osz
        order = lambda b: np.where(b >> (w - 1), -(b & ((1 << (w - 1)) - 1)), b & ((1 << (w - 1)) - 1))  # noqa: E731
        diff = np.abs(order(body[written].astype(np.int64)) - order(want[written].astype(np.int64)))
        assert diff.max(initial=0) <= ulp
    else:
        bad = np.argwhere(body[written] != want[written])
        assert bad.size == 0, (bad[:4], body[written][tuple(bad[0])], want[written][tuple(bad[0])])
    hl = lens.cpu().numpy()
    keep = ~written if sp.lengths else np.ones(m, bool)  # (lengths are written for the specs that ask)
    assert np.array_equal(hl[:m][~keep], wl[~keep]) and (hl[:m][keep] == -1515870811).all() and (hl[m:] == -1515870811).all()
    assert got.stats[sp.out_name].tolist() == st and got.skipped == skipped
    return got


def varied(arrs, esz):
    """Element lists around full-length arrays: short by a non-multiple of esz, longer, an empty list, no
    key, two elements."""
    e = [[a.tobytes()] for a in arrs]
    full = e[0][0]
    e[1] = [full[: max(len(full) - esz - 1, 0)]]
    e[2] = [full + b"\x7f" * (2 * esz + 1)]
    e[3], e[4], e[5] = [], None, [full, b"second"]
    return e


ROWS = [5, 0, 17, 17, -1, 3, 7, I64_MAX, 2, 1, 4, I64_MIN, 9, 18, 8, 20, 21, 6]  # (row0 = 3: entries 3..26 are records)


@pytest.mark.parametrize("src,out", [("uint8", "float32"), ("int16", "bfloat16"), ("float32", "float16")])
@pytest.mark.parametrize("count", [1, 3, 15, 16, 17, 1023, 1024, 1025, T - 1, T, T + 1, 2 * T + 5])
def test_counts_lengths_and_row_lists(dec, src, out, count):
    sp = W.Raw("t", src=src, out=out, shape=(count,), scale=SCALE[0], bias=BIAS[0], fill=7, lengths=True)
    elems = varied(arrays(src, count, 24, count), W.ITEMSIZE[src])
    res = dec.decode(*write(elems))
    s = list(res.slot_key).index("t")
    rs, base = np.asarray(res.row_splits[s]).astype(np.int64), int(res.slot_base[s])
    off = {int(res.bytes_off[base + rs[g]]) % 16 for g in range(24) if rs[g + 1] > rs[g]}
    assert len(off) == 16  # the element starts at every residue
    check(dec, sp, elems, rows=ROWS, row0=3)
    check(dec, sp, elems, rows=[2, 0, 1, 5, 40, -7, 3, 4], rows_dtype=np.int32)
    check(dec, sp, elems)  # a NULL d_rows: the identity list
    check(dec, sp, elems, rows=[])  # m == 0


@pytest.mark.parametrize("src,out", [(s, "float32") for s in sorted(NP_SRC)]
                         + [(s, "float16" if i % 2 else "bfloat16") for i, s in enumerate(sorted(NP_SRC))])
def test_every_source_type(dec, src, out):
    sp = W.Raw("t", src=src, out=out, shape=(343, 3), channels=3, scale=SCALE[:3], bias=BIAS[:3], fill=-3)
    elems = varied(arrays(src, 1029, 7, 1), W.ITEMSIZE[src])
    dec.decode(*write(elems))
    check(dec, sp, elems, shift=1)  # (the out pointer one element past 16-byte alignment)


@pytest.mark.parametrize("src", ["uint8", "int16", "float32"])
def test_out_same_copies_bits(dec, src):
    arrs = arrays(src, 1500, 7, 2)
    if src == "float32":
        for a in arrs:
            a.view(np.uint32)[::5] = [0x7FC00001, 0xFFA00123, 0x7F800001, 0x7F800000, 0x00000001] * 60
    sp = W.Raw("t", src=src, out="same", shape=(500, 3), channels=3, planar=True, scale=3.0, fill=1)
    elems = varied(arrs, W.ITEMSIZE[src])
    dec.decode(*write(elems))
    check(dec, sp, elems, rows=[6, 1, 0, 2, 9, 5], shift=1)


@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("hw", [(5, 7), "tile"])
def test_channels_and_planes(dec, hw, C, planar):
    """Plane sizes that are no multiple of 16 bytes; "tile": three pixels more than a tile of pixels."""
    shape = ((*hw, C) if hw != "tile" else (W.tile_elems(C) // C + 3, C))
    for src, out in (("uint8", "bfloat16"), ("float16", "float32")):
        sp = W.Raw("t", src=src, out=out, shape=shape, channels=C, planar=planar, scale=SCALE[:C], bias=BIAS[:C], fill=2)
        elems = varied(arrays(src, sp.count, 6, C), W.ITEMSIZE[src])
        dec.decode(*write(elems))
        check(dec, sp, elems, rows=[5, 1, 0, 2, 0, 7])


@pytest.mark.parametrize("out", ["float32", "bfloat16"])
def test_imagenet_normalize_within_one_ulp(dec, out):
    mean, std = np.array([0.485, 0.456, 0.406]) * 255, np.array([0.229, 0.224, 0.225]) * 255
    sp = W.Raw.normalize("t", mean, std, src="uint8", out=out, shape=(37, 41, 3), channels=3, planar=True)
    assert sp.scale == tuple(float(np.float32(1 / s)) for s in std)
    elems = [[a.tobytes()] for a in arrays("uint8", sp.count, 5, 4)]
    dec.decode(*write(elems))
    got = check(dec, sp, elems, rows=[4, 0, 3], ulp=1)
    assert tuple(got["t"].shape) == (3, 3, 37, 41)


def test_narrow_rows_and_one_wide_row(dec):
    """count = 16 float16 over 300 rows (a wave per row), and one row that Dense cannot serve."""
    arrs = arrays("float16", 16, 300, 5)
    elems = [[a.tobytes()] for a in arrs]
    dec.decode(*write(elems))
    check(dec, W.Raw("t", src="float16", out="float32", shape=(16,), scale=1.25, bias=0.25), elems)
    wide = [[arrays("uint8", 70001, 1, 6)[0].tobytes()]]
    dec.decode(*write(wide))
    assert 70001 > N.DENSE_MAX_WIDTH
    check(dec, W.Raw("t", out="float16", shape=(70001,), scale=0.75, bias=-2.0), wide)


@pytest.mark.parametrize("src,count,m", [("float16", 16, 40000), ("uint8", 1025, 9000)])
def test_more_work_items_than_workgroups(dec, src, count, m):
    """A launch has at most 32 workgroups per CU (8192 on 256 CUs): 40000 narrow rows, a wave each, and
    9000 wide rows, a workgroup each, make every group stride on to further items over the LDS it used."""
    sp = W.Raw("t", src=src, out="same", shape=(count,), fill=3)
    elems = varied(arrays(src, count, 24, 11), W.ITEMSIZE[src])
    dec.decode(*write(elems))
    check(dec, sp, elems, rows=np.random.default_rng(0).integers(-1, 25, m).tolist())


def test_a_callers_stream_and_allocated_outputs(dec):
    """``stream=``: the call is ordered with that stream alone. Outputs the call allocates hold ``fill`` in
    the rows no record fills, and a key the batch does not have is all ``fill``, padded and empty."""
    import torch

    sp = W.Raw("t", src="int16", out="float32", shape=(3000,), scale=SCALE[0], bias=BIAS[0], fill=5, lengths=True)
    gone = W.Raw("nokey", out="bfloat16", shape=(40,), fill=-1.5, lengths=True)
    elems = varied(arrays("int16", 3000, 24, 12), 2)
    dec.decode(*write(elems))
    rows = [23, 0, 1, 99, 2, 3, 4, 5, -1]
    s = torch.cuda.Stream(dev())
    check(dec, sp, elems, rows=rows, stream=s.cuda_stream)
    got = dec.raw([sp, gone], rows=torch.tensor(rows, device=dev()), stream=s.cuda_stream)
    s.synchronize()
    want, _, wl, st, skipped = expect(sp, elems, rows)
    assert np.array_equal(got["t"].cpu().numpy().view(np.uint32), want)
    assert got.lengths["t"].cpu().tolist() == wl.tolist() and got.stats["t"].tolist() == st and got.skipped == skipped == 2
    assert (got["nokey"].cpu().view(torch.int16).numpy().view(np.uint16) == gone.fill_bits).all()
    assert not got.lengths["nokey"].cpu().numpy().any() and got.stats["nokey"].tolist() == [0, 7, 7, 0]


def test_no_rows_launches_nothing(dec):
    """The C entry point with m == 0: success, counters zeroed, nothing else touched."""
    import torch

    elems = [[a.tobytes()] for a in arrays("uint8", 32, 4, 9)]
    dec.decode(*write(elems))
    good = W.Raw("t", shape=(32,))
    big, view = poisoned(good, 4)
    counters = torch.full((5,), 77, dtype=torch.int32, device=dev())
    a = (N.TfrgRawSpec * 1)()
    a[0].slot, a[0].src, a[0].out, a[0].count, a[0].channels = W.D.resolve_slot(dec, good), N.RAW_U8, N.RAW_OUT_F32, 32, 1
    a[0].out_ptr = view.data_ptr()
    for d_rows in (None, C.c_void_p(counters.data_ptr())):
        rc = dec._lib.tfrg_result_raw_rows(dec._ctx, a, 1, d_rows, N.ROWS_I32, 0, 0, C.c_void_p(counters.data_ptr()),
                                           C.c_void_p(counters.data_ptr() + 16), None)
        assert rc == 0
    torch.cuda.synchronize()
    assert counters.cpu().tolist() == [0] * 5 and (big.cpu().numpy() == POISON).all()


def test_materialized_bytes_column(dec):
    sp = W.Raw("t", src="int16", out="float32", shape=(9, 7, 3), channels=3, planar=True, scale=SCALE[:3], bias=BIAS[:3])
    elems = varied(arrays("int16", 189, 9, 7), 2)
    res = dec.decode(*write(elems), materialize_bytes=True)
    assert res.bytes_data is not None
    check(dec, sp, elems, rows=[8, 1, 2, 3, 4, 5, 0])


def test_implicit_offset_slot():
    """An optimistic u32 decode leaves the slot's bytes_off words implicit: the element lies at the
    record's end plus a constant (the setup of tests/test_implicit_off_gpu.py)."""
    from tests.test_implicit_off_gpu import Run, new_decoder

    arrs = arrays("int16", 12, 600, 8)
    payloads = [writer.encode_example([("label", "int64_list", [i % 1000]), ("t", "bytes_list", [a.tobytes()])])
                for i, a in enumerate(arrs)]
    buf, st, en = synth.framed(payloads)
    d = new_decoder((buf, st, en))
    try:
        run = Run(d, buf, st, en, "u32")
        sp = W.Raw("t", src="int16", out="bfloat16", shape=(12,), scale=SCALE[0], bias=BIAS[0])
        check(d, sp, [[a.tobytes()] for a in arrs], rows=[599, 0, 7, 7, 300, 600])
        assert int(run.info().implicit_off_slots) != 0
    finally:
        d.close()


def test_refusals_leave_the_outputs_alone(dec):
    import torch

    elems = [[a.tobytes()] for a in arrays("uint8", 32, 4, 9)]
    dec.decode(*write(elems))
    good = W.Raw("t", shape=(32,))
    big, view = poisoned(good, 4)
    slot = W.D.resolve_slot(dec, good)
    rows = torch.arange(4, device=dev())

    def call(n_specs=1, rows_dtype=N.ROWS_I64, m=4, d=dec, **over):
        a = (N.TfrgRawSpec * 17)()
        for s in a:
            s.slot, s.src, s.out, s.count, s.channels, s.out_ptr = slot, N.RAW_U8, N.RAW_OUT_F32, 32, 1, view.data_ptr()
            for k, v in over.items():
                setattr(s, k, v)
        rc = d._lib.tfrg_result_raw_rows(d._ctx, a, n_specs, C.c_void_p(rows.data_ptr()), rows_dtype, m, 0, None, None, None)
        assert rc == -1 and b"tfrg_result_raw_rows" in d._lib.tfrg_last_error()

    fresh = hip.HipDecoder(0)
    call(d=fresh)  # no result
    fresh.close()
    label = dec.keys.slots[(dec.keys.key_ids[b"label"], 3)]
    for kw in (dict(n_specs=0), dict(n_specs=17), dict(slot=label), dict(slot=1 << 20), dict(src=8), dict(out=4),
               dict(count=0), dict(count=(1 << 24) + 1), dict(channels=0), dict(channels=17), dict(count=32, channels=3),
               dict(out_ptr=None), dict(out_ptr=view.data_ptr() + 2), dict(reserved=1), dict(rows_dtype=2), dict(m=1 << 31)):
        call(**kw)
    torch.cuda.synchronize()
    assert (big.cpu().numpy() == POISON).all()


def test_shard_decoder_two_batches_one_shuffled_list():
    import torch

    arrs = arrays("uint8", 5 * 7 * 3, 64, 10)
    elems = [[a.tobytes()] for a in arrs]
    buf, st, en = write(elems)
    sd = shard.ShardDecoder(0, int(buf.size) // 2 + 64, 2, balanced=False)
    try:
        plan = sd.plan(st, en, int(buf.size))
        assert len(plan) == 2
        rst, ren = sd.rebase(plan, st, en)
        d_bytes = torch.zeros(((buf.size + 15) // 16) * 16 + 16, dtype=torch.uint8, device=dev())
        d_bytes[: buf.size].copy_(torch.from_numpy(buf.copy()))
        d_st, d_en = torch.from_numpy(rst.view(np.int64)).to(dev()), torch.from_numpy(ren.view(np.int64)).to(dev())
        sd.learn(plan, buf, st, en)
        sd.decode_device(plan, d_bytes.data_ptr(), d_st.data_ptr(), d_en.data_ptr())
        sp = W.Raw("t", out="bfloat16", shape=(5, 7, 3), channels=3, planar=True, scale=SCALE[:3], bias=BIAS[:3])
        rows = np.random.default_rng(0).permutation(64)[:40].tolist() + [64]
        got = check(None, sp, elems, rows=rows, run=lambda **kw: sd.raw(plan, [sp], **kw))
        assert tuple(got["t"].shape) == (41, 3, 5, 7) and got["t"].dtype == torch.bfloat16
    finally:
        sd.close()
