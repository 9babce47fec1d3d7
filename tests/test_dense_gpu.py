"""Dense device tensors (tfrg_result_dense / k_dense): ``HipDecoder.dense`` must equal
``BatchResult.dense`` -- the numpy densifier over the same decode's fetched columns, itself checked
against the oracle in tests/test_dense_host.py -- bit for bit (floats as uint32), with its lengths
and counters, and the generator's truth where the generator knows it."""

import ctypes as C

import numpy as np
import pytest

from tfr_reader import _native as N
from tfr_reader import dense as D
from tfr_reader import hip, shard, synth, writer

pytestmark = pytest.mark.gpu

QNAN = np.array(0x7FC01234, np.uint32).view(np.float32)
COLS = ("status", "aux", "verdict", "order", "row_splits", "i64", "f32", "bytes_off", "bytes_len", "slot_base")


def bits(a) -> np.ndarray:
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def same(got: D.DenseBatch, ref: D.DenseBatch, specs) -> None:
    for sp in specs:
        k = sp.out_name
        assert tuple(got[k].shape) == ref[k].shape, k
        assert np.array_equal(bits(got[k]), bits(ref[k])), k
        assert (k in got.lengths) == bool(sp.lengths)
        if sp.lengths:
            assert np.array_equal(got.lengths[k].cpu().numpy(), ref.lengths[k]), k
        assert got.stats[k].tolist() == ref.stats[k].tolist(), (k, got.stats[k], ref.stats[k])


def both(dec, res, specs, **kw):
    got, ref = dec.dense(specs, **kw), res.dense(specs)
    same(got, ref, specs)
    return got, ref


@pytest.fixture
def dec(monkeypatch):
    monkeypatch.setenv("TFRG_OPTIMISTIC", "1")  # (read at context creation; the suite may run with 0)
    monkeypatch.setenv("TFRG_TEMPLATES", "1")
    d = hip.HipDecoder(0)
    yield d
    d.close()


C1_SPECS = [
    D.Dense("label", "int64", lengths=True),
    D.Dense("label", "int32", name="l32"),
    D.Dense("label", "int64", 3, fill=-1, name="l3", lengths=True),
    D.Dense("label", "int32", 3, fill=-7, name="l32x3"),
    D.Dense("id", "uint8", 12, lengths=True),
    D.Dense("id", "uint8", 16, fill=0x20, name="id16", lengths=True),
    D.Dense("id", "uint8", 8, name="id8"),
]


def check_c1_truth(got, n: int) -> None:
    assert got["label"][:, 0].cpu().tolist() == [i % 1000 for i in range(n)]
    assert got["l32x3"].cpu().tolist() == [[i % 1000, -7, -7] for i in range(n)]
    ids = got["id"].cpu().numpy()
    id16 = got["id16"].cpu().numpy()
    id8 = got["id8"].cpu().numpy()
    for i in (0, 1, 63, 64, n // 2, n - 1):
        assert bytes(ids[i]) == b"img-%08d" % i
        assert bytes(id16[i]) == b"img-%08d    " % i
        assert bytes(id8[i]) == (b"img-%08d" % i)[:8]
    assert (got.lengths["id"].cpu().numpy() == 12).all() and (got.lengths["l3"].cpu().numpy() == 1).all()
    assert got.stats["id"].tolist() == [0, 0, 0, 0] and got.stats["id8"].tolist() == [n, 0, 0, 0]
    assert got.stats["id16"].tolist() == [0, n, 0, 0] and got.stats["l3"].tolist() == [0, n, 0, 0]


def d2h(ptr, count: int, dtype) -> np.ndarray:
    import torch

    host = np.zeros(count, dtype)
    rt = C.CDLL("libamdhip64.so")
    torch.cuda.synchronize()
    assert rt.hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(C.cast(ptr, C.c_void_p).value),
                        C.c_size_t(host.nbytes), 2) == 0
    return host


def test_c1_optimistic_placed_and_implicit_columns(dec):
    n = 5000
    buf, st, en = synth.framed(synth.c1_payloads(n))
    res = dec.decode(buf, st, en)
    assert int(res.info.implicit_cols) == 7 and int(res.info.placed_slots) & 3 == 3
    got, _ = both(dec, res, C1_SPECS, strict=False)
    check_c1_truth(got, n)
    dec.dense([D.Dense("label", "int64"), D.Dense("id", "uint8", 12)], strict=True)  # FixedLenFeature shapes
    with pytest.raises(ValueError, match="'id'"):
        dec.dense([D.Dense("id", "uint8", 16)], strict=True)
    # the full view is still there, from the device and through a fetch
    cols = dec.device_columns()
    S = len(res.slot_key)
    assert np.array_equal(d2h(cols.row_splits, S * (n + 1), np.uint32).reshape(S, n + 1), res.row_splits)
    assert np.array_equal(d2h(cols.bytes_len, n, np.uint32), res.bytes_len)
    assert np.array_equal(d2h(cols.status, n, np.int32), res.status)
    again = dec._fetch(buf, st, en, dec.info(), False)
    for k in COLS:
        assert np.array_equal(getattr(again, k), getattr(res, k)), k
    both(dec, res, C1_SPECS)  # and once more over the completed columns


@pytest.mark.parametrize("env", [{"TFRG_TEMPLATES": "0"}, {"TFRG_TEMPLATES": "0", "TFRG_SPEC": "0"},
                                 {"TFRG_OPTIMISTIC": "0"}, {"TFRG_DENSE_NT": "1"}])
def test_c1_other_decode_paths(monkeypatch, env):
    monkeypatch.setenv("TFRG_OPTIMISTIC", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = hip.HipDecoder(0)
    try:
        n = 5000
        buf, st, en = synth.framed(synth.c1_payloads(n))
        res = d.decode(buf, st, en)
        if "TFRG_SPEC" in env:
            assert int(res.info.placed_slots) == 0  # every row split read
        got, _ = both(d, res, C1_SPECS)
        check_c1_truth(got, n)
    finally:
        d.close()


def test_variable_length_ids(dec):
    blob, offs = synth.c1v_blob(3000, 0, 11)
    buf = synth.frame_blob(blob, offs)
    en = (np.diff(offs) + 16).cumsum().astype(np.uint64)
    st = en - (np.diff(offs) + 16).astype(np.uint64)
    res = dec.decode(buf, st, en)
    specs = [D.Dense("id", "uint8", 12, fill=0xFF, lengths=True), D.Dense("id", "uint8", 7, name="id7", lengths=True),
             D.Dense("label", "int64")]
    got, ref = both(dec, res, specs)
    lens = got.lengths["id"].cpu().numpy()
    assert lens.min() == 5 and lens.max() == 12 and np.array_equal(lens, ref.lengths["id7"])
    ids = synth.c1v_ids(3000, 11)
    out = got["id"].cpu().numpy()
    for i in (0, 1, 77, 2999):
        want = b"img-%d" % int(ids[i])
        assert bytes(out[i, : len(want)]) == want and (out[i, len(want):] == 0xFF).all()
    assert int(got.stats["id7"][0]) > 0 and int(got.stats["id7"][1]) > 0


def test_c3_all_slots_in_one_call(dec):
    n = 256
    buf, st, en = synth.framed(synth.c3_payloads(n, max_len=64))
    res = dec.decode(buf, st, en)
    ints = [k for k, kd in zip(res.slot_key, res.slot_kind) if kd == 3]
    flts = [k for k, kd in zip(res.slot_key, res.slot_kind) if kd == 2]
    assert len(ints) == 32 and len(flts) == 32
    specs = [D.Dense(k, "int64", 64, fill=-1, lengths=True) for k in ints]
    specs += [D.Dense(k, "float32", 64, fill=QNAN, lengths=True) for k in flts]
    assert len(specs) == N.DENSE_MAX_SPECS
    both(dec, res, specs)
    for w in (17, 1):
        specs = [D.Dense(ints[0], "int64", w, fill=-1, lengths=True), D.Dense(ints[5], "int32", w, fill=-1),
                 D.Dense(flts[0], "float32", w, fill=QNAN, lengths=True), D.Dense(flts[31], "float32", w, fill=QNAN)]
        _, ref = both(dec, res, specs)
    st17 = res.dense([D.Dense(k, "int64", 17) for k in ints[:8]]).stats
    assert sum(int(v[0]) for v in st17.values()) > 0 and sum(int(v[2]) for v in st17.values()) > 0  # truncated, empty


def _mixed(n: int) -> list[bytes]:
    recs = []
    for i in range(n):
        ent = []
        if i % 2:
            ent.append(("half", "int64_list", [i, -i]))
        ent.append(("empty", "float_list", [] if i % 3 else [1.5, 2.5, 3.5]))
        ent.append(("two", "int64_list" if i % 4 else "float_list", [7] if i % 4 else [0.25]))
        ent.append(("names", "bytes_list", [b"a" * (i % 7), b"second"][: 1 + (i % 5 == 0)] if i % 6 else []))
        recs.append(writer.encode_example(ent))
    return recs


def test_missing_keys_absent_key_and_two_kinds(dec):
    buf, st, en = synth.framed(_mixed(333))
    res = dec.decode(buf, st, en)
    specs = [
        D.Dense("half", "int64", 2, fill=-9, lengths=True),
        D.Dense("empty", "float32", 3, fill=QNAN, lengths=True),
        D.Dense("two", "int64", 1, fill=-1, name="two_i", lengths=True),
        D.Dense("two", "float32", 1, fill=-1.0, name="two_f", lengths=True),
        D.Dense("names", "uint8", 4, fill=0xEE, lengths=True),
        D.Dense("names", "uint8", 5, name="names5"),
        D.Dense("absent", "int64", 2, fill=3, lengths=True),
        D.Dense("absent", "float32", 2, fill=QNAN, name="absent_f"),
    ]
    got, _ = both(dec, res, specs)
    assert (got["absent"] == 3).all() and not got.lengths["absent"].any()
    assert got.stats["absent"].tolist() == [0, 333, 333, 0] and int(got.stats["names"][3]) > 0
    assert got["two_i"][:, 0].cpu().tolist() == [7 if i % 4 else -1 for i in range(333)]
    with pytest.raises(KeyError):
        dec.dense([D.Dense("absent", "int64")], strict=True)


def test_record_errors(dec):
    n = 300
    pl = synth.c1_payloads(n)
    bad = [3, 64, 127, 200, 299]
    for i in bad:
        pl[i] = bytes([0x0F]) + pl[i][1:]  # an unsupported wire type at the top level
    buf, st, en = synth.framed(pl)
    res = dec.decode(buf, st, en)
    assert int(res.info.n_errors) == 5 and np.flatnonzero(res.status).tolist() == bad
    specs = [D.Dense("label", "int64", fill=-1, lengths=True), D.Dense("id", "uint8", 12, fill=0x2A, lengths=True)]
    got, _ = both(dec, res, specs)
    lab, ids = got["label"].cpu().numpy(), got["id"].cpu().numpy()
    for i in bad:
        assert lab[i, 0] == -1 and (ids[i] == 0x2A).all()
        assert int(got.lengths["label"][i]) == 0 and int(got.lengths["id"][i]) == 0
    want = res.error(bad[0])
    with pytest.raises(type(want)) as ei:
        dec.dense(specs, strict=True)
    assert str(ei.value) == str(want)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_edge_sizes(dec, n):
    # bare payloads: the last record's id ends exactly at nbytes
    pl = synth.c1_payloads(n)
    lens = np.array([len(p) for p in pl], np.uint64)
    en = np.cumsum(lens, dtype=np.uint64)
    buf = np.frombuffer(b"".join(pl), np.uint8)
    res = dec.decode(buf, en - lens, en, payload_only=True)
    specs = [D.Dense("label", "int64", lengths=True), D.Dense("label", "int32", 3, fill=-1, name="l3"),
             D.Dense("id", "uint8", 5, name="id5", lengths=True), D.Dense("id", "uint8", 12),
             D.Dense("id", "uint8", 13, fill=0x11, name="id13"), D.Dense("id", "uint8", 20, fill=0x11, name="id20")]
    got, _ = both(dec, res, specs)
    assert tuple(got["id5"].shape) == (n, 5)
    if n:
        assert bytes(got["id"][n - 1].cpu().numpy()) == b"img-%08d" % (n - 1)
        assert int(res.bytes_off[n - 1]) + 12 == buf.size


def test_materialized_bytes_equal_the_views(dec):
    blob, offs = synth.c1v_blob(1000, 0, 5)
    buf = synth.frame_blob(blob, offs)
    en = (np.diff(offs) + 16).cumsum().astype(np.uint64)
    st = en - (np.diff(offs) + 16).astype(np.uint64)
    specs = [D.Dense("id", "uint8", 12, fill=0xFF, lengths=True), D.Dense("id", "uint8", 6, name="id6")]
    res = dec.decode(buf, st, en)
    views, _ = both(dec, res, specs)
    views = {k: bits(v) for k, v in views.items()}
    res = dec.decode(buf, st, en, materialize_bytes=True)
    assert res.bytes_data is not None
    mat, _ = both(dec, res, specs)
    for k in views:
        assert np.array_equal(bits(mat[k]), views[k]), k


def test_canaries_and_unaligned_outputs(dec):
    """Outputs carved from one buffer filled with 0xA5, at 16-byte aligned bases and at bases that are
    only element aligned (the element-granular loops): the 256 bytes before and after every region
    stay as they were."""
    import torch

    n = 257
    buf, st, en = synth.framed(synth.c1_payloads(n))
    res = dec.decode(buf, st, en)
    dev = torch.device("cuda", 0)
    tdt = {"int64": torch.int64, "int32": torch.int32, "uint8": torch.uint8}
    for shift in (0, 1):
        specs = [D.Dense("label", "int64", lengths=True), D.Dense("label", "int32", 3, fill=-1, name="l3", lengths=True),
                 D.Dense("id", "uint8", 12, lengths=True), D.Dense("id", "uint8", 5, name="id5", lengths=True),
                 D.Dense("id", "uint8", 8, name="id8")]
        big = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device=dev)
        at, out, regions = 256, {}, []

        def carve(nbytes: int, align: int) -> int:
            nonlocal at
            lo = (at + 15) // 16 * 16 + (align if shift else 0)
            regions.append((lo, lo + nbytes))
            at = lo + nbytes + 256
            return lo

        for sp in specs:
            isz = np.dtype(D.DTYPES[sp.dtype][2]).itemsize
            lo = carve(n * sp.width * isz, isz)
            t = big[lo : lo + n * sp.width * isz].view(tdt[sp.dtype]).view(n, sp.width)
            ll = carve(4 * n, 4)
            out[sp.out_name] = (t, big[ll : ll + 4 * n].view(torch.int32)) if sp.lengths else t
        got, _ = both(dec, res, specs, out=out)
        assert got["id"].data_ptr() == out["id"][0].data_ptr()
        host = big.cpu().numpy()
        for lo, hi in regions:
            assert (host[lo - 256 : lo] == 0xA5).all() and (host[hi : hi + 256] == 0xA5).all(), (shift, lo, hi)


def test_raw_pointer_outputs(dec):
    """``out=`` as raw device pointers (callers without torch): same bytes as the torch path, ordered
    with the stream whose handle is passed."""
    import torch

    n = 1000
    buf, st, en = synth.framed(synth.c1_payloads(n))
    res = dec.decode(buf, st, en)
    specs = [D.Dense("label", "int32", 2, fill=-3, lengths=True), D.Dense("id", "uint8", 12)]
    ref = res.dense(specs)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        lab = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        lens = torch.zeros(n, dtype=torch.int32, device=dev)
        ids = torch.zeros((n, 12), dtype=torch.uint8, device=dev)
        got = dec.dense(specs, out={"label": (lab.data_ptr(), lens.data_ptr()), "id": ids.data_ptr()}, stream=s.cuda_stream)
        total = int(lab.sum())  # on s, which waits for the collate
    assert got["label"] == lab.data_ptr() and got.lengths["label"] == lens.data_ptr() and got.stats == {}
    assert total == int(ref["label"].sum())
    assert np.array_equal(lab.cpu().numpy(), ref["label"]) and np.array_equal(ids.cpu().numpy(), ref["id"])
    assert np.array_equal(lens.cpu().numpy(), ref.lengths["label"])


def test_shard_dense_over_batches_and_streams(dec):
    import torch

    imgs = [synth.c4_file(f, "c1", base=2500) for f in range(3)]
    sb = shard.ShardBatch([synth.c4_file_name(f) for f in range(3)], imgs)
    truth = dec.decode(sb.buf, sb.starts, sb.ends)
    specs = [D.Dense("label", "int64", lengths=True), D.Dense("id", "uint8", 12, lengths=True),
             D.Dense("nope", "int32", 2, fill=-1)]
    ref = truth.dense(specs)
    sd = shard.ShardDecoder(0, batch_bytes=sb.nbytes // 3 + 4096, n_streams=2)
    try:
        plan = sd.plan(sb.starts, sb.ends, sb.nbytes)
        assert len(plan) >= 3
        dev = torch.device("cuda", 0)
        d_bytes = torch.zeros(((sb.nbytes + 15) // 16) * 16 + 16, dtype=torch.uint8, device=dev)
        d_bytes[: sb.nbytes].copy_(torch.from_numpy(sb.buf))
        rst, ren, firsts = sd.rebase32(plan, sb.starts, sb.ends)
        assert rst is None
        d_en = torch.from_numpy(ren.view(np.int32)).to(dev)
        sd.learn(plan, sb.buf, sb.starts, sb.ends)
        streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
        torch.cuda.synchronize(dev)
        sd.decode_device32(plan, d_bytes.data_ptr(), None, d_en.data_ptr(), firsts, streams=[s.cuda_stream for s in streams])
        got = sd.dense(plan, specs)
        total = int(got["label"].sum())  # consumed at once, on the current stream
        assert total == int(ref["label"].sum())
        same(got, ref, specs)
    finally:
        sd.close()


def test_load_tensors_in_selection_order(tmp_path):
    import tfr_reader as tfr

    synth.write_c4_dir(tmp_path, 3, "c1", base=200)
    ds = tfr.TFRecordDatasetReader.build_index_from_dataset_dir(str(tmp_path))
    n = len(ds)
    rng = np.random.default_rng(4)
    pick = rng.integers(0, n, 500)  # permuted, with repeats
    from tfr_reader import _frame as F

    c = F.columns(ds.index_df, ["tfrecord_filename", "tfrecord_start", "tfrecord_end"])
    sel = F.make_frame({k: [c[k][i] for i in pick.tolist()] for k in c})
    feats = ds.load_records(sel)
    specs = [D.Dense("label", "int64", lengths=True), D.Dense("id", "uint8", 12)]
    got = ds.load_tensors(sel, specs)
    assert got["label"][:, 0].cpu().tolist() == [f["label"].value[0] for f in feats]
    ids = got["id"].cpu().numpy()
    assert [bytes(r) for r in ids] == [f["id"].value[0] for f in feats]
    assert got.stats["id"].tolist() == [0, 0, 0, 0]


def test_argument_errors_leave_the_context_usable(dec):
    import torch

    n = 100
    buf, st, en = synth.framed(synth.c1_payloads(n))
    lib = N.lib()
    out = torch.zeros(n * 16, dtype=torch.uint8, device=torch.device("cuda", 0))
    stats = torch.zeros(8, dtype=torch.int32, device=out.device)

    def call(ctx=None, k=1, **kw):
        f = dict(slot=0, dtype=N.DENSE_I64, width=1, reserved=0, fill=0, out=out.data_ptr(), lengths=None)
        f.update(kw)
        arr = (N.TfrgDenseSpec * max(k, 1))(*[N.TfrgDenseSpec(**f) for _ in range(max(k, 1))])
        return lib.tfrg_result_dense(dec._ctx if ctx is None else ctx, arr, k, C.c_void_p(stats.data_ptr()), None)

    assert call() == -1 and b"no result" in lib.tfrg_last_error()
    res = dec.decode(buf, st, en)
    s_label = res.slot_key.index("label")
    s_id = res.slot_key.index("id")
    assert call(slot=s_label) == 0
    for bad in (dict(k=0), dict(k=65), dict(slot=len(res.slot_key)), dict(slot=s_label, dtype=N.DENSE_F32),
                dict(slot=s_label, dtype=N.DENSE_U8), dict(slot=s_id, dtype=N.DENSE_I32), dict(slot=s_label, dtype=4),
                dict(slot=s_label, width=0), dict(slot=s_label, width=4097), dict(slot=s_label, out=None),
                dict(slot=s_label, reserved=1)):
        assert call(**bad) == -1, bad
        assert lib.tfrg_last_error().startswith(b"tfrg_result_dense"), bad
        both(dec, res, [D.Dense("label", "int64", lengths=True), D.Dense("id", "uint8", 12)])
