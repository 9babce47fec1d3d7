"""Row-selected dense device tensors (tfrg_result_dense_rows / k_dense_rows): ``dense(rows=r)``
must equal the numpy reference -- ``BatchResult.dense`` over the same decode's fetched columns,
indexed by ``r`` (tests/test_dense_rows_host.py shows that this is ``densify(rows=r)``) -- bit for bit
(floats as uint32), with its lengths, its counters and ``skipped``; rows whose index is out of range
keep what the output held; and the generator's truth where the generator knows it."""

import ctypes as C

import numpy as np
import pytest

from tests.test_dense_rows_host import MIXED_SPECS, bits, counters, mixed, per_record
from tfr_reader import _native as N
from tfr_reader import dense as D
from tfr_reader import hip, shard, synth

pytestmark = pytest.mark.gpu

QNAN = np.array(0x7FC01234, np.uint32).view(np.float32)
COLS = ("status", "aux", "verdict", "order", "row_splits", "i64", "f32", "bytes_off", "bytes_len", "slot_base")
POISON = 0xA5
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

C1_SPECS = [
    D.Dense("label", "int64", lengths=True),
    D.Dense("label", "int32", name="l32"),
    D.Dense("label", "int64", 3, fill=-1, name="l3", lengths=True),
    D.Dense("label", "int32", 3, fill=-7, name="l32x3"),
    D.Dense("id", "uint8", 12, lengths=True),
    D.Dense("id", "uint8", 16, fill=0x20, name="id16", lengths=True),
    D.Dense("id", "uint8", 8, name="id8"),
]
# rows that share a 16-byte unit (row sizes 4, 8, 12, 3, 5, 12 bytes) and rows that are whole units
UNIT_SPECS = [
    D.Dense("label", "int32", 1, name="i32w1", lengths=True),
    D.Dense("label", "int64", 1, name="i64w1", lengths=True),
    D.Dense("label", "int32", 3, fill=-7, name="i32w3", lengths=True),
    D.Dense("id", "uint8", 3, name="u8w3", lengths=True),
    D.Dense("id", "uint8", 5, name="u8w5", lengths=True),
    D.Dense("id", "uint8", 12, name="u8w12", lengths=True),
    D.Dense("id", "uint8", 16, fill=0x20, name="u8w16", lengths=True),
    D.Dense("label", "int64", 2, fill=-1, name="i64w2", lengths=True),
]


def dev():
    import torch

    return torch.device("cuda", 0)


def to_dev(rows, dtype=np.int64):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(rows, dtype))).to(dev())


def poisoned(specs, m: int) -> dict:
    """out= for ``specs`` with m rows, every byte 0xA5 (lengths for every spec that has them)."""
    import torch

    tdt = {"int64": torch.int64, "int32": torch.int32, "float32": torch.float32, "uint8": torch.uint8}
    out = {}
    for sp in specs:
        isz = np.dtype(D.DTYPES[sp.dtype][2]).itemsize
        t = torch.full((m * sp.width * isz,), POISON, dtype=torch.uint8, device=dev()).view(tdt[sp.dtype]).view(m, sp.width)
        lens = torch.full((4 * m,), POISON, dtype=torch.uint8, device=dev()).view(torch.int32)
        out[sp.out_name] = (t, lens) if sp.lengths else t
    return out


class Ref:
    """The full host reference of one decode, computed once and indexed per row list."""

    def __init__(self, res, specs) -> None:
        self.res, self.specs, self.n = res, specs, len(res)
        self.full = res.dense([D.Dense(s.key, s.dtype, s.width, s.fill, True, s.out_name) for s in specs])
        self.flags = {s.out_name: per_record(res, s) for s in specs}

    def check(self, got: D.DenseBatch, rows, row0: int = 0) -> int:
        """``got`` (made over outputs prefilled with 0xA5) against the reference for ``rows`` (Python
        ints or an array); returns how many rows are out of range."""
        rows = [int(v) for v in np.asarray(rows).reshape(-1).tolist()] if not isinstance(rows, list) else rows
        ok = np.array([row0 <= v < row0 + self.n for v in rows], bool)
        idx = np.array([v - row0 if o else 0 for v, o in zip(rows, ok.tolist())], np.int64)
        for sp in self.specs:
            k = sp.out_name
            want = bits(self.full[k])[idx] if len(rows) else bits(self.full[k])[:0]
            have = bits(got[k])
            assert have.shape == (len(rows), sp.width), k
            assert np.array_equal(have[ok], want[ok]), k
            assert (have[~ok].view(np.uint8) == POISON).all(), k
            lens = self.full.lengths[k][idx]
            if sp.lengths:
                gl = got.lengths[k].cpu().numpy()
                assert np.array_equal(gl[ok], lens[ok]), k
                assert (gl[~ok].view(np.uint8) == POISON).all(), k
            empty, multi = self.flags[k]
            assert got.stats[k].tolist() == counters(lens[ok], sp.width, multi[idx][ok], empty[idx][ok]), k
        bad = int((~ok).sum())
        assert got.skipped == bad
        return bad


def run(dec, ref: Ref, rows, dtype=np.int64, **kw) -> D.DenseBatch:
    """dense(rows=) over poisoned outputs, checked against the reference."""
    got = dec.dense(ref.specs, rows=to_dev(rows, dtype), out=poisoned(ref.specs, len(rows)), **kw)
    host = D.DenseBatch({k: v.cpu().numpy() for k, v in got.items()}, got.lengths, got.stats, got.skipped)
    ref.check(host, rows)
    return got


def new_decoder(env: dict | None = None):
    mp = pytest.MonkeyPatch()
    mp.setenv("TFRG_OPTIMISTIC", "1")  # (read at context creation; the suite may run with 0)
    mp.setenv("TFRG_TEMPLATES", "1")
    for k, v in (env or {}).items():
        mp.setenv(k, v)
    try:
        return hip.HipDecoder(0)
    finally:
        mp.undo()


N1 = 5000


@pytest.fixture(scope="module")
def c1():
    """One optimistic C1 decode of 5000 records (placed slots, implicit bytes_len), kept for the
    tests that only draw rows from it: (decoder, fetched result, buf, starts, ends)."""
    d = new_decoder()
    buf, st, en = synth.framed(synth.c1_payloads(N1))
    res = d.decode(buf, st, en)
    assert int(res.info.implicit_cols) == 7 and int(res.info.placed_slots) & 3 == 3
    yield d, res, (buf, st, en)
    d.close()


@pytest.fixture(scope="module")
def c1_ref(c1):
    return Ref(c1[1], C1_SPECS)


@pytest.fixture
def dec():
    d = new_decoder()
    yield d
    d.close()


# ------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_identity_rows_equal_plain_dense(c1, c1_ref, dtype):
    d = c1[0]
    plain = d.dense(C1_SPECS)
    got = run(d, c1_ref, np.arange(N1), dtype)
    for sp in C1_SPECS:
        k = sp.out_name
        assert np.array_equal(bits(got[k].cpu().numpy()), bits(plain[k].cpu().numpy())), k
        if sp.lengths:
            assert np.array_equal(got.lengths[k].cpu().numpy(), plain.lengths[k].cpu().numpy()), k
        assert got.stats[k].tolist() == plain.stats[k].tolist(), k
    assert got["label"][:, 0].cpu().tolist() == [i % 1000 for i in range(N1)]
    ids = got["id"].cpu().numpy()
    for i in (0, 1, 63, 64, N1 // 2, N1 - 1):
        assert bytes(ids[i]) == b"img-%08d" % i


# ------------------------------------------------------------------------------------ 2. row-list shapes
def row_list(pattern: str, m: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(m)
    if pattern == "permutation":  # (of the first rows where m < n, wrapped where m > n)
        return rng.permutation(max(m, n))[:m] % n
    if pattern == "reversed":
        return (n - 1 - np.arange(m)) % n
    if pattern == "one":
        return np.full(m, n - 3)
    return rng.integers(0, n, m)


@pytest.mark.parametrize("pattern", ["permutation", "reversed", "one", "random"])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1023, 4097, 3 * N1])
def test_row_list_shapes(c1, c1_ref, m, pattern):
    rows = row_list(pattern, m, N1)
    got = run(c1[0], c1_ref, rows, np.int32 if m % 2 else np.int64)
    assert got["label"][:, 0].cpu().tolist() == (rows % 1000).tolist()  # the generator's truth
    ids = got["id"].cpu().numpy()
    for k in {0, m // 2, m - 1}:
        assert bytes(ids[k]) == b"img-%08d" % rows[k]


def test_host_row_lists_are_checked_and_uploaded(c1, c1_ref):
    d = c1[0]
    rows = [4999, 0, 0, 17]
    got = d.dense(C1_SPECS, rows=rows, out=poisoned(C1_SPECS, 4), strict=False)
    c1_ref.check(D.DenseBatch({k: v.cpu().numpy() for k, v in got.items()}, got.lengths, got.stats, got.skipped), rows)
    assert tuple(d.dense(C1_SPECS, rows=[])["id"].shape) == (0, 12)
    with pytest.raises(IndexError, match=r"rows\[1\] = 5000 "):
        d.dense(C1_SPECS, rows=np.array([0, N1]))
    with pytest.raises(IndexError, match=r"rows\[0\] = -1 "):
        d.dense(C1_SPECS, rows=[-1])


def test_row_lists_that_are_refused(c1):
    import torch

    d = c1[0]
    good = to_dev(np.arange(8))
    for bad, exc in ((good.to(torch.float32), TypeError), (good.view(2, 4), ValueError), (to_dev(np.arange(16))[::2], ValueError),
                     (good.cpu(), ValueError), ([0.5, 1.0], ValueError), ([[0, 1], [2, 3]], ValueError)):
        with pytest.raises(exc):
            d.dense(C1_SPECS, rows=bad)
    with pytest.raises((TypeError, ValueError)):
        d.dense(C1_SPECS, rows="0123")


# ------------------------------------------------------------------------------------ 3. other decode paths
def some_rows(n: int) -> list[np.ndarray]:
    rng = np.random.default_rng(n)
    return [rng.permutation(n), rng.integers(0, n, 2 * n + 5), np.full(70, n - 1)]


@pytest.mark.parametrize("env", [{"TFRG_TEMPLATES": "0"}, {"TFRG_OPTIMISTIC": "0"}])
def test_c1_decode_paths_that_store_row_splits(c1, env):
    d = new_decoder(env)
    try:
        res = d.decode(*c1[2])
        ref = Ref(res, C1_SPECS)
        for rows in some_rows(N1)[:2]:
            run(d, ref, rows)
    finally:
        d.close()


def test_variable_length_ids(dec):
    n = 3000
    blob, offs = synth.c1v_blob(n, 0, 11)
    buf = synth.frame_blob(blob, offs)
    en = (np.diff(offs) + 16).cumsum().astype(np.uint64)
    st = en - (np.diff(offs) + 16).astype(np.uint64)
    res = dec.decode(buf, st, en)
    specs = [D.Dense("id", "uint8", 12, fill=0xFF, lengths=True), D.Dense("id", "uint8", 7, name="id7", lengths=True),
             D.Dense("label", "int64")]
    ref = Ref(res, specs)
    ids = synth.c1v_ids(n, 11)
    for rows in some_rows(n):
        got = run(dec, ref, rows)
        out = got["id"].cpu().numpy()
        for k in (0, 1, len(rows) - 1):
            want = b"img-%d" % int(ids[rows[k]])
            assert bytes(out[k, : len(want)]) == want and (out[k, len(want):] == 0xFF).all()


def test_missing_keys_empty_lists_and_two_kinds(dec):
    res = dec.decode(*synth.framed(mixed(333)))
    specs = [*MIXED_SPECS, D.Dense("absent", "float32", 2, fill=QNAN, name="absent_f")]
    ref = Ref(res, specs)
    for rows in some_rows(333):
        got = run(dec, ref, rows)
        assert got.stats["absent"].tolist() == [0, len(rows), len(rows), 0]
        assert got["two_i"][:, 0].cpu().tolist() == [7 if i % 4 else -1 for i in rows.tolist()]
    with pytest.raises(KeyError):
        dec.dense([D.Dense("absent", "int64")], rows=to_dev([0]), strict=True)


def test_c3_all_slots_in_one_call(dec):
    n = 256
    res = dec.decode(*synth.framed(synth.c3_payloads(n, max_len=64)))
    ints = [k for k, kd in zip(res.slot_key, res.slot_kind) if kd == 3]
    flts = [k for k, kd in zip(res.slot_key, res.slot_kind) if kd == 2]
    assert len(ints) == 32 and len(flts) == 32
    specs = [D.Dense(k, "int64", 64, fill=-1, lengths=True) for k in ints]
    specs += [D.Dense(k, "float32", 64, fill=QNAN, lengths=True) for k in flts]
    assert len(specs) == N.DENSE_MAX_SPECS
    rows = some_rows(n)
    ref = Ref(res, specs)
    run(dec, ref, rows[0])
    run(dec, ref, rows[1])
    for w in (17, 1):
        specs = [D.Dense(ints[0], "int64", w, fill=-1, lengths=True), D.Dense(ints[5], "int32", w, fill=-1),
                 D.Dense(flts[0], "float32", w, fill=QNAN, lengths=True), D.Dense(flts[31], "float32", w, fill=QNAN)]
        ref = Ref(res, specs)
        for r in rows:
            run(dec, ref, r)


def test_materialized_bytes_equal_the_views(dec):
    n = 1000
    blob, offs = synth.c1v_blob(n, 0, 5)
    buf = synth.frame_blob(blob, offs)
    en = (np.diff(offs) + 16).cumsum().astype(np.uint64)
    st = en - (np.diff(offs) + 16).astype(np.uint64)
    specs = [D.Dense("id", "uint8", 12, fill=0xFF, lengths=True), D.Dense("id", "uint8", 6, name="id6")]
    rows = some_rows(n)[1]
    res = dec.decode(buf, st, en)
    views = run(dec, Ref(res, specs), rows)
    views = {k: v.cpu().numpy() for k, v in views.items()}
    res = dec.decode(buf, st, en, materialize_bytes=True)
    assert res.bytes_data is not None
    mat = run(dec, Ref(res, specs), rows)
    for k in views:
        assert np.array_equal(mat[k].cpu().numpy(), views[k]), k


# ------------------------------------------------------------------------------------ 4. skipped rows
BAD64 = [-1, N1, N1 + 1, (1 << 31) - 1, I64_MIN, I64_MAX, -N1, 1 << 32, (1 << 32) + 5, -(1 << 32)]
BAD32 = [-1, N1, N1 + 1, (1 << 31) - 1, -(1 << 31), -N1]


def with_bad(pattern: str, bad: list[int], m: int) -> list[int]:
    rng = np.random.default_rng(len(bad) + m)
    good = rng.integers(0, N1, m).tolist()
    if pattern == "alternating":
        return [bad[(k // 2) % len(bad)] if k % 2 else good[k] for k in range(m)]
    if pattern == "runs":  # runs of 1..9 bad entries between runs of 1..9 good ones
        out, k = [], 0
        while len(out) < m:
            run_len = 1 + (k * 7) % 9
            out += [bad[(k + j) % len(bad)] for j in range(run_len)] if k % 2 else good[len(out) : len(out) + run_len]
            k += 1
        return out[:m]
    return [bad[k % len(bad)] for k in range(m)]


@pytest.fixture(scope="module")
def unit_ref(c1):
    return Ref(c1[1], UNIT_SPECS)


@pytest.mark.parametrize("pattern", ["alternating", "runs", "all"])
@pytest.mark.parametrize("dtype,bad", [(np.int64, BAD64), (np.int32, BAD32)])
def test_rows_out_of_range_are_skipped(c1, unit_ref, pattern, dtype, bad):
    d = c1[0]
    for m in (1, 2, 3, 1027):
        rows = with_bad(pattern, bad, m)
        got = run(d, unit_ref, rows, dtype)
        if pattern == "all":
            assert got.skipped == m and all(v.tolist() == [0, 0, 0, 0] for v in got.stats.values())
    rows = with_bad(pattern, bad, 40)
    fixed = [UNIT_SPECS[0], UNIT_SPECS[1], UNIT_SPECS[5]]  # (FixedLenFeature shapes: strict has nothing else to raise)
    with pytest.raises(IndexError):
        d.dense(fixed, rows=to_dev(rows, dtype), strict=True)
    d.dense(fixed, rows=to_dev([0, N1 - 1], dtype), strict=True)


# ------------------------------------------------------------------------------------ 5. alignment
def test_canaries_and_unaligned_outputs(c1):
    """Outputs carved from one buffer filled with 0xA5, at 16-byte aligned bases and at bases that are
    only element aligned (the element-granular loops), rows in range and out of it: the 256 bytes
    before and after every region stay as they were."""
    import torch

    d, res = c1[0], c1[1]
    m = 257
    rng = np.random.default_rng(5)
    tdt = {"int64": torch.int64, "int32": torch.int32, "uint8": torch.uint8}
    specs = [D.Dense("label", "int64", lengths=True), D.Dense("label", "int32", 3, fill=-1, name="l3", lengths=True),
             D.Dense("id", "uint8", 12, lengths=True), D.Dense("id", "uint8", 5, name="id5", lengths=True),
             D.Dense("id", "uint8", 8, name="id8")]
    ref = Ref(res, specs)
    for shift in (0, 1):
        for rows in (rng.integers(0, N1, m).tolist(), with_bad("runs", BAD64, m)):
            big = torch.full((1 << 16,), POISON, dtype=torch.uint8, device=dev())
            at, out, regions = 256, {}, []

            def carve(nbytes: int, align: int) -> int:
                nonlocal at
                lo = (at + 15) // 16 * 16 + (align if shift else 0)
                regions.append((lo, lo + nbytes))
                at = lo + nbytes + 256
                return lo

            for sp in specs:
                isz = np.dtype(D.DTYPES[sp.dtype][2]).itemsize
                lo = carve(m * sp.width * isz, isz)
                t = big[lo : lo + m * sp.width * isz].view(tdt[sp.dtype]).view(m, sp.width)
                ll = carve(4 * m, 4)
                out[sp.out_name] = (t, big[ll : ll + 4 * m].view(torch.int32)) if sp.lengths else t
            got = d.dense(specs, rows=to_dev(rows), out=out)
            assert got["id"].data_ptr() == out["id"][0].data_ptr()
            ref.check(D.DenseBatch({k: v.cpu().numpy() for k, v in got.items()}, got.lengths, got.stats, got.skipped), rows)
            host = big.cpu().numpy()
            for lo, hi in regions:
                assert (host[lo - 256 : lo] == POISON).all() and (host[hi : hi + 256] == POISON).all(), (shift, lo, hi)


# ------------------------------------------------------------------------------------ 6. shard
@pytest.fixture(scope="module")
def sharded():
    """Three C1 files decoded by a ShardDecoder in at least 3 batches on 2 streams: (decoder, plan,
    the one-batch truth's result)."""
    import torch

    d = new_decoder()
    imgs = [synth.c4_file(f, "c1", base=2500) for f in range(3)]
    sb = shard.ShardBatch([synth.c4_file_name(f) for f in range(3)], imgs)
    truth = d.decode(sb.buf, sb.starts, sb.ends)
    d.close()
    sd = shard.ShardDecoder(0, batch_bytes=sb.nbytes // 3 + 4096, n_streams=2)
    plan = sd.plan(sb.starts, sb.ends, sb.nbytes)
    assert len(plan) >= 3
    d_bytes = torch.zeros(((sb.nbytes + 15) // 16) * 16 + 16, dtype=torch.uint8, device=dev())
    d_bytes[: sb.nbytes].copy_(torch.from_numpy(sb.buf))
    rst, ren, firsts = sd.rebase32(plan, sb.starts, sb.ends)
    assert rst is None
    d_en = torch.from_numpy(ren.view(np.int32)).to(dev())
    sd.learn(plan, sb.buf, sb.starts, sb.ends)
    streams = [torch.cuda.Stream(dev()), torch.cuda.Stream(dev())]
    torch.cuda.synchronize(dev())
    sd.decode_device32(plan, d_bytes.data_ptr(), None, d_en.data_ptr(), firsts, streams=[s.cuda_stream for s in streams])
    yield sd, plan, truth, (d_bytes, d_en, streams)
    sd.close()


SHARD_SPECS = [D.Dense("label", "int64", lengths=True), D.Dense("id", "uint8", 12, lengths=True),
               D.Dense("nope", "int32", 2, fill=-1, lengths=True)]


def test_shard_rows_cross_the_batches(sharded):
    sd, plan, truth, _ = sharded
    n = len(truth)
    assert int(plan[-1, 1]) == n
    ref = Ref(truth, SHARD_SPECS)
    full = sd.dense(plan, SHARD_SPECS)
    rng = np.random.default_rng(6)
    rows = rng.integers(0, n, 3000)
    rows[:6] = [0, n - 1, int(plan[1, 0]), int(plan[1, 0]) - 1, int(plan[2, 0]), int(plan[2, 0]) - 1]
    got = sd.dense(plan, SHARD_SPECS, rows=to_dev(rows), out=poisoned(SHARD_SPECS, len(rows)))
    total = int(got["label"].sum())  # consumed at once, on the current stream
    assert total == int(ref.full["label"][rows].sum())
    for sp in SHARD_SPECS:
        k = sp.out_name
        assert np.array_equal(bits(got[k].cpu().numpy()), bits(full[k].cpu().numpy())[rows]), k
        assert np.array_equal(got.lengths[k].cpu().numpy(), full.lengths[k].cpu().numpy()[rows]), k
    host = D.DenseBatch({k: v.cpu().numpy() for k, v in got.items()}, got.lengths, got.stats, got.skipped)
    assert ref.check(host, rows) == 0 and got.skipped == 0
    # b rows that no batch holds: every context skips them, and they keep the poison
    rows = rows.tolist()
    for k, v in zip((1, 2, 500, 2999), (-1, n, I64_MAX, I64_MIN)):
        rows[k] = v
    got = sd.dense(plan, SHARD_SPECS, rows=to_dev(rows), out=poisoned(SHARD_SPECS, len(rows)))
    host = D.DenseBatch({k: v.cpu().numpy() for k, v in got.items()}, got.lengths, got.stats, got.skipped)
    assert ref.check(host, rows) == 4 and got.skipped == 4
    with pytest.raises(IndexError):
        sd.dense(plan, SHARD_SPECS[:2], rows=to_dev(rows), strict=True)


# ------------------------------------------------------------------------------------ 7. C level
def test_c_level_row0_and_argument_errors(dec):
    import torch

    n = 100
    buf, st, en = synth.framed(synth.c1_payloads(n))
    lib = N.lib()
    m = 64
    out = torch.full((m * 16,), POISON, dtype=torch.uint8, device=dev())
    stats = torch.full((8,), 77, dtype=torch.int32, device=dev())
    skipped = torch.full((2,), 77, dtype=torch.int32, device=dev())
    row0 = 1 << 40
    rows = [row0 + (7 * k) % n for k in range(m)]
    rows[3], rows[10], rows[11], rows[40] = row0 - 1, row0 + n, 5, I64_MIN  # (5: in range only without row0)
    d_rows = to_dev(rows)

    def call(ctx=None, k=1, rows_ptr=d_rows.data_ptr(), rdt=N.ROWS_I64, m=m, row0=row0, **kw):
        f = dict(slot=0, dtype=N.DENSE_I64, width=1, reserved=0, fill=0, out=out.data_ptr(), lengths=None)
        f.update(kw)
        arr = (N.TfrgDenseSpec * max(k, 1))(*[N.TfrgDenseSpec(**f) for _ in range(max(k, 1))])
        return lib.tfrg_result_dense_rows(dec._ctx if ctx is None else ctx, arr, k, C.c_void_p(rows_ptr), rdt, m, row0,
                                          C.c_void_p(stats.data_ptr()), C.c_void_p(skipped.data_ptr()), None)

    assert call() == -1 and b"no result" in lib.tfrg_last_error()
    assert lib.tfrg_last_error().startswith(b"tfrg_result_dense_rows")
    res = dec.decode(buf, st, en)
    assert int(res.info.implicit_cols) == 7  # an optimistic decode
    s_label, s_id = res.slot_key.index("label"), res.slot_key.index("id")
    assert call(slot=s_label) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.int64)[:m]
    want = [(v - row0) % 1000 if row0 <= v < row0 + n else int.from_bytes(bytes([POISON]) * 8, "little", signed=True)
            for v in rows]
    assert got.tolist() == want
    assert stats.cpu().tolist()[:4] == [0, 0, 0, 0] and skipped.cpu().tolist()[0] == 4
    # the full view is still there after a rows call on an optimistic decode
    again = dec._fetch(buf, st, en, dec.info(), False)
    for k in COLS:
        assert np.array_equal(getattr(again, k), getattr(res, k)), k
    # m == 0 launches nothing (and takes a NULL list), but zeroes the counters
    skipped.fill_(77)
    assert call(slot=s_label, m=0, rows_ptr=None) == 0
    assert skipped.cpu().tolist()[0] == 0
    check = [D.Dense("label", "int64", lengths=True), D.Dense("id", "uint8", 12)]
    ref = Ref(res, check)
    for bad in (dict(k=0), dict(k=65), dict(slot=len(res.slot_key)), dict(slot=s_label, dtype=N.DENSE_F32),
                dict(slot=s_label, dtype=N.DENSE_U8), dict(slot=s_id, dtype=N.DENSE_I32), dict(slot=s_label, dtype=4),
                dict(slot=s_label, width=0), dict(slot=s_label, width=4097), dict(slot=s_label, out=None),
                dict(slot=s_label, reserved=1), dict(slot=s_label, rows_ptr=None), dict(slot=s_label, rdt=2),
                dict(slot=s_label, m=1 << 31), dict(slot=s_label, m=(1 << 32) - 1)):
        assert call(**bad) == -1, bad
        assert lib.tfrg_last_error().startswith(b"tfrg_result_dense_rows"), bad
        run(dec, ref, [99, 0, 50, 50, n])
        plain = dec.dense(check)
        assert np.array_equal(plain["label"].cpu().numpy(), ref.full["label"])


def test_every_row_of_an_empty_result_is_skipped(dec):
    import torch

    buf, st, en = synth.framed(synth.c1_payloads(10))
    res = dec.decode(buf, st, en)  # (the key table)
    s_label = res.slot_key.index("label")
    assert len(dec.decode(buf[:0], st[:0], en[:0])) == 0
    specs = [D.Dense("label", "int64", lengths=True), D.Dense("id", "uint8", 12)]
    rows = [0, 1, -1, 7, I64_MAX]
    out = poisoned(specs, len(rows))
    got = dec.dense(specs, rows=to_dev(rows), out=out)
    assert got.skipped == len(rows)
    assert all((bits(t.cpu().numpy()).view(np.uint8) == POISON).all() for t in got.values())
    assert got.stats["label"].tolist() == [0, 0, 0, 0]
    # and at the C level: no launch, m in every skipped counter, the stats zeroed
    lib = N.lib()
    stats = torch.full((8,), 77, dtype=torch.int32, device=dev())
    skipped = torch.full((2,), 77, dtype=torch.int32, device=dev())
    arr = (N.TfrgDenseSpec * 2)(*[N.TfrgDenseSpec(slot=s_label, dtype=N.DENSE_I64, width=1, reserved=0, fill=0,
                                                  out=out["label"][0].data_ptr(), lengths=None) for _ in range(2)])
    d_rows = to_dev(rows)
    assert lib.tfrg_result_dense_rows(dec._ctx, arr, 2, C.c_void_p(d_rows.data_ptr()), N.ROWS_I64, len(rows), 0,
                                      C.c_void_p(stats.data_ptr()), C.c_void_p(skipped.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert skipped.cpu().tolist() == [5, 5] and stats.cpu().tolist() == [0] * 8
    assert (out["label"][0].cpu().numpy().view(np.uint8) == POISON).all()


def test_raw_pointer_outputs_take_a_raw_row_list(c1, c1_ref):
    import torch

    d = c1[0]
    specs = [D.Dense("label", "int32", 2, fill=-3, lengths=True), D.Dense("id", "uint8", 12)]
    ref = Ref(c1[1], specs)
    m = 300
    rows = np.random.default_rng(8).integers(0, N1, m)
    s = torch.cuda.Stream(dev())
    with torch.cuda.stream(s):
        for name, dt in (("int32", np.int32), ("int64", np.int64)):
            d_rows = to_dev(rows, dt)
            lab = torch.zeros((m, 2), dtype=torch.int32, device=dev())
            lens = torch.zeros(m, dtype=torch.int32, device=dev())
            ids = torch.zeros((m, 12), dtype=torch.uint8, device=dev())
            got = d.dense(specs, out={"label": (lab.data_ptr(), lens.data_ptr()), "id": ids.data_ptr()},
                          rows=(d_rows.data_ptr(), m, name), stream=s.cuda_stream)
            assert got["label"] == lab.data_ptr() and got.stats == {}
            assert np.array_equal(lab.cpu().numpy(), ref.full["label"][rows])
            assert np.array_equal(ids.cpu().numpy(), ref.full["id"][rows])
            assert np.array_equal(lens.cpu().numpy(), ref.full.lengths["label"][rows])
        with pytest.raises(ValueError):
            d.dense(specs, out={"label": lab.data_ptr(), "id": ids.data_ptr()}, rows=(d_rows.data_ptr(), m, "int16"))
        with pytest.raises(TypeError):
            d.dense(specs, out={"label": lab.data_ptr(), "id": ids.data_ptr()}, rows=d_rows)


# ------------------------------------------------------------------------------------ 8. minibatches
SPECS_MB = [D.Dense("label", "int64"), D.Dense("id", "uint8", 12)]


def drawn(batches) -> list[int]:
    """The record numbers an epoch drew, from the decoded ids (``img-%08d`` of the row)."""
    out = []
    for b in batches:
        ids = b["id"].cpu().numpy()
        nums = [int(bytes(r)[4:]) for r in ids]
        assert b["label"][:, 0].cpu().tolist() == [v % 1000 for v in nums]
        assert b.skipped == 0
        out += nums
    return out


def test_minibatches_cover_an_epoch(c1):
    d = c1[0]
    a = drawn(d.minibatches(SPECS_MB, 512, seed=3))
    assert sorted(a) == list(range(N1)) and a != list(range(N1))
    sizes = [tuple(b["id"].shape) for b in D.minibatches(d, SPECS_MB, 512, seed=3)]
    assert sizes == [(512, 12)] * 9 + [(N1 - 9 * 512, 12)]
    assert drawn(d.minibatches(SPECS_MB, 512, seed=3)) == a
    assert drawn(d.minibatches(SPECS_MB, 512, seed=4)) != a
    part = drawn(d.minibatches(SPECS_MB, 512, seed=3, drop_last=True))
    assert part == a[: 9 * 512] and len(set(part)) == 9 * 512


def test_minibatches_over_a_shard_plan(sharded):
    sd, plan, truth, _ = sharded
    n = len(truth)
    want = truth.dense(SPECS_MB)
    order = []
    for b in sd.minibatches(plan, SPECS_MB, 512, seed=1):
        lab = b["label"][:, 0].cpu().numpy()
        ids = b["id"].cpu().numpy()
        assert b.skipped == 0
        order.append((lab, ids))
    labs = np.concatenate([x[0] for x in order])
    ids = np.concatenate([x[1] for x in order])
    assert labs.size == n
    # the shard's ids are not unique over its files: compare the multisets of whole rows
    key = lambda lab, idv: sorted(zip(lab.tolist(), (bytes(r) for r in idv)))  # noqa: E731
    assert key(labs, ids) == key(want["label"][:, 0], want["id"])
    again = np.concatenate([b["label"][:, 0].cpu().numpy() for b in sd.minibatches(plan, SPECS_MB, 512, seed=1)])
    assert np.array_equal(again, labs)
    other = np.concatenate([b["label"][:, 0].cpu().numpy() for b in sd.minibatches(plan, SPECS_MB, 512, seed=2)])
    assert not np.array_equal(other, labs)
    short = sum(int(b["id"].shape[0]) for b in sd.minibatches(plan, SPECS_MB, 512, seed=1, drop_last=True))
    assert short == n // 512 * 512


def test_rows_made_on_the_current_stream_just_before_the_call(c1, c1_ref):
    """Stream ordering: the row list is produced by kernels queued on the current (non-default)
    stream immediately before the call, and the outputs are consumed on it immediately after."""
    import torch

    d = c1[0]
    s = torch.cuda.Stream(dev())
    with torch.cuda.stream(s):
        big = torch.arange(1 << 22, device=dev(), dtype=torch.int64)
        rows = (big.flip(0)[: 1 << 16] * 7919) % N1  # (queued on s; not finished when dense() is called)
        got = d.dense(C1_SPECS[:1], rows=rows)
        total = int(got["label"].sum())
    host = rows.cpu().numpy()
    assert total == int((host % 1000).sum())
    assert np.array_equal(got["label"][:, 0].cpu().numpy(), host % 1000)
