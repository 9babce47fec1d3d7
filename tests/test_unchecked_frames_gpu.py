"""Unchecked-frame templates and CRC-less template passes (csrc/tfrg_tpl.hip, kLtFrame): records
whose two CRC fields are 0, as the reference's own writers leave them, take a template of their own
frame class with verdict TFRG_V_LEN_MATCH, and a crc=False decode takes templates of either class on
the mask match alone. Three contexts see every input: k_tpl_lane with staged windows on batches of
any size (TFRG_TPL_STAGE=2), with per-lane window loads (=0), both optimistic, and the canonical
walk without templates (TFRG_TEMPLATES=0) as the yardstick. Their columns must be equal, and the
oracle's record by record.

N = 5,003 C1 records (78 whole 64-record groups and one of 11) whose labels cross 127 / 128, so both
record lengths and both templates of a class occur in most groups.

aux: defined for failing records only (the canonical walk never writes it for an OK record, so the
yardstick's is whatever its buffer held). So aux is asserted equal to the yardstick's wherever the
yardstick's status is not 0, and all 0 after a confirmed optimistic decode that stored its statuses.
"""

import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gpu_parity import _compare_to_oracle
from tfr_reader import hip, synth, writer

pytestmark = pytest.mark.gpu

COLS = ("status", "verdict", "order", "row_splits", "i64", "f32", "bytes_off", "bytes_len", "slot_base")
N = 5003
STATUS, ORDER, BYTES_LEN = 1, 2, 4  # TFRG_IMPLICIT_*
SAMPLE_IDX = list(range(0, 130)) + list(range(130, N - 70, 61)) + list(range(N - 70, N))


@pytest.fixture(scope="module")
def orc():
    return O.Oracle()


def _c1(crc):
    blob, offs = synth.c1_blob(N, 100, 7)
    buf = synth.frame_blob(blob, offs, crc)
    ends = (offs[1:] + 16 * np.arange(1, N + 1)).astype(np.uint64)
    starts = np.concatenate([[0], ends[:-1]]).astype(np.uint64)
    assert int(ends[-1]) == buf.size and len(set((ends - starts).tolist())) == 2
    return buf, starts, ends


@pytest.fixture(scope="module")
def spec():
    return _c1(True)


@pytest.fixture(scope="module")
def zero():
    buf, st, en = _c1(False)
    assert not buf[int(st[9]) + 8 : int(st[9]) + 12].any() and not buf[int(en[9]) - 4 : int(en[9])].any()
    return buf, st, en


@pytest.fixture(scope="module")
def mixed(spec, zero):
    """Alternating runs of 200 spec-framed and 200 zero-CRC records."""
    buf, st, en = spec
    buf = buf.copy()
    is_zero = (np.arange(N) // 200) % 2 == 1
    for i in np.flatnonzero(is_zero):
        buf[int(st[i]) : int(en[i])] = zero[0][int(st[i]) : int(en[i])]
    return buf, st, en, is_zero


def _put32(buf, at, v):
    buf[at : at + 4] = np.frombuffer(int(v).to_bytes(4, "little"), np.uint8)


def _crc_zero_payload(label: int) -> bytes:
    """A C1 record (12-byte id b"img-" + 4 bytes + b"abcd") whose masked payload CRC-32C is 0:
    the CRC is affine in the id's 32 free bits; solved over GF(2)."""
    def pl(x):
        return writer.encode_example([("label", "int64_list", [label]),
                                      ("id", "bytes_list", [b"img-" + x.to_bytes(4, "little") + b"abcd"])])
    r = (-0xA282EAD8) & 0xFFFFFFFF  # masked(c) == 0  <=>  rotr15(c) == -0xA282EAD8
    base = O.crc32c(pl(0))
    want, x = (((r << 15) | (r >> 17)) & 0xFFFFFFFF) ^ base, 0
    rows = [(O.crc32c(pl(1 << k)) ^ base, 1 << k) for k in range(32)]
    for bit in range(32):
        piv = next(i for i, (v, _) in enumerate(rows) if (v >> bit) & 1)
        pv, px = rows.pop(piv)
        rows = [((v ^ pv, m ^ px) if (v >> bit) & 1 else (v, m)) for v, m in rows]
        if (want >> bit) & 1:
            want, x = want ^ pv, x ^ px
    assert want == 0 and O.masked_crc32c(pl(x)) == 0
    return pl(x)


def _trio(monkeypatch, sample, optimistic=True):
    """Fresh contexts: staged windows, per-lane windows (both learned `sample`), and no templates."""
    monkeypatch.setenv("TFRG_OPTIMISTIC", "1" if optimistic else "0")
    monkeypatch.setenv("TFRG_TEMPLATES", "1")
    monkeypatch.setenv("TFRG_TPL_STAGE", "2")
    staged = hip.HipDecoder(0)
    monkeypatch.setenv("TFRG_TPL_STAGE", "0")
    plain = hip.HipDecoder(0)
    monkeypatch.setenv("TFRG_TEMPLATES", "0")
    yard = hip.HipDecoder(0)
    for d in (staged, plain, yard):
        d.decode(*sample)
    assert staged.template_count() >= 1 and plain.template_count() >= 1 and yard.template_count() == 0
    return staged, plain, yard


def _close(trio):
    for d in trio:
        d.close()


def _upload(buf, st, en, mode):
    import torch

    dev = torch.device("cuda", 0)
    d_b = torch.zeros(buf.size + 32, dtype=torch.uint8, device=dev)
    d_b[: buf.size].copy_(torch.from_numpy(buf.copy()))
    if mode == "u64":
        d_s = torch.from_numpy(st.astype(np.int64)).to(dev)
        d_e = torch.from_numpy(en.astype(np.int64)).to(dev)
    else:
        d_s = torch.from_numpy(st.astype(np.uint32).view(np.int32)).to(dev)
        d_e = torch.from_numpy(en.astype(np.uint32).view(np.int32)).to(dev)
    torch.cuda.synchronize(dev)
    return d_b, d_s, d_e


def _launch(dec, dev_bufs, buf, st, en, mode, **flags):
    d_b, d_s, d_e = dev_bufs
    n = len(st)
    dec.set_record_bound(int((en - st).max()) if n else 16)
    if mode == "u64":
        dec.decode_device(d_b.data_ptr(), buf.size, d_s.data_ptr(), d_e.data_ptr(), n, **flags)
    else:
        dec.decode_device32(d_b.data_ptr(), buf.size, d_s.data_ptr() if mode == "u32" else None, d_e.data_ptr(),
                            int(st[0]) if n else 0, n, **flags)


def _device(dec, buf, st, en, mode="ends", first=0, count=None, **flags):
    """One device-resident decode of records [first, first + count): (result, re-runs)."""
    import torch

    n = len(st) - first if count is None else count
    st, en = np.ascontiguousarray(st[first : first + n]), np.ascontiguousarray(en[first : first + n])
    bufs = _upload(buf, st, en, mode)
    before = dec.device_bytes()[1]
    _launch(dec, bufs, buf, st, en, mode, **flags)
    info = dec.info()
    r = dec._fetch(buf, st, en, info, False)
    torch.cuda.synchronize()
    return r, dec.device_bytes()[1] - before


def _all(trio, buf, st, en, mode="ends", **kw):
    """The decode on the three contexts; columns equal. Returns the template contexts' results and
    re-runs (asserted equal) and the yardstick's result."""
    (a, ra), (b, rb), (y, ry) = (_device(d, buf, st, en, mode, **kw) for d in trio)
    assert ry == 0
    for r in (a, b):
        for k in COLS:
            assert np.array_equal(np.array(getattr(r, k)), np.array(getattr(y, k))), k
        assert list(r.info.kind_totals) == list(y.info.kind_totals)
        assert int(r.info.n_errors) == int(y.info.n_errors) and int(r.info.first_error) == int(y.info.first_error)
        ok = np.array(y.status) == 0
        assert np.array_equal(np.array(r.aux)[~ok], np.array(y.aux)[~ok])
        if int(r.info.implicit_cols):  # (a confirmed optimistic decode: k_tpl_lane took every record)
            assert ok.all() and not np.array(r.aux).any()
    for k in ("tpl_groups_missed", "implicit_cols", "placed_slots"):
        assert int(getattr(a.info, k)) == int(getattr(b.info, k)), k
    assert ra == rb
    return a, ra, y


def _oracle(r, orc, buf, idx, check_crc=True):
    bad = _compare_to_oracle(r, orc, buf, r.starts, r.ends, check_crc=check_crc, idx=idx)
    assert not bad, bad


@pytest.mark.parametrize("mode", ["ends", "u32", "u64"])
def test_zero_crc_batch_takes_templates(monkeypatch, orc, zero, mode):
    buf, st, en = zero
    trio = _trio(monkeypatch, zero)
    try:
        assert trio[0].template_frames() == 2 and trio[1].template_frames() == 2 and trio[2].template_frames() == 0
        r, reruns, _ = _all(trio, buf, st, en, mode)
        assert reruns == 0 and int(r.info.tpl_groups_missed) == 0
        assert not np.array(r.status).any() and (np.array(r.verdict) == 1).all()
        assert int(r.info.implicit_cols) == ORDER | BYTES_LEN
        _oracle(r, orc, buf, SAMPLE_IDX)
    finally:
        _close(trio)


def test_device_view_without_info(monkeypatch, zero):
    """tfrg_result_device straight after the decode: status, verdict and aux as the yardstick's."""
    import torch

    torch.zeros(1, device="cuda:0")
    hip_rt = ctypes.CDLL("libamdhip64.so")
    buf, st, en = zero
    trio = _trio(monkeypatch, zero)
    try:
        bufs = _upload(buf, st, en, "ends")
        got = []
        for d in trio:
            before = d.device_bytes()[1]
            _launch(d, bufs, buf, st, en, "ends")
            cols = d.device_columns()
            torch.cuda.synchronize()
            assert d.device_bytes()[1] == before
            out = {}
            for name, dt in (("status", np.int32), ("verdict", np.uint8), ("aux", np.int64)):
                host = np.full(N, 0x55, dt)
                p = ctypes.cast(getattr(cols, name), ctypes.c_void_p).value
                assert hip_rt.hipMemcpy(ctypes.c_void_p(host.ctypes.data), ctypes.c_void_p(p),
                                        ctypes.c_size_t(host.nbytes), 2) == 0
                out[name] = host
            got.append(out)
        y = got[2]
        assert not y["status"].any() and (y["verdict"] == 1).all()
        for g in got[:2]:
            assert np.array_equal(g["status"], y["status"]) and np.array_equal(g["verdict"], y["verdict"])
            assert not g["aux"].any()  # (every status 0: see the module docstring)
    finally:
        _close(trio)


def test_record_range_cuts(monkeypatch, orc, zero):
    buf, st, en = zero
    trio = _trio(monkeypatch, zero)
    try:
        for mode in ("ends", "u32"):
            r, reruns, _ = _all(trio, buf, st, en, mode, first=1001, count=3500)
            assert reruns == 0 and len(r) == 3500 and (np.array(r.verdict) == 1).all()
            _oracle(r, orc, buf, list(range(0, 70)) + list(range(70, 3500, 53)) + list(range(3430, 3500)))
        assert int(en[0]) < 64  # (the first record's window begins before the batch: head_fix)
        for count in (1, 63, 64, 65):
            for first in (0, 4000):
                r, reruns, _ = _all(trio, buf, st, en, "ends", first=first, count=count)
                assert reruns == 0 and len(r) == count and (np.array(r.verdict) == 1).all()
                assert int(r.info.tpl_groups_missed) == 0
                _oracle(r, orc, buf, range(count))
    finally:
        _close(trio)


def test_fallbacks_inside_a_zero_crc_batch(monkeypatch, orc, zero):
    buf, st, en = zero
    trio = _trio(monkeypatch, zero)
    try:
        bad = buf.copy()
        s, e = int(st[700]), int(en[700])
        _put32(bad, e - 4, O.masked_crc32c(bytes(buf[s + 12 : e - 4])))
        s, e = int(st[1400]), int(en[1400])
        _put32(bad, s + 8, O.masked_crc32c(bytes(buf[s : s + 8])))
        p0 = _crc_zero_payload((100 + 2100) % 1000)  # (record 2100's label: its length stays)
        s, e = int(st[2100]), int(en[2100])
        assert e - s == len(p0) + 16
        bad[s + 12 : e - 4] = np.frombuffer(p0, np.uint8)
        r, reruns, _ = _all(trio, bad, st, en, "ends")
        assert reruns == 1 and int(r.info.tpl_groups_missed) == 3
        v = np.array(r.verdict)
        assert int(v[700]) == 5 and int(v[1400]) == 3 and int(v[2100]) == 5
        assert (np.delete(v, [700, 1400, 2100]) == 1).all() and not np.array(r.status).any()
        _oracle(r, orc, bad, list(range(640, 770)) + list(range(1380, 1420)) + list(range(2050, 2150)))
    finally:
        _close(trio)


def test_mixed_batch_learned_from_itself(monkeypatch, orc, mixed):
    buf, st, en, is_zero = mixed
    trio = _trio(monkeypatch, (buf, st, en))
    try:
        assert trio[0].template_frames() == 3 and trio[0].template_count() == 4
        for mode in ("ends", "u64"):
            r, reruns, _ = _all(trio, buf, st, en, mode)
            assert reruns == 0 and int(r.info.tpl_groups_missed) == 0
            assert np.array_equal(np.array(r.verdict), np.where(is_zero, 1, 7).astype(np.uint8))
            assert not int(r.info.implicit_cols) & STATUS and int(r.info.implicit_cols) == ORDER | BYTES_LEN
        _oracle(r, orc, buf, list(range(0, 130)) + list(range(130, N, 37)))
    finally:
        _close(trio)


@pytest.mark.parametrize("which", ["spec", "zero"])
def test_crc_off_decodes_take_templates(monkeypatch, orc, spec, zero, which):
    buf, st, en = spec if which == "spec" else zero
    trio = _trio(monkeypatch, (buf, st, en))
    try:
        # host decode
        for d in trio[:2]:
            before = d.device_bytes()[1]
            h = d.decode(buf, st, en, crc=False)
            y = trio[2].decode(buf, st, en, crc=False)
            assert d.device_bytes()[1] == before and int(h.info.tpl_groups_missed) == 0
            assert int(h.info.implicit_cols) != 0 and not int(h.info.implicit_cols) & STATUS
            assert (np.array(h.verdict) == 1).all() and not np.array(h.status).any()
            for k in COLS:
                assert np.array_equal(np.array(getattr(h, k)), np.array(getattr(y, k))), k
        # device decode, ends
        r, reruns, _ = _all(trio, buf, st, en, "ends", crc=False)
        assert reruns == 0 and int(r.info.tpl_groups_missed) == 0
        assert int(r.info.implicit_cols) == ORDER | BYTES_LEN
        assert (np.array(r.verdict) == 1).all() and not np.array(r.status).any()
        _oracle(r, orc, buf, SAMPLE_IDX, check_crc=False)
        # a flipped length field: no template, the canonical walk's verdict 0
        bad = buf.copy()
        bad[int(st[900]) + 1] ^= 0x01
        r, reruns, _ = _all(trio, bad, st, en, "ends", crc=False)
        assert reruns == 1 and int(r.verdict[900]) == 0 and (np.delete(np.array(r.verdict), 900) == 1).all()
    finally:
        _close(trio)
    # every pass launched (not optimistic): the template pass runs for a crc=False decode and takes
    # every record -- tpl_groups_missed counts k_tpl_lane's misses, 0 too when it does not run, so the
    # templates are asserted to exist
    trio = _trio(monkeypatch, (buf, st, en), optimistic=False)
    try:
        r, reruns, _ = _all(trio, buf, st, en, "ends", crc=False)
        assert reruns == 0 and int(r.info.tpl_groups_missed) == 0 and trio[0].template_count() >= 1
        assert int(r.info.implicit_cols) == 0 and (np.array(r.verdict) == 1).all()
        bad = buf.copy()
        bad[int(en[901]) - 9] = 0xFF  # an id byte is variable: still the template's record
        bad[int(st[902]) + 12] ^= 0x40  # a fixed payload byte: not the template's
        r, reruns, _ = _all(trio, bad, st, en, "ends", crc=False)
        assert int(r.info.tpl_groups_missed) == 1
    finally:
        _close(trio)


def test_strict_crc_on_a_zero_crc_batch(monkeypatch, zero):
    buf, st, en = zero
    trio = _trio(monkeypatch, zero)
    try:
        n = 1500
        r, reruns, y = _all(trio, buf, st, en, "ends", count=n, strict_crc=True)
        # every record is an error there: none was taken by an unchecked template (a template hit
        # stores status 0), and the decode did not run optimistically
        assert reruns == 0 and int(r.info.n_errors) == n and int(y.info.n_errors) == n
        assert np.array(r.status).all() and int(r.info.implicit_cols) == 0
        assert int(r.info.tpl_groups_missed) == (n + 63) // 64
    finally:
        _close(trio)


def test_spec_only_context_reports_what_it_did(monkeypatch, orc, spec):
    buf, st, en = spec
    trio = _trio(monkeypatch, spec)
    try:
        assert trio[0].template_frames() == 1
        r, reruns, _ = _all(trio, buf, st, en, "ends")
        assert reruns == 0 and int(r.info.implicit_cols) == 7 and (np.array(r.verdict) == 7).all()
        bad = buf.copy()
        bad[int(en[700]) - 1] ^= 0x01
        r, reruns, _ = _all(trio, bad, st, en, "ends")
        assert reruns == 1 and int(r.verdict[700]) == 3 and (np.delete(np.array(r.verdict), 700) == 7).all()
        # strict mode on a spec-only context: optimistic as ever, the one bad record an error
        r, reruns, _ = _all(trio, bad, st, en, "ends", strict_crc=True)
        assert int(r.info.n_errors) == 1
    finally:
        _close(trio)
