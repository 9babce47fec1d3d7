"""The learner's per-slot end-relative rule (Learned::off_rel / rel_off, csrc/tfrg_learn.cpp): a bytes
slot is end-relative when every kept record shape holds it as one inline element at the same distance
from the record's end. An optimistic decode leaves the bytes_off words of such a slot implicit
(tfrg_info.implicit_off_slots), so a wrong bit or offset here is a wrong offset in every record.

The C ABI reports the rule only through a device context; tests/implicit_off_driver.cpp runs
learn_shapes on its own and prints it. The expected offsets are worked out here from the writer's
bytes: where the element lies in each payload, counted from the end of the framed record (the
payload's end + 4 bytes of data CRC). Host code only: no GPU, nothing loaded into Python."""

import shutil
import subprocess
from pathlib import Path

import pytest

from tfr_reader import synth, writer

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "tfrecords-reader_amd" / "csrc"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the learner's driver")
    exe = tmp_path_factory.mktemp("implicit_off") / "implicit_off_driver"
    srcs = [ROOT / "tests" / "implicit_off_driver.cpp", CSRC / "tfrg_learn.cpp", CSRC / "tfrg_cpu.cpp", CSRC / "tfrg_host.cpp"]
    p = subprocess.run(["g++", "-std=c++17", "-O1", *map(str, srcs), "-o", str(exe), "-lz", "-lpthread"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return exe


def _learn(driver, tmp_path, framed: bytes, schema) -> dict:
    f = tmp_path / "sample.tfrecord"
    f.write_bytes(framed)
    p = subprocess.run([str(driver), str(f), *[f"{k.encode().hex()}:{kind}" for k, kind in schema]],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = {}
    for line in p.stdout.splitlines():
        name, *vals = line.split()
        out[name] = vals
    return {"templates": int(out["templates"][0]), "off_rel": int(out["off_rel"][0], 16),
            "rel_off": [int(v) for v in out["rel_off"]], "len_const": int(out["len_const"][0]),
            "const_len": [int(v) for v in out["const_len"]]}


def _end_offsets(payloads, value_of) -> set[int]:
    """Where each record's element lies, counted from the end of its framed record."""
    got = set()
    for i, p in enumerate(payloads):
        v = value_of(i)
        at = p.rfind(v)
        assert at >= 0 and p.count(v) == 1
        got.add(at - len(p) - 4)
    return got


def _ids(i):
    return f"img-{i:08d}".encode()


def test_c1_label_varint_lengths_keep_the_ids_bit(driver, tmp_path):
    """Labels 100 .. 299: one- and two-byte varints, two shapes; the id is the payload's last field."""
    n = 200
    payloads = [writer.encode_example([("label", "int64_list", [100 + i]), ("id", "bytes_list", [_ids(i)])])
                for i in range(n)]
    assert len({len(p) for p in payloads}) == 2
    want = _end_offsets(payloads, _ids)
    assert want == {-16}
    for crc in (True, False):  # (spec frames, and the unchecked frames of crc=False writers)
        L = _learn(driver, tmp_path, writer.frame_records(payloads, crc), [("label", 3), ("id", 1)])
        assert L["templates"] == 2 and L["off_rel"] == 0b10 and L["rel_off"] == [0, -16]
        assert L["len_const"] == 1 and L["const_len"][1] == 12


def test_id_before_a_label_of_varying_length_clears_it(driver, tmp_path):
    n = 200
    payloads = [writer.encode_example([("id", "bytes_list", [_ids(i)]), ("label", "int64_list", [100 + i])])
                for i in range(n)]
    assert len(_end_offsets(payloads, _ids)) == 2
    L = _learn(driver, tmp_path, writer.frame_records(payloads), [("id", 1), ("label", 3)])
    assert L["templates"] == 2 and L["off_rel"] == 0 and L["len_const"] == 1 and L["const_len"][0] == 12


def test_id_before_a_label_of_one_length_keeps_it(driver, tmp_path):
    """One shape: the position is the same in every template whatever follows the id."""
    payloads = [writer.encode_example([("id", "bytes_list", [_ids(i)]), ("label", "int64_list", [i % 100])])
                for i in range(200)]
    (want,) = _end_offsets(payloads, _ids)
    L = _learn(driver, tmp_path, writer.frame_records(payloads), [("id", 1), ("label", 3)])
    assert L["templates"] == 1 and L["off_rel"] == 0b01 and L["rel_off"][0] == want


def test_variable_length_ids_last_in_the_payload(driver, tmp_path):
    """c1v: the id ends the payload, so its START moves with its length: not end-relative, and the
    lengths are not constant either."""
    n = 2000
    blob, offs = synth.c1v_blob(n, 0, 11)
    buf = synth.frame_blob(blob, offs)
    L = _learn(driver, tmp_path, buf.tobytes(), [("label", 3), ("id", 1)])
    assert L["templates"] == 16 and L["off_rel"] == 0 and L["len_const"] == 0


def test_two_bytes_slots_one_end_relative(driver, tmp_path):
    """a (8 bytes) before a label of varying length, b (6 bytes) after it: only b's bit, and the rule
    is per slot -- len_const holds for both."""
    def a_of(i):
        return f"a{i:07d}".encode()

    def b_of(i):
        return f"b{i:05d}".encode()

    payloads = [writer.encode_example([("a", "bytes_list", [a_of(i)]), ("label", "int64_list", [100 + i]),
                                       ("b", "bytes_list", [b_of(i)])]) for i in range(200)]
    assert len(_end_offsets(payloads, a_of)) == 2 and _end_offsets(payloads, b_of) == {-10}
    L = _learn(driver, tmp_path, writer.frame_records(payloads), [("a", 1), ("label", 3), ("b", 1)])
    assert L["templates"] == 2 and L["off_rel"] == 0b100 and L["rel_off"][2] == -10
    assert L["len_const"] == 1 and L["const_len"] == [8, 0, 6]


def test_a_slot_of_varying_length_does_not_clear_another_slots_bit(driver, tmp_path):
    """The rule does not depend on len_const: a's length varies (len_const off), b after it stays
    end-relative."""
    payloads = [writer.encode_example([("a", "bytes_list", [b"x" * (3 + i % 2)]), ("b", "bytes_list", [_ids(i)])])
                for i in range(200)]
    L = _learn(driver, tmp_path, writer.frame_records(payloads), [("a", 1), ("b", 1)])
    assert L["templates"] == 2 and L["len_const"] == 0 and L["off_rel"] == 0b10 and L["rel_off"][1] == -16


def test_an_absent_or_repeated_element_clears_it(driver, tmp_path):
    """A shape without the slot, and a shape with two elements in it (not one inline element)."""
    with_id = [writer.encode_example([("label", "int64_list", [i % 100]), ("id", "bytes_list", [_ids(i)])])
               for i in range(100)]
    without = [writer.encode_example([("label", "int64_list", [i % 100])]) for i in range(100)]
    L = _learn(driver, tmp_path, writer.frame_records(with_id + without), [("label", 3), ("id", 1)])
    assert L["templates"] == 2 and L["off_rel"] == 0
    two = [writer.encode_example([("label", "int64_list", [i % 100]), ("id", "bytes_list", [_ids(i), b"zz"])])
           for i in range(100)]
    L = _learn(driver, tmp_path, writer.frame_records(with_id + two), [("label", 3), ("id", 1)])
    assert L["off_rel"] == 0
