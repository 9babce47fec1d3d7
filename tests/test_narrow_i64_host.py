"""The learner's width rule for the int64 column (Learned::i64_width, csrc/tfrg_learn.cpp): 2 when every
int64 slot is one inline varint of at most 2 bytes in every kept record shape, 4 when of at most 4
bytes, 8 otherwise. An optimistic decode stores the column in elements of that width
(tfrg_info.i64_width), so a width too small here is a truncated value in every record.

The C ABI reports the width only through a decode on a device context; tests/narrow_i64_driver.cpp runs
learn_shapes on its own and prints it. The expected widths follow from the varint encoding alone: 7
value bits per byte, so a value below 2^14 takes at most 2 bytes, one below 2^28 at most 4, anything
larger 5 or more, and a negative value 10. Host code only: no GPU, nothing loaded into Python."""

import shutil
import subprocess
from pathlib import Path

import pytest

from tfr_reader import writer

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "tfrecords-reader_amd" / "csrc"
N = 400


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the learner's driver")
    exe = tmp_path_factory.mktemp("narrow_i64") / "narrow_i64_driver"
    srcs = [ROOT / "tests" / "narrow_i64_driver.cpp", CSRC / "tfrg_learn.cpp", CSRC / "tfrg_cpu.cpp", CSRC / "tfrg_host.cpp"]
    p = subprocess.run(["g++", "-std=c++17", "-O1", *map(str, srcs), "-o", str(exe), "-lz", "-lpthread"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return exe


def _learn(driver, tmp_path, payloads, schema) -> tuple[int, int]:
    """(templates, i64_width) of the framed payloads under the schema [(key, kind)]."""
    f = tmp_path / "sample.tfrecord"
    f.write_bytes(writer.frame_records(payloads))
    p = subprocess.run([str(driver), str(f), *[f"{k.encode().hex()}:{kind}" for k, kind in schema]],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = dict(line.split() for line in p.stdout.splitlines())
    return int(out["templates"]), int(out["i64_width"])


def _ids(i):
    return f"img-{i:08d}".encode()


def _c1(labels):
    """C1-shaped records whose labels cycle through `labels`: every value in N / len(labels) records."""
    return [writer.encode_example([("label", "int64_list", [labels[i % len(labels)]]), ("id", "bytes_list", [_ids(i)])])
            for i in range(N)]


C1 = [("label", 3), ("id", 1)]


def test_labels_0_to_999_take_two_bytes(driver, tmp_path):
    payloads = [writer.encode_example([("label", "int64_list", [i % 1000]), ("id", "bytes_list", [_ids(i)])])
                for i in range(2000)]
    assert _learn(driver, tmp_path, payloads, C1) == (2, 2)  # (1- and 2-byte varints: two shapes)


def test_the_largest_two_byte_varint(driver, tmp_path):
    assert _learn(driver, tmp_path, _c1([0, 127, 128, 16383]), C1) == (2, 2)


@pytest.mark.parametrize("value", [16384, (1 << 21) - 1, 1 << 21, (1 << 28) - 1], ids=["2^14", "2^21-1", "2^21", "2^28-1"])
def test_three_and_four_byte_varints_take_four_bytes(driver, tmp_path, value):
    nt, width = _learn(driver, tmp_path, _c1([5, value]), C1)
    assert nt == 2 and width == 4


@pytest.mark.parametrize("value", [1 << 28, -1, 1 << 40], ids=["2^28", "negative", "2^40"])
def test_longer_varints_are_not_placed_and_keep_eight_bytes(driver, tmp_path, value):
    """5 bytes and more: not an inline value (mode 1) in that shape, so nothing bounds the column."""
    nt, width = _learn(driver, tmp_path, _c1([5, value]), C1)
    assert nt == 2 and width == 8


def test_two_int64_slots_share_the_wider_width(driver, tmp_path):
    payloads = [writer.encode_example([("a", "int64_list", [i % 1000]), ("b", "int64_list", [20000 + i % 100]),
                                       ("id", "bytes_list", [_ids(i)])]) for i in range(N)]
    nt, width = _learn(driver, tmp_path, payloads, [("a", 3), ("b", 3), ("id", 1)])
    assert nt == 2 and width == 4  # (a alone would be 2: one width for the whole column)
    both_small = [writer.encode_example([("a", "int64_list", [i % 1000]), ("b", "int64_list", [i % 100]),
                                         ("id", "bytes_list", [_ids(i)])]) for i in range(N)]
    assert _learn(driver, tmp_path, both_small, [("a", 3), ("b", 3), ("id", 1)])[1] == 2


def test_no_int64_slot_has_nothing_to_narrow(driver, tmp_path):
    payloads = [writer.encode_example([("id", "bytes_list", [_ids(i)]), ("x", "float_list", [float(i)])]) for i in range(N)]
    nt, width = _learn(driver, tmp_path, payloads, [("id", 1), ("x", 2)])
    assert nt == 1 and width == 8


def test_an_absent_or_repeated_value_keeps_eight_bytes(driver, tmp_path):
    """A shape without the slot (order word 0), and a shape with two values in it (a list, not mode 1)."""
    with_label = _c1([7])[: N // 2]
    without = [writer.encode_example([("id", "bytes_list", [_ids(i)])]) for i in range(N // 2)]
    assert _learn(driver, tmp_path, with_label + without, C1) == (2, 8)
    two = [writer.encode_example([("label", "int64_list", [1, 2]), ("id", "bytes_list", [_ids(i)])]) for i in range(N // 2)]
    assert _learn(driver, tmp_path, with_label + two, C1) == (2, 8)


def test_nothing_learned_is_eight_bytes(driver, tmp_path):
    """No record of the schema's keys: no shape is kept, and the width is the default."""
    payloads = [writer.encode_example([("other", "int64_list", [1])]) for _ in range(10)]
    nt, width = _learn(driver, tmp_path, payloads, C1)
    assert width == 8
