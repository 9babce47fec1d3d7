"""The record-shape template learner (csrc/tfrg_learn.cpp) parses record bytes from outside the
program. It is built here on its own -- tests/learn_driver.cpp, the learner and the host decoder it
calls, with AddressSanitizer and UndefinedBehaviorSanitizer -- and run as a child process on every
golden TFRecord file and on three hostile mutations of each: truncated in the middle of the last
record, a length field set past the end of the file, one payload byte of the first record flipped.
Every run must end with status 0 and no sanitizer report; on the unmutated files the driver prints
what tfrg_learn_templates_host of the built library returns. Host code only: no GPU, nothing
preloaded, and the sanitized code never loads into this process."""
import json
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tfr_reader import _native as N

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "tfrecords-reader_amd" / "csrc"
FILES = sorted((ROOT / "tests" / "golden" / "files").glob("*.tfrecord"))
KINDS = {"bytes_list": 1, "float_list": 2, "int64_list": 3}
LT_WORDS = 8 + 4 * 16 + 3 * 64 + 3 * 16  # kLtWords (tfrg_layout.h)


def _pairs(path: Path) -> list[tuple[bytes, int]]:
    """(key, kind) of every entry of the file's golden records, in order of first appearance."""
    meta = json.loads(path.with_suffix(".json").read_text())
    out: list[tuple[bytes, int]] = []
    for rec in meta.get("records", []):
        for key_hex, kind, _ in rec.get("ok", []):
            p = (bytes.fromhex(key_hex), KINDS[kind])
            if p not in out:
                out.append(p)
    return out


# a file whose golden data names no keys (the framing edge cases) is learned against every file's keys
ALL_PAIRS = [p for f in FILES for p in _pairs(f)]
ALL_PAIRS = [p for i, p in enumerate(ALL_PAIRS) if p not in ALL_PAIRS[:i]]


def _schema(path: Path) -> list[tuple[bytes, int]]:
    return _pairs(path) or ALL_PAIRS


def _frames(data: bytes) -> list[tuple[int, int]]:
    """The driver's index: frames as their length fields give them; one past the file ends it."""
    out, pos = [], 0
    while pos + 12 <= len(data):
        e = (pos + 16 + struct.unpack_from("<Q", data, pos)[0]) & 0xFFFFFFFFFFFFFFFF
        out.append((pos, e))
        if e > len(data) or e <= pos:
            break
        pos = e
    return out


def _mutations(data: bytes) -> dict[str, bytes]:
    fr = _frames(data)
    if not fr or fr[-1][1] > len(data):
        fr = fr[:-1]
    if not fr:
        return {}
    out = {}
    s, e = fr[-1]
    out["truncated"] = data[: s + (e - s) // 2]
    out["length_past_end"] = data[:s] + struct.pack("<Q", len(data) + 4096) + data[s + 8 :]
    s, e = fr[0]
    if e - s > 16:
        k = s + 12 + (e - s - 16) // 2
        out["payload_flip"] = data[:k] + bytes([data[k] ^ 0x5A]) + data[k + 1 :]
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the learner's driver")
    exe = tmp_path_factory.mktemp("learn") / "learn_driver"
    srcs = [ROOT / "tests" / "learn_driver.cpp", CSRC / "tfrg_learn.cpp", CSRC / "tfrg_cpu.cpp", CSRC / "tfrg_host.cpp"]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           *map(str, srcs), "-o", str(exe), "-lz", "-lpthread"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return exe


def _run(driver: Path, path: Path, schema) -> str:
    args = [f"{k.hex()}:{kind}" for k, kind in schema]
    p = subprocess.run([str(driver), str(path), *args], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (path.name, p.returncode, p.stderr[-4000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    return p.stdout


def _library(data: bytes, schema) -> str:
    """What the driver prints, from the built library's tfrg_learn_templates_host."""
    keys: list[bytes] = []
    for k, _ in schema:
        if k not in keys:
            keys.append(k)
    blob = np.frombuffer(b"".join(keys) or b"\0", np.uint8)
    offs = np.zeros(len(keys) + 1, np.uint64)
    offs[1:] = np.cumsum([len(k) for k in keys])
    sk = np.array([keys.index(k) for k, _ in schema] or [0], np.uint32)
    sd = np.array([kind for _, kind in schema] or [0], np.uint8)
    fr = _frames(data)
    st = np.array([a for a, _ in fr] or [0], np.uint64)
    en = np.array([b for _, b in fr] or [0], np.uint64)
    buf = np.frombuffer(data or b"\0", np.uint8)
    out = np.zeros(32 * LT_WORDS, np.uint32)
    W = np.zeros(1, np.uint32)
    nt = N.lib().tfrg_learn_templates_host(len(keys), N.ptr(blob), N.ptr(offs), None, len(schema), N.ptr(sk), N.ptr(sd),
                                           N.ptr(buf), len(data), N.ptr(st), N.ptr(en), len(fr), 0, N.ptr(out),
                                           out.size, N.ptr(W))
    assert nt >= 0
    words = "".join(f" {int(w):x}" for w in out[: nt * LT_WORDS])
    return f"templates {nt}\nW {int(W[0])}\nwords{words}\n"


@pytest.mark.parametrize("path", FILES, ids=lambda p: p.stem)
def test_learner_clean_and_equal_to_the_library(driver, path):
    schema = _schema(path)
    assert _run(driver, path, schema) == _library(path.read_bytes(), schema)


@pytest.mark.parametrize("path", FILES, ids=lambda p: p.stem)
def test_learner_clean_on_mutated_files(driver, path, tmp_path):
    muts = _mutations(path.read_bytes())
    assert muts or path.stat().st_size < 16, "a file with a whole frame has mutations"
    for name, data in muts.items():
        q = tmp_path / f"{path.stem}.{name}.tfrecord"
        q.write_bytes(data)
        out = _run(driver, q, _schema(path))
        assert out.startswith("templates ")


def test_some_file_learns_templates(driver):
    """(the comparison above is not between two empty results)"""
    counts = [int(_run(driver, p, _schema(p)).split()[1]) for p in FILES if p.stem in ("c0_mini_crc", "demo")]
    assert counts and all(c >= 1 for c in counts)
