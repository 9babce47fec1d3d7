"""bench.py's command line on the GPU, on a directory of three files (run in this process):

* a plain run prints one line with the headline fields and none of the figures behind ``--full``;
  ``--steps`` is the number of timed steps and ``ms_per_step`` one step's time, consistent with
  ``value``;
* ``--dump-outputs`` writes float32 / float64 arrays of at most 64 MB that hold what the decode
  computed: every sampled record's status, verdict, dict order, label and id view equal what the
  deterministic generator wrote (synth.c1_blob), and a second run writes the same arrays;
* ``--full`` adds the consumer, per-kernel, roofline and pipeline figures to the same line.
"""

import json

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

FILES = 3
# (32 MiB batches: the three files are decoded as three batches on two streams)
ARGS = ["--gpus", "1", "--files", str(FILES), "--steps", "3", "--warmup", "1", "--batch-bytes", str(32 << 20)]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "config")
FULL_ONLY = ("kernels_ms", "roofline", "pipeline", "cpu_baseline", "confirm_ms", "device_view_ms", "consumer",
             "configs", "weak_scaling", "templates_off")
# (C1 records hold no float_list: an array without elements is not written)
DUMPED = ("records", "status", "verdict", "order", "counts", "int64_values", "bytes_views")


def _line(capsys, argv) -> dict:
    capsys.readouterr()
    bench.run(bench.parse_args(argv))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d) -> dict:
    assert sorted(p.name for p in d.iterdir()) == sorted(f"{k}.npy" for k in DUMPED)
    return {k: np.load(d / f"{k}.npy") for k in DUMPED}


def test_plain_run_line_and_dumped_outputs(capsys, tmp_path):
    d = _line(capsys, ARGS + ["--dump-outputs", str(tmp_path / "a")])
    assert all(k in d for k in HEADLINE) and not any(k in d for k in FULL_ONLY)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    w = bench.c4_workload("c1", 0, 1, FILES)
    assert d["config"]["records_per_gpu"] == w.n and d["config"]["batches_per_gpu"] >= 2
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - w.framed_bytes / (d["ms_per_step"] / 1e3) / 2**30) / d["value"] < 0.02

    a = _load(tmp_path / "a")
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64e6
    rec = a["records"].astype(np.int64)
    m = rec.size
    assert m == len(np.unique(rec)) and (np.diff(rec) > 0).all() and 0 <= rec[0] and rec[-1] < w.n
    assert m >= min(w.n, 100_000)  # (a C1 record costs ~84 bytes of dump)
    assert (a["status"] == 0).all() and (a["verdict"] == 7).all()
    # two key slots, one value each: `label` (int64_list) first in the record's dict, `id` second
    assert a["order"].shape == a["counts"].shape == (m, 2)
    assert (a["counts"] == 1).all() and (np.sort(a["order"], axis=1) == [1, 2]).all()
    assert all(v.size for v in a.values())
    assert a["int64_values"].shape == a["bytes_views"].shape == (m, 2)
    first = np.array([u[0] for u in w.units], np.int64)
    f = np.searchsorted(first, rec, side="right") - 1
    i = rec - first[f]
    assert np.array_equal(a["int64_values"][:, 0], np.zeros(m)) and np.array_equal(a["int64_values"][:, 1], i % 1000)
    off, ln = a["bytes_views"][:, 0].astype(np.int64), a["bytes_views"][:, 1]
    assert (ln == 12).all()
    x = (f * 1_000_003 + i) % 10**8
    want = np.empty((m, 12), np.uint8)
    want[:, :4] = np.frombuffer(b"img-", np.uint8)
    for k in range(8):
        want[:, 11 - k] = 48 + (x // 10**k) % 10
    assert np.array_equal(w.buf[off[:, None] + np.arange(12)], want)

    _line(capsys, ARGS + ["--dump-outputs", str(tmp_path / "b")])
    b = _load(tmp_path / "b")
    assert all(np.array_equal(a[k], b[k]) for k in DUMPED)


def test_full_run_adds_the_other_figures(capsys):
    d = _line(capsys, ARGS + ["--full", "--no-extra", "--no-cpu", "--profile-steps", "1"])
    assert all(k in d for k in HEADLINE)
    assert all(k in d for k in ("kernels_ms", "roofline", "pipeline", "consumer", "confirm_ms", "device_view_ms"))
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    assert d["kernels_ms"] and d["roofline"]["kernel"] in d["kernels_ms"]
    assert d["roofline"]["achievable_read_GBps"] > 0
