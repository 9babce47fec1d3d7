"""bench.py's host side: a plain run is the default (``--full`` and ``--dump-outputs`` off), and a
workload's byte figures are those of its records."""

import bench
from tfr_reader import synth


def test_workload_sizes_are_those_of_its_records():
    buf, st, en = synth.framed(synth.c1_payloads(300) + synth.c3_payloads(2))
    w = bench.Workload("w", "w", buf, st, en, [(0, 302)])
    assert w.framed_bytes == int((en - st).sum()) == buf.size
    assert w.max_record == int((en - st).max())


def test_plain_run_is_the_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"
