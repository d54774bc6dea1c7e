"""CPU: bench.py's command line (a plain run times the headline figure only; --full adds the other measurements) and what
--dump-outputs writes: the accumulator of the timed steps, or a fixed, seeded sample of it when it exceeds the size limit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_full_is_off_by_default_and_steps_are_taken_as_given():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert not a.full and a.steps == 7 and a.warmup == 3 and a.dump_outputs == ""
    b = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert b.full and b.dump_outputs == "out"


def test_dump_outputs_writes_the_accumulator_or_a_fixed_sample(tmp_path, monkeypatch):
    acc = np.random.default_rng(0).random((6, 10, 4), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "whole"), acc)
    got = np.load(tmp_path / "whole" / "accumulator.npy")
    assert got.dtype == np.float32 and np.array_equal(got, acc)

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", acc.nbytes - 1)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_PIXELS", 16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), acc)
    assert not os.path.exists(tmp_path / "a" / "accumulator.npy")
    s, pix = np.load(tmp_path / "a" / "accumulator_sample.npy"), np.load(tmp_path / "a" / "accumulator_sample_pixel.npy")
    assert s.dtype == np.float32 and s.shape == (16, 4) and pix.dtype == np.float64
    assert np.all(np.diff(pix) > 0) and np.array_equal(s, acc.reshape(-1, 4)[pix.astype(np.int64)])
    # the same sample every run
    assert np.array_equal(pix, np.load(tmp_path / "b" / "accumulator_sample_pixel.npy"))
    assert np.array_equal(s, np.load(tmp_path / "b" / "accumulator_sample.npy"))
