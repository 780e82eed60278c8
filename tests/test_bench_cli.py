"""bench.py's options without a GPU: a plain run is the default, `--dump-steps` needs `--full`, and `--dump-outputs`
writes float32 / float64 arrays."""
import sys

import numpy as np
import pytest

import bench


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse_args()
    assert args.full is False and args.dump_outputs is None and args.steps == 7 and args.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    args = bench.parse_args()
    assert args.full is True and args.dump_outputs == "out"


def test_dump_steps_needs_full(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--dump-steps", "steps.json"])
    with pytest.raises(SystemExit) as exc:
        bench.parse_args()
    assert exc.value.code == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-steps", "steps.json"])
    assert bench.parse_args().dump_steps == "steps.json"


def test_dump_outputs_writes_float32_or_float64(tmp_path):
    t_hat = np.array([1.0, -1.0, 1.0], dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "out"), t_hat=t_hat, log_scale=[3.5, 2.25, 1.0], count=np.arange(3))
    got = {name: np.load(tmp_path / "out" / f"{name}.npy") for name in ("t_hat", "log_scale", "count")}
    assert got["t_hat"].dtype == np.float32 and np.array_equal(got["t_hat"], t_hat)
    assert got["log_scale"].dtype == np.float64 and np.array_equal(got["log_scale"], [3.5, 2.25, 1.0])
    assert got["count"].dtype == np.float64 and np.array_equal(got["count"], [0.0, 1.0, 2.0])
