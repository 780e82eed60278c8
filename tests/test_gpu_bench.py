"""bench.py end to end on a small instance of the metric's network: the JSON contract of the driver
(one line; metric / value / unit / n_gpus / steps / warmup / ms_per_step / scaling / dtype / config.workload),
with `--full` the `roofline` and `cpu_baseline` objects and the oracle check that the N = 1 run carries, and the
outputs `--dump-outputs` writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_bench_line_contract(dtype, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--sites", "12", "--bond", "64", "--replicas", "8", "--cpu-seconds", "0.5", "--dtype", dtype, "--full",
           "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in r, key
    assert r["unit"] == "contractions/s" and r["n_gpus"] == 1 and r["steps"] == 3 and r["warmup"] == 1
    assert r["higher_is_better"] is True and r["scaling"] == "weak" and r["vs_baseline"] is None
    assert r["dtype"] == dtype and r["value"] > 0 and "workload" in r["config"] and "model" not in r["config"]
    roof = r["roofline"]
    assert roof["bound"] in ("hbm", "mfma") and roof["unit"] in ("GB/s", "TFLOP/s")
    assert roof["peak"] == (157.3 if dtype == "f32" else 78.6)
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    cpu = r["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["value"] > 0 and cpu["cores"] >= 1 and cpu["sample"]
    assert cpu["parity_vs_gpu"]["ok"] is True          # replica 0 of this very run against the oracle
    # the dumped outputs are what the timed path returned: replica 0 and the last one are those the oracle checked
    t_hat, log_scale = np.load(tmp_path / "t_hat.npy"), np.load(tmp_path / "log_scale.npy")
    assert t_hat.shape == (8,) and t_hat.dtype == (np.float32 if dtype == "f32" else np.float64)
    assert log_scale.shape == (8,) and log_scale.dtype == np.float64
    for r_, pv in ((0, cpu["parity_vs_gpu"]), (7, cpu["parity_vs_gpu"]["last_replica"])):
        assert [float(t_hat[r_]), float(log_scale[r_])] == pv["gpu"]
    assert r["device"]["compute_units"] > 0
    if dtype == "f32":   # the secondaries ride on the fp32 line and never replace it
        b = r["batched_mps"]
        assert "error" not in b, b
        assert b["unit"] == "inputs/s" and b["value"] > 0 and b["scaling"] == "weak"
        assert b["epilogue_summed_steps"] == 12 - 2 and b["parity_vs_oracle_first_64_inputs"]["ok"] is True
        assert "peps_strong_scaling" in r
        # ... and the other BASELINE configs (round-3 verdict, item 2): known answers and definition checks inside the line
        cfgs = r["configs"]
        for name in ("cfg1", "cfg2", "cfg3b_B1024", "cfg4_i_cp_hyper", "cfg4_ii_tucker_dense_hub",
                     "cfg4_iii_tucker_delta_hub", "cfg4_iv_cp_wide_r4096"):
            assert name in cfgs and "error" not in cfgs[name], (name, cfgs.get(name))
        assert cfgs["cfg1"]["known_answer"]["ok"] is True and cfgs["cfg1"]["device_us_per_contraction"] > 0
        assert cfgs["cfg2"]["known_answer"]["ok"] is True and cfgs["cfg2"]["known_answer"]["log_scale_hex"] == "0x1.12a72fbccf574p+10"
        assert cfgs["cfg3b_B1024"]["workload"].endswith("B1024_per_gpu") and cfgs["cfg3b_B1024"]["value"] > 0
        x4 = cfgs["cfg3b_B1024_x4_in_flight"]         # four batches of 1024 as replicas of one launch sequence
        assert "error" not in x4 and x4["workload"].endswith("x4_batches_in_flight") and x4["value"] > 0, x4
        for name in ("cfg4_i_cp_hyper", "cfg4_ii_tucker_dense_hub", "cfg4_iii_tucker_delta_hub", "cfg4_iv_cp_wide_r4096"):
            assert cfgs[name]["spot_check_vs_definition_f64"]["ok"] is True and 0 < cfgs[name]["frac_of_mfma_peak"] < 1
        # the hyperedge route and the materialised delta hub give the same entry (same factor matrices)
        a, b_ = cfgs["cfg4_i_cp_hyper"]["spot_check_vs_definition_f64"], cfgs["cfg4_iii_tucker_delta_hub"]["spot_check_vs_definition_f64"]
        assert a["want"] == b_["want"] and abs(a["got"] - b_["got"]) <= 1e-3 * abs(a["want"]) + 1e-9


def test_bench_plain_run_is_the_headline_alone(tmp_path):
    """A plain run (no `--full`): the headline keys and none of the extra measurements; `--steps` sets the timed
    steps, and `--dump-outputs` writes the last timed step's results, the same in a second run with the same arguments
    (seeded inputs)."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
           "--sites", "12", "--bond", "64", "--replicas", "8"]
    dumps = []
    for run in ("a", "b"):
        out = subprocess.run(cmd + ["--dump-outputs", str(tmp_path / run)], capture_output=True, text=True, timeout=600,
                             cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out.stdout
        r = json.loads(lines[0])
        assert r["unit"] == "contractions/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
        assert r["steps"] == 4 and r["warmup"] == 1 and r["value"] > 0
        assert abs(r["ms_per_step"] - 8 * 1e3 / r["value"]) <= 1e-3 * r["ms_per_step"] + 1e-3
        assert r["metric"].startswith("contractions/sec (MPS-12 overlap, bond=64")
        for key in ("roofline", "cpu_baseline", "latency", "device", "batched_mps", "peps_strong_scaling", "configs"):
            assert key not in r, key
        dumps.append((np.load(tmp_path / run / "t_hat.npy"), np.load(tmp_path / run / "log_scale.npy")))
    (t_a, c_a), (t_b, c_b) = dumps
    assert t_a.shape == (8,) and t_a.dtype == np.float32 and c_a.shape == (8,) and c_a.dtype == np.float64
    assert np.all(np.abs(t_a) == 1.0) and np.all(np.isfinite(c_a))      # closed networks: (sign, log|value|)
    np.testing.assert_array_equal(t_a, t_b)
    np.testing.assert_allclose(c_a, c_b, rtol=0, atol=1e-4)
