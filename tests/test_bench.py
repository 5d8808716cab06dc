"""bench.py's command line: a plain run prints the headline only, --full adds the measurements that need runs of their
own, --dump-outputs writes what the last timed step computed (same arguments -> same inputs -> comparable files)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "step_roofline", "kernels", "layers", "cpu_baseline")


def _bench(*args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), capture_output=True, text=True,
                       timeout=timeout)
    return r


def test_dump_outputs_stays_within_its_budget_with_a_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 20000)
    rng = np.random.default_rng(1)
    arrays = {"loss": np.array(3.5, np.float64), "small": rng.random(100, dtype=np.float32),
              "big": rng.random((4, 3, 40, 40), dtype=np.float32), "bigger": rng.random((8, 3, 40, 40), dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "bigger.npy", "loss.npy", "small.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 20000
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert got["loss"] == 3.5 and got["loss"].dtype == np.float64
    np.testing.assert_array_equal(got["small"], arrays["small"])            # fits: kept whole
    for name in ("big", "bigger"):                                         # too large: a sample of its own elements
        assert got[name].ndim == 1 and 0 < got[name].size < arrays[name].size
        assert np.isin(got[name], arrays[name].reshape(-1)).all()
        np.testing.assert_array_equal(got[name], np.load(tmp_path / "b" / (name + ".npy")))
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "c"), {"i": np.arange(4)})


@pytest.mark.parametrize("args,message", [(["--layers"], "--full"), (["--profile-kernels"], "--full"),
                                          (["--steps", "0"], "--steps")])
def test_bench_refuses_flags_it_cannot_honour(args, message):
    r = _bench(*args, timeout=300)
    assert r.returncode != 0 and message in r.stderr, r.stderr[-2000:]


SMALL = ["--size", "64", "--views", "2", "--warmup", "1"]


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_same_outputs_twice(tmp_path):
    lines = []
    for d in ("a", "b"):
        r = _bench(*SMALL, "--steps", "3", "--dump-outputs", str(tmp_path / d))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(out) == 1, r.stdout
        lines.append(json.loads(out[0]))
    line = lines[0]
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY), sorted(line)
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert lines[1]["final_loss"] == line["final_loss"]
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["loss.npy", "rendered.npy", "texture.npy", "texture_grad.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 10 ** 6
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), f
        np.testing.assert_array_equal(x, y, err_msg=f)          # seeded inputs, deterministic kernels: the same outputs
    assert np.load(tmp_path / "a" / "loss.npy") == line["final_loss"]
    assert np.load(tmp_path / "a" / "rendered.npy").shape == (2, 3, 64, 64)
    assert np.load(tmp_path / "a" / "texture.npy").shape == np.load(tmp_path / "a" / "texture_grad.npy").shape == (1, 64, 64, 3)


@pytest.mark.gpu
def test_full_run_adds_the_kernel_roofline_and_cpu_figures():
    r = _bench(*SMALL, "--steps", "2", "--full", "--layers")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])
    assert all(k in line for k in HEADLINE + FULL_ONLY), sorted(line)
    assert line["cpu_baseline"].get("value"), line["cpu_baseline"]
    assert 0 < line["roofline"]["frac"] <= 1 and 0 < line["step_roofline"]["frac"] <= 1
    assert any(f.startswith("conv") for f in line["kernels"]) and line["layers"]
