"""bench.py's plain run and its --dump-outputs: a plain run times the steps and prints the
headline line with every secondary leg (--full) left out; --dump-outputs writes what the last
timed step computed as float32 .npy files; the inputs are seeded, the same in every run.
One small pix2pix configuration (bs2) in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECONDARY = ("graph_equals_eager", "core", "fp32_exact", "roofline", "cpu_baseline")


def _plain_run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--batch", "2", "--dump-outputs", str(out_dir)],
                       cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@gpu
def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    out = _plain_run(tmp_path / "a")
    assert out["steps"] == 3 and out["warmup"] == 2
    assert out["unit"] == "images/s" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: 2 images per step
    assert abs(out["value"] - 2 / (out["ms_per_step"] * 1e-3)) <= 0.01 * out["value"]
    for k in SECONDARY:
        assert out[k] is None, (k, out[k])
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(a) == ["d_params", "g_params", "gen_output", "losses"]
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k, v in a.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
    assert a["gen_output"].shape == (2, 256, 256, 3)
    assert np.allclose(a["losses"], out["losses"], rtol=0, atol=1e-6)   # the line rounds to 6 places


def test_bench_inputs_are_seeded():
    """The same arguments give the same batch in every run (CPU: the host-side generator)."""
    sys.path.insert(0, REPO)
    import bench
    for model in ("pix2pix", "srgan"):
        wl = dict(bench.WORKLOADS[model], size=32)
        x0, y0 = bench.synthetic_batch(wl, 2, seed=1000)
        x1, y1 = bench.synthetic_batch(wl, 2, seed=1000)
        assert np.array_equal(x0, x1) and np.array_equal(y0, y1)
        assert x0.shape == (2, 32 // wl["scale"], 32 // wl["scale"], 3) and y0.shape == (2, 32, 32, 3)
