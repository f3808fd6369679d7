"""bench.py's output contract on the GPU: one JSON line on stdout with the driver's keys, whatever
native libraries print (a short run: one timed pass, no extra legs)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "render_wall_ms", "bit_exact_vs_oracle"}
CORNELL = ("cornell.scene", 256, 256, 64, 4, True, True)     # bench.py CONFIGS["cornell"]


def test_bench_prints_one_json_line():
    out = subprocess.run([sys.executable, "bench.py", "--scene", "cornell", "--steps", "2", "--warmup", "1",
                          "--no-extras"], cwd=REPO, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert KEYS <= set(rec), KEYS - set(rec)
    assert rec["n_gpus"] == 1 and rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["higher_is_better"] is True
    assert rec["unit"] == "Mrays/s" and rec["dtype"] == "f32" and rec["scaling"] in ("weak", "strong")
    assert isinstance(rec["config"], dict) and "workload" in rec["config"]


def test_bench_plain_run_dumps_the_timed_steps_outputs(tmp_path):
    """A plain `--gpus 1 --steps K --warmup W` run (no --full) leaves the moved legs' fields null, and
    --dump-outputs writes the framebuffer the K timed passes accumulated: bit for bit the oracle's passes 0..K-1."""
    import numpy as np
    import oracle_lib as O
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--scene", "cornell", "--steps", "2", "--warmup",
                          "1", "--dump-outputs", str(tmp_path)], cwd=REPO, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert KEYS <= set(rec), KEYS - set(rec)
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["roofline"] is None and rec["cpu_baseline"] is None and rec["bit_exact_vs_oracle"] is None
    scene_file, W, H, spp, bounces, sort, use_bvh = CORNELL
    ref, st = O.OracleScene(os.path.join(O.ASSETS, scene_file), use_bvh=use_bvh, image=(W, H, spp, bounces)).render(
        sort=sort, pass_begin=0, pass_count=2)
    fb = np.load(tmp_path / "framebuffer.npy")
    assert fb.dtype == np.float32 and fb.shape == (W * H * 3,)
    assert np.array_equal(fb, ref)
    counts = dict(zip(("passes", "generated_rays", "live_segments"), np.load(tmp_path / "work_counts.npy")))
    assert counts["passes"] == 2 and counts["live_segments"] == st["live_segments"]
