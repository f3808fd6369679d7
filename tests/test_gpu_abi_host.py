"""The C ABI as a plain C++ host binds it (round 6, verdict r05 item 2): tests/native/abi_host links librtamd.so
and calls rt_scene_load + rt_render the way the reference's main calls load_scene + gpu_raytrace
(raytracing.cu:344-358), with no GPU_MAX_HW_QUEUES and no RTAMD_* variable in its environment.
The library's constructor then asks HIP for the hardware queues its 20 pass streams need, so the drop-in runs at
the benchmark's speed (on HIP's default 4 queues 20 pass streams share queues and a pass takes ~2x as long), and
pass 0 of the BASELINE teapot frame equals the oracle's (tests/golden/bench_pass0.json)."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "tests", "native", "build", "abi_host")


def test_cpp_host_default_environment(tmp_path):
    import rtamd as R
    gold = json.load(open(os.path.join(REPO, "tests", "golden", "bench_pass0.json")))["teapot sort=on"]
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES" and not k.startswith("RTAMD_")}
    fb_path = str(tmp_path / "pass0.bin")
    out = subprocess.run([EXE, os.path.join(R.ASSETS, "teapot.scene"), R.ASSETS, "1920", "1080", "2048", "16", "20",
                          "2", fb_path], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    print("\n".join(json.dumps(x) for x in lines))
    runs = [x for x in lines if "rep" in x]
    assert len(runs) == 2 and all(r["passes"] == 20 and r["gpu_max_hw_queues"] == "24" for r in runs)
    # 20 passes of 41.5 M rays x 16 bounces: the default-queue cliff is ~11 ms/pass, the benchmark ~5.9
    assert runs[-1]["ms_per_pass"] < 8.0, runs
    # rt_trace_rays with index_out == nullptr and with stats == nullptr both returned RT_OK
    assert [x for x in lines if "trace_rays_null_outputs" in x] == [{"trace_rays_null_outputs": True, "live_segments": 1}]
    fb = np.fromfile(fb_path, dtype="<f4")
    assert fb.size == 1920 * 1080 * 3
    assert hashlib.sha256(fb.tobytes()).hexdigest() == gold["sha256"]
