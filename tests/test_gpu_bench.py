"""A plain bench.py run on the GPU: the result line's headline fields, no side measurement, and
--dump-outputs = what a caller of the timed path receives from its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_bitwise_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, V, STEPS, SEED = 160, 96, 2, 2, 1234          # more than one block per half-sweep, H no multiple of 32


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path, gpu_ctx_factory):
    from acmmp import scene, types
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "1", "--width", str(W), "--height", str(H), "--n-src", str(V),
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["metric"].startswith("Mpixels/sec PatchMatch propagation") and line["unit"] == "Mpixel-iterations/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["steps"] == STEPS
    assert line["ms_per_step"] > 0
    # value is the timed region's rate: pixel-iterations of the steps over steps x ms_per_step (3 decimals each)
    assert line["value"] == pytest.approx(W * H * 3 / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    for k in ("other_math_mode", "ms_per_depth_map", "pcie_inclusive", "clock", "cpu_baseline",
              "nondegenerate_variant", "end_to_end", "depth_exchange", "band_split"):
        assert line[k] is None, k

    assert sorted(os.listdir(out)) == ["costs.npy", "planes.npy"]
    planes, costs = np.load(out / "planes.npy"), np.load(out / "costs.npy")
    assert planes.dtype == np.float32 and planes.shape == (H, W, 4)
    assert costs.dtype == np.float32 and costs.shape == (H, W)
    # the same view, parameters, math mode and last step's seed through the C ABI directly
    sc = scene.sphere_scene(W, H, n_src=V, seed=SEED)
    c0 = sc.cameras[0]
    p = types.default_params(num_images=V + 1, max_iterations=3, depth_min=float(c0["depth_min"]) * 0.6,
                             depth_max=float(c0["depth_max"]) * 1.2)
    with gpu_ctx_factory() as ctx:
        ctx.set_math("fast")
        ctx.set_params(p)
        ctx.upload_views(sc.images, sc.cameras)
        ctx.run_patchmatch(SEED + STEPS - 1)
        want_p, want_c = ctx.download()
    # the dump holds finite numbers only: a NaN cost is written as -1, a non-finite plane component as 0
    assert np.isfinite(planes).all() and np.isfinite(costs).all()
    assert_bitwise_equal(planes, np.where(np.isfinite(want_p), want_p, np.float32(0)), "dumped planes")
    assert_bitwise_equal(costs, np.where(np.isfinite(want_c), want_c, np.float32(-1)), "dumped costs")
