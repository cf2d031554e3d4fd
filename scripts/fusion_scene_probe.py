"""Numbers of the whole-scene fusion: the unique / plain point ratio on the 256x128
ground-truth rig and on a small_dataset pipeline run, and the wall time of a plain acmmp_fusion_run_scene
against the per-view acmmp_fusion_run loop over the same views of the 768x384 rig.

    python scripts/fusion_scene_probe.py OUT.json [--reps 40]

Both timed paths end synchronised (the loop copies every view's points to the host, run_scene leaves them in
HBM; `scene_and_download` adds the copy of the whole cloud) and alternate within one process after a warm-up;
the shader clock under load is probed before and after."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "acmmp-spherical_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

from acmmp import capi, pipeline, scene  # noqa: E402


def rig(W, H, n, seed=3):
    sc = scene.sphere_scene(W, H, n_src=n - 1, seed=seed)
    bgr = [np.repeat(np.asarray(im, np.uint8)[..., None], 3, 2) for im in sc.images]
    return np.array(sc.cameras), sc.extra["gt_depths"], sc.extra["gt_normals"], bgr


def fusion_of(cams, depths, normals, bgr):
    fu = capi.Fusion(0, cams)
    for k in range(len(cams)):
        fu.set_view(k, depths[k], normals[k], bgr[k])
    return fu


def ratio(fu, n):
    refs, lists = list(range(n)), [[j for j in range(n) if j != k] for k in range(n)]
    plain, pc = fu.run_scene(refs, lists)
    fu.reset_used()
    uniq, uc = fu.run_scene(refs, lists, unique=True)
    return {"plain_points": plain, "unique_points": uniq, "ratio": round(uniq / max(plain, 1), 4),
            "plain_counts": pc.tolist(), "unique_counts": uc.tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=40)
    a = ap.parse_args()
    res = {"device": capi.device_identity(0), "clock_before": capi.clock_probe(0, 500.0)}

    fu = fusion_of(*rig(256, 128, 4))
    res["ratio_rig_256x128_4views"] = ratio(fu, 4)
    fu.close()

    from pipeline_support import small_dataset
    ds = small_dataset(64, 32, 3)
    pipe = pipeline.Pipeline(ds, order="reference", geom_iterations=1).run()
    plain = pipe.run_fusion()
    uniq = pipe.run_fusion(unique=True)
    res["ratio_small_dataset_64x32_3views"] = {"plain_points": int(plain.shape[0]), "unique_points": int(uniq.shape[0]),
                                               "ratio": round(uniq.shape[0] / max(plain.shape[0], 1), 4)}

    cams, depths, normals, bgr = rig(768, 384, 4)
    fu = fusion_of(cams, depths, normals, bgr)
    refs, lists = list(range(4)), [[j for j in range(4) if j != k] for k in range(4)]

    def loop():
        return sum(fu.run(k, lists[k]).shape[0] for k in refs)

    def scene_only():
        return fu.run_scene(refs, lists)[0]

    def scene_and_download():
        total, _ = fu.run_scene(refs, lists)
        return fu.scene_points(0, total).shape[0]

    paths = {"per_view_loop": loop, "run_scene": scene_only, "scene_and_download": scene_and_download}
    points = {k: f() for k, f in paths.items()}
    for _ in range(5):
        for f in paths.values():
            f()
    ms = {k: [] for k in paths}
    for _ in range(a.reps):
        for k, f in paths.items():
            t0 = time.perf_counter()
            f()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    res["timing_rig_768x384_4views"] = {
        "points": points, "reps": a.reps,
        "ms_median": {k: round(statistics.median(v), 4) for k, v in ms.items()},
        "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
        "ms_p90": {k: round(sorted(v)[int(0.9 * (len(v) - 1))], 4) for k, v in ms.items()}}
    fu.close()
    res["clock_after"] = capi.clock_probe(0, 500.0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
