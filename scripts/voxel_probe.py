"""Numbers of the voxel-grid reduction of the scene cloud: on the 768x384 ground-truth rig, 4 views,
at voxel sizes room/64, room/256 and room/1024 (the room is 10 long), the wall time of acmmp_fusion_voxelize on the
resident scene result, of voxelize plus the download of the voxel cloud, and of what a user did before: the
download of the whole scene cloud plus the numpy restatement of the same reduction on the host.

    python scripts/voxel_probe.py OUT.json [--reps 30] [--host-reps 3]

Every timed path ends synchronised; the device paths alternate within one process after a warm-up; the shader
clock under load is probed before and after.  The device result is checked bit for bit against the restatement."""
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

from acmmp import capi, scene  # noqa: E402

ROOM = 10.0


def rig(W, H, n, seed=3):
    sc = scene.sphere_scene(W, H, n_src=n - 1, seed=seed)
    bgr = [np.repeat(np.asarray(im, np.uint8)[..., None], 3, 2) for im in sc.images]
    return np.array(sc.cameras), sc.extra["gt_depths"], sc.extra["gt_normals"], bgr


def stats(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
            "ms_p90": round(sorted(ms)[int(0.9 * (len(ms) - 1))], 4)}


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    import voxel_support as vs
    res = {"device": capi.device_identity(0), "clock_before": capi.clock_probe(0, 500.0)}
    cams, depths, normals, bgr = rig(768, 384, 4)
    fu = capi.Fusion(0, cams)
    for k in range(4):
        fu.set_view(k, depths[k], normals[k], bgr[k])
    refs, lists = list(range(4)), [[j for j in range(4) if j != k] for k in range(4)]
    total, _ = fu.run_scene(refs, lists)
    res["scene"] = {"rig": "768x384", "views": 4, "points": total, "cloud_bytes": 36 * total}
    res["wave_combine_ab"] = "not built"
    res["sizes"] = {}
    for div in (64, 256, 1024):
        size = ROOM / div
        n, info = fu.voxelize(size)
        cloud = fu.scene_points(0, total)
        want = vs.voxelize(cloud, size)
        got = fu.voxel_points(0, n, counts=True)
        same = bool(np.array_equal(got[0].view(np.uint32), want["points"].view(np.uint32)) and
                    np.array_equal(got[1], want["counts"]))
        paths = {"voxelize": lambda: fu.voxelize(size),
                 "voxelize_and_download": lambda: fu.voxel_points(0, fu.voxelize(size)[0], counts=True),
                 "download_scene_cloud": lambda: fu.scene_points(0, total)}
        for _ in range(3):
            for f in paths.values():
                f()
        ms = {k: [] for k in paths}
        for _ in range(a.reps):
            for k, f in paths.items():
                ms[k].append(timed(f))
        host = [timed(lambda: vs.voxelize(cloud, size)) for _ in range(a.host_reps)]
        today = [timed(lambda: vs.voxelize(fu.scene_points(0, total), size)) for _ in range(a.host_reps)]
        res["sizes"][f"room/{div}"] = {
            "voxel_size": size, "voxels": n, "n_rejected": info["n_rejected"], "points_per_voxel": round(total / max(n, 1), 2),
            "voxel_cloud_bytes": 40 * n, "bit_identical_to_restatement": same, "table": fu.voxel_table(0),
            "reps": a.reps, "host_reps": a.host_reps,
            **{k: stats(v) for k, v in ms.items()},
            "numpy_restatement_on_host": stats(host), "download_scene_cloud_and_numpy_restatement": stats(today)}
    fu.close()
    res["clock_after"] = capi.clock_probe(0, 500.0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
