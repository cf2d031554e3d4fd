"""Numbers of the cleaning of the voxel cloud: on the 768x384 ground-truth rig, 4 views, at voxel sizes
room/64, room/256 and room/1024 (the room is 10 long), the wall time of acmmp_fusion_voxel_clean on the resident
voxel result at connectivity 26 and 6, its rounds, and the download of the clean cloud; beside them voxelize alone on
the same build, the download of the whole voxel cloud, and what a user did before: that download plus the filter on
the host.  The host filter here is the tests' sequential restatement, an untuned Python dict and union-find, so the
ratio to it is an upper bound on what the device pass saves against a tuned host library.

    python scripts/voxel_clean_probe.py OUT.json [--reps 30] [--host-reps 1]

Every timed path ends synchronised; the device paths alternate within one process after a warm-up; the shader
clock under load is probed before and after.  The device result is checked against the restatement."""
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
THRESHOLDS = (1, 10, 1)             # min_neighbours, min_component_voxels, min_component_points


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
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    import voxel_clean_support as cs
    import voxel_support as vs
    res = {"device": capi.device_identity(0), "clock_before": capi.clock_probe(0, 500.0),
           "note": "host_restatement is an untuned Python dict + union-find: device-to-host ratios are upper bounds",
           "thresholds": dict(zip(("min_neighbours", "min_component_voxels", "min_component_points"), THRESHOLDS))}
    cams, depths, normals, bgr = rig(768, 384, 4)
    fu = capi.Fusion(0, cams)
    for k in range(4):
        fu.set_view(k, depths[k], normals[k], bgr[k])
    refs, lists = list(range(4)), [[j for j in range(4) if j != k] for k in range(4)]
    total, _ = fu.run_scene(refs, lists)
    cloud = fu.scene_points(0, total)
    res["scene"] = {"rig": "768x384", "views": 4, "points": total}
    res["sizes"] = {}
    for div in (64, 256, 1024):
        size = ROOM / div
        nv, _ = fu.voxelize(size)
        vox = vs.voxelize(cloud, size)
        entry = {"voxel_size": size, "voxels": nv, "reps": a.reps, "host_reps": a.host_reps}
        kept = {}

        def clean_and_download(conn):
            n, _ = fu.voxel_clean(conn, *THRESHOLDS)
            return fu.clean_points(0, n, counts=True, component=True)
        paths = {"voxelize": lambda: fu.voxelize(size),
                 "download_voxel_cloud": lambda: fu.voxel_points(0, nv, counts=True)}
        for conn in (26, 6):
            paths[f"voxel_clean_{conn}"] = lambda conn=conn: kept.__setitem__(conn, fu.voxel_clean(conn, *THRESHOLDS))
            paths[f"voxel_clean_{conn}_and_download"] = lambda conn=conn: clean_and_download(conn)
        for _ in range(3):
            for f in paths.values():
                f()
        ms = {k: [] for k in paths}
        for _ in range(a.reps):
            for k, f in paths.items():
                ms[k].append(timed(f))
        entry.update({k: stats(v) for k, v in ms.items()})
        for conn in (26, 6):
            n, info = kept[conn]
            host = [timed(lambda: cs.clean(vox["keys"], vox["counts"], conn, *THRESHOLDS)) for _ in range(a.host_reps)]
            want = cs.clean(vox["keys"], vox["counts"], conn, *THRESHOLDS)
            fu.voxel_clean(conn, *THRESHOLDS)
            lab, sup = fu.voxel_labels(0, nv)
            same = bool(n == len(want["kept"]) and np.array_equal(lab, want["label"]) and np.array_equal(sup, want["support"]))
            entry[f"connectivity_{conn}"] = {"kept": n, **info, "clean_cloud_bytes": 48 * n, "equal_to_restatement": same,
                                            "host_restatement": stats(host)}
        entry["download_voxel_cloud_and_host_restatement_26_ms"] = round(
            entry["download_voxel_cloud"]["ms_median"] + entry["connectivity_26"]["host_restatement"]["ms_median"], 3)
        res["sizes"][f"room/{div}"] = entry
    fu.close()
    res["clock_after"] = capi.clock_probe(0, 500.0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
