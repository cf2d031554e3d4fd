"""Numbers of the visibility check of the voxel cloud: on the 768x384 ground-truth rig, 4 views, at
voxel sizes room/64, room/256 and room/1024 (the room is 10 long), the wall time of acmmp_fusion_voxel_visibility on
the resident voxel result over all four views at radius 0 and 1, and the download of the visible cloud; beside them
what a user did before: the download of the voxel cloud and of the four depth maps, plus the check on the host.  The
host check here is the tests' sequential restatement -- one ctypes call into the oracle per entry and view for the
projection, numpy for the comparisons -- which is untuned, so the ratio to it is an upper bound on what the device pass
saves against a tuned host library.

    python scripts/voxel_visibility_probe.py OUT.json [--reps 30]

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
REL_TOL = 0.01
THRESHOLDS = (1, 0)                 # min_support, max_conflicts


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
    a = ap.parse_args()
    import visibility_support as vis
    res = {"device": capi.device_identity(0), "clock_before": capi.clock_probe(0, 500.0),
           "note": "host_restatement is untuned (a ctypes call per entry and view, then numpy): device-to-host ratios "
                   "are upper bounds",
           "rel_tol": REL_TOL, "thresholds": dict(zip(("min_support", "max_conflicts"), THRESHOLDS))}
    cams, depths, normals, bgr = rig(768, 384, 4)
    fu = capi.Fusion(0, cams)
    for k in range(4):
        fu.set_view(k, depths[k], normals[k], bgr[k])
    views = list(range(4))
    total, _ = fu.run_scene(views, [[j for j in views if j != k] for k in views])
    res["scene"] = {"rig": "768x384", "views": 4, "points": total}
    P = depths[0].size
    res["sizes"] = {}
    for div in (64, 256, 1024):
        size = ROOM / div
        nv, _ = fu.voxelize(size)
        entry = {"voxel_size": size, "voxels": nv, "reps": a.reps, "depth_map_bytes": 4 * P * len(views)}
        kept = {}
        paths = {"download_voxel_cloud": lambda: fu.voxel_points(0, nv, counts=True)}
        for radius in (0, 1):
            def run(radius=radius):
                kept[radius] = fu.voxel_visibility(views, REL_TOL, radius, *THRESHOLDS)

            def run_and_download(radius=radius):
                n, _ = fu.voxel_visibility(views, REL_TOL, radius, *THRESHOLDS)
                return fu.visible_points(0, n, counts=True, tallies=True)
            paths[f"voxel_visibility_r{radius}"] = run
            paths[f"voxel_visibility_r{radius}_and_download"] = run_and_download
        for _ in range(3):
            for f in paths.values():
                f()
        ms = {k: [] for k in paths}
        for _ in range(a.reps):
            for k, f in paths.items():
                ms[k].append(timed(f))
        entry.update({k: stats(v) for k, v in ms.items()})
        # the host path, once: the voxel cloud (timed above), the projection, and per radius the comparisons
        pts = fu.voxel_points(0, nv)
        proj = [None]
        entry["host_projection_ms"] = round(timed(lambda: proj.__setitem__(0, vis.project(cams, pts[:, :3]))), 3)
        for radius in (0, 1):
            want = [None]
            host = timed(lambda: want.__setitem__(0, vis.visibility(cams, depths, pts, views, REL_TOL, radius, *THRESHOLDS,
                                                                    proj=proj[0])))
            n, info = fu.voxel_visibility(views, REL_TOL, radius, *THRESHOLDS)
            tal = fu.visibility_tallies(0, nv)
            same = bool(n == len(want[0]["kept"]) and np.array_equal(tal, want[0]["tallies"]) and
                        info["class_totals"] == want[0]["class_totals"])
            entry[f"radius_{radius}"] = {"kept": n, **info, "visible_cloud_bytes": 52 * n, "equal_to_restatement": same,
                                         "host_restatement_ms": round(entry["host_projection_ms"] + host, 3)}
        res["sizes"][f"room/{div}"] = entry
    fu.close()
    # the four depth maps to the host, as the host path needs them: device copies of them, read back
    bufs = [capi.DeviceBuffer(0, d.shape) for d in depths]
    for buf, d in zip(bufs, depths):
        buf.upload(d)

    def download_depths():
        return [buf.download() for buf in bufs]
    for _ in range(3):
        download_depths()
    res["download_depth_maps"] = stats([timed(download_depths) for _ in range(a.reps)])
    for buf in bufs:
        buf.free()
    for entry in res["sizes"].values():
        for radius in (0, 1):
            entry[f"radius_{radius}"]["host_path_ms"] = round(
                entry["download_voxel_cloud"]["ms_median"] + res["download_depth_maps"]["ms_median"] +
                entry[f"radius_{radius}"]["host_restatement_ms"], 3)
    res["clock_after"] = capi.clock_probe(0, 500.0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
