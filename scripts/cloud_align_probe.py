"""Numbers of the device ICP: cloud_distance_probe's synthetic surface clouds, about 1e5, 1e6 and 4e6
points per side, the data cloud moved by a small known rigid motion; one K-iteration acmmp_fusion_cloud_align against K
back-to-back acmmp_fusion_cloud_distance calls on the same clouds -- what a caller had to do for the correspondences of
K iterations before the align call existed: the grid rebuilt each time, d2 and nearest written each time (the host fit
and the transform of the cloud, which that caller also had to do, are not counted).

    python scripts/cloud_align_probe.py OUT.json [--reps 5] [--iterations 10] [--sizes 100000 1000000 4000000]

Every timed path ends synchronised; the two alternate within one process after a warm-up and the median is reported; the
shader clock under load is probed before and after."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from cloud_distance_probe import SPHERES, _camera, as_points, capi, stats, surface_cloud, timed  # noqa: E402


def small_motion():
    """(3, 4): one degree about (1, 2, 3) through the origin, then a shift of a few millimetres of the unit sphere."""
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    t = np.radians(1.0)
    M = np.zeros((3, 4))
    M[:, :3] = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    M[:, 3] = (0.004, -0.003, 0.002)
    return M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000, 4_000_000])
    a = ap.parse_args()
    K = a.iterations
    res = {"device": capi.device_identity(0), "clock_before": capi.clock_probe(0, 500.0), "spheres": len(SPHERES),
           "reps": a.reps, "iterations": K, "sizes": {}}
    known = small_motion()
    inv = np.zeros((3, 4))
    inv[:, :3] = known[:, :3].T
    inv[:, 3] = -known[:, :3].T @ known[:, 3]
    for n in a.sizes:
        ref = surface_cloud(n, 2)
        x = surface_cloud(n, 1).astype(np.float64)
        data = (x @ inv[:, :3].T + inv[:, 3]).astype(np.float32)
        # the cap: the largest displacement of the motion over the scene and a few spacings, so that the first
        # iteration's pairs are mostly the right ones
        spacing = np.sqrt(4 * np.pi * sum(s[3] ** 2 for s in SPHERES) / n)
        max_dist = float(np.float32(0.06 + 4.0 * spacing))
        fu = capi.Fusion(0, _camera())
        fu.set_scene(as_points(data))
        fu.set_reference_cloud(ref)
        out = {}

        def align():
            out["align"] = fu.cloud_align("scene", "rigid", max_dist, K)

        def distances():
            for _ in range(K):
                out["distance"] = fu.cloud_distance("scene", "data_to_ref", max_dist)
        align()
        distances()
        t = {"align": [], "distances": []}
        for _ in range(a.reps):
            t["align"].append(timed(align))
            t["distances"].append(timed(distances))
        r = out["align"]
        entry = {"points_per_side": n, "max_dist": max_dist, "align": stats(t["align"]), "distances": stats(t["distances"]),
                 "iterations_run": r.iterations, "stop_reason": r.stop_reason,
                 "n_matched": [rec.n_matched for rec in r.records], "mean": [rec.mean for rec in r.records],
                 "error_max_abs": float(np.abs(r.M - known).max()), **fu.distance_grid()}
        entry["distances_over_align"] = round(entry["distances"]["ms_median"] / entry["align"]["ms_median"], 3)
        entry["ms_per_iteration"] = round(entry["align"]["ms_median"] / max(r.iterations, 1), 4)
        fu.close()
        res["sizes"][str(n)] = entry
        print(n, json.dumps(entry), flush=True)
    res["clock_after"] = capi.clock_probe(0, 500.0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
