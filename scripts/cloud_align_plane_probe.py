"""Numbers of the point-to-plane device ICP: cloud_align_probe's clouds, caps and known motion; one
K-iteration acmmp_fusion_cloud_align_plane against one K-iteration rigid acmmp_fusion_cloud_align from the same start,
alternated within one process; per size the two times, the per-iteration ratio, and for both the matched mean after K
iterations and the distance of the transform from the known motion.  The data cloud's normals are those of the sphere
each point was sampled from (the direction from the centre of the sphere whose surface is nearest), moved with the cloud.

    python scripts/cloud_align_plane_probe.py OUT.json [--reps 5] [--iterations 10] [--sizes 100000 1000000 4000000]

Every timed path ends synchronised; the median of the repetitions after a warm-up is reported; the shader clock under
load is probed before and after."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from cloud_align_probe import small_motion  # noqa: E402
from cloud_distance_probe import SPHERES, _camera, as_points, capi, stats, surface_cloud, timed  # noqa: E402


def sphere_normals(x):
    """(n, 3) float64: for each point the unit direction from the centre of the sphere whose surface is nearest."""
    x = np.asarray(x, np.float64)
    best = np.full(len(x), np.inf)
    out = np.zeros((len(x), 3))
    for cx, cy, cz, r in SPHERES:
        d = x - (cx, cy, cz)
        length = np.linalg.norm(d, axis=1)
        off = np.abs(length - r)
        take = off < best
        out[take] = d[take] / length[take, None]
        best[take] = off[take]
    return out


def corner_error(M, known, lo, hi):
    """The largest distance between M c' and known c' over the eight corners of the box [lo, hi]."""
    worst = 0.0
    for k in range(8):
        c = np.array([hi[a] if k >> a & 1 else lo[a] for a in range(3)], np.float64)
        worst = max(worst, float(np.linalg.norm((M[:, :3] @ c + M[:, 3]) - (known[:, :3] @ c + known[:, 3]))))
    return worst


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
        pts = as_points((x @ inv[:, :3].T + inv[:, 3]).astype(np.float32))
        pts[:, 3:6] = (sphere_normals(x) @ inv[:, :3].T).astype(np.float32)
        spacing = np.sqrt(4 * np.pi * sum(s[3] ** 2 for s in SPHERES) / n)
        max_dist = float(np.float32(0.06 + 4.0 * spacing))             # cloud_align_probe's cap
        fu = capi.Fusion(0, _camera())
        fu.set_scene(pts)
        fu.set_reference_cloud(ref)
        out = {}

        def plane():
            out["plane"] = fu.cloud_align_plane("scene", max_dist, K)

        def point():
            out["point"] = fu.cloud_align("scene", "rigid", max_dist, K)
        plane()
        point()
        t = {"plane": [], "point": []}
        for _ in range(a.reps):
            t["plane"].append(timed(plane))
            t["point"].append(timed(point))
        lo, hi = ref.min(0).astype(np.float64), ref.max(0).astype(np.float64)
        entry = {"points_per_side": n, "max_dist": max_dist}
        for name in ("plane", "point"):
            r = out[name]
            after = fu.cloud_align("scene", "rigid", max_dist, 1, init=r.M).records[0]      # the matched mean under the result
            entry[name] = dict(stats(t[name]), iterations_run=r.iterations, stop_reason=r.stop_reason,
                               ms_per_iteration=round(stats(t[name])["ms_median"] / max(r.iterations, 1), 4),
                               mean=[rec.mean for rec in r.records], mean_after=after.mean, n_matched_after=after.n_matched,
                               error_max_abs=float(np.abs(r.M - known).max()), corner_error=corner_error(r.M, known, lo, hi))
        entry["plane"]["rms_plane"] = [rec.rms_plane for rec in out["plane"].records]
        entry["plane"]["n_no_normal"] = out["plane"].records[-1].n_no_normal
        entry["per_iteration_ratio"] = round(entry["plane"]["ms_per_iteration"] / entry["point"]["ms_per_iteration"], 3)
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
