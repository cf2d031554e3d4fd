"""Numbers of the nearest-neighbour cloud distances: two synthetic surface clouds -- points on a few
spheres with noise, about 1e5, 1e6 and 4e6 points per side -- measured against each other in both directions at the
automatic cell: the wall time of acmmp_fusion_cloud_distance, queries per second, the largest ring searched and the
longest cell list; beside them the same query on the host, the comparator of record: scipy.spatial.cKDTree (build and
query, capped at max_dist) where scipy can be imported, else the tests' numpy all-pairs restatement at the smallest size
only.  Where the host runs, the device's nearest indices and distances are checked against it.

    python scripts/cloud_distance_probe.py OUT.json [--reps 9] [--sizes 100000 1000000 4000000]

Every timed path ends synchronised (the call returns the summary); the two directions alternate within one process
after a warm-up and the median is reported; the shader clock under load is probed before and after."""
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

from acmmp import capi  # noqa: E402

SPHERES = ((0.0, 0.0, 0.0, 1.0), (1.6, 0.2, 0.1, 0.7), (-0.4, 1.5, 0.3, 0.5), (0.3, -0.2, 1.7, 0.9))
NOISE = 0.002
DIRECTIONS = ("data_to_ref", "ref_to_data")


def surface_cloud(n, seed):
    """n points on the spheres, by area, each moved by Gaussian noise; float32."""
    rng = np.random.default_rng(seed)
    area = np.array([s[3] ** 2 for s in SPHERES])
    which = rng.choice(len(SPHERES), n, p=area / area.sum())
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    s = np.array(SPHERES)[which]
    return (s[:, :3] + s[:, 3:4] * d + NOISE * rng.standard_normal((n, 3))).astype(np.float32)


def stats(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
            "ms_p90": round(sorted(ms)[int(0.9 * (len(ms) - 1))], 4)}


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def as_points(xyz):
    p = np.zeros((len(xyz), 9), np.float32)
    p[:, :3] = xyz
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000, 4_000_000])
    a = ap.parse_args()
    try:
        from scipy.spatial import cKDTree
        host_name = "scipy.spatial.cKDTree"
    except ImportError:
        cKDTree = None
        host_name = "numpy all-pairs restatement (smallest size only)"
    res = {"device": capi.device_identity(0), "clock_before": capi.clock_probe(0, 500.0), "host": host_name,
           "spheres": len(SPHERES), "noise": NOISE, "reps": a.reps, "sizes": {}}
    for n in a.sizes:
        data, ref = surface_cloud(n, 1), surface_cloud(n, 2)
        # the cap: about eight times the mean spacing of the points on their surfaces
        max_dist = float(np.float32(8.0 * np.sqrt(4 * np.pi * sum(s[3] ** 2 for s in SPHERES) / n)))
        taus = (max_dist / 8, max_dist / 4, max_dist / 2)
        fu = capi.Fusion(0, _camera())
        fu.set_scene(as_points(data))
        fu.set_reference_cloud(ref)
        entry = {"points_per_side": n, "max_dist": max_dist}
        out = {}

        def run(direction):
            out[direction] = fu.cloud_distance("scene", direction, max_dist, taus)
        for d in DIRECTIONS:
            run(d)
        t = {d: [] for d in DIRECTIONS}
        grid = {}
        for _ in range(a.reps):
            for d in DIRECTIONS:
                t[d].append(timed(lambda: run(d)))
                grid[d] = fu.distance_grid()
        for d in DIRECTIONS:
            r = out[d]
            row = stats(t[d])
            row.update(queries_per_s=round(r.n_query / (row["ms_median"] * 1e-3)), n_matched=r.n_matched, mean=r.mean,
                       within=r.within, **grid[d])
            q, tg = (data, ref) if d == "data_to_ref" else (ref, data)
            if cKDTree is not None:
                best = [None]

                def host():
                    best[0] = cKDTree(tg).query(q, k=1, distance_upper_bound=max_dist)
                row["host_ms"] = round(min(timed(host) for _ in range(2)), 1)
                hd, hi = best[0]
                fu.cloud_distance("scene", d, max_dist, taus)
                dist, nn = fu.distance_results()
                both = (nn >= 0) & (hi < len(tg))
                # the tree measures in float64 and breaks ties its own way: compare distances, and count other choices
                row["host_matched"] = int((hi < len(tg)).sum())
                row["max_abs_distance_difference"] = float(np.abs(dist[both] - hd[both]).max()) if both.any() else 0.0
                row["other_nearest"] = int((nn[both] != hi[both]).sum())
            elif n == min(a.sizes):
                import cloud_distance_support as cd
                best = [None]

                def host():
                    best[0] = cd.distances(q, tg, max_dist, taus, rows=64)
                row["host_ms"] = round(timed(host), 1)
                fu.cloud_distance("scene", d, max_dist, taus)
                d2, nn = fu.distance_results(squared=True)
                row["equal_to_restatement"] = bool(np.array_equal(d2.view(np.uint32), best[0][0].view(np.uint32)) and
                                                   np.array_equal(nn, best[0][1]) and cd.summary_of(out[d]) == best[0][2])
            else:
                row["host_ms"] = None
            entry[d] = row
        fu.close()
        res["sizes"][str(n)] = entry
        print(n, json.dumps(entry), flush=True)
    res["clock_after"] = capi.clock_probe(0, 500.0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def _camera():
    cam = np.zeros(1, capi.CAMERA_DTYPE)
    cam["width"], cam["height"] = 8, 8
    return cam


if __name__ == "__main__":
    main()
