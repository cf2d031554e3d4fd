"""Numbers of the point-to-triangle distances: the meshes of the 768x384 sphere rig's fused scene at voxel
sizes room/64, room/256 and room/1024 (the room is 10 long; trunc = 3 voxel sizes), measured against the rig's own scene
cloud ("fidelity") and against a reference cloud ("completeness": the scene cloud's points moved by Gaussian noise of
room/512, another seed).  Per size and per small_max (the default, 16, 64, 256): the wall time of
acmmp_fusion_surface_distance, queries per second, registrations per face, large faces, the largest ring; beside the
surface completeness the vertex-only completeness (cloud_distance, "mesh", "ref_to_data") at the same thresholds, and the
vertices no face refers to.  The rig's meshes have no long face, so the room/256 mesh is measured again with LONG_FACES
long slivers added through set_mesh (each about a quarter of the room long, a voxel wide): the case small_max is for.
Host: trimesh's closest_point over the whole reference cloud at room/64 where trimesh can be imported, with the largest
disagreement in float64; otherwise the tests' numpy restatement on the first HOST_QUERIES reference points at room/64,
checked equal to the device there and scaled to the cloud -- an upper bound on what a tuned host would need.

    python scripts/surface_distance_probe.py OUT.json [--reps 9]

Every timed call ends synchronised (it returns the summary); the two query clouds alternate within one process after a
warm-up and the median is reported; the shader clock under load is probed before and after."""
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
TRUNC_CELLS = 3.0
SMALL_MAX = (0, 16, 64, 256)
LONG_FACES = 256
LONG_SMALL_MAX = (16, 64, 256, 4096)
HOST_QUERIES = 128
QUERIES = ("scene", "reference")


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


def with_long_faces(vertices, faces, size, seed=5):
    """The mesh with LONG_FACES slivers added: from a random vertex a quarter of the room along a random direction, one
    voxel wide."""
    rng = np.random.default_rng(seed)
    a = vertices[rng.integers(0, len(vertices), LONG_FACES), :3].astype(np.float64)
    d = rng.standard_normal((LONG_FACES, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    w = np.cross(d, rng.standard_normal((LONG_FACES, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    extra = np.zeros((3 * LONG_FACES, 9), np.float32)
    extra[:, :3] = np.stack([a, a + (ROOM / 4) * d, a + (ROOM / 4) * d + size * w], 1).reshape(-1, 3)
    extra[:, 5] = 1.0
    tri = len(vertices) + np.arange(3 * LONG_FACES, dtype=np.int32).reshape(-1, 3)
    return np.concatenate([vertices, extra]), np.concatenate([faces, tri])


def time_plans(fu, plans, max_dist, taus, reps):
    """Per small_max: the plan, the grid and the two query clouds' times, alternated."""
    rows, out = {}, {}

    def run(q):
        out[q] = fu.surface_distance(q, max_dist, taus)
    for small_max in plans:
        fu.surface_plan(small_max)
        for q in QUERIES:
            run(q)
        t = {q: [] for q in QUERIES}
        for _ in range(reps):
            for q in QUERIES:
                t[q].append(timed(lambda: run(q)))
        plan, grid = fu.surface_plan(small_max), fu.surface_grid()
        row = dict(plan, **grid, registrations_per_face=round(plan["registrations"] / max(plan["small"], 1), 3))
        for q in QUERIES:
            r = out[q]
            row[q] = dict(stats(t[q]), queries_per_s=round(r.n_query / (statistics.median(t[q]) * 1e-3)),
                          n_query=r.n_query, n_matched=r.n_matched, mean=r.mean, within=r.within)
        rows["default" if small_max == 0 else str(small_max)] = row
    fu.surface_plan(0)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    res = {"device": capi.device_identity(0), "clock_before": capi.clock_probe(0, 500.0), "reps": a.reps,
           "trunc_cells": TRUNC_CELLS, "small_max": list(SMALL_MAX)}
    cams, depths, normals, bgr = rig(768, 384, 4)
    fu = capi.Fusion(0, cams)
    for k in range(4):
        fu.set_view(k, depths[k], normals[k], bgr[k])
    views = list(range(4))
    total, _ = fu.run_scene(views, [[j for j in views if j != k] for k in views])
    cloud = fu.scene_points(0, total)[:, :3]
    ref = (cloud + (ROOM / 512) * np.random.default_rng(7).standard_normal(cloud.shape)).astype(np.float32)
    fu.set_reference_cloud(ref)
    res["scene"] = {"rig": "768x384", "views": 4, "points": int(total), "reference_points": len(ref)}
    res["sizes"] = {}
    for div in (64, 256, 1024):
        size = float(np.float32(ROOM / div))
        fu.voxelize(size)
        nv, nf, _ = fu.voxel_mesh(views, float(np.float32(TRUNC_CELLS * size)), 1)
        max_dist = float(np.float32(4 * size))
        taus = (size / 2, size, 2 * size)
        entry = {"voxel_size": size, "vertices": nv, "faces": nf, "max_dist": max_dist, "thresholds": list(taus), "plans": {}}
        entry["plans"] = time_plans(fu, SMALL_MAX, max_dist, taus, a.reps)
        # the feature's reason: completeness against the surface beside completeness against the vertices
        s = fu.surface_distance("reference", max_dist, taus)
        v = fu.cloud_distance("mesh", "ref_to_data", max_dist, taus)
        entry["completeness"] = {"surface": {"within": s.within, "n_matched": s.n_matched, "mean": s.mean},
                                 "vertices": {"within": v.within, "n_matched": v.n_matched, "mean": v.mean},
                                 "n_valid": s.n_valid}
        mv, mf = fu.mesh_vertices(0, nv), fu.mesh_faces(0, nf)
        entry["vertices_without_a_face"] = int(nv - len(np.unique(mf)))
        if div == 256:
            lv, lf = with_long_faces(mv, mf, size)
            fu.set_mesh(lv, lf)
            entry["with_long_faces"] = {"added": LONG_FACES, "plans": time_plans(fu, LONG_SMALL_MAX, max_dist, taus, a.reps)}
        if div == 64:
            try:
                import trimesh
            except ImportError:
                trimesh = None
            if trimesh is not None:
                tm = trimesh.Trimesh(mv[:, :3].astype(np.float64), mf, process=False)
                best = [None]

                def host():
                    best[0] = trimesh.proximity.closest_point(tm, ref.astype(np.float64))
                ms = timed(host)
                dist, nn = fu.surface_results()
                both = nn >= 0
                entry["host"] = {"comparator": "trimesh.proximity.closest_point", "queries": len(ref), "ms": round(ms, 1),
                                 "max_abs_distance_difference": float(np.abs(dist[both] - best[0][1][both]).max()) if both.any() else 0.0}
            else:
                import surface_distance_support as sd
                best = [None]

                def host():
                    best[0] = sd.distances(ref[:HOST_QUERIES], mv, mf, max_dist, taus)
                ms = timed(host)
                d2, nn = fu.surface_results(0, HOST_QUERIES, squared=True)
                entry["host"] = {"comparator": "numpy restatement (no trimesh on this machine): an upper bound",
                                 "queries": HOST_QUERIES, "ms": round(ms, 1),
                                 "ms_scaled_to_the_cloud": round(ms * len(ref) / HOST_QUERIES, 1),
                                 "equal_to_restatement": bool(np.array_equal(d2.view(np.uint32), best[0][0].view(np.uint32)) and
                                                              np.array_equal(nn, best[0][1]))}
        res["sizes"][f"room/{div}"] = entry
        print(f"room/{div}", json.dumps(entry), flush=True)
    fu.close()
    res["clock_after"] = capi.clock_probe(0, 500.0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
