"""Numbers of the mesh sampling: the room/256 mesh of the 768x384 sphere rig's fused scene (the room is 10
long; trunc = 3 voxel sizes) sampled at spacings of half a voxel and two voxels, and a box of twelve wall-sized triangles
sampled at a spacing that gives about a million samples.  Per case: the wall time of acmmp_fusion_mesh_sample (median and
minimum), samples per second, the bytes written per second (40 per sample); the accuracy of the mesh against the ground
truth from the samples beside the accuracy from the vertices, with precision per threshold.  The rig's ground truth is
its own scene cloud (fused from the ground-truth depth maps); the box's is a million uniform points of its surface.
Host: the tests' numpy restatement on the same mesh, checked equal to the device -- untuned numpy, the comparator of
record and an upper bound on what a tuned host would need.

    python scripts/mesh_sample_probe.py OUT.json [--reps 30]

Every timed call ends synchronised (it returns the count); the median of the repetitions after a warm-up is reported; the
shader clock under load is probed before and after."""
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
BOX_HALF = (5.0, 3.0, 2.0)
BOX_SAMPLES = 1.0e6


def rig(W, H, n, seed=3):
    sc = scene.sphere_scene(W, H, n_src=n - 1, seed=seed)
    bgr = [np.repeat(np.asarray(im, np.uint8)[..., None], 3, 2) for im in sc.images]
    return np.array(sc.cameras), sc.extra["gt_depths"], sc.extra["gt_normals"], bgr


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def box_surface(n, seed=11):
    """n uniform float32 points on the surface of the box of half-extents BOX_HALF, faces drawn in proportion to area."""
    rng = np.random.default_rng(seed)
    h = np.array(BOX_HALF)
    area = np.array([h[1] * h[2], h[0] * h[2], h[0] * h[1]])
    axis = rng.choice(3, n, p=area / area.sum())
    p = (2 * rng.random((n, 3)) - 1) * h
    p[np.arange(n), axis] = np.where(rng.random(n) < 0.5, -1.0, 1.0) * h[axis]
    return p.astype(np.float32)


def measure(fu, source, max_dist, taus):
    r = fu.cloud_distance(source, "data_to_ref", max_dist, taus)
    return {"n_valid": r.n_valid, "n_matched": r.n_matched, "mean": r.mean,
            "precision": [w / r.n_valid if r.n_valid else 0.0 for w in r.within]}


def case(fu, spacing, reps, max_dist, taus, host_mesh=None):
    out = [None]

    def run():
        out[0] = fu.mesh_sample(spacing, 0)
    run()
    ms = [timed(run) for _ in range(reps)]
    n = out[0].n_samples
    med = statistics.median(ms)
    row = {"spacing": float(np.float32(spacing)), "n_samples": n, "n_skipped": out[0].n_skipped,
           "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "samples_per_s": round(n / (med * 1e-3)),
           "bytes_per_s_written": round(40 * n / (med * 1e-3)),
           "accuracy": {"samples": measure(fu, "samples", max_dist, taus), "vertices": measure(fu, "mesh", max_dist, taus)}}
    if host_mesh is not None:
        import mesh_sample_support as mss
        best = [None]

        def host():
            best[0] = mss.sample(host_mesh[0], host_mesh[1], spacing, 0)
        host_ms = timed(host)
        pts, face = fu.sample_points()
        row["host"] = {"comparator": "numpy restatement (untuned)", "ms": round(host_ms, 1),
                       "equal_to_restatement": bool(np.array_equal(pts.view(np.uint32), best[0][0].view(np.uint32)) and
                                                    np.array_equal(face, best[0][1]))}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    res = {"device": capi.device_identity(0), "clock_before": capi.clock_probe(0, 500.0), "reps": a.reps}
    cams, depths, normals, bgr = rig(768, 384, 4)
    fu = capi.Fusion(0, cams)
    for k in range(4):
        fu.set_view(k, depths[k], normals[k], bgr[k])
    views = list(range(4))
    total, _ = fu.run_scene(views, [[j for j in views if j != k] for k in views])
    truth = fu.scene_points(0, total)[:, :3]
    fu.set_reference_cloud(truth)
    size = float(np.float32(ROOM / 256))
    fu.voxelize(size)
    nv, nf, _ = fu.voxel_mesh(views, float(np.float32(TRUNC_CELLS * size)), 1)
    mesh = (fu.mesh_vertices(0, nv), fu.mesh_faces(0, nf))
    max_dist, taus = float(np.float32(4 * size)), (size / 4, size / 2, size)
    res["rig"] = {"rig": "768x384", "views": 4, "ground_truth_points": int(total), "voxel_size": size, "vertices": nv,
                  "faces": nf, "max_dist": max_dist, "thresholds": list(taus), "cases": {}}
    for name, spacing in (("half a voxel", 0.5 * size), ("two voxels", 2.0 * size)):
        res["rig"]["cases"][name] = case(fu, spacing, a.reps, max_dist, taus, host_mesh=mesh)
        print(name, json.dumps(res["rig"]["cases"][name]), flush=True)
    import mesh_render_support as rs
    box = rs.box_mesh(BOX_HALF)
    fu.set_mesh(*box)
    fu.set_reference_cloud(box_surface(1000000))
    h = np.array(BOX_HALF)
    spacing = float(np.sqrt(8 * (h[0] * h[1] + h[1] * h[2] + h[0] * h[2]) / BOX_SAMPLES))
    res["box"] = dict(case(fu, spacing, a.reps, 0.25, (0.01, 0.02, 0.05), host_mesh=box), half=list(BOX_HALF), faces=12,
                      vertices=8, max_dist=0.25, thresholds=[0.01, 0.02, 0.05], ground_truth_points=1000000)
    print("box", json.dumps(res["box"]), flush=True)
    fu.close()
    res["clock_after"] = capi.clock_probe(0, 500.0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
