"""Numbers of the evaluation regions: the 768x384 sphere rig's fused scene (about 1.07 M points) against
itself moved by noise, as surface_distance_probe and cloud_align_probe measure it.

    python scripts/eval_region_probe.py OUT.json [--reps 9] [--role feature|parent]

Measured: acmmp_fusion_region_classify with a 64-vertex prism, a 256^3 grid and 2 planes; acmmp_fusion_cloud_distance
(both directions) with no region and with an all-inside region on both sides -- the same answers, one more pass over each
cloud; and, with no region, the surface and the two align calls.  The no-region rows are the ones that are compared with
the parent commit: run the script with ACMMP_LIB naming a build of the parent and --role parent (the region rows are
then left out), alternate the two three times, and put the runs side by side with --merge.  Every timed call ends
synchronised; the calls alternate within one process after a warm-up; the shader clock under load is probed before and
after."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from surface_distance_probe import ROOM, capi, rig, stats, timed  # noqa: E402

from acmmp import io  # noqa: E402


def probe_region(lo, hi):
    """A 64-gon around the scene about z, a 256^3 grid with every bit set over its box, two planes below and above it:
    every valid point is inside."""
    c, r = 0.5 * (lo + hi), 0.75 * float(np.linalg.norm(hi - lo))
    t = 2 * np.pi * np.arange(64) / 64
    reg = io.Region()
    reg.axis, reg.axis_min, reg.axis_max = 2, float(lo[2] - 1), float(hi[2] + 1)
    reg.polygon = np.stack([c[0] + r * np.cos(t), c[1] + r * np.sin(t)], 1)
    reg.planes = np.array([[0, 0, 1, -(lo[2] - 1)], [0, 0, -1, hi[2] + 1]], np.float64)
    reg.cell = float((hi - lo).max() / 254)
    reg.origin = lo - reg.cell
    reg.dims = (256, 256, 256)
    reg.bits = np.full(256 ** 3 // 8, 0xff, np.uint8)
    return reg


def merge(paths, out):
    """The no-region medians of alternated feature and parent runs side by side: each side's band (minimum and maximum of
    its runs' medians) and whether the feature's median of medians lies inside the parent's band."""
    runs = [json.load(open(p)) for p in paths]
    rows = {}
    for call in ("distance_data_to_ref", "distance_ref_to_data", "surface_reference", "align", "align_plane"):
        side = {role: [r["no_region"][call]["ms_median"] for r in runs if r["role"] == role] for role in ("feature", "parent")}
        band = {role: [min(v), max(v)] for role, v in side.items() if v}
        row = {"medians": side, "band": band}
        if len(band) == 2:
            mid = float(np.median(side["feature"]))
            row["feature_median"] = mid
            row["inside_parent_band"] = bool(band["parent"][0] <= mid <= band["parent"][1])
        rows[call] = row
    with open(out, "w") as f:
        json.dump({"runs": paths, "no_region": rows, "feature": next((r for r in runs if r["role"] == "feature"), None)}, f, indent=1)
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--role", choices=["feature", "parent"], default="feature")
    ap.add_argument("--merge", nargs="+", default=None, help="run files to put side by side into OUT")
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.out)
    res = {"role": a.role, "library": capi.LIB_PATH, "device": capi.device_identity(0), "clock_before": capi.clock_probe(0, 500.0),
           "reps": a.reps}
    cams, depths, normals, bgr = rig(768, 384, 4)
    fu = capi.Fusion(0, cams)
    for k in range(4):
        fu.set_view(k, depths[k], normals[k], bgr[k])
    views = list(range(4))
    total, _ = fu.run_scene(views, [[j for j in views if j != k] for k in views])
    cloud = fu.scene_points(0, total)[:, :3]
    ref = (cloud + (ROOM / 512) * np.random.default_rng(7).standard_normal(cloud.shape)).astype(np.float32)
    fu.set_reference_cloud(ref)
    size = float(np.float32(ROOM / 256))
    max_dist, taus = 4 * size, (size / 4, size / 2, size)
    fu.voxelize(size)
    fu.voxel_mesh(views, float(np.float32(3 * size)), 1)
    res["scene"] = {"rig": "768x384", "views": 4, "points": int(total), "reference_points": len(ref), "max_dist": max_dist}
    out = {}
    calls = {
        "distance_data_to_ref": lambda: out.__setitem__("d2r", fu.cloud_distance("scene", "data_to_ref", max_dist, taus)),
        "distance_ref_to_data": lambda: out.__setitem__("r2d", fu.cloud_distance("scene", "ref_to_data", max_dist, taus)),
        "surface_reference": lambda: out.__setitem__("surf", fu.surface_distance("reference", max_dist, taus)),
        "align": lambda: out.__setitem__("align", fu.cloud_align("scene", "rigid", max_dist, 5)),
        "align_plane": lambda: out.__setitem__("plane", fu.cloud_align_plane("scene", max_dist, 5)),
    }

    def time_all(names):
        for n in names:
            calls[n]()
        t = {n: [] for n in names}
        for _ in range(a.reps):
            for n in names:
                t[n].append(timed(calls[n]))
        return {n: stats(v) for n, v in t.items()}

    res["no_region"] = time_all(list(calls))
    plain = {k: (v.n_valid, v.n_matched, v.sum_q) for k, v in out.items() if k in ("d2r", "r2d")}
    if a.role == "feature":
        ok = np.isfinite(cloud).all(1)
        reg = probe_region(np.minimum(cloud[ok].min(0), ref.min(0)).astype(np.float64),
                           np.maximum(cloud[ok].max(0), ref.max(0)).astype(np.float64))
        fu.set_region("data", reg)
        fu.set_region("reference", reg)
        calls["classify_scene"] = lambda: out.__setitem__("cls", fu.region_classify("scene"))
        res["region"] = time_all(["classify_scene", "distance_data_to_ref", "distance_ref_to_data"])
        res["region"]["counts"] = out["cls"]
        res["region"]["parts"] = {"planes": 2, "vertices": 64, "dims": [256, 256, 256]}
        res["region"]["points_per_s"] = round(out["cls"]["points"] / (res["region"]["classify_scene"]["ms_median"] * 1e-3))
        res["region"]["all_inside"] = out["cls"]["inside"] == out["cls"]["points"] - out["cls"]["invalid"]
        res["region"]["same_summaries"] = plain == {k: (v.n_valid, v.n_matched, v.sum_q) for k, v in out.items() if k in ("d2r", "r2d")}
    fu.close()
    res["clock_after"] = capi.clock_probe(0, 500.0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
