"""Numbers of the surface mesh of the voxel cloud: on the 768x384 ground-truth rig, 4 views, at voxel
sizes room/64, room/256 and room/1024 (the room is 10 long), the wall time of acmmp_fusion_voxel_mesh on the resident
voxel result over all four views (trunc = 3 voxel sizes, min_weight 1) alone and with the download of the mesh, the
samples, vertices and faces it produces and the bytes of its sample table; beside them the tests' sequential
restatement on the host, one run.  The restatement -- a ctypes call into the oracle per sample and view, then Python
loops over dicts -- is untuned, so the ratio to it is an upper bound on what the device pass saves against a tuned host
library; it is run only up to --host-max-entries entries (its time grows to many minutes beyond).

    python scripts/voxel_mesh_probe.py OUT.json [--reps 30] [--host-max-entries 50000]

Every timed path ends synchronised; the device paths alternate within one process after a warm-up; the shader
clock under load is probed before and after.  Where the restatement runs, the device result is checked against it."""
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
MIN_WEIGHT = 1


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
    ap.add_argument("--host-max-entries", type=int, default=50000)
    a = ap.parse_args()
    import voxel_clean_support as cs
    import voxel_mesh_support as ms
    import voxel_support as vs
    res = {"device": capi.device_identity(0), "clock_before": capi.clock_probe(0, 500.0),
           "note": "host_restatement is untuned (a ctypes call per sample and view, then Python loops): device-to-host "
                   "ratios are upper bounds",
           "trunc_cells": TRUNC_CELLS, "min_weight": MIN_WEIGHT}
    cams, depths, normals, bgr = rig(768, 384, 4)
    fu = capi.Fusion(0, cams)
    for k in range(4):
        fu.set_view(k, depths[k], normals[k], bgr[k])
    views = list(range(4))
    total, _ = fu.run_scene(views, [[j for j in views if j != k] for k in views])
    res["scene"] = {"rig": "768x384", "views": 4, "points": total}
    res["sizes"] = {}
    for div in (64, 256, 1024):
        size = float(np.float32(ROOM / div))
        trunc = float(np.float32(TRUNC_CELLS * size))
        ne, vinfo = fu.voxelize(size)
        out = {}

        def run():
            out["mesh"] = fu.voxel_mesh(views, trunc, MIN_WEIGHT)

        def run_and_download():
            nv, nf, _ = fu.voxel_mesh(views, trunc, MIN_WEIGHT)
            return fu.mesh_vertices(0, nv), fu.mesh_faces(0, nf)
        paths = {"voxel_mesh": run, "voxel_mesh_and_download": run_and_download}
        for _ in range(3):
            for f in paths.values():
                f()
        t = {k: [] for k in paths}
        for _ in range(a.reps):
            for k, f in paths.items():
                t[k].append(timed(f))
        nv, nf, info = out["mesh"]
        table = fu.mesh_table()
        entry = {"voxel_size": size, "trunc": trunc, "entries": ne, "reps": a.reps, "samples": info["samples"],
                 "samples_per_entry": round(info["samples"] / max(ne, 1), 3), "valid": info["valid"], "cubes": info["cubes"],
                 "vertices": nv, "faces": nf, "uncoloured": info["uncoloured"], "table_slots": table["slots"],
                 "table_bytes": 32 * table["slots"], "table_load": round(table["occupied"] / table["slots"], 4),
                 "result_bytes": 24 * info["samples"] + 36 * nv + 12 * nf, "mesh_bytes": 36 * nv + 12 * nf}
        entry.update({k: stats(v) for k, v in t.items()})
        if ne <= a.host_max_entries:
            pts = fu.voxel_points(0, ne)
            keys = vs.voxelize(fu.scene_points(0, total), size)["keys"]
            cells = np.array(cs.unpack(keys), np.int64).reshape(-1, 3)
            want = [None]
            entry["host_restatement_ms"] = round(timed(lambda: want.__setitem__(0, ms.mesh(
                cells, pts[:, 6:9], vinfo["origin"], size, cams, depths, views, trunc, MIN_WEIGHT))), 1)
            w = want[0]
            c, s, e = fu.mesh_samples(0, info["samples"])
            entry["equal_to_restatement"] = bool(
                info == w["info"] and np.array_equal(fu.mesh_vertices(0, nv).view(np.uint32), w["vertices"].view(np.uint32)) and
                np.array_equal(fu.mesh_faces(0, nf), w["faces"]) and np.array_equal(c, w["cells"]) and
                np.array_equal(s, w["tsdf"]) and np.array_equal(e, w["entry"]))
        else:
            entry["host_restatement_ms"] = None
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
