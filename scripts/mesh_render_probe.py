"""Numbers of the mesh rendered into a view: on the 768x384 ground-truth rig, 4 views, the mesh of the
voxel result at voxel sizes room/64, room/256 and room/1024 (the room is 10 long; trunc = 3 voxel sizes, min_weight 1),
the wall time of acmmp_fusion_mesh_render per view alone and with the download of the four maps, the faces rendered by
their own lane and by a workgroup, the candidate pixels, and the same render at other small / large thresholds; beside
them, at room/64 only, the hit test of the tests' exhaustive restatement on the host over one row in 16 of view 0,
one run, scaled to every row.  The restatement -- every pixel against every face in numpy -- is untuned, so the ratio
to it is an upper bound on what the device pass saves against a tuned host renderer.

    python scripts/mesh_render_probe.py OUT.json [--reps 30]

Every timed path ends synchronised; the device paths alternate within one process after a warm-up; the shader clock
under load is probed before and after.  Where the restatement runs, the device result is checked against it."""
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
THRESHOLDS = (16, 64, 256, 1024)
HOST_ROW_STEP = 16


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
    import mesh_render_support as rs
    res = {"device": capi.device_identity(0), "clock_before": capi.clock_probe(0, 500.0),
           "note": "host_restatement is untuned (every pixel against every face in numpy): device-to-host ratios are "
                   "upper bounds; times are per view, the median over the reps of each of the 4 views in turn",
           "trunc_cells": TRUNC_CELLS, "thresholds": list(THRESHOLDS)}
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
        fu.voxelize(size)
        nv, nf, _ = fu.voxel_mesh(views, float(np.float32(TRUNC_CELLS * size)), 1)
        entry = {"voxel_size": size, "vertices": nv, "faces": nf, "reps": a.reps, "thresholds": {}}
        state = {"view": 0}

        def run():
            state["info"] = fu.render_mesh(state["view"])

        def run_and_download():
            fu.render_mesh(state["view"])
            return fu.render_maps()
        for small_max in (0,) + THRESHOLDS:
            fu.render_plan(small_max)
            paths = {"render": run, "render_and_download": run_and_download}
            for _ in range(3):
                for f in paths.values():
                    f()
            t = {k: [] for k in paths}
            for rep in range(a.reps):
                state["view"] = rep % 4
                for k, f in paths.items():
                    t[k].append(timed(f))
            state["view"] = 0
            run()
            plan = fu.render_plan(small_max)
            row = {"n_small": plan["small"], "n_large": plan["large"], "n_candidates": plan["candidates"],
                   "candidates_per_face": round(plan["candidates"] / max(nf, 1), 2)}
            row.update({k: stats(v) for k, v in t.items()})
            if small_max == 0:
                entry.update(row)
                entry["view0"] = state["info"]
            else:
                entry["thresholds"][str(small_max)] = row
        fu.render_plan(0)
        if div == 64:
            # the restatement's hit test of every face against one row in HOST_ROW_STEP of view 0, then scaled
            V, T = fu.mesh_vertices(0, nv), fu.mesh_faces(0, nf)
            H, W = depths[0].shape
            pix = (np.arange(0, H, HOST_ROW_STEP)[:, None] * W + np.arange(W)[None, :]).reshape(-1)
            best = [None]

            def host():
                d = rs.rays(cams[0])[pix]
                frames, skipped = rs.camera_frame(cams[0], V, T)
                live = np.flatnonzero(~skipped)
                keys = np.full(len(pix), rs.NONE, np.uint64)
                step = max(1, (1 << 21) // len(pix))
                for f0 in range(0, len(live), step):
                    idx = live[f0:f0 + step]
                    hit, _, _, _, _, md = rs.hits(d, frames[idx], True)
                    key = (md.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)[None, :]
                    keys = np.minimum(keys, np.where(hit, key, rs.NONE).min(1))
                best[0] = keys
            ms_rows = timed(host)
            entry["host_rows"] = f"1 in {HOST_ROW_STEP}"
            entry["host_restatement_rows_ms"] = round(ms_rows, 1)
            entry["host_restatement_ms"] = round(ms_rows * HOST_ROW_STEP, 1)          # extrapolated to every row
            fu.render_mesh(0)
            depth, face, _, _ = fu.render_maps()
            won = best[0] != rs.NONE
            want_face = np.where(won, (best[0] & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
            want_depth = np.where(won, (best[0] >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0))
            entry["equal_to_restatement"] = bool(np.array_equal(face.reshape(-1)[pix], want_face) and
                                                 np.array_equal(depth.reshape(-1)[pix].view(np.uint32), want_depth.view(np.uint32)))
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
