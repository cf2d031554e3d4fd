"""Two point clouds against each other on the GPU: accuracy (every point of A to its nearest point of B), completeness
(the reverse), and precision, recall and F-score at every threshold -- acmmp_fusion_cloud_distance through set_scene
and set_reference_cloud.  For two runs of the pipeline, for example --math exact against --math fast.

    python scripts/compare_clouds.py A.ply B.ply --max-dist 0.02 --threshold 0.005 --threshold 0.01 [--out eval.json]
                                     [--align rigid|similarity [--align-max-dist D] [--align-iterations K] [--align-stride S]
                                      [--align-plane-iterations N]] [--surface] [--mesh-samples SPACING]

A is the data cloud, B the reference cloud; both are PLYs of the pipeline's layout.  With --align, A is first registered
to B on the GPU (acmmp_fusion_cloud_align) and measured under that transform, which the output then holds under "align".
With --align-plane-iterations, up to N rigid point-to-plane iterations along A's normals
(acmmp_fusion_cloud_align_plane) then refine that transform, and "align" gains "plane".
With --surface, A is a mesh PLY (io.write_mesh_ply's layout): its vertices are the data cloud, and the output gains
"surface" -- B's points and A's vertices against A's faces, point to triangle (acmmp_fusion_surface_distance), recall
from the surface (pipeline.evaluate_surface).
With --mesh-samples SPACING, A is a mesh PLY as well: its surface is sampled on the GPU, about one point per SPACING^2 of
area (acmmp_fusion_mesh_sample), and the output gains "mesh_samples" -- the samples against B in both directions, the
mesh's accuracy weighted by area (pipeline.evaluate_mesh_samples).
Prints the figures as one JSON line (pipeline.evaluate_clouds)."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "acmmp-spherical_amd"))

from acmmp import capi, io, pipeline  # noqa: E402


def compare(a_xyz, b_xyz, max_dist, thresholds=(), device=0, make=None, align=None, align_max_dist=None,
            align_iterations=30, align_stride=1, align_plane_iterations=None, a_normals=None, a_faces=None,
            surface=True, mesh_samples=None, region_a=None, region_b=None, region_queries_only=False):
    """evaluate_clouds of cloud A (n, 3) against cloud B, after align_clouds when align is "rigid" or "similarity";
    align_plane_iterations: its point-to-plane stage, along a_normals (n, 3).  make: the fusion object's factory
    (tests).  a_faces (m, 3): A is a mesh, loaded through set_mesh as well, and the result gains "surface" (unless
    surface is False) and, with mesh_samples (a spacing), "mesh_samples".  region_a, region_b: the evaluation regions of
    A (the data side) and of B (the reference side), io.Region or a file of io.read_region, in B's frame; they are set
    before the registration, region_queries_only keeps A's points outside its region as targets, and the result gains
    "region" as eval.json does."""
    if mesh_samples is not None and a_faces is None:
        raise ValueError("the mesh samples need A's faces")
    if align_plane_iterations is not None and (align is None or a_normals is None):
        raise ValueError("the plane stage needs align and A's normals")
    cam = np.zeros(1, capi.CAMERA_DTYPE)
    cam["width"], cam["height"] = 8, 8                        # the object needs a camera; no view is used
    fu = (make or (lambda c: capi.Fusion(device, c)))(cam)
    try:
        pts = np.zeros((len(a_xyz), 9), np.float32)
        pts[:, :3] = a_xyz
        if a_normals is not None:
            pts[:, 3:6] = a_normals
        fu.set_scene(pts)
        if a_faces is not None:
            fu.set_mesh(pts, a_faces)
        fu.set_reference_cloud(b_xyz)
        regions = {"data": region_a, "reference": region_b}
        for side, r in regions.items():
            if r is not None:
                fu.set_region(side, io.read_region(os.fspath(r)) if isinstance(r, (str, os.PathLike)) else r,
                              queries_only=region_queries_only and side == "data")
        registered = None
        if align is not None:
            registered = pipeline.align_clouds(fu, "scene", align, max_dist if align_max_dist is None else align_max_dist,
                                               align_iterations, align_stride, plane_iterations=align_plane_iterations)
        info = pipeline.evaluate_clouds(fu, "scene", max_dist, thresholds)
        if registered is not None:
            info["align"] = registered
        if region_a is not None or region_b is not None:
            info["region"] = {side: {"file": os.fspath(r) if isinstance(r, (str, os.PathLike)) else None,
                                     "queries_only": bool(region_queries_only and side == "data"),
                                     "counts": fu.region_classify("scene" if side == "data" else "reference")}
                              for side, r in regions.items() if r is not None}
        if a_faces is not None and surface:
            info["surface"] = pipeline.evaluate_surface(fu, "scene", max_dist, thresholds, info["accuracy"])
        if mesh_samples is not None:
            info["mesh_samples"] = pipeline.evaluate_mesh_samples(fu, mesh_samples, max_dist, thresholds)
        return info
    finally:
        if hasattr(fu, "close"):
            fu.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--max-dist", type=float, required=True)
    ap.add_argument("--threshold", type=float, action="append", default=[])
    ap.add_argument("--align", choices=["rigid", "similarity"], default=None)
    ap.add_argument("--align-max-dist", type=float, default=None, help="default: --max-dist")
    ap.add_argument("--align-iterations", type=int, default=30)
    ap.add_argument("--align-stride", type=int, default=1)
    ap.add_argument("--align-plane-iterations", type=int, default=None,
                    help="with --align: then at most this many point-to-plane iterations along A's normals")
    ap.add_argument("--surface", action="store_true", help="A is a mesh PLY: also measure against its faces")
    ap.add_argument("--mesh-samples", metavar="SPACING", type=float, default=None,
                    help="A is a mesh PLY: also sample its surface, one point per SPACING^2, and measure the samples")
    ap.add_argument("--eval-region-data", metavar="FILE", default=None,
                    help="measure only A's points inside this region (a SelectionPolygonVolume JSON or the project's region "
                         "JSON), given in B's frame and applied under each transform of --align")
    ap.add_argument("--eval-region-reference", metavar="FILE", default=None, help="the same for B's points")
    ap.add_argument("--eval-region-queries-only", action="store_true",
                    help="with --eval-region-data: A's points outside the region still serve as targets")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.align_plane_iterations is not None and a.align is None:
        ap.error("--align-plane-iterations needs --align")
    if a.eval_region_queries_only and a.eval_region_data is None:
        ap.error("--eval-region-queries-only needs --eval-region-data")
    normals = None
    if a.align_plane_iterations is not None and not a.surface and a.mesh_samples is None:
        rec = io.read_ply(a.a)
        normals = np.stack([rec["nx"], rec["ny"], rec["nz"]], 1)
    faces = None
    if a.surface or a.mesh_samples is not None:
        mesh_rec, faces = io.read_mesh_ply(a.a)
        a_xyz = np.ascontiguousarray(np.stack([mesh_rec["x"], mesh_rec["y"], mesh_rec["z"]], 1), np.float32)
        if a.align_plane_iterations is not None:
            normals = np.stack([mesh_rec["nx"], mesh_rec["ny"], mesh_rec["nz"]], 1)
    else:
        a_xyz = pipeline.reference_xyz(a.a)
    info = compare(a_xyz, pipeline.reference_xyz(a.b), a.max_dist, a.threshold, a.device,
                   align=a.align, align_max_dist=a.align_max_dist, align_iterations=a.align_iterations,
                   align_stride=a.align_stride, align_plane_iterations=a.align_plane_iterations, a_normals=normals,
                   a_faces=faces, surface=a.surface, mesh_samples=a.mesh_samples, region_a=a.eval_region_data,
                   region_b=a.eval_region_reference, region_queries_only=a.eval_region_queries_only)
    info.update(a=a.a, b=a.b)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(info, f, indent=1)
    print(json.dumps(info), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
