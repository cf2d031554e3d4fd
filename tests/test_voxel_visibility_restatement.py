"""The visibility check of the voxel cloud, the parts that need no GPU: the restatement (visibility_support) gives the
classes its constructed clouds have by construction, the cases of test_gpu_voxel_visibility.py are not vacuous on it,
every bad argument is refused, the new entry points are declared, bound and exported, and Pipeline.run_fusion's
visibility path and command line driven by RestatedVisibilityFusion."""
import os
import re
import subprocess

import numpy as np
import pytest

import visibility_support as vis
import voxel_clean_support as cs
import voxel_support as vs
from acmmp import capi, io, pipeline
from conftest import assert_bitwise_equal
from pipeline_support import OracleEngine, small_dataset

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["acmmp_fusion_voxel_visibility", "acmmp_fusion_visible_points", "acmmp_fusion_visibility_tallies"]
RED, BLUE = (255.0, 0.0, 0.0), (0.0, 0.0, 255.0)            # the floaters and the points behind the wall


def _voxels(rig):
    cams, depths, _, _, cloud, size = vis.constructed(rig)
    v = vs.voxelize(cloud, size)
    assert v["n_rejected"] == 0 and v["points"].shape[0] % 256 != 0
    return cams, depths, v


@pytest.mark.parametrize("rig", list(vis.RIGS))
def test_constructed_cases(rig):
    cams, depths, v = _voxels(rig)
    pts = v["points"]
    views = list(range(len(cams)))
    proj = vis.project(cams, pts[:, :3])
    run = lambda tol, radius, th: vis.visibility(cams, depths, pts, views, tol, radius, *th, proj=proj)
    for tol in (0.01, 0.05):
        for radius in (0, 1):
            out = run(tol, radius, (1, 0))
            print(rig, "tol", tol, "radius", radius, "class totals", out["class_totals"], "kept", len(out["kept"]),
                  "unsupported", out["n_unsupported"], "conflicting", out["n_conflicting"])
            assert min(out["class_totals"]) > 0 and sum(out["class_totals"]) == len(pts) * len(views)
            assert (out["tallies"].sum(1) <= len(views)).all() and 0 < len(out["kept"]) < len(pts)
            # an entry fails one condition, the other or both
            assert max(out["n_unsupported"], out["n_conflicting"]) <= len(pts) - len(out["kept"]) <= out["n_unsupported"] + out["n_conflicting"]
        assert (run(tol, 0, (1, 0))["tallies"] != run(tol, 1, (1, 0))["tallies"]).any()
        for min_support in (0, 1):
            a, b = run(tol, 0, (min_support, 0)), run(tol, 0, (min_support, 1))
            assert set(a["kept"]) < set(b["kept"])
        assert len(run(tol, 0, (0, 4096))["kept"]) == len(pts)
    # by construction, in view 0 at radius 0: a floater voxel that is one point of the cloud lies on a pixel's ray at half
    # its depth, in front of all the view sees there; a point at 1.5 x the depth lies behind it
    cls0 = vis.view_classes(proj[0], depths[0], 0.05, 0)
    alone = v["counts"] == 1
    for colour, want in ((RED, vis.CONFLICT), (BLUE, vis.OCCLUDED)):
        sel = alone & (pts[:, 6:] == np.array(colour, np.float32)).all(1)
        assert sel.sum() >= 50 and (cls0[sel] == want).all()
    # a wider window can only add samples: support never falls, and unobserved never rises
    t0, t1 = run(0.05, 0, (0, 0))["tallies"], run(0.05, 1, (0, 0))["tallies"]
    assert (t1[:, 0] >= t0[:, 0]).all() and (t1.sum(1) >= t0.sum(1)).all()


def test_a_view_listed_twice_counts_twice():
    cams, depths, v = _voxels("sphere")
    pts = v["points"][:200]
    once = vis.visibility(cams, depths, pts, [0, 1, 2, 3], 0.01, 1, 2, 1)
    cycle = vis.visibility(cams, depths, pts, [k % 4 for k in range(70)], 0.01, 1, 2, 1)
    per = [vis.visibility(cams, depths, pts, [k], 0.01, 1)["tallies"] for k in range(4)]
    assert np.array_equal(once["tallies"], sum(per))
    assert np.array_equal(cycle["tallies"], 18 * (per[0] + per[1]) + 17 * (per[2] + per[3]))


def test_bad_arguments():
    cams, depths, v = _voxels("pinhole")
    pts = v["points"][:10]
    ok = dict(views=[0, 1, 2], rel_tol=0.01, radius=1, min_support=1, max_conflicts=0)
    vis.visibility(cams, depths, pts, **ok)
    for bad in (dict(views=[]), dict(views=[0] * 4097), dict(views=[0, 3]), dict(views=[-1]), dict(rel_tol=float("nan")),
                dict(rel_tol=float("inf")), dict(rel_tol=1e39), dict(rel_tol=-0.01), dict(radius=2), dict(radius=-1),
                dict(min_support=-1), dict(max_conflicts=-1)):
        with pytest.raises(ValueError):
            vis.visibility(cams, depths, pts, **{**ok, **bad})
    vis.visibility(cams, depths, pts, **{**ok, "views": [0] * 4096})
    with pytest.raises(ValueError):                                # a view that was never set
        vis.visibility(cams, [depths[0], None, depths[2]], pts, **ok)
    # the sources
    rf = vis.RestatedVisibilityFusion(cams)
    for k in (0, 2):
        rf.set_view(k, depths[k], np.zeros((*depths[k].shape, 3), np.float32), np.zeros((*depths[k].shape, 3), np.uint8))
    rf.set_scene(vis.constructed("pinhole")[4])
    with pytest.raises(ValueError):
        rf.voxel_visibility([0], 0.01)                             # no voxel result
    rf.voxelize(vis.constructed("pinhole")[5])
    with pytest.raises(ValueError):
        rf.voxel_visibility([0], 0.01, source="clean")             # no clean result
    with pytest.raises(ValueError):
        rf.voxel_visibility([0], 0.01, source="scene")
    with pytest.raises(ValueError):
        rf.voxel_visibility([0, 1], 0.01)                          # view 1 was never set
    assert rf.voxel_visibility([0, 2, 0], 0.01)[0] > 0
    with pytest.raises(ValueError):
        rf.visible_points(0, rf.voxels["points"].shape[0] + 1)
    # an empty source gives zeros
    rf.voxelize(vis.constructed("pinhole")[5], min_points=10 ** 6)
    assert rf.voxel_visibility([0, 2], 0.01) == (0, {"unsupported": 0, "conflicting": 0, "class_totals": [0, 0, 0, 0]})
    assert rf.visible_points(0, 0).shape == (0, 9) and rf.visibility_tallies(0, 0).shape == (0, 3)


def test_restated_fusion_lifetimes():
    cams, depths, normals, colours, cloud, size = vis.constructed("sphere")
    rf = vis.RestatedVisibilityFusion(cams)
    for k in range(len(cams)):
        rf.set_view(k, depths[k], normals[k], colours[k])
    views = list(range(len(cams)))
    rf.set_scene(cloud)
    nv = rf.voxelize(size)[0]
    n, info = rf.voxel_visibility(views, 0.01, radius=1)
    p, cnt, tal = rf.visible_points(0, n, counts=True, tallies=True)
    all_tal = rf.visibility_tallies(0, nv)
    assert p.shape == (n, 9) and cnt.shape == (n,) and tal.shape == (n, 3) and all_tal.shape == (nv, 3)
    assert (tal[:, 0] >= 1).all() and (tal[:, 1] == 0).all() and info["unsupported"] + info["conflicting"] >= nv - n
    kept = np.flatnonzero((all_tal[:, 0] >= 1) & (all_tal[:, 1] == 0))
    assert_bitwise_equal(p, rf.voxels["points"][kept], "kept entries in order")
    rf.voxel_clean(26, 1)                                          # a clean leaves a visible result of the voxel result
    assert rf.visible_points(0, n).shape[0] == n
    nc = rf.voxel_visibility(views, 0.01, radius=1, source="clean")[0]
    assert 0 < nc <= n and rf.visibility_tallies(0, len(rf.cleaned["kept"])).shape[0] == len(rf.cleaned["kept"])
    rf.voxel_clean(26, 1)                                          # ... and discards one of the clean result
    with pytest.raises(ValueError):
        rf.visible_points(0, 1)
    for discard in (lambda: rf.voxelize(size), lambda: rf.set_scene(cloud)):
        rf.voxelize(size)
        rf.voxel_visibility(views, 0.01)
        discard()
        with pytest.raises(ValueError):
            rf.visible_points(0, 1)


def test_new_entry_points_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "acmmp.h")).read(), flags=re.S)
    L = capi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in capi.EXPORTS and hasattr(L, name), name
        assert re.search(rf"\bT {name}$", out, re.M), name
    for method in ("voxel_visibility", "visible_points", "visibility_tallies"):
        assert callable(getattr(capi.Fusion, method, None)), method
    assert re.search(r"#define\s+ACMMP_VIS_FROM_VOXELS\s+0\b", header) and re.search(r"#define\s+ACMMP_VIS_FROM_CLEAN\s+1\b", header)
    assert capi.VIS_SOURCES == {"voxel": 0, "clean": 1}


def test_pipeline_visibility_path_with_stub(tmp_path):
    ds = small_dataset(64, 32, 3)
    pipe = pipeline.Pipeline(ds, engine=OracleEngine(), order="reference", geom_iterations=1).run()
    plain = pipe.run_fusion(fusion_factory=vis.RestatedVisibilityFusion)
    ok = vs.finite_points(plain)
    size = float((plain[ok, :3].max(0) - plain[ok, :3].min(0)).max()) / 16
    # the new arguments at their defaults: today's voxel and clean paths, their bytes and their fusion_info
    for kw in (dict(), dict(voxel_min_neighbours=1, voxel_min_component_voxels=3)):
        before = pipe.run_fusion(fusion_factory=cs.RestatedCleanFusion, ply_path=str(tmp_path / "before.ply"), voxel_size=size, **kw)
        info = dict(pipe.fusion_info)
        same = pipe.run_fusion(fusion_factory=vis.RestatedVisibilityFusion, ply_path=str(tmp_path / "same.ply"), voxel_size=size,
                               visibility_tol=None, visibility_radius=0, visibility_min_support=1, visibility_max_conflicts=0, **kw)
        assert pipe.fusion_info == info and not any(k.startswith("vis") for k in info)
        assert_bitwise_equal(same, before, "defaults")
        assert (tmp_path / "same.ply").read_bytes() == (tmp_path / "before.ply").read_bytes()
    with pytest.raises(ValueError):
        pipe.run_fusion(fusion_factory=vis.RestatedVisibilityFusion, visibility_tol=0.01)          # needs voxel_size
    with pytest.raises(ValueError):
        pipe.run_fusion(fusion_factory=cs.RestatedCleanFusion, voxel_size=size, visibility_tol=0.01)   # no voxel_visibility
    cams, depths, _, _ = pipeline.fusion_inputs(ds, pipe.store, pipe.problems)
    for clean, vkw in ((False, dict(visibility_tol=0.01)),
                       (True, dict(visibility_tol=0.002, visibility_radius=1, visibility_min_support=2, visibility_max_conflicts=1))):
        made = []

        def factory(c):
            made.append(vis.RestatedVisibilityFusion(c))
            return made[-1]
        ckw = dict(voxel_min_neighbours=1, voxel_min_component_voxels=3) if clean else {}
        got = pipe.run_fusion(fusion_factory=factory, ply_path=str(tmp_path / "visible.ply"), chunk_points=5, voxel_size=size,
                              **ckw, **vkw)
        info = pipe.fusion_info
        # the restatement, by hand: all views, after clean when clean was asked
        vox = vs.voxelize(made[0].result[0], size)
        src = np.arange(len(vox["counts"]))
        if clean:
            src = cs.clean(vox["keys"], vox["counts"], 26, 1, 3, 1)["kept"]
            assert info["clean_voxels"] == len(src) < info["voxels"]
        want = vis.visibility(cams, depths, vox["points"][src], list(range(len(cams))), vkw["visibility_tol"],
                              vkw.get("visibility_radius", 0), vkw.get("visibility_min_support", 1),
                              vkw.get("visibility_max_conflicts", 0))
        print("clean", clean, vkw, info)
        assert 0 < len(want["kept"]) < len(src)
        assert_bitwise_equal(got, vox["points"][src][want["kept"]], "visible cloud")
        assert pipe.fused is got
        io.write_ply(str(tmp_path / "want.ply"), got)
        assert (tmp_path / "visible.ply").read_bytes() == (tmp_path / "want.ply").read_bytes()
        assert (info["visible_voxels"], info["vis_unsupported"], info["vis_conflicting"], info["vis_class_totals"]) == \
            (len(want["kept"]), want["n_unsupported"], want["n_conflicting"], want["class_totals"])
        assert (info["visibility_tol"], info["visibility_radius"], info["visibility_min_support"], info["visibility_max_conflicts"]) == \
            (vkw["visibility_tol"], vkw.get("visibility_radius", 0), vkw.get("visibility_min_support", 1),
             vkw.get("visibility_max_conflicts", 0))


def test_command_line_flags_parse():
    a = pipeline.arg_parser().parse_args(["folder", "--voxel-size", "0.05", "--visibility-tol", "0.02", "--visibility-radius", "1",
                                          "--visibility-min-support", "2", "--visibility-max-conflicts", "3"])
    assert (a.visibility_tol, a.visibility_radius, a.visibility_min_support, a.visibility_max_conflicts) == (0.02, 1, 2, 3)
    d = pipeline.arg_parser().parse_args(["folder"])
    assert (d.visibility_tol, d.visibility_radius, d.visibility_min_support, d.visibility_max_conflicts) == (None, 0, 1, 0)
    with pytest.raises(SystemExit):
        pipeline.arg_parser().parse_args(["folder", "--visibility-radius", "2"])
