"""Pipeline.run_fusion's evaluation-region options (CPU, through the restated fusion with the restated regions):
n_valid falls to the restatement's inside count, eval.json gains "region", the flags need --eval-cloud."""
import json
import os

import numpy as np
import pytest

import cloud_distance_support as cd
import eval_region_support as er
from acmmp import io, pipeline
from pipeline_support import OracleEngine, small_dataset

F32 = np.float32


class RestatedRegionFusion(cd.RestatedDistanceFusion):
    """RestatedDistanceFusion with capi.Fusion's set_region / region_classify from the restatement: a measuring call sees
    x = NaN where the class of a point of a side with a region is not 0 (queries only: where the side is the query)."""

    def __init__(self, cams):
        super().__init__(cams)
        self.regions = {"data": None, "reference": None}

    def set_region(self, side, region, queries_only=False):
        if side not in self.regions:
            raise ValueError("bad side")
        self.regions[side] = None if region is None else (region, bool(queries_only))
        self._distance = None

    def region_classify(self, source):
        pts = self.reference if source == "reference" else self._data(source)[1]
        r = self.regions["reference" if source == "reference" else "data"]
        return er.counts(er.classify(pts, None if r is None else r[0]))

    def _cropped(self, side, pts, as_target):
        r = self.regions[side]
        if r is None or (as_target and r[1]):
            return pts
        return er.substituted(pts, er.classify(pts, r[0]))

    def cloud_distance(self, source="scene", direction="data_to_ref", max_dist=1.0, thresholds=()):
        held, data = self._data(source)
        d2r = direction == "data_to_ref"
        q = self._cropped("data", data, False) if d2r else self._cropped("reference", self.reference, False)
        t = self._cropped("reference", self.reference, True) if d2r else self._cropped("data", data, True)
        d2, nearest, words = cd.distances(q, t, max_dist, thresholds)
        self._distance = (held, self.reference, d2, nearest)
        return cd.Summary(words, max_dist, len(tuple(thresholds)))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("region")
    pipe = pipeline.Pipeline(small_dataset(64, 32, 3), engine=OracleEngine(), order="reference", geom_iterations=1,
                             out_folder=str(tmp / "out")).run()
    plain = pipe.run_fusion(fusion_factory=RestatedRegionFusion, ply_path=str(tmp / "a" / "cloud.ply"))
    return tmp, pipe, plain


def _half(plain, tmp):
    """A crop file that cuts the scene in half: a prism about Z over the lower half of the cloud's x range."""
    xyz = plain[:, :3].astype(np.float64)
    lo, hi = xyz.min(0) - 1.0, xyz.max(0) + 1.0
    mid = float(np.median(xyz[:, 0]))
    poly = [[lo[0], lo[1], 0.0], [mid, lo[1], 0.0], [mid, hi[1], 0.0], [lo[0], hi[1], 0.0]]
    path = str(tmp / "crop.json")
    with open(path, "w") as f:
        json.dump({"class_name": "SelectionPolygonVolume", "version_major": 1, "version_minor": 0, "orthogonal_axis": "Z",
                   "axis_min": float(lo[2]), "axis_max": float(hi[2]), "bounding_polygon": poly}, f)
    return path


def test_a_prism_that_halves_the_scene(run):
    tmp, pipe, plain = run
    path = _half(plain, tmp)
    want = er.counts(er.classify(plain, io.read_region(path)))
    assert 0.3 * len(plain) < want["inside"] < 0.7 * len(plain) and want["prism"] == len(plain) - want["inside"]
    shift = float((plain[:, :3].max(0) - plain[:, :3].min(0)).max()) / 200
    ref = plain[:, :3].copy()
    ref[:, 1] += F32(shift)
    kw = dict(fusion_factory=RestatedRegionFusion, eval_cloud=ref, eval_max_dist=4 * shift, eval_thresholds=(2 * shift,))
    pipe.run_fusion(**kw)
    whole = pipe.eval_info
    assert "region" not in whole and whole["accuracy"]["n_valid"] == len(plain)
    got = pipe.run_fusion(ply_path=str(tmp / "b" / "cloud.ply"), eval_region_data=path, **kw)
    assert got.tobytes() == plain.tobytes()
    assert (tmp / "b" / "cloud.ply").read_bytes() == (tmp / "a" / "cloud.ply").read_bytes()      # nothing is cropped away
    info = json.load(open(tmp / "b" / "eval.json"))
    assert info == json.loads(json.dumps(pipe.eval_info))
    assert info["region"] == {"data": {"file": path, "queries_only": False, "counts": want}}
    assert info["accuracy"]["n_query"] == len(plain) and info["accuracy"]["n_valid"] == want["inside"]
    # the other direction: the reference's queries are whole, their targets are the half
    assert info["completeness"]["n_valid"] == len(ref) and info["completeness"]["n_matched"] < whole["completeness"]["n_matched"]
    # queries only: the targets are whole again; and the reference side
    pipe.run_fusion(eval_region_data=path, eval_region_queries_only=True, eval_region_reference=io.read_region(path), **kw)
    info = pipe.eval_info
    assert info["region"]["data"]["queries_only"] and not info["region"]["reference"]["queries_only"]
    assert info["region"]["reference"]["file"] is None and info["region"]["reference"]["counts"]["points"] == len(ref)
    assert info["accuracy"]["n_valid"] == want["inside"]
    assert info["completeness"]["n_valid"] == info["region"]["reference"]["counts"]["inside"] == info["completeness"]["n_matched"]


def test_the_flags_need_eval_cloud(run):
    tmp, pipe, plain = run
    path = _half(plain, tmp)
    for kw in (dict(eval_region_data=path), dict(eval_region_reference=path), dict(eval_region_queries_only=True),
               dict(eval_cloud=plain[:, :3], eval_max_dist=1.0, eval_region_queries_only=True)):
        with pytest.raises(ValueError):
            pipe.run_fusion(fusion_factory=RestatedRegionFusion, **kw)
    with pytest.raises(ValueError):                        # and a fusion object that has regions
        pipe.run_fusion(fusion_factory=cd.RestatedDistanceFusion, eval_cloud=plain[:, :3], eval_max_dist=1.0, eval_region_data=path)


def test_cli_region_options():
    a = pipeline.arg_parser().parse_args(["folder", "--eval-cloud", "gt.ply", "--eval-max-dist", "0.02", "--eval-region-data",
                                          "crop.json", "--eval-region-reference", "obs.json", "--eval-region-queries-only"])
    assert (a.eval_region_data, a.eval_region_reference, a.eval_region_queries_only) == ("crop.json", "obs.json", True)
    a = pipeline.arg_parser().parse_args(["folder"])
    assert (a.eval_region_data, a.eval_region_reference, a.eval_region_queries_only) == (None, None, False)
