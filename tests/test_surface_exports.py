"""The point-to-triangle entry points: declared in include/acmmp.h, exported by the library, listed in capi.EXPORTS; the
Python wrappers refuse bad arguments before they reach the library (no device)."""
import os
import re
import subprocess

import numpy as np
import pytest

from acmmp import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("acmmp_fusion_surface_distance", "acmmp_fusion_surface_results", "acmmp_fusion_surface_plan",
           "acmmp_fusion_surface_grid")


def test_declared_exported_and_listed():
    header = open(os.path.join(REPO, "include", "acmmp.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert re.search(r"acmmp_status\s+" + name + r"\s*\(", header), name
        assert name in capi.EXPORTS, name
        assert re.search(r"\sT\s+" + name + r"\s", exported), name
    consts = dict(re.findall(r"#define\s+ACMMP_SURF_FROM_(\w+)\s+(\d+)", header))
    assert {k.lower(): int(v) for k, v in consts.items()} == capi.SURF_QUERIES
    for k in ("scene", "voxels", "clean", "visible"):                      # a data cloud's constant is its ACMMP_DIST_FROM_*
        assert capi.SURF_QUERIES[k] == capi.DIST_SOURCES[k]
    assert capi.SURF_QUERIES["reference"] not in capi.DIST_SOURCES.values()


def test_wrappers_refuse_bad_arguments_without_a_device():
    fu = capi.Fusion.__new__(capi.Fusion)                                  # no library handle: a call would fail loudly
    fu.L = fu.h = None
    for kw in (dict(query="mesh"), dict(query="cloud"), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float("nan")),
               dict(max_dist=float("inf")), dict(thresholds=[0.1] * 9), dict(thresholds=[-0.1]), dict(thresholds=[2.0]),
               dict(thresholds=[float("nan")])):
        with pytest.raises(ValueError):
            fu.surface_distance(**{"query": "reference", "max_dist": 1.0, **kw})
    for args in ((-1, 1), (0, -1)):
        with pytest.raises(ValueError):
            fu.surface_results(*args)
    with pytest.raises(ValueError):
        fu.surface_plan(2 ** 31)
    with pytest.raises(AttributeError):                                    # a good call does reach the library
        fu.surface_distance("reference", 1.0, np.array([0.5], np.float32))
