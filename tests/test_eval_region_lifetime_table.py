"""The rows of the lifetime table (csrc/fusion_results.h) that the evaluation regions add, on the host alone:
eval_region_lifetime_walk.cpp is compiled with the host compiler under the address and undefined-behaviour sanitizers,
as mesh_sample_lifetime_walk.cpp is, and applies goes_with transitively with the class result held and R_REGION among
the causes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELD = ("voxels", "clean", "visible", "mesh", "samples", "render", "distance", "surface", "align", "classes")


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("walk") / "eval_region_lifetime_walk")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "acmmp-spherical_amd", "csrc"),
                    os.path.join(ROOT, "tests", "eval_region_lifetime_walk.cpp"), "-o", exe], check=True)
    return exe


def released(walk, mesh, distance, surface, align, classes):
    """cause -> the set of held results that go with it."""
    out = subprocess.run([walk, mesh, distance, surface, align, classes], check=True, capture_output=True, text=True)
    assert out.stderr == ""
    rows = dict(line.split() for line in out.stdout.splitlines())
    # the earlier enumerators keep their values, the two new names follow R_SAMPLES
    assert rows.pop("enumerators") == "10,11,12,13,0"
    # ACMMP_DIST_FROM_* name the data clouds, ACMMP_SURF_FROM_REFERENCE (5) the reference cloud
    assert rows.pop("sources") == "scene,voxels,clean,visible,mesh,reference,samples,none"
    return {cause: {h for h, c in zip(HELD, row) if c == "G"} for cause, row in rows.items()}


def test_region_as_a_cause(walk):
    gone = released(walk, "visible", "scene", "reference", "voxels", "scene")
    # a set or clear: the distance, surface and align results and the classes; no cloud, no mesh
    assert gone["region"] == {"distance", "surface", "align", "classes"}
    # nothing goes with a classify call
    assert gone["classes"] == set()
    assert all(gone[c] == set() for c in ("render", "distance", "surface", "align"))


def test_classes_of_a_data_cloud(walk):
    gone = released(walk, "none", "voxels", "reference", "voxels", "scene")
    assert "classes" in gone["scene"] and "classes" in gone["transform"]
    for cause in ("voxels", "clean", "visible", "mesh", "samples", "reference"):
        assert "classes" not in gone[cause], cause
    # of a cloud further down the chain: with everything upstream of it
    gone = released(walk, "visible", "scene", "reference", "scene", "samples")
    for cause in ("scene", "voxels", "clean", "visible", "mesh", "samples", "transform", "region"):
        assert "classes" in gone[cause], cause
    assert "classes" not in gone["reference"]


def test_classes_of_the_reference_cloud(walk):
    gone = released(walk, "none", "scene", "scene", "scene", "reference")
    assert "classes" in gone["reference"] and "classes" in gone["region"]
    for cause in ("scene", "voxels", "clean", "visible", "mesh", "samples", "transform"):
        assert "classes" not in gone[cause], cause


def test_the_earlier_rows_are_unchanged(walk):
    """The matrix of test_mesh_sample_lifetime_table.py, with the class column beside it."""
    gone = released(walk, "visible", "samples", "reference", "samples", "mesh")
    chain = {"mesh", "samples", "render", "distance", "surface", "align", "classes"}
    assert gone["mesh"] == chain - {"mesh"}
    assert gone["visible"] == chain
    assert gone["scene"] == chain | {"visible", "clean", "voxels"}
    assert gone["samples"] == {"distance", "align"}
    assert gone["reference"] == {"distance", "surface", "align"}
    assert gone["transform"] == {"distance", "surface", "classes"}
