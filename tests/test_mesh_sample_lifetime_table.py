"""The rows of the lifetime table (csrc/fusion_results.h) that concern the sample result, on the host alone:
mesh_sample_lifetime_walk.cpp is compiled with the host compiler under the address and undefined-behaviour sanitizers,
as fusion_lifetime_walk.cpp is, and applies goes_with transitively with R_SAMPLES held."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELD = ("voxels", "clean", "visible", "mesh", "samples", "render", "distance", "surface", "align")


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("walk") / "mesh_sample_lifetime_walk")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "acmmp-spherical_amd", "csrc"),
                    os.path.join(ROOT, "tests", "mesh_sample_lifetime_walk.cpp"), "-o", exe], check=True)
    return exe


def released(walk, mesh, distance, surface, align):
    """cause -> the set of held results that go with it."""
    out = subprocess.run([walk, mesh, distance, surface, align], check=True, capture_output=True, text=True)
    assert out.stderr == ""
    rows = dict(line.split() for line in out.stdout.splitlines())
    assert rows.pop("constant") == "6" and rows.pop("surface_source") == "other"     # ACMMP_DIST_FROM_SAMPLES; no surface source
    return {cause: {h for h, c in zip(HELD, row) if c == "G"} for cause, row in rows.items()}


def test_samples_of_a_voxel_mesh(walk):
    """The mesh of the visible result, the distance result and the align records of the samples."""
    gone = released(walk, "visible", "samples", "reference", "samples")
    # the samples go with the mesh and with whatever discards the mesh upstream, and take what was measured on them
    chain = {"mesh", "samples", "render", "distance", "surface", "align"}
    assert gone["mesh"] == chain - {"mesh"}
    assert gone["visible"] == chain
    assert gone["clean"] == chain | {"visible"}
    assert gone["voxels"] == chain | {"visible", "clean"}
    assert gone["scene"] == chain | {"visible", "clean", "voxels"}
    # replaced samples release only the distance result and the align records computed from them
    assert gone["samples"] == {"distance", "align"}
    # the reference cloud and the transform leave the samples alone
    assert gone["reference"] == {"distance", "surface", "align"}
    assert gone["transform"] == {"distance", "surface"}
    # and nothing goes with a render, a distance, a surface or an align call
    assert all(gone[c] == set() for c in ("render", "distance", "surface", "align"))


def test_samples_of_a_set_mesh(walk):
    """A mesh without a source: its samples survive the scene, the voxels, the clean and the visible result."""
    gone = released(walk, "none", "samples", "scene", "mesh")
    for cause in ("scene", "voxels", "clean", "visible"):
        assert not gone[cause] & {"mesh", "samples", "render", "distance"}, cause
    assert gone["mesh"] == {"samples", "render", "distance", "surface", "align"}
    assert gone["samples"] == {"distance"}


def test_results_of_other_clouds_outlive_the_samples(walk):
    gone = released(walk, "voxels", "mesh", "reference", "voxels")
    assert gone["samples"] == set()
    assert "samples" in gone["mesh"] and "samples" in gone["voxels"] and "samples" in gone["scene"]
    assert "samples" not in gone["clean"] and "samples" not in gone["reference"]
