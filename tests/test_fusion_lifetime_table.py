"""The lifetime table of the fusion results (csrc/fusion_results.h) on the host alone: the table and the source maps
hold no HIP type, so fusion_lifetime_walk.cpp compiles them with the host compiler under the address and undefined-
behaviour sanitizers and applies the table transitively, as fusion.cpp's invalidate does.  For every replacing call of
every configuration the set released must be the row of test_gpu_fusion_lifetimes.EXPECTED."""
import os
import subprocess

import pytest

import test_gpu_fusion_lifetimes as lt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what a replacing call replaces
CAUSE = {"run_scene": "scene", "set_scene": "scene", "voxelize": "voxels", "voxel_clean": "clean",
         "visibility<voxel": "visible", "visibility<clean": "visible", "mesh<voxel": "mesh", "mesh<clean": "mesh",
         "mesh<visible": "mesh", "set_mesh": "mesh", "mesh_render": "render", "set_reference_cloud": "reference",
         "set_cloud_transform": "transform", "clear_cloud_transform": "transform", "cloud_distance": "distance",
         "surface_distance": "surface", "cloud_align": "align", "cloud_align_plane": "align"}
# the Python binding's names of the voxel cloud
CLOUD = {"voxel": "voxels", None: "none"}


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("walk") / "fusion_lifetime_walk")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "acmmp-spherical_amd", "csrc"),
                    os.path.join(ROOT, "tests", "fusion_lifetime_walk.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("config", list(lt.CONFIGS))
def test_table_releases_what_the_matrix_expects(walk, config):
    cfg = lt.CONFIGS[config]
    sources = [cfg["visible"], cfg["mesh"], cfg["distance"], cfg["surface"], cfg["align"][1]]
    out = subprocess.run([walk] + [CLOUD.get(s, s) for s in sources], check=True, capture_output=True, text=True)
    assert out.stderr == ""
    released = dict(line.split() for line in out.stdout.splitlines())
    assert set(released) == set(CAUSE.values())
    assert set(CAUSE) == set(lt.CALLS)
    for call, row in zip(lt.CALLS, lt.EXPECTED[config]):
        assert released[CAUSE[call]] == row.replace("=", "K"), (config, call)
