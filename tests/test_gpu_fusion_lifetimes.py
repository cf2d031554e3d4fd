"""The whole lifetime graph of the fusion object's resident results (include/acmmp.h, the lifetime paragraphs of every
stage): every replacing call against every held result.  Each stage's own test walks its own edges; this one crosses
them -- a voxelize against a render of a mesh of the visible cloud, set_cloud_transform against a surface result
queried from the reference, set_mesh against align records on "mesh".

A configuration says which source each held result was computed from.  Per configuration EXPECTED holds one row per
replacing call and one letter per held result, in the order of HELD: G = gone (its reader refuses a one-element
range), K = kept, = the result the call itself installs (present afterwards)."""
import numpy as np
import pytest

import visibility_support as vis
from acmmp import capi
from fusion_scene_support import fill

pytestmark = pytest.mark.gpu

F32 = np.float32
HELD = ("voxels", "clean", "visible", "mesh", "render", "distance", "surface", "align")

# which source each held result of a configuration comes from; mesh None = installed by set_mesh
CONFIGS = {
    "deep": dict(visible="clean", mesh="visible", distance="visible", surface="visible", align=("point", "visible")),
    "clean": dict(visible="voxel", mesh="clean", distance="clean", surface="clean", align=("plane", "clean")),
    "voxels": dict(visible="clean", mesh="voxel", distance="voxels", surface="voxels", align=("point", "voxels")),
    "set": dict(visible="voxel", mesh=None, distance="mesh", surface="reference", align=("plane", "mesh")),
    "scene": dict(visible="clean", mesh=None, distance="scene", surface="scene", align=("point", "scene")),
}

CALLS = ("run_scene", "set_scene", "voxelize", "voxel_clean", "visibility<voxel", "visibility<clean", "mesh<voxel",
         "mesh<clean", "mesh<visible", "set_mesh", "mesh_render", "set_reference_cloud", "set_cloud_transform",
         "clear_cloud_transform", "cloud_distance", "surface_distance", "cloud_align", "cloud_align_plane")

# rows in the order of CALLS, letters in the order of HELD
EXPECTED = {
    #            V C S M R D F A
    "deep": ("GGGGGGGG",    # run_scene: everything described the previous scene
             "GGGGGGGG",    # set_scene
             "=GGGGGGG",    # voxelize
             "K=GGGGGG",    # voxel_clean: visible < clean, and the chain on it
             "KK=GGGGG",    # visibility from either source: mesh < visible, render, distance, surface, align < visible
             "KK=GGGGG",
             "KKK=GKGK",    # a mesh call: the render and the surface result
             "KKK=GKGK",
             "KKK=GKGK",
             "KKK=GKGK",    # set_mesh
             "KKKK=KKK",    # mesh_render
             "KKKKKGKG",    # set_reference_cloud: distance, align; a data query's surface result stays
             "KKKKKGKK",    # set_cloud_transform: distance only
             "KKKKKGKK",
             "KKKKK=KK", "KKKKKK=K", "KKKKKKK=", "KKKKKKK="),
    "clean": ("GGGGGGGG", "GGGGGGGG", "=GGGGGGG",
              "K=KGGGGG",   # voxel_clean: a visible result of the voxels stays; mesh < clean and what hangs on it go
              "KK=KKKKK", "KK=KKKKK",
              "KKK=GKGK", "KKK=GKGK", "KKK=GKGK", "KKK=GKGK", "KKKK=KKK",
              "KKKKKGKG", "KKKKKGKK", "KKKKKGKK",
              "KKKKK=KK", "KKKKKK=K", "KKKKKKK=", "KKKKKKK="),
    "voxels": ("GGGGGGGG", "GGGGGGGG", "=GGGGGGG",
               "K=GKKKKK",  # voxel_clean: visible < clean only
               "KK=KKKKK", "KK=KKKKK",
               "KKK=GKGK", "KKK=GKGK", "KKK=GKGK", "KKK=GKGK", "KKKK=KKK",
               "KKKKKGKG", "KKKKKGKK", "KKKKKGKK",
               "KKKKK=KK", "KKKKKK=K", "KKKKKKK=", "KKKKKKK="),
    "set": ("GGGKKKKK",     # a set mesh outlives the scene, with its render and what was measured on it
            "GGGKKKKK",
            "=GGKKKKK", "K=KKKKKK", "KK=KKKKK", "KK=KKKKK",
            "KKK=GGGG",     # a mesh call: render, distance < mesh, surface, align < mesh
            "KKK=GGGG", "KKK=GGGG", "KKK=GGGG", "KKKK=KKK",
            "KKKKKGGG",     # set_reference_cloud: a reference query's surface result too
            "KKKKKGGK",     # set_cloud_transform: distance, and a reference query's surface result
            "KKKKKGGK",
            "KKKKK=KK", "KKKKKK=K", "KKKKKKK=", "KKKKKKK="),
    "scene": ("GGGKKGGG",   # the set mesh and its render stay; what was measured on the scene goes
              "GGGKKGGG",
              "=GGKKKKK", "K=GKKKKK", "KK=KKKKK", "KK=KKKKK",
              "KKK=GKGK", "KKK=GKGK", "KKK=GKGK", "KKK=GKGK", "KKKK=KKK",
              "KKKKKGKG", "KKKKKGKK", "KKKKKGKK",
              "KKKKK=KK", "KKKKKK=K", "KKKKKKK=", "KKKKKKK="),
}

M_TEST = np.array([[1, 0, 0, 0.001], [0, 1, 0, 0], [0, 0, 1, -0.001]], np.float64)


class _Rig:
    """One fusion object on the constructed sphere rig, and the calls that build and replace its results."""

    def __init__(self):
        self.cams, depths, normals, colours, self.cloud, self.size = vis.constructed("sphere")
        self.views = list(range(len(self.cams)))
        self.fu = fill(capi.Fusion(0, self.cams), self.cams, depths, normals, colours)
        self.fu.set_scene(self.cloud)                                          # voxelised as test_gpu_cloud_distance._chain does
        voxels = self.fu.voxel_points(0, self.fu.voxelize(self.size)[0])
        self.ref = (voxels[::2, :3] + F32(0.25 * self.size)).astype(F32)
        nv, nf, _ = self.fu.voxel_mesh(self.views, 3 * self.size)
        assert nv > 0 and nf > 0
        self.host_mesh = (self.fu.mesh_vertices(0, nv), self.fu.mesh_faces(0, nf))   # what set_mesh installs

    def call(self, name, cfg):
        fu, size = self.fu, self.size
        kind, source = name.partition("<")[::2]
        if name == "run_scene":
            return fu.run_scene([0], [[1, 2]])
        if name == "set_scene":
            return fu.set_scene(self.cloud)
        if name == "voxelize":
            return fu.voxelize(size)
        if name == "voxel_clean":
            return fu.voxel_clean(26, 1, 2, 1)
        if kind == "visibility":
            return fu.voxel_visibility(self.views, 0.01, 1, 1, 0, source=source)
        if kind == "mesh":
            return fu.voxel_mesh(self.views, 3 * size, source=source)
        if name == "set_mesh":
            return fu.set_mesh(*self.host_mesh)
        if name == "mesh_render":
            return fu.render_mesh(0)
        if name == "set_reference_cloud":
            return fu.set_reference_cloud(self.ref)
        if name == "set_cloud_transform":
            return fu.set_cloud_transform(M_TEST)
        if name == "clear_cloud_transform":
            return fu.set_cloud_transform(None)
        if name == "cloud_distance":
            return fu.cloud_distance(cfg["distance"], "data_to_ref", size, (size,))
        if name == "surface_distance":
            return fu.surface_distance(cfg["surface"], size, (size,))
        if name == "cloud_align":
            return fu.cloud_align(cfg["align"][1], "rigid", size, 2)
        if name == "cloud_align_plane":
            return fu.cloud_align_plane(cfg["align"][1], size, 2)
        raise KeyError(name)

    def hold(self, cfg):
        """Every result of the configuration resident, each computed from the source the configuration names."""
        for name in ("set_scene", "voxelize", "voxel_clean", "visibility<" + cfg["visible"],
                     "set_mesh" if cfg["mesh"] is None else "mesh<" + cfg["mesh"], "mesh_render", "set_reference_cloud",
                     "cloud_distance", "surface_distance", "cloud_align_plane" if cfg["align"][0] == "plane" else "cloud_align"):
            self.call(name, cfg)

    def gone(self):
        """Per held result: does its reader refuse a one-element range (ACMMP_ERR_INVALID_ARGUMENT)?"""
        L, h = self.fu.L, self.fu.h
        rc = {"voxels": L.acmmp_fusion_voxel_points(h, 0, 1, None, None),
              "clean": L.acmmp_fusion_clean_points(h, 0, 1, None, None, None),
              "visible": L.acmmp_fusion_visible_points(h, 0, 1, None, None, None),
              "mesh": L.acmmp_fusion_mesh_vertices(h, 0, 1, None),
              "render": L.acmmp_fusion_render_maps(h, None, None, None, None),
              "distance": L.acmmp_fusion_distance_results(h, 0, 1, None, None),
              "surface": L.acmmp_fusion_surface_results(h, 0, 1, None, None),
              "align": min(L.acmmp_fusion_align_records(h, 0, 1, None, None, None),
                           L.acmmp_fusion_align_plane_records(h, 0, 1, None, None, None))}
        assert set(rc.values()) <= {0, 1}, rc
        return {k: v == 1 for k, v in rc.items()}


@pytest.fixture(scope="module")
def rig():
    r = _Rig()
    yield r
    r.fu.close()


@pytest.mark.parametrize("config", list(CONFIGS))
def test_every_call_against_every_held_result(rig, config):
    cfg = CONFIGS[config]
    assert len(EXPECTED[config]) == len(CALLS)
    wrong = []
    for name, row in zip(CALLS, EXPECTED[config]):
        rig.hold(cfg)
        before = rig.gone()
        assert not any(before.values()), f"{config}: not everything is held before {name}: {before}"
        rig.call(name, cfg)
        after = rig.gone()
        got = "".join("G" if after[r] else "K" for r in HELD)
        print(config, name, "expected", row, "got", got)
        if got != row.replace("=", "K"):
            wrong.append((name, row, got))
        if name.startswith("cloud_align"):                                     # one kind of records at a time
            L, h = rig.fu.L, rig.fu.h
            plane = name == "cloud_align_plane"
            assert L.acmmp_fusion_align_records(h, 0, 1, None, None, None) == (1 if plane else 0)
            assert L.acmmp_fusion_align_plane_records(h, 0, 1, None, None, None) == (0 if plane else 1)
    assert not wrong, f"{config}: (call, expected, got) {wrong}"
