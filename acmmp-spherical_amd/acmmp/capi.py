"""ctypes binding of the C ABI in include/acmmp.h (libacmmp.so, built in-tree for gfx950).

This is the Python-side FFI a maintainer would add next to the reference;
tests and bench.py drive the engine only through it.  There is no fallback: if the HIP
library is missing or no GPU is visible, every call fails loudly.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import mmap
import os
import threading
import weakref

import numpy as np

from .types import CAMERA_DTYPE, PARAMS_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
# ACMMP_LIB selects another in-tree build of the same library (A/B experiments); default: the product build
LIB_PATH = os.environ.get("ACMMP_LIB") or os.path.join(HERE, "libacmmp.so")

class _HostPool:
    """Recycled page-aligned private mappings for large D2H destinations.  Fresh heap pages made the copy into
    them crawl (30 ms for a 800x600 view's planes + costs, 0.9 ms into a hugepage mapping,
    profiles/r05_d2h_probe.json), and a new mapping per download pays its page faults every time: a mapping
    comes back here when the last array (or view) on it is collected and the next download of that size
    reuses its resident pages.  At most `cap` bytes are kept idle (ACMMP_HOST_POOL_BYTES, default 1 GiB):
    beyond it the least recently returned mappings are dropped, so sizes a pipeline no longer requests (an
    earlier pyramid scale) do not stay held; release() drops them all."""

    def __init__(self, cap: int | None = None):
        if cap is None:
            cap = int(os.environ.get("ACMMP_HOST_POOL_BYTES", str(1 << 30)))
        self.cap, self.held = cap, 0
        self.free = {}                      # size -> [mapping]; insertion order of `order` = recency
        self.order = []                     # (size, mapping) in the order they came back, oldest first
        self.lock = threading.Lock()

    def take(self, n: int):
        with self.lock:
            lst = self.free.get(n)
            if lst:
                mm = lst.pop()
                self.order = [(k, m) for (k, m) in self.order if m is not mm]
                self.held -= n
                return mm
        mm = mmap.mmap(-1, n, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS)
        if hasattr(mmap, "MADV_HUGEPAGE"):
            mm.madvise(mmap.MADV_HUGEPAGE)
        return mm

    def give(self, mm, n: int):
        # (called while the array still holds its buffer export: a dropped mapping is unmapped when the last
        # reference goes, not closed here)
        if n > self.cap:
            return
        with self.lock:
            while self.held + n > self.cap and self.order:
                k, old = self.order.pop(0)              # least recently returned first
                self.free[k].remove(old)
                self.held -= k
            self.free.setdefault(n, []).append(mm)
            self.order.append((n, mm))
            self.held += n

    def release(self):
        """Drop every idle mapping (e.g. when a pipeline evicts a pyramid scale)."""
        with self.lock:
            self.free, self.order, self.held = {}, [], 0


_POOL = _HostPool()


def host_empty(shape, dtype=np.float32) -> np.ndarray:
    """An uninitialised host array for a D2H copy: arrays of 4 MiB and up live on a 2 MiB aligned private
    mapping advised MADV_HUGEPAGE from _HostPool (see there); smaller ones are plain np.empty."""
    dt = np.dtype(dtype)
    count = int(np.prod(shape))
    n = count * dt.itemsize
    if n < (4 << 20):
        return np.empty(shape, dt)
    size = (n + (2 << 20) - 1) // (2 << 20) * (2 << 20) + (2 << 20)     # whole 2 MiB pages + alignment slack
    mm = _POOL.take(size)
    base = np.frombuffer(mm, np.uint8)
    off = (-base.ctypes.data) % (2 << 20)
    del base
    flat = np.frombuffer(mm, dt, count, off)       # the base every view of the result keeps alive
    weakref.finalize(flat, _POOL.give, mm, size)
    return flat.reshape(shape)


STATUS = {0: "ok", 1: "invalid argument", 2: "HIP runtime error", 3: "out of device memory",
          4: "call order violated", 5: "unsupported configuration", 6: "no HIP device"}

# Every symbol include/acmmp.h declares (checked against the header by tests/test_capi_exports.py).
EXPORTS = [
    "acmmp_abi_version", "acmmp_device_count", "acmmp_create", "acmmp_destroy", "acmmp_status_str", "acmmp_last_error",
    "acmmp_set_params", "acmmp_upload_views", "acmmp_upload_depths", "acmmp_set_state",
    "acmmp_set_scaled_state", "acmmp_set_planar_prior", "acmmp_run_patchmatch", "acmmp_run_patchmatch_ex",
    "acmmp_download", "acmmp_download_aux", "acmmp_device_outputs", "acmmp_synchronize", "acmmp_last_timing",
    "acmmp_last_kernel_timing", "acmmp_last_work", "acmmp_last_planar_timing", "acmmp_texel_bytes", "acmmp_set_math", "acmmp_get_math", "acmmp_jbu",
    "acmmp_debug_ncc", "acmmp_debug_geom", "acmmp_debug_ncc_nb", "acmmp_debug_ncc_ref", "acmmp_debug_band_cvec",
    "acmmp_debug_band_keep_mask", "acmmp_keep_mask_bytes",
    "acmmp_support_points", "acmmp_delaunay", "acmmp_prior_plane_params", "acmmp_depth_from_plane_param",
    "acmmp_planar_prior_host", "acmmp_set_planar_prior_from_maps", "acmmp_set_planar_prior_from_state",
    "acmmp_download_planar_prior",
    "acmmp_upload_depths_device", "acmmp_upload_views_device", "acmmp_export_depth", "acmmp_export_state", "acmmp_set_state_device", "acmmp_device_alloc", "acmmp_device_free", "acmmp_memcpy",
    "acmmp_comm_unique_id", "acmmp_comm_create", "acmmp_comm_destroy", "acmmp_comm_broadcast", "acmmp_comm_after",
    "acmmp_comm_allreduce_max", "acmmp_comm_band_exchange", "acmmp_run_patchmatch_band",
    "acmmp_band_begin", "acmmp_band_sweep", "acmmp_band_sweeps_left", "acmmp_band_halo_ranges",
    "acmmp_band_copy_rows", "acmmp_band_get_rows", "acmmp_band_set_rows", "acmmp_band_end",
    "acmmp_strip_plan",
    "acmmp_fusion_create", "acmmp_fusion_set_view", "acmmp_fusion_run", "acmmp_fusion_last_error",
    "acmmp_fusion_destroy", "acmmp_fusion_run_scene", "acmmp_fusion_scene_points", "acmmp_fusion_reset_used",
    "acmmp_fusion_download_used", "acmmp_fusion_voxelize", "acmmp_fusion_voxel_points", "acmmp_fusion_voxel_table",
    "acmmp_fusion_set_scene", "acmmp_fusion_voxel_clean", "acmmp_fusion_clean_points", "acmmp_fusion_voxel_labels",
    "acmmp_fusion_component_table",
    "acmmp_fusion_voxel_visibility", "acmmp_fusion_visible_points", "acmmp_fusion_visibility_tallies",
    "acmmp_fusion_voxel_mesh", "acmmp_fusion_mesh_vertices", "acmmp_fusion_mesh_faces", "acmmp_fusion_mesh_samples",
    "acmmp_fusion_mesh_table", "acmmp_fusion_set_mesh", "acmmp_fusion_mesh_render", "acmmp_fusion_render_maps",
    "acmmp_fusion_render_plan",
    "acmmp_fusion_set_reference_cloud", "acmmp_fusion_cloud_distance", "acmmp_fusion_distance_results",
    "acmmp_fusion_distance_grid",
    "acmmp_fusion_surface_distance", "acmmp_fusion_surface_results", "acmmp_fusion_surface_plan",
    "acmmp_fusion_surface_grid",
    "acmmp_fusion_mesh_sample", "acmmp_fusion_sample_points",
    "acmmp_fusion_set_cloud_transform", "acmmp_fusion_get_cloud_transform", "acmmp_fusion_cloud_align",
    "acmmp_fusion_align_records", "acmmp_fusion_cloud_align_plane", "acmmp_fusion_align_plane_records",
    "acmmp_fusion_set_region", "acmmp_fusion_get_region", "acmmp_fusion_region_classify", "acmmp_fusion_region_classes",
    "acmmp_image_cache_create", "acmmp_image_cache_destroy", "acmmp_image_cache_stats",
    "acmmp_upload_views_keyed", "acmmp_device_checksum", "acmmp_device_identity", "acmmp_clock_probe",
]


class AcmmpError(RuntimeError):
    pass


def keep_mask_bytes(W: int, H: int, model: int = 11, patch_size: int = 11, radius_increment: int = 2, fast: bool = True,
                    tex16: bool = True, n_src: int = 4, geom: bool = False) -> int:
    """Bytes the kept-sample mask adds to the scratch slab of such a run under the current environment
    (acmmp_keep_mask_bytes: the run's own gates; no GPU needed); 0 where the run publishes none."""
    n = int(load_library().acmmp_keep_mask_bytes(int(W), int(H), int(model), int(patch_size), int(radius_increment),
                                                 int(bool(fast)), int(bool(tex16)), int(n_src), int(bool(geom))))
    if n < 0:
        raise AcmmpError(f"keep_mask_bytes: invalid arguments ({W} x {H})")
    return n


def strip_plan(rows: int, want_strips: int):
    """The strip schedule of a run over `rows` checkerboard rows (acmmp_strip_plan; no GPU needed):
    (bounds, waits) with strip i = rows [bounds[i], bounds[i + 1]) and waits[i] the strips whose previous
    half-sweep strip i's next one waits for."""
    L = load_library()
    bounds = np.zeros(65, np.int32)
    waits = np.full(192, -1, np.int32)
    ns = int(L.acmmp_strip_plan(int(rows), int(want_strips), _p(bounds), _p(waits)))
    if ns < 1:
        raise AcmmpError(f"strip_plan: invalid arguments (rows={rows})")
    return [int(b) for b in bounds[:ns + 1]], [[int(w) for w in waits[3 * i:3 * i + 3] if w >= 0] for i in range(ns)]


_lib = None


def load_library(path: str = LIB_PATH):
    """Load libacmmp.so (no GPU needed to load it)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise AcmmpError(f"{path} is missing: build it with `python acmmp-spherical_amd/build.py` "
                         "(there is no CPU fallback)")
    L = C.CDLL(path)
    vp, i32, u64 = C.c_void_p, C.c_int, C.c_uint64
    L.acmmp_abi_version.restype = i32
    L.acmmp_device_count.restype = i32
    L.acmmp_create.argtypes = [i32, C.POINTER(vp)]
    L.acmmp_destroy.argtypes = [vp]
    L.acmmp_destroy.restype = None
    L.acmmp_status_str.argtypes = [i32]
    L.acmmp_status_str.restype = C.c_char_p
    L.acmmp_last_error.argtypes = [vp]
    L.acmmp_last_error.restype = C.c_char_p
    L.acmmp_set_params.argtypes = [vp, vp]
    L.acmmp_upload_views.argtypes = [vp, i32, vp, vp, vp]
    L.acmmp_upload_depths.argtypes = [vp, i32, vp, vp, vp]
    L.acmmp_set_state.argtypes = [vp, vp, vp]
    L.acmmp_set_scaled_state.argtypes = [vp, vp, i32, i32]
    L.acmmp_set_planar_prior.argtypes = [vp, vp, vp]
    L.acmmp_run_patchmatch.argtypes = [vp, u64]
    L.acmmp_run_patchmatch_ex.argtypes = [vp, u64, i32, i32]
    L.acmmp_download.argtypes = [vp, vp, vp]
    L.acmmp_download_aux.argtypes = [vp, vp, vp]
    L.acmmp_device_outputs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.acmmp_last_timing.argtypes = [vp, vp]
    L.acmmp_last_kernel_timing.argtypes = [vp, vp, vp]
    L.acmmp_last_work.argtypes = [vp, vp, vp]
    L.acmmp_last_planar_timing.argtypes = [vp, vp]
    L.acmmp_texel_bytes.argtypes = [vp]
    L.acmmp_set_math.argtypes = [vp, i32]
    L.acmmp_get_math.argtypes = [vp]
    L.acmmp_synchronize.argtypes = [vp]
    L.acmmp_jbu.argtypes = [vp, vp, i32, i32, vp, i32, i32, i32, vp]
    L.acmmp_debug_ncc.argtypes = [vp, i32, vp, vp, vp, vp]
    L.acmmp_debug_geom.argtypes = [vp, i32, vp, vp, vp, vp]
    L.acmmp_debug_ncc_nb.argtypes = [vp, i32, vp, vp, vp, vp]
    L.acmmp_debug_ncc_ref.argtypes = [vp, i32, vp, vp, vp, vp]
    L.acmmp_support_points.argtypes = [vp, i32, i32, vp, i32, vp]
    L.acmmp_delaunay.argtypes = [vp, i32, i32, i32, vp, i32, vp]
    L.acmmp_prior_plane_params.argtypes = [vp, vp, i32, i32, vp, vp]
    L.acmmp_depth_from_plane_param.argtypes = [vp, vp, i32, i32]
    L.acmmp_upload_depths_device.argtypes = [vp, i32, vp, vp, vp]
    L.acmmp_upload_views_device.argtypes = [vp, i32, vp, vp, vp]
    L.acmmp_export_depth.argtypes = [vp, vp]
    L.acmmp_export_state.argtypes = [vp, vp, vp]
    L.acmmp_set_state_device.argtypes = [vp, vp, vp]
    L.acmmp_device_alloc.argtypes = [i32, C.c_size_t, C.POINTER(vp)]
    L.acmmp_device_free.argtypes = [i32, vp]
    L.acmmp_memcpy.argtypes = [i32, vp, vp, C.c_size_t, i32]
    L.acmmp_comm_unique_id.argtypes = [vp]
    L.acmmp_comm_create.argtypes = [i32, vp, i32, i32, C.POINTER(vp)]
    L.acmmp_comm_destroy.argtypes = [vp]
    L.acmmp_comm_broadcast.argtypes = [vp, i32, vp, vp, vp]
    L.acmmp_comm_after.argtypes = [vp, vp]
    L.acmmp_comm_allreduce_max.argtypes = [vp, vp, i32]
    L.acmmp_comm_band_exchange.argtypes = [vp, vp, i32, i32, i32]
    L.acmmp_run_patchmatch_band.argtypes = [vp, vp, u64, i32, i32, i32, i32]
    L.acmmp_band_begin.argtypes = [vp, u64, i32, i32]
    L.acmmp_band_sweep.argtypes = [vp, C.POINTER(i32)]
    L.acmmp_band_sweeps_left.argtypes = [vp]
    L.acmmp_band_halo_ranges.argtypes = [vp, vp]
    L.acmmp_strip_plan.argtypes = [i32, i32, vp, vp]
    L.acmmp_band_copy_rows.argtypes = [vp, vp, i32, i32, i32]
    L.acmmp_band_get_rows.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    L.acmmp_band_set_rows.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    L.acmmp_debug_band_cvec.argtypes = [vp, i32, i32, i32, vp]
    L.acmmp_debug_band_keep_mask.argtypes = [vp, i32, i32, i32, vp]
    L.acmmp_keep_mask_bytes.argtypes = [i32] * 9
    L.acmmp_keep_mask_bytes.restype = C.c_longlong
    L.acmmp_band_end.argtypes = [vp, i32]
    L.acmmp_fusion_create.argtypes = [i32, i32, vp, C.POINTER(vp)]
    L.acmmp_fusion_set_view.argtypes = [vp, i32, vp, vp, vp]
    L.acmmp_fusion_run.argtypes = [vp, i32, i32, vp, vp, i32, vp]
    L.acmmp_fusion_last_error.argtypes = [vp]
    L.acmmp_fusion_destroy.argtypes = [vp]
    L.acmmp_fusion_run_scene.argtypes = [vp, i32, vp, vp, vp, i32, vp, C.POINTER(C.c_int64)]
    L.acmmp_fusion_scene_points.argtypes = [vp, C.c_int64, C.c_int64, vp, vp, vp, vp]
    L.acmmp_fusion_reset_used.argtypes = [vp]
    L.acmmp_fusion_download_used.argtypes = [vp, i32, vp]
    L.acmmp_fusion_voxelize.argtypes = [vp, C.c_float, vp, i32, vp, vp, vp, vp]
    L.acmmp_fusion_voxel_points.argtypes = [vp, C.c_int64, C.c_int64, vp, vp]
    L.acmmp_fusion_voxel_table.argtypes = [vp, C.c_int64, vp, vp, vp, vp]
    L.acmmp_fusion_set_scene.argtypes = [vp, C.c_int64, vp, vp, vp, vp]
    L.acmmp_fusion_voxel_clean.argtypes = [vp, i32, i32, C.c_int64, C.c_int64, vp, vp, vp, vp, vp]
    L.acmmp_fusion_clean_points.argtypes = [vp, C.c_int64, C.c_int64, vp, vp, vp]
    L.acmmp_fusion_voxel_labels.argtypes = [vp, C.c_int64, C.c_int64, vp, vp]
    L.acmmp_fusion_component_table.argtypes = [vp, C.c_int64, C.c_int64, vp, vp, vp]
    L.acmmp_fusion_voxel_visibility.argtypes = [vp, i32, i32, vp, C.c_float, i32, i32, i32, vp, vp, vp, vp]
    L.acmmp_fusion_visible_points.argtypes = [vp, C.c_int64, C.c_int64, vp, vp, vp]
    L.acmmp_fusion_visibility_tallies.argtypes = [vp, C.c_int64, C.c_int64, vp]
    L.acmmp_fusion_voxel_mesh.argtypes = [vp, i32, i32, vp, C.c_float, i32, vp, vp, vp, vp, vp, vp]
    L.acmmp_fusion_mesh_vertices.argtypes = [vp, C.c_int64, C.c_int64, vp]
    L.acmmp_fusion_mesh_faces.argtypes = [vp, C.c_int64, C.c_int64, vp]
    L.acmmp_fusion_mesh_samples.argtypes = [vp, C.c_int64, C.c_int64, vp, vp, vp]
    L.acmmp_fusion_mesh_table.argtypes = [vp, C.c_int64, vp, vp, vp, vp]
    L.acmmp_fusion_set_mesh.argtypes = [vp, C.c_int64, vp, C.c_int64, vp]
    L.acmmp_fusion_mesh_render.argtypes = [vp, i32, vp, C.c_float, vp, vp]
    L.acmmp_fusion_render_maps.argtypes = [vp, vp, vp, vp, vp]
    L.acmmp_fusion_render_plan.argtypes = [vp, i32, vp, vp, vp]
    L.acmmp_fusion_set_reference_cloud.argtypes = [vp, C.c_int64, vp]
    L.acmmp_fusion_cloud_distance.argtypes = [vp, i32, i32, C.c_float, i32, vp, vp]
    L.acmmp_fusion_distance_results.argtypes = [vp, C.c_int64, C.c_int64, vp, vp]
    L.acmmp_fusion_distance_grid.argtypes = [vp, C.c_float, vp, vp, vp, vp]
    L.acmmp_fusion_surface_distance.argtypes = [vp, i32, C.c_float, i32, vp, vp]
    L.acmmp_fusion_surface_results.argtypes = [vp, C.c_int64, C.c_int64, vp, vp]
    L.acmmp_fusion_surface_plan.argtypes = [vp, i32, vp, vp, vp, vp]
    L.acmmp_fusion_surface_grid.argtypes = [vp, C.c_float, vp, vp, vp, vp]
    L.acmmp_fusion_mesh_sample.argtypes = [vp, C.c_float, C.c_uint64, vp, vp]
    L.acmmp_fusion_sample_points.argtypes = [vp, C.c_int64, C.c_int64, vp, vp]
    L.acmmp_fusion_set_cloud_transform.argtypes = [vp, vp]
    L.acmmp_fusion_get_cloud_transform.argtypes = [vp, vp, vp]
    L.acmmp_fusion_cloud_align.argtypes = [vp, i32, i32, C.c_float, i32, i32, C.c_double, vp, vp, vp, vp]
    L.acmmp_fusion_align_records.argtypes = [vp, C.c_int64, C.c_int64, vp, vp, vp]
    L.acmmp_fusion_cloud_align_plane.argtypes = [vp, i32, C.c_float, i32, i32, C.c_double, vp, vp, vp, vp]
    L.acmmp_fusion_align_plane_records.argtypes = [vp, C.c_int64, C.c_int64, vp, vp, vp]
    L.acmmp_fusion_set_region.argtypes = [vp, i32, vp, i32]
    L.acmmp_fusion_get_region.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.acmmp_fusion_region_classify.argtypes = [vp, i32, vp]
    L.acmmp_fusion_region_classes.argtypes = [vp, C.c_int64, C.c_int64, vp]
    L.acmmp_planar_prior_host.argtypes = [vp, vp, vp, i32, i32, C.c_float, C.c_float, vp, vp, vp]
    L.acmmp_set_planar_prior_from_maps.argtypes = [vp, vp, vp, C.c_float, C.c_float, vp]
    L.acmmp_set_planar_prior_from_state.argtypes = [vp, C.c_float, C.c_float, vp]
    L.acmmp_download_planar_prior.argtypes = [vp, vp, vp]
    L.acmmp_image_cache_create.argtypes = [i32, C.c_size_t, C.POINTER(vp)]
    L.acmmp_image_cache_destroy.argtypes = [vp]
    L.acmmp_image_cache_stats.argtypes = [vp, vp]
    L.acmmp_upload_views_keyed.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32]
    L.acmmp_device_checksum.argtypes = [i32, vp, C.c_size_t, vp]
    L.acmmp_device_identity.argtypes = [i32, vp, i32, vp]
    L.acmmp_clock_probe.argtypes = [i32, C.c_float, vp]
    for name in EXPORTS:
        fn = getattr(L, name)
        if name not in ("acmmp_destroy", "acmmp_status_str", "acmmp_last_error", "acmmp_abi_version", "acmmp_device_count",
                        "acmmp_depth_from_plane_param", "acmmp_comm_destroy", "acmmp_fusion_last_error",
                        "acmmp_fusion_destroy", "acmmp_image_cache_destroy"):
            fn.restype = i32
    L.acmmp_depth_from_plane_param.restype = C.c_float
    L.acmmp_fusion_last_error.restype = C.c_char_p
    L.acmmp_image_cache_destroy.restype = None
    _lib = L
    return L


def device_count() -> int:
    """Visible HIP devices (the engine's runtime; 0 without a GPU)."""
    return int(load_library().acmmp_device_count())


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def checksum_host(arr) -> int:
    """acmmp_device_checksum on a host array (its bytes as little-endian 32-bit words): the sum mod 2^64 of
    splitmix64's finaliser of (i << 32) | w_i.  The CPU side of the exchange check and its tests."""
    w = np.frombuffer(np.ascontiguousarray(arr).tobytes(), np.uint32).astype(np.uint64)
    z = (np.arange(w.size, dtype=np.uint64) << np.uint64(32)) | w
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        z = z ^ (z >> np.uint64(31))
        return int(np.sum(z, dtype=np.uint64))


def device_identity(device: int) -> dict:
    """PCI bus id, UUID and (where the KFD topology lists the device) its KFD unique_id: which physical GPU a
    measurement ran on (bench.py `device`)."""
    L = load_library()
    bus = C.create_string_buffer(64)
    uuid = np.zeros(16, np.uint8)
    _host_check(L.acmmp_device_identity(device, C.cast(bus, C.c_void_p), 64, _p(uuid)), "device_identity")
    pci = bus.value.decode()
    out = {"pci_bus_id": pci, "uuid": uuid.tobytes().hex(), "kfd_unique_id": None}
    try:                                        # KFD node whose location_id is this bus:device.function
        dom, bus_, devfn = pci.split(":")
        dev_, fn = devfn.split(".")
        loc = (int(bus_, 16) << 8) | (int(dev_, 16) << 3) | int(fn, 16)
        root = "/sys/class/kfd/kfd/topology/nodes"
        for node in sorted(os.listdir(root)):
            with open(os.path.join(root, node, "properties")) as fh:
                props = dict(ln.split(None, 1) for ln in fh if len(ln.split(None, 1)) == 2)
            if (int(props.get("location_id", "-1")) == loc and
                    int(props.get("domain", "0")) == int(dom, 16)):
                out["kfd_unique_id"] = props.get("unique_id", "").strip() or None
                out["kfd_node"] = int(node)
                break
    except (OSError, ValueError):
        pass
    return out


def clock_probe(device: int, warm_ms: float = 1500.0) -> dict:
    """acmmp_clock_probe: the shader clock held under a VALU-dense load (median / min / max GHz over
    workgroups) after warm_ms of back-to-back launches."""
    out = np.zeros(4, np.float64)
    _host_check(load_library().acmmp_clock_probe(device, float(warm_ms), _p(out)), "clock_probe")
    return {"ghz": round(float(out[0]), 4), "ghz_min": round(float(out[1]), 4), "ghz_max": round(float(out[2]), 4),
            "probe_launch_ms": round(float(out[3]), 3), "warm_ms": warm_ms}


class ImageCache:
    """Prepared source images (padded fp32 + binary16) shared by the contexts of one GPU, keyed by the
    caller (acmmp_image_cache_*).  Safe to close before the contexts that used it."""

    def __init__(self, device: int = 0, budget_bytes: int = 0):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.acmmp_image_cache_create(device, C.c_size_t(budget_bytes), C.byref(h))
        if rc != 0:
            raise AcmmpError(f"acmmp_image_cache_create: {self.L.acmmp_status_str(rc).decode()}")
        self.h, self.device = h, device

    def stats(self) -> dict:
        out = np.zeros(5, np.uint64)
        _host_check(self.L.acmmp_image_cache_stats(self.h, _p(out)), "image_cache_stats")
        return dict(zip(("hits", "misses", "bytes", "entries", "evictions"), (int(x) for x in out)))

    def close(self):
        if self.h:
            self.L.acmmp_image_cache_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:                                            # noqa: BLE001
            pass


class Context:
    """One reference-view problem on one GPU -- the device side of the reference's ACMMP object."""

    def __init__(self, device: int = 0):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.acmmp_create(device, C.byref(h))
        if rc != 0:
            raise AcmmpError(f"acmmp_create({device}) failed: {STATUS.get(rc, rc)}")
        self.h = h
        self.device = device
        self.W = self.H = self.N = 0
        self._params = None

    def _check(self, rc, what):
        if rc != 0:
            msg = self.L.acmmp_last_error(self.h).decode()
            raise AcmmpError(f"{what}: {STATUS.get(rc, rc)}: {msg}")

    def close(self):
        if getattr(self, "h", None):
            self.L.acmmp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- setup
    MATH = {"exact": 0, "fast": 1}

    def set_math(self, mode: str):
        """'exact' (bit-identical to the oracle, the default) or 'fast' (DESIGN.md §2.4)."""
        self._check(self.L.acmmp_set_math(self.h, self.MATH[mode]), "set_math")

    def math(self) -> str:
        return {0: "exact", 1: "fast"}[int(self.L.acmmp_get_math(self.h))]

    def set_params(self, params):
        p = np.frombuffer(np.asarray(params, dtype=PARAMS_DTYPE).tobytes(), np.uint8).copy()
        self._params = p
        self._check(self.L.acmmp_set_params(self.h, _p(p)), "set_params")

    @staticmethod
    def _check_view_shapes(shapes, cams):
        """The C side sizes every copy from the cameras: a mismatched array would be read past its end."""
        if len(shapes) != len(cams):
            raise ValueError(f"{len(shapes)} images for {len(cams)} cameras")
        for i, (shp, cam) in enumerate(zip(shapes, cams)):
            if tuple(shp) != (int(cam["height"]), int(cam["width"])):
                raise ValueError(f"image {i} has shape {tuple(shp)}, camera says {int(cam['height'])}x{int(cam['width'])}")

    def _check_hw(self, arr, tail, what):
        """Row-major (H, W)+tail maps, or the same elements flat: any other shape (a transposed
        (W, H) map with the right element count included) is refused, not read in the wrong layout."""
        want = (self.H, self.W) + tail
        if arr.shape != want and arr.shape != (int(np.prod(want)),):
            raise ValueError(f"{what}: shape {arr.shape}, expected {want} (or flat {int(np.prod(want))})")

    def upload_views(self, images, cameras):
        imgs = [np.ascontiguousarray(im, np.float32) for im in images]
        cams = np.frombuffer(np.ascontiguousarray(cameras, dtype=CAMERA_DTYPE).tobytes(), CAMERA_DTYPE).copy()
        self._check_view_shapes([im.shape for im in imgs], cams)
        n = len(imgs)
        ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
        self._check(self.L.acmmp_upload_views(self.h, n, C.cast(ptrs, C.c_void_p), None, _p(cams)), "upload_views")
        self.N, self.H, self.W = n, imgs[0].shape[0], imgs[0].shape[1]

    def upload_views_device(self, bufs, cameras, cache: "ImageCache | None" = None, keys=None):
        """bufs: DeviceBuffer images (index 0 = reference) on this context's GPU.  With an ImageCache and
        one nonzero content key per view (the caller's promise that equal keys mean equal pixels), views
        the cache already holds are neither copied nor converted again (acmmp_upload_views_keyed)."""
        cams = np.frombuffer(np.ascontiguousarray(cameras, dtype=CAMERA_DTYPE).tobytes(), CAMERA_DTYPE).copy()
        self._check_view_shapes([tuple(b.shape[:2]) for b in bufs], cams)
        n = len(bufs)
        ptrs = (C.c_void_p * n)(*[b.ptr for b in bufs])
        if cache is not None:
            k = np.ascontiguousarray(keys, np.uint64)
            if k.shape != (n,):
                raise ValueError(f"upload_views_device: {n} views but keys of shape {k.shape}")
            self._check(self.L.acmmp_upload_views_keyed(self.h, cache.h, n, _p(k), C.cast(ptrs, C.c_void_p), None,
                                                        _p(cams), 1), "upload_views_keyed")
        else:
            self._check(self.L.acmmp_upload_views_device(self.h, n, C.cast(ptrs, C.c_void_p), None, _p(cams)),
                        "upload_views_device")
        self.N, self.H, self.W = n, bufs[0].shape[0], bufs[0].shape[1]

    def upload_depths(self, depths):
        ds = [np.ascontiguousarray(d, np.float32) for d in depths]
        n = len(ds)
        ptrs = (C.c_void_p * n)(*[d.ctypes.data for d in ds])
        w = np.array([d.shape[1] for d in ds], np.int32)
        h = np.array([d.shape[0] for d in ds], np.int32)
        self._check(self.L.acmmp_upload_depths(self.h, n, C.cast(ptrs, C.c_void_p), _p(w), _p(h)), "upload_depths")

    def upload_depths_device(self, bufs):
        """bufs: DeviceBuffer depth maps (index 0 = reference) on this context's GPU."""
        n = len(bufs)
        ptrs = (C.c_void_p * n)(*[b.ptr for b in bufs])
        w = np.array([b.shape[1] for b in bufs], np.int32)
        h = np.array([b.shape[0] for b in bufs], np.int32)
        self._check(self.L.acmmp_upload_depths_device(self.h, n, C.cast(ptrs, C.c_void_p), _p(w), _p(h)),
                    "upload_depths_device")

    def export_depth(self, buf):
        """Copy the last run's depth map into DeviceBuffer `buf` (H x W floats)."""
        self._check(self.L.acmmp_export_depth(self.h, C.c_void_p(buf.ptr)), "export_depth")

    def set_state(self, planes=None, costs=None):
        pl = None if planes is None else np.ascontiguousarray(planes, np.float32)
        co = None if costs is None else np.ascontiguousarray(costs, np.float32)
        if pl is not None:
            self._check_hw(pl, (4,), "set_state planes")
        if co is not None:
            self._check_hw(co, (), "set_state costs")
        self._check(self.L.acmmp_set_state(self.h, _p(pl), _p(co)), "set_state")

    def _check_state_bufs(self, planes_buf, costs_buf, what):
        # (H, W, 4) / (H, W) buffers, or larger flat ones (a view's buffers sized for its finest scale)
        for b, k, name in ((planes_buf, 4, "planes"), (costs_buf, 1, "costs")):
            if b is None:
                continue
            need = 4 * k * self.H * self.W
            if b.shape != ((self.H, self.W, 4) if k == 4 else (self.H, self.W)) and (len(b.shape) != 1 or b.nbytes < need):
                raise ValueError(f"{what} {name}: buffer shape {b.shape}, expected {(self.H, self.W)}"
                                 f"{' + (4,)' if k == 4 else ''} or a flat buffer of at least {need} bytes")

    def export_state(self, planes_buf=None, costs_buf=None):
        """Copy the last run's planes into DeviceBuffer `planes_buf` (H x W x 4) and its costs into
        `costs_buf` (H x W), HBM to HBM."""
        self._check_state_bufs(planes_buf, costs_buf, "export_state")
        self._check(self.L.acmmp_export_state(self.h, C.c_void_p(planes_buf.ptr if planes_buf else None),
                                              C.c_void_p(costs_buf.ptr if costs_buf else None)), "export_state")

    def set_state_device(self, planes_buf=None, costs_buf=None):
        """set_state from DeviceBuffers of this context's GPU (shapes as export_state)."""
        self._check_state_bufs(planes_buf, costs_buf, "set_state_device")
        self._check(self.L.acmmp_set_state_device(self.h, C.c_void_p(planes_buf.ptr if planes_buf else None),
                                                  C.c_void_p(costs_buf.ptr if costs_buf else None)), "set_state_device")

    def set_scaled_state(self, planes):
        pl = np.ascontiguousarray(planes, np.float32)
        self._check(self.L.acmmp_set_scaled_state(self.h, _p(pl), pl.shape[1], pl.shape[0]), "set_scaled_state")

    def set_planar_prior(self, prior_planes, masks):
        pr = np.ascontiguousarray(prior_planes, np.float32)
        mk = np.ascontiguousarray(masks, np.uint32)
        self._check_hw(pr, (4,), "set_planar_prior planes")
        self._check_hw(mk, (), "set_planar_prior masks")
        self._check(self.L.acmmp_set_planar_prior(self.h, _p(pr), _p(mk)), "set_planar_prior")

    def set_planar_prior_from_maps(self, depths, costs, depth_min: float, depth_max: float) -> int:
        """The planar block of ProcessProblem with its per-pixel work on the device (main.cpp:113-181):
        the same prior as planar_prior_host + set_planar_prior.  Returns the triangle count."""
        d = np.ascontiguousarray(depths, np.float32)
        c = np.ascontiguousarray(costs, np.float32)
        self._check_hw(d, (), "set_planar_prior_from_maps depths")
        self._check_hw(c, (), "set_planar_prior_from_maps costs")
        n = C.c_int(0)
        self._check(self.L.acmmp_set_planar_prior_from_maps(self.h, _p(d), _p(c), float(depth_min), float(depth_max),
                                                            C.byref(n)), "set_planar_prior_from_maps")
        return n.value

    def set_planar_prior_from_state(self, depth_min: float, depth_max: float) -> int:
        """The planar block from this context's last RunPatchMatch output in HBM (support points on the
        device, Delaunay and the planes on the host, raster + mask on the device): equal to
        set_planar_prior_from_maps on the downloaded maps, without downloading them.  Returns the
        triangle count."""
        n = C.c_int(0)
        self._check(self.L.acmmp_set_planar_prior_from_state(self.h, float(depth_min), float(depth_max), C.byref(n)),
                    "set_planar_prior_from_state")
        return n.value

    def download_planar_prior(self):
        prior = host_empty((self.H, self.W, 4), np.float32)
        masks = host_empty((self.H, self.W), np.uint32)
        self._check(self.L.acmmp_download_planar_prior(self.h, _p(prior), _p(masks)), "download_planar_prior")
        return prior, masks

    # -- run
    def run_patchmatch(self, seed: int, n_half_sweeps: int = -1, do_post: bool = True):
        self._check(self.L.acmmp_run_patchmatch_ex(self.h, C.c_uint64(seed), n_half_sweeps, int(do_post)),
                    "run_patchmatch")

    def download(self):
        planes = host_empty((self.H, self.W, 4), np.float32)
        costs = host_empty((self.H, self.W), np.float32)
        self._check(self.L.acmmp_download(self.h, _p(planes), _p(costs)), "download")
        return planes, costs

    def download_into(self, planes, costs):
        """D2H into caller-owned C-contiguous float32 arrays (H, W, 4) and (H, W)."""
        for a, tail in ((planes, (4,)), (costs, ())):
            if a.dtype != np.float32 or not a.flags.c_contiguous or a.shape != (self.H, self.W) + tail:
                raise ValueError("download_into: need C-contiguous float32 (H, W, 4) planes and (H, W) costs")
        self._check(self.L.acmmp_download(self.h, _p(planes), _p(costs)), "download")

    def download_rows_into(self, planes, costs, row0: int, row1: int):
        """D2H of rows [row0, row1) of the row-major outputs into caller-owned C-contiguous float32 arrays
        (row1 - row0, W, 4) and (row1 - row0, W) -- a band's share of a split run (acmmp_band_*)."""
        n = row1 - row0
        for a, tail in ((planes, (4,)), (costs, ())):
            if a.dtype != np.float32 or not a.flags.c_contiguous or a.shape != (n, self.W) + tail:
                raise ValueError("download_rows_into: need C-contiguous float32 (rows, W, 4) and (rows, W)")
        if not (0 <= row0 < row1 <= self.H):
            raise ValueError("download_rows_into: rows outside the view")
        pp, cp = self.device_outputs()
        dev = self.device
        _host_check(self.L.acmmp_memcpy(dev, _p(planes), C.c_void_p(pp + 16 * row0 * self.W), 16 * n * self.W, 1),
                    "memcpy D2H")
        _host_check(self.L.acmmp_memcpy(dev, _p(costs), C.c_void_p(cp + 4 * row0 * self.W), 4 * n * self.W, 1),
                    "memcpy D2H")

    def download_aux(self):
        sel = host_empty((self.H, self.W), np.uint32)
        pre = host_empty((self.H, self.W), np.float32)
        self._check(self.L.acmmp_download_aux(self.h, _p(sel), _p(pre)), "download_aux")
        return sel, pre

    def device_outputs(self):
        a, b = C.c_void_p(), C.c_void_p()
        self._check(self.L.acmmp_device_outputs(self.h, C.byref(a), C.byref(b)), "device_outputs")
        return a.value, b.value

    # ---- row-band split of one view (acmmp_band_*, SURVEY.md §8e latency mode) ----
    BAND_HALO = 23

    def band_begin(self, seed: int, row0: int, row1: int):
        self._check(self.L.acmmp_band_begin(self.h, seed, row0, row1), "band_begin")

    def band_sweep(self) -> int:
        colour = C.c_int32(0)
        self._check(self.L.acmmp_band_sweep(self.h, C.byref(colour)), "band_sweep")
        return colour.value

    def band_sweeps_left(self) -> int:
        return int(self.L.acmmp_band_sweeps_left(self.h))

    def band_halo_ranges(self):
        """((send_up), (recv_up), (send_down), (recv_down)) row ranges [a, b) after a half-sweep."""
        r = np.zeros(8, np.int32)
        self._check(self.L.acmmp_band_halo_ranges(self.h, _p(r)), "band_halo_ranges")
        return tuple((int(r[2 * k]), int(r[2 * k + 1])) for k in range(4))

    def band_copy_rows_from(self, src: "Context", colour: int, row_a: int, row_b: int):
        self._check(self.L.acmmp_band_copy_rows(self.h, src.h, colour, row_a, row_b), "band_copy_rows")

    def band_get_rows(self, colour: int, row_a: int, row_b: int) -> np.ndarray:
        """Rows [row_a, row_b) of `colour`'s current band state as one host array of 6 words per colour-grid pixel
        (plane x, y, z, w, cost as float32 bits, selected-view mask) -- the host transport of the halo."""
        n = (row_b - row_a) * ((self.W + 1) // 2)
        pl = np.empty((n, 4), np.float32)
        co = np.empty(n, np.float32)
        sel = np.empty(n, np.uint32)
        self._check(self.L.acmmp_band_get_rows(self.h, colour, row_a, row_b, _p(pl), _p(co), _p(sel)), "band_get_rows")
        return np.concatenate([pl.view(np.uint32), co.view(np.uint32)[:, None], sel[:, None]], axis=1)

    def debug_band_cvec(self, colour: int, row_a: int, row_b: int) -> np.ndarray:
        """The cached NCC cost vectors of rows [row_a, row_b) of `colour` in a band run -> (V, n) float32, n the rows'
        colour-grid pixels in band_get_rows' order; straight after band_begin, k_init's vectors of its planes."""
        out = np.empty((self.N - 1, (row_b - row_a) * ((self.W + 1) // 2)), np.float32)
        self._check(self.L.acmmp_debug_band_cvec(self.h, colour, row_a, row_b, _p(out)), "debug_band_cvec")
        return out

    def debug_band_keep_mask(self, colour: int, row_a: int, row_b: int) -> np.ndarray:
        """The kept-sample mask words of rows [row_a, row_b) of `colour` in a band run -> (n,) uint64 in
        band_get_rows' order (bit s set: sample s dropped); AcmmpError when the run publishes no mask."""
        out = np.empty((row_b - row_a) * ((self.W + 1) // 2), np.uint64)
        self._check(self.L.acmmp_debug_band_keep_mask(self.h, colour, row_a, row_b, _p(out)), "debug_band_keep_mask")
        return out

    def band_set_rows(self, colour: int, row_a: int, row_b: int, rows: np.ndarray):
        """Inverse of band_get_rows: write the (n, 6) words into `colour`'s current band state."""
        rows = np.asarray(rows, np.uint32).reshape(-1, 6)
        pl = np.ascontiguousarray(rows[:, :4]).view(np.float32)
        co = np.ascontiguousarray(rows[:, 4]).view(np.float32)
        sel = np.ascontiguousarray(rows[:, 5])
        self._check(self.L.acmmp_band_set_rows(self.h, colour, row_a, row_b, _p(pl), _p(co), _p(sel)), "band_set_rows")

    def band_end(self, do_post: bool = True):
        self._check(self.L.acmmp_band_end(self.h, int(do_post)), "band_end")

    def run_patchmatch_band(self, seed: int, row0: int, row1: int, comm=None, rank_up: int = -1,
                            rank_down: int = -1):
        """One band of a view split over ranks, halo exchange over RCCL (comm: a Comm, or None for a
        band covering the whole view)."""
        self._check(self.L.acmmp_run_patchmatch_band(self.h, comm.h if comm is not None else None, seed, row0, row1,
                                                     rank_up, rank_down), "run_patchmatch_band")

    def synchronize(self):
        self._check(self.L.acmmp_synchronize(self.h), "synchronize")

    def last_timing(self):
        ms = np.zeros(3, np.float32)
        self._check(self.L.acmmp_last_timing(self.h, _p(ms)), "last_timing")
        return {"init_ms": float(ms[0]), "prop_ms": float(ms[1]), "post_ms": float(ms[2])}

    KERNELS = ("k_eval_nb", "k_select", "k_eval_ref", "k_finish")

    def last_kernel_timing(self):
        """{kernel: (summed ms, launches)} for the half-sweep kernels of the last run."""
        ms = np.zeros(4, np.float32)
        n = np.zeros(4, np.int32)
        self._check(self.L.acmmp_last_kernel_timing(self.h, _p(ms), _p(n)), "last_kernel_timing")
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(self.KERNELS)}

    def last_work(self):
        """(pixels of the last run's k_eval_nb launches whose NCCs were evaluated, all pixels)."""
        e, t = C.c_ulonglong(0), C.c_ulonglong(0)
        self._check(self.L.acmmp_last_work(self.h, C.byref(e), C.byref(t)), "last_work")
        return e.value, t.value

    def last_planar_timing(self):
        """Host wall ms of the last set_planar_prior_from_state / _from_maps: support points, Delaunay, the rest of
        the host half (triangles, plane fits, tables), device half (staging + enqueueing upload, raster, mask)."""
        ms = np.zeros(4, np.float32)
        self._check(self.L.acmmp_last_planar_timing(self.h, _p(ms)), "last_planar_timing")
        return {"support_ms": float(ms[0]), "delaunay_ms": float(ms[1]), "planes_ms": float(ms[2]),
                "device_ms": float(ms[3])}

    def texel_bytes(self) -> int:
        """Bytes per source texel the NCC fetches read (2: binary16 copy, 4: fp32, 0: no views)."""
        return int(self.L.acmmp_texel_bytes(self.h))

    def jbu(self, ref, coarse, imagescale: int):
        ref = np.ascontiguousarray(ref, np.float32)
        coarse = np.ascontiguousarray(coarse, np.float32)
        out = np.empty_like(ref)
        self._check(self.L.acmmp_jbu(self.h, _p(ref), ref.shape[1], ref.shape[0], _p(coarse), coarse.shape[1],
                                     coarse.shape[0], imagescale, _p(out)), "jbu")
        return out

    def _debug(self, fn, px, py, planes):
        px = np.ascontiguousarray(px, np.int32)
        py = np.ascontiguousarray(py, np.int32)
        pl = np.ascontiguousarray(planes, np.float32).reshape(-1, 4)
        out = np.empty((len(px), self.N - 1), np.float32)
        self._check(fn(self.h, len(px), _p(px), _p(py), _p(pl), _p(out)), "debug")
        return out

    def debug_ncc(self, px, py, planes):
        return self._debug(self.L.acmmp_debug_ncc, px, py, planes)

    def debug_geom(self, px, py, planes):
        return self._debug(self.L.acmmp_debug_geom, px, py, planes)

    def _debug_k(self, fn, k, px, py, planes, what):
        px = np.ascontiguousarray(px, np.int32)
        py = np.ascontiguousarray(py, np.int32)
        pl = np.ascontiguousarray(planes, np.float32).reshape(len(px), k, 4)
        out = np.empty((len(px), k, self.N - 1), np.float32)
        self._check(fn(self.h, len(px), _p(px), _p(py), _p(pl), _p(out)), what)
        return out

    def debug_ncc_nb(self, px, py, planes):
        """k_eval_nb's own NCC (fast SPHERE from 2000x1000 up with patch_size 11: interpolated coordinates with
        their deferred per-sample fallbacks) of planes (n, 8, 4) at pixels (px, py) -> costs (n, 8, V)."""
        return self._debug_k(self.L.acmmp_debug_ncc_nb, 8, px, py, planes, "debug_ncc_nb")

    def debug_ncc_ref(self, px, py, planes):
        """The refinement's NCC (k_eval_ref's instance; fast SPHERE with V > 4 at the interpolation's sizes:
        interpolated coordinates; where they fall back, the per-sample costs of k_nb_fix<1, true>'s entry code,
        the production fallback path) of planes (n, 5, 4) at pixels (px, py) -> costs (n, 5, V)."""
        return self._debug_k(self.L.acmmp_debug_ncc_ref, 5, px, py, planes, "debug_ncc_ref")


# ---- planar-prior host side (no GPU): ACMMP.cpp:904-1011, main.cpp:113-181 ------------------

def _host_check(rc, what):
    if rc != 0:
        raise AcmmpError(f"{what}: {load_library().acmmp_status_str(rc).decode()}")


def _cam_ptr(cam):
    cam = np.frombuffer(np.asarray(cam).tobytes(), dtype=CAMERA_DTYPE).copy()
    return cam, cam.ctypes.data


def support_points(costs) -> np.ndarray:
    """GetSupportPoints (ACMMP.cpp:904-930) -> (n, 2) int32 (x, y) in the reference's order."""
    L = load_library()
    costs = np.ascontiguousarray(costs, np.float32)
    H, W = costs.shape
    n = C.c_int(0)
    L.acmmp_support_points(_p(costs), W, H, None, 0, C.byref(n))
    xy = np.zeros((max(n.value, 1), 2), np.int32)
    _host_check(L.acmmp_support_points(_p(costs), W, H, _p(xy), n.value, C.byref(n)), "support_points")
    return xy[:n.value]


def delaunay(xy, W: int, H: int) -> np.ndarray:
    """DelaunayTriangulation (ACMMP.cpp:932-955) -> (m, 3, 2) int32 triangle vertices."""
    L = load_library()
    xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
    m = C.c_int(0)
    L.acmmp_delaunay(_p(xy), xy.shape[0], W, H, None, 0, C.byref(m))
    tri = np.zeros((max(m.value, 1), 3, 2), np.int32)
    _host_check(L.acmmp_delaunay(_p(xy), xy.shape[0], W, H, _p(tri), m.value, C.byref(m)), "delaunay")
    return tri[:m.value]


def prior_plane_params(cam0, depths, tri) -> np.ndarray:
    """GetPriorPlaneParams (ACMMP.cpp:957-989) for one triangle ((3, 2) ints)."""
    L = load_library()
    depths = np.ascontiguousarray(depths, np.float32)
    H, W = depths.shape
    tri = np.ascontiguousarray(tri, np.int32).reshape(6)
    out = np.zeros(4, np.float32)
    cam, cp = _cam_ptr(cam0)
    _host_check(L.acmmp_prior_plane_params(cp, _p(depths), W, H, _p(tri), _p(out)), "prior_plane_params")
    return out


def depth_from_plane_param(cam0, plane, x: int, y: int) -> float:
    """GetDepthFromPlaneParam (ACMMP.cpp:991-1011)."""
    plane = np.ascontiguousarray(plane, np.float32)
    cam, cp = _cam_ptr(cam0)
    return float(load_library().acmmp_depth_from_plane_param(cp, _p(plane), int(x), int(y)))


def planar_prior_host(cam0, depths, costs, depth_min: float, depth_max: float):
    """main.cpp:113-181 + ACMMP.cpp:851-861 -> (prior_planes (H, W, 4), masks (H, W) uint32, n_triangles)."""
    L = load_library()
    depths = np.ascontiguousarray(depths, np.float32)
    costs = np.ascontiguousarray(costs, np.float32)
    H, W = depths.shape
    prior = np.zeros((H, W, 4), np.float32)
    masks = np.zeros((H, W), np.uint32)
    n = C.c_int(0)
    cam, cp = _cam_ptr(cam0)
    _host_check(L.acmmp_planar_prior_host(cp, _p(depths), _p(costs), W, H, float(depth_min), float(depth_max),
                                          _p(prior), _p(masks), C.byref(n)), "planar_prior_host")
    return prior, masks, n.value


# ---- device buffers + RCCL communicator (multi-GPU pipeline) ---------------------

class DeviceBuffer:
    """A float32 (H, W) buffer in HBM of one GPU (pipeline depth store)."""

    def __init__(self, device: int, shape):
        self.L = load_library()
        self.device, self.shape = device, tuple(int(v) for v in shape)
        self.nbytes = 4 * int(np.prod(self.shape))
        p = C.c_void_p()
        _host_check(self.L.acmmp_device_alloc(device, self.nbytes, C.byref(p)), "device_alloc")
        self.ptr = p.value

    def upload(self, arr):
        a = np.ascontiguousarray(arr, np.float32)
        assert a.shape == self.shape
        _host_check(self.L.acmmp_memcpy(self.device, C.c_void_p(self.ptr), _p(a), self.nbytes, 0), "memcpy H2D")

    def download(self):
        a = host_empty(self.shape, np.float32)
        _host_check(self.L.acmmp_memcpy(self.device, _p(a), C.c_void_p(self.ptr), self.nbytes, 1), "memcpy D2H")
        return a

    def checksum(self) -> int:
        """acmmp_device_checksum of the buffer (equal to checksum_host of its download)."""
        out = C.c_uint64(0)
        _host_check(self.L.acmmp_device_checksum(self.device, C.c_void_p(self.ptr), self.nbytes, C.byref(out)),
                    "device_checksum")
        return int(out.value)

    def free(self):
        if self.ptr:
            self.L.acmmp_device_free(self.device, C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Comm:
    """RCCL communicator of this process's GPU (one rank per process)."""

    ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * Comm.ID_BYTES)()
        _host_check(load_library().acmmp_comm_unique_id(C.cast(buf, C.c_void_p)), "comm_unique_id")
        return bytes(buf)

    def __init__(self, device: int, uid: bytes, nranks: int, rank: int):
        self.L = load_library()
        assert len(uid) == self.ID_BYTES
        buf = (C.c_uint8 * self.ID_BYTES).from_buffer_copy(uid)
        h = C.c_void_p()
        _host_check(self.L.acmmp_comm_create(device, C.cast(buf, C.c_void_p), nranks, rank, C.byref(h)),
                    "comm_create")
        self.h, self.nranks, self.rank = h, nranks, rank

    def broadcast(self, bufs, roots):
        """In-place grouped broadcast of DeviceBuffers, bufs[i] from rank roots[i]."""
        n = len(bufs)
        ptrs = (C.c_void_p * n)(*[b.ptr for b in bufs])
        nb = np.array([b.nbytes for b in bufs], np.uint64)
        rt = np.array(roots, np.int32)
        _host_check(self.L.acmmp_comm_broadcast(self.h, n, C.cast(ptrs, C.c_void_p), _p(nb), _p(rt)), "broadcast")

    def after(self, ctx: "Context"):
        """Collectives queued from now on start after the work `ctx` has queued so far (device-side order)."""
        _host_check(self.L.acmmp_comm_after(self.h, ctx.h), "comm_after")

    def band_exchange(self, ctx: "Context", colour: int, rank_up: int, rank_down: int):
        _host_check(self.L.acmmp_comm_band_exchange(self.h, ctx.h, colour, rank_up, rank_down), "band_exchange")

    def allreduce_max(self, vals):
        v = np.ascontiguousarray(vals, np.float64).copy()
        _host_check(self.L.acmmp_comm_allreduce_max(self.h, _p(v), v.size), "allreduce_max")
        return v

    def close(self):
        if self.h:
            self.L.acmmp_comm_destroy(self.h)
            self.h = None


# ---- GPU fusion (RunFusionCuda / SimpleFusionKernel, ACMMP.cu:1662-2105) ---------------------------

FUSE_UNIQUE = 1     # ACMMP_FUSE_UNIQUE
VIS_SOURCES = {"voxel": 0, "clean": 1}     # ACMMP_VIS_FROM_VOXELS, ACMMP_VIS_FROM_CLEAN
MESH_SOURCES = {"voxel": 0, "clean": 1, "visible": 2}     # ACMMP_MESH_FROM_VOXELS, _CLEAN, _VISIBLE
RENDER_COUNTS = ("agree", "mesh_in_front", "mesh_behind", "mesh_only", "raw_only", "neither", "back_facing")
DIST_SOURCES = {"scene": 0, "voxels": 1, "clean": 2, "visible": 3, "mesh": 4, "samples": 6}     # ACMMP_DIST_FROM_*
DIST_DIRECTIONS = {"data_to_ref": 0, "ref_to_data": 1}     # ACMMP_DIST_DATA_TO_REF (accuracy), _REF_TO_DATA (completeness)
SURF_QUERIES = {"scene": 0, "voxels": 1, "clean": 2, "visible": 3, "reference": 5}     # ACMMP_SURF_FROM_*
DIST_SUMMARY_WORDS = 268     # ACMMP_DIST_SUMMARY_WORDS: n_query, n_valid, n_matched, sum_q, within[8], hist[256]
ALIGN_MODES = {"rigid": 0, "similarity": 1}     # ACMMP_ALIGN_RIGID, ACMMP_ALIGN_SIMILARITY
ALIGN_STOP_REASONS = ("max_iterations", "converged", "degenerate")     # ACMMP_ALIGN_MAX_ITERATIONS, _CONVERGED, _DEGENERATE
ALIGN_RECORD_WORDS = 32     # ACMMP_ALIGN_RECORD_WORDS: n_query, n_valid, n_matched, sum_q, n_out_of_range, N, the moments
REGION_SIDES = {"data": 0, "reference": 1}     # ACMMP_REGION_DATA, ACMMP_REGION_REFERENCE
REGION_QUERIES_ONLY = 1     # ACMMP_REGION_QUERIES_ONLY
REGION_SOURCES = dict(DIST_SOURCES, reference=SURF_QUERIES["reference"])     # what region_classify takes
REGION_COUNTS = ("points", "invalid", "inside", "planes", "prism", "grid")     # ACMMP_REGION_COUNT_WORDS words
REGION_CLASS_BITS = {"invalid": 1, "planes": 2, "prism": 4, "grid": 8}     # ACMMP_REGION_CLASS_*


class RegionStruct(C.Structure):
    """acmmp_region (include/acmmp.h)."""
    _fields_ = [("n_planes", C.c_int32), ("n_vertices", C.c_int32), ("axis", C.c_int32), ("dims", C.c_int32 * 3),
                ("planes", C.c_double * 32), ("axis_min", C.c_double), ("axis_max", C.c_double),
                ("origin", C.c_double * 3), ("cell", C.c_double), ("polygon", C.c_void_p), ("bits", C.c_void_p)]


def region_struct(region):
    """(RegionStruct, the arrays it points into) of an io.Region-like object: planes, axis, axis_min, axis_max, polygon,
    origin, cell, dims, bits, a part absent where its array is None.  Shapes are checked here; values by the library."""
    st, keep = RegionStruct(), []
    if region.planes is not None:
        pl = np.ascontiguousarray(region.planes, np.float64).reshape(-1, 4)
        if pl.shape[0] > 8:
            raise ValueError("at most 8 planes")
        st.n_planes = pl.shape[0]
        st.planes[:pl.size] = pl.reshape(-1).tolist()
    if region.polygon is not None:
        poly = np.ascontiguousarray(region.polygon, np.float64).reshape(-1, 2)
        if not 3 <= poly.shape[0] <= 256:
            raise ValueError("the polygon has 3 to 256 vertices")
        st.n_vertices, st.axis = poly.shape[0], int(region.axis)
        st.axis_min, st.axis_max = float(region.axis_min), float(region.axis_max)
        st.polygon = poly.ctypes.data
        keep.append(poly)
    if region.dims is not None:
        dims = [int(x) for x in region.dims]
        if len(dims) != 3 or not all(1 <= x <= 4096 for x in dims):
            raise ValueError("dims are three integers in 1 .. 4096")
        bits = np.ascontiguousarray(region.bits, np.uint8).reshape(-1)
        if bits.size != (dims[0] * dims[1] * dims[2] + 7) // 8:
            raise ValueError("bits must hold ceil(nx ny nz / 8) bytes")
        st.dims[:] = dims
        st.origin[:] = [float(x) for x in np.asarray(region.origin, np.float64).reshape(3)]
        st.cell = float(region.cell)
        st.bits = bits.ctypes.data
        keep.append(bits)
    return st, keep


@dataclasses.dataclass
class MeshSamples:
    """What Fusion.mesh_sample returns."""
    n_samples: int         # points of the sample result
    n_skipped: int         # faces with a non-finite vertex, which have no samples


@dataclasses.dataclass
class AlignRecord:
    """One iteration of Fusion.cloud_align (step 3 of acmmp_fusion_cloud_align, include/acmmp.h)."""
    words: np.ndarray      # (32,) int64, the header's layout
    M: np.ndarray          # (3, 4) float64: the transform the iteration ran under
    shift: float           # the largest displacement of a corner of the targets' box under the iteration's step
    max_dist: float

    n_query = property(lambda self: int(self.words[0]))
    n_valid = property(lambda self: int(self.words[1]))
    n_matched = property(lambda self: int(self.words[2]))
    sum_q = property(lambda self: int(self.words[3]))
    n_out_of_range = property(lambda self: int(self.words[4]))
    n_pairs = property(lambda self: int(self.words[5]))

    @property
    def mean(self) -> float:
        """Mean distance of the matched queries (0 with none)."""
        k = 1048576.0 / float(np.float32(self.max_dist))
        return self.sum_q / (self.n_matched * k) if self.n_matched else 0.0


@dataclasses.dataclass
class CloudAlignment:
    """What Fusion.cloud_align and Fusion.cloud_align_plane return."""
    M: np.ndarray          # (3, 4) float64: data -> reference
    iterations: int
    stop_reason: str       # one of ALIGN_STOP_REASONS
    records: list          # AlignRecord (AlignPlaneRecord) per iteration


ALIGN_PLANE_RECORD_WORDS = 70     # ACMMP_ALIGN_PLANE_RECORD_WORDS
# ACMMP_ALIGN_PLANE_RECORD_*: the offsets of the header's layout
(ALIGN_PLANE_N_QUERY, ALIGN_PLANE_N_VALID, ALIGN_PLANE_N_MATCHED, ALIGN_PLANE_SUM_Q, ALIGN_PLANE_N_OUT_OF_RANGE,
 ALIGN_PLANE_N_NO_NORMAL, ALIGN_PLANE_N, ALIGN_PLANE_SUM_Q3, ALIGN_PLANE_PIVOT, ALIGN_PLANE_ZERO, ALIGN_PLANE_CC,
 ALIGN_PLANE_CR, ALIGN_PLANE_RR) = 0, 1, 2, 3, 4, 5, 6, 7, 10, 13, 14, 56, 68


@dataclasses.dataclass
class AlignPlaneRecord:
    """One iteration of Fusion.cloud_align_plane (step 4 of acmmp_fusion_cloud_align_plane, include/acmmp.h)."""
    words: np.ndarray      # (70,) int64, the header's layout
    M: np.ndarray          # (3, 4) float64: the transform the iteration ran under
    shift: float           # the largest displacement of a corner of the targets' box under the iteration's step
    max_dist: float

    n_query = property(lambda self: int(self.words[ALIGN_PLANE_N_QUERY]))
    n_valid = property(lambda self: int(self.words[ALIGN_PLANE_N_VALID]))
    n_matched = property(lambda self: int(self.words[ALIGN_PLANE_N_MATCHED]))
    sum_q = property(lambda self: int(self.words[ALIGN_PLANE_SUM_Q]))
    n_out_of_range = property(lambda self: int(self.words[ALIGN_PLANE_N_OUT_OF_RANGE]))
    n_no_normal = property(lambda self: int(self.words[ALIGN_PLANE_N_NO_NORMAL]))
    n_pairs = property(lambda self: int(self.words[ALIGN_PLANE_N]))
    pivot = property(lambda self: [int(x) for x in self.words[ALIGN_PLANE_PIVOT:ALIGN_PLANE_PIVOT + 3]])

    @property
    def mean(self) -> float:
        """Mean distance of the matched queries (0 with none)."""
        k = 1048576.0 / float(np.float32(self.max_dist))
        return self.sum_q / (self.n_matched * k) if self.n_matched else 0.0

    @property
    def rms_plane(self) -> float:
        """sqrt(sum r^2 / N) / (kq * 4096): the RMS point-to-plane residual of the N pairs, in the clouds' unit."""
        rr = int(self.words[ALIGN_PLANE_RR]) * (1 << 32) + int(self.words[ALIGN_PLANE_RR + 1])
        kq = 65536.0 / float(np.float32(self.max_dist))
        return float(np.sqrt(rr / self.n_pairs)) / (kq * 4096.0) if self.n_pairs else 0.0


@dataclasses.dataclass
class CloudDistance:
    """Summary of one Fusion.cloud_distance call (step 5 of acmmp_fusion_cloud_distance, include/acmmp.h)."""
    n_query: int
    n_valid: int
    n_matched: int
    sum_q: int
    max_dist: float
    within: list           # per threshold: the matched queries no further than it
    hist: np.ndarray       # (256,) int64: the matched queries by distance, bins of max_dist / 256

    @property
    def mean(self) -> float:
        """Mean distance of the matched queries (0 with none)."""
        k = 1048576.0 / float(np.float32(self.max_dist))
        return self.sum_q / (self.n_matched * k) if self.n_matched else 0.0

    @property
    def median_upper(self) -> float:
        """Upper edge of the histogram bin that holds the median matched distance (0 with none)."""
        if not self.n_matched:
            return 0.0
        b = int(np.searchsorted(np.cumsum(self.hist), (self.n_matched + 1) // 2))
        return (b + 1) * float(np.float32(self.max_dist)) / 256.0


class Fusion:
    """Depth-map fusion on one GPU.  cams: CAMERA_DTYPE array, each rescaled to its depth map."""

    def __init__(self, device: int, cams):
        self.L = load_library()
        self.cams = np.frombuffer(np.ascontiguousarray(cams, dtype=CAMERA_DTYPE).tobytes(), CAMERA_DTYPE).copy()
        h = C.c_void_p()
        _host_check(self.L.acmmp_fusion_create(device, len(self.cams), _p(self.cams), C.byref(h)), "fusion_create")
        self.h = h

    def _check(self, rc, what):
        if rc != 0:
            msg = self.L.acmmp_fusion_last_error(self.h).decode()
            raise AcmmpError(f"{what}: {self.L.acmmp_status_str(rc).decode()} ({msg})")

    def set_view(self, view: int, depth, normals, bgr):
        d = np.ascontiguousarray(depth, np.float32)
        n = np.ascontiguousarray(normals, np.float32)
        c = np.ascontiguousarray(bgr, np.uint8)
        H, W = int(self.cams[view]["height"]), int(self.cams[view]["width"])
        assert d.shape == (H, W) and n.shape == (H, W, 3) and c.shape == (H, W, 3)
        self._check(self.L.acmmp_fusion_set_view(self.h, view, _p(d), _p(n), _p(c)), "fusion_set_view")

    def run(self, ref: int, src_views) -> np.ndarray:
        """Consistent points of reference view `ref`, (n, 9) float32 in pixel order."""
        srcs = np.ascontiguousarray(src_views, np.int32)
        n = C.c_int(0)
        self.L.acmmp_fusion_run(self.h, ref, srcs.size, _p(srcs), None, 0, C.byref(n))
        out = np.zeros((max(n.value, 1), 9), np.float32)
        self._check(self.L.acmmp_fusion_run(self.h, ref, srcs.size, _p(srcs), _p(out), n.value, C.byref(n)),
                    "fusion_run")
        return out[:n.value]

    def run_scene(self, refs, src_lists, unique: bool = False):
        """Fuse the reference views `refs` in that order, view k against src_lists[k] (-1 = missing, at most
        32), in one device-resident pass; the result stays on the GPU until the next run_scene (read it with
        scene_points).  unique: the duplicate-free mode (ACMMP_FUSE_UNIQUE, include/acmmp.h) -- a depth sample
        contributes to the points of one reference view only, across calls until reset_used().
        Returns (total points, per-view counts)."""
        refs = np.ascontiguousarray(refs, np.int32).reshape(-1)
        if len(src_lists) != refs.size:
            raise ValueError("one source list per reference view")
        n_src = np.array([len(s) for s in src_lists], np.int32)
        srcs = np.full((max(refs.size, 1), 32), -1, np.int32)
        for k, s in enumerate(src_lists):
            srcs[k, :min(len(s), 32)] = np.asarray(s, np.int32).reshape(-1)[:32]     # (> 32 is refused below)
        counts = np.zeros(max(refs.size, 1), np.int32)
        total = C.c_int64(0)
        self._check(self.L.acmmp_fusion_run_scene(self.h, refs.size, _p(refs), _p(n_src), _p(srcs),
                                                  FUSE_UNIQUE if unique else 0, _p(counts), C.byref(total)),
                    "fusion_run_scene")
        self.scene_total = int(total.value)
        return self.scene_total, counts[:refs.size].copy()

    def scene_points(self, first: int, n: int, provenance: bool = False):
        """Points [first, first + n) of the last run_scene: (n, 9) float32, and with provenance also the
        position of each point's view in `refs`, its pixel r*W + c (int32) and its consistent-source mask
        (uint32, bit j = src_lists[k][j])."""
        pts = host_empty((n, 9), np.float32)
        if not provenance:
            self._check(self.L.acmmp_fusion_scene_points(self.h, first, n, _p(pts), None, None, None), "fusion_scene_points")
            return pts
        ref, pix, mask = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.uint32)
        self._check(self.L.acmmp_fusion_scene_points(self.h, first, n, _p(pts), _p(ref), _p(pix), _p(mask)),
                    "fusion_scene_points")
        return pts, ref, pix, mask

    def reset_used(self):
        """Clear every view's used mask (the duplicate-free mode starts over)."""
        self._check(self.L.acmmp_fusion_reset_used(self.h), "fusion_reset_used")

    def used(self, view: int) -> np.ndarray:
        """View's used mask, (H, W) uint8 (test hook)."""
        H, W = int(self.cams[view]["height"]), int(self.cams[view]["width"])
        m = np.empty((H, W), np.uint8)
        self._check(self.L.acmmp_fusion_download_used(self.h, view, _p(m)), "fusion_download_used")
        return m

    def voxelize(self, size: float, origin=None, min_points: int = 1):
        """Reduce the resident scene result to one point per occupied cell of a grid of `size` (centroid, mean
        normal, mean colour, point count; integer accumulation, so bit-reproducible: acmmp_fusion_voxelize,
        include/acmmp.h).  origin None: the component-wise minimum of the cloud.  Cells of fewer than min_points
        points are dropped.  The result stays on the GPU (read it with voxel_points) until the next voxelize or
        run_scene.  Returns (voxels, {"n_occupied", "n_rejected", "origin"})."""
        o = None if origin is None else np.ascontiguousarray(origin, np.float32).reshape(3)
        out = np.zeros(3, np.int64)
        used = np.zeros(3, np.float32)
        self._check(self.L.acmmp_fusion_voxelize(self.h, float(size), None if o is None else _p(o), int(min_points),
                                                 _p(out[0:1]), _p(out[1:2]), _p(out[2:3]), _p(used)), "fusion_voxelize")
        return int(out[0]), {"n_occupied": int(out[1]), "n_rejected": int(out[2]), "origin": used}

    def voxel_points(self, first: int, n: int, counts: bool = False):
        """Voxels [first, first + n) of the last voxelize, in order of first appearance in the scene cloud:
        (n, 9) float32, and with counts also the points per voxel (int32)."""
        pts = host_empty((max(n, 0), 9), np.float32)          # (a negative n is refused below)
        cnt = np.empty(max(n, 0), np.int32) if counts else None
        self._check(self.L.acmmp_fusion_voxel_points(self.h, first, n, _p(pts), None if cnt is None else _p(cnt)),
                    "fusion_voxel_points")
        return (pts, cnt) if counts else pts

    def voxel_table(self, force_slots: int = 0):
        """Test hook: sets the hash-table size of the next voxelize (0 = automatic) and returns the last
        successful run's {"slots", "occupied", "max_probe", "wrapped"}."""
        st = np.zeros(4, np.int64)
        self._check(self.L.acmmp_fusion_voxel_table(self.h, int(force_slots), _p(st[0:1]), _p(st[1:2]), _p(st[2:3]),
                                                    _p(st[3:4])), "fusion_voxel_table")
        return {"slots": int(st[0]), "occupied": int(st[1]), "max_probe": int(st[2]), "wrapped": int(st[3])}

    def set_scene(self, points, ref_index=None, pixel=None, src_mask=None):
        """Replace the scene result with a host cloud, (n, 9) float32 taken bit for bit; the provenance arrays
        default to -1 / -1 / 0 (acmmp_fusion_set_scene).  Discards the voxel and the clean result.  Returns n."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 9)
        n = pts.shape[0]
        opt = [None if a is None else np.ascontiguousarray(a, dt).reshape(-1)
               for a, dt in ((ref_index, np.int32), (pixel, np.int32), (src_mask, np.uint32))]
        if any(a is not None and a.size != n for a in opt):
            raise ValueError("one provenance entry per point")
        self._check(self.L.acmmp_fusion_set_scene(self.h, n, _p(pts) if n else None,
                                                  *[None if a is None or n == 0 else _p(a) for a in opt]), "fusion_set_scene")
        self.scene_total = n
        return n

    def voxel_clean(self, connectivity: int = 26, min_neighbours: int = 0, min_component_voxels: int = 1,
                    min_component_points: int = 1):
        """Drop the voxels of the last voxelize with fewer than min_neighbours occupied neighbours (6-, 18- or
        26-connectivity), label the connected components of the rest and keep those of at least
        min_component_voxels voxels and min_component_points points (acmmp_fusion_voxel_clean, include/acmmp.h).
        The result stays on the GPU (clean_points, voxel_labels, component_table) until the next voxel_clean,
        voxelize, run_scene or set_scene.
        Returns (kept voxels, {"components", "components_kept", "unsupported", "rounds"})."""
        out = np.zeros(5, np.int64)
        self._check(self.L.acmmp_fusion_voxel_clean(self.h, int(connectivity), int(min_neighbours), int(min_component_voxels),
                                                    int(min_component_points), *[_p(out[k:k + 1]) for k in range(5)]),
                    "fusion_voxel_clean")
        return int(out[0]), {"components": int(out[1]), "components_kept": int(out[2]), "unsupported": int(out[3]),
                             "rounds": int(out[4])}

    def clean_points(self, first: int, n: int, counts: bool = False, component: bool = False):
        """Kept voxels [first, first + n) of the last voxel_clean, in voxel order: (n, 9) float32; with counts also
        the points per voxel (int32), with component also the component id (int64)."""
        pts = host_empty((max(n, 0), 9), np.float32)          # (a negative n is refused below)
        cnt = np.empty(max(n, 0), np.int32) if counts else None
        comp = np.empty(max(n, 0), np.int64) if component else None
        self._check(self.L.acmmp_fusion_clean_points(self.h, first, n, _p(pts), None if cnt is None else _p(cnt),
                                                     None if comp is None else _p(comp)), "fusion_clean_points")
        extra = tuple(a for a in (cnt, comp) if a is not None)
        return (pts, *extra) if extra else pts

    def voxel_labels(self, first: int, n: int):
        """(label int64, support int32) of voxels [first, first + n) of the voxel result, from the last voxel_clean:
        the smallest voxel index of the voxel's component (-1: dropped for lack of support) and its neighbours."""
        lab, sup = np.empty(max(n, 0), np.int64), np.empty(max(n, 0), np.int32)
        self._check(self.L.acmmp_fusion_voxel_labels(self.h, first, n, _p(lab), _p(sup)), "fusion_voxel_labels")
        return lab, sup

    def component_table(self, first: int, n: int):
        """(root, voxels, points), int64 each, of components [first, first + n) of the last voxel_clean, in
        ascending order of root."""
        out = [np.empty(max(n, 0), np.int64) for _ in range(3)]
        self._check(self.L.acmmp_fusion_component_table(self.h, first, n, *[_p(a) for a in out]), "fusion_component_table")
        return tuple(out)

    def voxel_visibility(self, views, rel_tol: float, radius: int = 0, min_support: int = 1, max_conflicts: int = 0,
                         source: str = "voxel"):
        """Check the voxel result (source "voxel") or the clean result ("clean") against the depth maps of `views`
        (indices into the set; a view listed twice counts twice): every entry is projected into every view and is
        supported where a depth of the window of `radius` pixels agrees within rel_tol, occluded where the view's
        surface is nearer, in conflict where the view sees through it, unobserved otherwise; entries with at least
        min_support supports and at most max_conflicts conflicts are kept (acmmp_fusion_voxel_visibility,
        include/acmmp.h).  The result stays on the GPU (visible_points, visibility_tallies) until the next
        voxel_visibility or until its source goes.
        Returns (kept entries, {"unsupported", "conflicting", "class_totals"}), class_totals = [support, conflict,
        occluded, unobserved] summed over entries and views."""
        if source not in VIS_SOURCES:
            raise ValueError('source must be "voxel" or "clean"')
        v = np.ascontiguousarray(views, np.int32).reshape(-1)
        out = np.zeros(7, np.int64)
        self._check(self.L.acmmp_fusion_voxel_visibility(self.h, VIS_SOURCES[source], v.size, _p(v) if v.size else None,
                                                         float(rel_tol), int(radius), int(min_support), int(max_conflicts),
                                                         _p(out[0:1]), _p(out[1:2]), _p(out[2:3]), _p(out[3:7])),
                    "fusion_voxel_visibility")
        return int(out[0]), {"unsupported": int(out[1]), "conflicting": int(out[2]),
                             "class_totals": [int(x) for x in out[3:7]]}

    def visible_points(self, first: int, n: int, counts: bool = False, tallies: bool = False):
        """Kept entries [first, first + n) of the last voxel_visibility, in the source's order: (n, 9) float32; with
        counts also the points per entry (int32), with tallies also (support, conflict, occluded), (n, 3) int32."""
        pts = host_empty((max(n, 0), 9), np.float32)          # (a negative n is refused below)
        cnt = np.empty(max(n, 0), np.int32) if counts else None
        tal = np.empty((max(n, 0), 3), np.int32) if tallies else None
        self._check(self.L.acmmp_fusion_visible_points(self.h, first, n, _p(pts), None if cnt is None else _p(cnt),
                                                       None if tal is None else _p(tal)), "fusion_visible_points")
        extra = tuple(a for a in (cnt, tal) if a is not None)
        return (pts, *extra) if extra else pts

    def visibility_tallies(self, first: int, n: int):
        """(support, conflict, occluded) of entries [first, first + n) of the source of the last voxel_visibility,
        kept or not: (n, 3) int32."""
        tal = np.empty((max(n, 0), 3), np.int32)
        self._check(self.L.acmmp_fusion_visibility_tallies(self.h, first, n, _p(tal)), "fusion_visibility_tallies")
        return tal

    def voxel_mesh(self, views, trunc: float, min_weight: int = 1, source: str = "voxel"):
        """Surface mesh of the voxel result (source "voxel"), the clean result ("clean") or the visible result
        ("visible"): a signed distance, truncated at `trunc`, of the cells within one cell of an entry to the depth maps
        of `views`, summed in integers; surface-nets vertices in the cubes of samples seen by at least min_weight views
        whose signs differ, and two triangles per sign change along an axis (acmmp_fusion_voxel_mesh, include/acmmp.h).
        The result stays on the GPU (mesh_vertices, mesh_faces) until the next voxel_mesh or until its source goes.
        Returns (vertices, faces, {"samples", "valid", "cubes", "uncoloured"})."""
        if source not in MESH_SOURCES:
            raise ValueError('source must be "voxel", "clean" or "visible"')
        v = np.ascontiguousarray(views, np.int32).reshape(-1)
        out = np.zeros(6, np.int64)
        self._check(self.L.acmmp_fusion_voxel_mesh(self.h, MESH_SOURCES[source], v.size, _p(v) if v.size else None,
                                                   float(trunc), int(min_weight), *[_p(out[k:k + 1]) for k in range(6)]),
                    "fusion_voxel_mesh")
        return int(out[0]), int(out[1]), {"samples": int(out[2]), "valid": int(out[3]), "cubes": int(out[4]),
                                          "uncoloured": int(out[5])}

    def mesh_vertices(self, first: int, n: int):
        """Vertices [first, first + n) of the last voxel_mesh: (n, 9) float32 (position, normal, colour)."""
        v = host_empty((max(n, 0), 9), np.float32)            # (a negative n is refused below)
        self._check(self.L.acmmp_fusion_mesh_vertices(self.h, first, n, _p(v)), "fusion_mesh_vertices")
        return v

    def mesh_faces(self, first: int, n: int):
        """Triangles [first, first + n) of the last voxel_mesh: (n, 3) int32 vertex indices, counter-clockwise seen
        from free space."""
        t = np.empty((max(n, 0), 3), np.int32)
        self._check(self.L.acmmp_fusion_mesh_faces(self.h, first, n, _p(t)), "fusion_mesh_faces")
        return t

    def mesh_samples(self, first: int, n: int):
        """Test hook: (cells (n, 3) int32, tsdf (n, 2) int32 = (S, n), entry (n,) int64) of samples [first, first + n)
        of the last voxel_mesh."""
        cells, tsdf = np.empty((max(n, 0), 3), np.int32), np.empty((max(n, 0), 2), np.int32)
        ent = np.empty(max(n, 0), np.int64)
        self._check(self.L.acmmp_fusion_mesh_samples(self.h, first, n, _p(cells), _p(tsdf), _p(ent)), "fusion_mesh_samples")
        return cells, tsdf, ent

    def mesh_table(self, force_slots: int = 0):
        """Test hook: sets the sample-table size of the next voxel_mesh (0 = automatic) and returns the last
        successful call's {"slots", "occupied", "max_probe", "wrapped"}."""
        st = np.zeros(4, np.int64)
        self._check(self.L.acmmp_fusion_mesh_table(self.h, int(force_slots), _p(st[0:1]), _p(st[1:2]), _p(st[2:3]),
                                                   _p(st[3:4])), "fusion_mesh_table")
        return {"slots": int(st[0]), "occupied": int(st[1]), "max_probe": int(st[2]), "wrapped": int(st[3])}

    def set_mesh(self, vertices, faces):
        """Makes a host mesh the mesh result, as set_scene does for clouds: vertices (nv, 9) float32 (position, normal,
        colour), faces (nf, 3) int32.  It has no source: it stays until the next voxel_mesh or set_mesh."""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 9)
        t = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        self._check(self.L.acmmp_fusion_set_mesh(self.h, v.shape[0], _p(v) if v.size else None, t.shape[0],
                                                 _p(t) if t.size else None), "fusion_set_mesh")
        return v.shape[0], t.shape[0]

    def mesh_sample(self, spacing: float, seed: int = 0) -> MeshSamples:
        """Samples the faces of the mesh result into an area-uniform cloud, about one point per spacing^2 of surface,
        deterministic in (mesh, spacing, seed) bit for bit (acmmp_fusion_mesh_sample, include/acmmp.h).  The samples stay
        on the GPU (sample_points) as the source "samples" of cloud_distance, cloud_align and cloud_align_plane until
        the next mesh_sample or until the mesh goes.  Returns MeshSamples(n_samples, n_skipped): the points, and the
        faces with a non-finite vertex."""
        sp = float(np.float32(spacing))
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError("seed must be in [0, 2^64)")
        out = np.zeros(2, np.int64)
        self._check(self.L.acmmp_fusion_mesh_sample(self.h, sp, int(seed), _p(out[0:1]), _p(out[1:2])), "fusion_mesh_sample")
        self._n_samples = int(out[0])
        return MeshSamples(n_samples=int(out[0]), n_skipped=int(out[1]))

    def sample_points(self, first: int = 0, n: int | None = None):
        """(points (n, 9) float32 (position, normal, colour), face (n,) int32) of samples [first, first + n) of the last
        mesh_sample (n None: to the end)."""
        if first < 0 or (n is not None and n < 0):
            raise ValueError("first and n must be >= 0")
        if n is None:
            n = max(getattr(self, "_n_samples", 0) - first, 0)
        pts, face = host_empty((n, 9), np.float32), np.empty(n, np.int32)
        self._check(self.L.acmmp_fusion_sample_points(self.h, first, n, _p(pts), _p(face)), "fusion_sample_points")
        return pts, face

    def render_mesh(self, view=None, camera=None, rel_tol: float = 0.01):
        """Renders the mesh result into view `view`'s camera, or with view None into `camera` (one CAMERA_DTYPE record of
        the set's model): a z-buffer over all faces, exact at shared edges, the seam and the poles
        (acmmp_fusion_mesh_render, include/acmmp.h).  The maps stay on the GPU (render_maps) until the next render or
        until the mesh goes.  Returns {"width", "height", "skipped", "counts": {"agree", "mesh_in_front", "mesh_behind",
        "mesh_only", "raw_only", "neither", "back_facing"}}: the pixels by how the rendered depth agrees with the view's
        raw depth within rel_tol (all zero with view None) and the faces skipped."""
        counts, skipped = np.zeros(7, np.int64), np.zeros(1, np.int64)
        if view is None:
            cam = None if camera is None else np.frombuffer(np.ascontiguousarray(camera, dtype=CAMERA_DTYPE).tobytes(),
                                                            CAMERA_DTYPE).copy().reshape(-1)[:1]
            rc = self.L.acmmp_fusion_mesh_render(self.h, -1, None if cam is None else _p(cam), float(rel_tol), _p(counts), _p(skipped))
        else:
            if camera is not None:
                raise ValueError("a view or a camera, not both")
            cam = self.cams[view:view + 1] if 0 <= int(view) < len(self.cams) else None
            rc = self.L.acmmp_fusion_mesh_render(self.h, int(view), None, float(rel_tol), _p(counts), _p(skipped))
        self._check(rc, "fusion_mesh_render")
        self._render_shape = (int(cam[0]["height"]), int(cam[0]["width"]))
        return {"width": self._render_shape[1], "height": self._render_shape[0], "skipped": int(skipped[0]),
                "counts": dict(zip(RENDER_COUNTS, (int(x) for x in counts)))}

    def render_maps(self):
        """The last render_mesh: (depth (H, W) float32, 0 = nothing; face (H, W) int32, -1 = nothing; normal (H, W, 3)
        float32, world space; colour (H, W, 3) float32)."""
        H, W = getattr(self, "_render_shape", None) or (0, 0)
        depth, face = host_empty((H, W), np.float32), np.empty((H, W), np.int32)
        normal, colour = host_empty((H, W, 3), np.float32), host_empty((H, W, 3), np.float32)
        self._check(self.L.acmmp_fusion_render_maps(self.h, _p(depth), _p(face), _p(normal), _p(colour)), "fusion_render_maps")
        return depth, face, normal, colour

    def render_plan(self, small_max: int = 0):
        """Test hook: sets the candidate count up to which a face is rendered by its own lane (0 = the default) and
        returns the last render's {"small", "large", "candidates"}."""
        st = np.zeros(3, np.int64)
        self._check(self.L.acmmp_fusion_render_plan(self.h, int(small_max), _p(st[0:1]), _p(st[1:2]), _p(st[2:3])),
                    "fusion_render_plan")
        return {"small": int(st[0]), "large": int(st[1]), "candidates": int(st[2])}

    def set_reference_cloud(self, xyz):
        """Makes a host cloud, (n, 3) float32 taken bit for bit, the reference cloud of cloud_distance: ground truth, or
        another run's cloud.  It stays until the next set_reference_cloud.  Returns n."""
        p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self._check(self.L.acmmp_fusion_set_reference_cloud(self.h, p.shape[0], _p(p) if p.size else None),
                    "fusion_set_reference_cloud")
        return p.shape[0]

    def cloud_distance(self, source: str = "scene", direction: str = "data_to_ref", max_dist: float = 1.0,
                       thresholds=()) -> CloudDistance:
        """Nearest-neighbour distances between the resident cloud `source` ("scene", "voxels", "clean", "visible",
        "mesh", "samples") and the reference cloud, capped at max_dist: "data_to_ref" measures every point of the data cloud
        against the reference (accuracy), "ref_to_data" the reverse (completeness).  Exhaustive by definition, bit for
        bit (acmmp_fusion_cloud_distance, include/acmmp.h); at most 8 thresholds, each in [0, max_dist].  The per-query
        results stay on the GPU (distance_results) until the source or the reference cloud goes."""
        if source not in DIST_SOURCES:
            raise ValueError('source must be one of ' + ", ".join(DIST_SOURCES))
        if direction not in DIST_DIRECTIONS:
            raise ValueError('direction must be "data_to_ref" or "ref_to_data"')
        tau = np.ascontiguousarray(thresholds, np.float32).reshape(-1)
        out = np.zeros(DIST_SUMMARY_WORDS, np.int64)
        self._check(self.L.acmmp_fusion_cloud_distance(self.h, DIST_SOURCES[source], DIST_DIRECTIONS[direction],
                                                       float(max_dist), tau.size, _p(tau) if tau.size else None, _p(out)),
                    "fusion_cloud_distance")
        self._dist_queries = int(out[0])
        return CloudDistance(n_query=int(out[0]), n_valid=int(out[1]), n_matched=int(out[2]), sum_q=int(out[3]),
                             max_dist=float(np.float32(max_dist)), within=[int(x) for x in out[4:4 + tau.size]],
                             hist=out[12:268].copy())

    def distance_results(self, first: int = 0, n: int | None = None, squared: bool = False):
        """(dist (n,) float32, nearest (n,) int32) of queries [first, first + n) of the last cloud_distance (n None: to
        the end): dist = sqrt(d2), inf for a query that is unmatched or invalid, nearest = the target's index, -1 then.
        squared: d2 itself, the quantity the result is defined in."""
        if n is None:
            n = getattr(self, "_dist_queries", 0) - first
        d2, nn = np.empty(max(n, 0), np.float32), np.empty(max(n, 0), np.int32)      # (a negative n is refused below)
        self._check(self.L.acmmp_fusion_distance_results(self.h, first, n, _p(d2), _p(nn)), "fusion_distance_results")
        return (d2 if squared else np.sqrt(d2)), nn

    def distance_grid(self, force_cell: float = 0.0):
        """Test hook: sets the cell of the search grid of the next cloud_distance calls (0 = automatic) and returns the
        last successful call's {"cell", "cells", "max_list", "rings"}."""
        cell, st = np.zeros(1, np.float32), np.zeros(3, np.int64)
        self._check(self.L.acmmp_fusion_distance_grid(self.h, float(force_cell), _p(cell), _p(st[0:1]), _p(st[1:2]),
                                                      _p(st[2:3])), "fusion_distance_grid")
        return {"cell": float(cell[0]), "cells": int(st[0]), "max_list": int(st[1]), "rings": int(st[2])}

    def surface_distance(self, query: str = "reference", max_dist: float = 1.0, thresholds=()) -> CloudDistance:
        """Point-to-triangle distances from the cloud `query` ("reference": completeness against the surface; "scene",
        "voxels", "clean", "visible": the mesh's fidelity to that cloud) to the faces of the mesh result, capped at
        max_dist.  Exhaustive by definition, bit for bit (acmmp_fusion_surface_distance, include/acmmp.h); at most 8
        thresholds, each in [0, max_dist].  The per-query results stay on the GPU (surface_results) until the mesh or
        the query cloud goes."""
        if query not in SURF_QUERIES:
            raise ValueError('query must be one of ' + ", ".join(SURF_QUERIES))
        md = float(max_dist)
        if not (np.isfinite(md) and md > 0.0):
            raise ValueError("max_dist must be finite and > 0")
        tau = np.ascontiguousarray(thresholds, np.float32).reshape(-1)
        if tau.size > 8:
            raise ValueError("at most 8 thresholds")
        if not np.all(np.isfinite(tau) & (tau >= 0) & (tau <= np.float32(md))):
            raise ValueError("every threshold must be finite and in [0, max_dist]")
        out = np.zeros(DIST_SUMMARY_WORDS, np.int64)
        self._check(self.L.acmmp_fusion_surface_distance(self.h, SURF_QUERIES[query], md, tau.size,
                                                         _p(tau) if tau.size else None, _p(out)), "fusion_surface_distance")
        self._surf_queries = int(out[0])
        return CloudDistance(n_query=int(out[0]), n_valid=int(out[1]), n_matched=int(out[2]), sum_q=int(out[3]),
                             max_dist=float(np.float32(max_dist)), within=[int(x) for x in out[4:4 + tau.size]],
                             hist=out[12:268].copy())

    def surface_results(self, first: int = 0, n: int | None = None, squared: bool = False):
        """(dist (n,) float32, nearest_face (n,) int32) of queries [first, first + n) of the last surface_distance (n
        None: to the end): dist = sqrt(d2), inf for a query that is unmatched or invalid, nearest_face -1 then.
        squared: d2 itself, the quantity the result is defined in."""
        if first < 0 or (n is not None and n < 0):
            raise ValueError("first and n must be >= 0")
        if n is None:
            n = max(getattr(self, "_surf_queries", 0) - first, 0)
        d2, nn = np.empty(n, np.float32), np.empty(n, np.int32)
        self._check(self.L.acmmp_fusion_surface_results(self.h, first, n, _p(d2), _p(nn)), "fusion_surface_results")
        return (d2 if squared else np.sqrt(d2)), nn

    def surface_plan(self, small_max: int = 0):
        """Test hook: sets the number of cells above which a face goes to the overflow list instead of the grid (0 = the
        default, below 0 = every face) and returns the last surface_distance's {"small", "large", "registrations",
        "skipped"}."""
        if not -2 ** 31 <= int(small_max) < 2 ** 31:
            raise ValueError("small_max must fit an int32")
        st = np.zeros(4, np.int64)
        self._check(self.L.acmmp_fusion_surface_plan(self.h, int(small_max), _p(st[0:1]), _p(st[1:2]), _p(st[2:3]),
                                                     _p(st[3:4])), "fusion_surface_plan")
        return {"small": int(st[0]), "large": int(st[1]), "registrations": int(st[2]), "skipped": int(st[3])}

    def surface_grid(self, force_cell: float = 0.0):
        """Test hook: sets the cell of the face grid of the next surface_distance calls (0 = automatic) and returns the
        last successful call's {"cell", "cells", "max_list", "rings"}.  Apart from distance_grid."""
        cell, st = np.zeros(1, np.float32), np.zeros(3, np.int64)
        self._check(self.L.acmmp_fusion_surface_grid(self.h, float(force_cell), _p(cell), _p(st[0:1]), _p(st[1:2]),
                                                     _p(st[2:3])), "fusion_surface_grid")
        return {"cell": float(cell[0]), "cells": int(st[0]), "max_list": int(st[1]), "rings": int(st[2])}

    def set_cloud_transform(self, M):
        """Sets the (3, 4) float64 transform under which cloud_distance reads the data cloud, whatever the source, in
        both directions (a 4x4 matrix gives its first three rows); None clears it.  The reference cloud, the resident
        results and everything that is written stay as they are.  Discards the distance result."""
        if M is None:
            self._check(self.L.acmmp_fusion_set_cloud_transform(self.h, None), "fusion_set_cloud_transform")
            return
        m = np.ascontiguousarray(np.asarray(M, np.float64).reshape(-1)[:12])
        if m.size != 12:
            raise ValueError("the transform is a 3x4 matrix")
        self._check(self.L.acmmp_fusion_set_cloud_transform(self.h, _p(m)), "fusion_set_cloud_transform")

    def cloud_transform(self):
        """The (3, 4) float64 transform that is set, or None."""
        m, is_set = np.zeros(12, np.float64), np.zeros(1, np.int32)
        self._check(self.L.acmmp_fusion_get_cloud_transform(self.h, _p(m), _p(is_set)), "fusion_get_cloud_transform")
        return m.reshape(3, 4) if is_set[0] else None

    def cloud_align(self, source: str, mode: str, max_dist: float, max_iterations: int = 30, stride: int = 1,
                    min_shift: float = 0.0, init=None) -> CloudAlignment:
        """Registers the resident cloud `source` to the reference cloud by iterated closest points inside max_dist
        (acmmp_fusion_cloud_align, include/acmmp.h): mode "rigid" or "similarity", every stride-th point, from `init`
        (None: the identity), until the step moves no corner of the reference's box by more than min_shift or
        max_iterations have run.  The transform that is set is neither read nor written: install the result with
        set_cloud_transform(result.M)."""
        if source not in DIST_SOURCES:
            raise ValueError('source must be one of ' + ", ".join(DIST_SOURCES))
        if mode not in ALIGN_MODES:
            raise ValueError('mode must be "rigid" or "similarity"')
        m0 = None if init is None else np.ascontiguousarray(np.asarray(init, np.float64).reshape(-1)[:12])
        if m0 is not None and m0.size != 12:
            raise ValueError("init is a 3x4 matrix")
        M, it, stop = np.zeros(12, np.float64), np.zeros(1, np.int32), np.zeros(1, np.int32)
        self._check(self.L.acmmp_fusion_cloud_align(self.h, DIST_SOURCES[source], ALIGN_MODES[mode], float(max_dist),
                                                    int(max_iterations), int(stride), float(min_shift),
                                                    None if m0 is None else _p(m0), _p(M), _p(it), _p(stop)),
                    "fusion_cloud_align")
        return CloudAlignment(M=M.reshape(3, 4), iterations=int(it[0]), stop_reason=ALIGN_STOP_REASONS[int(stop[0])],
                              records=self.align_records(0, int(it[0]), max_dist))

    def align_records(self, first: int, n: int, max_dist: float = 1.0):
        """AlignRecord of iterations [first, first + n) of the last cloud_align (max_dist: that call's, for mean)."""
        w, M, sh = np.zeros((max(n, 0), ALIGN_RECORD_WORDS), np.int64), np.zeros((max(n, 0), 12)), np.zeros(max(n, 0))
        self._check(self.L.acmmp_fusion_align_records(self.h, first, n, _p(w), _p(M), _p(sh)), "fusion_align_records")
        return [AlignRecord(words=w[k].copy(), M=M[k].reshape(3, 4).copy(), shift=float(sh[k]),
                            max_dist=float(np.float32(max_dist))) for k in range(n)]

    def cloud_align_plane(self, source: str, max_dist: float, max_iterations: int = 30, stride: int = 1,
                          min_shift: float = 0.0, init=None) -> CloudAlignment:
        """Refines `init` (None: the identity; usually cloud_align's result) by iterated closest points with a
        point-to-plane residual along the data cloud's own normals (acmmp_fusion_cloud_align_plane, include/acmmp.h):
        rigid only, otherwise cloud_align's arguments, stop reasons and lifetimes.  The records are AlignPlaneRecord."""
        if source not in DIST_SOURCES:
            raise ValueError('source must be one of ' + ", ".join(DIST_SOURCES))
        m0 = None if init is None else np.ascontiguousarray(np.asarray(init, np.float64).reshape(-1)[:12])
        if m0 is not None and m0.size != 12:
            raise ValueError("init is a 3x4 matrix")
        M, it, stop = np.zeros(12, np.float64), np.zeros(1, np.int32), np.zeros(1, np.int32)
        self._check(self.L.acmmp_fusion_cloud_align_plane(self.h, DIST_SOURCES[source], float(max_dist), int(max_iterations),
                                                          int(stride), float(min_shift), None if m0 is None else _p(m0),
                                                          _p(M), _p(it), _p(stop)), "fusion_cloud_align_plane")
        return CloudAlignment(M=M.reshape(3, 4), iterations=int(it[0]), stop_reason=ALIGN_STOP_REASONS[int(stop[0])],
                              records=self.align_plane_records(0, int(it[0]), max_dist))

    def align_plane_records(self, first: int, n: int, max_dist: float = 1.0):
        """AlignPlaneRecord of iterations [first, first + n) of the last cloud_align_plane (max_dist: that call's)."""
        w, M, sh = np.zeros((max(n, 0), ALIGN_PLANE_RECORD_WORDS), np.int64), np.zeros((max(n, 0), 12)), np.zeros(max(n, 0))
        self._check(self.L.acmmp_fusion_align_plane_records(self.h, first, n, _p(w), _p(M), _p(sh)),
                    "fusion_align_plane_records")
        return [AlignPlaneRecord(words=w[k].copy(), M=M[k].reshape(3, 4).copy(), shift=float(sh[k]),
                                 max_dist=float(np.float32(max_dist))) for k in range(n)]

    def set_region(self, side: str, region, queries_only: bool = False):
        """Sets the evaluation region of a side of the comparison, "data" (every data cloud, read under the transform)
        or "reference" (acmmp_fusion_set_region, include/acmmp.h): cloud_distance, surface_distance, cloud_align and
        cloud_align_plane then treat the side's points outside it as invalid.  region: an io.Region (io.read_region), or
        None to clear.  queries_only: the points outside stay targets.  The region is copied and stays until it is
        replaced; a set or clear discards the distance, surface and align results."""
        if side not in REGION_SIDES:
            raise ValueError('side must be "data" or "reference"')
        flags = REGION_QUERIES_ONLY if queries_only else 0
        if region is None:
            self._check(self.L.acmmp_fusion_set_region(self.h, REGION_SIDES[side], None, flags), "fusion_set_region")
            return
        st, keep = region_struct(region)
        self._check(self.L.acmmp_fusion_set_region(self.h, REGION_SIDES[side], C.byref(st), flags), "fusion_set_region")
        del keep

    def region(self, side: str):
        """What is set for a side: None, or {"queries_only", "n_planes", "n_vertices", "dims"}."""
        if side not in REGION_SIDES:
            raise ValueError('side must be "data" or "reference"')
        w = np.zeros(7, np.int32)
        self._check(self.L.acmmp_fusion_get_region(self.h, REGION_SIDES[side], _p(w[0:1]), _p(w[1:2]), _p(w[2:3]),
                                                   _p(w[3:4]), _p(w[4:7])), "fusion_get_region")
        if not w[0]:
            return None
        return {"queries_only": bool(w[1] & REGION_QUERIES_ONLY), "n_planes": int(w[2]), "n_vertices": int(w[3]),
                "dims": tuple(int(x) for x in w[4:7])}

    def region_classify(self, source: str) -> dict:
        """Classifies the resident cloud `source` (a cloud_distance source, or "reference") under the region of its side,
        a data cloud under the transform that is set: {"points", "invalid", "inside", "planes", "prism", "grid"}, the last
        three the points each part fails.  The class bytes stay on the GPU (region_classes)."""
        if source not in REGION_SOURCES:
            raise ValueError('source must be one of ' + ", ".join(REGION_SOURCES))
        out = np.zeros(len(REGION_COUNTS), np.int64)
        self._check(self.L.acmmp_fusion_region_classify(self.h, REGION_SOURCES[source], _p(out)), "fusion_region_classify")
        self._region_points = int(out[0])
        return {k: int(v) for k, v in zip(REGION_COUNTS, out)}

    def region_classes(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """(n,) uint8 class bytes of points [first, first + n) of the last region_classify (n None: to the end): 0 =
        inside, else REGION_CLASS_BITS or-ed."""
        if first < 0 or (n is not None and n < 0):
            raise ValueError("first and n must be >= 0")
        if n is None:
            n = max(getattr(self, "_region_points", 0) - first, 0)
        cls = np.empty(n, np.uint8)
        self._check(self.L.acmmp_fusion_region_classes(self.h, first, n, _p(cls)), "fusion_region_classes")
        return cls

    def close(self):
        if self.h:
            self.L.acmmp_fusion_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
