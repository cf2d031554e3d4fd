"""Area-uniform samples of the mesh (acmmp_fusion_mesh_sample, include/acmmp.h) restated in numpy, step by step: uint64
arithmetic for steps 0, 3 and 5, float64 for steps 2 and 5, one rounding to float32 per output.  Also the meshes the
tests sample and capi.Fusion's sample surface on top of the restated fusion chain."""
import dataclasses
import functools

import numpy as np

import cloud_align_support as ca
import cloud_distance_support as cd
import mesh_render_support as rs
import surface_distance_support as sd

F32, F64, U64 = np.float32, np.float64, np.uint64
G1, G2 = U64(0xC13FA9A902A6328F), U64(0x91E10DA5C79E7B1D)
ONE = U64(1) << U64(53)
MAX_SAMPLES = 2 ** 31 - 1


def mix(z):
    """Step 0: splitmix64's finaliser on uint64 arrays (arithmetic mod 2^64)."""
    z = np.asarray(z, U64)
    with np.errstate(over="ignore"):
        z = z + U64(0x9e3779b97f4a7c15)
        z = (z ^ (z >> U64(30))) * U64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> U64(27))) * U64(0x94d049bb133111eb)
    return z ^ (z >> U64(31))


def face_hash(seed, nf):
    """h_f = mix(seed ^ mix(f)) for f = 0 .. nf."""
    return mix(U64(int(seed)) ^ mix(np.arange(nf, dtype=U64)))


def check_spacing(spacing):
    with np.errstate(over="ignore"):
        s = F32(spacing)
    if not np.isfinite(s) or not s > 0:
        raise ValueError("spacing must be finite and > 0")
    return s


def expected(vertices, faces, spacing):
    """Steps 1 to 3 without the rounding: (valid (F,) bool, e (F,) float64; 0 where invalid)."""
    s = check_spacing(spacing)
    V = np.asarray(vertices, F32).reshape(-1, 9)[:, :3]
    T = np.asarray(faces, np.int64).reshape(-1, 3)
    A, B, C = (V[T[:, k]].astype(F64) for k in range(3))
    ok = np.isfinite(A).all(1) & np.isfinite(B).all(1) & np.isfinite(C).all(1)
    with np.errstate(all="ignore"):
        E1, E2 = B - A, C - A
        Nx = E1[:, 1] * E2[:, 2] - E1[:, 2] * E2[:, 1]
        Ny = E1[:, 2] * E2[:, 0] - E1[:, 0] * E2[:, 2]
        Nz = E1[:, 0] * E2[:, 1] - E1[:, 1] * E2[:, 0]
        area = 0.5 * np.sqrt((Nx * Nx + Ny * Ny) + Nz * Nz)
        e = area / (F64(s) * F64(s))
    return ok, np.where(ok, e, 0.0)


def counts(vertices, faces, spacing, seed=0):
    """Steps 1 to 3: (n_f (F,) int64, n_skipped)."""
    ok, e = expected(vertices, faces, spacing)
    big = e >= 2.0 ** 31
    k = np.floor(np.where(big, 0.0, e))
    r = np.where(big, 0.0, e) - k
    T = (r * 9007199254740992.0).astype(U64)
    h = face_hash(seed, len(e))
    n = k.astype(np.int64) + ((h >> U64(11)) < T).astype(np.int64)
    n = np.where(big, np.int64(2 ** 31), n)
    return np.where(ok, n, 0).astype(np.int64), int((~ok).sum())


def weights(h, j, hashed=True):
    """Step 5's integers for samples j (uint64) of faces with hashes h (uint64): (i0, i1, i2)."""
    h, j = np.asarray(h, U64), np.asarray(j, U64)
    o1 = mix(h) if hashed else np.zeros_like(h)
    o2 = mix(o1) if hashed else np.zeros_like(h)
    with np.errstate(over="ignore"):
        i1 = (o1 + j * G1) >> U64(11)
        i2 = (o2 + j * G2) >> U64(11)
    fold = i1 + i2 > ONE
    i1 = np.where(fold, ONE - i1, i1)
    i2 = np.where(fold, ONE - i2, i2)
    return ONE - i1 - i2, i1, i2


def sample(vertices, faces, spacing, seed=0):
    """Steps 1 to 6.  Returns (points (N, 9) float32, face (N,) int32, n_skipped); N > 2^31 - 1 raises
    OverflowError before anything of size N is made."""
    V = np.asarray(vertices, F32).reshape(-1, 9)
    T = np.asarray(faces, np.int64).reshape(-1, 3)
    n, skipped = counts(V, T, spacing, seed)
    N = sum(int(x) for x in n)
    if N > MAX_SAMPLES:
        raise OverflowError("more than 2^31 - 1 samples")
    face = np.repeat(np.arange(len(n), dtype=np.int64), n)
    offset = np.cumsum(n) - n                                         # step 6: the exclusive prefix sum
    j = (np.arange(N, dtype=np.int64) - offset[face]).astype(U64)
    i0, i1, i2 = weights(face_hash(seed, len(n))[face], j)
    w0, w1, w2 = (i.astype(F64) * 2.0 ** -53 for i in (i0, i1, i2))
    A, B, C = (V[T[face, k]].astype(F64) for k in range(3))
    with np.errstate(all="ignore"):
        blend = (w0[:, None] * A + w1[:, None] * B) + w2[:, None] * C
        out = blend.astype(F32)
        M = blend[:, 3:6]
        length = np.sqrt((M[:, 0] * M[:, 0] + M[:, 1] * M[:, 1]) + M[:, 2] * M[:, 2])
        unit = (M / length[:, None]).astype(F32)
        out[:, 3:6] = np.where((length > 0)[:, None], unit, F32(0))
    return np.ascontiguousarray(out), face.astype(np.int32), skipped


# ---- the meshes of the tests

def square(side=1.0, at=(0.0, 0.0, 0.0)):
    """Two triangles making a square of the given side in the plane z = at[2], normals that differ per vertex."""
    xyz = np.array([[0, 0, 0], [side, 0, 0], [side, side, 0], [0, side, 0]], F64) + np.asarray(at, F64)
    normals = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, 0.6, 0.8], [0, 0, -1]], F32)
    return rs.as_mesh(xyz, [(0, 1, 2), (0, 2, 3)], normals=normals)


@functools.lru_cache(maxsize=None)
def tiny_faces(n=1000, seed=4):
    """n small triangles of areas around 3e-5 scattered in the unit cube, three vertices of their own each."""
    rng = np.random.default_rng(seed)
    centre = rng.random((n, 1, 3))
    corner = centre + 0.01 * rng.standard_normal((n, 3, 3))
    normals = rng.standard_normal((3 * n, 3))
    normals /= np.linalg.norm(normals, axis=1)[:, None]
    return rs.as_mesh(corner.reshape(-1, 3), np.arange(3 * n).reshape(n, 3), normals=normals.astype(F32),
                      colours=rng.integers(0, 256, (3 * n, 3)).astype(F32))


def spacing_for(vertices, faces, e_mean):
    """The float32 spacing at which the mean expected count of the valid faces is about e_mean."""
    ok, e = expected(vertices, faces, 1.0)
    return float(F32(np.sqrt(e[ok].mean() / e_mean)))


def embedded(where):
    """tiny_faces() with square()'s two faces at the front, in the middle or at the end of the face list."""
    tv, tf = tiny_faces()
    qv, qf = square()
    v = np.concatenate([tv, qv])
    qf = qf + len(tv)
    at = {"front": 0, "middle": len(tf) // 2, "end": len(tf)}[where]
    return v, np.concatenate([tf[:at], qf, tf[at:]]).astype(np.int32)


def with_bad_faces():
    """Valid faces with a degenerate one (A == B), one with a NaN vertex and one with an infinite vertex between them."""
    v, f = sd.cube()
    v = np.concatenate([v, rs.as_mesh([[np.nan, 0, 0], [0, np.inf, 0]], [])[0]])
    n = len(v) - 2
    f = np.concatenate([f[:3], [[1, 1, 2]], f[3:6], [[0, n, 2]], f[6:8], [[3, 1, n + 1]], f[8:]]).astype(np.int32)
    return v, f


def all_invalid():
    v = rs.as_mesh([[np.nan, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, np.inf]], [])[0]
    return v, np.array([[0, 1, 2], [1, 2, 3], [3, 0, 1]], np.int32)


def moved_cube():
    v, f = sd.cube()
    v = v.copy()
    v[:, :3] += F32(1e4)
    return v, f


# ---- capi.Fusion's sample surface on the restated chain

@dataclasses.dataclass
class Samples:
    n_samples: int
    n_skipped: int


class RestatedSampleFusion(sd.RestatedSurfaceFusion):
    """RestatedSurfaceFusion with capi.Fusion's mesh_sample / sample_points and the source "samples" of cloud_distance and
    cloud_align computed by the restatement.  The samples remember the mesh they were taken from and are gone once it
    has been replaced or discarded."""

    def __init__(self, cams):
        super().__init__(cams)
        self._samples = None                       # (the mesh result, points, face)

    def mesh_sample(self, spacing, seed=0):
        if self.meshed is None:
            raise ValueError("no mesh result")
        pts, face, skipped = sample(self.meshed["vertices"], self.meshed["faces"], spacing, seed)
        self._samples = (self.meshed, pts, face)
        return Samples(len(pts), skipped)

    def _held_samples(self):
        s = self._samples
        if s is None or s[0] is not self.meshed:
            raise ValueError("no such data result")
        return s

    def sample_points(self, first=0, n=None):
        s = self._samples if self._samples is not None and self._samples[0] is self.meshed else None
        total = 0 if s is None else len(s[1])
        n = total - first if n is None else n
        if first < 0 or n < 0 or first + n > total:
            raise ValueError("range beyond the sample result")
        if s is None:
            return np.zeros((0, 9), F32), np.zeros(0, np.int32)
        return s[1][first:first + n].copy(), s[2][first:first + n].copy()

    def cloud_distance(self, source="scene", direction="data_to_ref", max_dist=1.0, thresholds=()):
        if source != "samples":
            return super().cloud_distance(source, direction, max_dist, thresholds)
        if direction not in cd.DIRECTIONS:
            raise ValueError("bad direction")
        s = self._held_samples()
        if self.reference is None:
            raise ValueError("no reference cloud")
        data = cd.xyz_of(s[1]) if self._transform is None else ca.transform_points(self._transform, s[1])
        q, t = (data, self.reference) if direction == "data_to_ref" else (self.reference, data)
        d2, nearest, words = cd.distances(q, t, max_dist, thresholds)
        self._distance = (s[0], self.reference, d2, nearest)
        return cd.Summary(words, max_dist, len(tuple(thresholds)))

    def cloud_align(self, source, mode, max_dist, max_iterations=30, stride=1, min_shift=0.0, init=None):
        if source != "samples":
            return super().cloud_align(source, mode, max_dist, max_iterations, stride, min_shift, init)
        ca.check_arguments(mode, max_dist, max_iterations, stride, min_shift, init)
        s = self._held_samples()
        if self.reference is None:
            raise ValueError("no reference cloud")
        r = ca.align(cd.xyz_of(s[1]), self.reference, mode, max_dist, max_iterations, stride, min_shift, init)
        self._align = (s[0], self.reference, r.records)
        return r
