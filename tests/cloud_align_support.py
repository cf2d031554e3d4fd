"""Registration of the data cloud to the reference cloud (acmmp_fusion_set_cloud_transform / acmmp_fusion_cloud_align,
include/acmmp.h) restated in numpy: the float64 transform rounded once to float32, matching through
cloud_distance_support.distances, the moments in Python integers, the fit through numpy.linalg.svd, the loop.  Also the
clouds of the recovery test and capi.Fusion's alignment surface on top of the restated fusion chain."""
import dataclasses
import functools

import numpy as np

import cloud_distance_support as cd

F32 = np.float32
MODES = ("rigid", "similarity")
STOP_REASONS = ("max_iterations", "converged", "degenerate")
RECORD_WORDS = 32
N_QUERY, N_VALID, N_MATCHED, SUM_Q, N_OUT_OF_RANGE, N_PAIRS, SUM_P, SUM_Q3, PQ, PP = 0, 1, 2, 3, 4, 5, 6, 9, 12, 30
IDENTITY = np.eye(3, 4)


def as_matrix(M):
    """A (3, 4) float64 copy of a 3x4 or 4x4 matrix."""
    m = np.asarray(M, np.float64).reshape(-1)[:12]
    if m.size != 12:
        raise ValueError("the transform is a 3x4 matrix")
    return m.reshape(3, 4).copy()


def transform_points(M, xyz):
    """x'_k = (float)(((M[k,0]*x + M[k,1]*y) + M[k,2]*z) + M[k,3]) in float64, rounded once to float32."""
    M = as_matrix(M)
    p = cd.xyz_of(xyz).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        out = np.stack([((M[k, 0] * x + M[k, 1] * y) + M[k, 2] * z) + M[k, 3] for k in range(3)], 1)
        return np.ascontiguousarray(out.astype(F32))


def target_box(ref):
    """(c, hi): the per-axis minimum and maximum of the valid targets in float64; zeros when there is none."""
    T = cd.xyz_of(ref)
    Tv = T[cd.valid(T)].astype(np.float64)
    if not len(Tv):
        return np.zeros(3), np.zeros(3)
    return Tv.min(0), Tv.max(0)


def quantise(X, c, kq):
    """(int64) rint(((double)x - c) * kq) per coordinate, as float64 (the range test comes before the conversion)."""
    return np.rint((X.astype(np.float64) - c[None, :]) * kq)


def pair_moments(P, Q):
    """The words from N_PAIRS on for in-range integer pairs P, Q (lists of 3-tuples of Python ints): split sums."""
    w = [0] * RECORD_WORDS
    w[N_PAIRS] = len(P)
    for p, q in zip(P, Q):
        for a in range(3):
            w[SUM_P + a] += p[a]
            w[SUM_Q3 + a] += q[a]
            for b in range(3):
                prod = p[a] * q[b]
                w[PQ + 2 * (3 * a + b)] += prod >> 32
                w[PQ + 2 * (3 * a + b) + 1] += prod & 0xffffffff
        pp = p[0] * p[0] + p[1] * p[1] + p[2] * p[2]
        w[PP] += pp >> 32
        w[PP + 1] += pp & 0xffffffff
    return w


def iteration_record(M, data, ref, max_dist, stride=1):
    """The RECORD_WORDS Python integers of one iteration under M (steps 1 to 3)."""
    md = F32(max_dist)
    X = transform_points(M, cd.xyz_of(data)[::stride])
    T = cd.xyz_of(ref)
    d2, nn, summary = cd.distances(X, T, md)
    c, _ = target_box(T)
    kq = 65536.0 / float(md)
    hit = nn >= 0
    Pf, Qf = quantise(X[hit], c, kq), quantise(T[nn[hit]], c, kq)
    inr = (np.abs(Pf) < 2.0 ** 30).all(1) & (np.abs(Qf) < 2.0 ** 30).all(1)
    P = [tuple(int(v) for v in row) for row in Pf[inr]]
    Q = [tuple(int(v) for v in row) for row in Qf[inr]]
    w = pair_moments(P, Q)
    w[N_QUERY], w[N_VALID], w[N_MATCHED], w[SUM_Q] = summary[:4]
    w[N_OUT_OF_RANGE] = int((~inr).sum())
    return w


def join(w, at):
    return w[at] * (1 << 32) + w[at + 1]


def svd_parts(w):
    """(H, var, d) of a record: the float64 cross-covariance, the variance of P, H's singular values; None when N < 3."""
    w = [int(x) for x in w]
    N = w[N_PAIRS]
    if N < 3:
        return None
    nn = float(N) * float(N)
    H = np.array([[float(N * join(w, PQ + 2 * (3 * a + b)) - w[SUM_P + a] * w[SUM_Q3 + b]) / nn for b in range(3)]
                  for a in range(3)])
    V = N * join(w, PP) - sum(w[SUM_P + a] ** 2 for a in range(3))
    return H, (float(V) / nn if V else 0.0), np.linalg.svd(H, compute_uv=False)


def fit(record, c, max_dist, mode):
    """Step 4: D (3, 4) float64, or None for a degenerate iteration."""
    if mode not in MODES:
        raise ValueError("bad mode")
    parts = svd_parts(record)
    if parts is None or parts[1] == 0.0:
        return None
    H, var, _ = parts
    w = [int(x) for x in record]
    U, d, Vt = np.linalg.svd(H)
    if not d[1] > d[0] * 2.0 ** -40:
        return None
    V = Vt.T
    g = 1.0 if np.linalg.det(V @ U.T) >= 0 else -1.0
    R = V @ np.diag([1.0, 1.0, g]) @ U.T
    s = (d[0] + d[1] + g * d[2]) / var if mode == "similarity" else 1.0
    kq = 65536.0 / float(F32(max_dist))
    N = float(w[N_PAIRS])
    pm = np.asarray(c, np.float64) + np.array([float(w[SUM_P + a]) / N for a in range(3)]) / kq
    qm = np.asarray(c, np.float64) + np.array([float(w[SUM_Q3 + a]) / N for a in range(3)]) / kq
    D = np.zeros((3, 4))
    D[:, :3] = s * R
    D[:, 3] = qm - D[:, :3] @ pm
    return D


def compose(D, M):
    """D o M: per entry (D_a0*M_0b + D_a1*M_1b) + D_a2*M_2b, plus D_a3 in the last column."""
    D, M = as_matrix(D), as_matrix(M)
    out = np.zeros((3, 4))
    for a in range(3):
        for b in range(4):
            out[a, b] = (D[a, 0] * M[0, b] + D[a, 1] * M[1, b]) + D[a, 2] * M[2, b]
            if b == 3:
                out[a, b] += D[a, 3]
    return out


def corner_shift(D, lo, hi):
    """The largest |D c' - c'| over the eight corners of the box [lo, hi]."""
    D = as_matrix(D)
    best = 0.0
    for k in range(8):
        x = np.array([hi[a] if k >> a & 1 else lo[a] for a in range(3)], np.float64)
        y = np.array([((D[a, 0] * x[0] + D[a, 1] * x[1]) + D[a, 2] * x[2]) + D[a, 3] for a in range(3)])
        best = max(best, float(np.sqrt(((y - x) ** 2).sum())))
    return best


@dataclasses.dataclass
class Record:
    """capi.AlignRecord's fields and properties."""
    words: np.ndarray
    M: np.ndarray
    shift: float
    max_dist: float

    n_query = property(lambda self: int(self.words[N_QUERY]))
    n_valid = property(lambda self: int(self.words[N_VALID]))
    n_matched = property(lambda self: int(self.words[N_MATCHED]))
    sum_q = property(lambda self: int(self.words[SUM_Q]))
    n_out_of_range = property(lambda self: int(self.words[N_OUT_OF_RANGE]))
    n_pairs = property(lambda self: int(self.words[N_PAIRS]))

    @property
    def mean(self):
        return self.sum_q / (self.n_matched * (1048576.0 / self.max_dist)) if self.n_matched else 0.0


@dataclasses.dataclass
class Alignment:
    """capi.CloudAlignment's fields."""
    M: np.ndarray
    iterations: int
    stop_reason: str
    records: list


def check_arguments(mode, max_dist, max_iterations, stride, min_shift, init):
    with np.errstate(over="ignore"):
        md = F32(max_dist)
    if mode not in MODES or not np.isfinite(md) or not md > 0:
        raise ValueError("bad mode or max_dist")
    if not 1 <= int(max_iterations) <= 1024 or int(stride) < 1:
        raise ValueError("bad max_iterations or stride")
    if not np.isfinite(min_shift) or min_shift < 0:
        raise ValueError("bad min_shift")
    M = IDENTITY.copy() if init is None else as_matrix(init)
    if not np.isfinite(M).all():
        raise ValueError("bad init")
    return md, M


def align(data, ref, mode, max_dist, max_iterations=30, stride=1, min_shift=0.0, init=None):
    """The loop of acmmp_fusion_cloud_align over host clouds."""
    md, M = check_arguments(mode, max_dist, max_iterations, stride, min_shift, init)
    lo, hi = target_box(ref)
    records, stop = [], "max_iterations"
    for _ in range(int(max_iterations)):
        w = iteration_record(M, data, ref, md, stride)
        D = fit(w, lo, md, mode)
        rec = Record(np.array(w, np.int64), M.copy(), 0.0, float(md))
        records.append(rec)
        if D is None:
            stop = "degenerate"
            break
        M = compose(D, M)
        rec.shift = corner_shift(D, lo, hi)
        if rec.shift <= min_shift:
            stop = "converged"
            break
    return Alignment(M, len(records), stop, records)


def rotation(axis, degrees):
    """Rodrigues: the rotation by `degrees` about `axis`."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    t = np.radians(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def about(R, centre, shift=(0, 0, 0), scale=1.0):
    """(3, 4): x -> scale * R (x - centre) + centre + shift."""
    centre = np.asarray(centre, np.float64)
    M = np.zeros((3, 4))
    M[:, :3] = scale * R
    M[:, 3] = centre - M[:, :3] @ centre + np.asarray(shift, np.float64)
    return M


def inverse(M):
    M = as_matrix(M)
    A = np.linalg.inv(M[:, :3])
    out = np.zeros((3, 4))
    out[:, :3] = A
    out[:, 3] = -A @ M[:, 3]
    return out


def known_transform(mode):
    """The transform of the recovery test: 2 degrees about (1, 2, 3) through the cube's centre plus a small shift, and
    a scale of 1.03 in similarity mode."""
    return about(rotation((1, 2, 3), 2.0), (0.5, 0.5, 0.5), (0.012, -0.008, 0.01), 1.03 if mode == "similarity" else 1.0)


SMALL_ROTATION = about(rotation((3, -1, 2), 2.0), (0.5, 0.5, 0.5))          # the non-identity init of the record tests


@functools.lru_cache(maxsize=None)
def recovery_clouds(mode, seed=3):
    """(data, ref, known): ref = cd.clouds()[1]; data = 3000 of its finite points inside the unit cube moved by the
    inverse of the known transform, plus 300 uniform clutter points, shuffled."""
    rng = np.random.default_rng(seed)
    ref = cd.clouds()[1]
    inside = ref[cd.valid(ref) & (ref >= 0).all(1) & (ref <= 1).all(1)]
    sub = inside[rng.choice(len(inside), 3000, replace=False)]
    known = known_transform(mode)
    data = np.concatenate([transform_points(inverse(known), sub), rng.random((300, 3), dtype=F32)])
    return np.ascontiguousarray(data[rng.permutation(len(data))]), ref, known


@functools.lru_cache(maxsize=None)
def restated_recovery(mode):
    data, ref, _ = recovery_clouds(mode)
    return align(data, ref, mode, cd.MAX_DIST, 10)


class RestatedAlignFusion(cd.RestatedDistanceFusion):
    """RestatedDistanceFusion with capi.Fusion's set_cloud_transform / cloud_transform / cloud_align / align_records
    computed by the restatement, and their lifetime rules: the transform belongs to the object; a set or clear discards
    the distance result; the records go with their source result and with the reference cloud."""

    def __init__(self, cams):
        super().__init__(cams)
        self._transform = None
        self._align = None                         # (the source result, the reference cloud, the records)

    def set_cloud_transform(self, M):
        if M is not None:
            M = as_matrix(M)
            if not np.isfinite(M).all():
                raise ValueError("bad transform")
        self._transform = M
        self._distance = None

    def cloud_transform(self):
        return None if self._transform is None else self._transform.copy()

    def _data(self, source):
        held, xyz = super()._data(source)
        return held, (xyz if self._transform is None else transform_points(self._transform, xyz))

    def cloud_align(self, source, mode, max_dist, max_iterations=30, stride=1, min_shift=0.0, init=None):
        if source not in cd.SOURCES:
            raise ValueError("bad source")
        check_arguments(mode, max_dist, max_iterations, stride, min_shift, init)
        held, xyz = super()._data(source)
        if self.reference is None:
            raise ValueError("no reference cloud")
        r = align(xyz, self.reference, mode, max_dist, max_iterations, stride, min_shift, init)
        self._align = (held, self.reference, r.records)
        return r

    def align_records(self, first, n, max_dist=1.0):
        a = self._align
        now = (self.result, self.voxels, self.cleaned, self.visible, self.meshed)
        live = a is not None and a[1] is self.reference and any(a[0] is x for x in now)
        recs = a[2] if live else []
        if first < 0 or n < 0 or first + n > len(recs):
            raise ValueError("range beyond the align records")
        return recs[first:first + n]
