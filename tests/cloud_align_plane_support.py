"""Point-to-plane registration (acmmp_fusion_cloud_align_plane, include/acmmp.h) restated in numpy on top of
cloud_align_support and cloud_distance_support: the matching of the point call, the data cloud's normals under M in
float64, the quantisation, the row (L x Nn, Nn) and the residual in Python integers, the split sums, the pivot, the fit
through numpy.linalg.eigh, the loop.  Also the clouds of the GPU tests and capi.Fusion's plane surface on top of the
restated fusion chain."""
import dataclasses
import functools

import numpy as np

import cloud_align_support as ca
import cloud_distance_support as cd

F32 = np.float32
RECORD_WORDS = 70
N_QUERY, N_VALID, N_MATCHED, SUM_Q, N_OUT_OF_RANGE, N_NO_NORMAL, N_PAIRS, SUM_Q3, PIVOT, ZERO, CC, CR, RR = \
    0, 1, 2, 3, 4, 5, 6, 7, 10, 13, 14, 56, 68
CC_PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]           # the 21 products c_a c_b in the record's order


def points9(data):
    """(n, 9) float32: a data cloud with its normals at floats 3..5."""
    a = np.asarray(data, F32)
    if a.ndim != 2 or a.shape[1] != 9:
        raise ValueError("a data cloud is 9 floats per point")
    return a


def with_normals(xyz, normals):
    """cd.as_points with the given normals."""
    p = cd.as_points(xyz)
    p[:, 3:6] = normals
    return p


def quantised_normals(M, normals):
    """Step 2: (usable (n,) bool, Nn (n, 3) float64 holding integers; rows that are not usable hold zeros)."""
    M = ca.as_matrix(M)
    n = np.asarray(normals, F32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        u = np.stack([(M[a, 0] * n[:, 0] + M[a, 1] * n[:, 1]) + M[a, 2] * n[:, 2] for a in range(3)], 1)
        l2 = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
        usable = np.isfinite(n).all(1) & np.isfinite(l2) & (l2 > 0)
        Nn = np.zeros_like(u)
        Nn[usable] = np.rint(u[usable] / np.sqrt(l2[usable])[:, None] * 4096.0)
    return usable, Nn


def pivot(sum_q3, n):
    """Step 6: floor((2 sumQ_a + N) / (2 N)) per axis in integers; zeros when N is 0."""
    n = int(n)
    return [0, 0, 0] if n <= 0 else [(2 * int(s) + n) // (2 * n) for s in sum_q3]


def row(L, Nn, D):
    """(c: six ints, r) of one pair from the lever, the quantised normal and D = P - Q (Python ints)."""
    c = [L[1] * Nn[2] - L[2] * Nn[1], L[2] * Nn[0] - L[0] * Nn[2], L[0] * Nn[1] - L[1] * Nn[0], Nn[0], Nn[1], Nn[2]]
    return c, (D[0] * Nn[0] + D[1] * Nn[1]) + D[2] * Nn[2]


def split_add(w, at, prod):
    w[at] += prod >> 32
    w[at + 1] += prod & 0xffffffff


def row_moments(rows):
    """The words from CC on for rows [(c, r), ...] of Python ints: split sums."""
    w = [0] * RECORD_WORDS
    for c, r in rows:
        for k, (a, b) in enumerate(CC_PAIRS):
            split_add(w, CC + 2 * k, c[a] * c[b])
        for a in range(6):
            split_add(w, CR + 2 * a, c[a] * r)
        split_add(w, RR, r * r)
    return w


def point_pivot(M, data, ref, max_dist, stride=1):
    """g_0: the pivot from the point call's record under M (the pass before iteration 0)."""
    w = ca.iteration_record(M, cd.xyz_of(points9(data)), ref, max_dist, stride)
    return pivot(w[ca.SUM_Q3:ca.SUM_Q3 + 3], w[ca.N_PAIRS])


def iteration_record(M, g, data, ref, max_dist, stride=1):
    """The RECORD_WORDS Python integers of one iteration under M with the pivot g (steps 1 to 4)."""
    md = F32(max_dist)
    pts = points9(data)[::stride]
    X = ca.transform_points(M, pts[:, :3])
    T = cd.xyz_of(ref)
    d2, nn, summary = cd.distances(X, T, md)
    c, _ = ca.target_box(T)
    kq = 65536.0 / float(md)
    g = [int(x) for x in g]
    hit = nn >= 0
    Pf, Qf = ca.quantise(X[hit], c, kq), ca.quantise(T[nn[hit]], c, kq)
    usable, Nn = quantised_normals(M, pts[hit][:, 3:6])
    rows, w_sum_q, out_of_range, no_normal = [], [0, 0, 0], 0, 0
    for k in range(len(Pf)):
        if not ((np.abs(Pf[k]) < 2.0 ** 30).all() and (np.abs(Qf[k]) < 2.0 ** 30).all()):
            out_of_range += 1
            continue
        P, Q = [int(v) for v in Pf[k]], [int(v) for v in Qf[k]]
        lever = [Q[a] - g[a] for a in range(3)]
        if not all(abs(v) < 2 ** 30 for v in lever):
            out_of_range += 1
            continue
        if not usable[k]:
            no_normal += 1
            continue
        L = [v >> 12 for v in lever]
        n = [int(v) for v in Nn[k]]
        D = [P[a] - Q[a] for a in range(3)]
        assert all(abs(v) <= 2 ** 18 for v in L) and all(abs(v) <= 4096 for v in n) and all(abs(v) < 2 ** 17 for v in D)
        rows.append(row(L, n, D))
        for a in range(3):
            w_sum_q[a] += Q[a]
    w = row_moments(rows)
    w[N_QUERY], w[N_VALID], w[N_MATCHED], w[SUM_Q] = summary[:4]
    w[N_OUT_OF_RANGE], w[N_NO_NORMAL], w[N_PAIRS] = out_of_range, no_normal, len(rows)
    w[SUM_Q3:SUM_Q3 + 3] = w_sum_q
    w[PIVOT:PIVOT + 3] = g
    return w


def join(w, at):
    return int(w[at]) * (1 << 32) + int(w[at + 1])


def system(record):
    """(S (6, 6), b (6,)) in float64 from a record: S_ab = (double) sum c_a c_b, b_a = -(double) sum c_a r."""
    S = np.zeros((6, 6))
    for k, (a, b) in enumerate(CC_PAIRS):
        S[a, b] = S[b, a] = float(join(record, CC + 2 * k))
    return S, np.array([-float(join(record, CR + 2 * a)) for a in range(6)])


def scaled_system(record):
    """(S', b', s) after the Jacobi scaling, or None when N < 6 or a diagonal entry is 0."""
    if int(record[N_PAIRS]) < 6:
        return None
    S, b = system(record)
    if (np.diag(S) == 0).any():
        return None
    s = np.sqrt(np.diag(S))
    return S / np.outer(s, s), b / s, s


def condition(record):
    """lambda_max / lambda_min of the scaled system; inf where there is none or lambda_min <= 0."""
    parts = scaled_system(record)
    if parts is None:
        return np.inf
    lam = np.linalg.eigvalsh(parts[0])
    return float(lam[-1] / lam[0]) if lam[0] > 0 else np.inf


def rodrigues(omega):
    """R = I + A K + B K^2 of step 5."""
    om = np.asarray(omega, np.float64)
    K = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    theta2 = (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]
    if theta2 >= 2.0 ** -40:
        theta = np.sqrt(theta2)
        A, B = np.sin(theta) / theta, (1.0 - np.cos(theta)) / theta2
    else:
        A, B = 1.0 - theta2 / 6.0, 0.5 - theta2 / 24.0
    return np.eye(3) + A * K + B * (K @ K)


def solve(record):
    """x (6,) of step 5 in lattice units, or None for a degenerate record."""
    parts = scaled_system(record)
    if parts is None:
        return None
    Sp, bp, s = parts
    lam, V = np.linalg.eigh(Sp)
    if not lam[0] > lam[-1] * 2.0 ** -40:
        return None
    if not rotation_over_noise(record) > 4.0:
        return None
    return (V @ ((V.T @ bp) / lam)) / s


def rotation_over_noise(record):
    """The noise-floor rule of step 5: the smallest eigenvalue of what the translation columns leave of the rotation
    columns (the Schur complement of S, whose inverse is the rotation block of S^-1), over (S_33 + S_44 + S_55) / 18,
    what the levers' rounding alone puts there.  For a record that passes the rules before it."""
    Sp, _, s = scaled_system(record)
    lam, V = np.linalg.eigh(Sp)
    P = ((V / lam) @ V.T)[:3, :3] / np.outer(s[:3], s[:3])
    S, _ = system(record)
    return float(1.0 / (np.linalg.eigvalsh(P)[-1] * ((S[3, 3] + S[4, 4]) + S[5, 5]) / 18.0))


def fit(record, c, max_dist):
    """Step 5: D (3, 4) float64, or None for a degenerate iteration."""
    x = solve(record)
    if x is None:
        return None
    kq = 65536.0 / float(F32(max_dist))
    R = rodrigues(x[:3] / 4096.0)
    tau = x[3:] / kq
    G = np.asarray(c, np.float64) + np.array([float(int(v)) for v in record[PIVOT:PIVOT + 3]]) / kq
    D = np.zeros((3, 4))
    D[:, :3] = R
    D[:, 3] = G + tau - R @ G
    return D


@dataclasses.dataclass
class Record:
    """capi.AlignPlaneRecord's fields and properties."""
    words: np.ndarray
    M: np.ndarray
    shift: float
    max_dist: float

    n_query = property(lambda self: int(self.words[N_QUERY]))
    n_valid = property(lambda self: int(self.words[N_VALID]))
    n_matched = property(lambda self: int(self.words[N_MATCHED]))
    sum_q = property(lambda self: int(self.words[SUM_Q]))
    n_out_of_range = property(lambda self: int(self.words[N_OUT_OF_RANGE]))
    n_no_normal = property(lambda self: int(self.words[N_NO_NORMAL]))
    n_pairs = property(lambda self: int(self.words[N_PAIRS]))
    pivot = property(lambda self: [int(x) for x in self.words[PIVOT:PIVOT + 3]])

    @property
    def mean(self):
        return self.sum_q / (self.n_matched * (1048576.0 / self.max_dist)) if self.n_matched else 0.0

    @property
    def rms_plane(self):
        kq = 65536.0 / self.max_dist
        return float(np.sqrt(join(self.words, RR) / self.n_pairs)) / (kq * 4096.0) if self.n_pairs else 0.0


def check_arguments(max_dist, max_iterations, stride, min_shift, init):
    return ca.check_arguments("rigid", max_dist, max_iterations, stride, min_shift, init)


def align_plane(data, ref, max_dist, max_iterations=30, stride=1, min_shift=0.0, init=None):
    """The loop of acmmp_fusion_cloud_align_plane over host clouds (data: 9 floats per point)."""
    md, M = check_arguments(max_dist, max_iterations, stride, min_shift, init)
    data = points9(data)
    lo, hi = ca.target_box(ref)
    g = point_pivot(M, data, ref, md, stride)
    records, stop = [], "max_iterations"
    for _ in range(int(max_iterations)):
        w = iteration_record(M, g, data, ref, md, stride)
        D = fit(w, lo, md)
        rec = Record(np.array(w, np.int64), M.copy(), 0.0, float(md))
        records.append(rec)
        if D is None:
            stop = "degenerate"
            break
        nxt = ca.compose(D, M)
        shift = ca.corner_shift(D, lo, hi)
        if not (np.isfinite(nxt).all() and np.isfinite(shift)):
            stop = "degenerate"
            break
        M, rec.shift = nxt, shift
        if rec.shift <= min_shift:
            stop = "converged"
            break
        g = pivot(w[SUM_Q3:SUM_Q3 + 3], w[N_PAIRS])
    return ca.Alignment(M, len(records), stop, records)


def corner_error(M, known, lo=(0, 0, 0), hi=(1, 1, 1)):
    """The largest |M c' - known c'| over the eight corners of the box [lo, hi]: how far M is from the true motion."""
    M, known = ca.as_matrix(M), ca.as_matrix(known)
    best = 0.0
    for k in range(8):
        x = np.array([hi[a] if k >> a & 1 else lo[a] for a in range(3)], np.float64)
        best = max(best, float(np.linalg.norm((M[:, :3] @ x + M[:, 3]) - (known[:, :3] @ x + known[:, 3]))))
    return best


# ---- clouds

def cube_surface(n, rng):
    """(xyz (n, 3) float32, unit normals (n, 3) float32): uniform samples of the unit cube's six faces."""
    face = rng.integers(0, 6, n)
    uv = rng.random((n, 2))
    xyz, nrm = np.zeros((n, 3)), np.zeros((n, 3))
    for f in range(6):
        axis, side = f // 2, f % 2
        sel = face == f
        others = [a for a in range(3) if a != axis]
        xyz[sel, axis] = side
        xyz[np.ix_(sel, others)] = uv[sel]
        nrm[sel, axis] = 2 * side - 1
    return xyz.astype(F32), nrm.astype(F32)


KNOWN_MOTION = ca.about(ca.rotation((1, 2, 3), 1.5), (0.5, 0.5, 0.5), (0.008, -0.006, 0.007))
CLAIM_MAX_DIST, CLAIM_ITERATIONS, CLAIM_POINTS, CLAIM_SEED = 0.06, 8, 3000, 11


@functools.lru_cache(maxsize=None)
def two_samplings(n=CLAIM_POINTS, seed=CLAIM_SEED):
    """(data (n, 9), ref (n, 3), known): two independent samplings of the unit cube's surface; the data cloud, normals
    included, is moved by the inverse of the known rigid motion, so `known` takes it onto the reference surface."""
    rng = np.random.default_rng(seed)
    ref, _ = cube_surface(n, rng)
    xyz, nrm = cube_surface(n, rng)
    inv = ca.inverse(KNOWN_MOTION)
    data = with_normals(ca.transform_points(inv, xyz), (nrm.astype(np.float64) @ inv[:, :3].T).astype(F32))
    return data, ref, KNOWN_MOTION


EDGE_NORMALS = np.array([[0, 0, 0], [np.nan, 0, 1], [0, np.inf, 0], [-np.inf, 1, 1], [1e-42, 0, 0], [0, -3e-45, 2e-45],
                         [1e-3, 0, 0], [0, 6e-4, -8e-4], [1e3, 0, 0], [0, 600, 800], [1e19, 1e19, 1e19], [3e38, 3e38, 3e38],
                         [1e-30, 1e-30, 0]], F32)                      # zero, NaN, inf, denormal, lengths 1e-3 and 1e3, huge


@functools.lru_cache(maxsize=None)
def record_clouds(seed=1):
    """(data (n, 9), ref): cd.clouds() -- cube, cluster, duplicates, ties, a target at 1000 with queries beside it, invalid
    points -- with random unit normals on the data cloud, and the edge normals on the first queries that match."""
    Q, T = cd.clouds()
    rng = np.random.default_rng(seed)
    nrm = rng.standard_normal((len(Q), 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    data = with_normals(Q, nrm.astype(F32))
    with np.errstate(invalid="ignore"):
        inside = (Q >= 0).all(1) & (Q <= 1).all(1)                        # in range under any pivot near the cube
    matched = np.nonzero((cd.restated()[1] >= 0) & inside)[0]
    data[matched[:len(EDGE_NORMALS)], 3:6] = EDGE_NORMALS
    return data, T


SCALED_INIT = ca.about(ca.rotation((-1, 2, 1), 1.0), (0.5, 0.5, 0.5), (0.003, 0.0, -0.002), 1.01)
RECORD_ITERATIONS = 3
# name -> (clouds, max_dist, init, stride, iterations): the runs whose records and fits the GPU tests hold the device to
FIT_CASES = {
    "records": (record_clouds, cd.MAX_DIST, None, 1, RECORD_ITERATIONS),
    "records rotated": (record_clouds, cd.MAX_DIST, ca.SMALL_ROTATION, 1, RECORD_ITERATIONS),
    "records rotated stride 3": (record_clouds, cd.MAX_DIST, ca.SMALL_ROTATION, 3, RECORD_ITERATIONS),
    "records scaled stride 3": (record_clouds, cd.MAX_DIST, SCALED_INIT, 3, RECORD_ITERATIONS),
    "records scaled": (record_clouds, cd.MAX_DIST, SCALED_INIT, 1, RECORD_ITERATIONS),
    "two samplings": (lambda: two_samplings()[:2], CLAIM_MAX_DIST, None, 1, CLAIM_ITERATIONS),
}


@functools.lru_cache(maxsize=None)
def restated_fit_case(name):
    clouds, max_dist, init, stride, iterations = FIT_CASES[name]
    data, ref = clouds()
    return align_plane(data, ref, max_dist, iterations, stride, 0.0, init)


@functools.lru_cache(maxsize=None)
def restated_claim():
    """(plane run, point run) of the restatement on two_samplings(): the same start, cap and iteration count."""
    data, ref, _ = two_samplings()
    return restated_fit_case("two samplings"), ca.align(data[:, :3], ref, "rigid", CLAIM_MAX_DIST, CLAIM_ITERATIONS)


class RestatedAlignPlaneFusion(ca.RestatedAlignFusion):
    """RestatedAlignFusion with capi.Fusion's cloud_align_plane / align_plane_records computed by the restatement.  The
    object holds the records of the last align call of either kind."""

    def __init__(self, cams):
        super().__init__(cams)
        self._align_plane = None                   # (the source result, the reference cloud, the records)

    def _data9(self, source):
        held, _ = cd.RestatedDistanceFusion._data(self, source)
        full = {"scene": lambda: self.result[0], "voxels": lambda: self.voxels["points"],
                "clean": lambda: self.voxels["points"][self.cleaned["kept"]], "visible": lambda: self.visible["points"],
                "mesh": lambda: self.meshed["vertices"]}[source]()
        return held, np.asarray(full, F32)

    def cloud_align(self, *args, **kw):
        r = super().cloud_align(*args, **kw)
        self._align_plane = None
        return r

    def cloud_align_plane(self, source, max_dist, max_iterations=30, stride=1, min_shift=0.0, init=None):
        if source not in cd.SOURCES:
            raise ValueError("bad source")
        check_arguments(max_dist, max_iterations, stride, min_shift, init)
        held, data = self._data9(source)
        if self.reference is None:
            raise ValueError("no reference cloud")
        r = align_plane(data, self.reference, max_dist, max_iterations, stride, min_shift, init)
        self._align_plane = (held, self.reference, r.records)
        self._align = None
        return r

    def align_plane_records(self, first, n, max_dist=1.0):
        a = self._align_plane
        now = (self.result, self.voxels, self.cleaned, self.visible, self.meshed)
        live = a is not None and a[1] is self.reference and any(a[0] is x for x in now)
        recs = a[2] if live else []
        if first < 0 or n < 0 or first + n > len(recs):
            raise ValueError("range beyond the align records")
        return recs[first:first + n]
