"""Nearest-neighbour cloud distances (acmmp_fusion_cloud_distance, include/acmmp.h) restated in numpy: exhaustive over
all pairs, the float32 pair distance with the definition's association, the minimum of the 64-bit (distance bits,
index) key, the summary in Python integers.  Also the clouds the GPU tests measure, and capi.Fusion's distance surface
on top of the restated fusion chain."""
import functools

import numpy as np

import mesh_render_support as rs

F32 = np.float32
SOURCES = ("scene", "voxels", "clean", "visible", "mesh")
DIRECTIONS = ("data_to_ref", "ref_to_data")
MAX_TAU, HIST_BINS, SUMMARY_WORDS = 8, 256, 268
TAUS = (0.0, 0.002, 0.005, 0.01, 0.015, 0.02, 0.03, 0.04)          # the eight thresholds of the GPU tests
MAX_DIST = 0.04                                                   # and their cap: see test_generator_matched_share


def xyz_of(cloud):
    """(n, 3) float32: the first three floats of every point."""
    a = np.asarray(cloud, F32)
    a = a.reshape(-1, a.shape[-1] if a.ndim > 1 else 3)
    return np.ascontiguousarray(a[:, :3])


def valid(P):
    """Step 1: the three coordinates are finite."""
    return np.isfinite(P).all(1)


def pair_d2(Q, T):
    """Step 2 for every pair: (len(Q), len(T)) float32, d2 = (dx*dx + dy*dy) + dz*dz."""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = Q[:, None, 0] - T[None, :, 0]
        dy = Q[:, None, 1] - T[None, :, 1]
        dz = Q[:, None, 2] - T[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == F32
    return d2


def check_arguments(max_dist, taus):
    with np.errstate(over="ignore"):
        md = F32(max_dist)
        taus = [F32(t) for t in taus]
    if not np.isfinite(md) or not md > 0:
        raise ValueError("bad max_dist")
    if len(taus) > MAX_TAU or any(not np.isfinite(t) or t < 0 or t > md for t in taus):
        raise ValueError("bad thresholds")
    return md, taus


def distances(Q, T, max_dist, taus=(), rows=256):
    """Steps 1-5 of queries Q against targets T.  Returns (d2 float32, nearest int32, summary: SUMMARY_WORDS Python
    ints -- n_query, n_valid, n_matched, sum_q, within[8], hist[256])."""
    md, taus = check_arguments(max_dist, taus)
    Q, T = xyz_of(Q), xyz_of(T)
    vq, tidx = valid(Q), np.nonzero(valid(T))[0].astype(np.uint64)
    Tv = T[valid(T)]
    d2 = np.full(len(Q), np.inf, F32)
    nearest = np.full(len(Q), -1, np.int32)
    m2 = md * md
    assert m2.dtype == F32
    qi = np.nonzero(vq)[0]
    if len(Tv):
        for a in range(0, len(qi), rows):
            part = qi[a:a + rows]
            d = pair_d2(Q[part], Tv)
            assert not np.isnan(d).any()
            key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | tidx[None, :]
            win = key.min(1)                                              # step 3: the order of the targets is invisible
            w = (win >> np.uint64(32)).astype(np.uint32).view(F32)
            hit = w <= m2                                                 # step 4
            d2[part[hit]] = w[hit]
            nearest[part[hit]] = (win[hit] & np.uint64(0xffffffff)).astype(np.int64).astype(np.int32)
    matched = nearest >= 0
    k = 1048576.0 / float(md)
    q = np.rint(np.sqrt(d2[matched].astype(np.float64)) * k).astype(np.int64)
    summary = [len(Q), int(vq.sum()), int(matched.sum()), sum(int(x) for x in q)]
    for i in range(MAX_TAU):
        summary.append(int((d2[matched] <= taus[i] * taus[i]).sum()) if i < len(taus) else 0)
    hist = np.bincount(np.minimum(q >> 12, HIST_BINS - 1), minlength=HIST_BINS)
    summary += [int(x) for x in hist]
    assert len(summary) == SUMMARY_WORDS
    return d2, nearest, summary


def summary_of(r):
    """A capi.CloudDistance as the SUMMARY_WORDS integers of the header's layout."""
    within = list(r.within) + [0] * (MAX_TAU - len(r.within))
    return [r.n_query, r.n_valid, r.n_matched, r.sum_q, *within, *[int(x) for x in r.hist]]


def as_points(xyz):
    """A cloud of 9 floats per point around the positions (set_scene, set_mesh): unit normal, grey."""
    p = np.zeros((len(xyz), 9), F32)
    p[:, :3] = xyz
    p[:, 5] = 1.0
    p[:, 6:9] = 128.0
    return p


@functools.lru_cache(maxsize=None)
def clouds(seed=0, nq=3000, nt=4000):
    """(Q, T) of about nq queries and nt targets, shuffled: uniform in the unit cube, a dense cluster, exact duplicates
    (within a cloud and across the two), exact ties (a query midway between two targets), a few far outliers with
    queries beside one of them, a few points with a NaN or an infinite coordinate."""
    rng = np.random.default_rng(seed)
    u = lambda n: rng.random((n, 3), dtype=F32)
    centre = np.array([0.3, 0.6, 0.5], F32)
    cluster = lambda n: (centre + F32(0.01) * rng.standard_normal((n, 3)).astype(F32)).astype(F32)
    far = np.array([[1000, 1000, 1000], [-50, 0.5, 0.5], [0.5, 60, -40], [0.2, 0.2, -30], [70, -70, 0.1], [0.5, 0.5, 90]], F32)
    bad = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan],
                    [np.inf, 0.1, np.nan], [0.3, 0.6, np.nan]], F32)
    e = 1.0 / 64                                                          # exact in float32, and within MAX_DIST
    ties_t = np.array([[0.5 - e, 0.25, -0.5], [0.5 + e, 0.25, -0.5], [0.5, 0.25, -0.5 - e], [0.5, 0.25, -0.5 + e],
                       [0.5, 0.25 + 2 * e, -0.5]], F32)
    ties_q = np.array([[0.5, 0.25, -0.5], [0.5, 0.25 + e, -0.5]], F32)    # four targets at one distance; one nearest
    t_main = np.concatenate([u(int(nt * 0.65)), cluster(int(nt * 0.3))])
    T = np.concatenate([t_main, t_main[rng.integers(0, len(t_main), nt // 30)], far, bad, ties_t])
    q_main = np.concatenate([u(int(nq * 0.68)), cluster(int(nq * 0.22))])
    beside = far[0] + F32(0.01) * rng.standard_normal((8, 3)).astype(F32)
    Q = np.concatenate([q_main, q_main[rng.integers(0, len(q_main), nq // 40)], t_main[rng.integers(0, len(t_main), nq // 15)],
                        far[1:] * F32(1.5), beside.astype(F32), bad[::-1], ties_q])
    return np.ascontiguousarray(Q[rng.permutation(len(Q))]), np.ascontiguousarray(T[rng.permutation(len(T))])


@functools.lru_cache(maxsize=None)
def restated(direction="data_to_ref", offset=0.0, taus=TAUS, max_dist=MAX_DIST, seed=0):
    """distances() of clouds(seed), each coordinate moved by `offset` in float32, in one direction; computed once."""
    Q, T = (c + F32(offset) for c in clouds(seed))
    return distances(Q, T, max_dist, taus) if direction == "data_to_ref" else distances(T, Q, max_dist, taus)


class Summary:
    """What capi.Fusion.cloud_distance returns, from the restatement (capi.CloudDistance's fields and properties)."""

    def __init__(self, words, max_dist, n_tau):
        self.n_query, self.n_valid, self.n_matched, self.sum_q = words[:4]
        self.max_dist = float(F32(max_dist))
        self.within = list(words[4:4 + n_tau])
        self.hist = np.array(words[12:], np.int64)

    @property
    def mean(self):
        return self.sum_q / (self.n_matched * (1048576.0 / self.max_dist)) if self.n_matched else 0.0

    @property
    def median_upper(self):
        if not self.n_matched:
            return 0.0
        b = int(np.searchsorted(np.cumsum(self.hist), (self.n_matched + 1) // 2))
        return (b + 1) * self.max_dist / 256.0


class RestatedDistanceFusion(rs.RestatedRenderFusion):
    """RestatedRenderFusion with capi.Fusion's set_reference_cloud / cloud_distance / distance_results computed by the
    restatement.  A distance result remembers the source result and the reference cloud it was measured on and is gone
    once either has been replaced or discarded."""

    def __init__(self, cams):
        super().__init__(cams)
        self.reference = None
        self._distance = None                      # (the source result, the reference cloud, d2, nearest)

    def set_reference_cloud(self, xyz):
        self.reference = xyz_of(xyz).copy()
        return len(self.reference)

    def _data(self, source):
        """(the result object that holds the data cloud, its positions)."""
        if source == "scene" and self.result is not None:
            return self.result, xyz_of(self.result[0])
        if source == "voxels" and self.voxels is not None:
            return self.voxels, xyz_of(self.voxels["points"])
        if source == "clean" and self.cleaned is not None:
            return self.cleaned, xyz_of(self.voxels["points"][self.cleaned["kept"]])
        if source == "visible" and self.visible is not None:
            return self.visible, xyz_of(self.visible["points"])
        if source == "mesh" and self.meshed is not None:
            return self.meshed, xyz_of(self.meshed["vertices"])
        raise ValueError("no such data result")

    def cloud_distance(self, source="scene", direction="data_to_ref", max_dist=1.0, thresholds=()):
        if source not in SOURCES or direction not in DIRECTIONS:
            raise ValueError("bad source or direction")
        held, data = self._data(source)
        if self.reference is None:
            raise ValueError("no reference cloud")
        q, t = (data, self.reference) if direction == "data_to_ref" else (self.reference, data)
        d2, nearest, words = distances(q, t, max_dist, thresholds)
        self._distance = (held, self.reference, d2, nearest)
        return Summary(words, max_dist, len(tuple(thresholds)))

    def _live(self):
        d = self._distance
        if d is None:
            return None
        now = {"scene": self.result, "voxels": self.voxels, "clean": self.cleaned, "visible": self.visible, "mesh": self.meshed}
        return d if d[1] is self.reference and any(d[0] is x for x in now.values()) else None

    def distance_results(self, first=0, n=None, squared=False):
        d = self._live()
        total = 0 if d is None else len(d[2])
        n = total - first if n is None else n
        if first < 0 or n < 0 or first + n > total:
            raise ValueError("range beyond the distance result")
        d2 = np.zeros(0, F32) if n == 0 else d[2][first:first + n].copy()
        nn = np.zeros(0, np.int32) if n == 0 else d[3][first:first + n].copy()
        return (d2 if squared else np.sqrt(d2)), nn
