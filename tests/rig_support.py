"""General camera rigs for the parity tests (no GPU): a small ray caster with arbitrary K (inverted as a full
3x3), R, C and SPHERE cx, cy, and the rigs that reach what acmmp/scene.py's two never do -- a posed reference, per-view
intrinsics with skew, rolled and turned sources, samples behind a source, a query point on a source's centre.
tests/test_rig_inputs.py checks without a GPU that each rig exercises what it claims; tests/test_gpu_rigs.py runs
them on the engine.  DESIGN.md "Camera rigs under test" says which rig reaches which statement.

Every rig is a scene.Scene with extra["gt_depths"], one rendered depth map per view (pinhole: z-depth, SPHERE:
radial distance; 0 where the view's ray misses the surface, which a pinhole view can).  The surfaces, the texture
and the quantisation are scene.py's: the slanted plane z = 5 + 0.15 x + 0.08 y for pinhole rigs, the box room
[-5, 5] x [-3, 3] x [-4, 4] for SPHERE rigs.  A pixel whose ray misses gets a fixed grey.
"""
import functools

import numpy as np

import fastmath_support as fs
import np_reference as npr
from acmmp import scene
from acmmp.types import PINHOLE, SPHERE, make_camera

GREY = 128.0
PLANE_N, PLANE_C = np.array([-0.15, -0.08, 1.0]), 5.0
ROOM_HALF = np.array([5.0, 3.0, 4.0])
# moved(): 2.1 rad about (1, 2, 3), and an offset two orders above the scene's own extent
MOVE_AXIS, MOVE_ANGLE, MOVE_OFFSET = (1.0, 2.0, 3.0), 2.1, (30.0, -40.0, 20.0)


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    A = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * A + (1 - np.cos(angle)) * (A @ A)


def roll(angle):
    """Rotation about the optical axis (applied on the camera side: R = roll(a) @ R_look)."""
    return rodrigues((0, 0, 1), angle)


# ---------------------------------------------------------------- the ray caster

def cast(kind, W, H, R, C, K=None, cxcy=None):
    """Rays of a W x H view (X_cam = R X_world + t, C = -R^T t) against the model's surface ->
    (depth (H, W): pinhole z-depth / SPHERE distance, 0 where missed; hit points (H, W, 3); hit mask)."""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    if kind == "pinhole":
        rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(np.asarray(K, np.float64).reshape(3, 3)).T
        d = rays @ R                                   # world direction = R^T ray_cam (row-vector form)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = scene._plane_hit(np.asarray(C, np.float64), d, PLANE_N, PLANE_C)
        hit = np.isfinite(t) & (t > 0)                 # rays[..., 2] == 1: t is the z-depth
    else:
        d = scene.sphere_dirs(W, H, cxcy[0], cxcy[1]) @ R
        t = scene._box_hit(np.asarray(C, np.float64), d, ROOM_HALF)
        hit = np.isfinite(t) & (t > 0)
    t = np.where(hit, t, 0.0)
    return t, np.asarray(C, np.float64) + t[..., None] * d, hit


def texture_band(kind, W):
    """scene.py's texture band: wavelengths of 6..30 pixels at the surface."""
    ppu = 0.8 * W / PLANE_C if kind == "pinhole" else W / (2 * np.pi * float(np.mean(ROOM_HALF)))
    return 2 * np.pi * ppu / 30.0, 2 * np.pi * ppu / 6.0


def build_rig(kind, W, H, views, seed, quantize=True, n_waves=48):
    """views: one dict per view with R (3, 3), C (3,), and K (3, 3) or cxcy; index 0 is the reference."""
    fmin, fmax = texture_band(kind, W)
    if kind == "pinhole":
        dmin, dmax = PLANE_C * 0.6, PLANE_C * 1.6
    else:
        dmin, dmax = 0.5 * float(np.min(ROOM_HALF)), 1.2 * float(np.linalg.norm(ROOM_HALF))
    imgs, cams, depths = [], [], []
    for v in views:
        R, C = np.asarray(v["R"], np.float64), np.asarray(v["C"], np.float64)
        t, P, hit = cast(kind, W, H, R, C, K=v.get("K"), cxcy=v.get("cxcy"))
        img = np.where(hit, scene._texture(P, seed, n_waves=n_waves, fmin=fmin, fmax=fmax), GREY)
        if quantize:
            img = np.round(img)
        imgs.append(img.astype(np.float32))
        depths.append(t.astype(np.float32))
        if kind == "pinhole":
            cams.append(make_camera(PINHOLE, K=v["K"], R=R, t=-R @ C, width=W, height=H, depth_min=dmin, depth_max=dmax))
        else:
            cams.append(make_camera(SPHERE, params=[W / (2 * np.pi), *v["cxcy"]], R=R, t=-R @ C, width=W, height=H,
                                    depth_min=dmin, depth_max=dmax))
    return scene.Scene(imgs, np.array(cams), depths[0], kind, {"gt_depths": depths})


def view_depths(sc):
    """Rendered depth of every view of a rig whose world frame is the surfaces' own (scene.py's rigs)."""
    H, W = sc.images[0].shape
    out = []
    for c in sc.cameras:
        R = c["R"].astype(np.float64).reshape(3, 3)
        C = -R.T @ c["t"].astype(np.float64)
        if sc.kind == "pinhole":
            t = cast("pinhole", W, H, R, C, K=c["K"].astype(np.float64))[0]
        else:
            t = cast("sphere", W, H, R, C, cxcy=(float(c["params"][1]), float(c["params"][2])))[0]
        out.append(t.astype(np.float32))
    return out


# ---------------------------------------------------------------- the rigs

def moved(base, G=None, g=None):
    """The same images seen from a moved world frame X' = G X + g: R' = R G^T, t' = t - R' g.  In exact arithmetic
    every projection, and so every cost, equals the base rig's."""
    G = rodrigues(MOVE_AXIS, MOVE_ANGLE) if G is None else np.asarray(G, np.float64)
    g = np.asarray(MOVE_OFFSET if g is None else g, np.float64)
    cams = base.cameras.copy()
    for k in range(len(cams)):
        R = base.cameras[k]["R"].astype(np.float64).reshape(3, 3) @ G.T
        cams[k]["R"] = R.astype(np.float32).reshape(9)
        cams[k]["t"] = (base.cameras[k]["t"].astype(np.float64) - R @ g).astype(np.float32)
    depths = base.extra["gt_depths"] if "gt_depths" in base.extra else view_depths(base)
    return scene.Scene(list(base.images), cams, base.gt_depth, base.kind, {"gt_depths": depths, "G": G, "g": g})


def _ring(n_src, seed, baseline, kind):
    """scene.py's source centres: a ring around the reference."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_src):
        ang = 2 * np.pi * k / n_src + rng.uniform(-0.2, 0.2)
        if kind == "pinhole":
            out.append(baseline * np.array([np.cos(ang), 0.5 * np.sin(ang), 0.0]))
        else:
            out.append(baseline * np.array([np.cos(ang), rng.uniform(-0.3, 0.3), np.sin(ang)]))
    return out


def _pin_K(W, H, fx=0.8, fy=0.8, cx=0.5, cy=0.5, skew=0.0, k3=0.0):
    """fx, fy in units of W; cx, cy in units of W, H; K[1] = skew fx, K[3] = k3 fy."""
    return np.array([[fx * W, skew * fx * W, cx * W], [k3 * fy * W, fy * W, cy * H], [0, 0, 1]], np.float64)


# per source, cycled: focal factors (+-15%), principal points, K[1] / fx, K[3] / fy
SRC_F = (1.15, 0.85, 1.0)
SRC_PP = ((0.55, 0.44), (0.47, 0.58), (0.52, 0.5))
SRC_SKEW = (0.04, -0.03, 0.0)
SRC_K3 = (0.0, 0.01, 0.0)
REF_K = dict(fx=0.8, fy=0.65, cx=0.42, cy=0.57)


def intrinsics(W, H, V=3, seed=0, quantize=True):
    """Pinhole: every view its own K.  The reference has fx != fy and an off-centre principal point but no skew
    (PixelToDir and Get3DPointonWorld_cu ignore K[1], ProjectonCamera_cu honours it: a skewed reference view is
    inconsistent in the reference itself); the sources have skew, and one a non-zero K[3]."""
    views = [dict(R=np.eye(3), C=np.zeros(3), K=_pin_K(W, H, **REF_K))]
    for k, C in enumerate(_ring(V, seed + 1000, 0.5, "pinhole")):
        f = SRC_F[k % 3]
        views.append(dict(R=scene._look_rotation(-0.5 * C[0] / PLANE_C, 0.5 * C[1] / PLANE_C), C=C,
                          K=_pin_K(W, H, fx=0.8 * f, fy=0.65 * f, cx=SRC_PP[k % 3][0], cy=SRC_PP[k % 3][1],
                                   skew=SRC_SKEW[k % 3], k3=SRC_K3[k % 3])))
    return build_rig("pinhole", W, H, views, seed, quantize)


ROLLS = (np.pi / 2, np.pi, -np.pi / 2)


def rolled(W, H, V=3, seed=0, quantize=True):
    """Pinhole: sources rolled +90, 180, -90 degrees about the optical axis, on a baseline of 1.5 at depth 5 with a
    0.25 rad convergent yaw: a strongly non-affine homography whose x and y rows swap and change sign."""
    K = _pin_K(W, H)
    views = [dict(R=np.eye(3), C=np.zeros(3), K=K)]
    for k, C in enumerate(_ring(V, seed + 1000, 1.5, "pinhole")):
        look = scene._look_rotation(-0.25 * C[0] / 1.5, 0.25 * C[1] / 1.5)
        views.append(dict(R=roll(ROLLS[k % 3]) @ look, C=C, K=K))
    return build_rig("pinhole", W, H, views, seed, quantize)


def behind(W, H, V=3, seed=0, quantize=True):
    """Pinhole: the first source's centre at z = 4 on the reference axis, looking along +z, so a hypothesis nearer
    than 4 puts its samples behind that source (tz <= 0); the other sources are scene.py's."""
    K = _pin_K(W, H)
    views = [dict(R=np.eye(3), C=np.zeros(3), K=K), dict(R=np.eye(3), C=np.array([0.0, 0.0, 4.0]), K=K)]
    for C in _ring(V - 1, seed + 1000, 0.5, "pinhole"):
        views.append(dict(R=scene._look_rotation(-0.5 * C[0] / PLANE_C, 0.5 * C[1] / PLANE_C), C=C, K=K))
    return build_rig("pinhole", W, H, views, seed, quantize)


TURNS = (scene._look_rotation(np.pi / 2, 0.0), scene._look_rotation(np.pi, 0.0),
         roll(np.pi / 4) @ scene._look_rotation(0.0, np.pi / 3))
TURN_PP = ((0.6, 0.45), (0.44, 0.53), (0.53, 0.41))
INTERP_TURNS = (0, 2)         # the two-source rig of the interpolation case: the 90 degree yaw and the pitched, rolled one


def turned(W, H, V=3, seed=0, quantize=True, n_waves=48, turns=None):
    """SPHERE: the reference's cx, cy off-centre; sources yawed 90 and 180 degrees, and one pitched 60 and rolled 45
    degrees, with off-centre cx, cy of their own: the sources' seams and poles cross the reference image's interior."""
    views = [dict(R=np.eye(3), C=np.zeros(3), cxcy=(0.37 * W, 0.55 * H))]
    assert turns is None or len(turns) == V
    for k, C in enumerate(_ring(V, seed + 2000, 0.35, "sphere")):
        i = (k if turns is None else turns[k]) % 3
        views.append(dict(R=TURNS[i], C=C, cxcy=(TURN_PP[i][0] * W, TURN_PP[i][1] * H)))
    return build_rig("sphere", W, H, views, seed, quantize, n_waves=n_waves)


DEGENERATE_C = np.array([0.0, 0.0, 2.0])


def degenerate(kind, W, H, seed=0, quantize=True):
    """Either model: the first source's centre at (0, 0, 2) of the reference's frame (R0 = I, t0 = 0, integer principal
    point), turned a little so that its t has three non-zero components; two ordinary sources beside it."""
    first = scene._look_rotation(0.11, -0.07)
    if kind == "pinhole":
        K = _pin_K(W, H)
        views = [dict(R=np.eye(3), C=np.zeros(3), K=K), dict(R=first, C=DEGENERATE_C, K=K)]
        for C in _ring(2, seed + 1000, 0.5, "pinhole"):
            views.append(dict(R=scene._look_rotation(-0.5 * C[0] / PLANE_C, 0.5 * C[1] / PLANE_C), C=C, K=K))
    else:
        pp = (W / 2.0, H / 2.0)
        views = [dict(R=np.eye(3), C=np.zeros(3), cxcy=pp), dict(R=first, C=DEGENERATE_C, cxcy=pp)]
        for C in _ring(2, seed + 2000, 0.35, "sphere"):
            views.append(dict(R=scene._look_rotation(0.03, -0.02), C=C, cxcy=pp))
    return build_rig(kind, W, H, views, seed, quantize)


def degenerate_queries(sc):
    """Queries on a degenerate() rig whose point lies on the first source's centre: (px (25,), py, planes (25, 8, 4)).
    The pixel (cx, cy) has the ray (0, 0, 1) exactly; plane 0, (0, 0, -1, 2), is z = 2, and planes 1..7 are tilted
    about the point (0, 0, 2), so every plane puts that pixel's point on the centre: depth = 2 n_z / n_z = 2 exactly
    in binary32, the reference-frame point is (0, 0, 2), and R (0, 0, 2) + t with t = -2 R[:, 2] rounded is 0 in
    every component (one fma of exact operands each).  Query 0 is that pixel (the patch CENTRE is degenerate: 6x6
    patches of increment 2 have no sample there); queries 1..24 are its neighbours at offsets {-3, -1, 1, 3} and
    {-5, 5} diagonal, of which one SAMPLE each is that pixel."""
    c0 = sc.cameras[0]
    if int(c0["model"]) == SPHERE:
        cx, cy = int(c0["params"][1]), int(c0["params"][2])
        assert (cx, cy) == (c0["params"][1], c0["params"][2])
    else:
        cx, cy = int(c0["K"][2]), int(c0["K"][5])
        assert (cx, cy) == (c0["K"][2], c0["K"][5])
    offs = [(0, 0)] + [(i, j) for i in (-3, -1, 1, 3) for j in (-3, -1, 1, 3)] + \
           [(-5, -5), (-5, 5), (5, -5), (5, 5), (5, 1), (-1, 5), (1, -5), (-5, 3)]
    px = np.array([cx + i for i, _ in offs], np.int32)
    py = np.array([cy + j for _, j in offs], np.int32)
    rng = np.random.default_rng(77)
    planes = np.zeros((len(px), fs.PLANES, 4), np.float32)
    for q in range(len(px)):
        for h in range(fs.PLANES):
            n = np.array([0.0, 0.0, -1.0]) + (rng.normal(0, 0.15, 3) if h else 0.0)
            n = (n / np.linalg.norm(n)).astype(np.float32)
            planes[q, h] = [n[0], n[1], n[2], np.float32(-2.0) * n[2]]
    return px, py, planes


# ---------------------------------------------------------------- the cases the tests run

SIZES = fs.MODELS                       # pinhole 96x64, SPHERE 128x64


def _base(kind, V, quantize):
    W, H = SIZES[kind]
    make = scene.pinhole_scene if kind == "pinhole" else scene.sphere_scene
    return make(W, H, n_src=V, seed=W + V, quantize=quantize)


# name -> (model, source views, texel format); V = 5 = a full chunk of 4 (k_init) / 2 (k_eval_nb) and a partial one
RIGS = {
    "pinhole-moved": ("pinhole", 3, "f16"), "pinhole-moved-fp32": ("pinhole", 3, "fp32"),
    "pinhole-intrinsics": ("pinhole", 3, "f16"), "pinhole-intrinsics-v5": ("pinhole", 5, "f16"),
    "pinhole-rolled": ("pinhole", 3, "f16"), "pinhole-behind": ("pinhole", 3, "f16"),
    "sphere-moved": ("sphere", 3, "f16"), "sphere-moved-fp32": ("sphere", 3, "fp32"),
    "sphere-turned": ("sphere", 3, "f16"), "sphere-turned-fp32": ("sphere", 3, "fp32"),
    "sphere-turned-v5": ("sphere", 5, "f16"),
}
DEGENERATE = {"pinhole-degenerate": "pinhole", "sphere-degenerate": "sphere"}


@functools.lru_cache(maxsize=None)
def make_rig(name):
    """-> (scene, params) of one entry of RIGS or DEGENERATE, or of "<model>-base" (scene.py's rig, V = 3)."""
    if name in DEGENERATE:
        sc = degenerate(DEGENERATE[name], *SIZES[DEGENERATE[name]], seed=11)
        return sc, fs.params_for(sc)
    if name.endswith("-base"):
        sc = _base(name.split("-")[0], 3, True)
        sc.extra["gt_depths"] = view_depths(sc)
        return sc, fs.params_for(sc)
    kind, V, tex = RIGS[name]
    W, H = SIZES[kind]
    q = fs.TEXELS[tex]
    what = name.split("-")[1]
    if what == "moved":
        sc = moved(_base(kind, V, q))
    else:
        sc = {"intrinsics": intrinsics, "rolled": rolled, "behind": behind, "turned": turned}[what](
            W, H, V=V, seed=W + V, quantize=q)
    return sc, fs.params_for(sc)


def rig_seed(name):
    """A moved rig takes the seed of its base case (fastmath_support.query_sets): the same pixels and planes."""
    if name.split("-")[1] in ("moved", "base"):
        kind, V, tex = RIGS[name] if name in RIGS else (name.split("-")[0], 3, "f16")
        return 1000 * V + (0 if kind == "pinhole" else 500) + (0 if fs.TEXELS[tex] else 250)
    return 7000 + 40 * sorted(list(RIGS) + list(DEGENERATE)).index(name)


@functools.lru_cache(maxsize=None)
def rig_sets(name):
    """The four query sets of a rig (fastmath_support.query_sets_for)."""
    sc, p = make_rig(name)
    return fs.query_sets_for(sc, p, rig_seed(name))


@functools.lru_cache(maxsize=None)
def rig_f64(name, set_name):
    sc, p = make_rig(name)
    if set_name == "degenerate":
        return fs.f64_costs_for(sc, p, *degenerate_queries(sc))
    return fs.f64_costs_for(sc, p, *rig_sets(name)[set_name])


_oracle_cache = {}


def rig_oracle(oracle_mod, name, set_name):
    """The oracle's costs of one set, (n, 8, V) float32, computed once per process."""
    if (name, set_name) not in _oracle_cache:
        sc, p = make_rig(name)
        q = degenerate_queries(sc) if set_name == "degenerate" else rig_sets(name)[set_name]
        out = fs.oracle_costs_for(oracle_mod, sc, p, *q)
        out.setflags(write=False)
        _oracle_cache[(name, set_name)] = out
    return _oracle_cache[(name, set_name)]


def surface_diagnostics(sc, p, margin):
    """f64_ncc's diagnostics of the ground-truth surface plane of every pixel at least `margin` pixels inside:
    (xs, ys, diag) -- what source_edge_pixels ranks."""
    rc = sc.cameras[0]
    H, W = sc.images[0].shape
    ys, xs = np.mgrid[margin:H - margin, margin:W - margin]
    xs, ys = xs.ravel(), ys.ravel()
    d = npr.pixel_to_dir(rc, xs, ys)
    depth = sc.gt_depth[ys, xs].astype(np.float64)
    planes = np.concatenate([-d, depth[:, None]], axis=1).astype(np.float32)
    return xs, ys, fs.f64_ncc(sc, p, xs, ys, planes, diagnostics=True)[1]


def sample_points(sc, p, px, py, planes):
    """Float64 world points of the patch samples of queries (Q,), planes (Q, 4): (Q, S, 3), by f64_ncc's statements."""
    rc = sc.cameras[0]
    pl = np.asarray(planes, np.float32).astype(np.float64)
    rays, ii, jj = fs.sample_rays(sc, p, np.asarray(px, np.int64), np.asarray(py, np.int64))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        den = np.einsum("qsc,qc->qs", rays, pl[:, :3])
        dn = np.where(np.abs(den) < 1e-6, 1e6, -pl[:, 3:4] / den)
        return npr.world_point(rc, np.asarray(px)[:, None] + ii[None], np.asarray(py)[:, None] + jj[None], dn)


def geom_depths(sc, seed):
    """Depth maps for the geometric-consistency probes: each view's rendered depth times a (0.97, 1.03) jitter, with
    a lattice of zeros in the first source's (src_depth == 0 -> 3, ACMMP.cu:658)."""
    rng = np.random.default_rng(seed)
    out = [(d * rng.uniform(0.97, 1.03, d.shape)).astype(np.float32) for d in sc.extra["gt_depths"]]
    out[1][::7, ::5] = 0.0
    return out


# ---------------------------------------------------------------- fast mode: the hooks of one query set

def fast_hook_costs(ctx, monkeypatch, px, py, planes, V, sphere, what):
    """The fast-mode hook-against-hook bit equalities of tests/test_gpu_fast_instances.py (b) on one query set
    (ctx in the fast mode, views uploaded) -> {hook: fast costs (n, planes, V)} of every hook that is not tied to
    debug_ncc bit for bit, which T1 then holds to float64.  SPHERE, and pinhole with ACMMP_PIN_HOMOG=0:
    debug_ncc_nb == debug_ncc and debug_ncc_ref == debug_ncc; the pinhole product path (the homogeneous loop) differs
    from debug_ncc somewhere, and its two hooks equal each other."""
    from conftest import assert_bitwise_equal
    n = len(px)
    fx, fy, fpl = fs.flat_queries(px, py, planes)
    ref5 = np.ascontiguousarray(planes[:, :5])
    f = ctx.debug_ncc(fx, fy, fpl).reshape(n, planes.shape[1], V)
    f_nb = ctx.debug_ncc_nb(px, py, planes)
    f_ref = ctx.debug_ncc_ref(px, py, ref5)
    out = {"debug_ncc": f}
    if sphere:
        assert_bitwise_equal(f_nb, f, f"{what}: fast debug_ncc_nb vs debug_ncc")
        assert_bitwise_equal(f_ref, f[:, :5], f"{what}: fast debug_ncc_ref vs debug_ncc")
    else:
        monkeypatch.setenv("ACMMP_PIN_HOMOG", "0")
        ps_nb = ctx.debug_ncc_nb(px, py, planes)
        ps_ref = ctx.debug_ncc_ref(px, py, ref5)
        monkeypatch.delenv("ACMMP_PIN_HOMOG")
        assert_bitwise_equal(ps_nb, f, f"{what}: fast per-sample debug_ncc_nb vs debug_ncc")
        assert_bitwise_equal(ps_ref, f[:, :5], f"{what}: fast per-sample debug_ncc_ref vs debug_ncc")
        assert np.any(f_nb.view(np.uint32) != ps_nb.view(np.uint32)), what      # the homogeneous loop ran
        assert_bitwise_equal(f_ref, f_nb[:, :5], f"{what}: fast homogeneous debug_ncc_ref vs debug_ncc_nb")
        out["debug_ncc_nb_homog"] = f_nb
        out["debug_ncc_ref_homog"] = f_ref
    return out

