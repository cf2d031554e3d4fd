"""Binary32 restatement of the kept-sample word k_init publishes (KParams::keep): bit s of a
pixel's word is `w_s <= tau * sbw` with the kernels' own arithmetic --

  spatial table (k_spatial):  lat = -(y - cy) / H * pi_f;  scale_x = (2 pi_f / W) * det_cos(lat);  scale_y = pi_f / H;
                              sig = sigma_spatial * (pi_f / H);  sp_s = -sqrt(fma(dy, dy, dx * dx)) / (2 sig sig)
  weight (patch_sample):      w_s = det_exp(sp_s - |r_s - centre| / (2 sigma_color^2)), r the clamped fp32 reference texel
  sum (patch_sums):           sbw = ((w_0 + w_1) + ...) + w_35, one binary32 addition per sample, in sample order

every operation rounded to binary32 as the kernels' (compiled without contraction, so only the written fma fuses).
det_exp and det_cos are the CPU oracle's (oracle.detmath), which tests/test_detmath.py holds to the device functions bit
for bit.  The one fma is evaluated exactly in rational arithmetic and rounded once to binary32 (fma32).
A pixel whose sum is below 1e-6 is dead: its loop does not run and its word is 0."""
import numpy as np

from fractions import Fraction

f32 = np.float32
PI_F = f32(3.141592654)


def fma32(a, b, c):
    """fma(a, b, c) of binary32 arrays: the exact a * b + c rounded once, half to even, to binary32 (results here are
    normal numbers or zero)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    out = np.empty(a.shape, f32)
    memo = {}
    for k, (x, y, z) in enumerate(zip(a.ravel().tolist(), b.ravel().tolist(), c.ravel().tolist())):
        r = memo.get((x, y, z))
        if r is None:
            v = Fraction(x) * Fraction(y) + Fraction(z)
            if v == 0:
                r = 0.0
            else:
                sign, v = (-1.0, -v) if v < 0 else (1.0, v)
                e = v.numerator.bit_length() - v.denominator.bit_length()
                if Fraction(2) ** e > v:
                    e -= 1                                  # 2^e <= v < 2^(e+1)
                assert -126 <= e <= 127
                n = round(v / Fraction(2) ** (e - 23))      # int(Fraction) rounding: half to even
                r = sign * float(n) * 2.0 ** (e - 23)       # n <= 2^24: exact
            memo[(x, y, z)] = r
        out.ravel()[k] = r
    return out


def words(oracle, images, cams, params, px, py, tau):
    """-> (words uint64[n], live bool[n]) of the pixels (px, py), binary32 as the kernels."""
    rc, ref = cams[0], np.asarray(images[0], np.float32)
    H, W = ref.shape
    R, inc = int(params["patch_size"]) // 2, int(params["radius_increment"])
    offs = np.arange(-R, R + 1, inc)
    ii, jj = (a.ravel() for a in np.meshgrid(offs, offs, indexing="ij"))    # s = (i index) * nside + (j index)
    assert ii.size == 36
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    cy = f32(rc["params"][2])
    lat = (-(py.astype(f32) - cy)) / f32(H) * PI_F
    scale_x = (f32(2.0) * PI_F / f32(W)) * oracle.detmath("cos", lat.astype(f32))
    scale_y = PI_F / f32(H)
    sig = f32(params["sigma_spatial"]) * (PI_F / f32(H))
    den = f32(2.0) * sig * sig
    dx = ii.astype(f32)[None, :] * scale_x[:, None]
    dy = (jj.astype(f32) * scale_y)[None, :] * np.ones_like(dx)
    dxx = (dx * dx).astype(f32)
    fused = fma32(dy, dy, dxx)
    sp = (-np.sqrt(fused).astype(f32)) / den
    r = ref[np.clip(py[:, None] + jj[None, :], 0, H - 1), np.clip(px[:, None] + ii[None, :], 0, W - 1)]
    centre = ref[py, px]
    color_den = f32(2.0) * f32(params["sigma_color"]) * f32(params["sigma_color"])
    arg = (sp - (np.abs(r - centre[:, None]).astype(f32) / color_den).astype(f32)).astype(f32)
    w = oracle.detmath("exp", arg).reshape(arg.shape)
    sbw = np.zeros(len(px), f32)
    for s in range(36):
        sbw = (sbw + w[:, s]).astype(f32)
    live = ~(sbw < f32(1e-6))
    lim = (f32(tau) * sbw).astype(f32)
    drop = (w <= lim[:, None]) & live[:, None]
    out = np.zeros(len(px), np.uint64)
    for s in range(36):
        out |= drop[:, s].astype(np.uint64) << np.uint64(s)
    return out, live
