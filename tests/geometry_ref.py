"""Two references of csrc/geometry.hip (range crop, frustum crop, lidar -> image projection): numpy only.

(a) ``exact``: the plain statement in ``numpy.longdouble`` (80-bit, eps 1.1e-19).  Camera depth = row 2 of M . p, and
    (u, v) = (row 0, row 1) / row 2 of (P2 . M) . p, formed as ONE 4x4 . 4x4 product applied to the point, then the divide; no
    attention to the order of operations.  Besides the decisions it returns, per point, the *margins*: the distance of z, u, v,
    lim_w - u and lim_h - v from zero, and the distance of every coordinate from its two range bounds.

(b) ``project`` / ``keep``: the kernel's own order in the working type T (f32 or f64), every numpy operation on arrays of dtype T
    being one correctly rounded IEEE operation, none of them fused:

        cam_i = ((m_i0 x + m_i1 y) + (m_i2 z + m_i3))          i = 0..3, matrices cast to T first
        img_j = ((p_j0 cam_0 + p_j1 cam_1) + (p_j2 cam_2 + p_j3 cam_3))      j = 0..2
        z = cam_2, u = img_0 / img_2, v = img_1 / img_2
        keep  = z > 0 and u >= 0 and v >= 0 and u < lim_w and v < lim_h,   lim = T(size) - T(1e-3), as fill_params forms it
        range = lo <= f64(x) < hi per axis, the bounds rounded through f32 when bounds_f32 is set

    The library is built with -ffp-contract=off and divides with correct rounding, so the kernels are expected to equal (b) bit
    for bit.  Both layers read the SAME matrices: the caller hands (a) the matrices already rounded to T (``as_type``), rounding
    a matrix being a change of the input, not an error of the arithmetic.

The bound that ties (b) to (a) (``bounds``), with u_T the unit roundoff of T (2^-24, 2^-53) and g3 = 3 u_T / (1 - 3 u_T):

  1. cam_i is a sum of four terms, each of which passes through at most three roundings (its product, two additions; the bare
     m_i3 through two).  Standard forward analysis:  |cam_i^ - cam_i| <= g3 A_i,  A_i = |m_i0 x| + |m_i1 y| + |m_i2 z| + |m_i3|.
     This is the bound of z (i = 2).
  2. img_j^ is the same kind of sum over the COMPUTED cam_k^: its own rounding is at most g3 sum_k |p_jk| |cam_k^| and the
     inherited error at most sum_k |p_jk| g3 A_k.  With |cam_k^| <= (1 + g3) A_k:
         |img_j^ - img_j| <= (2 g3 + g3^2) B_j =: E_j,   B_j = sum_k |p_jk| A_k.
  3. q^ = fl(a^ / b^) with |a^ - a| <= E_a, |b^ - b| <= E_b < |b|, q = a / b:
         a^/b^ - a/b = ((a^ - a) b - a (b^ - b)) / (b b^)   =>   |a^/b^ - q| <= (E_a + |q| E_b) / (|b| - E_b) =: d
     and the division rounds once: |q^ - q| <= d + u_T (|q| + d) + the smallest subnormal of T.  Where E_b >= |b| the quotient
     is not bounded at all (bound = inf): such a point can only be decided by its depth.
  (a) itself carries 80-bit rounding: 32 eps_ld B_j is added to E_j and 32 eps_ld A_2 to the bound of z (eleven orders
  below the f32 terms, two below the f64 ones).

A decision of (a) is *sure* when the quantity it rests on lies farther from its limit than the bound: a point is surely out when
one test surely fails, surely in when every test surely passes, and *undecided* otherwise (``sure``).  The range test compares
f32 values promoted to f64 with f64 bounds and rounds nothing, so its bound is zero and (a) and (b) agree on every point."""
import collections

import numpy as np

LD = np.longdouble

Exact = collections.namedtuple('Exact', 'range_mask range_margin z u v w sight_mask sight_margin A B')
# sight_margin columns, and the bound that belongs to each
Z, U0, V0, UW, VH = range(5)
MARGIN_NAMES = ('z > 0', 'u >= 0', 'v >= 0', 'u < lim_w', 'v < lim_h')


def unit_roundoff(T):
    return float(np.finfo(T).eps) / 2


def as_type(mat, T):
    """The matrix as the kernel reads it under arithmetic T: rounded to T, handed on as f64 values."""
    return np.asarray(mat, np.float64).astype(T).astype(np.float64)


def limits(imsize_wh, math_f32):
    """(lim_w, lim_h) as fill_params forms them: f32(w) - 1e-3f in f32, or w - 1e-3 in f64; returned as f64 values."""
    if math_f32:
        return tuple(float(np.float32(s) - np.float32(1e-3)) for s in imsize_wh)
    return tuple(float(np.float64(s) - np.float64(1e-3)) for s in imsize_wh)


def bounds6(range6, bounds_f32):
    r = np.asarray(range6, np.float64)
    return r.astype(np.float32).astype(np.float64) if bounds_f32 else r


# ---- (a) --------------------------------------------------------------------------------------------------------------------------
def exact(xyz, m=None, p2=None, lims=None, range6=None):
    """xyz f32 (n, 3).  m, p2: 4x4 (the values the kernel reads), lims = limits(...); range6: the six bounds the kernel compares
    with (bounds6(...)).  Parts whose arguments are None come back as None.  Non-finite points fail every test of both filters
    (margin nan)."""
    xyz = np.asarray(xyz, np.float32)
    n = xyz.shape[0]
    p = xyz.astype(LD)
    out = dict.fromkeys(Exact._fields)
    finite = np.isfinite(xyz).all(1)
    with np.errstate(all='ignore'):
        if range6 is not None:
            lo, hi = np.asarray(range6[:3], np.float64).astype(LD), np.asarray(range6[3:], np.float64).astype(LD)
            out['range_mask'] = np.all((lo <= p) & (p < hi), axis=1) & finite
            out['range_margin'] = np.where(finite, np.minimum(np.abs(p - lo), np.abs(p - hi)).min(1), np.nan)
        if m is not None:
            M, P = np.asarray(m, np.float64).astype(LD), np.asarray(p2, np.float64).astype(LD)
            h = np.concatenate([p, np.ones((n, 1), LD)], 1)                 # (n, 4)
            z = h @ M[2]
            img = h @ (P @ M).T
            u, v = img[:, 0] / img[:, 2], img[:, 1] / img[:, 2]
            lw, lh = LD(lims[0]), LD(lims[1])
            out['z'], out['u'], out['v'], out['w'] = z, u, v, img[:, 2]
            out['sight_mask'] = (z > 0) & (u >= 0) & (v >= 0) & (u < lw) & (v < lh) & finite
            mg = np.stack([np.abs(z), np.abs(u), np.abs(v), np.abs(lw - u), np.abs(lh - v)], 1)
            out['sight_margin'] = np.where(finite[:, None], mg, np.nan)
            A = np.abs(h[:, None, :] * M[None]).sum(2)                      # (n, 4): A_i
            out['A'], out['B'] = A, A @ np.abs(P).T                         # (n, 4): B_j
    return Exact(**out)


def bounds(ex, T):
    """(bz, bu, bv): per-point bounds of |(b) - (a)| under arithmetic T from the magnitudes (a) recorded (module docstring, steps
    1 to 3); longdouble arrays, inf where the divisor is not bounded away from zero."""
    uT = LD(unit_roundoff(T))
    g3 = 3 * uT / (1 - 3 * uT)
    eld = LD(np.finfo(LD).eps)
    tiny = LD(np.finfo(T).smallest_subnormal)
    with np.errstate(all='ignore'):
        bz = (g3 + 32 * eld) * ex.A[:, 2]
        E = (2 * g3 + g3 * g3 + 32 * eld) * ex.B
        den = np.abs(ex.w) - E[:, 2]
        res = []
        for q, Ea in ((ex.u, E[:, 0]), (ex.v, E[:, 1])):
            d = (Ea + np.abs(q) * E[:, 2]) / den
            b = d + uT * (np.abs(q) + d) + tiny
            res.append(np.where((den > 0) & np.isfinite(b), b, np.inf))
    return bz, res[0], res[1]


def sure(ex, bz, bu, bv, lims):
    """(surely in, surely out) of the sight filter; everything else is undecided between the layers."""
    with np.errstate(all='ignore'):
        b = np.stack([bz, bu, bv, bu, bv], 1)
        lw, lh = LD(lims[0]), LD(lims[1])
        passes = np.stack([ex.z > 0, ex.u >= 0, ex.v >= 0, ex.u < lw, ex.v < lh], 1)
        clear = ex.sight_margin > b                                          # nan margins (non-finite points) are never clear
        bad = np.isnan(ex.sight_margin).all(1)                               # non-finite points: out in both layers
        sure_in = (passes & clear).all(1)
        sure_out = (~passes & clear).any(1) | bad
    return sure_in, sure_out


# ---- (b) --------------------------------------------------------------------------------------------------------------------------
def project(xyz, m, p2, T):
    """(z, u, v) arrays of dtype T in the order of project<T>."""
    xyz = np.asarray(xyz, np.float32)
    m, p2 = np.asarray(m, np.float64).astype(T), np.asarray(p2, np.float64).astype(T)
    x, y, z = (xyz[:, a].astype(T) for a in range(3))
    with np.errstate(all='ignore'):
        cam = [((m[i, 0] * x + m[i, 1] * y) + (m[i, 2] * z + m[i, 3])).astype(T) for i in range(4)]
        img = [((p2[j, 0] * cam[0] + p2[j, 1] * cam[1]) + (p2[j, 2] * cam[2] + p2[j, 3] * cam[3])).astype(T) for j in range(3)]
        res = cam[2], img[0] / img[2], img[1] / img[2]
    assert all(r.dtype == T for r in res)
    return res


def range_keep(xyz, range6, bounds_f32):
    r = bounds6(range6, bounds_f32)
    v = np.asarray(xyz, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore'):
        return np.all((r[:3] <= v) & (v < r[3:]), axis=1)


def sight_keep(xyz, m, p2, imsize_wh, math_f32):
    T = np.float32 if math_f32 else np.float64
    z, u, v = project(xyz, m, p2, T)
    lw, lh = (T(s) for s in limits(imsize_wh, math_f32))
    with np.errstate(invalid='ignore'):
        return (z > T(0)) & (u >= T(0)) & (v >= T(0)) & (u < lw) & (v < lh)


def keep(xyz, range6=None, bounds_f32=0, m=None, p2=None, imsize_wh=None, math_f32=0):
    """keep_point of every row."""
    ok = np.ones(len(xyz), bool)
    if range6 is not None:
        ok &= range_keep(xyz, range6, bounds_f32)
    if m is not None:
        ok &= sight_keep(xyz, m, p2, imsize_wh, math_f32)
    return ok


def lidar2img(xyz, m, p2, math_f32, swap_rc):
    """What mvx_lidar2img stores: (two columns f32 (n, 2), cam_z f32 (n,)); the f64 arithmetic returns through f32."""
    z, u, v = project(xyz, m, p2, np.float32 if math_f32 else np.float64)
    with np.errstate(all='ignore'):
        z, u, v = z.astype(np.float32), u.astype(np.float32), v.astype(np.float32)
    return (np.stack([v, u], 1) if swap_rc else np.stack([u, v], 1)), z
