"""Inputs of the geometry tests (tests/test_geometry_host.py, tests/test_geometry_direct_gpu.py): numpy only, seeded.

Clouds straddle the 256-point workgroup (cap 1, 255, 256, 257, 300, 1000), come as one frame or three, with 3, 4 or 6 columns,
and are spread beyond the range on every side and behind the camera, so that each filter rejects a real share.  Columns past xyz
hold values that name their (frame, row, column).  A per-frame ``n_in`` leaves rows at and beyond ``n_in[f]`` that WOULD pass
both filters of both random calibrations: a kernel that reads them keeps too much.

Calibrations: the KITTI one of the oracle; a generic one (a rotation about all three axes, other focal lengths, another image
size); and a dyadic one in which every product and quotient is exact in f32 whatever the order of operations, on which the edge
rows (``edges``) are placed exactly."""
import collections
import functools

import numpy as np

import mvx_oracle as O

RANGE = tuple(O.VELORANGE)                                  # 0, -40, -3, 70.4, 40, 1: hi x = 70.4 is no f32
SPREAD = (5.0, 5.0, 2.0)                                    # metres beyond the range on every side

FRAC_WH = (16.0000004, 370.00001)
Calib = collections.namedtuple('Calib', 'name m p2 imsize_wh')                   # m = R0_rect @ Tr_velo_to_cam (f64), P2 (f64)
Cloud = collections.namedtuple('Cloud', 'name pcd n_in cap F ncol')              # pcd f32 (F, cap, ncol); n_in i32 (F,) or None


def _rot(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return rz @ ry @ rx


@functools.lru_cache(None)
def calib(name):
    if name == 'kitti':
        c = O.KITTI_CALIB
        return Calib(name, c['R0_rect'] @ c['Tr_velo_to_cam'], c['P2'].copy(), (1224.0, 370.0))
    if name == 'generic':
        # camera axes (x right, y down, z forward) from lidar axes (x forward, y left, z up), then turned about all three
        axes = np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]])
        m = np.eye(4)
        m[:3, :3] = _rot(0.11, -0.07, 0.05) @ axes
        m[:3, 3] = (0.06, -0.11, -0.31)
        p2 = np.array([[503.7, 0.0, 331.2, 31.4], [0.0, 518.9, 247.6, 0.53], [0.0, 0.0, 1.0, 0.0031], [0.0, 0.0, 0.0, 1.0]])
        return Calib(name, m, p2, (640.0, 480.0))
    if name in ('dyadic', 'dyadic_frac'):
        # cam x = -y, cam y = -z, cam z = x; focal lengths 2 and 4, zero principal point, and P2[2][3] = 1: the divisor is depth + 1,
        # which is 2 at depth 1 (u = -y, v = -2 z, all exact) and 1 ON the camera plane, where (u, v) therefore stay finite and
        # inside the image and `z > 0` alone rejects the point.  Image 16 x 370: see `edges`.
        m = np.array([[0.0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0], [0, 0, 0, 1]])
        p2 = np.array([[2.0, 0, 0, 0], [0, 4.0, 0, 0], [0, 0, 1, 1], [0, 0, 0, 1]])
        # 'dyadic_frac': image sizes that are no f32 values and round to 16 and 370.  The f32 limits stay what they are, f32(w) -
        # 1e-3f, while w - 1e-3 formed in f64 and THEN rounded to f32 lands one step above them; for every integer size up to
        # 2048 the two coincide, so only such a size tells in which type the f32 limit was formed.
        return Calib(name, m, p2, (16.0, 370.0) if name == 'dyadic' else FRAC_WH)
    raise KeyError(name)


def f32_formed(c):
    """The pairing FrameBatch.prepared() builds for the projection: the matrix product formed in f32, P2 rounded to f32."""
    k = O.KITTI_CALIB
    assert c.name == 'kitti'
    m32 = (k['R0_rect'].astype(np.float32) @ k['Tr_velo_to_cam'].astype(np.float32)).astype(np.float64)
    return Calib('kitti_f32', m32, c.p2.astype(np.float32).astype(np.float64), c.imsize_wh)


# a point in front of both random cameras, well inside both images and the range: the filler of rows at and beyond n_in[f]
def _passing(g, n):
    return np.stack([g.uniform(15, 40, n), g.uniform(-2, 2, n), g.uniform(-1.5, 0.0, n)], 1)


CLOUDS = (
    # name       cap  F  ncol  n_in
    ('one',        1, 3, 3, None),                   # three frames of one point: kept; outside the image; beyond the range
    ('c255',     255, 1, 4, None),
    ('c256',     256, 1, 6, None),
    ('c257',     257, 3, 4, (257, 400, 100)),        # a last block of one point; one entry above cap, which the kernels clamp
    ('c300',     300, 3, 3, (300, 0, 137)),          # an empty frame in the middle
    ('c1000',   1000, 3, 6, (1000, 0, 137)),
    ('c1000one', 1000, 1, 4, None),
)
CLOUD_NAMES = tuple(c[0] for c in CLOUDS)


@functools.lru_cache(None)
def cloud(name):
    _, cap, F, ncol, n_in = CLOUDS[CLOUD_NAMES.index(name)]
    g = np.random.default_rng(700 + CLOUD_NAMES.index(name))
    lo, hi = np.array(RANGE[:3]) - SPREAD, np.array(RANGE[3:]) + SPREAD
    pcd = np.empty((F, cap, ncol), np.float64)
    pcd[..., :3] = lo + g.random((F, cap, 3)) * (hi - lo)
    if name == 'one':
        pcd[:, 0, :3] = [(20.0, 1.0, -1.0), (5.0, 30.0, -1.0), (75.0, 0.0, -1.0)]
    if n_in is not None:
        for f, n in enumerate(n_in):
            if n < cap:
                pcd[f, n:, :3] = _passing(g, cap - n)
    f_, r_, c_ = np.meshgrid(np.arange(F), np.arange(cap), np.arange(ncol), indexing='ij')
    tag = 1000.0 * (f_ + 1) + r_ + c_ / 8.0                                   # exact in f32, distinct per (frame, row, column)
    pcd[..., 3:] = tag[..., 3:]
    pcd = pcd.astype(np.float32)
    pcd.setflags(write=False)
    return Cloud(name, pcd, None if n_in is None else np.array(n_in, np.int32), cap, F, ncol)


def live(c, f):
    """Rows of frame f that the kernels read: n_in[f] clamped to cap."""
    return c.cap if c.n_in is None else min(int(c.n_in[f]), c.cap)


# ---- edge rows under the dyadic calibration -----------------------------------------------------------------------------------
# Image 16 x 370: f32(16) - 1e-3f lies 4.0e-7 BELOW 16 - 1e-3 and f32(370) - 1e-3f 7.1e-6 below 370 - 1e-3, so u = the f32 limit
# is dropped by the f32 arithmetic (u < lim is strict) and kept by the f64 one.  Range: hi x = 70.2 and lo y = -39.9 are no f32
# values and their f32 roundings lie BELOW them, so x = f32(70.2) passes `x < hi` only with the f64 bound, and y = f32(-39.9)
# passes `lo <= y` only with the f32 bound.
EDGE_RANGE = (0.0, -39.9, -3.0, 70.2, 40.0, 1.0)
_f = np.float32
STEP = float(np.finfo(np.float32).smallest_subnormal)       # the smallest positive f32
LIM_W32, LIM_H32 = _f(16) - _f(1e-3), _f(370) - _f(1e-3)

Edge = collections.namedtuple('Edge', 'name xyz filt keep_f32 keep_f64 quantity margin')
# filt: 's' = sight only (math_f32 1 / 0 -> keep_f32 / keep_f64), 'r' = range only (bounds_f32 1 / 0 -> keep_f32 / keep_f64).
# quantity: the sight_margin column, or None for the range margin.  margin: the distance from the limit in (a) per arithmetic,
# (f32, f64): a number = exactly that (0, or one step of the coordinate times the exact scale: v = -2 z moves in steps of two),
# 'ulp' = exactly one f32 step at the limit's magnitude, 'sub' = positive and below one such step (the f32 and f64 limits differ
# by less than that), None = not stated.
_below = lambda v: np.nextafter(_f(v), _f(-np.inf))
_above = lambda v: np.nextafter(_f(v), _f(np.inf))
U_AT, U_DN, U_UP = LIM_W32, _below(LIM_W32), _above(LIM_W32)          # u = -y: the f32 limit, one f32 below it, one above
V_AT, V_DN, V_UP = LIM_H32, _below(LIM_H32), _above(LIM_H32)          # v = -2 z
EDGES = (
    #     name                 x                    y                      z                filter  f32    f64   quantity, margin
    Edge('inside',            (1.0,                 -1.0,                  -1.0),             's', True,  True,  None, None),
    Edge('z == 0',            (0.0,                 -1.0,                  -1.0),             's', False, False, 0, (0.0, 0.0)),
    Edge('z one step',        (STEP,                -1.0,                  -1.0),             's', True,  True,  0, (STEP, STEP)),
    Edge('u == 0',            (1.0,                 0.0,                   -1.0),             's', True,  True,  1, (0.0, 0.0)),
    Edge('u one step below',  (1.0,                 STEP,                  -1.0),             's', False, False, 1, (STEP, STEP)),
    Edge('v == 0',            (1.0,                 -1.0,                  0.0),              's', True,  True,  2, (0.0, 0.0)),
    Edge('v one step below',  (1.0,                 -1.0,                  STEP),             's', False, False, 2, (2 * STEP, 2 * STEP)),
    Edge('u == lim32',        (1.0,                 -U_AT,                 -1.0),             's', False, True,  3, (0.0, 'sub')),
    Edge('u below lim32',     (1.0,                 -U_DN,                 -1.0),             's', True,  True,  3, ('ulp', None)),
    Edge('u above lim64',     (1.0,                 -U_UP,                 -1.0),             's', False, False, 3, (None, 'sub')),
    Edge('v == lim32',        (1.0,                 -1.0,                  -V_AT / _f(2)),    's', False, True,  4, (0.0, 'sub')),
    Edge('v below lim32',     (1.0,                 -1.0,                  -V_DN / _f(2)),    's', True,  True,  4, ('ulp', None)),
    Edge('v above lim64',     (1.0,                 -1.0,                  -V_UP / _f(2)),    's', False, False, 4, (None, 'sub')),
    Edge('x == lo',           (0.0,                 1.0,                   -1.0),             'r', True,  True,  None, (0.0, 0.0)),
    Edge('y == hi',           (1.0,                 40.0,                  -1.0),             'r', False, False, None, (0.0, 0.0)),
    Edge('z == lo',           (1.0,                 1.0,                   -3.0),             'r', True,  True,  None, (0.0, 0.0)),
    Edge('z == hi',           (1.0,                 1.0,                   1.0),              'r', False, False, None, (0.0, 0.0)),
    Edge('y below hi',        (1.0,                 _below(40.0),          -1.0),             'r', True,  True,  None, ('ulp', 'ulp')),
    Edge('x == f32(hi)',      (_f(70.2),            1.0,                   -1.0),             'r', False, True,  None, (0.0, 'sub')),
    Edge('y == f32(lo)',      (1.0,                 _f(-39.9),             -1.0),             'r', True,  False, None, (0.0, 'sub')),
    Edge('nan x',             (np.nan,              -1.0,                  -1.0),             'sr', False, False, None, None),
    Edge('nan y',             (1.0,                 np.nan,                -1.0),             'sr', False, False, None, None),
    Edge('nan z',             (1.0,                 -1.0,                  np.nan),           'sr', False, False, None, None),
    Edge('+inf x',            (np.inf,              -1.0,                  -1.0),             'sr', False, False, None, None),
    Edge('-inf y',            (1.0,                 -np.inf,               -1.0),             'sr', False, False, None, None),
    Edge('+inf z',            (1.0,                 -1.0,                  np.inf),           'sr', False, False, None, None),
)


@functools.lru_cache(None)
def edges(ncol=4):
    """The edge rows as one frame of a cloud, f32 (1, len(EDGES), ncol); columns past xyz as in `cloud`."""
    pcd = np.zeros((1, len(EDGES), ncol), np.float32)
    pcd[0, :, :3] = np.array([[_f(v) for v in e.xyz] for e in EDGES], np.float32)
    for c in range(3, ncol):
        pcd[0, :, c] = 1000.0 + np.arange(len(EDGES)) + c / 8.0
    pcd.setflags(write=False)
    return Cloud('edges', pcd, None, len(EDGES), 1, ncol)
