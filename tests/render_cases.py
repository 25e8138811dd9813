"""Seeded inputs of the render tests (numpy only): the BEV and the camera case of tests/test_render_gpu.py, whose boxes are
built by rejection so that every pre-floor endpoint coordinate (tests/render_ref.py) is at least MARGIN px away from an
integer -- cos and sin may differ in the last bit between the GPU and numpy, and a coordinate that close to a pixel boundary
could land on either side.  tests/test_render_host.py checks on the CPU that the generators reach their box counts."""
import math

import numpy as np

import render_ref as R

MARGIN = 1e-6
MAX_TRIES = 64


def word(prio, rgb):
    return (int(prio) << 24) | (int(rgb[0]) << 16) | (int(rgb[1]) << 8) | int(rgb[2])


def as_i32(words):
    """u32 words -> the int32 array the library's wrappers carry them in."""
    return np.asarray(words, dtype=np.uint32).view(np.int32)


def margin_ok(segments):
    """Every coordinate of ((a0, a1), (b0, b1)) segments at least MARGIN from an integer (all of them finite)."""
    for seg in segments:
        for end in seg:
            for v in end:
                if not math.isfinite(v) or abs(v - round(v)) < MARGIN:
                    return False
    return True


def rejection(rng, draw, endpoints_of):
    """The first of at most MAX_TRIES draws whose endpoints keep the margin; returns (box f32 (7,), tries)."""
    for t in range(1, MAX_TRIES + 1):
        box = np.asarray(draw(rng), dtype=np.float32)
        if margin_ok(endpoints_of(box)):
            return box, t
    raise AssertionError('no box with a %g px margin in %d draws' % (MARGIN, MAX_TRIES))


# ---- BEV: 37 x 45 at 0.5 m, F = 3, n_points = (0, 1, 300), cap 320, n_boxes = (0, 1, 7) ------------------------------------
BEV = dict(H=37, W=45, res=0.5, x0=0.0, y0=-11.25, z0=-3.0, z1=1.0, cmax=8, cap=320, n_points=(0, 1, 300), bcap=9, n_boxes=(0, 1, 7))
SATURATED_CELL = (10, 25)          # (i, j) of the 40 points in one pixel
TIE_CELL = (20, 30)                # equal z, different r
ORDER_CELL = (22, 31)              # the higher point has the smaller r: z decides before r


def bev_case(seed=0):
    g = np.random.default_rng(seed)
    c = dict(BEV)
    F, cap, H, W, res = 3, c['cap'], c['H'], c['W'], c['res']
    lo = np.array([c['x0'] - 1.0, c['y0'] - 1.0, c['z0'] - 0.5, -0.2])
    hi = np.array([c['x0'] + H * res + 1.0, c['y0'] + W * res + 1.0, c['z1'] + 0.5, 1.2])
    pts = np.zeros((F, cap, 6), np.float32)
    pts[..., :4] = g.uniform(lo, hi, (F, cap, 4))              # rows behind n_points are valid points that must not be drawn
    pts[..., 4:] = g.uniform(0, 30, (F, cap, 2))
    p = pts[2]
    p[0, :3] = (c['x0'], c['y0'], 0.0)                                          # exactly on the lower bounds: drawn
    p[1, :3] = (c['x0'] + H * res, 0.0, 0.0)                                    # on the upper bound of x: not drawn
    p[2, :3] = (1.0, c['y0'] + W * res, 0.0)                                    # on the upper bound of y: not drawn
    p[3, 0], p[4, 1], p[5, 2], p[6, 0], p[7, 3] = np.nan, np.inf, np.nan, -np.inf, np.nan
    i, j = SATURATED_CELL
    p[10:50, 0] = c['x0'] + (i + g.uniform(0.1, 0.9, 40)) * res
    p[10:50, 1] = c['y0'] + (j + g.uniform(0.1, 0.9, 40)) * res
    for (ci, cj), rows, zs, rs in ((TIE_CELL, (50, 51), (0.25, 0.25), (0.2, 0.7)), (ORDER_CELL, (52, 53), (0.5, -0.5), (0.1, 0.9))):
        for row, z, r in zip(rows, zs, rs):
            p[row, :4] = (c['x0'] + (ci + 0.5) * res, c['y0'] + (cj + 0.5) * res, z, r)
    # no other point of the frame in the three special cells
    for row in list(range(8, 10)) + list(range(54, 300)):
        while (math.floor((float(p[row, 0]) - c['x0']) / res), math.floor((float(p[row, 1]) - c['y0']) / res)) in \
                (SATURATED_CELL, TIE_CELL, ORDER_CELL):
            p[row, :2] = g.uniform(lo[:2], hi[:2])

    xm, ym = c['x0'] + H * res, c['y0'] + W * res
    ends = lambda b: R.bev_endpoints(b, c['x0'], c['y0'], res)
    u = lambda a, b: float(g.uniform(a, b))
    draws = [
        lambda g: (u(40, 45), u(28, 32), -1.0, u(3.5, 4.5), u(1.5, 2.0), 1.5, np.float32(np.pi / 2)),        # wholly outside
        lambda g: (xm - u(0.2, 0.8), ym - u(1.0, 2.0), -1.0, u(3.5, 4.5), u(1.5, 2.0), 1.5, u(0.3, 1.2)),    # half outside
        lambda g: (u(3, 5), u(-9, -7), u(-1, 0), 0.0, 0.0, 0.0, u(-3, 3)),                                   # zero size
        lambda g: (u(8, 9), u(0, 1), -1.0, u(3.5, 4.5), u(1.5, 2.0), 1.5, 0.0),                              # yaw 0
        lambda g: (u(8.5, 9.5), u(0.5, 1.5), -1.0, u(3.5, 4.5), u(1.5, 2.0), 1.5, u(0.4, 1.1)),              # over it, higher prio
        lambda g: (u(9, 10), u(0, 1), -1.0, u(3.5, 4.5), u(1.5, 2.0), 1.5, u(-1.1, -0.4)),                   # same prio, other colour
    ]
    boxes = g.uniform(-5, 25, (F, c['bcap'], 7)).astype(np.float32)            # slots behind n_boxes: garbage that must not draw
    colors = np.zeros((F, c['bcap']), np.int64)
    for f in range(F):
        for b in range(c['bcap']):
            colors[f, b] = word(g.integers(1, 200), g.integers(0, 256, 3))
    tries = []
    for k, d in enumerate(draws):
        boxes[2, k], t = rejection(g, d, ends)
        tries.append(t)
    boxes[2, 6] = boxes[2, 5]
    boxes[2, 6, 4] = np.nan                                                     # a NaN box: status bit, the rest still draw
    boxes[2, 6, 0] = 12.0
    boxes[1, 0], t = rejection(g, lambda g: (u(6, 12), u(-6, 6), -1.0, u(3.5, 4.5), u(1.5, 2.0), 1.5, u(-3, 3)), ends)
    tries.append(t)
    for k, prio in enumerate((5, 6, 7, 3, 9, 9, 200)):
        colors[2, k] = word(prio, g.integers(0, 256, 3))
    for f in range(F):                                                          # every live finite box keeps the margin
        for b in range(c['n_boxes'][f]):
            if np.isfinite(boxes[f, b]).all():
                assert margin_ok(ends(boxes[f, b])), (f, b)
    lut = g.integers(0, 256, (256, 3), dtype=np.uint8)                          # random: a wrong index shows
    c.update(points6=pts, n_points=np.array(c['n_points'], np.int32), boxes=boxes, n_boxes=np.array(c['n_boxes'], np.int32),
             colors=colors, lut=lut, tries=tries, background=word(0, (9, 17, 33)))
    return c


# ---- camera: 29 x 41, a KITTI-like P2 scaled to that size ----------------------------------------------------------------
CAMERA = dict(H=29, W=41, z_near=0.5, depth_max=70.4, cap=64, n_points=(40, 25), bcap=6, n_boxes=(4, 2))


def camera_matrix():
    """P2 @ Tr_velo_to_cam f64 (4, 4): KITTI's P2 (f = 721.5377, c = (609.5593, 172.854) on 1242 x 375) scaled to 41 x 29 and
    a Tr_velo_to_cam with KITTI-sized off-axis terms."""
    sx, sy = 41 / 1242.0, 29 / 375.0
    p2 = np.array([[721.5377 * sx, 0.0, 609.5593 * sx, 44.85728 * sx], [0.0, 721.5377 * sy, 172.854 * sy, 0.2163791 * sy],
                   [0.0, 0.0, 1.0, 0.002745884], [0.0, 0.0, 0.0, 1.0]])
    tr = np.array([[7.533745e-03, -9.999714e-01, -6.166020e-04, -4.069766e-03], [1.480249e-02, 7.280733e-04, -9.998902e-01, -7.631618e-02],
                   [9.998621e-01, 7.523790e-03, 1.480755e-02, -2.717806e-01], [0.0, 0.0, 0.0, 1.0]])
    return p2 @ tr


def camera_case(seed=1):
    g = np.random.default_rng(seed)
    c = dict(CAMERA)
    F, cap, H, W = 2, c['cap'], c['H'], c['W']
    mats = np.stack([camera_matrix(), camera_matrix()])
    mats[1, :3, 3] += (0.3, -0.2, 0.05)
    pts = np.zeros((F, cap, 6), np.float32)
    pts[..., 0] = g.uniform(0.5, 90.0, (F, cap))                 # beyond depth_max too: clamped
    pts[..., 1:4] = g.uniform(-1, 1, (F, cap, 3))
    pts[..., 4] = g.uniform(-4, H + 4, (F, cap))
    pts[..., 5] = g.uniform(-4, W + 4, (F, cap))
    pts[0, 0, [0, 4, 5]] = (30.0, 10.5, 20.5)                    # a farther point first ...
    pts[0, 1, [0, 4, 5]] = (8.0, 10.2, 20.9)                     # ... and a nearer one over it
    pts[0, 2, 4], pts[0, 3, 5], pts[0, 4, 0] = np.nan, np.inf, np.nan
    ends = [lambda b, f=f: R.camera_endpoints(b, mats[f], c['z_near']) for f in range(F)]
    u = lambda a, b: float(g.uniform(a, b))

    def far_box(g):
        """20 km wide and 10 km high, 1.5 m ahead, centred on the optical axis: the diagonal of its front face from the top right
        to the bottom left corner runs along the image plane (its slope cancels the tilt of Tr_velo_to_cam's depth row), so it
        crosses the image with both ends in front of the camera and more than 10^5 px away."""
        wide = u(19990, 20010)
        high = wide * (7.523790e-03 / 1.480755e-02) * u(0.999, 1.001)
        return (u(1.4, 1.6), u(-0.3, 0.3), -0.5 * high + u(-0.2, 0.2), u(0.9, 1.1), wide, high, 0.0)

    draws0 = [
        lambda g: (u(10, 14), u(-1, 2), u(-1.8, -1.4), u(3.5, 4.5), u(1.5, 2.0), u(1.4, 1.7), u(-3, 3)),            # in front
        lambda g: (u(2.1, 2.3), u(-0.5, 0.5), u(-1.8, -1.4), u(3.9, 4.1), u(1.5, 1.7), u(1.4, 1.7), u(0.45, 0.55)),   # a corner behind
        lambda g: (u(-12, -8), u(-1, 1), u(-1.8, -1.4), u(3.5, 4.5), u(1.5, 2.0), u(1.4, 1.7), u(-3, 3)),           # wholly behind
        far_box,                                                                                                      # > 10^5 px
    ]
    draws1 = [lambda g: (u(6, 20), u(-3, 3), u(-1.8, -1.4), u(3.5, 4.5), u(1.5, 2.0), u(1.4, 1.7), u(-3, 3))] * 2
    boxes = g.uniform(-5, 25, (F, c['bcap'], 7)).astype(np.float32)
    colors = np.zeros((F, c['bcap']), np.int64)
    tries = []
    for f, draws in enumerate((draws0, draws1)):
        for k, d in enumerate(draws):
            boxes[f, k], t = rejection(g, d, ends[f])
            tries.append(t)
        for b in range(c['bcap']):
            colors[f, b] = word(g.integers(1, 256), g.integers(0, 256, 3))
    for f in range(F):
        for b in range(c['n_boxes'][f]):
            assert margin_ok(ends[f](boxes[f, b])), (f, b)
    c.update(points6=pts, n_points=np.array(c['n_points'], np.int32), boxes=boxes, n_boxes=np.array(c['n_boxes'], np.int32),
             colors=colors, mats=mats, lut=g.integers(0, 256, (256, 3), dtype=np.uint8), tries=tries,
             images=g.integers(0, 256, (F, H, W, 3), dtype=np.uint8))
    return c
