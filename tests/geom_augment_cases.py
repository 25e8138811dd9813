"""Inputs of the geometric-augmentation tests and the restatement's results on them (tests/geom_augment_ref.py); host only.

One frame set of F = 4: point counts 0, 1, 257, 5001 (one frame crosses a block of 256 points, one spans many), box counts
0, 1, 12, 32 (the cap), globals phi = +-pi/4, s = 0.95 / 1.05, flip on and off.  Frame 3 holds the constructed boxes:
  A, B   two neighbours: A's trials 0..2 land on B, trial 3 is a small move (with T = 1 A keeps its pose);
  C      a car fenced in by four cars 0.1 m away whose every trial shifts it by 1 .. 1.5 m on both axes: all trials fail;
  D, E   a pair overlapping below the threshold (IoU 0.032) with points in the overlap: they belong to D, the lower index.
The seeds are chosen so that the restatement's band assertions hold; ``build`` asserts what the cases are meant to contain."""
import numpy as np

import geom_augment_ref as G

VELORANGE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]
IOU_THR = 0.05
F, B, CAP = 4, 32, 5203            # an odd capacity: the frames start on both row parities
N_POINTS = (0, 1, 257, 5001)
N_BOXES = (0, 1, 12, 32)
GLOB = np.array([[np.pi / 4, 0.95, 0, 0], [-np.pi / 4, 1.05, 1, 0], [np.pi / 4, 1.05, 1, 0], [-np.pi / 4, 0.95, 0, 0]], np.float32)
CAR = (3.9, 1.6, 1.56)
A_, B_, C_, D_, E_ = 0, 1, 2, 7, 8          # indices in frame 3; the fence of C is 3..6
_CACHE = {}


def _iou():
    import mvx_oracle as O
    return lambda a, b: O.bbox_pairwise(a, b, True)


def _car(x, y, r, z=-1.6):
    return [x, y, z, CAR[0], CAR[1], CAR[2], r]


def _boxes(rng):
    out = [np.zeros((0, 7), np.float32), np.array([_car(20.0, 3.0, 0.3)], np.float32)]
    b2 = [_car(x + rng.uniform(-1, 1), y + rng.uniform(-1, 1), rng.uniform(-np.pi, np.pi)) for x in (10, 18, 26, 34) for y in (-8, 0, 8)]
    out.append(np.array(b2, np.float32))
    b3 = [_car(20.0, -20.0, 0.0), _car(25.0, -20.0, 0.0),                      # A, B
          _car(40.0, -20.0, 0.0),                                              # C and its fence
          _car(40.0, -20.0 + 1.7, 0.0), _car(40.0, -20.0 - 1.7, 0.0), _car(40.0 + 4.0, -20.0, 0.0), _car(40.0 - 4.0, -20.0, 0.0),
          _car(30.0, -8.0, 0.0), _car(30.0, -6.5, 0.0)]                        # D, E
    spots = [(x, y) for x in (6, 14, 22, 30, 38, 46, 54, 62) for y in (2, 10, 18, -30)]
    for x, y in spots[:32 - len(b3)]:
        b3.append(_car(x + rng.uniform(-1, 1), y + rng.uniform(-1, 1), rng.uniform(-np.pi, np.pi), z=rng.uniform(-2.0, -1.2)))
    out.append(np.array(b3, np.float32))
    return out


def _noise(rng):
    noise, _ = G.draw_like(F, B, 32, rng)
    n3 = noise[3]
    n3[A_, :3] = [[5.0, 0.0, 0.1, 0.0], [4.7, 0.2, -0.1, 0.05], [5.3, -0.2, 0.0, -0.05]]
    n3[A_, 3] = [0.2, 0.1, 0.05, 0.1]
    sign = np.where(n3[C_, :, :2] < 0, -1.0, 1.0)
    n3[C_, :, :2] = sign * (1.0 + 0.5 * np.minimum(np.abs(n3[C_, :, :2]), 1.0))          # 1 .. 1.5 m: never over the fence
    return noise


def _cloud(rng, boxes, n_want, noise, glob, iou):
    """Points inside every box (in its own frame, 0.98 of the half sizes) plus background, cleaned of everything near a face,
    cut to ``n_want`` rows; column 3 = the row's index, columns 4..5 arbitrary bit patterns (one NaN with a payload)."""
    if n_want == 0:
        return np.zeros((0, 6), np.float32)
    parts = []
    per = max(4, (n_want * 2) // (3 * max(1, boxes.shape[0])))
    for b in boxes.astype(np.float64):
        loc = rng.uniform(-0.49, 0.49, (per, 2)) * b[3:5]
        xy = G.rot(loc, b[6]) + b[:2]
        parts.append(np.concatenate([xy, b[2] + rng.uniform(0.01, 0.99, (per, 1)) * b[5]], 1))
    if boxes.shape[0] > E_:                                         # the overlap of D and E
        d = boxes[D_].astype(np.float64)
        parts.insert(0, np.stack([d[0] + rng.uniform(-1.5, 1.5, 6), np.full(6, d[1] + 0.75), np.full(6, d[2] + 0.5)], 1))
    lo, hi = np.array(VELORANGE[:3]), np.array(VELORANGE[3:])
    parts.append(rng.uniform(lo - 2.0, hi + 2.0, (2 * n_want, 3)))
    xyz = np.concatenate(parts, 0)
    xyz = xyz[rng.permutation(xyz.shape[0])] if n_want > 1 else xyz
    pts = np.zeros((xyz.shape[0], 6), np.float32)
    pts[:, :3] = xyz
    pts = G.clean_cloud(pts, boxes, noise, glob, VELORANGE, IOU_THR, iou)
    assert pts.shape[0] >= n_want
    pts = pts[:n_want].copy()
    pts[:, 3] = np.arange(n_want, dtype=np.float32)
    pts[:, 4:] = rng.uniform(0, 1224, (n_want, 2)).astype(np.float32)
    pts[:, 4:].view(np.uint32)[0, 0] = 0x7FC12345                  # a NaN with a payload: columns 3..5 pass bitwise
    return pts


def build(T, seed=0):
    """dict(boxes, noise (F, B, T, 4), glob, clouds, refs): the inputs for ``T`` trials and the restatement's result per frame."""
    key = (T, seed)
    if key in _CACHE:
        return _CACHE[key]
    iou = _iou()
    rng = np.random.default_rng(100 + seed)
    boxes = _boxes(rng)
    noise = np.ascontiguousarray(_noise(rng)[:, :, :T])
    clouds, refs = [], []
    for f in range(F):
        c = _cloud(rng, boxes[f], N_POINTS[f], noise[f], GLOB[f], iou)
        clouds.append(c)
        refs.append(G.augment_frame(c, boxes[f], noise[f], GLOB[f], VELORANGE, IOU_THR, iou))      # asserts the bands
    r3 = refs[3]
    # what the cases are meant to contain
    assert r3['trial'][A_] == (3 if T > 3 else -1) and r3['trial'][C_] == -1
    assert 0 in r3['trial'].tolist()
    own = r3['owner']
    in_both = (G.owner_of(boxes[3][[E_]], clouds[3][:, :3])[0] == 0) & (own == D_)
    assert in_both.sum() >= 1                                                   # points in the overlap belong to D
    assert 0 < r3['kept_boxes'].size < 32 and 0 < r3['kept_points'].size < N_POINTS[3]
    assert refs[2]['kept_boxes'].size > 0 and refs[2]['kept_points'].size > 0
    moved_pts = sum(int(((r['owner'] >= 0) & (r['trial'][np.maximum(r['owner'], 0)] >= 0)).sum()) for r in refs[1:] if r['trial'].size)
    assert moved_pts > 100
    out = dict(boxes=boxes, noise=noise, glob=GLOB.copy(), clouds=clouds, refs=refs)
    _CACHE[key] = out
    return out
