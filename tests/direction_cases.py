"""Inputs of the direction tests (tests/test_direction_host.py, tests/test_direction_gpu.py): the focal-loss cases of
focal_cases.py with direction logits appended and the ground-truth yaws redrawn over [-3 pi / 2, pi / 2] (the range labels
reach the loss with), and planted detections for the decode.

The f32 kernels and the f64 reference may legitimately differ where a floor() flips or an NMS comparison ties, and nowhere
else, so the builders ASSERT on the CPU that no input sits there (a draw that does is redrawn with the next seed, never
dropped):
  * every mod(g6 - dir_offset, pi) is at least MARGIN from 0 and pi (the direction bit);
  * every decoded mod(theta - dir_offset, pi) is at least MARGIN from 0 and pi (the fold);
  * every pairwise BEV IoU of an NMS case is at least MARGIN away from iou_thr."""
import math

import numpy as np

import direction_ref as DR
import focal_cases as C

MARGIN = 1e-3
OFFSETS = (0.0, math.pi / 4)
SATURATED = np.array([-90, -20, 0, 20, 90], np.float32)


def _yaws(rng, n, offsets):
    """n yaws f32 uniform over [-3 pi / 2, pi / 2], clear of the bin boundaries of every offset; None when the draw is not."""
    y = rng.uniform(-1.5 * math.pi, 0.5 * math.pi, n).astype(np.float32)
    if any(DR.fold_margin(y, off).min() < MARGIN for off in offsets):
        return None
    return y


def with_direction(name, saturated=False, seed=100, offsets=OFFSETS):
    """focal_cases.<name>() + 'dir' f32 (F*l*w, A) ~ N(0,3) (or the saturated tiling), yaws redrawn; both bits occur."""
    base = getattr(C, name)()
    rows, A = base['heads'].shape[0], base['A']
    while True:
        rng = np.random.default_rng(seed)
        case = dict(base)
        case['gts'] = base['gts'].copy()
        case['gts'][:, 6] = rng.uniform(-1.5 * math.pi, 0.5 * math.pi, base['gts'].shape[0]).astype(np.float32)
        if saturated:
            case['dir'] = np.resize(SATURATED, rows * A).reshape(rows, A).copy()
        else:
            case['dir'] = rng.normal(0.0, 3.0, (rows, A)).astype(np.float32)
        if admissible(case, offsets):
            check_case(case, offsets)
            return case
        seed += 1


def _used_yaws(case):
    return np.concatenate([case['gts'][int(case['gt_off'][f]) + case['gi'][f, :int(case['counts'][f, 0])], 6]
                           for f in range(case['F'])])


def admissible(case, offsets=OFFSETS):
    """No yaw within MARGIN of a bin boundary, both direction bits among the listed boxes, yaws spanning more than pi."""
    used = _used_yaws(case)
    for off in offsets:
        bits = DR.direction_bit(used, off)
        if DR.fold_margin(case['gts'][:, 6], off).min() < MARGIN or bits.min() == bits.max():
            return False
    return float(used.max() - used.min()) > math.pi


def check_case(case, offsets=OFFSETS):
    assert admissible(case, offsets)
    for f in range(case['F']):                                  # entries beyond the counts are garbage the kernels never read
        n_pos, n_neg = (int(v) for v in case['counts'][f])
        assert (case['pos'][f, :, n_pos:] == C.GARBAGE).all() and (case['gi'][f, n_pos:] == C.GARBAGE).all()
        assert (case['neg'][f, :, n_neg:] == -C.GARBAGE).all()


def wide_rows(case):
    """The rows a direction model's heads GEMM writes: [A cls | 7A reg | A dir | pad to a multiple of 4], pad = NaN-free junk
    that nothing may read into a result (the loss reads columns < 9A only)."""
    rows, A = case['heads'].shape[0], case['A']
    ld = (9 * A + 3) // 4 * 4
    wide = np.full((rows, ld), 7.0, np.float32)
    wide[:, :8 * A] = case['heads']
    wide[:, 8 * A:9 * A] = case['dir']
    return wide


# ---- decode: planted boxes on a 6 x 5 grid ----------------------------------------------------------------------------------
DL, DW, DA, DF = 6, 5, 2, 2
IOU_THR = 0.1


def decode_anchors():
    """f32 [6][5][2][7]: Car anchors (3.9 x 1.6 x 1.56) every 2.0 m / 1.6 m, yaw 0 and pi / 2."""
    an = C.anchor_grid(DL, DW, DA)
    an[..., 0] = (np.arange(DL, dtype=np.float32) * 2.0 + 1.0)[:, None, None]
    an[..., 1] = (np.arange(DW, dtype=np.float32) * 1.6 - 4.0)[None, :, None]
    return an


def _decode_draw(seed, dir_offset, n_box):
    import detect_ref as D
    import mvx_oracle as O
    rng = np.random.default_rng(seed)
    an = decode_anchors()
    cls = np.full((DF, DL, DW, DA), -10.0, np.float32)
    reg = rng.normal(0.0, 0.1, (DF, DL, DW, 7 * DA)).astype(np.float32)
    dirl = rng.normal(0.0, 3.0, (DF, DL, DW, DA)).astype(np.float32)
    planted = []
    for f in range(DF):
        cells = rng.permutation(DL * DW)[:n_box]
        yaws = _yaws(rng, n_box, (dir_offset,))
        if yaws is None:
            return None
        frame = []
        for k, cell in enumerate(cells):
            x, y, a = int(cell) // DW, int(cell) % DW, int(rng.integers(0, DA))
            g = np.zeros(7, np.float32)
            g[0:3] = an[x, y, a, 0:3] + rng.uniform(-0.5, 0.5, 3).astype(np.float32)
            g[3:6] = an[x, y, a, 3:6] * rng.uniform(0.9, 1.1, 3).astype(np.float32)
            g[6] = yaws[k]
            r = D.encode(g, an[x, y, a])
            shift = (0.0, math.pi, -math.pi, 0.0)[k % 4]        # half of them half a turn off
            r[6] += shift
            reg[f, x, y, 7 * a:7 * a + 7] = r.astype(np.float32)
            bit = int(DR.direction_bit(g[6], dir_offset))
            dirl[f, x, y, a] = 3.0 if bit else -3.0
            cls[f, x, y, a] = 3.0 - 0.25 * k                    # distinct logits: the candidate order is the planting order
            frame.append(dict(gt=g, n=(x * DW + y) * DA + a, bit=bit, shift=shift))
        planted.append(frame)
    # conditions on what the device decodes (its f32 inputs): the fold, the bits, the NMS comparisons
    for f, frame in enumerate(planted):
        idx = np.array([p['n'] for p in frame])
        r = reg[f].reshape(-1, DA, 7).reshape(-1, 7)[idx]
        theta = r[:, 6].astype(np.float64) + an.reshape(-1, 7)[idx, 6]
        if DR.fold_margin(theta, dir_offset).min() < MARGIN:
            return None
        boxes = DR.decode_dir(r, an.reshape(-1, 7)[idx], dirl[f].reshape(-1)[idx], dir_offset)
        plain = D.decode(r, an.reshape(-1, 7)[idx], 'loss')
        for b in (boxes, plain):
            q = D.corners(b)
            iou = O.bbox_pairwise(q, q, True)
            off_diag = iou[~np.eye(len(idx), dtype=bool)]
            if (np.abs(off_diag - IOU_THR) < MARGIN).any():
                return None
        if not (iou[~np.eye(len(idx), dtype=bool)] > IOU_THR).any() and f == 0:
            return None                                         # frame 0 must exercise a suppression
    bits = [p['bit'] for frame in planted for p in frame]
    if min(bits) == max(bits):
        return None
    return dict(F=DF, l=DL, w=DW, A=DA, anchors=an, cls=cls, reg=reg, dir=dirl, planted=planted, dir_offset=dir_offset,
                iou_thr=IOU_THR)


def decode_case(dir_offset=math.pi / 4, seed=200, n_box=6):
    """Two frames of ``n_box`` planted boxes each: the chosen anchor of every box regresses it perfectly (half of them with
    r6 half a turn off), its direction logit is +-3 by the box's bit, its cls logit 3 - 0.25 k; everything else is
    background at -10.  Redrawn with the next seed until every condition of the module docstring holds."""
    while True:
        case = _decode_draw(seed, dir_offset, n_box)
        if case is not None:
            return case
        seed += 1
        assert seed < 400, 'no admissible draw'


def decode_heads(case, with_dir=True):
    """The case as channels-last head rows: (F*l*w, 20) = [cls 2 | reg 14 | dir 2 | 0 0], or the plain (F*l*w, 16)."""
    F, l, w = case['F'], case['l'], case['w']
    parts = [case['cls'], case['reg']]
    if with_dir:
        parts += [case['dir'], np.zeros((F, l, w, 2), np.float32)]
    return np.concatenate(parts, axis=3).reshape(F * l * w, -1)
