"""Inputs of the IoU-head tests (tests/test_iou_head_host.py, tests/test_iou_head_gpu.py): the direction cases of
direction_cases.py with IoU logits appended and the regression rows of the listed positives set to
``detect_ref.encode(gt, anchor)`` plus noise of graded size, so that the IoU targets cover [0, 1] (the N(0,1.5) regressions
of focal_cases decode to boxes that miss their ground truth: q would be 0 almost everywhere).

The builders ASSERT on the CPU, and redraw with the next seed when a draw fails (never drop an entry), that per case
  * at least one entry is rejected by the bounding circles (q = 0 exactly),
  * at least one entry overlaps its box in the BEV but not vertically (q = 0 exactly),
  * at least a quarter of the entries have q in (0.1, 0.9), at least one q > 0.95,
  * one entry has a size regression of 200: expf overflows, q = 0,
  * no entry sits within MARGIN of a decision (circle rejection, vertical overlap 0) where f32 and f64 may disagree;
and for the decode cases that no two candidates have float64 s closer than 1e-4 unless their logits are identical, no exp(s)
lies within 1e-4 of score_thr and no pairwise IoU within 1e-3 of iou_thr."""
import functools
import math

import numpy as np

import detect_ref as D
import direction_cases as DC
import focal_cases as C
import iou_head_ref as IR

MARGIN = IR.ZERO_MARGIN
ROLES = ('tight', 'mid', 'far', 'vert', 'overflow', 'mid', 'loose', 'mid')


def _noise(rng, role, grade):
    """The regression error of an entry by its role: 'tight' a few millimetres, 'mid' / 'loose' graded shifts, 'far' a shift
    beyond the bounding circles, 'vert' a tight box lifted above its ground truth, 'overflow' a size regression of 200."""
    e = rng.normal(0.0, 0.002, 7)
    if role == 'mid':
        e[0:2] += rng.choice([-1.0, 1.0], 2) * (0.04 + 0.05 * grade)           # in diagonals of the anchor (4.2 m)
        e[3:6] += rng.normal(0.0, 0.05, 3)
        e[6] += rng.normal(0.0, 0.05)
    elif role == 'loose':
        e[0:2] += rng.choice([-1.0, 1.0], 2) * (0.2 + 0.1 * grade)
        e[6] += rng.normal(0.0, 0.4)
    elif role == 'far':
        e[0] += 3.0                                                            # 12.6 m: the circles (r ~ 2.1 m) are apart
    elif role == 'vert':
        e[2] += 2.0                                                            # two anchor heights up: no vertical overlap
    elif role == 'overflow':
        e[3 + int(rng.integers(0, 3))] = 200.0
    return e


def _set_rows(case, rng):
    """Regression rows of the listed anchors = encode(gt of the anchor's FIRST entry, anchor) + the role's noise."""
    F, l, w, A = case['F'], case['l'], case['w'], case['A']
    heads = case['heads'].reshape(F, l, w, 8 * A).copy()
    seen, n = set(), 0
    for f in range(F):
        for k, x, y, z, row in IR._entry_rows(case, f):
            if (f, x, y, z) in seen:
                continue
            seen.add((f, x, y, z))
            role = ROLES[n % len(ROLES)]
            r = D.encode(case['gts'][row, :7], case['anchors'][x, y, z]) + _noise(rng, role, (n // len(ROLES)) % 4)
            heads[f, x, y, A + 7 * z:A + 7 * z + 7] = r.astype(np.float32)
            n += 1
    case['heads'] = heads.reshape(F * l * w, 8 * A)


def conditions(case):
    """The list of violated conditions of the module docstring (empty = admissible), and the entry records."""
    q, recs = IR.targets(case)
    bad = []
    fin = [r for r in recs if r['finite']]
    if not any(r['gap'] > MARGIN for r in fin):
        bad.append('no entry rejected by the circles')
    if not any(r['gap'] <= 0 and r['inter'] > 0.1 and r['ih'] < -MARGIN for r in fin):
        bad.append('no entry with BEV overlap and no vertical overlap')
    if 4 * sum(0.1 < r['q'] < 0.9 for r in recs) < len(recs):
        bad.append('fewer than a quarter of the entries in (0.1, 0.9)')
    if not any(r['q'] > 0.95 for r in recs):
        bad.append('no entry above 0.95')
    if sum(not r['finite'] for r in recs) < 1:
        bad.append('no overflowing size regression')
    if any(abs(r['gap']) <= MARGIN or abs(r['ih']) <= MARGIN for r in fin):
        bad.append('an entry within MARGIN of a decision')
    return bad, recs


def _extend_case1(case):
    """Five more positives in frame 0 of case 1 (its 4 entries cannot meet five conditions): distinct anchors, boxes 0 / 1."""
    extra = [(0, 1, 1), (2, 0, 0), (5, 3, 1), (3, 4, 0), (0, 4, 1)]
    for k, e in enumerate(extra):
        case['pos'][0, :, 4 + k] = e
        case['gi'][0, 4 + k] = k % 2
    case['counts'][0, 0] = 9


def _base(name):
    if name == 'case3':              # case 3's grid with ~300 positives per frame: nq > 1, entries no multiple of 128
        base = C.random_case(2, 44, 50, 2, 301, 25, 6, seed=3)
        seed = 100
        while True:
            rng = np.random.default_rng(seed)
            base['gts'][:, 6] = rng.uniform(-1.5 * math.pi, 0.5 * math.pi, base['gts'].shape[0]).astype(np.float32)
            base['dir'] = rng.normal(0.0, 3.0, (base['heads'].shape[0], base['A'])).astype(np.float32)
            if DC.admissible(base):
                DC.check_case(base)
                return base
            seed += 1
    return DC.with_direction(name)


@functools.lru_cache(maxsize=None)
def with_iou(name, saturated=False, seed=300):
    """direction_cases.with_direction(<name>) + 'iou' f32 (F*l*w, A) ~ N(0,3) (or the saturated tiling), regression rows of
    the positives as described above.  Treat the result as read-only: it is shared between the tests."""
    base = _base(name)
    rows, A = base['heads'].shape[0], base['A']
    while True:
        rng = np.random.default_rng(seed)
        case = dict(base)
        for key in ('pos', 'gi', 'counts', 'gts', 'heads'):
            case[key] = base[key].copy()
        if name == 'case1':
            _extend_case1(case)
        _set_rows(case, rng)
        if saturated:
            case['iou'] = np.resize(DC.SATURATED[::-1], rows * A).reshape(rows, A).copy()
        else:
            case['iou'] = rng.normal(0.0, 3.0, (rows, A)).astype(np.float32)
        bad, recs = conditions(case)
        if not bad:
            case['recs'] = recs
            return case
        seed += 1
        assert seed < 340, 'no admissible draw of %s: %s' % (name, bad)


def wide_rows(case):
    """The rows an IoU model's heads GEMM writes: [A cls | 7A reg | A dir | A iou | pad to a multiple of 4] (A = 2: 20)."""
    rows, A = case['heads'].shape[0], case['A']
    ld = (10 * A + 3) // 4 * 4
    wide = np.full((rows, ld), 7.0, np.float32)
    wide[:, :8 * A] = case['heads']
    wide[:, 8 * A:9 * A] = case['dir']
    wide[:, 9 * A:10 * A] = case['iou']
    return wide


# ---- decode -----------------------------------------------------------------------------------------------------------------
SCORE_THR = 0.3


@functools.lru_cache(maxsize=None)
def decode_case(alpha=0.5, seed=400):
    """direction_cases.decode_case() with IoU logits: the planted anchors get IoU logits that reverse part of the cls order,
    two of them IDENTICAL (cls, iou) pairs (the index tie), one a NaN IoU logit, one an IoU logit that takes it below
    SCORE_THR; the background keeps cls -10 and gets IoU logits around -8 (never admitted, also at a = 1)."""
    import mvx_oracle as O
    base = DC.decode_case()
    F, l, w, A = base['F'], base['l'], base['w'], base['A']
    while True:
        rng = np.random.default_rng(seed)
        case = dict(base)
        case['cls'] = base['cls'].copy()
        iou = rng.normal(-8.0, 0.5, base['cls'].shape).astype(np.float32)       # the background: never admitted, at any a > 0
        special = {}
        for f, frame in enumerate(base['planted']):
            ns = [p['n'] for p in frame]
            flat_c, flat_u = case['cls'][f].reshape(-1), iou[f].reshape(-1)
            flat_u[ns] = rng.uniform(-1.0, 3.0, len(ns)).astype(np.float32)
            flat_c[ns[1]], flat_u[ns[1]] = flat_c[ns[0]], flat_u[ns[0]]          # identical logits: lowest index first
            flat_u[ns[2]] = np.nan                                               # dropped
            flat_u[ns[3]] = -6.0                                                 # below the threshold unless a = 0
            special[f] = dict(tie=(ns[0], ns[1]), nan=ns[2], low=ns[3])
        case.update(iou=iou, special=special, score_thr=SCORE_THR)
        if _decode_ok(case, alpha, O):
            return case
        seed += 1
        assert seed < 440, 'no admissible decode draw'


def _decode_ok(case, alpha, O):
    import direction_ref as DR
    F, A = case['F'], case['A']
    an = case['anchors'].reshape(-1, 7)
    for a in sorted({alpha, 1.0}):
        for f in range(F):
            c, u = case['cls'][f].reshape(-1), case['iou'][f].reshape(-1)
            s = IR.rectified_log(c, u, a)
            with np.errstate(invalid='ignore'):
                if (np.abs(np.exp(s) - case['score_thr']) < 1e-4).any():
                    return False
            keep, _, _ = IR.candidates(c, u, a, case['score_thr'], 1000)
            if len(keep) < 3:
                return False
            for i in range(len(keep)):
                for j in range(i + 1, len(keep)):
                    same = c[keep[i]] == c[keep[j]] and u[keep[i]] == u[keep[j]]
                    if not same and abs(s[keep[i]] - s[keep[j]]) < 1e-4:
                        return False
            r = case['reg'][f].reshape(-1, 7)[keep]
            boxes = DR.decode_dir(r, an[keep], case['dir'][f].reshape(-1)[keep], case['dir_offset'])
            quads = D.corners(boxes)
            iou = O.bbox_pairwise(quads, quads, True)
            off = iou[~np.eye(len(keep), dtype=bool)]
            if (np.abs(off - case['iou_thr']) < 1e-3).any():
                return False
    return True


def decode_heads(case, with_iou=True):
    """The case as channels-last head rows (F*l*w, 20) = [cls 2 | reg 14 | dir 2 | iou 2] (or zeros in the last two)."""
    F, l, w = case['F'], case['l'], case['w']
    last = case['iou'] if with_iou else np.zeros((F, l, w, 2), np.float32)
    return np.concatenate([case['cls'], case['reg'], case['dir'], last], axis=3).reshape(F * l * w, -1)
