"""KITTI object evaluation: AP of 2D bbox, BEV and 3D boxes plus AOS, easy / moderate / hard, R11 and R40, on the GPU.

The semantics are those of the widely used kitti-object-eval-python tool, quirks included (DESIGN.md section 3.17 states
them).  The reference has no evaluation.  Here:
  * ``read_kitti_file`` / ``parse_kitti_lines``: ``label_2`` rows of every class, with the score column of result files;
  * ``evaluate``: all frames of a split in one flat layout, four stages on the device (csrc/kitti_eval.hip): overlaps,
    the threshold pass, get_thresholds, the counting pass with its fixed-order frame sums.  The cleaning flags are set on
    the host (vectorised), and the curves' TP scores are sorted with torch on the device.  Precision and AP come from the
    curves' totals (41 entries each) on the host;
  * ``format_table``: the familiar text block; ``evaluate_dirs``: label and result directories;
  * ``annos_from_detections``: detections in memory -> annotations through ``detect.kitti_lines``, so results in memory
    and on disk score identically.
"""
import os

import numpy as np
import torch

from modules import _hip
from modules import Extension as X

MIN_HEIGHT = (40, 25, 25)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
DIFFICULTIES = ('easy', 'moderate', 'hard')
METRICS = ('bbox', 'bev', '3d')
NEIGHBOUR = {'car': 'van', 'pedestrian': 'person_sitting'}
# minimum overlaps of the 2D / BEV / 3D metrics: the strict setting, then the loose one
MIN_OVERLAPS = {'car': ((0.7, 0.7, 0.7), (0.7, 0.5, 0.5)),
                'pedestrian': ((0.5, 0.5, 0.5), (0.5, 0.25, 0.25)),
                'cyclist': ((0.5, 0.5, 0.5), (0.5, 0.25, 0.25))}
N_THRESHOLDS = 41                       # MVX_KITTI_THRESHOLDS
MAX_DETECTIONS = 4096                   # MVX_DETECT_MAX_PRE
MAX_GT = 1024                           # MVX_KITTI_MAX_GT: GT plus don't-care rows of one frame
MAX_CURVES = 72                         # MVX_KITTI_MAX_CURVES
FIELDS = ('truncated', 'occluded', 'alpha', 'bbox', 'hwl', 'location', 'rotation_y', 'score')


# ---- files ---------------------------------------------------------------------------------------------------------------
def _empty_anno():
    return dict(name=np.zeros((0,), dtype='<U16'), truncated=np.zeros((0,)), occluded=np.zeros((0,)), alpha=np.zeros((0,)),
                bbox=np.zeros((0, 4)), hwl=np.zeros((0, 3)), location=np.zeros((0, 3)), rotation_y=np.zeros((0,)),
                score=np.zeros((0,)))


def parse_kitti_lines(lines):
    """``label_2`` rows ``name trunc occl alpha x1 y1 x2 y2 h w l x y z ry [score]`` -> dict of float64 arrays (``bbox``
    (n,4), ``hwl`` (n,3) in file order, ``location`` (n,3), ...; ``score`` 0 where the column is absent) and ``name``."""
    rows = [ln.split() for ln in lines if ln.strip()]
    if not rows:
        return _empty_anno()
    for r in rows:
        if len(r) not in (15, 16):
            raise ValueError('a KITTI label row has 15 or 16 columns, not %d: %r' % (len(r), ' '.join(r)))
    num = np.array([[float(v) for v in r[1:15]] + [float(r[15]) if len(r) == 16 else 0.0] for r in rows], dtype=np.float64)
    return dict(name=np.array([r[0] for r in rows]), truncated=num[:, 0], occluded=num[:, 1], alpha=num[:, 2], bbox=num[:, 3:7],
                hwl=num[:, 7:10], location=num[:, 10:13], rotation_y=num[:, 13], score=num[:, 14])


def read_kitti_file(path):
    """One label or result file (every class, every column).  A file without rows has no objects; a missing file raises
    FileNotFoundError naming it."""
    if not os.path.isfile(path):
        raise FileNotFoundError('KITTI file not found: %s' % path)
    with open(path, 'r') as f:
        return parse_kitti_lines(f.read().splitlines())


def annos_from_detections(dets, calib, imsize):
    """One frame's detections (dict with 'boxes' (n,7) LiDAR xyzlwhr and 'scores') -> the annotation its result file would
    read back as (``detect.kitti_lines``, then ``parse_kitti_lines``)."""
    from modules.detect import kitti_lines
    return parse_kitti_lines(kitti_lines(dets, calib, imsize))


def bev_quads_camera(location, hwl, rotation_y):
    """BEV corner quads (n,4,2) f32 in the camera (x, z) plane of boxes with size (h, w, l) and yaw ry: the l x w rectangle
    about (x, z), corners (-l/2,-w/2), (-l/2,w/2), (l/2,w/2), (l/2,-w/2) turned by ry.  Float64 arithmetic, one rounding
    to f32: the device and any host reference start from the same bits."""
    loc = np.asarray(location, np.float64).reshape(-1, 3)
    dims = np.asarray(hwl, np.float64).reshape(-1, 3)
    ry = np.asarray(rotation_y, np.float64).reshape(-1)
    l, w = dims[:, 2:3], dims[:, 1:2]
    cx = np.array([-0.5, -0.5, 0.5, 0.5]) * l
    cz = np.array([-0.5, 0.5, 0.5, -0.5]) * w
    c, s = np.cos(ry)[:, None], np.sin(ry)[:, None]
    q = np.stack([c * cx + s * cz + loc[:, 0:1], -s * cx + c * cz + loc[:, 2:3]], 2)
    return q.astype(np.float32)


def box_rows(anno):
    """f64 (n,8) rows x1 y1 x2 y2 l w h y of an annotation (the layout of the device kernels)."""
    hwl = anno['hwl']
    return np.concatenate([anno['bbox'], hwl[:, 2:3], hwl[:, 1:2], hwl[:, 0:1], anno['location'][:, 1:2]], 1).astype(np.float64)


# ---- cleaning ------------------------------------------------------------------------------------------------------------
def clean_flags(gt_name, gt_trunc, gt_occl, gt_height, det_name, det_height, cls, diff):
    """(ignored_gt, ignored_det) int8 of every row for one class and difficulty (names lower case)."""
    cls = cls.lower()
    vc = np.where(gt_name == cls, 1, np.where(gt_name == NEIGHBOUR.get(cls, '\0'), 0, -1))
    ignore = (gt_occl > MAX_OCCLUSION[diff]) | (gt_trunc > MAX_TRUNCATION[diff]) | (gt_height <= MIN_HEIGHT[diff])
    ig = np.where((vc == 1) & ~ignore, 0, np.where((vc == 0) | ((vc == 1) & ignore), 1, -1))
    idt = np.where(det_height < MIN_HEIGHT[diff], 1, np.where(det_name == cls, 0, -1))
    return ig.astype(np.int8), idt.astype(np.int8)


def curve_table(classes):
    """The curves of ``classes``: list of (class, setting, metric, difficulty) and the matching (metric, flag set) rows and
    minimum overlaps; curve index = ((class * 2 + setting) * 3 + metric) * 3 + difficulty."""
    keys, desc, mo = [], [], []
    for ci, cls in enumerate(classes):
        table = MIN_OVERLAPS[cls.lower()]
        for k in range(2):
            for m in range(3):
                for d in range(3):
                    keys.append((cls, k, METRICS[m], DIFFICULTIES[d]))
                    desc.append((m, ci * 3 + d))
                    mo.append(table[k][m])
    return keys, np.array(desc, np.int32).reshape(-1, 2), np.array(mo, np.float64)


# ---- the flat layout -----------------------------------------------------------------------------------------------------
class EvalInput:
    """All frames of an evaluation in the flat layout of csrc/kitti_eval.hip (host arrays; ``to(dev)`` uploads them)."""

    def __init__(self, gt_annos, dt_annos, classes):
        if len(gt_annos) != len(dt_annos):
            raise ValueError('%d GT frames but %d result frames' % (len(gt_annos), len(dt_annos)))
        if not gt_annos:
            raise ValueError('no frames to evaluate')
        for cls in classes:
            if cls.lower() not in MIN_OVERLAPS:
                raise ValueError('no overlap settings for class %r (known: Car, Pedestrian, Cyclist)' % cls)
        self.classes = tuple(classes)
        self.F = len(gt_annos)
        gts, dcs = [], []
        for a in gt_annos:
            care = np.char.lower(a['name'].astype(str)) != 'dontcare'
            gts.append({k: a[k][care] for k in ('name',) + FIELDS})
            dcs.append(a['bbox'][~care])
        nd = np.array([len(a['name']) for a in dt_annos], np.int64)
        ng = np.array([len(a['name']) for a in gts], np.int64)
        nc = np.array([len(b) for b in dcs], np.int64)
        bad = np.nonzero((nd > MAX_DETECTIONS) | (ng + nc > MAX_GT))[0]
        if len(bad):
            f = int(bad[0])
            raise X.MvxHipError('frame %d holds %d detections and %d GT + don\'t-care rows (limits %d and %d)'
                                % (f, nd[f], ng[f] + nc[f], MAX_DETECTIONS, MAX_GT))
        z = np.zeros(1, np.int64)
        self.off = np.stack([np.concatenate([z, np.cumsum(n)]) for n in (nd, ng, nc)]).astype(np.int32)
        self.pair_off = np.stack([np.concatenate([z, np.cumsum(p)]) for p in (nd * ng, nd * nc, np.minimum(nd, ng))])
        self.n_pairs, self.n_dc_pairs, self.n_slots = (int(v) for v in self.pair_off[:, -1])

        def cat(annos, key, shape):
            parts = [a[key] for a in annos]
            return np.concatenate(parts).reshape(shape) if parts else np.zeros(shape)
        self.det_rows = np.concatenate([box_rows(a) for a in dt_annos]).reshape(-1, 8)
        self.gt_rows = np.concatenate([box_rows(a) for a in gts]).reshape(-1, 8)
        self.dc_rows = np.concatenate(dcs).reshape(-1, 4).astype(np.float64)
        self.det_quads = bev_quads_camera(cat(dt_annos, 'location', (-1, 3)), cat(dt_annos, 'hwl', (-1, 3)), cat(dt_annos, 'rotation_y', (-1,)))
        self.gt_quads = bev_quads_camera(cat(gts, 'location', (-1, 3)), cat(gts, 'hwl', (-1, 3)), cat(gts, 'rotation_y', (-1,)))
        self.scores = cat(dt_annos, 'score', (-1,)).astype(np.float64)
        self.det_alpha = cat(dt_annos, 'alpha', (-1,)).astype(np.float64)
        self.gt_alpha = cat(gts, 'alpha', (-1,)).astype(np.float64)
        det_name = np.char.lower(cat(dt_annos, 'name', (-1,)).astype(str))
        gt_name = np.char.lower(cat(gts, 'name', (-1,)).astype(str))
        det_h = self.det_rows[:, 3] - self.det_rows[:, 1]
        gt_h = self.gt_rows[:, 3] - self.gt_rows[:, 1]
        gt_trunc, gt_occl = cat(gts, 'truncated', (-1,)), cat(gts, 'occluded', (-1,))
        n_sets = 3 * len(classes)
        self.ignored_gt = np.zeros((n_sets, len(gt_name)), np.int8)
        self.ignored_det = np.zeros((n_sets, len(det_name)), np.int8)
        for ci, cls in enumerate(classes):
            for d in range(3):
                self.ignored_gt[ci * 3 + d], self.ignored_det[ci * 3 + d] = clean_flags(
                    gt_name, gt_trunc, gt_occl, gt_h, det_name, det_h, cls, d)
        self.keys, self.curves, self.min_overlaps = curve_table(classes)
        if len(self.keys) > MAX_CURVES:
            raise X.MvxHipError('%d curves; at most %d per evaluation' % (len(self.keys), MAX_CURVES))

    def to(self, dev):
        """Device copies of the arrays the kernels read."""
        t = {}
        for k in ('off', 'pair_off', 'det_rows', 'gt_rows', 'dc_rows', 'det_quads', 'gt_quads', 'scores', 'det_alpha', 'gt_alpha',
                  'ignored_gt', 'ignored_det'):
            t[k] = torch.from_numpy(np.ascontiguousarray(getattr(self, k))).to(dev)
        return t


def run_device(inp, dev, events=None):
    """The four device stages of ``inp`` (EvalInput).  Returns device tensors: overlaps (3, n_pairs), dc_overlaps, tp_scores
    (sorted descending per curve), n_valid_gt, thresholds (C, 41), n_thresholds, n_gt, totals (C, 41, 3), similarity (C, 41).
    ``events``: a list that receives a recorded torch.cuda.Event before the first stage and after each stage."""
    def mark():
        if events is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            events.append(e)
    t = inp.to(dev)
    mark()
    ov, dco = _hip.kitti_eval_overlaps(inp, t)
    mark()
    tp_scores, n_valid = _hip.kitti_eval_tp_scores(inp, t, ov)
    tp_sorted = torch.sort(tp_scores, dim=1, descending=True).values
    mark()
    thr, n_thr, n_gt = _hip.kitti_eval_thresholds(inp, tp_sorted, n_valid)
    mark()
    totals, sim = _hip.kitti_eval_counts(inp, t, ov, dco, thr, n_thr)
    mark()
    return dict(overlaps=ov, dc_overlaps=dco, tp_scores=tp_sorted, n_valid_gt=n_valid, thresholds=thr, n_thresholds=n_thr,
                n_gt=n_gt, totals=totals, similarity=sim)


# ---- precision and AP ----------------------------------------------------------------------------------------------------
def _ratio(num, den):
    """num / den, 0 where den == 0 (a threshold at which no detection counts)."""
    out = np.zeros(np.broadcast(num, den).shape)
    np.divide(num, den, out=out, where=den != 0)
    return out


def suffix_max(a):
    return np.maximum.accumulate(a[..., ::-1], axis=-1)[..., ::-1]


def ap_r11(prec):
    s = 0.0
    for i in range(0, N_THRESHOLDS, 4):
        s = s + prec[..., i]
    return s / 11 * 100


def ap_r40(prec):
    s = 0.0
    for i in range(1, N_THRESHOLDS):
        s = s + prec[..., i]
    return s / 40 * 100


def evaluate(gt_annos, dt_annos, classes=('Car',), device=None, events=None):
    """KITTI AP of result annotations ``dt_annos`` against ``gt_annos`` (lists of dicts from ``read_kitti_file``, one per
    frame, same order).  Returns

      ap[cls] = [per overlap setting: {'min_overlaps': (2D, BEV, 3D), 'bbox' | 'bev' | '3d' | 'aos':
                 {'R11': [easy, moderate, hard], 'R40': [...]}}]
      curves  = {'keys': [(cls, setting, metric, difficulty)], 'thresholds' (C,41), 'n_thresholds' (C,), 'tp' / 'fp' / 'fn'
                 (C,41) int, 'similarity' (C,41), 'n_gt' (C,)}

    (C = 18 curves per class).  ``events``: as in ``run_device`` (per-stage device times)."""
    dev = device or X.device()
    inp = EvalInput(gt_annos, dt_annos, classes)
    out = run_device(inp, dev, events)
    thr, n_thr, n_gt, totals, sim = (out[k].cpu().numpy() for k in ('thresholds', 'n_thresholds', 'n_gt', 'totals', 'similarity'))
    return assemble(inp.keys, classes, thr, n_thr, n_gt, totals, sim)


def assemble(keys, classes, thr, n_thr, n_gt, totals, sim):
    """The result dict of ``evaluate`` from the curves' totals (host arrays)."""
    tp, fp, fn = (totals[..., k].astype(np.int64) for k in range(3))
    valid = np.arange(N_THRESHOLDS)[None, :] < n_thr[:, None]
    prec = suffix_max(np.where(valid, _ratio(tp, tp + fp), 0.0))
    aos = suffix_max(np.where(valid, _ratio(sim, tp + fp), 0.0))
    r11, r40, a11, a40 = ap_r11(prec), ap_r40(prec), ap_r11(aos), ap_r40(aos)
    ap = {}
    for cls in classes:
        ap[cls] = [dict(min_overlaps=MIN_OVERLAPS[cls.lower()][k]) for k in range(2)]
    for c, (cls, k, metric, d) in enumerate(keys):
        slot = ap[cls][k]
        di = DIFFICULTIES.index(d)
        for name, v11, v40 in ((metric, r11, r40),) + ((('aos', a11, a40),) if metric == 'bbox' else ()):
            e = slot.setdefault(name, {'R11': [0.0] * 3, 'R40': [0.0] * 3})
            e['R11'][di] = float(v11[c])
            e['R40'][di] = float(v40[c])
    curves = dict(keys=list(keys), thresholds=thr, n_thresholds=n_thr, tp=tp, fp=fp, fn=fn, similarity=sim, n_gt=n_gt)
    return dict(ap=ap, curves=curves)


def format_table(result):
    """The familiar text block: per class and overlap setting the R11 lines, then the AP_R40 lines."""
    lines = []
    for cls, settings in result['ap'].items():
        for s in settings:
            mo = ', '.join('%.2f' % v for v in s['min_overlaps'])
            for tag, key in (('AP', 'R11'), ('AP_R40', 'R40')):
                lines.append('%s %s@%s:' % (cls, tag, mo))
                for name, label in (('bbox', 'bbox AP'), ('bev', 'bev  AP'), ('3d', '3d   AP'), ('aos', 'aos  AP')):
                    lines.append('%s:%s' % (label, ', '.join('%.4f' % v for v in s[name][key])))
    return '\n'.join(lines)


def read_dirs(label_dir, result_dir, names):
    """(GT annotations, result annotations) of ``<dir>/<name>.txt`` for every name (a missing file raises)."""
    gt = [read_kitti_file(os.path.join(label_dir, n + '.txt')) for n in names]
    dt = [read_kitti_file(os.path.join(result_dir, n + '.txt')) for n in names]
    return gt, dt


def evaluate_dirs(label_dir, result_dir, names, classes=('Car',), device=None, events=None):
    """``evaluate`` of ``<result_dir>/<name>.txt`` against ``<label_dir>/<name>.txt`` for every name."""
    gt, dt = read_dirs(label_dir, result_dir, names)
    return evaluate(gt, dt, classes, device, events)


def summary(result):
    """JSON-ready {cls: [{'min_overlaps', metric: {'R11', 'R40'}}]} of a result."""
    return {cls: [{k: (list(v) if k == 'min_overlaps' else v) for k, v in s.items()} for s in settings]
            for cls, settings in result['ap'].items()}
