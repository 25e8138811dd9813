"""CPU-only checks of the KITTI object evaluation (csrc/kitti_eval.hip, modules/kitti_eval.py): the worked checks and every
rule of the metric contract on the host reference (tests/kitti_eval_ref.py); the package's vectorised cleaning and its AP
from curve totals against the reference; the file reader; the C ABI's size query and its argument checks before any
launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

import kitti_eval_ref as R


def anno(rows):
    """Annotation from rows (name, trunc, occl, alpha, (x1, y1, x2, y2), (h, w, l), (x, y, z), ry, score)."""
    from modules.kitti_eval import parse_kitti_lines
    lines = [' '.join([r[0]] + [repr(float(v)) for v in (r[1], r[2], r[3]) + tuple(r[4]) + tuple(r[5]) + tuple(r[6]) + (r[7], r[8])])
             for r in rows]
    return parse_kitti_lines(lines)


def car(x1=100.0, y1=100.0, x2=200.0, y2=200.0, x=0.0, z=20.0, ry=0.0, name='Car', trunc=0.0, occl=0, alpha=0.0, score=0.0,
        l=4.0, w=1.6, h=1.5, y=1.6):
    return (name, trunc, occl, alpha, (x1, y1, x2, y2), (h, w, l), (x, y, z), ry, score)


def _ap(result, cls='Car', k=0, metric='bbox'):
    return result['ap'][cls][k][metric]


# ---- the two worked checks ---------------------------------------------------------------------------------------------
def test_worked_check_single_car():
    res = R.evaluate([anno([car()])], [anno([car(score=0.9)])])
    for metric in ('bbox', 'bev', '3d', 'aos'):
        for k in range(2):
            e = _ap(res, k=k, metric=metric)
            assert e['R11'] == [100 / 11] * 3 and e['R40'] == [0.0] * 3, (metric, k, e)


def test_worked_check_forty_cars():
    gts, dts = [], []
    for i in range(40):
        c = car(x=3.0 * i - 60.0, x1=10.0 * i, x2=10.0 * i + 8.0)
        gts.append(anno([c]))
        dts.append(anno([c[:8] + (0.5 + 0.01 * i,)]))
    res = R.evaluate(gts, dts)
    for metric in ('bbox', 'bev', '3d', 'aos'):
        e = _ap(res, metric=metric)
        assert np.allclose(e['R11'], 1000 / 11, rtol=0, atol=1e-12) and np.allclose(e['R40'], 97.5, rtol=0, atol=1e-12), (metric, e)


# ---- one rule per case ---------------------------------------------------------------------------------------------------
def _stat(gt_rows, dt_rows, metric=0, min_overlap=0.7, diff=0, thresh=0.0, compute_fp=True, cls='Car'):
    gt, dt = anno(gt_rows), anno(dt_rows)
    ig, idt, dc, _ = R.clean_data(gt, dt, cls, diff)
    ovs, _ = R.frame_overlaps(dt, gt)
    dco = R.image_iou(dt['bbox'], dc, dontcare=True)
    return R.compute_statistic(ovs[metric], gt, dt, ig, idt, dco, metric, min_overlap, thresh, compute_fp)


def test_van_matched_by_a_car_detection_is_neither_tp_nor_fp():
    tp, fp, fn, _, _ = _stat([car(name='Van')], [car(score=0.8)])
    assert (tp, fp, fn) == (0, 0, 0)


def test_dontcare_absorbs_a_false_positive_on_2d_only():
    gt = [car(name='DontCare', x1=90.0, y1=90.0, x2=250.0, y2=250.0, x=-30.0)]
    dt = [car(score=0.8)]
    assert _stat(gt, dt, metric=0)[:3] == (0, 0, 0)
    assert _stat(gt, dt, metric=1, min_overlap=0.5)[:3] == (0, 1, 0)
    assert _stat(gt, dt, metric=2, min_overlap=0.5)[:3] == (0, 1, 0)


def test_gt_heights_at_the_limits_are_excluded_by_le():
    for diff, hmin in ((0, 40.0), (1, 25.0)):
        at = R.clean_data(anno([car(y2=100.0 + hmin)]), anno([]), 'Car', diff)
        above = R.clean_data(anno([car(y2=100.0 + hmin + 0.01)]), anno([]), 'Car', diff)
        assert at[0] == [1] and at[3] == 0
        assert above[0] == [0] and above[3] == 1


def test_detection_heights_at_the_limits_are_kept_by_lt():
    for diff, hmin in ((0, 40.0), (1, 25.0)):
        at = R.clean_data(anno([]), anno([car(y2=100.0 + hmin)]), 'Car', diff)
        below = R.clean_data(anno([]), anno([car(y2=100.0 + hmin - 0.01)]), 'Car', diff)
        assert at[1] == [0] and below[1] == [1]


def test_a_duplicate_detection_is_a_false_positive():
    assert _stat([car()], [car(score=0.8), car(score=0.7)])[:3] == (1, 1, 0)


def test_tied_scores_take_the_lower_index():
    # GT A overlaps detections 0 and 1 (same score); GT B only detection 1: A must take 0, so B finds 1
    gt = [car(x1=100.0, x2=200.0, x=0.0), car(x1=120.0, x2=220.0, x=0.5)]
    dt = [car(x1=100.0, x2=200.0, x=0.0, score=0.8), car(x1=110.0, x2=210.0, x=0.25, score=0.8)]
    ov = R.frame_overlaps(anno(dt), anno(gt))[0][0]
    assert ov[0, 0] > 0.7 and ov[1, 0] > 0.7 and ov[1, 1] > 0.7 and ov[0, 1] < 0.7
    tp, fp, fn, _, scores = _stat(gt, dt, compute_fp=False)
    assert (tp, fn) == (2, 0) and scores == [0.8, 0.8]


def test_aos_counts_minus_one_for_a_frame_without_tp_and_fp():
    one = R.evaluate([anno([car(alpha=0.3)])], [anno([car(score=0.9, alpha=0.3)])])
    two = R.evaluate([anno([car(alpha=0.3)]), anno([])], [anno([car(score=0.9, alpha=0.3)]), anno([])])
    assert _ap(one, metric='aos')['R11'][0] == pytest.approx(100 / 11)
    assert _ap(two, metric='bbox')['R11'][0] == pytest.approx(100 / 11)
    assert _ap(two, metric='aos')['R11'][0] == 0.0                 # (1 + (-1)) / 1
    c = two['curves']
    assert c['similarity'][0][0] == 0.0 and c['tp'][0][0] == 1 and c['fp'][0][0] == 0


# ---- package host code against the reference ---------------------------------------------------------------------------
def _random_frames(seed, F=6):
    g = np.random.default_rng(seed)
    gts, dts = [], []
    for _ in range(F):
        rows = []
        for _ in range(g.integers(0, 6)):
            x1, y1 = g.uniform(0, 1000), g.uniform(100, 300)
            rows.append(car(name=str(g.choice(['Car', 'Van', 'Pedestrian', 'DontCare'])), x1=x1, y1=y1, x2=x1 + g.uniform(5, 150),
                            y2=y1 + g.choice([25.0, 40.0, g.uniform(10, 120)]), x=g.uniform(-20, 20), z=g.uniform(5, 60),
                            ry=g.uniform(-3, 3), trunc=g.choice([0.0, 0.2, 0.4, 0.8]), occl=int(g.integers(0, 4)),
                            alpha=g.uniform(-3, 3)))
        gts.append(anno(rows))
        drows = [r[:8] + (float(np.round(g.uniform(0, 1), 2)),) for r in rows if r[0] != 'DontCare' and g.uniform() < 0.8]
        dts.append(anno(drows))
    return gts, dts


def test_package_cleaning_flags_equal_the_reference():
    from modules.kitti_eval import EvalInput
    gts, dts = _random_frames(3, F=12)
    inp = EvalInput(gts, dts, ('Car', 'Pedestrian'))
    for ci, cls in enumerate(('Car', 'Pedestrian')):
        for d in range(3):
            ig, idt = [], []
            for gt, dt in zip(gts, dts):
                a, b, _, _ = R.clean_data(gt, dt, cls, d)
                care = [n.lower() != 'dontcare' for n in gt['name']]
                ig += [v for v, c in zip(a, care) if c]
                idt += b
            assert inp.ignored_gt[ci * 3 + d].tolist() == ig and inp.ignored_det[ci * 3 + d].tolist() == idt
    assert inp.off[:, -1].tolist() == [len(inp.det_rows), len(inp.gt_rows), len(inp.dc_rows)]


def test_package_ap_from_totals_equals_the_reference():
    from modules.kitti_eval import assemble, curve_table
    gts, dts = _random_frames(4)
    ref = R.evaluate(gts, dts, ('Car',))
    c = ref['curves']
    keys, _, _ = curve_table(('Car',))
    assert keys == c['keys']
    totals = np.stack([c['tp'], c['fp'], c['fn']], -1).astype(np.int32)
    got = assemble(keys, ('Car',), c['thresholds'], c['n_thresholds'], c['n_gt'], totals, c['similarity'])
    for k in range(2):
        for metric in ('bbox', 'bev', '3d', 'aos'):
            for key in ('R11', 'R40'):
                assert np.allclose(got['ap']['Car'][k][metric][key], ref['ap']['Car'][k][metric][key], rtol=0, atol=1e-9)


def test_format_table_lists_every_metric():
    from modules.kitti_eval import assemble, curve_table, format_table
    keys, _, _ = curve_table(('Car',))
    C = len(keys)
    res = assemble(keys, ('Car',), np.zeros((C, 41)), np.zeros(C, np.int64), np.zeros(C, np.int64), np.zeros((C, 41, 3), np.int32),
                   np.zeros((C, 41)))
    text = format_table(res).splitlines()
    assert text[0] == 'Car AP@0.70, 0.70, 0.70:' and text[1] == 'bbox AP:0.0000, 0.0000, 0.0000'
    assert text[2].startswith('bev  AP:') and text[3].startswith('3d   AP:') and text[4].startswith('aos  AP:')
    assert text[5] == 'Car AP_R40@0.70, 0.70, 0.70:' and text[10] == 'Car AP@0.70, 0.50, 0.50:' and len(text) == 20


def test_eval_input_refuses_frames_over_the_limits():
    from modules import Extension as X
    from modules.kitti_eval import EvalInput
    with pytest.raises(X.MvxHipError):
        EvalInput([anno([])], [anno([car(score=0.5)] * 4097)], ('Car',))
    with pytest.raises(X.MvxHipError):
        EvalInput([anno([car()] * 600 + [car(name='DontCare')] * 425)], [anno([])], ('Car',))
    with pytest.raises(ValueError):
        EvalInput([anno([])], [anno([])], ('Truck',))


# ---- files ---------------------------------------------------------------------------------------------------------------
def test_read_kitti_file_rows_dontcare_empty_and_missing(tmp_path):
    from modules.kitti_eval import read_kitti_file
    p = tmp_path / 'a.txt'
    p.write_text('Car 0.00 0 -1.57 599.41 156.40 629.75 189.25 2.85 2.63 12.34 0.47 1.49 69.44 -1.56\n'
                 'DontCare -1 -1 -10.00 503.89 169.71 590.61 190.13 -1.00 -1.00 -1.00 -1000.00 -1000.00 -1000.00 -10.00\n')
    a = read_kitti_file(str(p))
    assert a['name'].tolist() == ['Car', 'DontCare'] and a['bbox'].shape == (2, 4) and a['score'].tolist() == [0.0, 0.0]
    assert a['hwl'][0].tolist() == [2.85, 2.63, 12.34] and a['location'][0].tolist() == [0.47, 1.49, 69.44]
    assert a['rotation_y'][0] == -1.56 and a['alpha'][0] == -1.57 and a['occluded'][1] == -1
    e = tmp_path / 'e.txt'
    e.write_text('')
    assert len(read_kitti_file(str(e))['name']) == 0
    with pytest.raises(FileNotFoundError, match='missing.txt'):
        read_kitti_file(str(tmp_path / 'missing.txt'))


def test_written_results_read_back(tmp_path):
    import modules.config as cfg
    from modules.data import Synthetic as S
    from modules.detect import write_kitti_results
    from modules.kitti_eval import annos_from_detections, read_kitti_file
    calib = {k: torch.Tensor(np.asarray(v)) for k, v in S.KITTI_CALIB.items()}
    g = np.random.default_rng(2)
    n = 6
    boxes = torch.tensor(np.stack([g.uniform(5, 60, n), g.uniform(-20, 20, n), g.uniform(-2, 0, n), g.uniform(3, 5, n),
                                   g.uniform(1.4, 2, n), g.uniform(1.3, 1.9, n), g.uniform(-3, 3, n)], 1), dtype=torch.float32)
    dets = {'boxes': boxes, 'scores': torch.tensor(g.uniform(0.05, 1, n), dtype=torch.float32)}
    write_kitti_results(str(tmp_path / 'r.txt'), dets, calib, cfg.imsize)
    disk = read_kitti_file(str(tmp_path / 'r.txt'))
    mem = annos_from_detections(dets, calib, cfg.imsize)
    assert disk['name'].tolist() == ['Car'] * n
    for k in disk:
        assert np.array_equal(disk[k], mem[k]), k
    assert np.allclose(disk['score'], dets['scores'].numpy(), atol=5e-5)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
def test_kitti_eval_symbols_and_workspace_query():
    from modules import Extension as X
    lib = ctypes.CDLL(X.LIB_PATH)
    for name in ('mvx_kitti_eval_workspace_bytes', 'mvx_kitti_eval_overlaps', 'mvx_kitti_eval_tp_scores',
                 'mvx_kitti_eval_thresholds', 'mvx_kitti_eval_counts'):
        assert hasattr(lib, name) and name in X.PROTOTYPES
    assert X.ABI_VERSION == 10 and X.lib.mvx_abi_version() == 10
    one = X.lib.mvx_kitti_eval_workspace_bytes(3769, 18)
    assert one >= 3769 * 18 * 41 * 20
    assert X.lib.mvx_kitti_eval_workspace_bytes(3769, 54) > 2 * one


FAKE = ctypes.c_void_p(1 << 20)


def _off(nd, ng, nc):
    z = [0]
    off = np.array([np.concatenate([z, np.cumsum(v)]) for v in (nd, ng, nc)], np.int32)
    return off, off.ctypes.data_as(ctypes.c_void_p)


def _curves(metric=0, s=0, mo=0.7, n=18):
    c = np.array([[metric, s]] * n, np.int32)
    m = np.array([mo] * n, np.float64)
    return c, m


def _counts(off_host, curves, mo, n_sets=3, ws_bytes=1 << 40, ws=FAKE, F=None, n_curves=None):
    from modules import Extension as X
    F = off_host[0].shape[1] - 1 if F is None else F
    n_curves = len(curves[0]) if n_curves is None else n_curves
    return X.lib.mvx_kitti_eval_counts(F, off_host[1], FAKE, FAKE, n_curves, curves[0].ctypes.data_as(ctypes.c_void_p),
                                       mo.ctypes.data_as(ctypes.c_void_p), n_sets, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE,
                                       FAKE, FAKE, FAKE, ws, ws_bytes, None)


@pytest.mark.parametrize('case', ['dets', 'gt_dc', 'frames', 'metric', 'set', 'curves', 'min_overlap', 'workspace', 'aligned'])
def test_kitti_eval_rejects_bad_arguments_before_any_launch(case):
    from modules import Extension as X
    nd, ng, nc = [100, 5], [10, 7], [2, 0]
    metric, s, mo, n = 0, 0, 0.7, 18
    kw = {}
    if case == 'dets':
        nd = [100, 4097]
    elif case == 'gt_dc':
        ng, nc = [10, 1000], [2, 25]
    elif case == 'frames':
        kw['F'] = 0
    elif case == 'metric':
        metric = 3
    elif case == 'set':
        s = 3
    elif case == 'curves':
        n = 73
    elif case == 'min_overlap':
        mo = 1.0
    elif case == 'workspace':
        kw['ws_bytes'] = 1024
    elif case == 'aligned':
        kw['ws'] = ctypes.c_void_p((1 << 20) + 8)
    off = _off(nd, ng, nc)
    curves = _curves(metric, s, mo, n)
    assert _counts(off, curves, curves[1], **kw) == -1
    if case in ('dets', 'gt_dc', 'frames'):
        F = kw.get('F', 2)
        assert X.lib.mvx_kitti_eval_overlaps(F, off[1], FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None) == -1
    if case in ('dets', 'gt_dc', 'frames', 'metric', 'set', 'curves', 'min_overlap'):
        assert X.lib.mvx_kitti_eval_tp_scores(kw.get('F', 2), off[1], FAKE, FAKE, n, curves[0].ctypes.data_as(ctypes.c_void_p),
                                              curves[1].ctypes.data_as(ctypes.c_void_p), 3, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE,
                                              None) == -1


def test_kitti_eval_rejects_missing_pointers():
    from modules import Extension as X
    off = _off([3, 0], [2, 4], [1, 1])
    assert X.lib.mvx_kitti_eval_overlaps(2, off[1], FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, None) == -1
    assert X.lib.mvx_kitti_eval_overlaps(2, off[1], None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None) == -1
    assert X.lib.mvx_kitti_eval_overlaps(2, None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None) == -1
    assert X.lib.mvx_kitti_eval_thresholds(2, 0, 5, FAKE, FAKE, FAKE, FAKE, FAKE, None) == -1
    assert X.lib.mvx_kitti_eval_thresholds(2, 18, 5, None, FAKE, FAKE, FAKE, FAKE, None) == -1
    bad = np.array([[1, 3, 3], [0, 2, 6], [0, 1, 2]], np.int32)            # offsets must start at 0
    assert X.lib.mvx_kitti_eval_overlaps(2, bad.ctypes.data_as(ctypes.c_void_p), FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE,
                                         FAKE, None) == -1
    assert math.isfinite(float(X.lib.mvx_kitti_eval_workspace_bytes(0, 0)))
