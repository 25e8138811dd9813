"""KITTI object evaluation on the GPU (csrc/kitti_eval.hip, modules/kitti_eval.py) against the host reference
(tests/kitti_eval_ref.py): overlap matrices, every curve's thresholds and tp / fp / fn exactly, AP and AOS to 1e-9, on
seeded random splits; bitwise reproducibility; GT scored against itself; detect_like.py --eval end to end; over-limit
frames refused."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kitti_eval_ref as R
import mvx_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _anno(rows):
    from modules.kitti_eval import parse_kitti_lines
    return parse_kitti_lines([' '.join([r[0]] + ['%r' % float(v) for v in r[1:]]) for r in rows])


def random_split(seed, F=48):
    """Frames of 0..12 Cars, Vans, DontCares and Pedestrians (mixed truncation / occlusion, 2D heights across the 25 / 40 px
    limits); detections: jittered copies of the GT whose IoUs straddle 0.5 and 0.7, duplicates, clutter, scores on a 0.05
    grid (ties); some frames without GT or without detections."""
    g = np.random.default_rng(seed)
    gts, dts = [], []
    for f in range(F):
        rows = []
        n = 0 if f % 11 == 3 else int(g.integers(0, 13))
        for _ in range(n):
            name = str(g.choice(['Car', 'Car', 'Car', 'Van', 'DontCare', 'Pedestrian']))
            x1, y1 = g.uniform(0, 1100), g.uniform(120, 250)
            hpx = float(g.choice([25.0, 40.0, 24.5, 39.5, 25.5, 40.5, g.uniform(15, 150)]))
            h, w, l = (1.7, 0.6, 0.8) if name == 'Pedestrian' else (g.uniform(1.4, 1.8), g.uniform(1.5, 1.9), g.uniform(3.4, 4.8))
            rows.append([name, float(g.choice([0.0, 0.1, 0.15, 0.3, 0.45, 0.6])), int(g.integers(0, 4)), g.uniform(-3, 3),
                         x1, y1, x1 + g.uniform(20, 160), y1 + hpx, h, w, l, g.uniform(-25, 25), g.uniform(1.2, 2.0),
                         g.uniform(5, 70), g.uniform(-3.1, 3.1)])
        gts.append(_anno(rows))
        drows = []
        if f % 13 != 5:
            for r in rows:
                if r[0] == 'DontCare' or g.uniform() < 0.15:
                    continue
                d = list(r)
                if r[0] == 'Van' and g.uniform() < 0.5:
                    d[0] = 'Car'
                j = g.uniform(0, 0.35)                       # jitter: BEV / 3D IoU from ~1 down to well below 0.5
                d[11] += g.normal(0, j)
                d[13] += g.normal(0, j)
                d[12] += g.normal(0, j * 0.3)
                d[10] *= 1 + g.normal(0, j * 0.2)
                d[9] *= 1 + g.normal(0, j * 0.2)
                d[14] += g.normal(0, j * 0.5)
                for k in (4, 6):
                    d[k] += g.normal(0, 40 * j)
                d[5] += g.normal(0, 10 * j)
                d[7] += g.normal(0, 10 * j)
                d[3] = r[3] + g.normal(0, 0.3)
                d.append(np.round(g.uniform(0.05, 1.0) * 20) / 20)
                drows.append(d)
                if g.uniform() < 0.15:                       # duplicate
                    drows.append(d[:15] + [np.round(g.uniform(0.05, 1.0) * 20) / 20])
            for _ in range(int(g.integers(0, 5))):           # clutter
                x1, y1 = g.uniform(0, 1100), g.uniform(120, 250)
                drows.append([str(g.choice(['Car', 'Pedestrian'])), -1, -1, g.uniform(-3, 3), x1, y1, x1 + g.uniform(20, 150),
                              y1 + g.uniform(15, 120), 1.6, 1.7, 4.0, g.uniform(-25, 25), 1.6, g.uniform(5, 70),
                              g.uniform(-3.1, 3.1), np.round(g.uniform(0.05, 1.0) * 20) / 20])
            order = g.permutation(len(drows))
            drows = [drows[i] for i in order]
        dts.append(_anno(drows))
    return gts, dts


def _compare_curves(got, ref):
    assert got['keys'] == ref['keys']
    assert np.array_equal(got['n_thresholds'], ref['n_thresholds'])
    assert np.array_equal(got['n_gt'], ref['n_gt'])
    assert np.array_equal(got['thresholds'], ref['thresholds'])
    for name in ('tp', 'fp', 'fn'):
        assert np.array_equal(got[name], ref[name]), name
    assert np.allclose(got['similarity'], ref['similarity'], rtol=0, atol=1e-9)


def _compare_ap(got, ref):
    for cls, settings in ref['ap'].items():
        for k, s in enumerate(settings):
            for metric in ('bbox', 'bev', '3d', 'aos'):
                for key in ('R11', 'R40'):
                    a, b = got['ap'][cls][k][metric][key], s[metric][key]
                    assert np.allclose(a, b, rtol=0, atol=1e-9), (cls, k, metric, key, a, b)


@pytest.mark.parametrize('seed,classes', [(0, ('Car',)), (1, ('Car', 'Pedestrian'))])
def test_overlaps_and_curves_match_the_reference(seed, classes):
    from modules import kitti_eval as ke
    gts, dts = random_split(seed)
    stale = O._oracle_c().oracle_anchor_stale_reads()
    ref = R.evaluate(gts, dts, classes)
    assert O._oracle_c().oracle_anchor_stale_reads() == stale      # the oracle's clipping never read an unwritten slot
    inp = ke.EvalInput(gts, dts, classes)
    out = ke.run_device(inp, DEV)
    ov, dco = out['overlaps'].cpu().numpy(), out['dc_overlaps'].cpu().numpy()
    n_apart = n_clipped = 0
    for f in range(inp.F):
        nd = int(inp.off[0, f + 1] - inp.off[0, f])
        ng = int(inp.off[1, f + 1] - inp.off[1, f])
        nc = int(inp.off[2, f + 1] - inp.off[2, f])
        care = np.char.lower(gts[f]['name'].astype(str)) != 'dontcare'
        p0, q0 = inp.pair_off[0, f], inp.pair_off[1, f]
        for m in range(3):
            dev_m = ov[m, p0:p0 + nd * ng].reshape(ng, nd).T
            assert np.array_equal(dev_m, ref['overlaps'][f][m][:, care]), (f, m)
        apart = ref['apart'][f][:, care]
        n_apart += int(apart.sum())
        n_clipped += int((~apart).sum())
        if apart.any():                 # where the circles are apart the clipped IoU is rounding noise only
            dq = ke.bev_quads_camera(dts[f]['location'], dts[f]['hwl'], dts[f]['rotation_y'])
            gq = ke.bev_quads_camera(gts[f]['location'][care], gts[f]['hwl'][care], gts[f]['rotation_y'][care])
            assert np.abs(O.bbox_pairwise(dq, gq, True)[apart]).max() < 1e-4
            assert (ov[1, p0:p0 + nd * ng].reshape(ng, nd).T[apart] == 0).all()
        assert np.array_equal(dco[q0:q0 + nd * nc].reshape(nc, nd).T, ref['dc_overlaps'][f]), f
    assert n_apart > 0 and n_clipped > 0
    got = ke.assemble(inp.keys, classes, *(out[k].cpu().numpy() for k in ('thresholds', 'n_thresholds', 'n_gt', 'totals',
                                                                              'similarity')))
    _compare_curves(got['curves'], ref['curves'])
    _compare_ap(got, ref)
    assert max(ref['curves']['n_thresholds']) > 10 and ref['curves']['fp'].sum() > 0 and ref['curves']['fn'].sum() > 0
    assert (ref['curves']['similarity'] < 0).any() or (ref['curves']['similarity'] != 0).any()


def test_two_runs_are_bitwise_identical():
    from modules import kitti_eval as ke
    gts, dts = random_split(2)
    inp = ke.EvalInput(gts, dts, ('Car', 'Pedestrian', 'Cyclist'))
    a = ke.run_device(inp, DEV)
    b = ke.run_device(inp, DEV)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_gt_as_detections_scores_hand_derived_values():
    """Every non-DontCare label row returned as a detection with score 1: no FP anywhere, every valid GT a TP; with all
    scores tied the thresholds are n_thr copies of 1.0 and precision is 1 at each, so AP = the share of recall points
    below n_thr (100 when n_gt >= 41).  AOS: every TP adds 1, every frame without a valid GT (tp + fp = 0) adds -1."""
    from modules import kitti_eval as ke
    gts, _ = random_split(3, F=48)
    dts = []
    for a in gts:
        care = np.char.lower(a['name'].astype(str)) != 'dontcare'
        d = {k: v[care] for k, v in a.items()}
        d['score'] = np.ones(int(care.sum()))
        dts.append(d)
    res = ke.evaluate(gts, dts, ('Car', 'Pedestrian'))
    c = res['curves']
    for i, (cls, k, metric, diff) in enumerate(c['keys']):
        n = int(c['n_gt'][i])
        n_thr = len(R.get_thresholds([1.0] * n, n)) if n else 0
        assert c['n_thresholds'][i] == n_thr and (c['thresholds'][i][:n_thr] == 1.0).all()
        assert (c['fp'][i] == 0).all() and (c['tp'][i][:n_thr] == n).all() and (c['fn'][i] == 0).all(), (cls, k, metric, diff)
        r11 = sum(1 for j in range(0, 41, 4) if j < n_thr) / 11 * 100
        r40 = sum(1 for j in range(1, 41) if j < n_thr) / 40 * 100
        e = res['ap'][cls][k][metric]
        d = ke.DIFFICULTIES.index(diff)
        assert e['R11'][d] == pytest.approx(r11, abs=1e-9) and e['R40'][d] == pytest.approx(r40, abs=1e-9)
        if metric == 'bbox':
            empty = sum(1 for gt, dt in zip(gts, dts) if R.clean_data(gt, dt, cls, d)[3] == 0)
            v = (n - empty) / n if n else 0.0
            a = [max(v, 0.0) if n_thr < 41 else v] * n_thr + [0.0] * (41 - n_thr)
            assert c['similarity'][i][0] == (n - empty if n else 0.0)
            assert res['ap'][cls][k]['aos']['R11'][d] == pytest.approx(R.ap_r11(a), abs=1e-9)
            assert res['ap'][cls][k]['aos']['R40'][d] == pytest.approx(R.ap_r40(a), abs=1e-9)
    assert c['n_gt'][2] >= 41 and res['ap']['Car'][0]['3d']['R40'][2] == pytest.approx(100.0)


def test_detect_like_eval_matches_the_reference(tmp_path):
    root = str(tmp_path / 'kitti')
    cmd = [sys.executable, os.path.join(REPO, 'mvxnet-makise_amd', 'detect_like.py'), root, '--synthetic', '8', '--eval',
           '--score-thr', '0.3']
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=REPO)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert 'Car AP@0.70, 0.70, 0.70:' in p.stdout and rec['frames'] == 8
    from modules import kitti_eval as ke
    names = open(os.path.join(root, 'ImageSets', 'train.txt')).read().split()
    gt, dt = ke.read_dirs(os.path.join(root, 'training', 'label_2'), os.path.join(root, 'results', 'data'), names)
    assert sum(len(d['name']) for d in dt) > 0
    ref = R.evaluate(gt, dt, ('Car',))
    for k, s in enumerate(ref['ap']['Car']):
        for metric in ('bbox', 'bev', '3d', 'aos'):
            for key in ('R11', 'R40'):
                assert np.allclose(rec['ap']['Car'][k][metric][key], s[metric][key], rtol=0, atol=1e-9), (k, metric, key)


def test_over_limit_frames_are_refused():
    from modules import Extension as X
    from modules import _hip
    from modules import kitti_eval as ke
    gts, dts = random_split(4, F=4)
    inp = ke.EvalInput(gts, dts, ('Car',))
    t = inp.to(DEV)
    inp.off = inp.off.copy()
    inp.off[0, 2:] += 4097                               # the host offsets claim a frame of 4,097 detections
    with pytest.raises(X.MvxHipError, match='argument error'):
        _hip.kitti_eval_overlaps(inp, t)
    with pytest.raises(X.MvxHipError, match='argument error'):
        _hip.kitti_eval_tp_scores(inp, t, torch.zeros((3, 1), dtype=torch.float64, device=DEV))
    big = [_anno([['Car', 0, 0, 0, 0, 0, 10, 50, 1.5, 1.6, 4, 0, 1.6, 20, 0]] * 1025)]
    with pytest.raises(X.MvxHipError):
        ke.evaluate(big, [_anno([])], ('Car',), DEV)
