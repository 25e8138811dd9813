"""Test-time augmentation on the GPU (csrc/tta.hip, modules/tta.py, detect.detect_frame_set(tta=...)): the fusion's decisions
exactly and its values within the data path's bars against the float64 reference (tests/tta_ref.py on the cases of
tests/tta_cases.py); identity, empty and repeated runs bitwise; the detection step with views against its manual composition.

Worst distances of test_direct_fuse_matches_the_reference measured on an MI355X (the four parameter sets alike): position
3.78e-6 m, size 5.06e-8 relative, score 0, yaw 1.18e-7 rad."""
import numpy as np
import pytest
import torch

import tta_cases as C
import tta_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')
POS_TOL, REL_TOL, YAW_TOL = 1e-4, 1e-6, 1e-5      # metres, relative (sizes, scores), radians modulo 2 pi
_CASE = {}


def _case():
    if not _CASE:
        _CASE['case'] = C.build()
    return _CASE['case']


def _dev_dets(case):
    n = case['counts'].shape[0]
    meta = torch.zeros((3, n), dtype=torch.int32)
    meta[0] = torch.from_numpy(case['counts'])
    return dict(boxes=torch.from_numpy(case['boxes']).to(DEV), scores=torch.from_numpy(case['scores']).to(DEV), meta=meta.to(DEV))


def _fuse(case, read=True, **kw):
    from modules import tta
    return tta.fuse_views(_dev_dets(case), case['views'], case['F'], iou_thr=C.IOU_THR, fuse_iou=C.FUSE_IOU, read=read, **kw)


def _compare(got, ref):
    """Decisions exactly, values within the bars; returns the worst (position, size, score, yaw) distances."""
    assert got['src'].tolist() == ref['src'].tolist()
    assert got['n_views'].tolist() == ref['n_views'].tolist()
    b, s = got['boxes'].cpu().numpy().astype(np.float64), got['scores'].cpu().numpy().astype(np.float64)
    if b.shape[0] == 0:
        return 0.0, 0.0, 0.0, 0.0
    return (float(np.abs(b[:, :3] - ref['boxes'][:, :3]).max()), float((np.abs(b[:, 3:6] - ref['boxes'][:, 3:6]) / ref['boxes'][:, 3:6]).max()),
            float((np.abs(s - ref['scores']) / ref['scores']).max()), float(R.yaw_distance(b[:, 6], ref['boxes'][:, 6]).max()))


@pytest.mark.parametrize('full_turn', [False, True])
@pytest.mark.parametrize('min_views', [1, 2])
def test_direct_fuse_matches_the_reference(full_turn, min_views):
    case = _case()                              # F = 2, V = 3, post_max = 24: 65 merged entries in frame 0, an empty view in frame 1
    ref = R.fuse(case['boxes'], case['scores'], case['counts'], case['views'], case['F'], C.IOU_THR, C.FUSE_IOU, min_views=min_views,
                 full_turn=full_turn)
    got = _fuse(case, min_views=min_views, full_turn=full_turn)
    assert len(got) == 2
    worst = np.zeros(4)
    for g, r in zip(got, ref):
        assert g['status'] == 0 and g['boxes'].shape[0] == r['boxes'].shape[0] > 0
        worst = np.maximum(worst, _compare(g, r))
    print('tta fuse worst distances (full_turn=%s, min_views=%d): position %.3g m, size %.3g rel, score %.3g rel, yaw %.3g rad'
          % ((full_turn, min_views) + tuple(worst)))
    assert worst[0] <= POS_TOL and worst[1] <= REL_TOL and worst[2] <= REL_TOL and worst[3] <= YAW_TOL
    assert (got[0]['n_views'] == 1).sum().item() == (1 if min_views == 1 else 0)
    pad = _fuse(case, read=False, min_views=min_views, full_turn=full_turn)
    for f, g in enumerate(got):
        n = g['boxes'].shape[0]
        assert pad['meta'][0, f].item() == n
        assert not pad['boxes'][f, n:].any() and not pad['scores'][f, n:].any() and not pad['n_views'][f, n:].any()
        assert (pad['src'][f, n:] == -1).all()


def test_out_max_keeps_the_best_clusters():
    case = _case()
    ref = R.fuse(case['boxes'], case['scores'], case['counts'], case['views'], case['F'], C.IOU_THR, C.FUSE_IOU, out_max=5)
    got = _fuse(case, out_max=5)
    for g, r in zip(got, ref):
        assert g['boxes'].shape[0] == 5
        _compare(g, r)


def test_one_identity_view_returns_the_input_bitwise():
    case = C.build(views=np.array([[0, 1, 0, 0]], np.float32), n_ground=(10,), post_max=16)
    got = _fuse(case)
    assert len(got) == 1
    for f, g in enumerate(got):
        n = int(case['counts'][f])
        keep = R.D.greedy_nms(R.D.corners(case['boxes'][f, :n]), C.IOU_THR, 100)          # the jittered twin of box 0 goes
        assert len(keep) == n - 1 and g['src'].tolist() == keep
        assert np.array_equal(g['boxes'].cpu().numpy(), case['boxes'][f, keep])
        assert np.array_equal(g['scores'].cpu().numpy(), case['scores'][f, keep])
        assert (g['n_views'] == 1).all()


def test_scale_rotation_and_flip_come_back_to_the_planted_box():
    views = np.array([[0.4, 1.07, 1.0, 0.0], [-0.3, 0.93, 0.0, 0.0], [0.0, 1.0, 1.0, 0.0]], np.float32)
    case = C.single_boxes(views)
    for full_turn in (False, True):
        g = _fuse(case, min_views=3, full_turn=full_turn)[0]
        assert g['boxes'].shape[0] == 1 and g['n_views'].tolist() == [3] and g['src'].tolist() == [2 * 4]      # the best score: view 2
        b, p = g['boxes'].cpu().numpy().astype(np.float64)[0], case['ground'][0][0].astype(np.float64)
        assert np.abs(b[:3] - p[:3]).max() <= POS_TOL
        assert (np.abs(b[3:6] - p[3:6]) / p[3:6]).max() <= REL_TOL
        assert R.yaw_distance(b[6], p[6]) <= YAW_TOL
        assert abs(g['scores'].item() - (0.5 + 0.6 + 0.7) / 3) <= REL_TOL * 0.6


def test_empty_frames_give_zero_counts_and_zeroed_padding():
    case = C.build(n_ground=(6,), post_max=8)
    case['counts'][:] = 0
    out = _fuse(case, read=False)
    assert out['meta'].tolist() == [[0], [0]]
    assert not out['boxes'].any() and not out['scores'].any() and not out['n_views'].any() and (out['src'] == -1).all()
    assert out['boxes'].shape == (1, 8, 7)
    got = _fuse(case)
    assert len(got) == 1 and got[0]['boxes'].shape == (0, 7) and got[0]['src'].shape == (0,)


def test_a_non_finite_entry_is_dropped_and_flagged():
    from modules import _hip
    case = C.build(n_ground=(6,), post_max=8)
    clean = _fuse(case)[0]
    assert clean['status'] == 0
    victim = int(clean['src'][0])               # the head of the best cluster
    case['boxes'][victim // 8, victim % 8, 3] = np.inf
    ref = R.fuse(case['boxes'], case['scores'], case['counts'], case['views'], 1, C.IOU_THR, C.FUSE_IOU)[0]
    got = _fuse(case)[0]
    assert ref['bad'] and got['status'] == _hip.TTA_NONFINITE and victim not in got['src'].tolist()
    _compare(got, ref)
    assert torch.isfinite(got['boxes']).all()


def test_two_runs_are_bitwise_identical():
    case = _case()
    a = _fuse(case, read=False, full_turn=True)
    b = _fuse(case, read=False, full_turn=True)
    for k in ('boxes', 'scores', 'n_views', 'src', 'meta'):
        assert torch.equal(a[k], b[k]), k


def _anchors():
    import modules.config as cfg
    from modules.data import Preprocessing as pre
    return pre.createAnchors(cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2, cfg.velorange, cfg.carsize)


def test_detect_frame_set_with_views_is_its_manual_composition():
    import bench
    import modules.config as cfg
    from MVXNet import MVXNet
    from modules import Extension as X
    from modules import tta
    from modules.detect import detect_frame_set, postprocess
    from modules.pipeline import FrameBatch
    batch = bench.make_batch([0, 1], DEV, 20000, 'S2')
    torch.manual_seed(0)
    model = MVXNet().to(DEV)
    anchors = _anchors()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    kw = dict(score_thr=0.3, iou_thr=0.01, post_max=100)
    # tta=None: today's path -- postprocess of the step's own heads, parameters and buffers untouched
    keep = {}
    plain = detect_frame_set(model, batch, anchors, cfg.imsize, keep=keep, tta=None, **kw)
    F, h1, w1 = keep['geom']
    again = postprocess(keep['heads'], anchors, F, h1, w1, **kw)
    assert len(plain) == 2 and min(d['boxes'].shape[0] for d in plain) > 0
    for a, b in zip(plain, again):
        assert sorted(a) == sorted(b) == ['anchor_idx', 'boxes', 'n_candidates', 'scores', 'status']
        assert torch.equal(a['boxes'], b['boxes']) and torch.equal(a['scores'], b['scores']) and torch.equal(a['anchor_idx'], b['anchor_idx'])
    # one identity view: the same lists
    ident = detect_frame_set(model, batch, anchors, cfg.imsize, tta=tta.views(['identity']), **kw)
    for a, b in zip(plain, ident):
        assert torch.equal(a['boxes'], b['boxes']) and torch.equal(a['scores'], b['scores']) and torch.equal(a['anchor_idx'], b['anchor_idx'])
        assert (b['n_views'] == 1).all() and b['src'].tolist() == list(range(b['boxes'].shape[0]))
        assert a['n_candidates'] == b['n_candidates'] and a['status'] == b['status']
    # identity + flip against expand_batch -> plain detection of the four frames -> re-padded -> fuse_views
    names = ['identity', 'flip']
    fused = detect_frame_set(model, batch, anchors, cfg.imsize, tta=names, **kw)
    big = tta.expand_batch(batch, names)
    assert big.n_frames == 4 and big.fpn_levels[0] is batch.fpn_levels[0] and big.fpn_levels[3] is batch.fpn_levels[1]
    pts, n_pts = batch.prepared()
    for f in range(2):                          # the identity views: points, counts and order bitwise the source's
        n = int(n_pts[f])
        assert int(big.n_points[2 * f]) == n and torch.equal(big.points6[2 * f, :n], pts[f, :n])
        assert torch.equal(big.perms[2 * f], batch.perms[f])
        if int(big.n_points[2 * f + 1]) == n:   # nothing fell out of the range: y negated, columns 3..5 not touched
            assert torch.equal(big.points6[2 * f + 1, :n, 1], -pts[f, :n, 1]) and torch.equal(big.points6[2 * f + 1, :n, 3:], pts[f, :n, 3:])
    # (the operand scales of a frame set span its frames: an identity view among four frames is not bitwise that frame among two)
    per = detect_frame_set(model, big, anchors, cfg.imsize, **kw)
    padded = dict(boxes=torch.zeros((4, 100, 7), device=DEV), scores=torch.zeros((4, 100), device=DEV),
                  meta=torch.zeros((3, 4), dtype=torch.int32, device=DEV))
    for k, d in enumerate(per):
        n = d['boxes'].shape[0]
        padded['boxes'][k, :n], padded['scores'][k, :n], padded['meta'][0, k] = d['boxes'], d['scores'], n
    manual = tta.fuse_views(padded, names, 2, iou_thr=0.01, fuse_iou=0.5, min_views=1, full_turn=False)
    assert sum(d['boxes'].shape[0] for d in fused) > 0 and set(fused[0]) == set(plain[0]) | {'n_views', 'src'}
    for f, (a, b) in enumerate(zip(fused, manual)):
        for k in ('boxes', 'scores', 'n_views', 'src'):
            assert torch.equal(a[k], b[k]), k
        view, rank = a['src'] // 100, a['src'] % 100
        for i in range(a['src'].shape[0]):
            assert a['anchor_idx'][i] == per[2 * f + int(view[i])]['anchor_idx'][int(rank[i])]
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k
    # 17 frames do not fit a frame set
    wide = FrameBatch(torch.zeros((17, 8, 6), device=DEV), None, torch.zeros((17,), dtype=torch.int32, device=DEV), [None] * 17)
    with pytest.raises(X.MvxHipError, match=r'17 frames x 1 views = 17 .* 16'):
        detect_frame_set(model, wide, anchors, cfg.imsize, tta=['identity'], **kw)
