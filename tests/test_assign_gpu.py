"""The max-IoU anchor assigner through the C ABI and through Calc at small grids: mvx_assign_anchors_frames (csrc/assign.hip,
DESIGN.md 3.29) on the inputs of tests/assign_cases.py.

References.  The rule: tests/assign_ref.assign_from_iou.  Its IoU table: mvx_bbox_pairwise(gts, anchors, 1) of the same run (an
existing kernel, tested against the truth in test_targets_direct_gpu.py) with the pairs whose bounding circles are apart
(targets_ref.circles_apart32) set to 0 -- every list, count and gt_best bit for bit and in order.  Geometric truth:
assign_ref.truth_table (float64), on the anchors and ground truths that IoUs within targets_cases.IOU_BOUND = 3e-4 of it cannot
decide differently, and gt_best within that bound.

Measured on an MI355X: all 26 tests pass; gt_best within 5.8e-6 of the truth on the three grids.

That the tests can fail: each of these changes to the kernels, built into a scratch library, fails the number of tests given
(the 26 tests of this file, run once against each library).
    ties to the highest g (the key holds g instead of ~g)                            13
    a forced match that does not override (the forced bit ranks below the IoU)         4   (12x10x3 exact and truth, the override
                                                                                          test, more than 1024 pairs)
    the window one cell too small without status 1 (cells of radius R - 1)            1   (the smallest accepted radius)
    a compaction that loses order across workgroups (block b takes the offset of     21
      block nb - 1 - b)
    gi not frame-local (the key holds the global g)                                   7   (frames with a non-empty frame behind
                                                                                          another, Calc replay, Calc, the loader)
    the not-negative list without the forced positives below pos_thr                 13"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import assign_cases as AC
import assign_ref as AR
import targets_cases as C

pytestmark = pytest.mark.gpu
SENT = -7
FSENT = -12345.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _assign(g, bev, R_, off=None, cap=None, slack=0, neg=AC.NEG, pos=AC.POS, force=AC.FORCE):
    """mvx_assign_anchors_frames through the ABI.  ``off``: ground-truth offsets of the frames (default: one frame).  The output
    buffers hold F * 3 * cap + slack (gi: F * cap + slack) elements and start as SENT (gt_best: FSENT).  Returns flat numpy buffers."""
    from modules import Extension as X
    G = bev.shape[0]
    off = [0, G] if off is None else list(off)
    F = len(off) - 1
    A = g['A']
    cap = g['l'] * g['w'] * A if cap is None else cap
    p = torch.full((F * 3 * cap + slack,), SENT, dtype=torch.int64, device='cuda')
    n = torch.full((F * 3 * cap + slack,), SENT, dtype=torch.int64, device='cuda')
    gi = torch.full((F * cap + slack,), SENT, dtype=torch.int64, device='cuda')
    counts = torch.full((F, 2), SENT, dtype=torch.int32, device='cuda')
    best = torch.full((G + 4,), FSENT, dtype=torch.float32, device='cuda')
    status = torch.zeros((1,), dtype=torch.int32, device='cuda')
    nbytes = X.lib.mvx_assign_anchors_frames_workspace_bytes(G, F, g['l'], g['w'], A)
    ws = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device='cuda')           # the workspace arrives dirty
    d_gt = _dev(bev.reshape(G, 8).astype(np.float32)) if G else None
    d_an = _dev(g['bevs'])
    c_off = (ctypes.c_int32 * (F + 1))(*off)
    rc = X.lib.mvx_assign_anchors_frames(X.ptr(d_gt), c_off, F, X.ptr(d_an), g['l'], g['w'], A, float(neg), float(pos), float(force),
                                         int(R_), X.ptr(p), X.ptr(n), X.ptr(gi), cap, X.ptr(counts), X.ptr(best), X.ptr(status),
                                         X.ptr(ws), nbytes, X.stream())
    torch.cuda.synchronize()
    return dict(rc=rc, F=F, cap=cap, G=G, pos=p.cpu().numpy(), neg=n.cpu().numpy(), gi=gi.cpu().numpy(), counts=counts.cpu().numpy(),
                best=best.cpu().numpy(), status=int(status.item()))


def _lists(res, f=0):
    """[px, py, pz, nx, ny, nz, gi] of frame f, and that nothing past the counts was written."""
    cap = res['cap']
    n_pos, n_neg = (int(v) for v in res['counts'][f])
    p = res['pos'][f * 3 * cap:(f + 1) * 3 * cap].reshape(3, cap)
    n = res['neg'][f * 3 * cap:(f + 1) * 3 * cap].reshape(3, cap)
    gi = res['gi'][f * cap:(f + 1) * cap]
    assert (p[:, n_pos:] == SENT).all() and (n[:, n_neg:] == SENT).all() and (gi[n_pos:] == SENT).all()
    return [p[0, :n_pos], p[1, :n_pos], p[2, :n_pos], n[0, :n_neg], n[1, :n_neg], n[2, :n_neg], gi[:n_pos]]


def _table(g, bev):
    """The rule's iou(g, a) of this run: mvx_bbox_pairwise(gts, anchors, 1), 0 where the bounding circles are apart."""
    from modules import _hip
    abev = g['bevs'].reshape(-1, 4, 2)
    if bev.shape[0] == 0:
        return np.zeros((0, abev.shape[0]), np.float32)
    iou = _hip.bbox_pairwise(_dev(bev.astype(np.float32)), _dev(abev), 1).cpu().numpy()
    iou[AC.apart(bev, abev)] = 0.0
    return iou


def _expected(g, bev, neg=AC.NEG, pos=AC.POS, force=AC.FORCE):
    """([px, py, pz, nx, ny, nz, gi], gt_best) from assign_from_iou on the run's own IoU table."""
    r = AR.assign_from_iou(_table(g, bev), neg, pos, force)
    return AR.triples(r['pos'], g['w'], g['A']) + AR.triples(r['notneg'], g['w'], g['A']) + [r['gi']], r['gt_best']


def _same(got, want):
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), 'list %d of (px, py, pz, nx, ny, nz, gi) differs: %s != %s' % (k, a, b)


def _exact(res, g, bev, off=None, **thr):
    """Every frame of a result against the rule on that frame's boxes alone; gt_best bit for bit; the padding untouched."""
    off = [0, bev.shape[0]] if off is None else off
    assert res['rc'] == 0 and res['status'] == 0
    for f in range(len(off) - 1):
        sl = slice(off[f], off[f + 1])
        want, best = _expected(g, bev[sl], **thr)
        _same(_lists(res, f), want)
        assert tuple(res['counts'][f]) == (len(want[6]), len(want[3]))
        assert np.array_equal(res['best'][sl], best)
    assert (res['best'][res['G']:] == FSENT).all()


@functools.lru_cache(maxsize=None)
def _grid_result(name):
    c = AC.case(name)
    return _assign(c['g'], c['bev'], max(c['g']['l'], c['g']['w']))


# ---------------------------------------------------------------------------------------------------------------------------
# exact, truth
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', AC.GRID_CASES)
def test_exact_on_small_grids(name):
    """Corners, centre, a box equal to an anchor (twice), yaw +-pi/4 and a truck; A = 2, 1 and 3."""
    c = AC.case(name)
    res = _grid_result(name)
    _exact(res, c['g'], c['bev'])
    lists = _lists(res)
    flat = AC.flat(lists[0], lists[1], lists[2], c['g'])
    assert np.all(np.diff(flat) > 0) and np.all(np.diff(AC.flat(lists[3], lists[4], lists[5], c['g'])) > 0)
    assert set(lists[2].tolist()) == set(range(c['g']['A']))                 # every orientation has positives
    assert (lists[6] == 5).any() and not (lists[6] == 6).any()               # the repeated box: all to the lower g
    assert (lists[6] == 9).sum() == 1                                        # the truck: its one forced anchor


@pytest.mark.parametrize('name', AC.GRID_CASES)
def test_against_the_truth_where_it_decides(name):
    c = AC.case(name)
    g = c['g']
    res = _grid_result(name)
    lists = _lists(res)
    truth = AC.truth(name)
    ua, ug = AR.undecidable(truth, AC.NEG, AC.POS, AC.FORCE, C.IOU_BOUND)
    assert ua.mean() <= 0.02 and ug.sum() <= 3
    skip = ua | AR.candidates(truth, ug, C.IOU_BOUND)
    want = AR.assign_from_iou(truth, AC.NEG, AC.POS, AC.FORCE)
    got = dict(pos=AC.flat(lists[0], lists[1], lists[2], g), gi=lists[6], notneg=AC.flat(lists[3], lists[4], lists[5], g))
    (pa, ga, na), (pb, gb, nb) = AR.dense(got, c['N']), AR.dense(want, c['N'])
    keep = ~skip
    assert np.array_equal(pa[keep], pb[keep]) and np.array_equal(ga[keep], gb[keep]) and np.array_equal(na[keep], nb[keep])
    err = np.abs(res['best'][:res['G']].astype(np.float64) - want['gt_best'])
    print('%s: gt_best within %.2e of the truth (bound %.0e); %d of %d anchors compared' % (name, err.max(), C.IOU_BOUND, keep.sum(), c['N']))
    assert err.max() <= C.IOU_BOUND
    # every decidable box with a best IoU >= force holds a positive, unless a box with an equal or better claim took its anchor
    for k in np.flatnonzero(~ug):
        if want['forced'][k]:
            assert (lists[6] == k).any(), k


def test_thresholds_only_and_other_thresholds():
    c = AC.case('24x20x2')
    for thr in (dict(force=2.0), dict(neg=0.3, pos=0.3, force=0.25), dict(neg=0.12, pos=0.7, force=0.5)):
        _exact(_assign(c['g'], c['bev'], 24, **thr), c['g'], c['bev'], **thr)
    res = _assign(c['g'], c['bev'], 24, force=2.0)
    assert not np.isin(_lists(res)[6], [6, 7, 8, 9]).any()


def test_a_forced_match_overrides_a_threshold_match():
    """Box 0 lies 0.1 m ahead of the anchor (10, 10, 0): the anchor one cell further on is its positive by threshold (IoU 0.86).  Box
    1, 3.9 x 0.9 m, lies on that second anchor, which is its best (IoU 0.56): the forced match takes the anchor over."""
    c = AC.case('24x20x2')
    g = c['g']
    an = g['anchors']
    a0, a1 = an[10, 10, 0].copy(), an[11, 10, 0].copy()
    a0[0] += np.float32(0.1)
    a1[4] = 0.9
    bev = C.bev(np.stack([a0, a1]))
    res = _assign(g, bev, 24)
    _exact(res, g, bev)
    table = _table(g, bev)
    k = int(AC.flat(11, 10, 0, g))
    assert table[0, k] >= 0.6 > table[1, k] >= 0.1 and table[1].argmax() == k and table[0].argmax() != k
    lists = _lists(res)
    flat = AC.flat(lists[0], lists[1], lists[2], g)
    assert lists[6][flat == k].tolist() == [1] and (lists[6] == 0).sum() >= 2
    thr = _lists(_assign(g, bev, 24, force=2.0))
    assert np.array_equal(AC.flat(thr[0], thr[1], thr[2], g), flat) and not thr[6].any()          # the same anchors, all box 0's


# ---------------------------------------------------------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sizes', [[10], [0, 4, 6], [4, 0, 6], [4, 6, 0], AC.FRAME_SIZES], ids=['F1', 'F3first', 'F3middle', 'F3last', 'F16'])
def test_frames_with_empty_frames_in_place(sizes):
    from modules import Extension as X
    assert len(AC.FRAME_SIZES) == X.MAX_FRAMES
    g = C.grid('24x20x2')
    bev = C.bev(C.many_gts('24x20x2', sum(sizes), seed=21)) if len(sizes) > 3 else AC.case('24x20x2')['bev']
    off = [0] + np.cumsum(sizes).tolist()
    res = _assign(g, bev, 24, off=off)
    _exact(res, g, bev, off)
    for f, n in enumerate(sizes):
        if n == 0:
            assert tuple(res['counts'][f]) == (0, 0)
            continue
        sl = slice(off[f], off[f + 1])
        single = _assign(g, bev[sl], 24)
        _same(_lists(res, f), _lists(single))
        assert np.array_equal(res['best'][sl], single['best'][:n])
        gi = _lists(res, f)[6]
        assert len(gi) > 0 and gi.min() >= 0 and gi.max() < n         # local to the frame


def test_no_box_at_all_touches_only_the_counts():
    from modules import Extension as X
    g = C.grid('24x20x2')
    empty = _assign(g, np.zeros((0, 4, 2), np.float32), 24, off=[0] * (X.MAX_FRAMES + 1))
    assert empty['rc'] == 0 and empty['status'] == 0 and not empty['counts'].any()
    assert (empty['pos'] == SENT).all() and (empty['neg'] == SENT).all() and (empty['gi'] == SENT).all() and (empty['best'] == FSENT).all()


# ---------------------------------------------------------------------------------------------------------------------------
# window
# ---------------------------------------------------------------------------------------------------------------------------
def test_status_bit_1_window_too_small_for_a_truck():
    c = AC.case('24x20x2')
    g = C.grid('120x60x2')
    truck = C.bev(C.grid_gts('120x60x2'))[9:10]
    res = _assign(g, truck, 2)
    assert res['rc'] == 0 and res['status'] == 1
    res = _assign(c['g'], c['bev'][9:10], 2)                        # 0.4 m cells: 2 cells do not cover a 10 m box either
    assert res['rc'] == 0 and res['status'] == 1


def _calc_lists(r):
    return [t.cpu().numpy() for t in list(r[0]) + list(r[1]) + [r[2]]]


def test_calc_replays_with_a_wider_window_and_is_exact(monkeypatch):
    """Calc.assignAnchors[Frames] with a first radius of 2 on 0.1 m cells: status bit 1, doubled until the kernel can show that the
    window gives the dense result -- which is then what it gives."""
    from modules import Calc, _hip
    g = C.grid('120x60x2')
    gt = C.grid_gts('120x60x2')
    bev = C.bev(gt)
    calls = []
    real = _hip.assign_anchors_frames
    monkeypatch.setattr(Calc, '_anchor_radius', lambda *a: 2)
    monkeypatch.setattr(_hip, 'assign_anchors_frames', lambda *a, **k: (calls.append(a[6]), real(*a, **k))[1])
    t_an = torch.from_numpy(g['bevs']).cuda().contiguous()
    info = {}
    pi, ni, gi = Calc.assignAnchors(torch.from_numpy(bev[9:10]), t_an, info=info)
    assert calls[0] == 2 and len(calls) > 2 and calls == sorted(calls) and calls[-1] <= 55
    want, best = _expected(g, bev[9:10])
    _same(_calc_lists((pi, ni, gi)), want)
    assert np.array_equal(info['gt_best'][0].numpy(), best) and len(want[6]) == 1 and info['forced_only'] == 1 and info['none'] == 0
    del calls[:]
    frames = [(torch.from_numpy(bev[:4]), None), None, (torch.from_numpy(bev[4:]), None)]
    out = Calc.assignAnchorsFrames(frames, t_an)
    assert calls[0] == 2 and len(calls) > 2 and out[1] is None
    for r, sl in ((out[0], slice(0, 4)), (out[2], slice(4, 10))):
        _same(_calc_lists(r), _expected(g, bev[sl])[0])


def test_the_smallest_accepted_radius_is_needed():
    """A car 0.19 m ahead of a cell centre, neg = 0.008: the anchor 10 cells on overlaps it by a 0.09 m sliver (IoU 0.012), the one
    11 cells on cannot touch it.  Radius 9 is refused (status 1), radius 10 is accepted and every one of its cells counts."""
    g = C.grid('24x20x2')
    box = g['anchors'][12, 10, 0].copy()
    box[0] += np.float32(0.19)
    bev = C.bev(box[None])
    thr = dict(neg=0.008, pos=0.6, force=0.1)
    assert _assign(g, bev, 9, **thr)['status'] == 1
    res = _assign(g, bev, 10, **thr)
    _exact(res, g, bev, **thr)
    lists = _lists(res)
    listed = set(zip(lists[3].tolist(), lists[4].tolist(), lists[5].tolist()))
    assert (22, 10, 0) in listed and (2, 10, 0) not in listed
    assert 0.008 <= _table(g, bev)[0, int(AC.flat(22, 10, 0, g))] < 0.02


def test_thin_boxes_whose_bounding_circles_nearly_touch():
    """4.0 x 0.4 m anchors on 0.1 m cells: the anchor 32 cells ahead has IoU 0.105 >= force = neg = 0.1 while the two bounding
    circles nearly touch -- a bounding-circle shortcut that is too eager would drop it."""
    g = C.grid('120x60x2thin')
    bev = C.bev(C.thin_gts())
    thr = dict(neg=0.1, pos=0.6, force=0.1)
    res = _assign(g, bev, 55, **thr)
    _exact(res, g, bev, **thr)
    lists = _lists(res)
    assert (72, 30, 0) in set(zip(lists[3].tolist(), lists[4].tolist(), lists[5].tolist()))
    table = _table(g, bev)
    assert 0.1 <= table[0, int(AC.flat(72, 30, 0, g))] < 0.11
    res43 = _assign(g, bev, 43, **thr)                                # the radius Calc derives from the anchor table: still exact
    _exact(res43, g, bev, **thr)


# ---------------------------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------------------------
def test_centre_outside_the_grid_is_no_error_and_the_window_is_clipped():
    g = C.grid('24x20x2')
    rng = g['rng']
    cl, cw = (rng[3] - rng[0]) / g['l'], (rng[4] - rng[1]) / g['w']
    car = [3.9, 1.6, 1.56]
    gt = np.array([[rng[0] - 0.5 * cl, 0.3, -1.0] + car + [0.02],                 # half a cell outside, each side
                   [rng[3] + 0.5 * cl, -0.6, -1.0] + car + [-0.03],
                   [14.0, rng[1] - 0.5 * cw, -1.0] + car + [1.5],
                   [15.0, rng[4] + 0.5 * cw, -1.0] + car + [1.6],
                   [rng[0] - 0.5 * cl, rng[1] - 0.5 * cw, -1.0] + car + [0.0],      # outside both ways
                   [rng[3] + 30.0, rng[4] + 30.0, -1.0] + car + [0.0]], np.float32)  # nowhere near: no anchor, best IoU 0
    bev = C.bev(gt)
    for R_ in (6, 9, 24):
        res = _assign(g, bev, R_)
        assert res['status'] == 0                                             # no bit 4: there is none
        _exact(res, g, bev)
    gi = _lists(res)[6]
    assert set(gi.tolist()) == {0, 1, 2, 3, 4} and res['best'][5] == 0.0


def test_status_bit_2_cap_exceeded():
    c = AC.case('24x20x2')
    want = _lists(_grid_result('24x20x2'))
    n_pos = len(want[6])
    cap = n_pos - 3
    assert 0 < cap < n_pos < len(want[3])
    res = _assign(c['g'], c['bev'], 24, cap=cap, slack=64)
    assert res['rc'] == 0 and res['status'] == 2 and tuple(res['counts'][0]) == (cap, cap)
    _same(_lists(res), [w[:cap] for w in want])
    assert (res['pos'][3 * cap:] == SENT).all() and (res['neg'][3 * cap:] == SENT).all() and (res['gi'][cap:] == SENT).all()
    res = _assign(c['g'], c['bev'], 24, cap=n_pos, slack=64)                  # the positives fit exactly, the not-negatives do not
    assert res['status'] == 2 and tuple(res['counts'][0]) == (n_pos, n_pos)
    _same(_lists(res), want[:3] + [w[:n_pos] for w in want[3:6]] + want[6:])


def test_more_than_1024_pairs_in_one_frame():
    """600 ground truths at A = 2 in ONE frame: 1,200 workgroups of the window kernel, three blocks of the per-box kernel."""
    g = C.grid('24x20x2')
    bev = C.bev(C.many_gts('24x20x2', 600, seed=C.MANY_SEED))
    res = _assign(g, bev, 24)
    _exact(res, g, bev)
    gi = _lists(res)[6]
    assert (gi < 512).any() and (gi >= 512).any()


def test_lists_keep_their_order_across_workgroups():
    """12 x 10 x 3 = 360 anchors is two blocks of the compaction, 24 x 20 x 2 = 960 four: positives in the first and the last."""
    for name in ('12x10x3', '24x20x2'):
        c = AC.case(name)
        lists = _lists(_grid_result(name))
        flat = AC.flat(lists[0], lists[1], lists[2], c['g'])
        assert flat.min() < 256 and flat.max() >= (c['N'] // 256) * 256 and np.all(np.diff(flat) > 0)


# ---------------------------------------------------------------------------------------------------------------------------
# reproducibility
# ---------------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal():
    g = C.grid('24x20x2')
    bev = C.bev(C.many_gts('24x20x2', sum(AC.FRAME_SIZES), seed=21))
    off = [0] + np.cumsum(AC.FRAME_SIZES).tolist()
    a, b = _assign(g, bev, 24, off=off), _assign(g, bev, 24, off=off)
    for k in ('pos', 'neg', 'gi', 'counts', 'best', 'status'):
        assert np.array_equal(a[k], b[k]), k


def test_focal_loss_gradients_are_bitwise_reproducible_with_these_lists():
    """No anchor is listed twice, which is what loss_frames.hip asks for a bitwise reproducible gradient -- and what the reference's
    lists of the same boxes (7 anchors twice) do not give."""
    from modules import Calc
    from modules.voxelnet.FocalLoss import FocalLoss
    c = AC.case('24x20x2')
    g = c['g']
    t_an = torch.from_numpy(g['bevs']).cuda().contiguous()
    frames = [(torch.from_numpy(c['bev']), None), (torch.from_numpy(c['bev'][::-1].copy()), None)]
    lists = Calc.assignAnchorsFrames(frames, t_an)
    for pi, _, _ in lists:
        flat = AC.flat(*(t.cpu().numpy() for t in pi), g)
        assert len(set(flat.tolist())) == len(flat) > 0
    gts = [torch.from_numpy(c['gt']).cuda(), torch.from_numpy(c['gt'][::-1].copy()).cuda()]
    targets = [(t[0], t[1], t[2], gt) for t, gt in zip(lists, gts)]
    heads = torch.randn((2 * g['l'] * g['w'], 16), generator=torch.Generator().manual_seed(5)).cuda()
    anchors = torch.from_numpy(g['anchors']).cuda()
    crit = FocalLoss()
    l1, _, d1 = crit.heads_loss_frames(heads, 2, g['l'], g['w'], targets, anchors)
    l2, _, d2 = crit.heads_loss_frames(heads, 2, g['l'], g['w'], targets, anchors)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(d1).all()) and float(d1.abs().max()) > 0
    assert torch.equal(d1, d2) and torch.equal(l1, l2)


# ---------------------------------------------------------------------------------------------------------------------------
# through Calc and the loader
# ---------------------------------------------------------------------------------------------------------------------------
def test_calc_device_boxes_give_the_lists_of_host_boxes_and_info():
    from modules import Calc
    c = AC.case('24x20x2')
    g = c['g']
    t_an = torch.from_numpy(g['bevs']).cuda().contiguous()
    host = [(torch.from_numpy(c['bev'][:4]), torch.from_numpy(c['gt'][:4, :2])), None, (torch.from_numpy(c['bev'][4:]), None)]
    devf = [None if fr is None else (fr[0].cuda(), None) for fr in host]
    ih, idv = {}, {}
    a, b = Calc.assignAnchorsFrames(host, t_an, info=ih), Calc.assignAnchorsFrames(devf, t_an, info=idv)
    assert a[1] is None and b[1] is None
    for f, sl in ((0, slice(0, 4)), (2, slice(4, 10))):
        _same(_calc_lists(a[f]), _calc_lists(b[f]))
        want, best = _expected(g, c['bev'][sl])
        _same(_calc_lists(a[f]), want)
        assert all(t.is_cuda and t.dtype == torch.int64 for t in list(a[f][0]) + list(a[f][1]) + [a[f][2]])
        assert np.array_equal(ih['gt_best'][f].numpy(), best) and np.array_equal(idv['gt_best'][f].numpy(), best)
    # frame 2 holds the boxes 4..9: the two at +-pi/4 and the truck owe their positive to the forced match, no box is left without
    # a best IoU >= force (the duplicate's best IoU is 1.0: that its anchors went to the other copy is not counted)
    assert ih['gt_best'][1] is None and ih['forced_only'] == idv['forced_only'] == 3 and ih['none'] == idv['none'] == 0
    thr = {}
    Calc.assignAnchorsFrames(host, t_an, forceThr=2.0, info=thr)
    assert thr['forced_only'] == 0 and thr['none'] == 3
    one = Calc.assignAnchors(torch.from_numpy(c['bev'][4:]).cuda(), t_an)
    _same(_calc_lists(one), _calc_lists(a[2]))
    # more frames than a frame set holds: groups of MAX_FRAMES
    many = Calc.assignAnchorsFrames([host[0], None] * 17 + [host[2]], t_an)           # 18 frames with boxes: 16 + 2
    assert len(many) == 35 and many[1] is None and many[33] is None
    for k in (0, 30, 32):
        _same(_calc_lists(many[k]), _calc_lists(a[0]))
    _same(_calc_lists(many[34]), _calc_lists(a[2]))


def test_batch_from_dataset_with_an_assigner_feeds_the_focal_loss(tmp_path):
    import modules.config as cfg
    from modules import Calc, pipeline as pl
    from modules.data import Load, Preprocessing as pre, Synthetic as S
    from modules.voxelnet.FocalLoss import FocalLoss
    import train_like
    root = str(tmp_path / 'kitti')
    S.write_kitti_tree(root, [0, 1], points=3000, raw_points=9000)
    ds = Load.createDataset(['000000', '000001'], root=root)
    dev = torch.device('cuda')
    anchors = pre.createAnchors(cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2, cfg.velorange, cfg.carsize)
    bevs = Calc.bbox3d2bev(anchors.reshape(anchors.shape[:2] + (-1, 7))).to(dev).contiguous()
    seen = []

    def assigner(frames):
        seen.append(len(frames))
        return Calc.assignAnchorsFrames(frames, bevs, 0.45, 0.6, 0.1)
    np.random.seed(0)
    batch, targets = pl.batch_from_dataset(ds, ['000000', '000001'], dev, bevs, train_like.fpn_maps_for, cap_points=3000, assigner=assigner)
    np.random.seed(0)
    _, plain = pl.batch_from_dataset(ds, ['000000', '000001'], dev, bevs, train_like.fpn_maps_for, cap_points=3000)
    assert seen == [2] and len(targets) == 2
    live = [t for t in targets if t is not None]
    assert live and [t is None for t in targets] == [t is None for t in plain]
    for t in live:
        n_box = t[3].shape[0]
        assert len(t[0][0]) >= 1 and set(t[2].tolist()) <= set(range(n_box)) and len(t[1][0]) >= len(t[0][0])
    packed, has_reg = FocalLoss.pack_targets(targets, dev)
    assert has_reg == [t is not None for t in targets]
    assert packed.counts.cpu().tolist() == [[0, 0] if t is None else [len(t[0][0]), len(t[1][0])] for t in targets]
