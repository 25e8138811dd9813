"""CPU checks of the label-path test material: the reference-arithmetic oracle (oracle/anchors_c.c) against the float64 truth
tests/targets_ref.py on the box pairs of tests/targets_cases.py -- which defines the IoU tolerance of
tests/test_targets_direct_gpu.py --, the bounding-circle shortcut, voxel_loss64 against torch, and every case against its own
name."""
import math

import numpy as np
import torch

import mvx_oracle as O
import targets_cases as C
import targets_ref as R


def _round_up_one_digit(v):
    e = 10.0 ** math.floor(math.log10(v))
    return math.ceil(v / e - 1e-9) * e


def test_truth_on_configurations_known_in_closed_form():
    known = {'identical': (8.0, 1.0), 'shared_full_edge': (0.0, 0.0), 'shared_partial_edge': (0.0, 0.0),
             'corner_touches_corner': (0.0, 0.0), 'corner_on_edge': (0.0, 0.0), 'corner_on_edge_inside': (2.0, 0.25),
             'one_inside_the_other': (2.0, 0.25), 'cross_0_over_90': (4.0, 1.0 / 3.0), 'disjoint_1mm': (0.0, 0.0),
             'clockwise_first': (4.5, 4.5 / 11.5), 'clockwise_second': (4.5, 4.5 / 11.5)}
    seen = set()
    for n, _, _, _, t_iou, t_inter in C.pair_table():
        key = n.split('@')[0]
        if key in known:
            seen.add(key)
            assert t_inter == known[key][0] and abs(t_iou - known[key][1]) < 1e-15, n
    assert seen == set(known)
    # independent of the origin: the same configuration gives the same truth at the three placements
    for key in ('45_over_0', 'clockwise_both'):
        vals = [(t_iou, t_inter) for n, _, _, _, t_iou, t_inter in C.pair_table() if n.split('@')[0] == key]
        assert len(vals) == 3 and vals[0] == vals[1] == vals[2]


def test_oracle_against_the_truth_defines_the_iou_bound():
    rows = C.pair_table()
    stale = [r for r in rows if r[3] > 0]
    clean = [r for r in rows if r[3] == 0]
    assert len(stale) >= 5, [r[0] for r in stale]
    assert sum(r[0].startswith('along_fan_line_leftover/') for r in stale) == 4
    assert len(clean) >= 100
    e_iou = max(abs(r[1] - r[4]) for r in clean)
    e_inter = max(abs(r[2] - r[5]) for r in clean)
    print('oracle on %d clean pairs: max IoU error %.3e, max intersection error %.3e; %d stale pairs' % (len(clean), e_iou, e_inter, len(stale)))
    assert e_iou <= C.IOU_BOUND and e_inter <= C.INTER_BOUND
    # the derivation of the bounds from the recorded measurement
    assert abs(C.IOU_BOUND - _round_up_one_digit(4 * C.MEASURED_IOU)) < 1e-12
    assert abs(C.INTER_BOUND - _round_up_one_digit(4 * C.MEASURED_INTER)) < 1e-12
    assert e_iou <= 1.01 * C.MEASURED_IOU + 1e-6 and e_inter <= 1.01 * C.MEASURED_INTER + 1e-5


def test_circles_apart_only_skips_empty_intersections():
    _, qa, qb = C.pair_arrays()
    ra, rb = C.random_pairs(20000, seed=5)
    qa, qb = np.concatenate([qa, ra]), np.concatenate([qb, rb])
    apart = R.circles_apart32(qa, qb)
    assert 2000 < int(apart[-20000:].sum()) < 18000                 # the random set probes both sides of the test
    for a, b in zip(qa[apart], qb[apart]):
        assert R.poly_iou64(a, b)[0] == 0.0
    # and the truth is not 0 throughout: of the random pairs it does NOT skip, a good part do intersect
    kept = np.flatnonzero(~apart[-20000:])[:500]
    assert sum(R.poly_iou64(ra[k], rb[k])[0] > 0 for k in kept) > 100


def test_voxel_loss64_agrees_with_the_torch_restatement():
    c = C.loss_small('5x7x2')
    losses, _, _ = R.voxel_loss64(c['score'], c['reg'], c['pos'], c['neg'], c['gi'], c['gts'], c['anchors'])
    cls, rl = O.voxel_loss(tuple(c['pos']), tuple(c['neg']), c['gi'], torch.from_numpy(c['gts']), torch.from_numpy(c['score']),
                           torch.from_numpy(c['reg']), torch.from_numpy(c['anchors']).reshape(c['L'], c['W'], -1), c['A'])
    assert abs(losses[0] - float(cls.detach())) < 1e-5 * abs(float(cls.detach()))
    assert abs(losses[1] - float(rl.detach())) < 1e-5 * abs(float(rl.detach()))


def test_voxel_loss64_closed_form_gradients_agree_with_autograd():
    for c in (C.loss_small('12x10x3'), C.loss_kink()):
        L, W, A = c['L'], c['W'], c['A']
        losses, ds, dr = R.voxel_loss64(c['score'], c['reg'], c['pos'], c['neg'], c['gi'], c['gts'], c['anchors'], f32_roundings=False)
        score = torch.from_numpy(c['score']).double().requires_grad_(True)
        reg = torch.from_numpy(c['reg']).double().requires_grad_(True)
        eps = float(np.float32(1e-6))
        pi, ni = tuple(torch.from_numpy(c['pos'])), tuple(torch.from_numpy(c['neg']))
        neg_all = -torch.log(1 - score + eps)
        cls = 1.5 * (-torch.log(score[pi] + eps).sum() / (len(pi[0]) + eps)) + (neg_all.sum() - neg_all[ni].sum()) / (L * W * A - len(ni[0]) + eps)
        g = torch.from_numpy(c['gts']).double()[torch.from_numpy(c['gi'])]
        an = torch.from_numpy(c['anchors']).double()[pi]
        d = torch.sqrt(an[:, 3] ** 2 + an[:, 4] ** 2)[:, None]
        t = torch.cat([(g[:, :2] - an[:, :2]) / d, ((g[:, 2] - an[:, 2]) / an[:, 5])[:, None], torch.log(g[:, 3:6] / an[:, 3:6]),
                       (g[:, 6] - an[:, 6])[:, None]], dim=1)
        rl = torch.nn.functional.smooth_l1_loss(reg.reshape(L, W, A, 7)[pi], t)
        (cls + rl).backward()
        assert abs(losses[0] - float(cls.detach())) < 1e-10 * abs(float(cls.detach())) and abs(losses[1] - float(rl.detach())) < 1e-10 * abs(float(rl.detach()))
        np.testing.assert_allclose(ds, score.grad.numpy(), rtol=1e-10, atol=1e-16)
        np.testing.assert_allclose(dr, reg.grad.numpy(), rtol=1e-10, atol=1e-16)


def test_box_pair_table_satisfies_its_names():
    names, qa, qb = C.pair_arrays()
    assert len(names) == len(set(names))
    for key in ('identical', 'shared_full_edge', 'shared_partial_edge', 'corner_touches_corner', 'corner_on_edge',
                'one_inside_the_other', 'cross_0_over_90', '45_over_0', 'sliver_1e-4', 'disjoint_1mm', 'clockwise_first'):
        assert sum(n.split('@')[0] == key for n in names) == 3, key
    assert sum(n.startswith('random/') for n in names) == 64
    by = {n: (a.astype(np.float64), b.astype(np.float64)) for n, a, b in zip(names, qa, qb)}
    area = R._area64
    for tag, (x, y) in C.PLACEMENTS.items():
        a, b = by['identical@' + tag]
        assert np.array_equal(a, b)
        a, b = by['shared_full_edge@' + tag]
        assert np.array_equal(a[[3, 0]], b[[2, 1]])                 # a's right edge IS b's left edge, to the bit
        a, b = by['shared_partial_edge@' + tag]
        assert a[0, 0] == b[1, 0] and b[2, 1] > a[3, 1] and b[2, 1] < a[0, 1] < b[1, 1]
        a, b = by['corner_touches_corner@' + tag]
        assert np.array_equal(a[0], b[2])
        a, b = by['corner_on_edge@' + tag]
        assert b[2, 0] == a[0, 0] and a[3, 1] < b[2, 1] < a[0, 1]   # b's left corner ON a's right edge
        a, b = by['sliver_1e-4@' + tag]
        assert 0.5e-4 < a[0, 0] - b[1, 0] < 1.5e-4
        a, b = by['disjoint_1mm@' + tag]
        assert 0.9e-3 < b[1, 0] - a[0, 0] < 1.1e-3
        assert area(by['clockwise_first@' + tag][0]) < 0 < area(by['clockwise_first@' + tag][1])
        assert area(by['clockwise_second@' + tag][1]) < 0 and area(by['clockwise_both@' + tag][0]) < 0 > area(by['clockwise_both@' + tag][1])
    a = by['edge_through_origin/itself'][0]
    assert a[1, 0] == 0 == a[2, 0] and a[1, 1] > 0 > a[2, 1]
    assert np.array_equal(by['corner_at_origin/itself'][0][2], [0, 0])
    a = by['contains_origin/itself'][0]
    assert a[:, 0].min() < 0 < a[:, 0].max() and a[:, 1].min() < 0 < a[:, 1].max()
    # every coordinate of the degenerate configurations is a multiple of 2^-2: exact in f32 up to 2^22
    for n, (a, b) in by.items():
        if n.split('@')[0] in ('identical', 'shared_full_edge', 'shared_partial_edge', 'corner_touches_corner', 'corner_on_edge',
                               'one_inside_the_other', 'cross_0_over_90', '45_over_0') or '_origin/' in n:
            assert np.array_equal(a * 4, np.round(a * 4)) and np.array_equal(b * 4, np.round(b * 4)), n


def test_grids_and_ground_truths_satisfy_their_names():
    for name, (l, w, A, rng) in C.GRIDS.items():
        g = C.grid(name)
        assert g['anchors'].shape == (l, w, A, 7) and g['bevs'].shape == (l, w, A, 4, 2) and rng != O.VELORANGE
        if name.endswith('thin'):
            continue
        gt = C.grid_gts(name)
        nls, nws = C.centre_cells(g, gt)
        assert (nls >= 0).all() and (nls < l).all() and (nws >= 0).all() and (nws < w).all()
        assert {(0, 0), (0, w - 1), (l - 1, 0), (l - 1, w - 1)} <= set(zip(nls.tolist(), nws.tolist()))
        assert np.array_equal(gt[5], gt[6]) and np.array_equal(gt[5], g['anchors'][l // 3, w // 3, 0])
        assert abs(gt[7, 6] - np.pi / 4) < 1e-6 and abs(gt[8, 6] + np.pi / 4) < 1e-6 and gt[9, 3] >= 10.0
    assert np.allclose(C.grid('12x10x3')['anchors'][0, 0, :, 6], [0, np.pi / 2, np.pi / 4])
    g = C.grid('120x60x2')
    assert abs((g['anchors'][1, 0, 0, 0] - g['anchors'][0, 0, 0, 0]) - 0.1) < 1e-5


def test_classify_inputs_are_free_of_stale_reads():
    """The GPU tests compare with the oracle by array_equal, which needs inputs on which it consumes no stale slot."""
    lib = O._oracle_c()
    before = lib.oracle_anchor_stale_reads()
    for name in C.GRIDS:
        g = C.grid(name)
        gt = C.grid_gts(name)
        nls, nws = C.centre_cells(g, gt)
        pi, ni, gi = O.classify_anchors_cells(C.bev(gt), g['bevs'], nls, nws, 0.45, 0.6)
        assert len(gi) > 0 and len(ni[0]) > len(gi)
    g = C.grid('120x60x2thin')
    gt = C.thin_gts()
    nls, nws = C.centre_cells(g, gt)
    _, ni, _ = O.classify_anchors_cells(C.bev(gt), g['bevs'], nls, nws, 0.1, 0.6)
    assert (nls[0], nws[0]) == (40, 30) and (72, 30, 0) in set(zip(*[c.tolist() for c in ni]))
    d = float(np.float32(3.24))
    assert d > 0.8 * 2 * math.hypot(2.0, 0.2) + 1e-3 and d < 1.01 * 2 * math.hypot(2.0, 0.2)
    g = C.grid('24x20x2')
    gt = C.many_gts('24x20x2', 600, seed=C.MANY_SEED)
    nls, nws = C.centre_cells(g, gt)
    pi, ni, gi = O.classify_anchors_cells(C.bev(gt), g['bevs'], nls, nws, 0.45, 0.6)
    assert lib.oracle_anchor_stale_reads() == before
    # more than 1024 (ground truth, orientation) pairs, and both trips of the concatenation hold positives and non-negatives
    assert gt.shape[0] * g['A'] > 1024
    assert (gi < 512).any() and (gi >= 512).any() and len(ni[0]) > len(gi)


def test_loss_cases_satisfy_their_names():
    for name, (L, W, A) in C.LOSS_GRIDS.items():
        c = C.loss_small(name)
        assert c['score'].shape == (L, W, A) and c['reg'].shape == (L, W, 7 * A)
        p, n = c['pos'].T.tolist(), c['neg'].T.tolist()
        assert p.count(p[-1]) == 2 and n.count(n[-1]) == 3
        assert set(map(tuple, p)) <= set(map(tuple, n))              # every positive is listed as non-negative too
        ad = np.abs(c['reg'])
        assert (ad > 2).any() and (ad < 0.5).any()
    c = C.loss_small('32x32x2')
    assert c['pos'].shape[1] > 1024 and c['neg'].shape[1] > 1024
    assert C.loss_gt_ld9()['gts'].shape[1] == 9
    assert C.loss_no_positive()['pos'].shape[1] == 0 and C.loss_no_positive()['neg'].shape[1] > 0 and C.loss_no_positive()['reg'] is not None
    assert C.loss_no_lists()['pos'].shape[1] == 0 == C.loss_no_lists()['neg'].shape[1]
    c = C.loss_all_listed()
    assert c['neg'].shape[1] == 70 == len(set(map(tuple, c['neg'].T.tolist())))
    c = C.loss_saturated()
    listed, positive = set(map(tuple, c['neg'].T.tolist())), set(map(tuple, c['pos'].T.tolist()))
    for v in (0.0, 1.0):
        at = set(zip(*np.nonzero(c['score'] == v)))
        assert at & positive and at & (listed - positive) and at - listed, v
    c = C.loss_kink()
    an = c['anchors'][tuple(c['pos'])]
    assert np.array_equal(R.targets32(c['gts'][c['gi']], an), np.zeros((7, 7), np.float32))
    r = c['reg'].reshape(5, 7, 2, 7)[tuple(c['pos'])]
    for col in range(7):                                             # every regression channel meets every kink value
        assert sorted(r[:, col].tolist()) == sorted(C.KINK.tolist())
    assert (np.abs(r) == 1.0).sum() == 14 and 1 - 1e-7 < C.KINK[2] < 1 < C.KINK[4] < 1 + 2e-7
    c = C.loss_large()
    assert c['L'] * c['W'] * c['A'] > 512 * 1024
