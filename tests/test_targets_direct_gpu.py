"""The label path through the C ABI at small grids: mvx_bbox_pairwise, mvx_classify_anchors[_frames] (csrc/bev_iou.h,
csrc/anchors.hip) and mvx_voxel_loss (csrc/loss.hip) on the inputs of tests/targets_cases.py.

References.  Order of the walk and f32 IoU arithmetic: the C oracle (O.classify_anchors_cells, O.bbox_pairwise), bit for bit,
on inputs where it consumes no stale scratch slot.  Geometric truth of the IoU: targets_ref.poly_iou64, within
targets_cases.IOU_BOUND = 3e-4 / INTER_BOUND = 2e-3 m^2 (4x the oracle's own largest error, 7.4e-5 / 3.9e-4, measured on the CPU
in test_targets_direct_host.py).  VoxelLoss: targets_ref.voxel_loss64, losses to 1e-5 relative, gradients to rtol 1e-5 with
atol 1e-9 -- the tolerances of test_targets_gpu.py.

The reference's IoU arithmetic is not symmetric in its two boxes (the oracle gives IoU(a, b) != IoU(b, a) on 87 of the 135 clean
pairs: the fan sums run in another order), so "swapping the arguments transposes the result" is checked as
pairwise(B, A)[j][i] == oracle(b_j, a_i), bit for bit.

Measured on an MI355X (every test prints its figures before it asserts).  mvx_bbox_pairwise against the truth: IoU 7.4e-5 and
intersection 3.9e-4 m^2 on the clean pairs (bit-equal to the oracle), 4.7e-8 and 8.4e-6 m^2 on the stale pairs.  mvx_voxel_loss:
losses within 1.4e-7 relative, gradients within 0.02 of their tolerance.

That the tests can fail: each of these changes to the kernels, built into a scratch library, fails the number of tests given.
    anchor_concat ignores the s_base carry                  1   (more than 1024 pairs)
    gi not made frame-local                                 2   (frames with empty frames; Calc replay, frames)
    the cap test is `o > cap`                               1   (status bit 2)
    counts not clipped                                      1   (status bit 2)
    circles_apart with factor 0.8                           1   (thin boxes whose bounding circles nearly touch)
    cut() leaves the degenerate slot unwritten              1   (pair table: 2.9e-3 IoU error on the along_fan_line_leftover pairs)
    tri_pair drops the sign                                16
    den_neg ignores n_neg                                  31
    loss_lists adds without atomics                        26
    reg_scale = 1 / n_pos                                  29
    loss_dense swaps ss.l / ss.w                     not run   (its swapped offsets leave small tensors; restated in numpy on
                                                                16x12x1, where they stay inside: clsLoss moves by 5 %)
    SmoothL1 test `ad <= 1`                                 0   (unobservable: at |diff| = 1 both branches give value 0.5 and
                                                                gradient 1; test_voxel_loss_on_the_smooth_l1_kink pins both
                                                                neighbours)"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mvx_oracle as O
import targets_cases as C
import targets_ref as R

pytestmark = pytest.mark.gpu
SENT = -7
FSENT = -12345.0
A_W, B_W, EPS = 1.5, 1.0, 1e-6


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------------------
# mvx_bbox_pairwise
# ---------------------------------------------------------------------------------------------------------------------------
def _pairwise(b1, b2, iou):
    """(n1,4,2) x (n2,4,2) -> (n1,n2) through the ABI; the output starts as FSENT."""
    from modules import Extension as X
    n1, n2 = b1.shape[0], b2.shape[0]
    out = torch.full((n1, n2), FSENT, dtype=torch.float32, device='cuda')
    d1, d2 = _dev(b1.reshape(n1, 8)), _dev(b2.reshape(n2, 8))
    rc = X.lib.mvx_bbox_pairwise(X.ptr(d1) if n1 else None, n1, X.ptr(d2) if n2 else None, n2, int(iou), X.ptr(out) if n1 * n2 else None,
                                 X.stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def test_pairwise_table_against_the_oracle_and_the_truth():
    rows = C.pair_table()
    _, qa, qb = C.pair_arrays()
    clean = np.array([r[3] == 0 for r in rows])
    assert (~clean).sum() >= 5
    for mode, k_or, k_tr, bound in ((1, 1, 4, C.IOU_BOUND), (0, 2, 5, C.INTER_BOUND)):
        rc, out = _pairwise(qa, qb, mode)                          # the whole table as ONE N x M call
        assert rc == 0 and out.shape == (len(rows), len(rows)) and np.isfinite(out).all() and not (out == FSENT).any()
        got = np.diag(out)
        want = np.array([r[k_or] for r in rows], np.float32)
        truth = np.array([r[k_tr] for r in rows])
        err = np.abs(got.astype(np.float64) - truth)
        print('%s: largest error against the truth %.3e on clean pairs, %.3e on stale pairs (bound %.0e)'
              % ('IoU' if mode else 'intersection', err[clean].max(), err[~clean].max(), bound))
        assert np.array_equal(got[clean], want[clean])
        assert (err <= bound).all(), [rows[i][0] for i in np.flatnonzero(err > bound)]


@pytest.mark.parametrize('n1,n2', [(9, 7), (8, 8), (13, 5), (1, 1)])
def test_pairwise_workgroup_edge_and_swapped_arguments(n1, n2):
    """n1 * n2 = 63, 64, 65 and 1 threads around the 64-thread workgroup; every entry against the oracle's result for that very
    pair, and the call with the arguments swapped against the oracle on the swapped pair."""
    _, qa, qb = C.pair_arrays()
    pick = np.random.default_rng(n1 * 100 + n2).permutation(len(qa))
    a, b = qa[pick[:n1]], qb[pick[n1:n1 + n2]]
    for x, y in ((a, b), (b, a)):
        rc, out = _pairwise(x, y, 1)
        assert rc == 0 and not (out == FSENT).any()
        n_clean = 0
        for i in range(x.shape[0]):
            for j in range(y.shape[0]):
                iou, _, stale = C.oracle_pair(x[i], y[j])
                if stale == 0:
                    n_clean += 1
                    assert out[i, j] == iou, (i, j)
        assert n_clean >= (x.shape[0] * y.shape[0] * 3) // 4


def test_pairwise_without_boxes_touches_nothing():
    _, qa, qb = C.pair_arrays()
    rc, out = _pairwise(qa[:0], qb[:3], 1)
    assert rc == 0 and out.shape == (0, 3)
    from modules import Extension as X
    out = torch.full((4, 3), FSENT, dtype=torch.float32, device='cuda')
    d2 = _dev(qb[:3].reshape(3, 8))
    assert X.lib.mvx_bbox_pairwise(X.ptr(d2), 0, X.ptr(d2), 3, 1, X.ptr(out), X.stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == FSENT).all())


# ---------------------------------------------------------------------------------------------------------------------------
# mvx_classify_anchors / mvx_classify_anchors_frames
# ---------------------------------------------------------------------------------------------------------------------------
def _classify(g, bev, nls, nws, neg_thr, pos_thr, R_, off=None, cap=None, slack=0):
    """mvx_classify_anchors_frames through the ABI.  ``off``: ground-truth offsets of the frames (default: one frame).  The output
    buffers hold F * 3 * cap + slack (gi: F * cap + slack) elements and start as SENT.  Returns flat numpy buffers."""
    from modules import Extension as X
    G = bev.shape[0]
    off = [0, G] if off is None else list(off)
    F = len(off) - 1
    A = g['A']
    wn = 2 * R_ + 1
    gmax = max(off[f + 1] - off[f] for f in range(F))
    cap = max(1, gmax * A * wn * wn) if cap is None else cap
    pos = torch.full((F * 3 * cap + slack,), SENT, dtype=torch.int64, device='cuda')
    neg = torch.full((F * 3 * cap + slack,), SENT, dtype=torch.int64, device='cuda')
    gi = torch.full((F * cap + slack,), SENT, dtype=torch.int64, device='cuda')
    counts = torch.full((F, 2), SENT, dtype=torch.int32, device='cuda')
    status = torch.zeros((1,), dtype=torch.int32, device='cuda')
    nbytes = X.lib.mvx_classify_anchors_workspace_bytes(G, A, R_)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device='cuda')
    d_gt = _dev(bev.reshape(G, 8).astype(np.float32)) if G else None
    d_an = _dev(g['bevs'])
    d_nl, d_nw = (_dev(nls.astype(np.int64)), _dev(nws.astype(np.int64))) if G else (None, None)
    c_off = (ctypes.c_int32 * (F + 1))(*off)
    rc = X.lib.mvx_classify_anchors_frames(X.ptr(d_gt), c_off, F, X.ptr(d_an), g['l'], g['w'], A, X.ptr(d_nl), X.ptr(d_nw),
                                           float(neg_thr), float(pos_thr), int(R_), X.ptr(pos), X.ptr(neg), X.ptr(gi), cap,
                                           X.ptr(counts), X.ptr(status), X.ptr(ws), nbytes, X.stream())
    torch.cuda.synchronize()
    return dict(rc=rc, F=F, cap=cap, pos=pos.cpu().numpy(), neg=neg.cpu().numpy(), gi=gi.cpu().numpy(),
                counts=counts.cpu().numpy(), status=int(status.item()))


def _lists(res, f=0):
    cap = res['cap']
    n_pos, n_neg = (int(v) for v in res['counts'][f])
    p = res['pos'][f * 3 * cap:(f + 1) * 3 * cap].reshape(3, cap)[:, :n_pos]
    n = res['neg'][f * 3 * cap:(f + 1) * 3 * cap].reshape(3, cap)[:, :n_neg]
    return [p[0], p[1], p[2], n[0], n[1], n[2], res['gi'][f * cap:f * cap + n_pos]]


def _oracle(g, bev, nls, nws, neg_thr, pos_thr):
    """The oracle's seven lists; asserts that it consumed no stale slot on the way."""
    lib = O._oracle_c()
    before = lib.oracle_anchor_stale_reads()
    pi, ni, gi = O.classify_anchors_cells(bev, g['bevs'], nls, nws, neg_thr, pos_thr)
    assert lib.oracle_anchor_stale_reads() == before
    return list(pi) + list(ni) + [gi]


def _same(got, want):
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), 'list %d of (px, py, pz, nx, ny, nz, gi) differs' % k


@functools.lru_cache(maxsize=None)
def _grid_case(name):
    g = C.grid(name)
    gt = C.grid_gts(name)
    nls, nws = C.centre_cells(g, gt)
    return g, gt, C.bev(gt), nls, nws


@pytest.mark.parametrize('name', ['24x20x2', '16x12x1', '12x10x3'])
def test_classify_small_grids(name):
    """Corners, centre, a box equal to an anchor (twice), yaw +-pi/4 and a truck; A = 2, 1 and 3."""
    g, gt, bev, nls, nws = _grid_case(name)
    want = _oracle(g, bev, nls, nws, 0.45, 0.6)
    res = _classify(g, bev, nls, nws, 0.45, 0.6, max(g['l'], g['w']))
    assert res['rc'] == 0 and res['status'] == 0
    _same(_lists(res), want)
    assert len(want[6]) > 0 and set(want[2].tolist()) == set(range(g['A']))          # every orientation has positives
    assert (want[6] == 5).any() and (want[6] == 6).any()          # the repeated box has its positives twice


def test_classify_window_radius_55():
    g, gt, bev, nls, nws = _grid_case('120x60x2')
    want = _oracle(g, bev, nls, nws, 0.12, 0.6)
    res = _classify(g, bev, nls, nws, 0.12, 0.6, 55, cap=1 << 16)
    assert res['rc'] == 0 and res['status'] == 0
    _same(_lists(res), want)
    one = _classify(g, bev[5:6], nls[5:6], nws[5:6], 0.12, 0.6, 55)
    assert one['status'] == 0
    lists = _lists(one)
    _same(lists, _oracle(g, bev[5:6], nls[5:6], nws[5:6], 0.12, 0.6))
    assert np.abs(lists[3] - nls[5]).max() > 27                   # a listed cell more than 27 cells from the centre


def test_classify_thin_boxes_whose_bounding_circles_nearly_touch():
    g = C.grid('120x60x2thin')
    gt = C.thin_gts()
    nls, nws = C.centre_cells(g, gt)
    want = _oracle(g, C.bev(gt), nls, nws, 0.1, 0.6)
    res = _classify(g, C.bev(gt), nls, nws, 0.1, 0.6, 55)
    assert res['status'] == 0
    _same(_lists(res), want)
    assert (72, 30, 0) in set(zip(want[3].tolist(), want[4].tolist(), want[5].tolist()))


def test_classify_more_than_1024_pairs():
    """600 ground truths at A = 2: the 1024-thread concatenation makes two trips, the second one on top of the first's totals."""
    g = C.grid('24x20x2')
    gt = C.many_gts('24x20x2', 600, seed=C.MANY_SEED)
    nls, nws = C.centre_cells(g, gt)
    want = _oracle(g, C.bev(gt), nls, nws, 0.45, 0.6)
    assert gt.shape[0] * g['A'] > 1024 and (want[6] < 512).any() and (want[6] >= 512).any()
    res = _classify(g, C.bev(gt), nls, nws, 0.45, 0.6, 24, cap=1 << 16)
    assert res['rc'] == 0 and res['status'] == 0 and int(res['counts'][0, 1]) < (1 << 16)
    _same(_lists(res), want)


FRAME_SIZES = [3, 0, 1, 0, 0, 7, 2, 0, 1, 1, 0, 4, 0, 0, 5, 0]


def test_classify_frames_with_empty_frames_in_place():
    from modules import Extension as X
    assert len(FRAME_SIZES) == X.MAX_FRAMES
    g = C.grid('24x20x2')
    gt = C.many_gts('24x20x2', sum(FRAME_SIZES), seed=21)
    bev = C.bev(gt)
    nls, nws = C.centre_cells(g, gt)
    off = [0] + np.cumsum(FRAME_SIZES).tolist()
    res = _classify(g, bev, nls, nws, 0.45, 0.6, 24, off=off)
    assert res['rc'] == 0 and res['status'] == 0
    for f, n in enumerate(FRAME_SIZES):
        if n == 0:
            assert tuple(res['counts'][f]) == (0, 0)
            continue
        sl = slice(off[f], off[f + 1])
        single = _classify(g, bev[sl], nls[sl], nws[sl], 0.45, 0.6, 24)
        _same(_lists(res, f), _lists(single))
        _same(_lists(res, f), _oracle(g, bev[sl], nls[sl], nws[sl], 0.45, 0.6))
        gi = _lists(res, f)[6]
        assert len(gi) > 0 and gi.min() >= 0 and gi.max() < n         # local to the frame
    empty = _classify(g, bev[:0], nls[:0], nws[:0], 0.45, 0.6, 24, off=[0] * (X.MAX_FRAMES + 1))
    assert empty['rc'] == 0 and empty['status'] == 0 and not empty['counts'].any()
    assert (empty['pos'] == SENT).all() and (empty['gi'] == SENT).all()


def test_status_bit_1_window_too_small():
    g, gt, bev, nls, nws = _grid_case('24x20x2')
    res = _classify(g, bev[9:10], nls[9:10], nws[9:10], 0.45, 0.6, 2)
    assert res['rc'] == 0 and res['status'] == 1


def _calc_inputs(g, gt):
    bev = torch.from_numpy(C.bev(gt))
    return bev, torch.from_numpy(gt[:, :2].copy()), torch.from_numpy(g['bevs']).cuda().contiguous()


def test_calc_replays_with_a_wider_window(monkeypatch):
    """Calc.classifyAnchors[Frames] with a first radius estimate of 2 for a truck: status bit 1, widen, replay."""
    from modules import Calc, _hip
    g, gt, bev, nls, nws = _grid_case('24x20x2')
    calls = []
    real_one, real_frames = _hip.classify_anchors, _hip.classify_anchors_frames
    monkeypatch.setattr(Calc, '_window_radius', lambda *a: 2)
    monkeypatch.setattr(_hip, 'classify_anchors', lambda *a, **k: (calls.append(a[6]), real_one(*a, **k))[1])
    monkeypatch.setattr(_hip, 'classify_anchors_frames', lambda *a, **k: (calls.append(a[7]), real_frames(*a, **k))[1])
    t_bev, t_cen, t_an = _calc_inputs(g, gt)
    pi, ni, gi = Calc.classifyAnchors(t_bev, t_cen, t_an, g['rng'], 0.45, 0.6)
    assert calls[0] == 2 and len(calls) > 2 and calls == sorted(calls)
    _same([t.cpu().numpy() for t in list(pi) + list(ni) + [gi]], _oracle(g, bev, nls, nws, 0.45, 0.6))
    del calls[:]
    frames = [(t_bev[:4], t_cen[:4]), None, (t_bev[4:], t_cen[4:])]
    out = Calc.classifyAnchorsFrames(frames, t_an, g['rng'], 0.45, 0.6)
    assert calls[0] == 2 and len(calls) > 2 and out[1] is None
    for r, sl in ((out[0], slice(0, 4)), (out[2], slice(4, 10))):
        _same([t.cpu().numpy() for t in list(r[0]) + list(r[1]) + [r[2]]], _oracle(g, bev[sl], nls[sl], nws[sl], 0.45, 0.6))


def test_status_bit_2_cap_exceeded():
    g, gt, bev, nls, nws = _grid_case('24x20x2')
    full = _classify(g, bev, nls, nws, 0.45, 0.6, 24)
    want = _lists(full)
    n_pos = len(want[6])
    cap = n_pos - 3
    assert 0 < cap < n_pos < len(want[3])
    res = _classify(g, bev, nls, nws, 0.45, 0.6, 24, cap=cap, slack=64)
    assert res['rc'] == 0 and res['status'] == 2 and tuple(res['counts'][0]) == (cap, cap)
    _same(_lists(res), [w[:cap] for w in want])
    assert (res['pos'][3 * cap:] == SENT).all() and (res['neg'][3 * cap:] == SENT).all() and (res['gi'][cap:] == SENT).all()


def test_status_bit_4_centre_outside_the_grid():
    from modules import Calc
    from modules.Extension import MvxHipError
    g, gt, bev, nls, nws = _grid_case('24x20x2')
    nls, nws = nls.copy(), nws.copy()
    nls[2], nws[4] = -1, g['w']
    valid = np.array([k for k in range(len(gt)) if k not in (2, 4)])
    want = _oracle(g, bev[valid], nls[valid], nws[valid], 0.45, 0.6)
    want[6] = valid[want[6]]                                       # the original numbering
    res = _classify(g, bev, nls, nws, 0.45, 0.6, 24)
    assert res['rc'] == 0 and res['status'] == 4
    _same(_lists(res), want)
    outside = gt.copy()
    outside[2, 0] = g['rng'][0] - 1.0
    t_bev, t_cen, t_an = _calc_inputs(g, outside)
    with pytest.raises(MvxHipError):
        Calc.classifyAnchors(t_bev, t_cen, t_an, g['rng'], 0.45, 0.6)


# ---------------------------------------------------------------------------------------------------------------------------
# mvx_voxel_loss
# ---------------------------------------------------------------------------------------------------------------------------
def _alloc(shape, kind, fill):
    """(base, view): a (L,W,C) view in one of three layouts inside ``base``, which starts as ``fill``."""
    L, W, Cc = shape
    if kind == 'lwc':
        base = torch.full((L, W, Cc), fill, dtype=torch.float32, device='cuda')
        return base, base
    if kind == 'clw':                                              # the RPN's (1,C,L,W) map, permuted
        base = torch.full((1, Cc, L, W), fill, dtype=torch.float32, device='cuda')
        return base, base[0].permute(1, 2, 0)
    base = torch.full((L, W + 2, Cc + 3), fill, dtype=torch.float32, device='cuda')        # padded pitch in both dimensions
    return base, base[:, :W, :Cc]


def _padding_untouched(base, shape, kind):
    L, W, Cc = shape
    return kind != 'pad' or (bool((base[:, W:, :] == FSENT).all()) and bool((base[:, :, Cc:] == FSENT).all()))


def _place(arr, kind):
    base, view = _alloc(arr.shape, kind, FSENT)
    view.copy_(torch.from_numpy(arr))
    return base, view


def _padded_lists(c, extra=5):
    """Capacity-sized device lists whose tails hold out-of-range garbage."""
    n_pos, n_neg = c['pos'].shape[1], c['neg'].shape[1]
    cap = max(n_pos, n_neg) + extra
    pos = np.full((3, cap), C.GARBAGE, np.int64)
    neg = np.full((3, cap), -C.GARBAGE, np.int64)
    gi = np.full((cap,), C.GARBAGE, np.int64)
    pos[:, :n_pos], neg[:, :n_neg], gi[:n_pos] = c['pos'], c['neg'], c['gi']
    return _dev(pos), _dev(neg), _dev(gi), n_pos, n_neg


def _run_loss(c, lay_in='lwc', lay_out=None, with_reg=True):
    from modules import _hip
    lay_out = lay_out or lay_in
    L, W, A = c['L'], c['W'], c['A']
    _, score = _place(c['score'], lay_in)
    reg = _place(c['reg'], lay_in)[1] if with_reg else None
    ds_base, ds = _alloc((L, W, A), lay_out, FSENT)
    dr_base, dr = _alloc((L, W, 7 * A), lay_out, FSENT)
    dr.zero_()
    pos, neg, gi, n_pos, n_neg = _padded_lists(c)
    losses, ds2, dr2 = _hip.voxel_loss(score, reg, pos, neg, gi, n_pos, n_neg, _dev(c['gts']), _dev(c['anchors']), A, A_W, B_W, EPS,
                                       dscore_out=ds, dreg_out=dr if with_reg else None)
    torch.cuda.synchronize()
    assert ds2 is ds and _padding_untouched(ds_base, (L, W, A), lay_out) and _padding_untouched(dr_base, (L, W, 7 * A), lay_out)
    return losses.cpu().numpy().astype(np.float64), ds.cpu().numpy().astype(np.float64), dr.cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _loss_ref(getter, *args):
    c = getattr(C, getter)(*args)
    return R.voxel_loss64(c['score'], c['reg'], c['pos'], c['neg'], c['gi'], c['gts'], c['anchors'], A_W, B_W, EPS)


def _check_loss(got, ref, with_reg=True, where=None):
    (losses, ds, dr), (rl, rds, rdr) = got, ref
    assert np.isfinite(losses).all() and np.isfinite(ds).all() and np.isfinite(dr).all()
    if where is not None:
        ds, rds = ds.reshape(-1)[where], rds.reshape(-1)[where]
    e_l = np.abs(losses - rl) / np.maximum(np.abs(rl), 1e-300)
    e_s = (np.abs(ds - rds) / (1e-5 * np.abs(rds) + 1e-9)).max()
    e_r = (np.abs(dr - rdr) / (1e-5 * np.abs(rdr) + 1e-9)).max() if with_reg else 0.0
    print('loss errors %.2e / %.2e (relative); dscore %.2e and dreg %.2e of their tolerances' % (e_l[0], e_l[1] if with_reg else 0.0, e_s, e_r))
    np.testing.assert_allclose(losses[0], rl[0], rtol=1e-5, atol=0)
    np.testing.assert_allclose(ds, rds, rtol=1e-5, atol=1e-9)
    if with_reg:
        np.testing.assert_allclose(losses[1], rl[1], rtol=1e-5, atol=0)
        np.testing.assert_allclose(dr, rdr, rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize('lay_in,lay_out', [('lwc', 'lwc'), ('clw', 'clw'), ('pad', 'pad'), ('lwc', 'clw'), ('clw', 'pad'), ('pad', 'lwc')])
@pytest.mark.parametrize('name', list(C.LOSS_GRIDS))
def test_voxel_loss_grids_and_layouts(name, lay_in, lay_out):
    """A = 2, 1, 3; a positive listed twice and a non-negative three times; lists beyond 1024 entries (32x32x2)."""
    _check_loss(_run_loss(C.loss_small(name), lay_in, lay_out), _loss_ref('loss_small', name))


def test_voxel_loss_gt_ld_9():
    _check_loss(_run_loss(C.loss_gt_ld9()), _loss_ref('loss_gt_ld9'))


def test_voxel_loss_without_positives_but_with_reg():
    got = _run_loss(C.loss_no_positive())
    _check_loss(got, _loss_ref('loss_no_positive'))
    assert got[0][1] == 0.0 and not got[2].any()


def test_voxel_loss_without_lists():
    got = _run_loss(C.loss_no_lists())
    _check_loss(got, _loss_ref('loss_no_lists'))
    assert got[0][1] == 0.0 and not got[2].any() and (got[1] > 0).all()


def test_voxel_loss_every_anchor_listed():
    _check_loss(_run_loss(C.loss_all_listed()), _loss_ref('loss_all_listed'))


def test_voxel_loss_scores_of_exactly_0_and_1():
    _check_loss(_run_loss(C.loss_saturated()), _loss_ref('loss_saturated'))


def test_voxel_loss_on_the_smooth_l1_kink():
    """|diff| = 1 exactly and one ulp to either side.  At exactly 1 both branches give the same value (0.5) and the same
    gradient (1), so `ad < 1` against `ad <= 1` cannot be told apart there; the neighbours pin the branches' formulas."""
    c = C.loss_kink()
    got = _run_loss(c)
    _check_loss(got, _loss_ref('loss_kink'))
    rows = got[2].reshape(5, 7, 2, 7)[tuple(c['pos'])] * 49.0       # d regLoss / d reg * (7 n_pos)
    want = np.where(np.abs(C.KINK) < 1, C.KINK, np.sign(C.KINK)).astype(np.float64)
    for k in range(7):
        np.testing.assert_allclose(rows[k], np.roll(want, k), rtol=1e-6, atol=0)


def test_voxel_loss_dense_pass_strides_its_grid():
    """520 x 512 x 2 > 512 blocks x 1024: the losses, and dscore at 4,096 seeded positions plus every listed one."""
    c = C.loss_large()
    where = np.random.default_rng(4).integers(0, c['L'] * c['W'] * c['A'], 4096)
    listed = (c['neg'][0] * c['W'] + c['neg'][1]) * c['A'] + c['neg'][2]
    _check_loss(_run_loss(c), _loss_ref('loss_large'), where=np.concatenate([where, listed]))


@pytest.mark.parametrize('name', ['5x7x2', '12x10x3'])
def test_voxel_loss_counts_on_the_device(name):
    """counts_dev: the true counts on the device, wrong ones in n_pos / n_neg, garbage behind the lists.  One workgroup in the
    dense pass at these sizes, so the f64 sums and hence the losses repeat bit for bit."""
    from modules import Extension as X
    c = C.loss_small(name)
    L, W, A = c['L'], c['W'], c['A']
    score, reg, gts, an = _dev(c['score']), _dev(c['reg']), _dev(c['gts']), _dev(c['anchors'])
    pos, neg, gi, n_pos, n_neg = _padded_lists(c)
    cap = pos.shape[1]
    counts = _dev(np.array([n_pos, n_neg], np.int32))
    scratch = torch.empty((4,), dtype=torch.float64, device='cuda')

    def call(counts_dev, np_, nn_, dscore):
        losses = torch.full((2,), FSENT, dtype=torch.float32, device='cuda')
        rc = X.lib.mvx_voxel_loss(X.ptr(score), W * A, A, 1, X.ptr(reg), W * 7 * A, 7 * A, 1, X.ptr(pos), cap, X.ptr(neg), cap, X.ptr(gi),
                                  X.ptr(counts_dev), np_, nn_, X.ptr(gts), c['gts'].shape[1], X.ptr(an), L, W, A, A_W, B_W, EPS,
                                  X.ptr(dscore), W * A, A, 1, None, 0, 0, 0, X.ptr(losses), X.ptr(scratch), X.stream())
        torch.cuda.synchronize()
        return rc, losses.cpu().numpy()
    rc_h, host = call(None, n_pos, n_neg, None)
    rc_d, dev = call(counts, 1, 2, None)
    assert rc_h == 0 and rc_d == 0 and np.array_equal(host, dev)
    np.testing.assert_allclose(host.astype(np.float64), _loss_ref('loss_small', name)[0], rtol=1e-5, atol=0)
    dscore = torch.full((L, W, A), FSENT, dtype=torch.float32, device='cuda')
    rc, losses = call(counts, 1, 2, dscore)
    assert rc < 0 and (losses == FSENT).all() and bool((dscore == FSENT).all())
