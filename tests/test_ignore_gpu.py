"""The ignore pass through the C ABI, through Calc and through the loader at small grids: mvx_box_point_counts_frames and
mvx_ignore_anchors_frames (csrc/ignore.hip) on the inputs of tests/ignore_cases.py.

References.  The rule: tests/ignore_ref.ignore_rule, applied to the lists mvx_assign_anchors_frames wrote in the same run, to the
float64 projection of the anchor centres (ignore_ref.project) and to mvx_bbox_pairwise(ignore quads, anchors, 0) of the same run
with the pairs whose bounding circles are apart set to 0 -- every list, count and stat bit for bit and in order.  The point
counts: ignore_ref.point_counts64 (numpy float64).  Every fixture is shown inside the test to leave no decision to rounding: no
centre within 1e-6 px of a rectangle edge, no point within 1e-6 m of a box face, no pair with |inter - ioa_thr * area| below 1e-4
of the area."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import assign_cases as AC
import focal_ref as FR
import ignore_cases as IC
import ignore_ref as IR
import targets_cases as C

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7


def _dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))
    return torch.from_numpy(a).cuda()


def _offsets(items):
    return np.concatenate([[0], np.cumsum([0 if t is None else len(t) for t in items])]).astype(np.int32)


def _cat(items, shape, dtype):
    parts = [np.asarray(t, dtype).reshape((-1,) + shape) for t in items if t is not None and len(t)]
    return np.concatenate(parts) if parts else None


def _assign(g, cars):
    """The assigner's raw device outputs for per-frame Car boxes (n, 7): (pos, neg, gi, counts i32 (2F,), gt_off list)."""
    from modules import _hip
    off = _offsets(cars).tolist()
    bev = _cat([C.bev(c) if len(c) else None for c in cars], (4, 2), np.float32)
    bev = np.zeros((0, 4, 2), np.float32) if bev is None else bev
    pos, neg, gi, host = _hip.assign_anchors_frames(_dev(bev), off, _dev(g['bevs']), IC.NEG, IC.POS, IC.FORCE, min(55, max(g['l'], g['w'])))
    F = len(cars)
    return pos, neg, gi, host[:2 * F].contiguous(), off


def _ignore(g, lists, gt_points=None, min_points=0, rects=None, mats=None, quads=None, ioa=IC.IOA, cap_out=None, slack=0):
    """mvx_ignore_anchors_frames through the ABI on the device lists ``lists`` of _assign.  Per-frame sources (lists with None for
    a frame that has none).  The output buffers hold F * 3 * cap_out + slack (gi: F * cap_out + slack) elements and start as SENT;
    the workspace arrives dirty.  Returns flat numpy buffers."""
    from modules import Extension as X
    pos, neg, gi, counts, off = lists
    F, cap = gi.shape
    N = g['l'] * g['w'] * g['A']
    cap_out = N if cap_out is None else cap_out
    p = torch.full((F * 3 * cap_out + slack,), SENT, dtype=torch.int64, device='cuda')
    n = torch.full((F * 3 * cap_out + slack,), SENT, dtype=torch.int64, device='cuda')
    go = torch.full((F * cap_out + slack,), SENT, dtype=torch.int64, device='cuda')
    c_out = torch.full((F, 2), SENT, dtype=torch.int32, device='cuda')
    stats = torch.full((F, 4), SENT, dtype=torch.int32, device='cuda')
    status = torch.zeros((1,), dtype=torch.int32, device='cuda')
    nbytes = X.lib.mvx_ignore_anchors_frames_workspace_bytes(F, g['l'], g['w'], g['A'])
    ws = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device='cuda')
    d_pts = None if gt_points is None else _dev(gt_points, np.int32)
    d_goff = None if gt_points is None else _dev(off, np.int32)
    r_all = None if rects is None else _cat(rects, (4,), np.float32)
    d_rect = None if r_all is None else _dev(r_all)
    d_roff = None if r_all is None else _dev(_offsets(rects))
    d_mats = None
    if r_all is not None:
        d_mats = _dev(np.stack([np.zeros((3, 4)) if m is None else np.asarray(m, np.float64) for m in mats]))
    q_all = None if quads is None else _cat(quads, (4, 2), np.float32)
    d_quad = None if q_all is None else _dev(q_all)
    d_qoff = None if q_all is None else _dev(_offsets(quads))
    d_an, d_bev = _dev(g['anchors']), _dev(g['bevs'])
    rc = X.lib.mvx_ignore_anchors_frames(X.ptr(pos), X.ptr(neg), X.ptr(gi), cap, X.ptr(counts), F, X.ptr(d_goff), X.ptr(d_pts),
                                         int(min_points), X.ptr(d_an), X.ptr(d_bev), g['l'], g['w'], g['A'], X.ptr(d_rect), X.ptr(d_roff),
                                         X.ptr(d_mats), X.ptr(d_quad), X.ptr(d_qoff), float(ioa), X.ptr(p), X.ptr(n), X.ptr(go), cap_out,
                                         X.ptr(c_out), X.ptr(stats), X.ptr(status), X.ptr(ws), nbytes, X.stream())
    torch.cuda.synchronize()
    return dict(rc=rc, F=F, cap=cap_out, pos=p.cpu().numpy(), neg=n.cpu().numpy(), gi=go.cpu().numpy(), counts=c_out.cpu().numpy(),
                stats=stats.cpu().numpy(), status=int(status.item()))


def _lists(res, f=0):
    """[px, py, pz, nx, ny, nz, gi] of frame f, and that nothing past the counts was written."""
    cap = res['cap']
    n_pos, n_neg = (int(v) for v in res['counts'][f])
    p = res['pos'][f * 3 * cap:(f + 1) * 3 * cap].reshape(3, cap)
    n = res['neg'][f * 3 * cap:(f + 1) * 3 * cap].reshape(3, cap)
    gi = res['gi'][f * cap:(f + 1) * cap]
    assert (p[:, n_pos:] == SENT).all() and (n[:, n_neg:] == SENT).all() and (gi[n_pos:] == SENT).all()
    return [p[0, :n_pos], p[1, :n_pos], p[2, :n_pos], n[0, :n_neg], n[1, :n_neg], n[2, :n_neg], gi[:n_pos]]


def _incoming(lists, g, f):
    """(pos flat, gi, notneg flat) of frame f of the assigner's device lists."""
    pos, neg, gi, counts, _ = lists
    n_pos, n_neg = (int(v) for v in counts.cpu().numpy()[2 * f:2 * f + 2])
    p, n = pos[f, :, :n_pos].cpu().numpy(), neg[f, :, :n_neg].cpu().numpy()
    return AC.flat(p[0], p[1], p[2], g), gi[f, :n_pos].cpu().numpy(), AC.flat(n[0], n[1], n[2], g)


def _inter_table(g, quads):
    """mvx_bbox_pairwise(quads, anchors, 0) of this run, 0 where the bounding circles are apart."""
    from modules import _hip
    abev = np.ascontiguousarray(g['bevs'].reshape(-1, 4, 2))
    inter = _hip.bbox_pairwise(_dev(quads, np.float32), _dev(abev), 0).cpu().numpy()
    inter[AC.apart(quads, abev)] = 0.0
    return inter


def _expected(g, lists, f, gt_points=None, min_points=0, rects=None, matrix=None, quads=None, ioa=IC.IOA):
    """ignore_rule on frame f with this run's tables; asserts the fixture's conditions on the way."""
    N = g['l'] * g['w'] * g['A']
    pos, gi, notneg = _incoming(lists, g, f)
    k = {}
    if rects is not None and len(rects):
        k['centres'] = IR.project(g['anchors'].reshape(-1, 7), matrix)
        k['rects'] = rects
        assert IR.in_rects(*k['centres'], rects)[1] > 1e-6
    if quads is not None and len(quads):
        k['inter'] = _inter_table(g, quads)
        k['area'] = IR.area32(g['bevs'].reshape(-1, 4, 2))
        assert IR.box_margin(k['inter'], k['area'], ioa) >= 1e-4
    if gt_points is not None:
        off = lists[4]
        k['gt_points'] = np.asarray(gt_points)[off[f]:off[f + 1]]
    return IR.ignore_rule(N, pos, gi, notneg, min_points=min_points, ioa_thr=ioa, **k)


def _same(res, f, want, g):
    got = _lists(res, f)
    exp = _triples(want['pos'], g) + _triples(want['notneg'], g) + [want['gi']]
    for k, (a, b) in enumerate(zip(got, exp)):
        assert np.array_equal(a, b), 'frame %d, list %d of (px, py, pz, nx, ny, nz, gi) differs: %s != %s' % (f, k, a, b)
    assert tuple(res['counts'][f]) == (len(want['pos']), len(want['notneg']))
    assert res['stats'][f].tolist() == want['stats'], (f, res['stats'][f].tolist(), want['stats'])


def _triples(flat, g):
    flat = np.asarray(flat, np.int64)
    return [flat // (g['w'] * g['A']), (flat // g['A']) % g['w'], flat % g['A']]


# ---------------------------------------------------------------------------------------------------------------------------
# base case, A = 1, 2, 3
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('A', [1, 2, 3])
def test_base_case_exact(A):
    """grid_gts' nine cars; the truck and a 5.0 x 2.0 m van at yaw 0.3 as look-alike boxes; two rectangles; box 4 holds too few
    points.  Every clause of the rule has work to do."""
    g = IC.orientations(IC.grid('24x20x2'), A)
    cars, alike = IC.base_boxes()
    lists = _assign(g, [cars])
    gt_points = [9, 5, 30, 7, 4, 12, 0, 5, 6]
    src = dict(gt_points=gt_points, min_points=5, rects=[IC.RECTS['24x20x2']], quads=[C.bev(alike)])
    res = _ignore(g, lists, mats=[IC.MATRIX], **src)
    assert res['rc'] == 0 and res['status'] == 0
    want = _expected(g, lists, 0, gt_points=gt_points, min_points=5, rects=IC.RECTS['24x20x2'], matrix=IC.MATRIX, quads=C.bev(alike))
    _same(res, 0, want, g)
    demoted, by_rect, by_box, sparse = want['stats']
    print('A = %d: %s' % (A, want['stats']))
    assert demoted >= 1 and by_rect > 50 and by_box >= 5 and sparse == 2
    inc = _incoming(lists, g, 0)
    assert len(want['pos']) == len(inc[0]) - demoted and not np.isin(want['gi'], [4, 6]).any()
    lst = _lists(res)
    assert np.all(np.diff(AC.flat(lst[3], lst[4], lst[5], g)) > 0) and np.all(np.diff(AC.flat(lst[0], lst[1], lst[2], g)) > 0)
    # each source alone, and none: the lists of the assigner come back
    for part in (dict(gt_points=gt_points, min_points=5), dict(rects=[IC.RECTS['24x20x2']]), dict(quads=[C.bev(alike)])):
        r = _ignore(g, lists, mats=[IC.MATRIX], **part)
        w = _expected(g, lists, 0, gt_points=part.get('gt_points'), min_points=part.get('min_points', 0),
                      rects=part['rects'][0] if 'rects' in part else None, matrix=IC.MATRIX,
                      quads=part['quads'][0] if 'quads' in part else None)
        _same(r, 0, w, g)
    plain = _ignore(g, lists)
    got = _lists(plain)
    assert plain['rc'] == 0 and plain['stats'][0].tolist() == [0, 0, 0, 0]
    assert np.array_equal(AC.flat(got[0], got[1], got[2], g), inc[0]) and np.array_equal(got[6], inc[1])
    assert np.array_equal(AC.flat(got[3], got[4], got[5], g), inc[2])


def test_ioa_is_over_the_anchor_area_and_other_thresholds():
    """The 10 x 2.6 m truck covers whole anchors: at ioa_thr = 0.9 an anchor inside it is still shielded, which intersection over
    union (at most 6.24 / 26 = 0.24) could never do."""
    g = IC.grid('24x20x2')
    cars, alike = IC.base_boxes()
    lists = _assign(g, [cars])
    for ioa in (0.25, 0.7, 0.9):
        res = _ignore(g, lists, quads=[C.bev(alike)], ioa=ioa)
        want = _expected(g, lists, 0, quads=C.bev(alike), ioa=ioa)
        _same(res, 0, want, g)
        assert want['stats'][2] > 0


# ---------------------------------------------------------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------------------------------------------------------
def _frame_set(F):
    """Per frame (cars, rects or None, quads or None): frame 0 rectangles and no Car, frame 1 Cars only, frame 2 nothing at all (F >=
    3), the others a mixture."""
    cars9, alike = IC.base_boxes()
    none = np.zeros((0, 7), np.float32)
    frames = [(none, IC.RECTS['24x20x2'], None), (cars9, None, None), (none, None, None)]
    more = C.many_gts('24x20x2', sum(AC.FRAME_SIZES), seed=21)
    off = np.cumsum([0] + AC.FRAME_SIZES)
    for k in range(3, 16):
        c = more[off[k]:off[k + 1]]
        frames.append((c, [IC.RECT_A] if k % 2 else None, C.bev(alike[k % 2:k % 2 + 1]) if k % 3 else None))
    return frames[:F] if F > 1 else [(cars9, IC.RECTS['24x20x2'], C.bev(alike))]


@pytest.mark.parametrize('F', [1, 3, 16])
def test_frames_exact(F):
    from modules import Extension as X
    assert X.MAX_FRAMES == 16
    g = IC.grid('24x20x2')
    frames = _frame_set(F)
    lists = _assign(g, [fr[0] for fr in frames])
    rects, quads = [fr[1] for fr in frames], [fr[2] for fr in frames]
    shift = np.array([[0.0, 0.0, 0.0, 2.0], [0.0, 0.0, 0.0, 0.5], [0.0, 0.0, 0.0, 0.0]])
    mats = [None if r is None else IC.MATRIX + k * shift for k, r in enumerate(rects)]               # a matrix of its own per frame
    res = _ignore(g, lists, rects=rects, mats=mats, quads=quads)
    assert res['rc'] == 0 and res['status'] == 0
    for f, (cars, r, q) in enumerate(frames):
        want = _expected(g, lists, f, rects=r, matrix=mats[f], quads=q)
        _same(res, f, want, g)
        if r is not None:
            assert want['stats'][1] > 0
        if len(cars) == 0 and r is None and q is None:
            assert tuple(res['counts'][f]) == (0, 0)
        if len(cars) == 0 and r is not None:
            assert res['counts'][f][0] == 0 and res['counts'][f][1] == want['stats'][1] + want['stats'][2] > 0


# ---------------------------------------------------------------------------------------------------------------------------
# 18 blocks, cap_out, behind the camera
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wide():
    g = IC.grid('44x50x2')
    cars = IC.cars_for('44x50x2', 12, seed=5)
    return g, cars, _assign(g, [cars])


def test_a_list_that_crosses_block_boundaries():
    g, cars, lists = _wide()
    res = _ignore(g, lists, rects=[[IC.RECT_ALL]], mats=[IC.MATRIX])
    want = _expected(g, lists, 0, rects=[IC.RECT_ALL], matrix=IC.MATRIX)
    _same(res, 0, want, g)
    nn = want['notneg']
    blocks = np.unique(nn // 256)
    assert len(nn) > 2000 and len(blocks) >= 12 and blocks.max() == 17 and np.all(np.diff(nn) > 0)
    res = _ignore(g, lists, rects=[[IC.RECT_A]], mats=[IC.MATRIX])
    _same(res, 0, _expected(g, lists, 0, rects=[IC.RECT_A], matrix=IC.MATRIX), g)


def test_status_bit_2_cap_out_too_small_and_nothing_written_past_it():
    g, cars, lists = _wide()
    want = _expected(g, lists, 0, rects=[IC.RECT_ALL], matrix=IC.MATRIX)
    n_pos, n_neg = len(want['pos']), len(want['notneg'])
    cap = 1000
    assert n_pos < cap < n_neg
    res = _ignore(g, lists, rects=[[IC.RECT_ALL]], mats=[IC.MATRIX], cap_out=cap, slack=64)
    assert res['rc'] == 0 and res['status'] == 2 and tuple(res['counts'][0]) == (n_pos, cap)
    got = _lists(res)
    exp = _triples(want['pos'], g) + _triples(want['notneg'][:cap], g) + [want['gi']]
    for a, b in zip(got, exp):
        assert np.array_equal(a, b)
    assert (res['pos'][3 * cap:] == SENT).all() and (res['neg'][3 * cap:] == SENT).all() and (res['gi'][cap:] == SENT).all()
    assert res['stats'][0].tolist() == want['stats']
    small = _ignore(g, lists, rects=[[IC.RECT_ALL]], mats=[IC.MATRIX], cap_out=n_pos - 1, slack=64)
    assert small['status'] == 2 and tuple(small['counts'][0]) == (n_pos - 1, n_pos - 1)
    assert (small['pos'][3 * (n_pos - 1):] == SENT).all() and (small['gi'][n_pos - 1:] == SENT).all()


def test_anchors_behind_the_camera_are_left_alone():
    g = IC.grid('24x20x2behind')
    cars = IC.cars_for('24x20x2behind', 5, seed=9)
    lists = _assign(g, [cars])
    res = _ignore(g, lists, rects=[[IC.RECT_ALL]], mats=[IC.MATRIX])
    want = _expected(g, lists, 0, rects=[IC.RECT_ALL], matrix=IC.MATRIX)
    _same(res, 0, want, g)
    px, py, d = IR.project(g['anchors'].reshape(-1, 7), IC.MATRIX)
    behind = np.flatnonzero(d <= 0)
    inc = _incoming(lists, g, 0)
    assert len(behind) > 100 and want['stats'][1] > 0
    assert np.array_equal(np.intersect1d(want['notneg'], behind), np.intersect1d(inc[2], behind))
    # without the depth test the anchors straight behind the camera would land in the picture: the test is what keeps them out
    a = g['anchors'].reshape(-1, 7).astype(np.float64)[behind]
    hom = np.stack([a[:, 0], a[:, 1], a[:, 2] + a[:, 5] / 2.0, np.ones(len(a))], axis=1) @ IC.MATRIX.T
    u, v = hom[:, 0] / hom[:, 2], hom[:, 1] / hom[:, 2]
    assert ((u >= 0) & (u <= 1242) & (v >= 0) & (v <= 375)).sum() > 10


# ---------------------------------------------------------------------------------------------------------------------------
# point counts, demotion
# ---------------------------------------------------------------------------------------------------------------------------
def _count(points, n_points, boxes, gt_off):
    from modules import _hip
    return _hip.box_point_counts_frames(_dev(points), _dev(n_points, np.int32), _dev(boxes, np.float32), _dev(gt_off, np.int32)).cpu().numpy()


def test_point_counts_against_float64():
    fx = IC.point_fixture()
    want, margin = IR.point_counts64(fx['points'], fx['n_points'], fx['boxes'], fx['gt_off'])
    assert margin > 1e-6
    got = _count(fx['points'], fx['n_points'], fx['boxes'], fx['gt_off'])
    print('point counts %s' % got.tolist())
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(_count(fx['points'], fx['n_points'], fx['boxes'], fx['gt_off']), got)          # integer sums: reproducible
    # a count past the capacity is clipped to it, a negative one to 0; a frame without boxes; more than 64 boxes in a frame
    n = np.array([10 ** 6, -5, 1], np.int32)
    full, _ = IR.point_counts64(fx['points'], [3072, 0, 1], fx['boxes'], fx['gt_off'])
    assert np.array_equal(_count(fx['points'], n, fx['boxes'], fx['gt_off']), full)
    off = np.array([0, 0, 6, 6], np.int32)
    alone, _ = IR.point_counts64(fx['points'], fx['n_points'], fx['boxes'], off)
    assert np.array_equal(_count(fx['points'], fx['n_points'], fx['boxes'], off), alone)
    many = np.tile(fx['boxes'][:3], (24, 1))                                                           # 72 boxes: two LDS chunks
    m_off = np.array([0, 72, 72, 72], np.int32)
    m_want, _ = IR.point_counts64(fx['points'], fx['n_points'], many, m_off)
    assert np.array_equal(_count(fx['points'], fx['n_points'], many, m_off), m_want) and (m_want > 100).all()


def test_demotion_at_exactly_min_points():
    """Cars 0 and 1 of the base case hold exactly min_points - 1 and min_points points, counted by the kernel."""
    g = IC.grid('24x20x2')
    cars, _ = IC.base_boxes()
    lists = _assign(g, [cars])
    pts = np.zeros((1, 64, 6), np.float32)
    pts[0, :, :3] = [100.0, 100.0, 100.0]
    k = 0
    for b, n in ((0, 4), (1, 5), (2, 9)):
        for j in range(n):
            c, s = np.cos(cars[b, 6]), np.sin(cars[b, 6])
            u, v = 0.3 * (j - n / 2.0) / n * cars[b, 3], 0.1 * cars[b, 4]
            pts[0, k, :3] = [cars[b, 0] + u * c + v * s, cars[b, 1] - u * s + v * c, cars[b, 2] + 0.5 * cars[b, 5]]
            k += 1
    want_counts, margin = IR.point_counts64(pts, [k], cars, [0, 9])
    assert margin > 1e-6 and want_counts.tolist() == [4, 5, 9, 0, 0, 0, 0, 0, 0]
    counts = _count(pts, np.array([k], np.int32), cars, np.array([0, 9], np.int32))
    assert np.array_equal(counts, want_counts)
    res = _ignore(g, lists, gt_points=counts, min_points=5)
    want = _expected(g, lists, 0, gt_points=counts, min_points=5)
    _same(res, 0, want, g)
    inc_pos, inc_gi, inc_nn = _incoming(lists, g, 0)
    keep = np.isin(inc_gi, [1, 2])
    assert (inc_gi == 0).any() and keep.any() and want['stats'] == [int((~keep).sum()), 0, 0, 7]
    # the kept entries, their gi untouched, in their order; the not-negative list unchanged
    assert np.array_equal(want['pos'], inc_pos[keep]) and np.array_equal(want['gi'], inc_gi[keep]) and np.array_equal(want['notneg'], inc_nn)
    assert not _ignore(g, lists, gt_points=counts, min_points=0)['stats'].any()


# ---------------------------------------------------------------------------------------------------------------------------
# reproducibility, no change without the switch
# ---------------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal():
    g = IC.grid('24x20x2')
    frames = _frame_set(16)
    lists = _assign(g, [fr[0] for fr in frames])
    rects, quads = [fr[1] for fr in frames], [fr[2] for fr in frames]
    mats = [None if r is None else IC.MATRIX for r in rects]
    a, b = (_ignore(g, lists, rects=rects, mats=mats, quads=quads) for _ in range(2))
    for k in ('pos', 'neg', 'gi', 'counts', 'stats', 'status'):
        assert np.array_equal(a[k], b[k]), k


def _calc_lists(r):
    return [t.cpu().numpy() for t in list(r[0]) + list(r[1]) + [r[2]]]


def test_ignore_none_is_the_direct_assigner_result():
    from modules import Calc
    g = IC.grid('24x20x2')
    cars, _ = IC.base_boxes()
    bevs = _dev(g['bevs'])
    frames = [(torch.from_numpy(C.bev(cars[:4])), None), None, (torch.from_numpy(C.bev(cars[4:])), None)]
    out = Calc.assignAnchorsFrames(frames, bevs, ignore=None)
    pos, neg, gi, counts, off = _assign(g, [cars[:4], cars[4:]])
    counts = counts.cpu().numpy()
    assert out[1] is None
    for f, k in ((0, 0), (1, 2)):
        n_pos, n_neg = int(counts[2 * f]), int(counts[2 * f + 1])
        want = [pos[f, j, :n_pos].cpu().numpy() for j in range(3)] + [neg[f, j, :n_neg].cpu().numpy() for j in range(3)] + [gi[f, :n_pos].cpu().numpy()]
        for a, b in zip(_calc_lists(out[k]), want):
            assert np.array_equal(a, b)


def test_regions_without_a_source_change_nothing_but_the_launches():
    """Calc.assignAnchorsFrames on (boxes, None, boxes): ``ignore=None`` launches the assigner's five kernels per enqueue and no
    other; an IgnoreRegions without any source and min_points = 0 adds the ignore pass's four behind every one of them and returns
    the same lists and the same ``info`` (the rule, tests/ignore_ref.py, is the identity on them), with all-zero stats."""
    from modules import Calc
    from modules import Extension as X
    g = IC.grid('24x20x2')
    cars, _ = IC.base_boxes()
    bevs = _dev(g['bevs'])
    frames = [(torch.from_numpy(C.bev(cars[:4])), None), None, (torch.from_numpy(C.bev(cars[4:])), None)]
    runs = []
    for ignore in (None, Calc.IgnoreRegions(3, min_points=0)):
        info = {}
        n0 = X.lib.mvx_launch_count()
        out = Calc.assignAnchorsFrames(frames, bevs, IC.NEG, IC.POS, IC.FORCE, info=info, ignore=ignore)
        runs.append((out, info, X.lib.mvx_launch_count() - n0))
    (plain, info_p, n_p), (ign, info_i, n_i) = runs
    enqueues = n_p // 5
    print('launches: %d without regions, %d with (%d enqueue(s))' % (n_p, n_i, enqueues))
    assert enqueues >= 1 and n_p == 5 * enqueues and n_i == (5 + 4) * enqueues
    assert plain[1] is None and ign[1] is None
    N = g['l'] * g['w'] * g['A']
    for k in (0, 2):
        a, b = _calc_lists(plain[k]), _calc_lists(ign[k])
        assert len(a[0]) > 0 and len(a[3]) > len(a[0])
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        rule = IR.ignore_rule(N, AC.flat(a[0], a[1], a[2], g), a[6], AC.flat(a[3], a[4], a[5], g))
        for x, y in zip(a, _triples(rule['pos'], g) + _triples(rule['notneg'], g) + [rule['gi']]):
            assert np.array_equal(x, y)
        assert rule['stats'] == [0, 0, 0, 0]
        assert torch.equal(info_p['gt_best'][k], info_i['gt_best'][k])
    assert info_p['gt_best'][1] is None and info_i['gt_best'][1] is None
    assert (info_p['forced_only'], info_p['none']) == (info_i['forced_only'], info_i['none'])
    assert 'ignore_stats' not in info_p and info_i['ignore_stats'] == [0, 0, 0, 0]


def test_calc_with_ignore_regions_and_a_frame_without_cars(monkeypatch):
    """Through Calc: the regions of three frames, one without a Car but with rectangles (live: empty positives, a not-negative
    list), one with nothing (None); the stats in ``info``; and a radius replay enqueues the ignore pass again."""
    from modules import Calc, _hip
    g = IC.grid('24x20x2')
    cars, alike = IC.base_boxes()
    bevs = _dev(g['bevs'])
    an7 = torch.from_numpy(g['anchors'])
    frames = [(torch.from_numpy(C.bev(cars)), None), None, None]
    gt_points = torch.tensor([9, 5, 30, 7, 4, 12, 0, 5, 6], dtype=torch.int32).cuda()
    reg = Calc.IgnoreRegions(3, anchors=an7, rects=[torch.tensor(IC.RECTS['24x20x2']), torch.tensor([IC.RECT_A]), None],
                             matrix=[IC.MATRIX, IC.MATRIX, None], quads=[torch.from_numpy(C.bev(alike)), None, None],
                             boxes3d=[torch.from_numpy(cars), None, None], min_points=5, ioa_thr=IC.IOA)
    reg.gt_points = [gt_points, None, None]
    info = {}
    out = Calc.assignAnchorsFrames(frames, bevs, IC.NEG, IC.POS, IC.FORCE, info=info, ignore=reg)
    lists = _assign(g, [cars, np.zeros((0, 7), np.float32)])
    w0 = _expected(g, lists, 0, gt_points=gt_points.cpu().numpy(), min_points=5, rects=IC.RECTS['24x20x2'], matrix=IC.MATRIX, quads=C.bev(alike))
    w1 = _expected(g, lists, 1, rects=[IC.RECT_A], matrix=IC.MATRIX)
    for r, w in ((out[0], w0), (out[1], w1)):
        exp = _triples(w['pos'], g) + _triples(w['notneg'], g) + [w['gi']]
        for a, b in zip(_calc_lists(r), exp):
            assert np.array_equal(a, b)
        assert all(t.is_cuda and t.dtype == torch.int64 for t in list(r[0]) + list(r[1]) + [r[2]])
    assert out[2] is None and len(out[1][2]) == 0 and len(out[1][0][0]) == 0 and len(out[1][1][0]) == w1['stats'][1] > 0
    assert info['ignore_stats'] == [a + b for a, b in zip(w0['stats'], w1['stats'])] and info['gt_best'][1] is None
    assert len(info['gt_best'][0]) == 9
    # a first radius of 2 with a 10 m box among the Cars: replayed, and the ignore pass with it
    calls = []
    real_a, real_i = _hip.assign_anchors_frames, _hip.ignore_anchors_frames
    monkeypatch.setattr(Calc, '_anchor_radius', lambda *a: 2)
    monkeypatch.setattr(_hip, 'assign_anchors_frames', lambda *a, **k: (calls.append('a%d' % a[6]), real_a(*a, **k))[1])
    monkeypatch.setattr(_hip, 'ignore_anchors_frames', lambda *a, **k: (calls.append('i'), real_i(*a, **k))[1])
    truck = C.grid_gts('24x20x2')[9:10]
    reg2 = Calc.IgnoreRegions(1, anchors=an7, rects=[torch.tensor([IC.RECT_A])], matrix=[IC.MATRIX])
    out2 = Calc.assignAnchorsFrames([(torch.from_numpy(C.bev(truck)), None)], bevs, IC.NEG, IC.POS, IC.FORCE, ignore=reg2)
    assert calls[0] == 'a2' and calls[1] == 'i' and len(calls) >= 4 and calls[-1] == 'i' and calls[-2].startswith('a')
    lists2 = _assign(g, [truck])
    w2 = _expected(g, lists2, 0, rects=[IC.RECT_A], matrix=IC.MATRIX)
    for a, b in zip(_calc_lists(out2[0]), _triples(w2['pos'], g) + _triples(w2['notneg'], g) + [w2['gi']]):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------------------------
def test_losses_on_the_rewritten_lists():
    """FocalLoss: exact zeros in d_heads' classification columns on every ignored anchor, and the float64 reference with those
    anchors out of the negative set.  VoxelLoss runs on the same lists."""
    from modules import _hip
    g = IC.grid('24x20x2')
    l, w, A = g['l'], g['w'], g['A']
    cars, alike = IC.base_boxes()
    none = np.zeros((0, 7), np.float32)
    lists = _assign(g, [cars, none])
    pos, neg, gi, counts, off = lists
    gt_points = _dev([9, 5, 30, 7, 4, 12, 0, 5, 6], np.int32)
    rects = _dev(np.array(IC.RECTS['24x20x2'] + [IC.RECT_A], np.float32))
    mats = _dev(np.stack([IC.MATRIX, IC.MATRIX]))
    p2, n2, g2, words = _hip.ignore_anchors_frames(pos, neg, gi, counts, _dev(g['anchors']), _dev(g['bevs']), _dev(off, np.int32), gt_points, 5,
                                                   rects, _dev([0, 2, 3], np.int32), mats, _dev(C.bev(alike)), _dev([0, 2, 2], np.int32), IC.IOA)
    F = 2
    host = words.cpu().numpy()
    c2, stats, status = host[:2 * F].reshape(F, 2), host[2 * F:6 * F].reshape(F, 4), host[6 * F]
    assert status == 0 and stats[0].min() > 0 and stats[1].tolist()[1] > 0 and c2[1, 0] == 0 and c2[1, 1] > 0
    heads = torch.randn((F * l * w, 8 * A), generator=torch.Generator().manual_seed(11)).cuda()
    gts = _dev(cars)
    losses, d = _hip.focal_loss_frames(heads, F, l, w, A, p2, n2, g2, words[:2 * F].view(F, 2), gts, _dev(off, np.int32), _dev(g['anchors']),
                                       0.25, 2.0, 1.0, 2.0)
    case = dict(F=F, l=l, w=w, A=A, heads=heads.cpu().numpy(), pos=p2.cpu().numpy(), neg=n2.cpu().numpy(), gi=g2.cpu().numpy(), counts=c2,
                gts=cars, gt_off=np.asarray(off, np.int32), anchors=g['anchors'])
    ref_losses, ref_d, (positive, ignored) = FR.focal_ref(case)
    # the ignored set is the rule's: not negative and not positive, the newly ignored anchors among them
    for f, k in ((0, dict(gt_points=gt_points.cpu().numpy(), min_points=5, rects=IC.RECTS['24x20x2'], matrix=IC.MATRIX, quads=C.bev(alike))),
                 (1, dict(rects=[IC.RECT_A], matrix=IC.MATRIX))):
        want = _expected(g, lists, f, **k)
        nn = np.zeros((l * w * A,), bool)
        nn[want['notneg']] = True
        nn[want['pos']] = False
        assert np.array_equal(ignored[f].reshape(-1), nn) and nn.sum() >= sum(want['stats'][:3]) > 0
    d_cls = d.view(F, l, w, 8 * A)[..., :A].cpu().numpy()
    assert (d_cls[ignored] == 0.0).all() and (d_cls[~ignored] != 0.0).all()
    scale = float(ref_d.abs().max())
    np.testing.assert_allclose(losses.double().cpu().numpy(), ref_losses.numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(d.double().cpu().numpy(), ref_d.numpy(), rtol=1e-5, atol=1e-7 * scale)
    # VoxelLoss on the same lists, frame 0 (positives) and frame 1 (none: n_pos = 0 with n_notneg > 0)
    score = torch.sigmoid(heads.view(F, l, w, 8 * A)[..., :A]).contiguous()
    reg = heads.view(F, l, w, 8 * A)[..., A:].contiguous()
    for f in range(F):
        n_pos, n_neg = int(c2[f, 0]), int(c2[f, 1])
        regress = n_pos > 0
        ls, dscore, _ = _hip.voxel_loss(score[f], reg[f] if regress else None, p2[f] if regress else None, n2[f], g2[f] if regress else None,
                                        n_pos, n_neg, gts if regress else None, _dev(g['anchors']) if regress else None, A, 1.5, 1.0, 1e-6)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(ls).all()) and bool(torch.isfinite(dscore).all())
        listed = np.zeros((l, w, A), bool)
        nl = n2[f, :, :n_neg].cpu().numpy()
        listed[nl[0], nl[1], nl[2]] = True
        ds = dscore.cpu().numpy()
        assert (ds[listed & ~positive[f]] == 0.0).all() and (ds[~listed] != 0.0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# geometry helpers
# ---------------------------------------------------------------------------------------------------------------------------
def test_geometry_helpers_against_the_augmentation_kernels():
    import modules.config as cfg
    from modules import pipeline as pl
    from modules.augment import Geometry
    r = np.random.default_rng(3)
    F, P = 3, 500
    pts = np.zeros((F, P, 6), np.float32)
    pts[..., 0] = r.uniform(20.0, 50.0, (F, P))
    pts[..., 1] = r.uniform(-15.0, 15.0, (F, P))
    pts[..., 2] = r.uniform(-2.0, 0.5, (F, P))
    pts[..., 3:] = r.uniform(0.0, 1.0, (F, P, 3))
    boxes = np.array([[30.0, -8.0, -1.5, 3.9, 1.6, 1.5, 0.2], [38.0, 0.0, -1.6, 4.1, 1.7, 1.6, -2.9], [45.0, 9.0, -1.4, 3.7, 1.5, 1.4, 1.5]], np.float32)
    glob = np.array([[0.2, 1.03, 0.0, 0.0], [-0.15, 0.97, 1.0, 0.0], [0.0, 1.0, 1.0, 0.0]], np.float32)
    from modules import _hip
    noise = np.zeros((F, _hip.GT_PASTE_MAX_BOXES, 4, 4), np.float32)
    batch = pl.FrameBatch(torch.from_numpy(pts).cuda(), None, torch.full((F,), P, dtype=torch.int32).cuda(), [None] * F)
    res = Geometry.augmentGeometryFrames(batch, [torch.from_numpy(boxes)] * F, noise, glob, iou_thr=0.05, shuffle=False)
    lo, hi = np.array(cfg.velorange[:3]), np.array(cfg.velorange[3:])
    for f in range(F):
        want = Geometry.transform_boxes(boxes, glob[f])
        assert res.kept[f] == [0, 1, 2] and np.abs(res.bbox3d[f].cpu().numpy() - want).max() <= 1e-5
        G = Geometry.global_matrix(glob[f])
        moved = (np.concatenate([pts[f, :, :3].astype(np.float64), np.ones((P, 1))], axis=1) @ G.T)[:, :3]
        inside = np.all((moved >= lo + 1e-3) & (moved < hi - 1e-3), axis=1)
        edge = np.all((moved >= lo - 1e-3) & (moved < hi + 1e-3), axis=1) & ~inside
        assert not edge.any() and inside.sum() == res.n_points[f] > 300
        got = batch.points6[f, :res.n_points[f]].cpu().numpy()
        assert np.abs(got[:, :3] - moved[inside]).max() <= 1e-4                       # the order of the kept points is kept
        assert np.array_equal(got[:, 3:], pts[f, inside, 3:])                         # ... and their pixel: M inv(G) finds it again


# ---------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------
VAN = 'Van 0.00 0 0.00 300.00 150.00 420.00 230.00 2.20 1.90 5.00 %.4f %.4f %.4f %.4f\n'
DONTCARE = 'DontCare -1 -1 -10 %.2f %.2f %.2f %.2f -1 -1 -1 -1000 -1000 -1000 -10\n'


def _extend_labels(root, names):
    """A Van 3 m beside the first Car of every frame and two DontCare rectangles, appended to the label files of the tree."""
    from modules.data import Synthetic as S
    v2c = S.KITTI_CALIB['Tr_velo_to_cam']
    for name in names:
        path = os.path.join(root, 'training', 'label_2', name + '.txt')
        with open(path) as f:
            car = f.readline().split(' ')
        cam = np.array([float(v) for v in car[11:14]])
        lid = np.linalg.inv(v2c) @ np.array([cam[0], cam[1], cam[2], 1.0])
        van = v2c @ np.array([lid[0], lid[1] + 3.0, lid[2], 1.0])
        with open(path, 'a') as f:
            f.write(VAN % (van[0], van[1], van[2], float(car[14])))
            f.write(DONTCARE % (560.0, 150.0, 700.0, 230.0))
            f.write(DONTCARE % (100.0, 160.0, 180.0, 200.0))


def test_batch_from_dataset_with_ignore_regions(tmp_path):
    import modules.config as cfg
    from modules import Calc, pipeline as pl
    from modules.data import Load, Preprocessing as pre, Synthetic as S
    from modules.voxelnet.FocalLoss import FocalLoss
    import train_like
    root = str(tmp_path / 'kitti')
    names = S.write_kitti_tree(root, [0, 1], points=3000, raw_points=9000)
    _extend_labels(root, names)
    ds = Load.createDataset(names, root=root)
    labels = Load.readIgnoreLabels(names, root=root, classes=('Van',))
    assert all(tuple(r.shape) == (2, 4) and tuple(b.shape) == (1, 7) for r, b in labels)
    dev = torch.device('cuda')
    anchors = pre.createAnchors(cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2, cfg.velorange, cfg.carsize)
    an7 = anchors.reshape(anchors.shape[:2] + (-1, 7))
    bevs = Calc.bbox3d2bev(an7).to(dev).contiguous()
    infos = []

    def assigner(frames, ignore=None):
        infos.append({})
        return Calc.assignAnchorsFrames(frames, bevs, 0.45, 0.6, 0.1, info=infos[-1], ignore=ignore)
    keep = {}
    np.random.seed(0)
    batch, targets = pl.batch_from_dataset(ds, names, dev, bevs, train_like.fpn_maps_for, cap_points=3000, assigner=assigner,
                                           ignore={'labels': labels, 'anchors': an7, 'min_points': 5, 'keep': keep})
    np.random.seed(0)
    _, plain = pl.batch_from_dataset(ds, names, dev, bevs, train_like.fpn_maps_for, cap_points=3000, assigner=assigner)
    regions = keep['regions']
    assert 'ignore_stats' in infos[0] and 'ignore_stats' not in infos[1]
    demoted, by_rect, by_box, sparse = infos[0]['ignore_stats']
    print('end to end: %s' % infos[0]['ignore_stats'])
    assert by_rect > 0 and by_box > 0
    for k, (t, p) in enumerate(zip(targets, plain)):
        # the count is the cloud's own: the same boxes and points through the reference
        cars = ds[k][3].numpy()
        cnt, _ = IR.point_counts64(batch.points6[k:k + 1].cpu().numpy(), batch.n_points[k:k + 1].cpu().numpy(), cars, [0, len(cars)])
        assert np.array_equal(regions.gt_points[k].cpu().numpy(), cnt)
        n_sparse = int((cnt < 5).sum())
        assert t is not None and p is not None and tuple(t[3].shape) == tuple(p[3].shape)
        kept = ~np.isin(p[2].cpu().numpy(), np.flatnonzero(cnt < 5))
        for a, b in zip(t[0], p[0]):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()[kept])
        assert np.array_equal(t[2].cpu().numpy(), p[2].cpu().numpy()[kept]) and len(t[1][0]) > len(p[1][0])
        sparse -= n_sparse
    assert sparse == 0
    packed, has_reg = FocalLoss.pack_targets(targets, dev)
    assert packed.counts.cpu().tolist() == [[len(t[0][0]), len(t[1][0])] for t in targets]
    with pytest.raises(ValueError):
        pl.batch_from_dataset(ds, names, dev, bevs, train_like.fpn_maps_for, cap_points=3000, ignore={'labels': labels, 'anchors': an7})
    # the prefetch loader builds the same targets on its own stream
    from modules.data.Prefetch import PrefetchLoader
    by_name = dict(zip(names, labels))
    name_of = {id(d): n for d, n in zip(ds, names)}
    loader = PrefetchLoader([ds], lambda d: name_of[id(d)], torch.device('cuda', 0), bevs, train_like.fpn_maps_for, 3000, assigner=assigner,
                            ignore={'labels_of': lambda n: by_name[n], 'anchors': an7, 'min_points': 5})
    got = list(loader)
    assert len(got) == 1 and infos[-1]['ignore_stats'] == infos[0]['ignore_stats']
    torch.cuda.synchronize()
    for t, u in zip(targets, got[0][1]):
        for a, b in zip(list(t[0]) + list(t[1]) + [t[2], t[3]], list(u[0]) + list(u[1]) + [u[2], u[3]]):
            assert torch.equal(a, b)
    with pytest.raises(ValueError):
        PrefetchLoader([ds], lambda d: name_of[id(d)], torch.device('cuda', 0), bevs, train_like.fpn_maps_for, 3000, ignore={'labels_of': lambda n: by_name[n]})


def test_train_like_with_the_ignore_flags(tmp_path):
    from modules.data import Synthetic as S
    root, ckpt = str(tmp_path / 'kitti'), str(tmp_path / 'ckpt')
    names = S.write_kitti_tree(root, [0, 1, 2, 3], points=3000, raw_points=9000)
    _extend_labels(root, names)
    p = subprocess.run([sys.executable, os.path.join(REPO, 'mvxnet-makise_amd', 'train_like.py'), root, '--mode', 'fast', '--frames', '2',
                        '--steps', '2', '--points', '3000', '--targets', 'maxiou', '--loss', 'focal', '--ignore-dontcare',
                        '--ignore-classes', 'Van', '--min-gt-points', '5', '--checkpoints', ckpt],
                       capture_output=True, text=True, timeout=600, cwd=REPO)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [s for s in p.stdout.splitlines() if 'ignored:' in s]
    assert len(line) == 1, p.stdout[-2000:]
    import re
    nums = [int(v) for v in re.findall(r'(\d+) (?:positive|anchor|by a look|sparse)', line[0])]
    assert len(nums) == 4 and nums[1] > 0 and nums[2] > 0, line[0]
    assert 'ignore regions: 8 DontCare rectangle(s), 4 box(es) of Van' in p.stdout
    assert os.path.exists(os.path.join(ckpt, 'epoch1.pkl'))
