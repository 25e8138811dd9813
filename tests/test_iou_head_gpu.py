"""The IoU-aware confidence head on the GPU (csrc/loss_frames.hip mvx_focal_loss_iou_frames, csrc/detect.hip
mvx_detect_frames_iou, the IoU columns of modules/rpn_frames.py) against the float64 restatement tests/iou_head_ref.py, on the
inputs of tests/iou_head_cases.py.

Tolerances.  The IoU target q: per case, four times the worst distance between the exact float64 clip and the project's
accepted f32 arithmetic (the C oracle's clipping on O.bbox3d2bev quads, times the vertical term; iou_head_ref.q_f32) over the
case's own pairs -- the device differs from the oracle in cosf / sinf and expf by a few ulp on operands of the same size.
Entries that must be 0 (circles apart, no vertical overlap, an overflowing decode) are compared exactly, skipped entries are
-1.  Losses: relative 1e-5.  IoU gradient: rtol 1e-5 plus atol = 1e-7 * max |reference gradient| (the direction tests' bars)
plus iou_scale * the q bar per entry of the anchor: q is the term's one new error source and enters the gradient with
factor iou_scale.  The cls, reg and dir terms are compared BITWISE with mvx_focal_loss_dir_frames on the same inputs (the
losses also at rtol 1e-5 with the reference).  Every test prints the worst figures before it asserts.

Measured on an MI355X (worst |q - q64| against the bar of the case): see DESIGN.md 3.35."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

import direction_cases as DC
import iou_head_cases as IC
import iou_head_ref as IR

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'mvxnet-makise_amd')
P = dict(alpha=0.25, gamma=2.0, cls_weight=1.0, reg_weight=2.0, dir_weight=0.2, dir_offset=math.pi / 4, iou_weight=1.0)
LISTS = ('pos', 'neg', 'gi', 'counts', 'gts', 'gt_off', 'anchors')


@functools.lru_cache(maxsize=None)
def _reference(name, saturated=False):
    """(reference tuple, q bar of the case, worst f32-oracle distance): computed once per case and shared, never modified."""
    case = IC.with_iou(name, saturated)
    q = IR.targets(case)[0]
    ref = IR.iou_head_ref(case, q=q, **P)
    q32 = IR.q_f32(case, case['recs'])
    q64 = np.array([r['q'] for r in case['recs']])
    ok = ~np.isnan(q32)
    worst = float(np.abs(q32[ok] - q64[ok]).max())
    return ref, 4.0 * worst, worst


def _dev(case):
    return {k: torch.from_numpy(np.ascontiguousarray(case[k])).cuda() for k in LISTS}


def _inputs(case, layout):
    """'inside': direction and IoU logits are columns 8A..9A and 9A..10A of the wide rows; 'separate': (rows, 4) tensors of
    their own beside plain 8A-wide rows."""
    A = case['A']
    if layout == 'inside':
        heads = torch.from_numpy(IC.wide_rows(case)).cuda()
        return heads, heads[:, 8 * A:9 * A], heads[:, 9 * A:10 * A]
    heads = torch.from_numpy(np.ascontiguousarray(case['heads'])).cuda()
    own = []
    for key in ('dir', 'iou'):
        t = torch.full((heads.shape[0], 4), 7.0, dtype=torch.float32, device='cuda')
        t[:, :A] = torch.from_numpy(case[key]).cuda()
        own.append(t[:, :A])
    return heads, own[0], own[1]


def _run(case, layout='inside', want_grads=True, **kw):
    """-> (losses (F,4), d_heads, d_dir, d_iou, q (F,cap)) on the host."""
    from modules import _hip
    p = dict(P, **kw)
    t = _dev(case)
    heads, dirl, ioul = _inputs(case, layout)
    out = _hip.focal_loss_iou_frames(heads, dirl, ioul, case['F'], case['l'], case['w'], case['A'], t['pos'], t['neg'], t['gi'],
                                     t['counts'], t['gts'], t['gt_off'], t['anchors'], p['alpha'], p['gamma'], p['cls_weight'],
                                     p['reg_weight'], p['dir_weight'], p['dir_offset'], p['iou_weight'], want_grads=want_grads,
                                     want_q=True)
    torch.cuda.synchronize()
    if not want_grads:
        assert out[1] is None and out[2] is None and out[3] is None
        return out[0].cpu(), None, None, None, out[4].cpu()
    return out[0].cpu(), out[1].cpu(), out[2].cpu().contiguous(), out[3].cpu().contiguous(), out[4].cpu()


def _run_dir(case, layout):
    """mvx_focal_loss_dir_frames on the same inputs (the wide rows keep the IoU logits in their last columns)."""
    from modules import _hip
    t = _dev(case)
    heads, dirl, _ = _inputs(case, layout)
    out = _hip.focal_loss_dir_frames(heads, dirl, case['F'], case['l'], case['w'], case['A'], t['pos'], t['neg'], t['gi'],
                                     t['counts'], t['gts'], t['gt_off'], t['anchors'], P['alpha'], P['gamma'], P['cls_weight'],
                                     P['reg_weight'], P['dir_weight'], P['dir_offset'])
    torch.cuda.synchronize()
    return out[0].cpu(), out[1].cpu(), out[2].cpu().contiguous()


def _check_q(case, q, ref_q, bar):
    recs = case['recs']
    ref_q = np.asarray(ref_q)
    got = q.double().numpy()
    assert got.shape == ref_q.shape
    skipped = ref_q == -1.0
    assert (got[skipped] == -1.0).all() and (got[~skipped] >= 0.0).all() and (got[~skipped] <= 1.0).all()
    zero = np.zeros_like(skipped)
    for r in recs:
        zero[r['f'], r['k']] = IR.must_be_zero(r)
    assert zero.sum() >= 3 and (got[zero] == 0.0).all()                       # bit for bit
    rest = ~skipped & ~zero
    err = float(np.abs(got[rest] - ref_q[rest]).max())
    print('q: worst |device - float64| = %.3e over %d entries, bar %.3e (4 x the f32 oracle\'s %.3e); %d exact zeros, %d skipped'
          % (err, rest.sum(), bar, bar / 4, zero.sum(), skipped.sum()))
    assert err <= bar


def _iou_atol(case, bar, iou_weight):
    """(rows, A): iou_scale * q bar, once per entry of the anchor."""
    F, l, w, A = case['F'], case['l'], case['w'], case['A']
    atol = np.zeros((F, l, w, A))
    for r in case['recs']:
        atol[r['f'], r['x'], r['y'], r['z']] += iou_weight / max(1, int(case['counts'][r['f'], 0])) * bar
    return atol.reshape(F * l * w, A)


def _check(case, got, name, saturated=False, layout='inside'):
    (ref_losses, ref_d, ref_dd, ref_du, ref_q), bar, _ = _reference(name, saturated)
    losses, d, dd, du, q = got
    A = case['A']
    for t in (losses, d, dd, du):
        assert bool(torch.isfinite(t).all())
    _check_q(case, q, ref_q, bar)
    err_l = float(((losses.double() - ref_losses).abs() / ref_losses.abs().clamp_min(1e-300))[ref_losses != 0].max())
    scale = float(ref_du.abs().max())
    tol = 1e-5 * ref_du.abs().numpy() + 1e-7 * scale + _iou_atol(case, bar, P['iou_weight'])
    err_u = float((np.abs(du.double().numpy() - ref_du.numpy()) / tol).max())
    print('worst loss error %.2e (relative), worst IoU gradient error %.2e of its tolerance' % (err_l, err_u))
    np.testing.assert_allclose(losses.double().numpy(), ref_losses.numpy(), rtol=1e-5, atol=0)
    assert (np.abs(du.double().numpy() - ref_du.numpy()) <= tol).all()
    # the other three terms: mvx_focal_loss_dir_frames on the same inputs, bit for bit (its own tests hold it to direction_ref)
    dl, ddh, ddd = _run_dir(case, layout)
    assert torch.equal(dl, losses[:, :3]) and torch.equal(ddh[:, :9 * A if layout == 'inside' else 8 * A], d[:, :9 * A if layout == 'inside' else 8 * A])
    assert torch.equal(ddd, dd)
    # layout: the IoU gradient sits in columns 9A..10A of the wide rows, nothing flows into the regression from it
    if layout == 'inside':
        assert d.shape[1] == (10 * A + 3) // 4 * 4 and torch.equal(d[:, 9 * A:10 * A], du) and torch.equal(d[:, 8 * A:9 * A], dd)
        if d.shape[1] > 10 * A:
            assert float(d[:, 10 * A:].abs().max()) == 0.0
    else:
        assert d.shape[1] == 8 * A
    listed = np.zeros(du.shape, bool).reshape(case['F'], case['l'], case['w'], A)
    for r in case['recs']:
        listed[r['f'], r['x'], r['y'], r['z']] = True
    assert float(du.reshape(listed.shape)[torch.from_numpy(~listed)].abs().max()) == 0.0


@pytest.mark.parametrize('layout', ['inside', 'separate'])
def test_case1_duplicates_empty_frames_and_both_layouts(layout):
    case = IC.with_iou('case1')
    got = _run(case, layout)
    _check(case, got, 'case1', layout=layout)
    losses = got[0]
    assert float(losses[1, 3]) == 0.0 and float(losses[2, 3]) == 0.0 and float(losses[0, 3]) > 0.0
    assert float(got[4][1:].max()) == -1.0                                     # frames without positives: every slot skipped
    DC.check_case(dict(case, counts=case['counts']))                           # beyond the counts: GARBAGE, never read
    assert torch.equal(_run(case, layout)[0], losses)                          # the four losses repeat bitwise, duplicates or not
    assert torch.equal(_run(case, layout, want_grads=False)[0], losses)


@pytest.mark.parametrize('layout', ['inside', 'separate'])
def test_saturated_iou_logits_stay_finite_and_accurate(layout):
    case = IC.with_iou('case1', True)
    assert float(np.abs(case['iou']).max()) == 90.0
    _check(case, _run(case, layout), 'case1', True, layout=layout)


@pytest.mark.parametrize('layout', ['inside', 'separate'])
def test_case3_strided_loop_several_partials_bitwise_repeatable_and_forward_only(layout):
    case = IC.with_iou('case3')
    assert case['gi'].shape[1] > 256 and int(case['counts'][0, 0]) % 128 != 0      # nq = 3, a ragged last round
    first = _run(case, layout)
    _check(case, first, 'case3', layout=layout)
    second = _run(case, layout)
    for a, b in zip(first, second):                                            # no anchor is listed twice here
        assert torch.equal(a, b)
    losses, none, _, _, q = _run(case, layout, want_grads=False)
    assert none is None and torch.equal(losses, first[0]) and torch.equal(q, first[4])


def test_case4_three_anchors_separate_tensors():
    case = IC.with_iou('case4')
    _check(case, _run(case, 'separate'), 'case4', layout='separate')


def test_case5_sixteen_frames():
    case = IC.with_iou('case5')
    _check(case, _run(case), 'case5')


def test_zero_weight_leaves_the_direction_results_and_no_target_output_is_needed():
    from modules import _hip
    case = IC.with_iou('case5')
    losses, d, dd, du, _ = _run(case, iou_weight=0.0)
    dl, ddh, ddd = _run_dir(case, 'inside')
    assert torch.equal(losses[:, :3], dl) and float(losses[:, 3].abs().max()) == 0.0 and float(du.abs().max()) == 0.0
    assert torch.equal(d[:, :18], ddh[:, :18]) and torch.equal(dd, ddd)
    t = _dev(case)
    heads, dirl, ioul = _inputs(case, 'inside')
    out = _hip.focal_loss_iou_frames(heads, dirl, ioul, case['F'], case['l'], case['w'], case['A'], t['pos'], t['neg'], t['gi'],
                                     t['counts'], t['gts'], t['gt_off'], t['anchors'], *[P[k] for k in P])       # q_out = NULL
    torch.cuda.synchronize()
    assert out[4] is None and torch.equal(out[0].cpu(), _run(case)[0])


# ---- decode -----------------------------------------------------------------------------------------------------------------
def _detect(case, heads, alpha, with_iou=True, debug=True):
    from modules import _hip
    F, l, w, A = case['F'], case['l'], case['w'], case['A']
    v = heads.view(F, l, w, 20)
    anc = torch.from_numpy(case['anchors']).cuda()
    return _hip.detect_frames(v[..., :A], v[..., A:8 * A], anc, F, l, w, A, case['score_thr'], case['iou_thr'], 32, 16, debug=debug,
                              dir_logits=v[..., 8 * A:9 * A], dir_offset=case['dir_offset'],
                              iou_logits=v[..., 9 * A:10 * A] if with_iou else None, iou_alpha=alpha)


@pytest.mark.parametrize('alpha', [0.5, 1.0])
def test_decode_ranks_and_scores_by_the_rectified_score(alpha):
    case = IC.decode_case()
    F = case['F']
    heads = torch.from_numpy(IC.decode_heads(case)).cuda()
    boxes, scores, idx, meta, cand, _, _ = _detect(case, heads, alpha)
    torch.cuda.synchronize()
    counts, n_cand, status = meta.tolist()
    for f in range(F):
        c, u = case['cls'][f].reshape(-1), case['iou'][f].reshape(-1)
        keep, want, n = IR.candidates(c, u, alpha, case['score_thr'], 32)
        got = cand[f].cpu().numpy()
        assert n_cand[f] == n and status[f] == 0
        assert list(got[:len(keep)]) == list(keep) and (got[len(keep):] == -1).all()      # selection and order, exactly
        sp = case['special'][f]
        assert sp['nan'] not in got and sp['low'] not in got                   # the NaN IoU logit drops its anchor
        lo, hi = sorted(sp['tie'])
        where = list(got)
        assert where.index(lo) + 1 == where.index(hi)                          # identical logits: lowest anchor index first
        if alpha == 1.0:                                                       # the IoU logit alone
            assert list(u[keep]) == sorted(u[keep], reverse=True)
        k = counts[f]
        kept = idx[f, :k].cpu().numpy()
        by = {int(a): s for a, s in zip(keep, want)}
        ref_scores = np.array([by[int(a)] for a in kept])
        got_scores = scores[f, :k].cpu().double().numpy()
        print('frame %d: %d candidates, %d kept, worst relative score error %.2e'
              % (f, n, k, np.abs(got_scores / ref_scores - 1).max()))
        np.testing.assert_allclose(got_scores, ref_scores, rtol=1e-5, atol=0)
        assert (np.diff(got_scores) <= 0).all() and 0 < k <= len(keep)


def test_decode_with_alpha_zero_or_a_null_head_is_the_direction_decode_bitwise():
    case = IC.decode_case()
    heads = torch.from_numpy(IC.decode_heads(case)).cuda()
    old = _detect(case, heads, 0.5, with_iou=False, debug=False)               # mvx_detect_frames_dir
    zero = _detect(case, heads, 0.0, debug=False)                              # a = 0: cls^1 iou^0, the head is not read
    torch.cuda.synchronize()
    for o, z in zip(old, zero):
        assert torch.equal(o, z)
    assert int(old[3][1, 0]) == 6                                              # the NaN and the low IoU logit do not matter here
    from modules.detect import postprocess
    anchors = torch.from_numpy(case['anchors'].reshape(case['l'], case['w'], 14))
    kw = dict(score_thr=case['score_thr'], iou_thr=case['iou_thr'], pre_max=32, post_max=16, dir_offset=case['dir_offset'])
    off = postprocess(heads, anchors, case['F'], case['l'], case['w'], **kw)               # a heads tensor: None means off
    on = postprocess(heads, anchors, case['F'], case['l'], case['w'], iou=True, **kw)
    v = heads.view(case['F'], case['l'], case['w'], 20).permute(0, 3, 1, 2)
    maps = postprocess((v[:, :2], v[:, 2:16], v[:, 16:18], v[:, 18:20]), anchors, case['F'], case['l'], case['w'], **kw)   # a 4th map: on
    for f in range(case['F']):
        assert torch.equal(off[f]['scores'], old[1][f, :len(off[f]['scores'])]) and off[f]['n_candidates'] == 6
        assert on[f]['n_candidates'] == 4 and maps[f]['n_candidates'] == 4
        assert torch.equal(on[f]['scores'], maps[f]['scores']) and torch.equal(on[f]['boxes'], maps[f]['boxes'])


# ---- the per-frame autograd path, the whole step, the tools -------------------------------------------------------------------
def test_forward_of_an_iou_model_returns_score_and_reg_and_leaves_iou_without_gradient(golden):
    import modules.config as cfg
    from MVXNet import MVXNet
    from modules import whole
    g = golden('mvxnet_small')
    old = list(cfg.config['voxelshape'])
    cfg.config['voxelshape'] = [int(v) for v in g['voxelshape']]
    try:
        dev = torch.device('cuda')
        torch.manual_seed(4)
        model = MVXNet(direction=True, iou=True).to(dev)
        feats = [torch.from_numpy(g[k])[None].to(dev) for k in ('f0', 'f1', 'f2')]
        idx = torch.from_numpy(g['idx']).to(dev)
        imsize = torch.from_numpy(g['imsize_hw']).to(dev)
        h1, w1 = cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2

        def vox():
            return torch.from_numpy(g['voxels'].copy())[None].to(dev)
        with torch.no_grad():
            heads = whole.forward_heads(model, vox(), feats, idx, imsize)
        assert heads.shape == (h1 * w1, 20) and float(heads[:, 18:].abs().max()) > 0.0      # logits, not padding
        score, reg = model(vox(), feats, idx, [None], imsize)
        assert score.shape == (1, 2, h1, w1) and reg.shape == (1, 14, h1, w1)
        v = heads.view(1, h1, w1, 20)
        assert torch.equal(score.detach(), torch.sigmoid(v[..., :2]).permute(0, 3, 1, 2))
        assert torch.equal(reg.detach(), v[..., 2:16].permute(0, 3, 1, 2))
        (score.sum() + reg.square().sum()).backward()
        torch.cuda.synchronize()
        rpn = model.backbone.rpn
        for p in (rpn.iou.weight, rpn.iou.bias, rpn.dir.weight, rpn.dir.bias):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0
        assert float(rpn.cls.weight.grad.abs().max()) > 0.0 and float(rpn.reg.bias.grad.abs().max()) > 0.0
    finally:
        cfg.config['voxelshape'] = old


def _case_of_step(heads, F, l, w, targets, anchors):
    from test_direction_gpu import _case_of_step as direction
    case = direction(heads, F, l, w, targets, anchors)
    case['iou'] = np.ascontiguousarray(heads.cpu().numpy()[:, 18:20])
    return case


def test_whole_model_step_with_the_iou_criterion(tmp_path):
    """pipeline.train_step_full on the two synthetic frames of the direction test with MVXNet(direction=True, iou=True) and
    FocalLoss(direction=True, iou=True): losses against the reference on the step's own head output, the IoU head's bias
    gradient = the column sums of the reference IoU gradient, and both mismatched pairings refused before any launch."""
    sys.path.insert(0, PKG)
    import modules.config as cfg
    from modules import parallel, pipeline as pl
    from modules.Calc import bbox3d2bev
    from modules.data import Load, Preprocessing as pre, Synthetic as S
    from modules.voxelnet.FocalLoss import FocalLoss
    from modules.Extension import MvxHipError
    from MVXNet import MVXNet
    import train_like
    root = str(tmp_path / 'kitti')
    S.write_kitti_tree(root, [0, 1], points=3000, raw_points=9000)
    ds = Load.createDataset(['000000', '000001'], root=root)
    dev = torch.device('cuda')
    anchors = pre.createAnchors(cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2, cfg.velorange, cfg.carsize)
    bevs = bbox3d2bev(anchors.reshape(anchors.shape[:2] + (-1, 7))).to(dev).contiguous()
    anchors = anchors.to(dev)
    torch.manual_seed(0)
    model = MVXNet(direction=True, iou=True).to(dev)
    bucket = parallel.GradBucket([p for p in model.parameters() if p.requires_grad])
    crit = FocalLoss(direction=True, iou=True)
    np.random.seed(0)
    batch, targets = pl.batch_from_dataset(ds, ['000000', '000001'], dev, bevs, train_like.fpn_maps_for, cap_points=3000)
    assert any(t is not None and len(t[0][0]) > 0 for t in targets)
    bucket.zero()
    rpn = model.backbone.rpn
    with pytest.raises(MvxHipError, match='rpn.iou'):                          # an IoU model needs the IoU criterion
        pl.train_step_full(model, batch, targets, FocalLoss(direction=True), anchors, cfg.imsize)
    assert float(bucket.flat.abs().max()) == 0.0                               # refused before anything was launched
    k = {}
    out = pl.train_step_full(model, batch, targets, crit, anchors, cfg.imsize, keep=k)
    torch.cuda.synchronize()
    F, h1, w1 = k['geom'][0], k['geom'][5], k['geom'][6]
    assert F == 2 and k['heads'].shape == (F * h1 * w1, 20) and float(k['heads'][:, 18:].abs().max()) > 0.0
    tl = [targets[f] for f in out['live']]
    case = _case_of_step(k['heads'], F, h1, w1, tl, anchors)
    ref_losses, ref_d, ref_dd, ref_du, _ = IR.iou_head_ref(case, crit.alpha, crit.gamma, crit.cls_weight, crit.reg_weight,
                                                           crit.dir_weight, crit.dir_offset, crit.iou_weight)
    has = [t is not None and len(t[0][0]) > 0 for t in tl]
    print('step losses (cls, reg, dir, iou): %s / %s / %s / %s' % (out['cls'], out['reg'], out['dir'], out['iou']))
    np.testing.assert_allclose(out['cls'], ref_losses[:, 0].numpy(), rtol=1e-5)
    np.testing.assert_allclose(out['reg'], ref_losses[:, 1].numpy()[has], rtol=1e-5)
    np.testing.assert_allclose(out['dir'], ref_losses[:, 2].numpy()[has], rtol=1e-5)
    np.testing.assert_allclose(out['iou'], ref_losses[:, 3].numpy()[has], rtol=1e-5)
    np.testing.assert_allclose(out['loss'], [float(r.sum()) if h else float(r[0]) for r, h in zip(ref_losses, has)], rtol=1e-5)
    assert len(out['iou']) == sum(has) and all(v > 0 for v in out['iou'])
    for name, p in model.named_parameters():
        if p.requires_grad:
            assert bool(torch.isfinite(p.grad).all()), name
    for got, want in ((rpn.dir.bias.grad, ref_dd.sum(dim=0)), (rpn.iou.bias.grad, ref_du.sum(dim=0))):
        err = float((got.cpu().double() - want).abs().max() / want.abs().max())
        print('bias gradient vs column sums of the reference gradient: %.2e' % err)
        assert err < 1e-4
    assert float(rpn.iou.weight.grad.abs().max()) > 0.0
    # the other mismatch: an IoU criterion on a direction model without rpn.iou
    torch.manual_seed(0)
    direct = MVXNet(direction=True).to(dev)
    dbucket = parallel.GradBucket([p for p in direct.parameters() if p.requires_grad])
    dbucket.zero()
    with pytest.raises(MvxHipError, match='rpn.iou'):
        pl.train_step_full(direct, batch, targets, crit, anchors, cfg.imsize)
    assert float(dbucket.flat.abs().max()) == 0.0


def test_train_like_detect_like_and_the_detect_calls_with_the_iou_head(tmp_path, golden, capsys):
    sys.path.insert(0, PKG)
    import detect_like
    import modules.config as cfg
    import train_like
    from modules import pipeline as pl
    from modules.Calc import bbox3d2bev
    from modules.data import Load, Preprocessing as pre
    from modules.detect import detect_frame_set
    from MVXNet import MVXNet
    root, ck = str(tmp_path / 'kitti'), str(tmp_path / 'ck')
    args = train_like.parse_args([root, '--direction', '--iou-head', '--loss', 'focal', '--mode', 'fast', '--frames', '2', '--steps',
                                  '2', '--synthetic', '3', '--points', '3000', '--checkpoints', ck])
    np.random.seed(0)
    r = train_like.train(args)
    text = capsys.readouterr().out
    assert r['steps'] == 2 and len(r['losses']) == 3 and all(np.isfinite(v) for v in r['losses'])
    assert 'average IoU loss' in text and 'IoU head: iou_weight=1' in text
    path = os.path.join(ck, 'epoch1.pkl')
    state = torch.load(path, map_location='cpu')
    assert 'backbone.rpn.iou.weight' in state and 'backbone.rpn.iou.bias' in state
    names = open(os.path.join(root, 'ImageSets', 'train.txt')).read().split()

    def scores_of(alpha, out):
        detect_like.main(detect_like.parse_args([root, '--checkpoint', path, '--out', out, '--frames', '2', '--points', '3000',
                                                 '--score-thr', '0', '--iou-alpha', str(alpha)]))
        assert all(os.path.exists(os.path.join(out, n + '.txt')) for n in names)
        return [float(line.split()[-1]) for n in names for line in open(os.path.join(out, n + '.txt')).read().splitlines()]
    half, plain = scores_of(0.5, str(tmp_path / 'res_half')), scores_of(0.0, str(tmp_path / 'res_zero'))
    assert 'IoU head of the checkpoint' in capsys.readouterr().out             # the key is recognised
    assert len(half) > 0 and len(plain) > 0 and sorted(half) != sorted(plain)  # --iou-alpha is honoured
    # MVXNet.detect of the loaded model on the small golden frame, rectified and not
    g = golden('mvxnet_small')
    dev = torch.device('cuda')
    model = MVXNet(direction=True, iou=True).to(dev)
    model.load_state_dict(state)
    old = list(cfg.config['voxelshape'])
    cfg.config['voxelshape'] = [int(v) for v in g['voxelshape']]
    try:
        feats = [torch.from_numpy(g[k])[None].to(dev) for k in ('f0', 'f1', 'f2')]
        h1, w1 = cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2
        anchors = pre.createAnchors(h1, w1, cfg.velorange, cfg.carsize)
        inputs = lambda: (torch.from_numpy(g['voxels'].copy())[None].to(dev), feats, torch.from_numpy(g['idx']).to(dev), [None],
                          torch.from_numpy(g['imsize_hw']).to(dev), anchors)
        kw = dict(score_thr=0.0, iou_thr=0.5, pre_max=256, post_max=64)
        det = model.detect(*inputs(), **kw)
        det0 = model.detect(*inputs(), iou=False, **kw)
    finally:
        cfg.config['voxelshape'] = old
    s, s0 = det['scores'].cpu().numpy(), det0['scores'].cpu().numpy()
    assert len(s) > 0 and (np.diff(s) <= 0).all() and (s > 0).all() and (s < 1).all() and not np.array_equal(s, s0[:len(s)])
    # one frame set with test-time augmentation on the IoU model
    ds = Load.createDataset(names[:2], root=root)
    anchors = pre.createAnchors(cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2, cfg.velorange, cfg.carsize)
    bevs = bbox3d2bev(anchors.reshape(anchors.shape[:2] + (-1, 7))).to(dev).contiguous()
    batch, _ = pl.batch_from_dataset(ds, names[:2], dev, bevs, train_like.fpn_maps_for, cap_points=3000)
    keep = {}
    fused = detect_frame_set(model, batch, anchors.to(dev), cfg.imsize, tta=['identity', 'flip'], keep=keep, score_thr=0.0,
                             iou_thr=0.5, pre_max=256, post_max=32)
    assert len(fused) == 2 and keep['heads'].shape[1] == 20
    for d in fused:
        sc = d['scores'].cpu().numpy()
        assert d['boxes'].shape[0] == sc.shape[0] > 0 and np.isfinite(sc).all() and 'n_views' in d
