"""The direction classifier and the sine angle loss on the GPU (csrc/loss_frames.hip mvx_focal_loss_dir_frames,
csrc/detect.hip mvx_detect_frames_dir, the 20-wide heads of modules/rpn_frames.py) against the float64 restatement
tests/direction_ref.py, on the inputs of tests/direction_cases.py.

Tolerances.  Losses: relative 1e-5.  Gradients: rtol 1e-5 plus atol = 1e-7 * max |reference gradient| -- the focal loss's own
(tests/test_focal_loss_gpu.py).  The angle column alone gets a further atol = reg_scale * 2^-20 * max(1, M), M the largest
magnitude among r6, g6 and an6: three f32 roundings of operands up to M move D = r6 - (g6 - an6) by at most 3 * 2^-24 * M, the
derivative of the term with respect to D is at most 1 in magnitude, and 2^-20 is that bound with a factor 5 of margin.  Every
test prints the worst figures before it asserts."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

import direction_cases as DC
import direction_ref as DR

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'mvxnet-makise_amd')
P = dict(alpha=0.25, gamma=2.0, cls_weight=1.0, reg_weight=2.0, dir_weight=0.2, dir_offset=math.pi / 4)
LISTS = ('pos', 'neg', 'gi', 'counts', 'gts', 'gt_off', 'anchors')


@functools.lru_cache(maxsize=None)
def _case(name, saturated=False):
    return DC.with_direction(name, saturated=saturated)


@functools.lru_cache(maxsize=None)
def _reference(name, saturated=False, dir_offset=math.pi / 4):
    """Computed once per (case, offset) and shared; callers do not modify it."""
    return DR.direction_ref(_case(name, saturated), **dict(P, dir_offset=dir_offset))


def _dev(case):
    return {k: torch.from_numpy(np.ascontiguousarray(case[k])).cuda() for k in LISTS}


def _run(case, layout='inside', want_grads=True, **kw):
    """'inside': the direction logits are columns 8A..9A of the wide rows; 'separate': a (rows, 4) tensor of their own beside
    plain 8A-wide rows.  Returns (losses (F,3), d_heads as the kernel wrote it, d_dir (rows, A)) on the host."""
    from modules import _hip
    p = dict(P, **kw)
    t = _dev(case)
    A = case['A']
    if layout == 'inside':
        heads = torch.from_numpy(DC.wide_rows(case)).cuda()
        logits = heads[:, 8 * A:9 * A]
    else:
        heads = torch.from_numpy(np.ascontiguousarray(case['heads'])).cuda()
        own = torch.full((heads.shape[0], 4), 7.0, dtype=torch.float32, device='cuda')
        own[:, :A] = torch.from_numpy(case['dir']).cuda()
        logits = own[:, :A]
    losses, d, dd = _hip.focal_loss_dir_frames(heads, logits, case['F'], case['l'], case['w'], A, t['pos'], t['neg'], t['gi'],
                                               t['counts'], t['gts'], t['gt_off'], t['anchors'], p['alpha'], p['gamma'],
                                               p['cls_weight'], p['reg_weight'], p['dir_weight'], p['dir_offset'],
                                               want_grads=want_grads)
    torch.cuda.synchronize()
    if not want_grads:
        assert d is None and dd is None
        return losses.cpu(), None, None
    return losses.cpu(), d.cpu(), dd.cpu().contiguous()


def _angle_atol(case):
    """(rows, 8A) extra absolute tolerance: reg_scale * 2^-20 * max(1, M) on the angle columns of listed anchors, 0 elsewhere."""
    F, l, w, A = case['F'], case['l'], case['w'], case['A']
    atol = np.zeros((F, l, w, 8 * A))
    heads = case['heads'].reshape(F, l, w, 8 * A)
    for f in range(F):
        px, py, pz, rows, n_pos = DR._entries(case, f)
        if n_pos == 0:
            continue
        reg_scale = P['reg_weight'] / (n_pos * 7)
        for x, y, z, g in zip(px, py, pz, rows):
            col = A + 7 * z + 6
            M = max(abs(float(heads[f, x, y, col])), abs(float(case['gts'][g, 6])), abs(float(case['anchors'][x, y, z, 6])), 1.0)
            atol[f, x, y, col] += reg_scale * 2.0 ** -20 * M           # once per entry: duplicates add up like their terms
    return atol.reshape(F * l * w, 8 * A)


def _check(case, got, ref):
    (losses, d, dd), (ref_losses, ref_d, ref_dd, _) = got, ref
    A = case['A']
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(d).all()) and bool(torch.isfinite(dd).all())
    scale = float(max(ref_d.abs().max(), ref_dd.abs().max()))
    atol = 1e-7 * scale + _angle_atol(case)
    d8 = d[:, :8 * A].double().numpy()
    err_l = float(((losses.double() - ref_losses).abs() / ref_losses.abs().clamp_min(1e-300))[ref_losses != 0].max())
    err_d = float((np.abs(d8 - ref_d.numpy()) / (1e-5 * np.abs(ref_d.numpy()) + atol)).max())
    err_dd = float(((dd.double() - ref_dd).abs() / (1e-5 * ref_dd.abs() + 1e-7 * scale)).max())
    print('worst loss error %.2e (relative), worst gradient error %.2e / direction gradient %.2e of their tolerances'
          % (err_l, err_d, err_dd))
    np.testing.assert_allclose(losses.double().numpy(), ref_losses.numpy(), rtol=1e-5, atol=0)
    assert (np.abs(d8 - ref_d.numpy()) <= 1e-5 * np.abs(ref_d.numpy()) + atol).all()
    np.testing.assert_allclose(dd.double().numpy(), ref_dd.numpy(), rtol=1e-5, atol=1e-7 * scale)


def _check_layout(case, d, dd, layout):
    """Wide rows: the direction gradient sits in columns 8A..9A, the pad columns are exactly 0."""
    A = case['A']
    if layout == 'inside':
        assert d.shape[1] == (9 * A + 3) // 4 * 4
        assert torch.equal(d[:, 8 * A:9 * A], dd)
        if d.shape[1] > 9 * A:
            assert float(d[:, 9 * A:].abs().max()) == 0.0
    else:
        assert d.shape[1] == 8 * A


def _cls_is_the_plain_kernels(case, losses, d):
    """The cls loss and the cls gradient columns: bitwise those of mvx_focal_loss_frames on the same inputs."""
    from modules import _hip
    t = _dev(case)
    heads = torch.from_numpy(np.ascontiguousarray(case['heads'])).cuda()
    pl, pd = _hip.focal_loss_frames(heads, case['F'], case['l'], case['w'], case['A'], t['pos'], t['neg'], t['gi'], t['counts'],
                                    t['gts'], t['gt_off'], t['anchors'], P['alpha'], P['gamma'], P['cls_weight'], P['reg_weight'])
    torch.cuda.synchronize()
    assert torch.equal(pl[:, 0].cpu(), losses[:, 0])
    assert torch.equal(pd[:, :case['A']].cpu(), d[:, :case['A']])


@pytest.mark.parametrize('layout', ['inside', 'separate'])
def test_case1_duplicates_empty_frames_and_both_layouts(layout):
    case, ref = _case('case1'), _reference('case1')
    losses, d, dd = _run(case, layout)
    _check(case, (losses, d, dd), ref)
    _check_layout(case, d, dd, layout)
    _cls_is_the_plain_kernels(case, losses, d)
    assert float(losses[1, 1]) == 0.0 and float(losses[1, 2]) == 0.0 and float(losses[2, 2]) == 0.0
    positive = ref[3][0]
    d4 = dd.reshape(case['F'], case['l'], case['w'], case['A'])
    assert float(d4[torch.from_numpy(~positive)].abs().max()) == 0.0          # only listed anchors get a direction gradient
    assert float(d4[torch.from_numpy(positive)].abs().min()) > 0.0
    DC.check_case(case)                                                        # beyond the counts: GARBAGE, never read


@pytest.mark.parametrize('layout', ['inside', 'separate'])
def test_saturated_direction_logits_stay_finite_and_accurate(layout):
    case = _case('case1', True)
    assert float(np.abs(case['dir']).max()) == 90.0
    got = _run(case, layout)
    _check(case, got, _reference('case1', True))
    _check_layout(case, got[1], got[2], layout)


def test_other_offset():
    case = _case('case1')
    _check(case, _run(case, dir_offset=0.0), _reference('case1', False, 0.0))


@pytest.mark.parametrize('layout', ['inside', 'separate'])
def test_case3_several_workgroups_bitwise_repeatable_and_forward_only(layout):
    case = _case('case3')
    first = _run(case, layout)
    _check(case, first, _reference('case3'))
    _check_layout(case, first[1], first[2], layout)
    _cls_is_the_plain_kernels(case, first[0], first[1])
    second = _run(case, layout)
    assert torch.equal(first[0], second[0])
    assert torch.equal(first[1], second[1]) and torch.equal(first[2], second[2])          # no anchor is listed twice here
    losses, none, _ = _run(case, layout, want_grads=False)
    assert none is None and torch.equal(losses, first[0])


def test_case1_losses_repeat_bitwise_with_duplicates():
    case = _case('case1')
    assert torch.equal(_run(case)[0], _run(case)[0])
    assert torch.equal(_run(case, want_grads=False)[0], _run(case)[0])


@pytest.mark.parametrize('layout', ['inside', 'separate'])
def test_case4_three_anchors_rows_of_28(layout):
    case = _case('case4')
    got = _run(case, layout)
    _check(case, got, _reference('case4'))
    _check_layout(case, got[1], got[2], layout)
    if layout == 'inside':
        assert got[1].shape[1] == 28                                           # 24 + 3 direction logits + one pad column


def test_case5_sixteen_frames():
    case = _case('case5')
    got = _run(case)
    _check(case, got, _reference('case5'))
    _check_layout(case, got[1], got[2], 'inside')


# ---- decode ---------------------------------------------------------------------------------------------------------------
def _yaw_close(a, b, tol):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return np.abs(np.sin(d)).max() <= tol and (np.cos(d) > 0).all()


@pytest.mark.parametrize('dir_offset', DC.OFFSETS)
def test_decode_folds_the_yaw_with_the_direction_bit(dir_offset):
    from modules import _hip
    from modules.detect import postprocess
    case = DC.decode_case(dir_offset)
    F, l, w, A = case['F'], case['l'], case['w'], case['A']
    anchors = torch.from_numpy(case['anchors'].reshape(l, w, A * 7))
    anc = case['anchors'].reshape(-1, 7)
    kw = dict(score_thr=0.05, iou_thr=case['iou_thr'], pre_max=32, post_max=16)
    wide = torch.from_numpy(DC.decode_heads(case)).cuda()
    plain = torch.from_numpy(DC.decode_heads(case, with_dir=False)).cuda()
    dets = postprocess(wide, anchors, F, l, w, dir_offset=dir_offset, **kw)          # direction=None: the 20-wide rows carry it
    dets_plain = postprocess(plain, anchors, F, l, w, **kw)
    dets_off = postprocess(wide, anchors, F, l, w, direction=False, **kw)
    n_supp = 0
    for f in range(F):
        frame = case['planted'][f]
        by_anchor = {p['n']: p for p in frame}
        got, idx = dets[f]['boxes'].cpu().numpy().astype(np.float64), dets[f]['anchor_idx'].cpu().numpy()
        assert dets[f]['status'] == 0 and dets[f]['n_candidates'] == len(frame)
        assert 0 < len(idx) <= len(frame)
        n_supp += len(frame) - len(idx)
        reg = case['reg'][f].reshape(-1, 7)[idx]
        want = DR.decode_dir(reg, anc[idx], case['dir'][f].reshape(-1)[idx], dir_offset)
        np.testing.assert_allclose(got[:, :6], want[:, :6], rtol=1e-5, atol=1e-6)
        assert _yaw_close(got[:, 6], want[:, 6], 1e-5)
        assert (got[:, 6] >= -math.pi).all() and (got[:, 6] < math.pi).all()
        gts = np.array([by_anchor[int(n)]['gt'] for n in idx], np.float64)
        err = np.abs(DR.wrap_pi(got[:, 6] - gts[:, 6]))
        print('frame %d: worst |yaw - g6| mod 2 pi = %.2e over %d boxes (%d planted)' % (f, err.max(), len(idx), len(frame)))
        assert err.max() <= 1e-4                                               # also for the boxes regressed half a turn off
        np.testing.assert_allclose(got[:, :6], gts[:, :6], rtol=1e-5, atol=1e-5)
        # a half turn changes no rectangle: the same anchors survive without the direction head
        assert np.array_equal(idx, dets_plain[f]['anchor_idx'].cpu().numpy())
        assert torch.equal(dets_off[f]['boxes'], dets_plain[f]['boxes'])
        # ... whose yaws are the raw regression: off by half a turn where it was planted so
        raw = dets_plain[f]['boxes'].cpu().numpy()[:, 6].astype(np.float64)
        off = np.array([by_anchor[int(n)]['shift'] != 0.0 for n in idx])
        turn = np.abs(DR.wrap_pi(raw - gts[:, 6]))
        assert (turn[~off] < 1e-4).all() and (np.abs(turn[off] - math.pi) < 1e-4).all() and off.any()
    assert n_supp > 0                                                          # the NMS did suppress something
    # a null direction head is mvx_detect_frames, bit for bit
    v = plain.view(F, l, w, 16)
    a_dev = torch.from_numpy(case['anchors']).cuda()
    old = _hip.detect_frames(v[..., :A], v[..., A:], a_dev, F, l, w, A, 0.05, case['iou_thr'], 32, 16)
    vw = wide.view(F, l, w, 20)
    new = _hip.detect_frames(vw[..., :A], vw[..., A:8 * A], a_dev, F, l, w, A, 0.05, case['iou_thr'], 32, 16, dir_logits=None)
    for o, n in zip(old, new):
        assert torch.equal(o, n)
    # a NaN regressed yaw is reported, not folded away
    bad = wide.clone()
    n0 = case['planted'][0][0]['n']
    bad[n0 // A, A + 7 * (n0 % A) + 6] = float('nan')
    db = postprocess(bad, anchors, F, l, w, dir_offset=dir_offset, **kw)
    assert db[0]['status'] & 2 and n0 not in db[0]['anchor_idx'].tolist() and db[1]['status'] == 0


def test_postprocess_direction_true_needs_the_columns():
    from modules.detect import postprocess
    from modules.Extension import MvxHipError
    case = DC.decode_case()
    anchors = torch.from_numpy(case['anchors'].reshape(case['l'], case['w'], 14))
    plain = torch.from_numpy(DC.decode_heads(case, with_dir=False)).cuda()
    with pytest.raises(MvxHipError):
        postprocess(plain, anchors, case['F'], case['l'], case['w'], direction=True)


# ---- the per-frame autograd paths ----------------------------------------------------------------------------------------
def test_forward_of_a_direction_model_returns_score_and_reg_and_leaves_dir_without_gradient(golden):
    """MVXNet.forward on the single node reads the head width from the tensor: (score, reg) of the reference's shapes from the
    20-wide rows, equal to the first 16 columns; its backward gives the direction head a zero gradient and the others theirs."""
    import modules.config as cfg
    from MVXNet import MVXNet
    from modules import whole
    g = golden('mvxnet_small')
    old = list(cfg.config['voxelshape'])
    cfg.config['voxelshape'] = [int(v) for v in g['voxelshape']]
    try:
        dev = torch.device('cuda')
        torch.manual_seed(4)
        model = MVXNet(direction=True).to(dev)
        feats = [torch.from_numpy(g[k])[None].to(dev) for k in ('f0', 'f1', 'f2')]
        idx = torch.from_numpy(g['idx']).to(dev)
        imsize = torch.from_numpy(g['imsize_hw']).to(dev)
        h1, w1 = cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2

        def vox():
            return torch.from_numpy(g['voxels'].copy())[None].to(dev)
        with torch.no_grad():
            heads = whole.forward_heads(model, vox(), feats, idx, imsize)
        assert heads.shape == (h1 * w1, 20) and float(heads[:, 18:].abs().max()) == 0.0
        assert float(heads[:, 16:18].abs().max()) > 0.0
        score, reg = model(vox(), feats, idx, [None], imsize)
        assert score.shape == (1, 2, h1, w1) and reg.shape == (1, 14, h1, w1)
        v = heads.view(1, h1, w1, 20)
        assert torch.equal(score.detach(), torch.sigmoid(v[..., :2]).permute(0, 3, 1, 2))
        assert torch.equal(reg.detach(), v[..., 2:16].permute(0, 3, 1, 2))
        (score.sum() + reg.square().sum()).backward()
        torch.cuda.synchronize()
        rpn = model.backbone.rpn
        for p in (rpn.dir.weight, rpn.dir.bias):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0
        assert float(rpn.cls.weight.grad.abs().max()) > 0.0 and float(rpn.reg.bias.grad.abs().max()) > 0.0
        assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
    finally:
        cfg.config['voxelshape'] = old


# ---- whole step and loop --------------------------------------------------------------------------------------------------
def _case_of_step(heads, F, l, w, targets, anchors):
    from test_focal_loss_gpu import _case_of_step as plain
    h = heads.cpu().numpy()
    case = plain(torch.from_numpy(np.ascontiguousarray(h[:, :16])), F, l, w, targets, anchors)
    case['dir'] = np.ascontiguousarray(h[:, 16:18])
    return case


def test_whole_model_step_with_the_direction_criterion(tmp_path):
    """pipeline.train_step_full on the batch of test_whole_model_step_with_the_focal_criterion with MVXNet(direction=True) and
    FocalLoss(direction=True): losses against the reference on the step's own head output, finite gradients, the direction
    head's bias gradient = the column sums of the reference direction gradient, and the mismatched pairings refused."""
    sys.path.insert(0, PKG)
    import modules.config as cfg
    from modules import parallel, pipeline as pl
    from modules.Calc import bbox3d2bev
    from modules.data import Load, Preprocessing as pre, Synthetic as S
    from modules.voxelnet.FocalLoss import FocalLoss
    from modules.voxelnet.Loss import VoxelLoss
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
    model = MVXNet(direction=True).to(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    bucket = parallel.GradBucket(params)
    crit = FocalLoss(direction=True)
    np.random.seed(0)
    batch, targets = pl.batch_from_dataset(ds, ['000000', '000001'], dev, bevs, train_like.fpn_maps_for, cap_points=3000)
    assert any(t is not None and len(t[0][0]) > 0 for t in targets)
    bucket.zero()
    rpn = model.backbone.rpn
    for bad in (FocalLoss(), VoxelLoss()):                                     # a direction model needs the direction criterion
        with pytest.raises(MvxHipError):
            pl.train_step_full(model, batch, targets, bad, anchors, cfg.imsize)
    assert float(rpn.dir.bias.grad.abs().max()) == 0.0 and float(rpn.dir.weight.grad.abs().max()) == 0.0
    k = {}
    out = pl.train_step_full(model, batch, targets, crit, anchors, cfg.imsize, keep=k)
    torch.cuda.synchronize()
    F, h1, w1 = k['geom'][0], k['geom'][5], k['geom'][6]
    assert F == 2 and k['heads'].shape == (F * h1 * w1, 20)
    assert float(k['heads'][:, 18:].abs().max()) == 0.0                        # the two zero rows of w_heads
    tl = [targets[f] for f in out['live']]
    ref_losses, ref_d, ref_dd, _ = DR.direction_ref(_case_of_step(k['heads'], F, h1, w1, tl, anchors), crit.alpha, crit.gamma,
                                                    crit.cls_weight, crit.reg_weight, True, crit.dir_weight, crit.dir_offset)
    has = [t is not None and len(t[0][0]) > 0 for t in tl]
    print('step losses (cls, reg, dir): %s / %s / %s' % (out['cls'], out['reg'], out['dir']))
    np.testing.assert_allclose(out['cls'], ref_losses[:, 0].numpy(), rtol=1e-5)
    np.testing.assert_allclose(out['reg'], ref_losses[:, 1].numpy()[has], rtol=1e-5)
    np.testing.assert_allclose(out['dir'], ref_losses[:, 2].numpy()[has], rtol=1e-5)
    np.testing.assert_allclose(out['loss'], [float(r[0] + r[1] + r[2]) if h else float(r[0]) for r, h in zip(ref_losses, has)],
                               rtol=1e-5)
    for name, p in model.named_parameters():
        if p.requires_grad:
            assert bool(torch.isfinite(p.grad).all()), name
    cols, dcols = ref_d.sum(dim=0), ref_dd.sum(dim=0)
    for got, want in ((rpn.cls.bias.grad, cols[:2]), (rpn.reg.bias.grad, cols[2:]), (rpn.dir.bias.grad, dcols)):
        err = float((got.cpu().double() - want).abs().max() / want.abs().max())
        print('bias gradient vs column sums of the reference gradient: %.2e' % err)
        assert err < 1e-4
    assert float(rpn.dir.weight.grad.abs().max()) > 0.0
    # the other mismatch, and the plain pairing's heads stay 16 wide
    torch.manual_seed(0)
    plain = MVXNet().to(dev)
    pbucket = parallel.GradBucket([p for p in plain.parameters() if p.requires_grad])
    pbucket.zero()
    with pytest.raises(MvxHipError):
        pl.train_step_full(plain, batch, targets, crit, anchors, cfg.imsize)
    assert float(pbucket.flat.abs().max()) == 0.0                              # refused before anything was launched
    k2 = {}
    out2 = pl.train_step_full(plain, batch, targets, FocalLoss(), anchors, cfg.imsize, keep=k2)
    assert k2['heads'].shape[1] == 16 and 'dir' not in out2 and len(out2['loss']) == 2


def test_train_like_and_detect_like_with_direction(tmp_path, golden):
    sys.path.insert(0, PKG)
    import detect_like
    import modules.config as cfg
    import train_like
    from modules.data import Preprocessing as pre
    from MVXNet import MVXNet
    root, ck = str(tmp_path / 'kitti'), str(tmp_path / 'ck')
    args = train_like.parse_args([root, '--direction', '--loss', 'focal', '--mode', 'fast', '--frames', '2', '--steps', '2',
                                  '--synthetic', '3', '--points', '3000', '--checkpoints', ck, '--quiet'])
    np.random.seed(0)
    r = train_like.train(args)
    assert r['steps'] == 2 and len(r['losses']) == 3 and all(np.isfinite(v) for v in r['losses'])
    state = torch.load(os.path.join(ck, 'epoch1.pkl'), map_location='cpu')
    assert 'backbone.rpn.dir.weight' in state and 'backbone.rpn.dir.bias' in state
    for argv in (['--loss', 'voxel', '--mode', 'fast'], ['--loss', 'focal', '--mode', 'module']):
        with pytest.raises(SystemExit) as e:
            train_like.parse_args([root, '--direction'] + argv)
        assert e.value.code == 2
    out = str(tmp_path / 'res')
    detect_like.main(detect_like.parse_args([root, '--checkpoint', os.path.join(ck, 'epoch1.pkl'), '--out', out, '--frames', '2',
                                             '--points', '3000']))
    names = open(os.path.join(root, 'ImageSets', 'train.txt')).read().split()
    assert len(names) == 3 and all(os.path.exists(os.path.join(out, n + '.txt')) for n in names)
    # MVXNet.detect of the loaded model on the small golden frame: yaws in [-pi, pi)
    g = golden('mvxnet_small')
    old = list(cfg.config['voxelshape'])
    cfg.config['voxelshape'] = [int(v) for v in g['voxelshape']]
    try:
        dev = torch.device('cuda')
        model = MVXNet(direction=True).to(dev)
        model.load_state_dict(state)
        feats = [torch.from_numpy(g[k])[None].to(dev) for k in ('f0', 'f1', 'f2')]
        h1, w1 = cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2
        anchors = pre.createAnchors(h1, w1, cfg.velorange, cfg.carsize)
        det = model.detect(torch.from_numpy(g['voxels'].copy())[None].to(dev), feats, torch.from_numpy(g['idx']).to(dev), [None],
                           torch.from_numpy(g['imsize_hw']).to(dev), anchors, score_thr=0.0, iou_thr=0.5, pre_max=256, post_max=64)
    finally:
        cfg.config['voxelshape'] = old
    yaw = det['boxes'][:, 6].cpu().double().numpy()
    assert yaw.shape[0] > 0 and (yaw >= -math.pi).all() and (yaw < math.pi).all()
