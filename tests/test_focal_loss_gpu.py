"""The focal loss of all frames in one call (csrc/loss_frames.hip, modules/voxelnet/FocalLoss.py) against the float64
restatement tests/focal_ref.py, on the inputs of tests/focal_cases.py.

Tolerances: losses to relative 1e-5 (the bar tests/test_targets_gpu.py holds VoxelLoss to); d_heads to rtol 1e-5 plus
atol = 1e-7 * max |reference gradient|, which only covers entries where f32 underflows.  A numpy f32 emulation of the
kernel's formulas on these very inputs has its losses within 8e-8 and its gradients within 0.17 of that bound (case 3 the
worst); every test prints the two figures of the kernels before it asserts."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import focal_cases as C
import focal_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'mvxnet-makise_amd')
DEFAULT = dict(alpha=0.25, gamma=2.0, cls_weight=1.0, reg_weight=2.0)


@functools.lru_cache(maxsize=None)
def _case(name):
    return getattr(C, name)()


@functools.lru_cache(maxsize=None)
def _reference(name, alpha=0.25, gamma=2.0):
    """Computed once per (case, parameters) and shared; callers do not modify it."""
    return R.focal_ref(_case(name), alpha=alpha, gamma=gamma, cls_weight=1.0, reg_weight=2.0)


def _run(case, want_grads=True, **kw):
    from modules import _hip
    dev = torch.device('cuda')
    p = dict(DEFAULT, **kw)
    t = {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(dev) for k in ('heads', 'pos', 'neg', 'gi', 'counts', 'gts', 'gt_off', 'anchors')}
    losses, d = _hip.focal_loss_frames(t['heads'], case['F'], case['l'], case['w'], case['A'], t['pos'], t['neg'], t['gi'], t['counts'],
                                       t['gts'], t['gt_off'], t['anchors'], p['alpha'], p['gamma'], p['cls_weight'], p['reg_weight'],
                                       want_grads=want_grads)
    torch.cuda.synchronize()
    return losses.cpu(), (d.cpu() if d is not None else None)


def _check(got, ref):
    (losses, d), (ref_losses, ref_d, _) = got, ref
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(d).all())
    scale = float(ref_d.abs().max())
    err_l = float(((losses.double() - ref_losses).abs() / ref_losses.abs().clamp_min(1e-300)).max())
    err_d = float(((d.double() - ref_d).abs() / (1e-5 * ref_d.abs() + 1e-7 * scale)).max())
    print('worst loss error %.2e (relative), worst gradient error %.2e of its tolerance' % (err_l, err_d))
    np.testing.assert_allclose(losses.double().numpy(), ref_losses.numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(d.double().numpy(), ref_d.numpy(), rtol=1e-5, atol=1e-7 * scale)


@pytest.mark.gpu
def test_case1_duplicates_ignored_anchors_and_empty_frames():
    case = _case('case1')
    ref = _reference('case1')
    losses, d = _run(case)
    _check((losses, d), ref)
    assert float(losses[1, 1]) == 0.0 and float(losses[2, 1]) == 0.0          # no positive: no regression loss
    positive, ignored = ref[2]
    A = case['A']
    d4 = d.reshape(case['F'], case['l'], case['w'], 8 * A)
    assert ignored.sum() == 3 + 4 and positive.sum() == 3
    assert float(d4[..., :A][torch.from_numpy(ignored)].abs().max()) == 0.0
    dreg = d4[..., A:].reshape(case['F'], case['l'], case['w'], A, 7)
    assert float(dreg[torch.from_numpy(~positive)].abs().max()) == 0.0
    assert float(dreg[torch.from_numpy(positive)].abs().min()) > 0.0
    # a frame without lists is all negative: its gradient is positive everywhere
    assert float(d4[1, ..., :A].min()) > 0.0


@pytest.mark.gpu
def test_case2_saturated_logits_stay_finite_and_accurate():
    _check(_run(_case('case2')), _reference('case2'))


@pytest.mark.gpu
def test_case3_several_workgroups_bitwise_repeatable_and_forward_only():
    case = _case('case3')
    first = _run(case)
    _check(first, _reference('case3'))
    second = _run(case)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    losses, none = _run(case, want_grads=False)
    assert none is None and torch.equal(losses, first[0])


@pytest.mark.gpu
def test_case4_three_anchors_per_location():
    _check(_run(_case('case4')), _reference('case4'))


@pytest.mark.gpu
def test_case5_sixteen_frames():
    _check(_run(_case('case5')), _reference('case5'))


@pytest.mark.gpu
@pytest.mark.parametrize('alpha,gamma', [(0.25, 2.0), (0.5, 0.0), (0.75, 1.5)])
def test_case6_parameters(alpha, gamma):
    _check(_run(_case('case1'), alpha=alpha, gamma=gamma), _reference('case1', alpha, gamma))


def _case_of_step(heads, F, l, w, targets, anchors):
    """The step's head output and targets in the layout of focal_ref, through numpy on the host (not through pack_targets)."""
    n_pos = [0 if t is None else int(t[0][0].shape[0]) for t in targets]
    n_neg = [0 if t is None else int(t[1][0].shape[0]) for t in targets]
    cap = max(1, max(n_pos + n_neg))
    pos, neg, gi, counts = C.empty_lists(F, cap)
    gts, off = [], [0]
    for f, t in enumerate(targets):
        if t is not None:
            for j in range(3):
                pos[f, j, :n_pos[f]] = t[0][j].cpu().numpy()
                neg[f, j, :n_neg[f]] = t[1][j].cpu().numpy()
            gi[f, :n_pos[f]] = t[2].cpu().numpy()
            gts.append(t[3].detach().cpu().float().numpy()[:, :7])
        counts[f] = (n_pos[f], n_neg[f])
        off.append(off[-1] + (0 if t is None else gts[-1].shape[0]))
    return dict(F=F, l=l, w=w, A=2, heads=heads.cpu().numpy(), pos=pos, neg=neg, gi=gi, counts=counts,
                gts=np.concatenate(gts) if gts else np.zeros((1, 7), np.float32), gt_off=np.array(off, np.int32),
                anchors=anchors.detach().cpu().float().numpy().reshape(l, w, 2, 7))


@pytest.mark.gpu
def test_whole_model_step_with_the_focal_criterion(tmp_path):
    """One pipeline.train_step_full with criterion=FocalLoss() on two synthetic frames of 3,000 points (the batch of
    test_whole_model_step_hip_rpn_agrees_with_the_module_rpn): the losses against the reference on the step's own head output,
    finite parameter gradients, and the head biases' gradients = the column sums of the reference d_heads (1e-4 of the largest)."""
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
    model = MVXNet().to(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    bucket = parallel.GradBucket(params)
    crit = FocalLoss()
    np.random.seed(0)
    batch, targets = pl.batch_from_dataset(ds, ['000000', '000001'], dev, bevs, train_like.fpn_maps_for, cap_points=3000)
    assert any(t is not None and len(t[0][0]) > 0 for t in targets)
    with pytest.raises(MvxHipError):
        pl.train_step_full(model, batch, targets, crit, anchors, cfg.imsize, rpn_hip=False)
    bucket.zero()
    rpn = model.backbone.rpn
    assert float(rpn.cls.bias.grad.abs().max()) == 0.0 and float(rpn.reg.bias.grad.abs().max()) == 0.0
    k = {}
    out = pl.train_step_full(model, batch, targets, crit, anchors, cfg.imsize, keep=k)
    torch.cuda.synchronize()
    F, h1, w1 = k['geom'][0], k['geom'][5], k['geom'][6]
    assert F == 2 and k['heads'].shape == (F * h1 * w1, 16)
    tl = [targets[f] for f in out['live']]
    ref_losses, ref_d, _ = R.focal_ref(_case_of_step(k['heads'], F, h1, w1, tl, anchors),
                                       crit.alpha, crit.gamma, crit.cls_weight, crit.reg_weight)
    np.testing.assert_allclose(out['cls'], ref_losses[:, 0].numpy(), rtol=1e-5)
    has = [t is not None and len(t[0][0]) > 0 for t in tl]
    np.testing.assert_allclose(out['reg'], ref_losses[:, 1].numpy()[has], rtol=1e-5)
    np.testing.assert_allclose(out['loss'], ref_losses.sum(dim=1).numpy(), rtol=1e-5)
    for name, p in model.named_parameters():
        if p.requires_grad:
            assert bool(torch.isfinite(p.grad).all()), name
    cols = ref_d.sum(dim=0)
    for got, want in ((rpn.cls.bias.grad, cols[:2]), (rpn.reg.bias.grad, cols[2:])):
        err = float((got.cpu().double() - want).abs().max() / want.abs().max())
        print('bias gradient vs column sums of the reference d_heads: %.2e' % err)
        assert err < 1e-4


@pytest.mark.gpu
def test_train_like_runs_with_the_focal_loss(tmp_path):
    sys.path.insert(0, PKG)
    import train_like
    ck = str(tmp_path / 'ck')
    args = train_like.parse_args([str(tmp_path / 'kitti'), '--loss', 'focal', '--mode', 'fast', '--frames', '2', '--steps', '2',
                                  '--synthetic', '3', '--points', '3000', '--checkpoints', ck, '--quiet'])
    np.random.seed(0)
    r = train_like.train(args)
    assert r['steps'] == 2 and len(r['losses']) == 3 and all(np.isfinite(v) for v in r['losses'])
    assert os.path.exists(os.path.join(ck, 'epoch1.pkl')) and os.path.exists(os.path.join(ck, 'epoch1_opt.pkl'))
