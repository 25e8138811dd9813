"""The rotated 3D IoU regression loss on the GPU (csrc/box_iou_loss.hip mvx_box_iou_loss_frames, FocalLoss(iou_loss=True);
DESIGN.md 3.36) against the float64 restatements of tests/box_iou_ref.py, on the inputs of tests/box_iou_cases.py.

Tolerances.  q: per case, four times the worst distance between the kernel's algorithm restated in f32 numpy and the exact
float64 clip over the case's own pairs (the IoU-head tests' convention: the device differs from numpy in cosf / sinf / expf by a
few ulp on the same operands); that bar must itself stay below 1e-4, and the far-range pairs (x = 69, y = -39) meet their bar
like the near ones.  Gradient: rtol 1e-5 plus four times the f32 restatement's worst gradient distance of the case, a bar that
must stay below 1e-3 of the largest reference gradient.  The term and the mean q: relative 1e-5.  What the call must not touch
is compared bitwise.  Every test prints its worst figure before it asserts.

Measured on an MI355X: DESIGN.md 3.36."""
import os
import sys

import numpy as np
import pytest
import torch

import box_iou_cases as BC
import box_iou_ref as BR
import iou_head_cases as IC

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'mvxnet-makise_amd')
LISTS = ('pos', 'gi', 'counts', 'gts', 'gt_off', 'anchors')
FOCAL = (0.25, 2.0, 1.0, 2.0)                   # alpha, gamma, cls_weight, reg_weight


def _dev(case):
    t = {k: torch.from_numpy(np.ascontiguousarray(case[k])).cuda() for k in LISTS}
    t['heads'] = torch.from_numpy(np.ascontiguousarray(case['heads'])).cuda()
    return t


def _call(case, t, weight=BC.WEIGHT, **kw):
    from modules import _hip
    out = _hip.box_iou_loss_frames(t['heads'], case['F'], case['l'], case['w'], case['A'], t['pos'], t['gi'], t['counts'], t['gts'],
                                   t['gt_off'], t['anchors'], weight, **kw)
    torch.cuda.synchronize()
    return out


def _focal_prefill(case, t):
    """(losses, d_heads) of the focal call that runs in front of the new one: the plain entry on 16-wide rows, the direction
    entry (logits in columns 16..17) on 20-wide ones."""
    from modules import _hip
    F, l, w, A = case['F'], case['l'], case['w'], case['A']
    neg = torch.zeros_like(t['pos'])
    if case['heads'].shape[1] == 8 * A:
        losses, d = _hip.focal_loss_frames(t['heads'], F, l, w, A, t['pos'], neg, t['gi'], t['counts'], t['gts'], t['gt_off'],
                                           t['anchors'], *FOCAL)
    else:
        losses, d, _ = _hip.focal_loss_dir_frames(t['heads'], t['heads'][:, 8 * A:9 * A], F, l, w, A, t['pos'], neg, t['gi'], t['counts'],
                                                  t['gts'], t['gt_off'], t['anchors'], *FOCAL, 0.2, 0.785)
    torch.cuda.synchronize()
    return losses, d


def _listed(case, width):
    """bool (rows, width): the regression columns of the anchors the taken entries name."""
    m = np.zeros((case['heads'].shape[0], width), bool)
    for f in range(case['F']):
        for _, x, y, z, _ in BR.entries(case, f):
            m[(f * case['l'] + x) * case['w'] + y, case['A'] + 7 * z:case['A'] + 7 * z + 7] = True
    return torch.from_numpy(m)


# ---- 1. q, 2. the gradient, the term and the mean -----------------------------------------------------------------------------------
@pytest.mark.parametrize('where,ld', BC.PAIR_CASES)
def test_q_term_and_gradient_against_float64(where, ld):
    case, ref = BC.pair_case(where, ld), BC.reference(where, ld)
    out, d, q = _call(case, _dev(case), want_q=True)
    out, d, q = out.cpu().double().numpy(), d.cpu().double().numpy(), q.cpu().double().numpy()
    assert d.shape == case['heads'].shape and np.isfinite(d).all() and np.isfinite(out).all()
    skipped = ref['q'] < 0
    assert (q[skipped] == -1.0).all() and (q[~skipped] > 0.0).all() and (q[~skipped] <= 1.0).all()
    err_q = float(np.abs(q[~skipped] - ref['q'][~skipped]).max())
    print('%s, rows of %d: q worst |device - float64| = %.3e over %d pairs, bar %.3e (4 x the f32 restatement\'s %.3e)'
          % (where, ld, err_q, (~skipped).sum(), ref['q_bar'], ref['worst_q']))
    tol = 1e-5 * np.abs(ref['grad']) + ref['grad_bar']
    err_g = np.abs(d - ref['grad'])
    print('gradient worst |device - float64| = %.3e (largest gradient %.3f), bar %.3e = 4 x the f32 restatement\'s %.3e; worst '
          'share of its tolerance %.2f' % (err_g.max(), ref['grad_max'], ref['grad_bar'], ref['worst_grad'], (err_g / tol).max()))
    err_o = float(np.abs(out[1:] / ref['out'][1:] - 1).max())
    print('term and mean q: worst relative error %.2e' % err_o)
    assert ref['q_bar'] <= BC.Q_BAR_MAX and ref['grad_bar'] <= BC.GRAD_BAR_MAX * ref['grad_max']
    assert err_q <= ref['q_bar']
    assert (err_g <= tol).all()
    assert (out[0] == 0.0).all()                                               # the frame without a positive: term 0, mean 0
    np.testing.assert_allclose(out[1:], ref['out'][1:], rtol=1e-5, atol=0)
    assert float(np.abs(d[~_listed(case, ld).numpy()]).max()) == 0.0


# ---- 3. additive and confined -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('where,ld', [('near', 16), ('far', 20)])
def test_gradient_is_added_to_the_listed_regression_columns_and_nothing_else_is_touched(where, ld):
    case, ref = BC.pair_case(where, ld), BC.reference(where, ld)
    t = _dev(case)
    losses, filled = _focal_prefill(case, t)
    assert filled.shape[1] == ld and float(filled[:, :case['A']].abs().max()) > 0.0
    listed = _listed(case, ld)
    before, l_before = filled.cpu(), losses.cpu()
    out, d, _ = _call(case, t, d_heads=filled, loss_add=losses[:, 1:2])
    assert d is filled
    after, l_after = filled.cpu(), losses.cpu()
    assert torch.equal(after[~listed].view(torch.int32), before[~listed].view(torch.int32))      # cls, dir, pad, other anchors
    added = (after - before).double().numpy()
    # one rounding of the f32 sum, one of the difference taken here
    tol = 1e-5 * np.abs(ref['grad']) + ref['grad_bar'] + 2.0 ** -22 * (np.abs(before.double().numpy()) + np.abs(ref['grad']))
    print('added gradient vs float64: worst share of its tolerance %.2f' % (np.abs(added - ref['grad']) / tol).max())
    assert (np.abs(added - ref['grad']) <= tol).all() and float(np.abs(added[listed.numpy()]).max()) > 0.1
    assert torch.equal(l_after[:, 1], l_before[:, 1] + out.cpu()[:, 0])        # the term went into column 1, one f32 addition
    keep = [c for c in range(losses.shape[1]) if c != 1]
    assert torch.equal(l_after[:, keep], l_before[:, keep])
    # a d_heads of another stride, junk beyond the rows' own columns
    buf = torch.full((filled.shape[0], 24), 3.25, dtype=torch.float32, device='cuda')
    buf[:, :ld] = before.cuda()
    _call(case, t, d_heads=buf)
    assert torch.equal(buf[:, :ld].cpu().view(torch.int32), after.view(torch.int32)) and bool((buf[:, ld:] == 3.25).all())
    # weight 0: nothing is touched at all; want_grads=False: no gradient is touched
    again, l_again = before.cuda(), l_before.cuda()
    out0, _, _ = _call(case, t, weight=0.0, d_heads=again, loss_add=l_again[:, 1:2])
    assert torch.equal(again.cpu().view(torch.int32), before.view(torch.int32)) and torch.equal(l_again.cpu(), l_before)
    assert float(out0[:, 0].abs().max()) == 0.0 and torch.equal(out0[:, 1].cpu(), out.cpu()[:, 1])
    outf, none, qf = _call(case, t, want_grads=False, want_q=True, d_heads=again)
    assert none is again and torch.equal(again.cpu().view(torch.int32), before.view(torch.int32)) and torch.equal(outf, out)
    # no anchor is listed twice: two runs are bitwise equal
    a, b = _call(case, t, want_q=True), _call(case, t, want_q=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(a[2], qf)


# ---- 4. edges -----------------------------------------------------------------------------------------------------------------------
def test_edges():
    case = BC.edge_case()
    s = case['slots']
    t = _dev(case)
    near = BC.reference('near')                    # the bars of the near case: these boxes lie at the same range
    bar = near['q_bar']
    q64, out64 = BR.q_ref(case, 1.0)
    _, grad64, _ = BR.loss_autograd(case, 1.0)
    d0 = torch.full(case['heads'].shape, 0.5, dtype=torch.float32, device='cuda')
    out, d, q = _call(case, t, weight=1.0, want_q=True, d_heads=d0)
    q, d, out = q.cpu().double().numpy()[0], d.cpu().double().numpy() - 0.5, out.cpu().double().numpy()
    A, W = case['A'], case['w']

    def cols(name):
        x, y, z = (int(v) for v in case['pos'][0, :, s[name]])
        return d[x * W + y, A + 7 * z:A + 7 * z + 7]
    print('edge q:', {n: float(q[k]) for n, k in s.items()}, 'out', out.tolist())
    assert q[s['exact']] >= 1.0 - bar and np.isfinite(cols('exact')).all()
    assert abs(q[s['half_turn']] - q[s['exact']]) <= bar and np.isfinite(cols('half_turn')).all()
    for name in ('touching', 'apart', 'no_vertical', 'overflow'):             # q = 0 exactly, nothing added, the term counts 1
        assert q[s[name]] == 0.0 and (cols(name) == 0.0).all(), name
    for name in ('outside_grid', 'gi_high', 'gi_negative'):
        assert q[s[name]] == -1.0, name
    assert (cols('gi_high') == 0.0).all() and (cols('gi_negative') == 0.0).all() and (q[len(s):] == -1.0).all()
    taken = q >= 0
    assert int(taken.sum()) == 9
    np.testing.assert_allclose(out[0], out64[0], rtol=1e-5)                    # 12 listed, 9 taken, four of them contribute 1
    assert abs(out[0, 0] - (9 - q[taken].sum()) / 12) < 1e-6
    assert abs(q[s['twice_a']] - q64[0, s['twice_a']]) <= bar and q[s['twice_a']] == q[s['twice_b']]
    for name in ('twice_a', 'plain'):                                          # listed twice: counted twice, gradient and term
        x, y, z = (int(v) for v in case['pos'][0, :, s[name]])
        want = grad64[x * W + y, A + 7 * z:A + 7 * z + 7]
        err = float(np.abs(cols(name) - want).max())
        print('%s: gradient error %.2e of %.3f' % (name, err, np.abs(want).max()))
        assert err <= 1e-5 * np.abs(want).max() + near['grad_bar']
    single = BR.kernel_entry(BR.reg_row(case, 0, 2, 2, 0)[0], case['anchors'][2, 2, 0], case['gts'][int(case['gi'][0, s['twice_a']])],
                             np.float64)[1] * (-1.0 / 12)
    np.testing.assert_allclose(cols('twice_a'), 2 * single, rtol=1e-4, atol=1e-6)
    # everything else of d_heads is what it was
    listed = _listed(case, case['heads'].shape[1]).numpy()
    assert (d[~listed] == 0.0).all()


# ---- 5. through the criterion -------------------------------------------------------------------------------------------------------
def _targets_of(case):
    out = []
    for f in range(case['F']):
        n_pos, n_neg = int(case['counts'][f, 0]), int(case['counts'][f, 1])
        lo, hi = int(case['gt_off'][f]), int(case['gt_off'][f + 1])
        if n_pos == 0 and n_neg == 0:
            out.append(None)
            continue
        pi = tuple(case['pos'][f, j, :n_pos] for j in range(3)) if n_pos else None
        ni = tuple(case['neg'][f, j, :n_neg] for j in range(3)) if n_neg else None
        out.append((pi, ni, case['gi'][f, :n_pos], torch.from_numpy(case['gts'][lo:hi].copy()) if hi > lo else None))
    return out


@pytest.mark.parametrize('kind', ['plain', 'direction', 'iou'])
def test_criterion_adds_the_term_to_the_regression_loss_and_gradient_only(kind):
    from modules.voxelnet.FocalLoss import FocalLoss
    case = IC.with_iou('case1')
    F, l, w, A = case['F'], case['l'], case['w'], case['A']
    heads = torch.from_numpy(case['heads'] if kind == 'plain' else IC.wide_rows(case)).cuda()
    kw = {'plain': {}, 'direction': dict(direction=True), 'iou': dict(direction=True, iou=True)}[kind]
    anchors = torch.from_numpy(case['anchors']).cuda()
    targets = _targets_of(case)
    off, on = FocalLoss(**kw), FocalLoss(iou_loss=True, iou_loss_weight=0.6, **kw)
    l0, has0, d0 = off.heads_loss_frames(heads, F, l, w, targets, anchors)
    l1, has1, d1 = on.heads_loss_frames(heads, F, l, w, targets, anchors)
    torch.cuda.synchronize()
    assert off.last_box_iou is None and tuple(on.last_box_iou.shape) == (F, 2) and has0 == has1
    assert l0.shape == l1.shape == (F, {'plain': 2, 'direction': 3, 'iou': 4}[kind]) and d0.shape == d1.shape == heads.shape
    term = on.last_box_iou[:, 0]
    print('%s: regression loss %s -> %s, term %s, mean IoU %s' % (kind, l0[:, 1].tolist(), l1[:, 1].tolist(), term.tolist(),
                                                                  on.last_box_iou[:, 1].tolist()))
    keep = [c for c in range(l0.shape[1]) if c != 1]
    assert torch.equal(l0[:, keep], l1[:, keep]) and torch.equal(l1[:, 1], l0[:, 1] + term) and float(term.max()) > 0.0
    reg = torch.zeros(heads.shape[1], dtype=torch.bool)
    reg[A:8 * A] = True
    assert torch.equal(d0[:, ~reg].view(torch.int32), d1[:, ~reg].view(torch.int32))
    assert not torch.equal(d0[:, reg], d1[:, reg])
    # the term and its gradient are those of the reference on the same rows
    c = dict(case, heads=heads.cpu().numpy())
    out64, grad64, _ = BR.loss_autograd(c, 0.6)
    np.testing.assert_allclose(on.last_box_iou.cpu().double().numpy(), out64, rtol=1e-4, atol=1e-6)
    added = (d1 - d0).cpu().double().numpy()
    assert np.abs(added - grad64).max() <= 1e-4 * np.abs(grad64).max() + 2.0 ** -22 * float(d0.abs().max())
    # forward only
    l2, _, none = on.heads_loss_frames(heads, F, l, w, targets, anchors, want_grads=False)
    assert none is None and torch.equal(l2, l1)


# ---- 6. through the pipeline --------------------------------------------------------------------------------------------------------
def test_whole_model_step_changes_the_regression_head_only(tmp_path):
    """pipeline.train_step_full on the two synthetic frames of the IoU-head pipeline test, MVXNet(direction=True, iou=True), with
    and without iou_loss: the losses differ in reg by the term, rpn.reg's gradient changes, the cls / dir / iou heads' gradients
    are bitwise what they were."""
    sys.path.insert(0, PKG)
    import modules.config as cfg
    from modules import parallel, pipeline as pl
    from modules.Calc import bbox3d2bev
    from modules.data import Load, Preprocessing as pre, Synthetic as S
    from modules.voxelnet.FocalLoss import FocalLoss
    from MVXNet import MVXNet
    import train_like
    root = str(tmp_path / 'kitti')
    S.write_kitti_tree(root, [0, 1], points=3000, raw_points=9000)
    ds = Load.createDataset(['000000', '000001'], root=root)
    dev = torch.device('cuda')
    anchors = pre.createAnchors(cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2, cfg.velorange, cfg.carsize)
    bevs = bbox3d2bev(anchors.reshape(anchors.shape[:2] + (-1, 7))).to(dev).contiguous()
    anchors = anchors.to(dev)
    np.random.seed(0)
    batch, targets = pl.batch_from_dataset(ds, ['000000', '000001'], dev, bevs, train_like.fpn_maps_for, cap_points=3000)
    assert any(t is not None and len(t[0][0]) > 0 for t in targets)
    res = {}
    for on in (False, True):
        torch.manual_seed(0)
        model = MVXNet(direction=True, iou=True).to(dev)
        bucket = parallel.GradBucket([p for p in model.parameters() if p.requires_grad])
        crit = FocalLoss(direction=True, iou=True, iou_loss=on)
        bucket.zero()
        keep = {}
        out = pl.train_step_full(model, batch, targets, crit, anchors, cfg.imsize, keep=keep)
        torch.cuda.synchronize()
        rpn = model.backbone.rpn
        res[on] = (out, keep['heads'].clone(), {n: getattr(rpn, n).weight.grad.clone() for n in ('cls', 'reg', 'dir', 'iou')},
                   {n: getattr(rpn, n).bias.grad.clone() for n in ('cls', 'reg', 'dir', 'iou')}, crit.last_box_iou)
    (o0, h0, w0, b0, none), (o1, h1, w1, b1, box) = res[False], res[True]
    assert none is None and torch.equal(h0, h1)                                # the same forward, bit for bit
    has = [t is not None and len(t[0][0]) > 0 for t in [targets[f] for f in o1['live']]]
    term = [v for v, h in zip(box[:, 0].tolist(), has) if h]
    print('reg loss %s -> %s, term %s, mean IoU of the positives %s' % (o0['reg'], o1['reg'], term, box[:, 1].tolist()))
    assert o0['cls'] == o1['cls'] and o0['dir'] == o1['dir'] and o0['iou'] == o1['iou']
    np.testing.assert_allclose(np.array(o1['reg']) - np.array(o0['reg']), term, rtol=1e-4, atol=1e-6)
    assert all(v > 0 for v in term) and all(0.0 <= v <= 1.0 for v in box[:, 1].tolist())
    for n in ('cls', 'dir', 'iou'):
        assert torch.equal(w0[n], w1[n]) and torch.equal(b0[n], b1[n]), n
    assert not torch.equal(w0['reg'], w1['reg']) and not torch.equal(b0['reg'], b1['reg'])
    assert bool(torch.isfinite(w1['reg']).all())
