"""``bntrack`` on the GPU (csrc/bn_running.hip, modules/bn_running.py): the update kernel against torch's BatchNorm, the table
kernel against float64, every BatchNorm site of the frame-set path wired in training and in eval mode, and the round trip
train_like.py --bn-track -> checkpoint -> detect_like.py."""
import os
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as Fn
from torch.nn.modules.batchnorm import _BatchNorm

import bn_running_ref as R
import bn_rows_cases as B

pytestmark = pytest.mark.gpu
DEV = 'cuda'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'mvxnet-makise_amd')
EPS = 1e-5


# ---- 1. the update kernel against torch ---------------------------------------------------------------------------------
@pytest.mark.parametrize('F,C,dead', [(1, 4, None), (1, 132, None), (3, 4, None), (3, 132, None), (3, 4, 1), (3, 132, 1)])
def test_update_kernel_is_torchs_batchnorm_frame_after_frame(F, C, dead):
    """mean_inv through the library's own statistics and finaliser, folded by ONE launch from non-trivial buffers, against
    ``torch.nn.BatchNorm2d(...).double()`` on the CPU fed the live frames one at a time.  inv is one f32 rounding of a float64
    value, so var + eps is good to about 2^-23, the single f32 store adds 2^-24: the buffers are held to 1e-6 (|expected| + eps),
    about five times their sum, the mean to 1e-6 |expected| + 1e-7 sqrt(var)."""
    import modules.config as cfg
    from modules import _hip
    from modules import Extension as X
    eps = cfg.eps
    h, w = 24, 32                                  # 768 sites per frame and channel: a stable variance
    gen = torch.Generator().manual_seed(100 * F + C)
    y = (torch.randn((F, h, w, C), generator=gen) * 3.0 + 1.5) * (1.0 + torch.arange(F).view(F, 1, 1, 1) * 0.25)
    rm0 = torch.randn((C,), generator=gen)
    rv0 = torch.rand((C,), generator=gen) + 0.5
    yd = y.to(DEV).contiguous()
    mi = _hip.bn_finalize(_hip.row_stats_frames(yd, C, F), h * w, eps, F)
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    nbt = torch.tensor(5, dtype=torch.int64, device=DEV)
    table = _hip.bn_site_table([(mi, rm, rv, nbt, 0.1, X.ROWS_GRID, F * h * w)])
    mask = None if dead is None else ((1 << F) - 1) & ~(1 << dead)
    c0 = X.lib.mvx_launch_count()
    _hip.bn_running_update_sites(table, F, eps, live_mask=mask)
    assert X.lib.mvx_launch_count() - c0 == 1
    torch.cuda.synchronize()
    erm, erv, n = R.torch_fold([None if f == dead else y[f] for f in range(F)], rm0, rv0, eps, 0.1)
    assert int(nbt) == 5 + n and n == F - (dead is not None)
    var = torch.stack([y[f].double().reshape(-1, C).var(dim=0, unbiased=False) for f in range(F) if f != dead]).min(dim=0).values
    e_m = (rm.cpu().double() - erm).abs()
    e_v = (rv.cpu().double() - erv).abs()
    print('update F %d C %d dead %s: mean %.2e of its bound, var %.2e of its bound'
          % (F, C, dead, float((e_m / (1e-6 * erm.abs() + 1e-7 * var.sqrt())).max()), float((e_v / (1e-6 * (erv.abs() + eps))).max())))
    assert bool((e_m <= 1e-6 * erm.abs() + 1e-7 * var.sqrt()).all())
    assert bool((e_v <= 1e-6 * (erv.abs() + eps)).all())
    # and the float64 restatement of the kernel, from the same mean_inv: one f32 store (the last bit is left to the two
    # float64 chains, one on the GPU, one in torch on the CPU)
    frm, frv, _ = R.fold(mi, [0 if f == dead else h * w for f in range(F)], rm0, rv0, eps, 0.1)
    assert R.ulp_distance(rm, frm.float()) <= 1 and R.ulp_distance(rv, frv.float()) <= 1


def _random_sites(n_sites, widths, pops, F, seed):
    from modules import Extension as X
    gen = torch.Generator().manual_seed(seed)
    sites, keep = [], []
    for k in range(n_sites):
        C, n = widths[k % len(widths)], pops[k % len(pops)]
        mi = torch.stack([torch.randn((F, C), generator=gen), torch.rand((F, C), generator=gen) + 0.5], dim=1).to(DEV).contiguous()
        rm, rv = torch.randn((C,), generator=gen).to(DEV), (torch.rand((C,), generator=gen) + 0.5).to(DEV)
        nbt = torch.tensor(k, dtype=torch.int64, device=DEV)
        keep.append((mi, rm.clone(), rv.clone(), rm, rv, nbt, n, 0.05 + 0.01 * (k % 40)))
        sites.append((mi, rm, rv, nbt, 0.05 + 0.01 * (k % 40), X.ROWS_GRID, F * n))
    return sites, keep


def _check_sites(keep, F, eps):
    for k, (mi, rm0, rv0, rm, rv, nbt, n, m) in enumerate(keep):
        frm, frv, live = R.fold(mi, [n] * F, rm0, rv0, eps, m)
        assert R.ulp_distance(rm, frm.float()) <= 1 and R.ulp_distance(rv, frv.float()) <= 1 and int(nbt) == k + F, k
        assert bool((rm != rm0).any())
        if n == 1:
            assert torch.equal(rv, rv0)


@pytest.mark.parametrize('n_sites,pops,launches', [
    (40, (1, 7, 30, 64, 200), 1),                                       # the model's case and more: one launch
    (60, (7, 30, 64), 2),                                               # more sites than one table holds: 48 + 12
    (20, (2, 3, 5, 7, 11, 13, 17, 19, 23, 29), 3),                      # more populations than one table holds: 8 + 8 + 4 sites
    (110, (2, 3, 5, 7, 11, 13, 17, 19, 23), 14)])                       # both limits: a table per 8 sites (the 9th population is new)
def test_update_kernel_population_of_one_and_tables_of_any_length(n_sites, pops, launches):
    """n_f = 1 folds the mean and leaves running_var alone; a table goes out in ONE launch while it has room for 48 sites and 8
    distinct populations, in further launches beyond; every site equals the float64 fold of its own mean_inv, exactly once."""
    import modules.config as cfg
    from modules import _hip
    from modules import Extension as X
    eps, F = cfg.eps, 2
    sites, keep = _random_sites(n_sites, (4, 16, 132, 256), pops, F, 3 + n_sites)
    c0 = X.lib.mvx_launch_count()
    _hip.bn_running_update_sites(_hip.bn_site_table(sites), F, eps)
    assert X.lib.mvx_launch_count() - c0 == launches
    torch.cuda.synchronize()
    _check_sites(keep, F, eps)
    # the eval direction over the same table: every mean_inv from its (just folded) buffers
    c0 = X.lib.mvx_launch_count()
    _hip.bn_running_mean_inv_sites(_hip.bn_site_table(sites), F, eps)
    assert X.lib.mvx_launch_count() - c0 == -(-n_sites // X.BN_SITES_PER_LAUNCH)
    torch.cuda.synchronize()
    for mi, _, _, rm, rv, _, _, _ in keep:
        assert R.ulp_distance(mi, R.mean_inv_of(rm, rv, eps, F)) <= 1


# ---- 2. the table kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [4, 132])
def test_table_kernel_is_float64_rounded_once(C):
    import modules.config as cfg
    from modules import _hip
    from modules import Extension as X
    eps, F = cfg.eps, 3
    gen = torch.Generator().manual_seed(C)
    rm = torch.randn((C,), generator=gen)
    rv = torch.rand((C,), generator=gen) * 4.0
    rv[0], rv[1] = 0.0, 1e-12                              # running_var = 0: 1 / sqrt(eps)
    buf = torch.full((F * 2 * C + 64,), float('nan'), device=DEV)           # mean_inv with 64 guard floats right behind it
    mi, guard = buf[:F * 2 * C].view(F, 2, C), buf[F * 2 * C:]
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    _hip.bn_running_mean_inv_sites(_hip.bn_site_table([(mi, rm.to(DEV), rv.to(DEV), nbt, 0.1, X.ROWS_GRID, 0)]), F, eps)
    torch.cuda.synchronize()
    ref = R.mean_inv_of(rm, rv, eps, F)
    assert torch.equal(mi[:, 0].cpu(), ref[:, 0])
    assert R.ulp_distance(mi[:, 1], ref[:, 1]) <= 1
    assert abs(float(mi[0, 1, 0]) - 1.0 / np.sqrt(eps)) <= 1.0 / np.sqrt(eps) * 2.0 ** -23
    for f in range(1, F):
        assert torch.equal(mi[f], mi[0])
    assert torch.isnan(guard).all() and int(nbt) == 0


# ---- the small model ----------------------------------------------------------------------------------------------------
@pytest.fixture
def small_tracked():
    """The small grid of tests/test_frames_gpu.py; ``bntrack`` is switched per model through the returned setter."""
    import modules.config as cfg
    old, old_r, old_t = list(cfg.config['voxelshape']), list(cfg.config['velorange']), cfg.config.get('bntrack', False)
    cfg.config['voxelshape'] = [16, 24, 10]
    cfg.config['velorange'] = [0.0, -2.4, -3.0, 3.2, 2.4, 1.0]
    cfg.config['voxelsize'] = [0.2, 0.2, 0.4]
    try:
        yield cfg
    finally:
        cfg.config['bntrack'] = old_t
        cfg.config['voxelshape'], cfg.config['velorange'] = old, old_r
        cfg.config['voxelsize'] = [(old_r[k + 3] - old_r[k]) / old[k] for k in range(3)]


def _batch(golden, B_, with_empty):
    from test_frames_gpu import _small_batch
    batch, _ = _small_batch(golden, B_, with_empty)
    for f in range(B_):
        nlive = int(batch.n_points[f])
        if nlive:
            batch.perms[f, :nlive] = torch.randperm(nlive, generator=torch.Generator().manual_seed(f)).to(DEV)
    return batch


def _targets(cfg, B_):
    """Anchors of the small grid and per frame two positives (ground truth = the anchor, moved a little), six negatives."""
    from modules.data import Preprocessing as pre
    h1, w1 = cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2
    anchors = pre.createAnchors(h1, w1, cfg.velorange, cfg.carsize)
    a4 = anchors.reshape(h1, w1, 2, 7)
    targets = []
    for f in range(B_):
        px, py, pa = [1 + f % 3, 5], [2, 7 + f % 3], [0, 1]
        gt = torch.stack([a4[x, y, a] for x, y, a in zip(px, py, pa)]).clone()
        gt[:, :3] += torch.tensor([0.05, -0.04, 0.02]) * (1 + f)
        gt[:, 6] += 0.05
        neg = ([0, 0, 3, 6, 7, 7], [0, 11, 4, 1, 10, 5], [0, 1, 0, 1, 0, 1])
        targets.append(((torch.tensor(px), torch.tensor(py), torch.tensor(pa)), tuple(torch.tensor(v) for v in neg),
                        torch.tensor([0, 1]), gt.to(DEV)))
    return anchors.to(DEV), targets


def _model(cfg, track):
    from MVXNet import MVXNet
    from modules import parallel
    cfg.config['bntrack'] = track
    torch.manual_seed(3)
    model = MVXNet().to(DEV)
    bucket = parallel.GradBucket([p for p in model.parameters() if p.requires_grad])
    return model, bucket


def _bns(model):
    return [(k, m) for k, m in model.named_modules() if isinstance(m, _BatchNorm)]


# ---- 3. every site is wired: training -------------------------------------------------------------------------------------
@pytest.mark.parametrize('B_,with_empty', [(3, False), (4, True)])
def test_training_step_folds_every_site_and_leaves_the_arithmetic_alone(golden, small_tracked, B_, with_empty):
    import modules.pipeline as pl
    from modules import Extension as X
    from modules.voxelnet import VoxelLoss
    cfg = small_tracked
    batch = _batch(golden, B_, with_empty)
    anchors, targets = _targets(cfg, B_)
    crit = VoxelLoss()
    res = {}
    for track in (True, False):
        model, bucket = _model(cfg, track)
        if track:
            gen = torch.Generator().manual_seed(9)
            for _, m in _bns(model):                          # non-trivial starting buffers, torch's momentum
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
        bucket.zero()
        pl.train_step_full(model, batch, targets, crit, anchors, cfg.imsize)          # warms the weight caches of this model
        before = {k: (m.running_mean.clone(), m.running_var.clone(), int(m.num_batches_tracked)) for k, m in _bns(model)} if track else None
        bucket.zero()
        keep = {}
        c0 = X.lib.mvx_launch_count()
        out = pl.train_step_full(model, batch, targets, crit, anchors, cfg.imsize, keep=keep)
        launches = X.lib.mvx_launch_count() - c0
        torch.cuda.synchronize()
        res[track] = (model, bucket.flat.clone(), out, launches, keep, before)
    model, flat_t, out_t, n_t, keep, before = res[True]
    plain, flat_u, out_u, n_u, keep_u, _ = res[False]
    live = B_ - int(with_empty)
    assert out_t['live'] == out_u['live'] and len(out_t['live']) == live
    # tracking does not touch the arithmetic: losses and every parameter gradient bit for bit, exactly one launch more
    assert out_t['loss'] == out_u['loss'] and out_t['cls'] == out_u['cls'] and out_t['reg'] == out_u['reg']
    assert all(torch.equal(a, b) for a, b in zip(model.parameters(), plain.parameters()))
    assert torch.equal(flat_t, flat_u) and float(flat_t.abs().max()) > 0.0
    assert torch.equal(keep['heads'], keep_u['heads'])
    assert n_t - n_u == 1, (n_t, n_u)
    assert 'bn_sites' not in keep_u and all(m.running_mean is None for _, m in _bns(plain)) and not any('.bn.' in k for k in plain.state_dict())
    # every BatchNorm module of the model is a site, once
    names = {id(m): k for k, m in _bns(model)}
    sites = keep['bn_sites']
    assert len(sites) == len(names) == 30 and {id(bn) for bn, _, _ in sites} == set(names)
    worst = 0.0
    for bn, mi, pop in sites:
        k = names[id(bn)]
        rm0, rv0, n0 = before[k]
        assert mi.shape == (live, 2, bn.num_features) and len(pop) == live and min(pop) > 1, k
        erm, erv, folded = R.fold(mi, pop, rm0, rv0, cfg.eps, bn.momentum)
        assert int(bn.num_batches_tracked) == n0 + live == 2 * live and folded == live, k
        for got, exp in ((bn.running_mean, erm), (bn.running_var, erv)):
            e = float(((got.cpu().double() - exp).abs() / (exp.abs() + cfg.eps)).max())
            worst = max(worst, e)
            assert e <= 3 * 2.0 ** -24, (k, e)
        # no buffer is left where it started
        assert bool((bn.running_mean != rm0).any()) and bool((bn.running_var != rv0).any()), k
    print('30 sites, %d live frames: buffers within %.2e of the float64 fold of their own mean_inv (bound %.2e)'
          % (live, worst, 3 * 2.0 ** -24))
    # the populations the fold took: the dense voxel rows for the row layouts, the sites of the map for the grids
    pops = {names[id(bn)]: pop for bn, _, pop in sites}
    vox = [v for v in out_t['voxels'] if v > 0]
    assert pops['head.fusion.fcn1.bn'] == pops['backbone.fcn.bn'] == [v * cfg.samplenum for v in vox]
    H, W = cfg.voxelshape[0], cfg.voxelshape[1]
    assert pops['backbone.cml.conv3.bn'] == [2 * H * W] * live and pops['backbone.rpn.blk3.5.bn'] == [H * W // 64] * live
    assert pops['backbone.rpn.deconv3.bn'] == pops['backbone.rpn.deconv2.bn'] == pops['backbone.rpn.deconv1.bn'] == [H * W // 4] * live


def test_fresh_buffers_move_and_the_other_entry_points_fold_their_sites(golden, small_tracked):
    """From torch's initial 0 / 1 no buffer stays there after one step; train_step_frame_set folds the 11 sites up to the CML,
    train_step_rows_only the 8 row sites; a training entry on an eval model, the per-frame executor and frame-set lanes refuse."""
    import modules.pipeline as pl
    from modules.Extension import MvxHipError
    from test_frames_gpu import _small_batch
    cfg = small_tracked
    batch = _batch(golden, 3, False)
    _, G = _small_batch(golden, 1)
    model, bucket = _model(cfg, True)
    bucket.zero()
    pl.train_step_frame_set(model, batch, G, [370.0, 1224.0])
    torch.cuda.synchronize()
    moved = [k for k, m in _bns(model) if int(m.num_batches_tracked) == 3]
    assert len(moved) == 11 and not any('.rpn.' in k for k in moved)
    for k, m in _bns(model):
        if k in moved:
            assert bool((m.running_mean != 0).all()) and bool((m.running_var != 1).all()), k
            assert bool(torch.isfinite(m.running_mean).all()) and bool((m.running_var > 0).all()), k
        else:
            assert int(m.num_batches_tracked) == 0 and bool((m.running_mean == 0).all()) and bool((m.running_var == 1).all()), k
    bucket.zero()
    pl.train_step_rows_only(model, batch, {}, with_fusion=True, imsize=[370.0, 1224.0])
    torch.cuda.synchronize()
    assert sorted(k for k, m in _bns(model) if int(m.num_batches_tracked) == 6) == sorted(k for k in moved if '.cml.' not in k)
    for call in (lambda: pl.train_step_frames(model, batch, G, [370.0, 1224.0]),):
        with pytest.raises(MvxHipError, match='frame-set path'):
            call()
    old = pl.SET_LANES
    pl.SET_LANES = 2
    try:
        with pytest.raises(MvxHipError, match='SET_LANES'):
            pl.train_step_frame_set(model, batch, G, [370.0, 1224.0])
    finally:
        pl.SET_LANES = old
    model.eval()
    with pytest.raises(MvxHipError, match='eval'):
        pl.train_step_frame_set(model, batch, G, [370.0, 1224.0])
    _hip_join()


def _hip_join():
    from modules import _hip
    _hip.join_side_stream()
    torch.cuda.synchronize()


# ---- 4. every site is wired: eval -------------------------------------------------------------------------------------------
def _rpn_eval_f64(rpn, x, eps):
    """The RPN in eval mode restated with torch in float64 on the CPU (voxelnet/Pipe.py:45-75): x (F,128,H,W)."""
    def p(t):
        return t.detach().cpu().double()

    def bn(m, y):
        return Fn.batch_norm(y, p(m.bn.running_mean), p(m.bn.running_var), None, None, False, 0.0, eps)

    outs = []
    for blk in (rpn.blk1, rpn.blk2, rpn.blk3):
        for li, m in enumerate(blk):
            x = bn(m, Fn.relu(Fn.conv2d(x, p(m.conv.weight), p(m.conv.bias), stride=2 if li == 0 else 1, padding=1)))
        outs.append(x)
    ups = [bn(m, Fn.relu(Fn.conv_transpose2d(o, p(m.deconv.weight), p(m.deconv.bias), stride=s, padding=pad)))
           for o, m, s, pad in zip(outs, (rpn.deconv1, rpn.deconv2, rpn.deconv3), (1, 2, 4), (1, 0, 0))]
    up = torch.cat(ups, dim=1)
    return (Fn.conv2d(up, p(rpn.cls.weight), p(rpn.cls.bias)), Fn.conv2d(up, p(rpn.reg.weight), p(rpn.reg.bias)))


def test_eval_forward_normalises_every_site_with_its_running_statistics(golden, small_tracked):
    from modules import _hip
    from modules import Extension as X
    from modules.detect import detect_frame_set
    cfg = small_tracked
    batch = _batch(golden, 3, False)
    anchors, _ = _targets(cfg, 3)
    model, bucket = _model(cfg, True)
    bucket.zero()
    gen = torch.Generator().manual_seed(21)
    for _, m in _bns(model):                                  # distinct values, NOT the batch statistics
        m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.2 + 0.1)
        m.running_var.copy_(torch.rand(m.num_features, generator=gen) * 0.5 + 0.25)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    # training mode first: batch statistics as ever, nothing written
    kt = {}
    detect_frame_set(model, batch, anchors, cfg.imsize, keep=kt, score_thr=0.0)
    model.eval()
    ke = {}
    dets = detect_frame_set(model, batch, anchors, cfg.imsize, keep=ke, score_thr=0.0)
    torch.cuda.synchronize()
    assert len(dets) == 3 and all(bool(torch.isfinite(d['boxes']).all()) for d in dets)
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k
    for k, p_ in model.named_parameters():
        if k in grads:
            assert torch.equal(p_.grad, grads[k]), k
    F = 3
    names = {id(m): k for k, m in _bns(model)}
    sites = ke['bn_sites']
    assert len(sites) == 30 and {id(bn) for bn, _, _ in sites} == set(names) and len(kt['bn_sites']) == 30
    # every site's mean_inv is bitwise the table kernel's output for its module
    for bn, mi, _ in sites:
        own = torch.empty_like(mi)
        _hip.bn_running_mean_inv_sites(_hip.bn_site_table([(own, bn.running_mean, bn.running_var, bn.num_batches_tracked, 0.1,
                                                             X.ROWS_GRID, 0)]), F, cfg.eps)
        assert torch.equal(mi, own), names[id(bn)]
        assert R.ulp_distance(mi, R.mean_inv_of(bn.running_mean, bn.running_var, cfg.eps, F)) <= 1, names[id(bn)]
    # the saved state of the forward holds the same tensors
    S, rs = ke['saved'], ke['rpn']
    by_module = {id(bn): mi for bn, mi, _ in sites}
    fus = model.head.fusion._bns()
    for i, rec in enumerate(S.fusion):
        assert rec[4] is by_module[id(fus[i])]
    # the next layer's input = (y - running_mean) * inv, formed by torch from the saved y (the bound of tests/test_bn_rows_gpu.py)
    def applied(y, bn):
        C = bn.num_features
        yd = y.detach().cpu().double().reshape(-1, C)
        return (yd - bn.running_mean.cpu().double()) / torch.sqrt(bn.running_var.cpu().double() + cfg.eps)
    worst = 0.0
    for i in range(len(S.fusion) - 1):
        ref = applied(S.fusion[i][3], fus[i])
        e = float((S.fusion[i + 1][0].cpu().double() - ref).abs().max() / ref.abs().max())
        worst = max(worst, e)
        assert e < B.BOUND, ('fusion', i, e)
    n_s1 = 0
    for blk in rs['blocks']:
        layers = blk['layers']
        for li, rec in enumerate(layers):
            if rec['kind'] != 's1':
                continue
            nxt = layers[li + 1]['x'] if li + 1 < len(layers) else blk['out']
            ref = applied(rec['y'], rec['m'].bn)
            e = float((nxt.cpu().double().reshape(ref.shape) - ref).abs().max() / ref.abs().max())
            worst = max(worst, e)
            n_s1 += 1
            assert e < B.BOUND, ('rpn', rec['bi'], li, e)
    assert n_s1 == 13
    print('eval apply of 4 fusion + 13 RPN layers: %.2e of the largest value (bound %.0e)' % (worst, B.BOUND))
    # same input, same products: the first fusion layer's pre-normalisation y, eval against training mode
    assert torch.equal(S.fusion[0][3], kt['saved'].fusion[0][3])
    assert not torch.equal(S.fusion[1][0], kt['saved'].fusion[1][0])            # ... normalised differently
    # the RPN heads against the float64 restatement, fed the library's own normalised CML output
    Fq, h1, w1 = ke['geom']
    x3 = S.x3.view(F, S.D3, S.H, S.W, S.C3).permute(0, 4, 1, 2, 3).reshape(F, S.C3 * S.D3, S.H, S.W).cpu().double()
    cls, reg = _rpn_eval_f64(model.backbone.rpn, x3, cfg.eps)
    heads = ke['heads'].view(F, h1, w1, 16).cpu().double()
    e_score = float((torch.sigmoid(heads[..., :2]) - torch.sigmoid(cls.permute(0, 2, 3, 1))).abs().max())
    e_reg = float((heads[..., 2:] - reg.permute(0, 2, 3, 1)).abs().max() / reg.abs().max())
    print('eval RPN heads vs float64 torch: score %.2e (abs), reg %.2e (max-norm rel); bound 1e-4 (tests/test_rpn_gpu.py)' % (e_score, e_reg))
    assert e_score < 1e-4 and e_reg < 1e-4


# ---- 5. round trip ----------------------------------------------------------------------------------------------------------
def _result_files(out, names):
    return {n: open(os.path.join(out, n + '.txt')).read() for n in names}


def test_train_like_checkpoint_runs_in_eval_mode_in_detect_like(tmp_path, capsys):
    sys.path.insert(0, PKG)
    import detect_like
    import modules.config as cfg
    import train_like
    from modules import bn_running as bnr
    root, ck = str(tmp_path / 'kitti'), str(tmp_path / 'ck')
    args = train_like.parse_args([root, '--synthetic', '8', '--mode', 'fast', '--bn-track', '--steps', '3', '--frames', '2',
                                  '--points', '3000', '--checkpoints', ck, '--quiet'])
    np.random.seed(0)
    r = train_like.train(args)
    assert r['steps'] == 3 and len(r['losses']) == 6 and all(np.isfinite(v) for v in r['losses'])
    assert not cfg.config.get('bntrack', False)                # the switch lasted as long as the run
    path = os.path.join(ck, 'epoch1.pkl')
    state = torch.load(path, map_location='cpu')
    counts = [int(v) for k, v in state.items() if k.endswith('.num_batches_tracked')]
    assert len(counts) == 30 and set(counts) == {6}            # 3 steps of 2 live frames
    for k, v in state.items():
        if k.endswith('.running_var'):
            assert bool((v > 0).all()) and bool((v != 1).any()) and bool(torch.isfinite(state[k[:-3] + 'mean']).all()), k
    names = open(os.path.join(root, 'ImageSets', 'train.txt')).read().split()[:4]
    with open(os.path.join(root, 'ImageSets', 'four.txt'), 'w') as f:
        f.write('\n'.join(names) + '\n')
    common = [root, '--split', 'four', '--frames', '2', '--points', '3000', '--score-thr', '0.0', '--pre-max', '64', '--post-max', '16']
    capsys.readouterr()
    detect_like.main(detect_like.parse_args(common + ['--checkpoint', path, '--out', str(tmp_path / 'run')]))
    assert 'eval mode' in capsys.readouterr().out and not cfg.config.get('bntrack', False)
    run = _result_files(str(tmp_path / 'run'), names)
    rows = [ln.split() for text in run.values() for ln in text.splitlines()]
    assert rows and all(np.isfinite([float(v) for v in row[1:]]).all() for row in rows)
    # per-frame statistics on the same weights: the files of an untracked model
    detect_like.main(detect_like.parse_args(common + ['--checkpoint', path, '--bn-stats', 'batch', '--out', str(tmp_path / 'batch')]))
    plain = os.path.join(ck, 'plain.pkl')
    torch.save(bnr.strip_running(state), plain)
    detect_like.main(detect_like.parse_args(common + ['--checkpoint', plain, '--out', str(tmp_path / 'plain')]))
    assert 'eval mode' not in capsys.readouterr().out
    batch_files = _result_files(str(tmp_path / 'batch'), names)
    assert batch_files == _result_files(str(tmp_path / 'plain'), names)
    assert batch_files != run                                  # running statistics give other boxes than the frames' own
    # resuming the untracked weights into a tracked model is allowed and says so
    os.replace(plain, os.path.join(ck, 'epoch2.pkl'))
    torch.save(torch.load(os.path.join(ck, 'epoch1_opt.pkl')), os.path.join(ck, 'epoch2_opt.pkl'))
    args2 = train_like.parse_args([root, '-r', '2', '--mode', 'fast', '--bn-track', '--bn-momentum', '0.2', '--steps', '1',
                                   '--frames', '2', '--points', '3000', '--checkpoints', ck])
    r2 = train_like.train(args2)
    assert 'holds no running statistics' in capsys.readouterr().out
    bns = [m for m in r2['model'].modules() if isinstance(m, _BatchNorm)]
    assert all(int(m.num_batches_tracked) == 2 and m.momentum == 0.2 for m in bns)
