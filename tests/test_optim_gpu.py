"""The fused AdamW (csrc/optim.hip, modules/optim.py) on the GPU against tests/optim_ref.py, the float64 restatement of its
contract, and against torch.optim.AdamW.

Parity tolerance: torch's CPU float32 ``AdamW(foreach=False)`` implements the same contract; its largest absolute distance from
the float64 reference on the same inputs is measured here, per quantity (p, m, v), and the device gets 4x that distance (the
margin covers the different rounding order of the two scalar factors: torch divides by sqrt(1 - beta2^t), the kernel multiplies
by its reciprocal).  The bound never comes from the device result.

Shapes and their flat offsets: (1,) at 0 and (5, 7) at 4 (16-byte path with a scalar tail), (3,) at 1 and (4097,) at 39
(misaligned: scalar path, one full chunk + a chunk of one), (64, 64) at 4136 (16-byte path, exactly one full chunk), (2, 3, 3, 3,
3) at 8232 (16-byte path, tail of 2), (8192,) at 8394 (scalar path, two full chunks); 16,586 elements, slices of 20 elements per
workgroup in the norm pass."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from optim_ref import RefAdamW, max_dist      # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'mvxnet-makise_amd')
SHAPES = [(1,), (3,), (5, 7), (4097,), (64, 64), (2, 3, 3, 3, 3), (8192,)]
EPS = 1e-6
pytestmark = pytest.mark.gpu


def _inputs(steps=10, scale=1.0):
    """Seeded parameters and ``steps`` gradient lists, on the CPU (f32)."""
    g = torch.Generator().manual_seed(1234)
    params = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[scale * torch.randn(s, generator=g) * (0.1 + k % 3) for s in SHAPES] for k in range(steps)]
    return params, grads


class TorchCPU:
    """torch.optim.AdamW(foreach=False) on float32 CPU clones; ``div`` divides the gradients first (f32), ``max_norm`` clips them
    with torch.nn.utils.clip_grad_norm_."""

    def __init__(self, params, **kw):
        self.ps = [torch.nn.Parameter(p.clone()) for p in params]
        self.opt = torch.optim.AdamW(self.ps, eps=EPS, foreach=False, **kw)

    def step(self, grads, max_norm=0.0, div=None):
        for p, g in zip(self.ps, grads):
            p.grad = g.clone() if div is None else g / div
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(self.ps, max_norm, foreach=False)
        self.opt.step()

    def pmv(self):
        st = self.opt.state
        return ([p.detach().numpy() for p in self.ps], [st[p]['exp_avg'].numpy() for p in self.ps],
                [st[p]['exp_avg_sq'].numpy() for p in self.ps])


class Hip:
    def __init__(self, params, late_idx=(), **kw):
        from modules import optim, parallel
        self.ps = [torch.nn.Parameter(p.clone().cuda()) for p in params]
        bucket = parallel.GradBucket(self.ps, late=[self.ps[i] for i in late_idx]) if late_idx else None
        self.opt = optim.AdamW(self.ps, eps=EPS, bucket=bucket, **kw)

    def step(self, grads, **kw):
        for p, g in zip(self.ps, grads):
            p.grad.copy_(g)
        self.opt.step(**kw)

    def pmv(self):
        o = self.opt
        return ([p.detach().cpu().numpy() for p in self.ps], [o.moments(p)[0].cpu().numpy() for p in self.ps],
                [o.moments(p)[1].cpu().numpy() for p in self.ps])


def _ref_pmv(ref):
    return ref.p, ref.m, ref.v


def _assert_parity(hip, tcpu, ref, what):
    """Device within 4x torch-CPU's own distance from the float64 reference, per quantity; prints the figures first."""
    for name, h, t, r in zip('pmv', hip.pmv(), tcpu.pmv(), _ref_pmv(ref)):
        d_t, d_h = max_dist(r, t), max_dist(r, h)
        print('%s %s: torch-CPU %.3e, device %.3e (bound %.3e)' % (what, name, d_t, d_h, 4 * d_t))
        assert d_t > 0.0 and d_h <= 4 * d_t, (what, name, d_h, d_t)


def _bitwise(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for qa, qb in zip(a.pmv(), b.pmv()) for x, y in zip(qa, qb))


@pytest.mark.parametrize('wd,betas', [(0.01, (0.9, 0.999)), (0.0, (0.8, 0.99))])
def test_parity_after_1_and_10_steps(wd, betas):
    params, grads = _inputs(10)
    kw = dict(lr=1e-3, betas=betas, weight_decay=wd)
    hip, tcpu, ref = Hip(params, **kw), TorchCPU(params, **kw), RefAdamW(params, eps=EPS, **kw)
    for k in range(10):
        hip.step(grads[k]); tcpu.step(grads[k]); ref.step(grads[k])
        if k in (0, 9):
            _assert_parity(hip, tcpu, ref, 'step %d wd %g' % (k + 1, wd))
    assert hip.opt.steps() == 10 and hip.opt.skipped_steps() == 0


def test_clipping():
    params, grads = _inputs(2)
    n0 = float(np.sqrt(sum(float((g.double() ** 2).sum()) for g in grads[0])))
    grads = [[g * (50.0 / n0) for g in gs] for gs in grads]            # norm of the first step about 50
    kw = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)
    hip, tcpu, ref = Hip(params, max_norm=10.0, **kw), TorchCPU(params, **kw), RefAdamW(params, eps=EPS, max_norm=10.0, **kw)
    for k in range(2):
        hip.step(grads[k]); tcpu.step(grads[k], max_norm=10.0); ref.step(grads[k])
        assert 40.0 < ref.norm and ref.coef < 0.25
        assert hip.opt.last_norm() == pytest.approx(ref.norm, rel=1e-12)
        assert hip.opt.last_coef() == pytest.approx(ref.coef, rel=1e-12)
    _assert_parity(hip, tcpu, ref, 'clipped')
    # a limit that never binds is no clipping at all: coef = 1 exactly
    a, b = Hip(params, max_norm=1e9, **kw), Hip(params, max_norm=0.0, **kw)
    for k in range(2):
        a.step(grads[k]); b.step(grads[k])
    assert a.opt.last_coef() == 1.0 and _bitwise(a, b)


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
def test_guard_skips_a_non_finite_step(bad):
    """One inf / NaN at the last element of the (3,) parameter's gradient (flat offset 3; that parameter takes the scalar path
    of the update).  The step changes nothing, is counted, and does not advance t: the next clean step equals the first clean
    step of a fresh optimizer bit for bit.  With ``guard=False`` none of this is required: the value goes into the weights as it
    does with torch."""
    params, grads = _inputs(1)
    kw = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01, max_norm=10.0)
    clean = Hip(params, **kw)
    clean.step(grads[0])
    poisoned = [g.clone() for g in grads[0]]
    poisoned[1][-1] = bad
    hip, fresh = Hip(params, **kw), Hip(params, **kw)
    hip.step(poisoned)
    assert _bitwise(hip, fresh)                                     # p as initialised, m = v = 0
    assert hip.opt.skipped_steps() == 1 and hip.opt.steps() == 0
    hip.step(grads[0])
    assert _bitwise(hip, clean) and hip.opt.steps() == 1 and hip.opt.skipped_steps() == 1


def test_count_slot_scales_the_gradient():
    params, grads = _inputs(2)
    kw = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)
    hip, tcpu, ref = Hip(params, **kw), TorchCPU(params, **kw), RefAdamW(params, eps=EPS, **kw)
    three = torch.tensor([3.0], device='cuda')
    for k in range(2):
        hip.step(grads[k], count=three); tcpu.step(grads[k], div=3.0); ref.step(grads[k], count=3.0)
    _assert_parity(hip, tcpu, ref, 'count 3')
    a, b, c = Hip(params, **kw), Hip(params, **kw), Hip(params, **kw)
    for k in range(2):
        a.step(grads[k], count=torch.tensor([0.0], device='cuda'))
        b.step(grads[k], count=torch.tensor([1.0], device='cuda'))
        c.step(grads[k])
    assert _bitwise(a, b) and _bitwise(b, c)


def test_two_runs_are_bitwise_identical():
    params, grads = _inputs(5)
    kw = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01, max_norm=1.0)
    a, b = Hip(params, **kw), Hip(params, **kw)
    for k in range(5):
        a.step(grads[k]); b.step(grads[k])
    assert _bitwise(a, b)
    assert a.opt.last_norm() == b.opt.last_norm() and a.opt.last_coef() == b.opt.last_coef() < 1.0


def test_flat_buffers_off_the_16_byte_grid():
    """The ABI asks 4-byte alignment of the flat buffers only.  With all three one element off the 16-byte grid every slice of the
    norm pass starts with a scalar head, and the chunks that were aligned are not any more ((4097,) at 39 + 1 the other way
    round): p, m and v must not depend on it, bit for bit, nor the norm beyond f64 rounding."""
    from modules import _hip, optim
    params, grads = _inputs(2)
    kw = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)       # no clipping: the norms agree to f64 rounding, not bitwise
    hip = Hip(params, **kw)
    ps = [p.clone().cuda() for p in params]
    n = sum(p.numel() for p in ps)
    g, m, v = (torch.zeros(n + 1, device='cuda')[1:] for _ in range(3))
    assert g.data_ptr() % 16 == 4
    table = torch.from_numpy(optim.chunk_table([torch.nn.Parameter(p) for p in ps])).cuda()
    state = torch.zeros(8, dtype=torch.float64, device='cuda')
    for k in range(2):
        hip.step(grads[k])
        g.copy_(torch.cat([x.reshape(-1) for x in grads[k]]))
        _hip.optim_adamw_step(table, g, m, v, None, state, 1e-3, 0.9, 0.999, EPS, 0.01, 0.0, True)
        assert float(state[2]) == pytest.approx(hip.opt.last_norm(), rel=1e-13) and float(state[3]) == 1.0
    hp, hm, hv = hip.pmv()
    off = 0
    for i, p in enumerate(ps):
        k = p.numel()
        for got, want in ((p, hp[i]), (m[off:off + k], hm[i]), (v[off:off + k], hv[i])):
            assert np.array_equal(got.cpu().numpy().reshape(-1).view(np.uint32), want.reshape(-1).view(np.uint32)), i
        off += k


def test_step_advances_every_parameter_version():
    params, grads = _inputs(1)
    hip = Hip(params, lr=1e-3)
    before = [p._version for p in hip.ps]
    hip.step(grads[0])
    assert all(p._version > v for p, v in zip(hip.ps, before))


@pytest.fixture(scope='module')
def torch_four_steps():
    """Pure torch-CPU run and float64 reference over 4 steps: the interchange tests' tolerance (no device result in it)."""
    params, grads = _inputs(4)
    kw = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)
    tcpu, ref = TorchCPU(params, **kw), RefAdamW(params, eps=EPS, **kw)
    for k in range(4):
        tcpu.step(grads[k]); ref.step(grads[k])
    return {n: 4 * max_dist(r, t) for n, t, r in zip('pmv', tcpu.pmv(), _ref_pmv(ref))}


@pytest.mark.parametrize('direction', ['hip->torch', 'torch->hip'])
def test_checkpoint_interchange(direction, torch_four_steps):
    """Three steps with one optimizer, its state_dict() loaded by the other, one more step on each side with the same
    gradient.  The bucket is reordered by a ``late=`` list, so a state keyed by bucket position instead of by the order the
    parameters were passed in would land on the wrong parameter (and on the wrong shape)."""
    params, grads = _inputs(4)
    kw = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)
    hip, tcpu = Hip(params, late_idx=(2, 4), **kw), TorchCPU(params, **kw)
    assert [tuple(p.shape) for p in hip.opt.bucket.params] != [tuple(p.shape) for p in hip.ps]
    first, second = (hip, tcpu) if direction == 'hip->torch' else (tcpu, hip)
    for k in range(3):
        first.step(grads[k])
    sd = first.opt.state_dict()
    assert sorted(sd['state']) == list(range(len(SHAPES))) and set(sd['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq'}
    assert [tuple(sd['state'][i]['exp_avg'].shape) for i in range(len(SHAPES))] == SHAPES
    assert sd['state'][0]['step'].dtype == torch.float32 and float(sd['state'][0]['step']) == 3.0
    assert set(sd['param_groups'][0]) == set(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]).state_dict()['param_groups'][0])
    second.opt.load_state_dict(sd)
    with torch.no_grad():
        for q, p in zip(second.ps, first.ps):
            q.copy_(p.detach())
    first.step(grads[3]); second.step(grads[3])
    assert hip.opt.steps() == 4
    for name, h, t in zip('pmv', hip.pmv(), tcpu.pmv()):
        d = max(float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) for x, y in zip(h, t))
        print('%s %s: device vs torch %.3e (bound %.3e)' % (direction, name, d, torch_four_steps[name]))
        assert d <= torch_four_steps[name], (direction, name, d)


def test_in_the_model(tmp_path):
    """One whole-model step on two synthetic frames, then the HIP optimizer on the model against torch's CPU AdamW and the
    float64 reference on clones; a second step on the same batch must see the new weights (the packed-weight caches key on the
    parameter version: stale caches would reproduce the first losses)."""
    import modules.config as cfg
    from modules import optim, parallel, pipeline as pl
    from modules.Calc import bbox3d2bev
    from modules.data import Load, Preprocessing as pre, Synthetic as S
    from modules.voxelnet import VoxelLoss
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
    bucket = parallel.GradBucket(params, late=[model.head.fusion.fcn1.fc.weight])
    kw = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)
    opt = optim.AdamW(params, eps=cfg.eps, bucket=bucket, **kw)
    crit = VoxelLoss()
    np.random.seed(0)
    batch, targets = pl.batch_from_dataset(ds, ['000000', '000001'], dev, bevs, train_like.fpn_maps_for, cap_points=3000)
    opt.zero_grad()
    out1 = pl.train_step_full(model, batch, targets, crit, anchors, cfg.imsize)
    p0 = [p.detach().cpu() for p in params]
    g0 = [p.grad.detach().cpu().clone() for p in params]
    assert all(bool(torch.isfinite(g).all()) for g in g0)
    opt.step()
    tcpu = torch.optim.AdamW([torch.nn.Parameter(p.clone()) for p in p0], eps=cfg.eps, foreach=False, **kw)
    tps = tcpu.param_groups[0]['params']
    for p, g in zip(tps, g0):
        p.grad = g
    tcpu.step()
    ref = RefAdamW([p.numpy() for p in p0], eps=cfg.eps, **kw)
    ref.step([g.numpy() for g in g0])
    got = ([p.detach().cpu().numpy() for p in params], [opt.moments(p)[0].cpu().numpy() for p in params],
           [opt.moments(p)[1].cpu().numpy() for p in params])
    tor = ([p.detach().numpy() for p in tps], [tcpu.state[p]['exp_avg'].numpy() for p in tps],
           [tcpu.state[p]['exp_avg_sq'].numpy() for p in tps])
    for name, h, t, r in zip('pmv', got, tor, _ref_pmv(ref)):
        d_t, d_h = max_dist(r, t), max_dist(r, h)
        print('model %s: torch-CPU %.3e, device %.3e (bound %.3e)' % (name, d_t, d_h, 4 * d_t))
        assert d_t > 0.0 and d_h <= 4 * d_t, (name, d_h, d_t)
    assert opt.last_norm() == pytest.approx(ref.norm, rel=1e-12) and opt.skipped_steps() == 0
    opt.zero_grad()
    out2 = pl.train_step_full(model, batch, targets, crit, anchors, cfg.imsize)
    assert len(out2['loss']) == len(out1['loss']) == 2 and all(np.isfinite(v) for v in out2['loss'])
    assert all(a != b for a, b in zip(out1['loss'], out2['loss'])), (out1['loss'], out2['loss'])


def test_two_ranks_data_parallel_with_the_hip_optimizer(tmp_path):
    """Two ranks on one GPU (gloo, as the existing rehearsal), each process under its own ``timeout -k 10``: train_like.py in
    --mode fast with the HIP optimizer, clipping on, the division by the global frame count folded into the update.  The
    script ends in assert_replicas_in_sync: a non-zero exit code means the replicas diverged (or a rank failed)."""
    root = str(tmp_path / 'kitti')
    sk = socket.socket()
    sk.bind(('127.0.0.1', 0))
    port = sk.getsockname()[1]
    sk.close()
    cmd = ['timeout', '-k', '10', '300', sys.executable, os.path.join(PKG, 'train_like.py'), root, '--mode', 'fast', '--optimizer', 'hip',
           '--clip-grad-norm', '10', '--steps', '2', '--synthetic', '4', '--points', '3000', '--frames', '1', '--checkpoints',
           str(tmp_path / 'ck')]
    procs = []
    for rank in range(2):
        env = dict(os.environ, MVX_DIST_BACKEND='gloo', RANK=str(rank), LOCAL_RANK='0', WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=str(tmp_path)))
    outs = [p.communicate() for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, (so[-1500:], se[-3000:])
    assert 'optimizer: step 2' in outs[0][0] and '0 step(s) skipped' in outs[0][0]


@pytest.mark.parametrize('mode', ['fast', 'module'])
def test_train_like_resumes_across_optimizers(tmp_path, mode):
    """torch -> hip -> torch: each run resumes model and optimizer state from the checkpoint the other optimizer wrote."""
    import train_like
    from modules.data import Synthetic as S
    root = str(tmp_path / 'kitti')
    S.write_kitti_tree(root, [0, 1], points=3000, raw_points=9000)
    ck = str(tmp_path / 'ck')
    base = [root, '-n', '1', '--mode', mode, '--frames', '2', '--points', '3000', '--checkpoints', ck, '--quiet', '--steps', '1']
    np.random.seed(0)
    train_like.train(train_like.parse_args(base))
    r2 = train_like.train(train_like.parse_args(base + ['-r', '1', '--optimizer', 'hip', '--clip-grad-norm', '10', '--lr-schedule',
                                                        'cosine', '--warmup-steps', '1']))
    assert r2['steps'] == 1 and all(np.isfinite(v) for v in r2['losses'])
    assert r2['opt'].steps() == 2 and r2['opt'].skipped_steps() == 0            # torch's step count was restored and advanced
    r3 = train_like.train(train_like.parse_args(base + ['-r', '2']))
    assert all(np.isfinite(v) for v in r3['losses'])
    st = r3['opt'].state_dict()['state']
    assert st and all(int(v['step']) == 3 for v in st.values())
