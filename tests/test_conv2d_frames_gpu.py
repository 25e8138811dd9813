"""The exact-f32 2-D convolution entry points of the RPN (mvx_conv2d_forward_frames, mvx_conv2d_dgrad_frames,
mvx_conv2d_wgrad_frames; csrc/conv3d.hip) through the C ABI against torch.nn.functional.conv2d in float64 on the CPU, frame by
frame: y before the BatchNorm, mean and inverse deviation per frame, dx, and dW summed over the frames.

MVX_FLAG_TAPS2 cases compare the CHAIN with a true stride-2, padding-1 convolution of the ORIGINAL image with the ORIGINAL weight:
the space-to-depth image is built by mvx_space_to_depth_frames, the weight rearranged by rpn_frames._s2d_weight, the input
gradient brought back by the reverse shuffle and the weight gradient folded back as rpn_frames._s2d_weight_grad does; with
planes = 2 the reference's channel is c * planes + d.

Cases (h, w of the convolved map):
    ragged      F = 3, 21 x 37, 64 -> 128, stride 1; ragged in both axes, every frame its own input scale
    taps2p2     F = 2, 9 x 17, 4*64 -> 128, TAPS2, two planes of 32 channels: a parity block (64) is two K chunks, the
                structural zeros are skipped
    taps2k16    F = 2, 9 x 17, 4*16 -> 64, TAPS2: a parity block of 16 channels is no whole K chunk (32), conv_set_taps2 leaves
                s2d = 0 and the structural zeros are executed
    onetile     F = 1, 8 x 16, 32 -> 64: exactly one tile (forward only: the input- and weight-gradient kernels take cin in
                multiples of 64 and refuse this one with the size error, writing nothing)
    onesite     F = 1, 1 x 1, 64 -> 64: every tap but the centre in the padding
    persistent  F = 4, 53 x 100, 32 -> 256, stride 1, forward only, with a zeroed work counter: 49 tiles x 4 frames x 4 channel
                blocks = 784 units > 3 x CUs, so the launch is the persistent one and the last workgroup finalises the
                statistics; again with tuning key 2 = 1 << 60 (32-channel units, 1568 units)

Every destination, statistics and workspace buffer starts as NaN (counters as a sentinel) with a guard behind it; afterwards
exactly the outputs differ.  Bounds: 1e-5 of the largest float64 magnitude (the project's bound for these kernels,
tests/test_conv3d_gpu.py), 2e-5 for mean and inverse deviation.  Every case prints its errors (-s).

Measured on an MI355X in one run of this file (y, mean, inverse deviation; dx; dW, the same accumulated into 0.5):
    ragged      9.155e-07 8.310e-08 1.297e-07; 1.058e-06; 4.142e-07 4.142e-07
    taps2p2     7.934e-07 1.395e-07 2.057e-07; 7.871e-07; 3.840e-07 3.840e-07 (dW folded back on the 3 x 3 kernel)
    taps2k16    3.846e-07 8.944e-08 1.396e-07; 5.356e-07; 3.524e-07 3.524e-07
    onetile     4.599e-07 1.131e-07 2.546e-07
    onesite     2.366e-07 2.366e-07 0;         1.640e-07; 4.835e-08 8.337e-08
    persistent  8.680e-07 6.665e-08 6.435e-08 with 64- and with 32-channel units alike
taps2k16 first showed that the weight gradient returned the executed structural zeros as non-zero numbers (-59.6 in the first
element); wgrad_reduce now returns them as zero, as include/mvx_hip.h promises."""
import ctypes

import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
GUARD = 64
EPS = 1e-6
BOUND, BOUND_MI = 1e-5, 2e-5
SENTINEL = 0x5a5a5a5a
K_CHUNK = 32                           # BK of csrc/conv_geom.h


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _nan(n, dtype=torch.float32):
    return torch.full((n,), NAN, dtype=dtype, device=DEV)


def _dev(t):
    """A device copy with GUARD NaN elements behind it."""
    buf = _nan(t.numel() + GUARD)
    buf[:t.numel()] = t.reshape(-1).to(DEV)
    return buf[:t.numel()].view(t.shape)


def _counter(first):
    c = torch.full((1 + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    c[0] = first
    return c


def rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-300))


def _nchw(t):
    """channels-last (F, h, w, c) f32 -> float64 (F, c, h, w) on the CPU"""
    return t.detach().cpu().double().permute(0, 3, 1, 2).contiguous()


# ---- calls -------------------------------------------------------------------------------------------------------------------
def forward(x, wpk, b, F, h, w, cin, cout, flags, persistent=False):
    """-> y (F, h, w, cout), mean_inv (F, 2, cout); the guards are checked here."""
    from modules import _hip
    from modules import Extension as X
    n, ns = F * h * w * cout, F * _hip.STATS_REPLICAS * 2 * cout
    y, st, mi = _nan(n + GUARD), _nan(ns + GUARD, torch.float64), _nan(F * 2 * cout + GUARD)
    done, work = _counter(SENTINEL), _counter(0)
    rc = X.lib.mvx_conv2d_forward_frames(_p(x), _p(wpk), _p(b), _p(y), _p(st), h, w, cin, cout, _hip.FLAG_RELU | flags, _p(done), EPS,
                                         _p(mi), _p(work) if persistent else None, F, X.stream())
    torch.cuda.synchronize()
    assert rc == 0, 'mvx_conv2d_forward_frames returned %d' % rc
    assert torch.isnan(y[n:]).all() and torch.isnan(st[ns:]).all() and torch.isnan(mi[F * 2 * cout:]).all()
    assert (done[1:] == SENTINEL).all() and (work[1:] == SENTINEL).all()
    assert not torch.isnan(y[:n]).any() and not torch.isnan(st[:ns]).any() and not torch.isnan(mi[:F * 2 * cout]).any()
    return y[:n].view(F, h, w, cout), mi[:F * 2 * cout].view(F, 2, cout)


def dgrad(dz, wpk_d, F, h, w, cin, cout, flags, expect=0):
    from modules import Extension as X
    n = F * h * w * cin
    dx = _nan(n + GUARD)
    rc = X.lib.mvx_conv2d_dgrad_frames(_p(dz), _p(wpk_d), _p(dx), h, w, cin, cout, flags, None, F, X.stream())
    torch.cuda.synchronize()
    if expect != 0:
        assert rc != 0 and torch.isnan(dx).all(), 'a refused call must not write'
        return None
    assert rc == 0, 'mvx_conv2d_dgrad_frames returned %d' % rc
    assert torch.isnan(dx[n:]).all() and not torch.isnan(dx[:n]).any()
    return dx[:n].view(F, h, w, cin)


def wgrad(x, dz, F, h, w, cin, cout, flags, fill=NAN, expect=0):
    from modules import Extension as X
    n = cout * cin * 9
    nbytes = X.lib.mvx_conv2d_wgrad_workspace_bytes_frames(h, w, cin, cout, F)
    assert nbytes % 4 == 0
    ws = _nan(max(nbytes // 4, 1) + GUARD)
    dw = _nan(n + GUARD)
    dw[:n] = fill
    rc = X.lib.mvx_conv2d_wgrad_frames(_p(x), _p(dz), _p(dw), h, w, cin, cout, flags, _p(ws), nbytes, F, X.stream())
    torch.cuda.synchronize()
    assert torch.isnan(dw[n:]).all() and torch.isnan(ws[max(nbytes // 4, 1):]).all()
    if expect != 0:
        assert rc != 0 and torch.isnan(dw).all() and torch.isnan(ws).all(), 'a refused call must not write'
        return None
    assert rc == 0, 'mvx_conv2d_wgrad_frames returned %d' % rc
    assert not torch.isnan(dw[:n]).any()
    return dw[:n].view(cout, cin, 3, 3)


def mean_inv_ref(y64):
    """(F, c, h, w) float64 -> (F, 2, c): per frame and channel over the sites, biased variance"""
    mean = y64.mean((2, 3))
    var = ((y64 - mean[:, :, None, None]) ** 2).mean((2, 3))
    return torch.stack([mean, 1.0 / torch.sqrt(var + EPS)], 1)


def check_forward(tag, y, mi, y_ref):
    e_y = rel(_nchw(y), y_ref)
    ref_mi = mean_inv_ref(y_ref)
    e_m = max(rel(mi[f, 0], ref_mi[f, 0]) for f in range(y.shape[0]))
    e_i = max(rel(mi[f, 1], ref_mi[f, 1]) for f in range(y.shape[0]))
    print('%s: y %.3e, mean %.3e, inverse deviation %.3e' % (tag, e_y, e_m, e_i))
    assert e_y < BOUND and e_m < BOUND_MI and e_i < BOUND_MI, tag


# ---- stride 1 -----------------------------------------------------------------------------------------------------------------
STRIDE1 = {'ragged': (3, 21, 37, 64, 128, True), 'onetile': (1, 8, 16, 32, 64, False), 'onesite': (1, 1, 1, 64, 64, True)}


@pytest.mark.parametrize('name', list(STRIDE1))
def test_stride1(name):
    from modules import _hip
    F, h, w, cin, cout, has_backward = STRIDE1[name]
    if name == 'onetile':
        assert (h, w) == (8, 16)                        # TH x TW of csrc/conv_geom.h
    g = torch.Generator().manual_seed(17 + h)
    scale = torch.tensor([1.0, 3.0, 0.3])[:F, None, None, None]
    x = torch.randn((F, h, w, cin), generator=g) * scale
    wt = torch.randn((cout, cin, 3, 3), generator=g) * 0.05
    b = torch.randn((cout,), generator=g) * 0.1
    dz = torch.randn((F, h, w, cout), generator=g) * scale
    xr = _nchw(x).requires_grad_(True)
    wr = wt.double().requires_grad_(True)
    pre = Fn.conv2d(xr, wr, b.double(), stride=1, padding=1)
    pre.backward(_nchw(dz))
    xd, dzd, wd, bd = _dev(x), _dev(dz), wt.to(DEV), _dev(b)
    y, mi = forward(xd, _hip.conv3d_pack(wd, False), bd, F, h, w, cin, cout, 0)
    check_forward(name, y, mi, torch.relu(pre.detach()))
    if not has_backward:
        # the model's 32-channel input layers have no backward on these kernels: the input gradient produces cin in blocks of
        # 64, the weight gradient reads it in blocks of 64; both refuse with the size error and write nothing
        assert cin % 64
        dgrad(dzd, _hip.conv3d_pack(wd, True), F, h, w, cin, cout, 0, expect=-1)
        wgrad(xd, dzd, F, h, w, cin, cout, 0, expect=-1)
        return
    dx = dgrad(dzd, _hip.conv3d_pack(wd, True), F, h, w, cin, cout, 0)
    e_dx = rel(_nchw(dx), xr.grad)
    print('%s: dx %.3e' % (name, e_dx))
    assert e_dx < BOUND
    dw = wgrad(xd, dzd, F, h, w, cin, cout, 0)
    dw_acc = wgrad(xd, dzd, F, h, w, cin, cout, _hip.FLAG_ACCUMULATE, fill=0.5)
    e_dw, e_acc = rel(dw, wr.grad), rel(dw_acc.double() - 0.5, wr.grad)
    print('%s: dw %.3e, accumulated into 0.5: %.3e' % (name, e_dw, e_acc))
    assert e_dw < BOUND and e_acc < BOUND


# ---- stride 2 as a 2x2 window on the space-to-depth image -------------------------------------------------------------------------
TAPS2 = {'taps2p2': (2, 9, 17, 2, 32, 128), 'taps2k16': (2, 9, 17, 1, 16, 64)}


@pytest.mark.parametrize('name', list(TAPS2))
def test_stride2_chain(name):
    from modules import _hip
    from modules import Extension as X
    from modules import rpn_frames as rf
    F, h, w, P, C, cout = TAPS2[name]
    cin0, cin = P * C, 4 * P * C
    if name == 'taps2k16':
        assert (cin // 4) % K_CHUNK != 0                # the parity block is no whole K chunk: structural zeros are executed
    else:
        assert (cin // 4) % K_CHUNK == 0 and P == 2
    H, W = 2 * h, 2 * w
    g = torch.Generator().manual_seed(29 + C)
    scale = torch.tensor([1.0, 3.0])[:, None, None, None, None]
    img = torch.randn((F, P, H, W, C), generator=g) * scale          # [F*planes][H][W][C]
    wt = torch.randn((cout, cin0, 3, 3), generator=g) * 0.05
    b = torch.randn((cout,), generator=g) * 0.1
    dz = torch.randn((F, h, w, cout), generator=g)
    # the reference's image: channel c * planes + d
    xr = img.double().permute(0, 4, 1, 2, 3).reshape(F, cin0, H, W).contiguous().requires_grad_(True)
    wr = wt.double().requires_grad_(True)
    pre = Fn.conv2d(xr, wr, b.double(), stride=2, padding=1)
    assert pre.shape == (F, cout, h, w)
    pre.backward(_nchw(dz))
    imgd, dzd, wd, bd = _dev(img), _dev(dz), wt.to(DEV), _dev(b)
    s2d = _nan(F * h * w * cin + GUARD)
    assert X.lib.mvx_space_to_depth_frames(_p(imgd), _p(s2d), F, P, H, W, C, 0, X.stream()) == 0
    w2 = rf._s2d_weight(wd, P).contiguous()
    assert w2.shape == (cout, cin, 3, 3)
    y, mi = forward(s2d, _hip.conv3d_pack(w2, False), bd, F, h, w, cin, cout, rf.TAPS2)
    assert torch.isnan(s2d[F * h * w * cin:]).all()
    check_forward(name, y, mi, torch.relu(pre.detach()))
    # input gradient, back through the reverse shuffle
    dx2 = dgrad(dzd, _hip.conv3d_pack(w2, True), F, h, w, cin, cout, rf.TAPS2)
    dimg = _nan(img.numel() + GUARD)
    assert X.lib.mvx_space_to_depth_frames(_p(dx2), _p(dimg), F, P, H, W, C, 1, X.stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(dimg[img.numel():]).all()
    ref_dimg = xr.grad.view(F, C, P, H, W).permute(0, 2, 3, 4, 1)
    e_dx = rel(dimg[:img.numel()].view(F, P, H, W, C), ref_dimg)
    print('%s: dx (back in the image layout) %.3e' % (name, e_dx))
    assert e_dx < BOUND
    # weight gradient: structural zeros exact, the rest folded back onto the 3 x 3 kernel
    _, mask, _ = rf._s2d_index(cout, cin0, P, DEV)
    zero = (mask == 0).view(1, cin, 3, 3).expand(cout, -1, -1, -1)
    assert int(zero.sum()) == cout * cin * 9 - cout * cin0 * 9
    for flags, fill in ((rf.TAPS2, NAN), (rf.TAPS2 | _hip.FLAG_ACCUMULATE, 0.5)):
        dw2 = wgrad(s2d[:F * h * w * cin], dzd, F, h, w, cin, cout, flags, fill=fill)
        if flags & _hip.FLAG_ACCUMULATE:
            assert (dw2[zero] == 0.5).all(), 'a structural zero of the weight gradient changed the buffer it is added to'
            dw2 = dw2 - 0.5
        else:
            assert (dw2[zero] == 0).all(), 'structural zeros of the weight gradient are not exact zeros'
        folded = torch.zeros((cout, cin0, 3, 3), device=DEV)
        with rf.grad_targets({id(wd): folded}):
            rf._s2d_weight_grad(dw2.contiguous(), wd, P)
        e_dw = rel(folded, wr.grad)
        print('%s: dw folded back%s %.3e' % (name, ' (accumulated into 0.5)' if fill == 0.5 else '', e_dw))
        assert e_dw < BOUND


# ---- the persistent launch ------------------------------------------------------------------------------------------------------
_PERSISTENT = {}


def _persistent_case():
    if not _PERSISTENT:
        F, h, w, cin, cout = 4, 53, 100, 32, 256
        g = torch.Generator().manual_seed(41)
        x = torch.randn((F, h, w, cin), generator=g) * torch.tensor([1.0, 3.0, 0.3, 1.7])[:, None, None, None]
        wt = torch.randn((cout, cin, 3, 3), generator=g) * 0.05
        b = torch.randn((cout,), generator=g) * 0.1
        ref = torch.relu(Fn.conv2d(_nchw(x), wt.double(), b.double(), stride=1, padding=1))
        _PERSISTENT.update(shape=(F, h, w, cin, cout), x=x, wt=wt, b=b, ref=ref)
    return _PERSISTENT


@pytest.mark.parametrize('units', ['wide', 'narrow'])
def test_persistent_launch_finalises_in_the_launch(units):
    from modules import _hip
    from modules import Extension as X
    c = _persistent_case()
    F, h, w, cin, cout = c['shape']
    tiles = -(-h // 8) * -(-w // 16)
    n_units = tiles * F * (cout // 64)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert tiles == 49 and n_units == 784 and n_units > 3 * cus, 'the launch would not be the persistent one'
    assert n_units >= 3 * cus // 2 + 1                  # by the library's own rule these stay 64-channel units
    xd, wd, bd = _dev(c['x']), c['wt'].to(DEV), _dev(c['b'])
    wpk = _hip.conv3d_pack(wd, False)
    if units == 'wide':
        y, mi = forward(xd, wpk, bd, F, h, w, cin, cout, 0, persistent=True)
    else:
        X.check(X.lib.mvx_tuning_set(2, 1 << 60), 'mvx_tuning_set')
        try:
            y, mi = forward(xd, wpk, bd, F, h, w, cin, cout, 0, persistent=True)
        finally:
            X.check(X.lib.mvx_tuning_set(2, -1), 'mvx_tuning_set')
    check_forward('persistent, %s units (%d)' % (units, n_units * (2 if units == 'narrow' else 1)), y, mi, c['ref'])
