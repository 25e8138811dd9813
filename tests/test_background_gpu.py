"""The kernels of the CML background rewrite (csrc/activity.hip, the closed-form and tile-restricted kernels of csrc/conv3d.hip and
csrc/conv3d_split.hip), one by one against float64: tests/background_ref.py (dense torch-CPU / numpy) on the cases of
tests/background_cases.py, whose properties and sensitivity tests/test_background_host.py proves on the CPU.

Rules of this file:
  * every kernel gets its inputs from the REFERENCE, rounded to f32, never from another kernel under test;
  * whatever the header calls undefined is NaN in the input: dyhat off the flagged tiles, dz off the tiles of the restricted
    backward, x off the tiles a layer reads; every output starts as a recognisable NaN (POISON) and is followed by guard rows;
  * no tolerance comes from a kernel: they are derived (one rounding of an f64 sum; 3 u for the BatchNorm apply), the bounds
    tests/test_conv3d_gpu.py holds the dense kernels to, or four times the distance of a plain f32 evaluation from float64;
  * each measured figure is printed in front of its assertion (pytest -s)."""
import numpy as np
import pytest
import torch

import background_cases as BC
import background_ref as B

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = B.U
C = BC.C
POISON = 0x7FC0BEEF                     # a quiet NaN with a payload: what an unwritten f32 element must still hold
GUARD = 64                              # elements behind every output that must stay untouched
FLAG_RELU, FLAG_ACCUMULATE, FLAG_BG_TAPS = 1, 4, 32
NAMES = sorted(BC.CASES)
ARITH = [(False, '32-channel units'), (False, '64-channel units'), (2, '8x16 units'), (2, '16x16 units'), (3, '8x16 units'),
         (3, '16x16 units'), (4, '8x16 units'), (4, '16x16 units')]
ARITH_IDS = ['%s-%s' % ({False: 'f32', 2: 'bf16x3', 3: 'bf16x6', 4: 'fp16x3'}[a], u.split()[0]) for a, u in ARITH]


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def poisoned(*shape):
    """A POISON-filled f32 buffer of the shape plus GUARD elements -> (view of the shape, whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), POISON, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf[:n].view(*shape), buf


def untouched(t):
    """bool: the elements that still hold POISON."""
    return t.contiguous().view(torch.int32) == POISON


def guard_ok(buf):
    return bool(untouched(buf[-GUARD:]).all())


def f64(t):
    return t.detach().double().cpu().numpy()


def site_mask(flags, wi):
    return torch.from_numpy(np.ascontiguousarray(B.tile_sites(flags, wi.H, wi.W))).to(DEV)


def flat(flags):
    return dev(np.asarray(flags).reshape(flags.shape[0], -1), torch.int32)


def within(got, ref, tol, what):
    """|got - ref| <= tol everywhere (tol an array or a number); prints the largest ratio first."""
    diff = np.abs(np.asarray(got, np.float64) - ref)
    assert np.isfinite(diff).all(), what + ': not finite'
    tol = np.broadcast_to(np.asarray(tol, np.float64), diff.shape)
    ratio = float(np.where(tol > 0, diff / np.where(tol > 0, tol, 1.0), np.where(diff > 0, np.inf, 0.0)).max())
    print('  %-58s %.3g of its bound (largest error %.3g)' % (what, ratio, float(diff.max())))
    assert ratio <= 1.0, (what, ratio)


def set_units(arith, units):
    from modules import Extension as X
    if arith:
        X.check(X.lib.mvx_tuning_set(1, 0 if units.startswith('16') else 1 << 60), 'mvx_tuning_set')
    else:
        X.check(X.lib.mvx_tuning_set(2, (1 << 60) if units.startswith('32') else 0), 'mvx_tuning_set')


def reset_units():
    from modules import Extension as X
    X.check(X.lib.mvx_tuning_set(1, 768), 'mvx_tuning_set')
    X.check(X.lib.mvx_tuning_set(2, -1), 'mvx_tuning_set')


def tagged(a, valid=None):
    """Device tensor of a (NaN allowed) carrying the range tag of its valid part: what the fp16x3 kernels scale a gradient by."""
    from modules import _hip
    t = dev(a)
    return _hip.tag_amax(t, dev([float(np.nanmax(np.abs(a if valid is None else valid)))]))


def layer(name, li):
    """The f32-valued tensors of conv2 / conv3 as a namespace (see BC.layer_tensors)."""
    L, x, c_in, w, b, y, mi, x_out, c_out, ybg_out, dz, g_in = BC.layer_tensors(name, li)
    return BC.types.SimpleNamespace(L=L, x=x, c_in=c_in, w=w, b=b, y=y, mi=mi, x_out=x_out, c_out=c_out, ybg_out=ybg_out, dz=dz, g_in=g_in)


# ---- 1. mvx_conv3d_background / mvx_conv3d_background_taps_frames --------------------------------------------------------------------
@pytest.mark.parametrize('li', [0, 1], ids=['conv2', 'conv3'])
@pytest.mark.parametrize('name', NAMES)
def test_background_taps(name, li):
    from modules import _hip
    from modules import Extension as X
    wi, t = BC.wiring(name), layer(name, li)
    L, F = t.L, wi.F
    P = F * L.dout
    ref, tol = BC.table(name, li)
    w, c_in = dev(t.w), dev(t.c_in)
    bg, buf = poisoned(P * 13, C)
    X.check(X.lib.mvx_conv3d_background_taps_frames(X.ptr(w), X.ptr(c_in), L.din, L.dout, C, C, L.sd, L.pd, X.ptr(bg), F, X.stream()),
            'mvx_conv3d_background_taps_frames')
    wrapped = _hip.conv3d_background_taps(w, c_in, L.din, L.sd, L.pd, F)
    torch.cuda.synchronize()
    assert guard_ok(buf) and torch.equal(wrapped.view(torch.int32), bg.view(torch.int32))
    got = f64(bg)
    within(got[:P], ref[:P], tol[:P], 'totals')
    within(got[P:4 * P], ref[P:4 * P], tol[P:4 * P], 'depth taps')
    within(got[4 * P:], ref[4 * P:], tol[4 * P:], 'border classes')
    taps = got[P:4 * P].reshape(P, 3, C)
    for p in range(P):
        for kd in range(3):
            if not 0 <= (p % L.dout) * L.sd - L.pd + kd < L.din:
                assert (taps[p, kd] == 0).all(), (p, kd)
    # the head of the table is mvx_conv3d_background of each frame, bit for bit
    for f in range(F):
        one = _hip.conv3d_background(w, c_in[f * L.din:(f + 1) * L.din].contiguous(), L.din, L.sd, L.pd)
        assert torch.equal(one.view(torch.int32), bg[f * L.dout:(f + 1) * L.dout].view(torch.int32)), f


# ---- 2. mvx_bn_background_frames -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'linear'])
@pytest.mark.parametrize('with_pre', [True, False], ids=['bg_pre', 'bias-only'])
@pytest.mark.parametrize('name', NAMES)
def test_bn_background(name, with_pre, relu):
    from modules import _hip
    from modules import Extension as X
    wi, t = BC.wiring(name), layer(name, 0)
    L, F = t.L, wi.F
    P = F * L.dout
    pre = B.f32(BC.table(name, 0)[0][:P]) if with_pre else None
    mi = B.f32(t.mi)
    v_ref, c_ref, c_tol = BC.bn_background(pre, t.b, mi, L.dout, relu)
    pre_d, b_d, mi_d = (dev(pre) if with_pre else None), dev(t.b), dev(mi)
    (ybg, buf_y), (c, buf_c) = poisoned(P, C), poisoned(P, C)
    X.check(X.lib.mvx_bn_background_frames(X.ptr(pre_d), X.ptr(b_d), X.ptr(mi_d), L.dout, C, FLAG_RELU if relu else 0, X.ptr(ybg),
                                           X.ptr(c), F, X.stream()), 'mvx_bn_background_frames')
    wc, wy = _hip.bn_background(pre_d, b_d, mi_d, L.dout, C, relu=relu, want_y=True, F=F)
    torch.cuda.synchronize()
    assert guard_ok(buf_y) and guard_ok(buf_c)
    assert torch.equal(wc.view(torch.int32), c.view(torch.int32)) and torch.equal(wy.view(torch.int32), ybg.view(torch.int32))
    assert np.array_equal(f64(ybg), B.f32(v_ref)), 'y_bg = [ReLU](bg_pre + bias): one f32 addition'
    within(f64(c), c_ref, c_tol, 'c_out against float64')
    # the header's claim: what mvx_bn_apply writes at a site that holds y_bg, bit for bit
    for f in range(F):
        rows = slice(f * L.dout, (f + 1) * L.dout)
        applied = _hip.bn_apply(ybg[rows].contiguous(), mi_d[f].contiguous())
        assert torch.equal(applied.view(torch.int32), c[rows].view(torch.int32)), f
    if F == 1:
        (y1, _), (c1, _) = poisoned(P, C), poisoned(P, C)
        X.check(X.lib.mvx_bn_background(X.ptr(pre_d), X.ptr(b_d), X.ptr(mi_d), L.dout, C, FLAG_RELU if relu else 0, X.ptr(y1), X.ptr(c1),
                                        X.stream()), 'mvx_bn_background')
        assert torch.equal(y1.view(torch.int32), ybg.view(torch.int32)) and torch.equal(c1.view(torch.int32), c.view(torch.int32))


# ---- 3. mvx_bn_apply_tiles_frames / _read_frames -------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3], ids=['layer1', 'conv2', 'conv3'])
@pytest.mark.parametrize('name', NAMES)
def test_bn_apply_tiles(name, n):
    from modules import _hip
    from modules import Extension as X
    wi, d = BC.wiring(name), BC.dense(name)
    F, H, W = wi.F, wi.H, wi.W
    tflag = (wi.conv2.tflag_in, wi.conv2.tflag_out, wi.conv3.tflag_out)[n - 1]
    read = (wi.conv2.read_in, wi.conv3.read_in, None)[n - 1]
    y, mi, cb = B.f32(d['y%d' % n]), B.f32(d['mi%d' % n]), B.f32(d['c%d' % n])
    P = y.shape[0]
    ref, tol = BC.bn_apply(y, mi)
    on = B.tile_sites(tflag, H, W)
    y_d, mi_d, cb_d, tf_d = dev(BC.poison(y, on)), dev(mi), dev(cb), flat(tflag)          # y is NaN on the unflagged tiles
    on_d = site_mask(tflag, wi)
    out, buf = poisoned(P, H, W, C)
    X.check(X.lib.mvx_bn_apply_tiles_frames(X.ptr(y_d), X.ptr(mi_d), X.ptr(cb_d), X.ptr(tf_d), X.ptr(out), P // F, H, W, C, F,
                                            X.stream()), 'mvx_bn_apply_tiles_frames')
    torch.cuda.synchronize()
    assert guard_ok(buf) and not torch.isnan(out).any()
    dense_apply = torch.cat([_hip.bn_apply(dev(y[f * (P // F):(f + 1) * (P // F)]), mi_d[f].contiguous()) for f in range(F)])
    assert torch.equal(out[on_d].view(torch.int32), dense_apply[on_d].view(torch.int32)), 'flagged tiles = mvx_bn_apply'
    const = cb_d[:, None, None, :].expand(P, H, W, C)
    assert torch.equal(out[~on_d].view(torch.int32), const[~on_d].view(torch.int32)), 'the other tiles hold c_bg'
    got = f64(out)
    within(got[on], ref[on], tol[on], 'flagged tiles against float64')
    within(got[~on], ref[~on], tol[~on] + U * np.abs(ref[~on]), 'background tiles against float64 (c_bg rounded)')
    assert torch.equal(_hip.bn_apply_tiles(y_d, mi_d, cb_d, tf_d, F).view(torch.int32), out.view(torch.int32))
    if read is not None:
        rd = site_mask(np.asarray(read) | (np.asarray(tflag) != 0), wi)
        out_r, buf_r = poisoned(P, H, W, C)
        X.check(X.lib.mvx_bn_apply_tiles_read_frames(X.ptr(y_d), X.ptr(mi_d), X.ptr(cb_d), X.ptr(tf_d), X.ptr(flat(read)), X.ptr(out_r),
                                                     P // F, H, W, C, F, X.stream()), 'mvx_bn_apply_tiles_read_frames')
        torch.cuda.synchronize()
        assert guard_ok(buf_r)
        assert torch.equal(out_r[rd].view(torch.int32), out[rd].view(torch.int32)), 'flagged or read tiles as without read flags'
        assert bool(untouched(out_r[~rd]).all()), 'a tile that is neither flagged nor read is not written'
        into, buf_i = poisoned(P, H, W, C)
        assert _hip.bn_apply_tiles(y_d, mi_d, cb_d, tf_d, F, read=flat(read), out=into) is into
        torch.cuda.synchronize()
        assert guard_ok(buf_i) and torch.equal(into.view(torch.int32), out_r.view(torch.int32))
        print('  %s layer %d: %d of %d tiles neither flagged nor read' % (name, n, int(((np.asarray(read) == 0) & (np.asarray(tflag) == 0)).sum()),
                                                                     tflag.size))


# ---- 4. mvx_conv3d_forward_bg*_frames with MVX_FLAG_BG_TAPS --------------------------------------------------------------------------
@pytest.mark.parametrize('arith,units', ARITH, ids=ARITH_IDS)
@pytest.mark.parametrize('li', [0, 1], ids=['conv2', 'conv3'])
@pytest.mark.parametrize('name', NAMES)
def test_forward_bg_with_tap_constants(name, li, arith, units):
    from modules import _hip
    from modules import Extension as X
    wi, t = BC.wiring(name), layer(name, li)
    L, F, H, W = t.L, wi.F, wi.H, wi.W
    P = F * L.dout
    y_ref, sums_ref, mi_ref = BC.forward(name, li)
    table = dev(B.f32(BC.table(name, li)[0]))
    w, b = dev(t.w), dev(t.b)
    bg_in = _hip.Background(dev(t.c_in), dev(L.mask_in, torch.uint8), flat(L.hflag_in))
    mask_out = dev(L.mask_out, torch.uint8)
    read = B.tile_sites(L.read_in, H, W)
    x_clean, x_nan = dev(t.x), dev(BC.poison(t.x, read))
    tol = BC.CONV_TOL[arith]
    try:
        set_units(arith, units)
        wpk = _hip.conv3d_pack(w, False, split=arith)
        out, stats = _hip.conv3d_forward_bg(x_clean, wpk, b, C, L.sd, L.pd, bg_in, mask_out, table, split=arith, F=F, bg_taps=True)
        out_n, mi = _hip.conv3d_forward_bg(x_nan, wpk, b, C, L.sd, L.pd, bg_in, mask_out, table, finalize_eps=B.EPS, split=arith, F=F,
                                           bg_taps=True)
        torch.cuda.synchronize()
        if F == 1:                                      # the single-frame entry points: bit for bit
            one, st1 = torch.empty_like(out), torch.zeros((32, 2, C), dtype=torch.float64, device=DEV)
            a = (X.ptr(x_nan), X.ptr(wpk), X.ptr(b), X.ptr(one), X.ptr(st1), L.din, L.dout, H, W, C, C, L.sd, L.pd,
                 FLAG_RELU | FLAG_BG_TAPS | _hip.split_flags(arith), X.ptr(bg_in.hflag), X.ptr(mask_out), X.ptr(table), 1)
            if arith:
                X.check(X.lib.mvx_conv3d_forward_bg_split(*a, X.stream()), 'mvx_conv3d_forward_bg_split')
            else:
                X.check(X.lib.mvx_conv3d_forward_bg(*a, None, None, 0.0, 0.0, None, None, X.stream()), 'mvx_conv3d_forward_bg')
            torch.cuda.synchronize()
            assert torch.equal(one.view(torch.int32), out.view(torch.int32))
            assert torch.allclose(st1.sum(0), stats.view(-1, 2, C).sum(0), rtol=1e-12, atol=0)
        err = B.rel_err(f64(out), y_ref)
        print('  %s conv%d %s %s: %.3g from float64 (bound %.3g)' % (name, li + 2, ARITH_IDS[ARITH.index((arith, units))], units, err, tol))
        if err >= tol:
            # the project's rule for a split arithmetic: at most twice the DENSE kernel's distance on the same input, plus 5e-7
            dn = torch.cat([_hip.conv3d_forward(x_clean[f * L.din:(f + 1) * L.din], wpk, b, C, L.sd, L.pd, split=arith)[0] for f in range(F)])
            dense_err = B.rel_err(f64(dn), y_ref)
            print('    dense kernel on the same input: %.3g' % dense_err)
            assert err < 2 * dense_err + 5e-7
    finally:
        reset_units()
    assert not torch.isnan(out_n).any() and torch.equal(out_n.view(torch.int32), out.view(torch.int32)), 'tiles off the read flags are not read'
    st = f64(stats.view(F, -1, 2, C).sum(1))
    np.testing.assert_allclose(st[:, 0], sums_ref[:, 0], rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(st[:, 1], sums_ref[:, 1], rtol=1e-5, atol=1e-3)
    within(f64(mi), mi_ref, BC.mean_inv_bound(y_ref, mi_ref, tol * float(np.abs(y_ref).max())), 'mean and inverse std')
    # background sites: bit-equal to one another and to mvx_bn_background's y_bg
    _, ybg = _hip.bn_background(table[:P], b, mi, L.dout, C, want_y=True, F=F)
    bgs = mask_out == 0
    const = ybg[:, None, None, :].expand(P, H, W, C)
    assert bool(bgs.any()) and torch.equal(out[bgs].view(torch.int32), const[bgs].view(torch.int32))


# ---- 5. mvx_plane_tap_sums ---------------------------------------------------------------------------------------------------------
def run_tap_sums(dz, flags=None, inactive=None):
    from modules import _hip
    from modules import Extension as X
    P, H, W, Cn = dz.shape
    T, buf = poisoned(P, 9, Cn)
    ws = _hip.workspace(X.lib.mvx_plane_tap_sums_workspace_bytes(P, Cn), dz.device, 'test_tap_sums')
    X.check(X.lib.mvx_plane_tap_sums(X.ptr(dz), P, H, W, Cn, X.ptr(flags), X.ptr(inactive), X.ptr(T), X.ptr(ws), ws.numel(), X.stream()),
            'mvx_plane_tap_sums')
    wrapped = _hip.plane_tap_sums(dz, flags, inactive)
    torch.cuda.synchronize()
    assert guard_ok(buf) and not torch.isnan(T).any()
    return f64(T), f64(wrapped)


@pytest.mark.parametrize('name', NAMES)
def test_plane_tap_sums(name):
    wi = BC.wiring(name)
    L = wi.conv2
    on = B.tile_sites(L.bflag_out, wi.H, wi.W)
    # dyadic gradient: every partial sum is exact, so both forms equal the reference; the ragged planes of 'model' pin each of the
    # nine border kinds
    dz = BC.dyadic_dz(name, 0)
    ref = B.tap_sums(dz)
    inactive = B.region_sums(dz, ~on)
    assert np.array_equal(B.f32(ref), ref) and np.array_equal(B.f32(inactive), inactive)
    for label, args in (('dense', (dev(dz),)), ('tiles', (dev(BC.poison(dz, on)), flat(L.bflag_out), dev(inactive)))):
        got, wrapped = run_tap_sums(*args)
        assert np.array_equal(got, ref) and np.array_equal(wrapped, ref), label
    # the chain's gradient: four times the distance of an f32 numpy evaluation of the same sums from float64, plus one rounding
    dz = B.f32(BC.dense(name)['dz2'])
    ref = B.tap_sums(dz)
    tol = 4 * float(np.abs(B.tap_sums(dz.astype(np.float32)) - ref).max()) + U * np.abs(ref)
    got, wrapped = run_tap_sums(dev(BC.poison(dz, on)), flat(L.bflag_out), dev(B.f32(B.region_sums(dz, ~on))))
    within(got, ref, tol, 'tile form on the chain gradient')
    assert np.array_equal(got, wrapped)


# ---- 6. mvx_conv3d_input_grad_sums_frames --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('li', [0, 1], ids=['stride1', 'stride2'])
@pytest.mark.parametrize('name', NAMES)
def test_input_grad_sums(name, li):
    from modules import _hip
    from modules import Extension as X
    wi, inp = BC.wiring(name), BC.inputs(name)
    L, F = wi.layers[li], wi.F
    T, ref, tol = BC.input_grad_sums(name, li)
    assert np.array_equal(B.f32(T), T)
    w, T_d = dev(inp.w[li]), dev(T)
    A, buf = poisoned(F * L.din, C)
    X.check(X.lib.mvx_conv3d_input_grad_sums_frames(X.ptr(w), X.ptr(T_d), L.din, L.dout, C, C, L.sd, L.pd, X.ptr(A), F, X.stream()),
            'mvx_conv3d_input_grad_sums_frames')
    wrapped = _hip.conv3d_input_grad_sums(w, T_d, L.din, L.sd, L.pd, F)
    torch.cuda.synchronize()
    assert guard_ok(buf) and torch.equal(wrapped.view(torch.int32), A.view(torch.int32))
    within(f64(A), ref, tol, 'plane sums of the dense input gradient')
    if F == 1:
        A1, _ = poisoned(L.din, C)
        X.check(X.lib.mvx_conv3d_input_grad_sums(X.ptr(w), X.ptr(T_d), L.din, L.dout, C, C, L.sd, L.pd, X.ptr(A1), X.stream()),
                'mvx_conv3d_input_grad_sums')
        assert torch.equal(A1.view(torch.int32), A.view(torch.int32))


# ---- 7. mvx_conv3d_dgrad_tiles*_frames -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('arith,units', ARITH, ids=ARITH_IDS)
@pytest.mark.parametrize('li', [0, 1], ids=['conv2', 'conv3'])
@pytest.mark.parametrize('name', NAMES)
def test_dgrad_tiles(name, li, arith, units):
    from modules import _hip
    from modules import Extension as X
    wi, t = BC.wiring(name), layer(name, li)
    L, F, H, W = t.L, wi.F, wi.H, wi.W
    ref = BC.dgrad(name, li)
    valid = B.tile_sites(L.bflag_out, H, W) if L.bflag_out is not None else np.ones(t.dz.shape[:3], bool)
    dz_nan = tagged(BC.poison(t.dz, valid), t.dz)                   # dz is undefined off the tiles of the layer's restricted backward
    dz_clean = _hip.tag_amax(dev(t.dz), _hip.amax_of(dz_nan))
    flags = flat(L.bflag_in)
    on = B.tile_sites(L.bflag_in, H, W)
    on_d = site_mask(L.bflag_in, wi)
    w = dev(t.w)
    sf = _hip.split_flags(arith)
    try:
        set_units(arith, units)
        wpd = _hip.conv3d_pack(w, True, split=arith)

        def run(frames_entry):
            dx, buf = poisoned(F * L.din, H, W, C)
            _hip.bind_amax(arith, dz_nan)
            a = (X.ptr(dz_nan), X.ptr(wpd), X.ptr(dx), L.din, L.dout, H, W, C, C, L.sd, L.pd)
            if arith and frames_entry:
                rc = X.lib.mvx_conv3d_dgrad_tiles_split_frames(*a, sf, X.ptr(flags), None, F, X.stream())
            elif arith:
                rc = X.lib.mvx_conv3d_dgrad_tiles_split(*a, sf, X.ptr(flags), X.stream())
            elif frames_entry:
                rc = X.lib.mvx_conv3d_dgrad_tiles_frames(*a, X.ptr(flags), None, None, F, X.stream())
            else:
                rc = X.lib.mvx_conv3d_dgrad_tiles(*a, X.ptr(flags), None, None, X.stream())
            X.check(rc, 'mvx_conv3d_dgrad_tiles')
            torch.cuda.synchronize()
            assert guard_ok(buf)
            return dx
        dx = run(True)
        wrapped = _hip.conv3d_dgrad_tiles(dz_nan, wpd, L.din, C, L.sd, L.pd, flags, arith, F)
        dense = torch.cat([_hip.conv3d_dgrad(_hip.tag_amax(dz_clean[f * L.dout:(f + 1) * L.dout], _hip.amax_of(dz_nan)), wpd, L.din, C,
                                             L.sd, L.pd, split=arith) for f in range(F)])
        single = run(False) if F == 1 else None
        torch.cuda.synchronize()
    finally:
        reset_units()
    assert not torch.isnan(dx[on_d]).any(), 'a flagged tile read dz where it is undefined'
    err = float(np.abs(f64(dx)[on] - ref[on]).max() / np.abs(ref[on]).max())
    print('  %s conv%d %s: %.3g from float64 on the flagged tiles (bound %.3g)' % (name, li + 2, ARITH_IDS[ARITH.index((arith, units))], err,
                                                                               BC.CONV_TOL[arith]))
    assert err < BC.CONV_TOL[arith]
    assert torch.equal(dx[on_d].view(torch.int32), dense[on_d].view(torch.int32)), 'flagged tiles = mvx_conv3d_dgrad on the whole dz'
    assert torch.equal(dx[on_d].view(torch.int32), wrapped[on_d].view(torch.int32))
    if single is not None:
        assert torch.equal(dx[on_d].view(torch.int32), single[on_d].view(torch.int32))
    # an unflagged tile whose vertical partner (tile rows 2k, 2k + 1) is unflagged too is not written.  (The partner of a FLAGGED
    # tile is written by the 16 x 16 units of the split gather: nothing is asserted about it.)
    fl = np.asarray(L.bflag_in) != 0
    pair = fl.copy()
    pair[:, 0:fl.shape[1] - fl.shape[1] % 2:2] |= fl[:, 1::2]
    pair[:, 1::2] |= fl[:, 0:fl.shape[1] - fl.shape[1] % 2:2]
    alone = site_mask(~pair, wi)
    print('  %d tiles off the flags and off their partners' % int((~pair).sum()))
    assert bool(untouched(dx[alone]).all()), 'tiles off the flags (and off their partners) keep the sentinel'


# ---- 8. mvx_conv3d_wgrad_bg_frames ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('arith', [False, 2, 3, 4], ids=['f32', 'bf16x3', 'bf16x6', 'fp16x3'])
@pytest.mark.parametrize('li', [0, 1], ids=['conv2', 'conv3'])
@pytest.mark.parametrize('name', NAMES)
def test_wgrad_bg(name, li, arith):
    from modules import _hip
    from modules import Extension as X
    wi, t = BC.wiring(name), layer(name, li)
    L, F, H, W = t.L, wi.F, wi.H, wi.W
    ref = BC.wgrad(name, li)
    valid = B.tile_sites(L.bflag_out, H, W) if L.bflag_out is not None else np.ones(t.dz.shape[:3], bool)
    x = dev(BC.poison(t.x, B.tile_sites(L.read_in, H, W)))          # x is not written off the tiles the layer reads
    dz = tagged(BC.poison(t.dz, valid), t.dz)
    T = dev(B.f32(B.tap_sums(t.dz)))
    bg_in = _hip.Background(dev(t.c_in), None, flat(L.hflag_in))
    dw = _hip.conv3d_wgrad_bg(x, dz, L.sd, L.pd, bg_in, T, split=arith, F=F)
    start = B.f32(np.random.default_rng(5).standard_normal(ref.shape) * float(np.abs(ref).max()) / 4)
    acc = dev(start)
    assert _hip.conv3d_wgrad_bg(x, dz, L.sd, L.pd, bg_in, T, accumulate_into=acc, split=arith, F=F) is None
    torch.cuda.synchronize()
    assert not torch.isnan(dw).any(), 'the weight gradient read x or dz where they are undefined'
    err = B.rel_err(f64(dw), ref)
    print('  %s conv%d %s: %.3g from float64 (bound %.3g)' % (name, li + 2, arith or 'f32', err, BC.CONV_TOL[arith]))
    assert err < BC.CONV_TOL[arith]
    # accumulate_into adds exactly once.  The kernel adds the gathered part s and then the closed-form part r to the start, the
    # plain call forms s + r: (start + s) + r against start + (s + r), three roundings of sums no larger than |start| + |s| + |r|
    # with |s| <= |dw| + |r| and |r| <= |c_in| (x) |T| (the two parts cancel, so |dw| alone does not bound them)
    big = np.abs(start) + np.abs(f64(dw)) + 2 * BC.rank_one(t.c_in, B.f32(B.tap_sums(t.dz)), L, F)
    within(f64(acc), start + f64(dw), 3 * U * big, 'accumulated onto a non-zero start')
    if F == 1:
        one = torch.empty_like(dw)
        nbytes = X.lib.mvx_conv3d_wgrad_bg_workspace_bytes(L.dout, H, W, C, C)
        ws = _hip.workspace(nbytes, x.device, 'test_wgrad_bg')
        _hip.bind_amax(arith, None, dz)
        X.check(X.lib.mvx_conv3d_wgrad_bg(X.ptr(x), X.ptr(dz), X.ptr(one), L.din, L.dout, H, W, C, C, L.sd, L.pd, _hip.split_flags(arith, True),
                                          X.ptr(bg_in.hflag), X.ptr(bg_in.c), X.ptr(T), X.ptr(ws), ws.numel(), X.stream()), 'mvx_conv3d_wgrad_bg')
        torch.cuda.synchronize()
        assert torch.equal(one.view(torch.int32), dw.view(torch.int32))


# ---- 9. mvx_bn_relu_backward_tiles_frames ----------------------------------------------------------------------------------------------
def bn_backward_case(which):
    if which == 'alone':
        bc = BC.bn_case()
        return bc.dyhat, bc.y, bc.mi, bc.c, bc.ybg, bc.flags, bc.F, bc.ref
    name, li = which
    wi, t = BC.wiring(name), BC.dense(name)
    n = li + 2
    ref = BC.bn_backward(name, li)
    return (B.f32(t['g%d' % n]), B.f32(t['y%d' % n]), B.f32(t['mi%d' % n]), B.f32(t['c%d' % n]), B.f32(t['ybg%d' % n]), ref['flags'],
            wi.F, ref)


@pytest.mark.parametrize('which', ['alone', ('model', -1), ('model', 0), ('wide', -1), ('wide', 0)], ids=str)
def test_bn_relu_backward_tiles(which):
    from modules import _hip
    from modules import Extension as X
    dyhat, y, mi, c, ybg, flags, F, ref = bn_backward_case(which)
    P, H, W, Cn = y.shape
    on = ~ref['off']
    on_d = torch.from_numpy(np.ascontiguousarray(on)).to(DEV)
    print('  %s: plain f32 evaluation, relative to the largest element: %s' % (which, ref['f32']))
    g_d, y_d, mi_d, c_d, ybg_d = dev(BC.poison(dyhat, on)), dev(y), dev(mi), dev(c), dev(ybg)
    A_d, fl_d = dev(B.f32(ref['A'])), flat(flags)
    ws = _hip.workspace(X.lib.mvx_bn_relu_backward_tiles_workspace_bytes_frames(P // F, H, W, Cn, F), g_d.device, 'test_bn_tiles')

    def run(db, flag_bits):
        (dz, buf), (inact, buf_i) = poisoned(P, H, W, Cn), poisoned(P, Cn)
        amax = torch.full((1,), -1.0, device=DEV)
        X.check(X.lib.mvx_bn_relu_backward_tiles_frames(X.ptr(g_d), X.ptr(y_d), X.ptr(mi_d), X.ptr(c_d), X.ptr(ybg_d), X.ptr(A_d), X.ptr(fl_d),
                                                        P // F, H, W, Cn, X.ptr(dz), X.ptr(db), X.ptr(inact), X.ptr(amax), flag_bits,
                                                        X.ptr(ws), ws.numel(), F, X.stream()), 'mvx_bn_relu_backward_tiles_frames')
        torch.cuda.synchronize()
        assert guard_ok(buf) and guard_ok(buf_i)
        return dz, inact, amax
    db, buf_db = poisoned(Cn)
    dz, inact, amax = run(db, 0)
    assert guard_ok(buf_db)
    assert not torch.isnan(dz[on_d]).any(), 'a flagged tile read dyhat where it is undefined'
    assert bool(untouched(dz[~on_d]).all()), 'dz is written on the flagged tiles only'
    within(f64(dz)[on], ref['dz'][on], ref['tol_dz'], 'dz on the flagged tiles')
    within(f64(db), ref['dbias'], ref['tol_dbias'], 'dbias')
    within(f64(inact), ref['inact'], ref['tol_inact'], 'sums of dz over the other tiles')
    assert float(amax) == float(dz[on_d].abs().max()), 'dz_amax = max |dz| over the written tiles'
    # MVX_FLAG_ACCUMULATE onto a non-zero start
    start = B.f32(np.random.default_rng(3).standard_normal(Cn) * float(np.abs(ref['dbias']).max()) / 4)
    db_acc = dev(start)
    dz2, inact2, _ = run(db_acc, FLAG_ACCUMULATE)
    within(f64(db_acc), start + ref['dbias'], ref['tol_dbias'] + U * np.abs(start + ref['dbias']), 'dbias accumulated onto a non-zero start')
    assert torch.equal(dz2[on_d].view(torch.int32), dz[on_d].view(torch.int32))
    # frames without a flagged tile (the empty frame of layer 1): the "other tiles" are the whole plane
    empty = [p for p in range(P) if not np.asarray(flags)[p].any()]
    if which == ('model', -1):
        assert len(empty) == P // F
    if empty:
        within(f64(inact)[empty], ref['plane'][empty], ref['tol_inact'], 'planes without a flagged tile: the dense plane sums')
    # the wrapper
    bg = _hip.Background(c_d, None, None, y_bg=ybg_d, bflag=fl_d)
    wdz, wdb, winact = _hip.bn_relu_backward_tiles(g_d, y_d, mi_d, bg, A_d, want_inactive_sums=True, F=F)
    torch.cuda.synchronize()
    assert torch.equal(wdz[on_d].view(torch.int32), dz[on_d].view(torch.int32))
    assert float(_hip.amax_of(wdz)) == float(amax)
    within(f64(wdb), ref['dbias'], ref['tol_dbias'], 'dbias (wrapper)')
    within(f64(winact), ref['inact'], ref['tol_inact'], 'inactive sums (wrapper)')
    if F == 1:
        (dz1, _), (in1, _), (db1, _) = poisoned(P, H, W, Cn), poisoned(P, Cn), poisoned(Cn)
        X.check(X.lib.mvx_bn_relu_backward_tiles(X.ptr(g_d), X.ptr(y_d), X.ptr(mi_d), X.ptr(c_d), X.ptr(ybg_d), X.ptr(A_d), X.ptr(fl_d), P, H, W,
                                                 Cn, X.ptr(dz1), X.ptr(db1), X.ptr(in1), 0, X.ptr(ws), ws.numel(), X.stream()),
                'mvx_bn_relu_backward_tiles')
        torch.cuda.synchronize()
        assert torch.equal(dz1[on_d].view(torch.int32), dz[on_d].view(torch.int32)) and bool(untouched(dz1[~on_d]).all())
        within(f64(db1), ref['dbias'], ref['tol_dbias'], 'dbias (single-frame entry)')
        within(f64(in1), ref['inact'], ref['tol_inact'], 'inactive sums (single-frame entry)')


# ---- 10. the restricted backward composed: every kernel fed by the previous one ------------------------------------------------------
@pytest.mark.parametrize('arith', [False, 2, 3, 4], ids=['f32', 'bf16x3', 'bf16x6', 'fp16x3'])
def test_restricted_backward_composed(arith):
    """frames.cml_backward's order of calls through the _hip wrappers on 'model' (four frames, one empty), from the upstream
    gradient of x3 down to dz1.  Bound of each result: the SUM of the relative bounds of the kernels on its path (each relative
    to the largest element of what that kernel produces): BatchNorm backward of conv3 -> tap sums / weight gradient / input
    gradient / plane sums -> tile-restricted BatchNorm backward of conv2 -> the same again -> that of layer 1."""
    from modules import _hip
    from modules import Extension as X
    import sparse_first_cases as K
    name = 'model'
    wi, d, inp = BC.wiring(name), BC.dense(name), BC.inputs(name)
    F, H, W = wi.F, wi.H, wi.W
    L2, L3 = wi.conv2, wi.conv3
    desc = X.FramesDesc.make(K.voxels('model', F)[1], [0] * (F + 1), 1)

    def up(key, read=None):
        a = B.f32(d[key])
        return dev(a if read is None else BC.poison(a, B.tile_sites(read, H, W)))
    x1, x2 = up('x1', L2.read_in), up('x2', L3.read_in)
    y1, y2, y3 = up('y1'), up('y2'), up('y3')
    mi1, mi2, mi3 = up('mi1'), up('mi2'), up('mi3')
    c1, c2, ybg1, ybg2 = up('c1'), up('c2'), up('ybg1'), up('ybg2')
    w2, w3 = dev(inp.w2), dev(inp.w3)
    db1, db2, db3 = (torch.zeros((C,), device=DEV) for _ in range(3))
    bflag2, tflag1 = flat(L2.bflag_out), flat(L2.bflag_in)
    wpd2, wpd3 = _hip.conv3d_pack(w2, True, split=arith), _hip.conv3d_pack(w3, True, split=arith)
    # conv3: dense gradient in, restricted gradient and closed-form plane sums out
    dz3, _ = _hip.bn_relu_backward(up('g3'), y3, mi3, 1.0, dbias_out=db3, desc=desc, kind=X.ROWS_GRID)
    T3 = _hip.plane_tap_sums(dz3)
    dw3 = _hip.conv3d_wgrad_bg(x2, dz3, L3.sd, L3.pd, _hip.Background(c2, None, flat(L3.hflag_in)), T3, split=arith, F=F)
    g2 = _hip.conv3d_dgrad_tiles(dz3, wpd3, L3.din, C, L3.sd, L3.pd, bflag2, arith, F)
    A2 = _hip.conv3d_input_grad_sums(w3, T3, L3.din, L3.sd, L3.pd, F)
    # conv2
    dz2, _, inact2 = _hip.bn_relu_backward_tiles(g2, y2, mi2, _hip.Background(c2, None, None, y_bg=ybg2, bflag=bflag2), A2, dbias_out=db2,
                                                 want_inactive_sums=True, F=F)
    T2 = _hip.plane_tap_sums(dz2, bflag2, inact2)
    dw2 = _hip.conv3d_wgrad_bg(x1, dz2, L2.sd, L2.pd, _hip.Background(c1, None, flat(L2.hflag_in)), T2, split=arith, F=F)
    g1 = _hip.conv3d_dgrad_tiles(dz2, wpd2, L2.din, C, L2.sd, L2.pd, tflag1, arith, F)
    A1 = _hip.conv3d_input_grad_sums(w2, T2, L2.din, L2.sd, L2.pd, F)
    # layer 1
    dz1, _ = _hip.bn_relu_backward_tiles(g1, y1, mi1, _hip.Background(c1, None, None, y_bg=ybg1, bflag=tflag1), A1, dbias_out=db1, F=F)
    torch.cuda.synchronize()

    def rel(ref, key, what):
        return ref['tol_' + key] / float(np.abs(ref[what]).max())
    bn3, bn2, bn1 = BC.bn_backward_dense(name), BC.bn_backward(name, 0), BC.bn_backward(name, -1)
    conv = BC.CONV_TOL[arith]
    sums = 4 * U                                           # tap sums and plane sums: f64 accumulation, rounded once, read once
    to_dz3 = rel(bn3, 'dz', 'dz')
    to_dz2 = to_dz3 + conv + sums + rel(bn2, 'dz', 'dz')
    to_dz1 = to_dz2 + conv + sums + rel(bn1, 'dz', 'dz')
    on1 = B.tile_sites(L2.bflag_in, H, W)
    checks = (('db3', f64(db3), d['db3'], rel(bn3, 'dbias', 'dbias')), ('dw3', f64(dw3), d['dw3'], to_dz3 + sums + conv),
              ('db2', f64(db2), d['db2'], to_dz3 + conv + sums + rel(bn2, 'dbias', 'dbias')), ('dw2', f64(dw2), d['dw2'], to_dz2 + sums + conv),
              ('dz1 on its tiles', f64(dz1)[on1], d['dz1'][on1], to_dz1))
    errs = [(what, float(np.abs(got - ref).max() / np.abs(ref).max()), bound) for what, got, ref, bound in checks]
    for what, err, bound in errs:
        print('  %-18s %.3g from float64 (sum of the kernels\' bounds %.3g)' % (what, err, bound))
    for what, err, bound in errs:
        assert err <= bound, (what, err, bound)
