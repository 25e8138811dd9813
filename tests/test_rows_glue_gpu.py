"""The voxel-row glue kernels -- csrc/vfe.hip and the row half of csrc/fusion.hip -- one by one against the float64 host reference
tests/rows_ref.py, on dense rows, compact rows, and compact frame sets with empty frames (first, middle, last, consecutive).

Kernels that move data or do one or two f32 operations per element run on DYADIC inputs: values, means and gradients are
multiples of 1/16 with magnitude <= 8 and 1/sqrt(var + eps) is a power of two, so (y - m) * inv, every maximum and every
gradient or padded-row sum is exact in f32 (sums stay far below 2^24 units of 1/16) and the float64 reference rounds back
exactly: those comparisons are array_equal, argmax included, with many exact ties (30 % of the elements share one value, a
voxel's padded row ties with its largest real row).  One random-input variant per arithmetic kernel uses a derived bound."""
import functools

import numpy as np
import pytest
import torch

import rows_ref as R

gpu = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24                  # unit roundoff of f32
GUARD = 3                       # rows behind every output that must stay untouched
T_SET = 35
# 16 frames = MVX_MAX_FRAMES of the ABI; frames 0, 7, 8 and 15 are empty
VOX_OFF_A = [0, 250, 250, 590]
VOX_OFF_B = [0, 0, 40, 75, 130, 131, 200, 260, 260, 260, 300, 371, 440, 500, 555, 590, 590]


def _vcnt(rng, V, T):
    """Real rows per voxel: 0, 1, T-1 and T well represented (at least five voxels each of 0, 1 and T), small random counts
    otherwise (a few thousand rows in all); the first and the last voxel are full."""
    kind = rng.random(V)
    c = rng.integers(2, 12, V)
    c[kind < 0.10] = 0
    c[(kind >= 0.10) & (kind < 0.25)] = 1
    c[(kind >= 0.25) & (kind < 0.32)] = T - 1
    c[(kind >= 0.32) & (kind < 0.40)] = T
    c[1:6], c[6:11], c[11:16] = 0, 1, T
    c[0] = c[-1] = T
    return c


@functools.lru_cache(None)
def layout(name):
    """V is chosen so that the thread count of the form that runs (V * C scalar, V * C / 4 float4) is no multiple of 256: the
    last workgroup is partly filled."""
    rng = np.random.default_rng(sorted(('dense', 'compact', 'setA', 'setB', 'map1300')).index(name))
    if name == 'dense':
        return R.Layout(5, 37)
    if name == 'compact':
        return R.Layout(35, 300, _vcnt(rng, 300, 35))
    if name == 'map1300':                                   # 1 300 dense rows for the bookkeeping kernels
        return R.Layout(5, 260, rng.integers(0, 6, 260))
    return R.Layout(T_SET, 590, _vcnt(rng, 590, T_SET), VOX_OFF_A if name == 'setA' else VOX_OFF_B)


def as_compact(L):
    """The dense layout seen by the bookkeeping kernels: every row real."""
    return L if L.compact else R.Layout(L.T, L.V, np.full((L.V,), L.T))


class DevRows:
    """What _hip._rows_args and the compact-input wrappers read of a CompactRows / frames.FrameSet."""

    def __init__(self, L, rows_sel=None):
        from modules import Extension as X
        self.voff = torch.tensor(L.voff, dtype=torch.int32, device=DEV)
        self.vcnt = torch.tensor(L.vcnt, dtype=torch.int32, device=DEV)
        self.n_real, self.V, self.T, self.rows = L.n_real, L.V, L.T, L.rows
        self.desc = X.FramesDesc.make(L.vox_off, L.real_off, L.T) if L.F > 1 else None
        self.rows_sel = None if rows_sel is None else torch.tensor(rows_sel, dtype=torch.int32, device=DEV)


def dev_rows(L, rows_sel=None):
    return DevRows(L, rows_sel) if L.compact else None


def dyadic(rng, shape, tie=None):
    a = rng.integers(-128, 129, shape) / 16.0
    if tie is not None:
        a[rng.random(shape) < 0.3] = tie
    return a


def dyadic_mean_inv(rng, L, C):
    """(2, C), or (F, 2, C) with different values per frame: a kernel that reads another frame's statistics fails."""
    shape = (L.F, C) if L.F > 1 else (C,)
    return np.stack([rng.integers(-16, 17, shape) / 16.0, 2.0 ** rng.integers(-1, 3, shape)], axis=-2)


def rows_input(rng, L, C):
    """Dyadic rows with ties; the padded row of a partly filled voxel ties with its largest real row in the even channels (the
    earlier, real row must win); the padded row of a FULL voxel holds the largest value there is (it must not take part)."""
    y = dyadic(rng, (L.rows, C), tie=0.5)
    if L.compact:
        for v in range(L.V):
            n, pad = int(L.vcnt[v]), L.n_real + v
            if n == L.T:
                y[pad] = 8.0
            elif n > 0 and v % 2 == 0:
                y[pad, ::2] = y[L.voff[v]:L.voff[v] + n, ::2].max(0)
    return y


def f32(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)


def host(t):
    return t.cpu().numpy().astype(np.float64)


def guarded(a):
    """The reference padded with the guard rows no kernel may write."""
    return np.concatenate([a, np.full((GUARD,) + a.shape[1:], np.nan)])


def same_rows_written(got, ref):
    """Exactly the rows the reference writes are finite in a NaN pre-filled output."""
    return np.array_equal(np.isfinite(got), np.isfinite(ref))


def forward(concat, y, mi, L, cr):
    """mvx_vfe_bn_max_concat_frames / mvx_bn_segment_max_frames into NaN pre-filled outputs with guard rows, and the _hip wrapper
    of the same kernel, whose result must be the same bits.  -> (out incl. guard rows, argmax incl. guard rows)"""
    from modules import _hip
    from modules import Extension as X
    C = y.shape[1]
    out = torch.full(((y.shape[0] if concat else L.V) + GUARD, 2 * C if concat else C), float('nan'), device=DEV)
    am = torch.full((L.V + GUARD, C), -7, dtype=torch.int32, device=DEV)
    vo, vc, nr, d = _hip._rows_args(cr)
    fn = X.lib.mvx_vfe_bn_max_concat_frames if concat else X.lib.mvx_bn_segment_max_frames
    X.check(fn(X.ptr(y), X.ptr(mi), X.ptr(out), X.ptr(am), L.V, L.T, C, vo, vc, nr, d, X.stream()), 'forward')
    wout, wam = (_hip.vfe_bn_max_concat if concat else _hip.bn_segment_max)(y, mi, L.V, L.T, cr)
    torch.cuda.synchronize()
    assert torch.equal(wout, out[:-GUARD]) and torch.equal(wam, am[:-GUARD])
    return host(out), am.cpu().numpy()


LAYOUTS = ['dense', 'compact', 'setA', 'setB']
CHANNELS = [16, 128, 18]                                   # float4 forms; 18: the scalar forms (C % 4 != 0), frame set B included


# ---- 1. vfe_bn_max_concat(_frames), bn_segment_max(_frames) ----------------------------------------------------------------
@gpu
@pytest.mark.parametrize('C', CHANNELS)
@pytest.mark.parametrize('name', LAYOUTS)
def test_bn_max_forward_exact(name, C):
    L = layout(name)
    rng = np.random.default_rng(100 + C)
    y, mi = rows_input(rng, L, C), dyadic_mean_inv(rng, L, C)
    cr = dev_rows(L)
    ref_out, ref_am = R.bn_max_concat(y, mi, L)
    _, ref_feat, _ = R.bn_max(y, mi, L)
    out, am = forward(True, f32(y), f32(mi), L, cr)
    assert same_rows_written(out, guarded(ref_out))
    assert np.array_equal(out[:-GUARD, :C], ref_out[:, :C]), 'normalised rows'
    assert np.array_equal(out[:-GUARD, C:], ref_out[:, C:]), 'maximum broadcast to every stored row'
    assert np.array_equal(am[:-GUARD], ref_am) and (am[-GUARD:] == -7).all(), 'argmax: the first maximal row'
    feat, am2 = forward(False, f32(y), f32(mi), L, cr)
    assert same_rows_written(feat, guarded(ref_feat))
    assert np.array_equal(feat[:-GUARD], ref_feat)
    assert np.array_equal(am2[:-GUARD], ref_am) and (am2[-GUARD:] == -7).all()
    if L.compact:                                          # the padded row is selected only where it stands for a row
        assert not (ref_am[L.vcnt == L.T] == L.T).any() and (ref_am[L.vcnt == 0] == 0).all()


@gpu
@pytest.mark.parametrize('C', [16, 18])
@pytest.mark.parametrize('name', LAYOUTS)
def test_bn_max_forward_random(name, C):
    L = layout(name)
    rng = np.random.default_rng(200 + C)
    y = rng.standard_normal((L.rows, C)).astype(np.float32)
    shape = (L.F, C) if L.F > 1 else (C,)
    mi = np.stack([rng.standard_normal(shape) * 0.1, rng.random(shape) + 0.5], axis=-2).astype(np.float32)
    cr = dev_rows(L)
    yh = R.normalise(y, mi, L)
    # f32: d = fl(y - m) = (y - m)(1 + e1), r = fl(d * inv) = (y - m) inv (1 + e1)(1 + e2) with |e| <= u / (1 + u), u = 2^-24, so
    # |r - exact| <= |y - m| inv (2u + 3u^2) / (1 + u)^2 < 2u (|y| + |m|) inv.  (No FMA can form here: a difference feeds a product.)
    bound = np.full(yh.shape, np.nan)
    for v in range(L.V):
        m = np.asarray(mi[L.frame_of(v)] if mi.ndim == 3 else mi, np.float64)
        for r in L.stored(v):
            bound[r] = 2 * U * (np.abs(y[r].astype(np.float64)) + np.abs(m[0])) * m[1]
    for concat in (True, False):
        out, am = forward(concat, f32(y), f32(mi), L, cr)
        if concat:
            assert (np.abs(out[:-GUARD, :C] - yh) <= bound).all(), 'normalised rows'
        for v in range(L.V):
            rows = L.in_max(v)
            assert (am[v] >= 0).all() and (am[v] < len(rows)).all()
            chosen = np.asarray([rows[t] for t in am[v]])
            cols = np.arange(C)
            # the chosen row's float64 value lies within the bound (of that element) of the float64 maximum
            assert (yh[rows].max(0) - yh[chosen, cols] <= bound[chosen, cols]).all(), 'argmax'
            got = out[rows[0], C:] if concat else out[v]
            assert (np.abs(got - yh[chosen, cols]) <= bound[chosen, cols]).all(), 'maximum'
            if concat:
                assert all(np.array_equal(out[r, C:], got) for r in L.stored(v))


# ---- 2. vfe_max_concat_backward, segment_max_backward ------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('C', CHANNELS)
@pytest.mark.parametrize('name', LAYOUTS)
def test_max_backward_exact(name, C):
    from modules import _hip
    from modules import Extension as X
    L = layout(name)
    rng = np.random.default_rng(300 + C)
    _, _, am = R.bn_max(rows_input(rng, L, C), dyadic_mean_inv(rng, L, C), L)
    cr = dev_rows(L)
    vo, vc, nr, _ = _hip._rows_args(cr)
    am_d = torch.tensor(am, dtype=torch.int32, device=DEV)
    g, dfeat = dyadic(rng, (L.rows, 2 * C)), dyadic(rng, (L.V, C))
    for kind, up, ref, fn, wrap in (('concat', g, R.max_concat_backward(g, am, L), X.lib.mvx_vfe_max_concat_backward, _hip.vfe_max_concat_backward),
                                    ('segmax', dfeat, R.segment_max_backward(dfeat, am, L), X.lib.mvx_segment_max_backward, _hip.segment_max_backward)):
        up_d = f32(up)
        dyh = torch.full((L.rows + GUARD, C), float('nan'), device=DEV)
        X.check(fn(X.ptr(up_d), X.ptr(am_d), X.ptr(dyh), L.V, L.T, C, vo, vc, nr, X.stream()), kind)
        w = wrap(up_d, am_d, L.V, L.T, cr)
        torch.cuda.synchronize()
        assert torch.equal(w, dyh[:-GUARD]), kind
        got = host(dyh)
        assert same_rows_written(got, guarded(ref)), kind
        assert np.array_equal(got[:-GUARD], ref), kind     # not selected: g[:, :C] (concat), exactly 0 (segmax)


# ---- 3 and 4. row_compact_map(_frames), voxel_row_offsets(_frames) ---------------------------------------------------------
def dense_voxels(L, vc, seed):
    """Dense voxel rows (V * T, vc) of a compact layout: voxel v has vcnt[v] real rows -- its first rows, or, every third partly
    filled voxel, with a padding row in the MIDDLE of them; padding rows have x == y == z == 0 and junk behind (the map kernel
    zeroes it in place).  A real row may have one or two zero coordinates.  Whole voxels of padding: vcnt == 0."""
    rng = np.random.default_rng(seed)
    vox = rng.integers(1, 129, (L.V * L.T, vc)) / 16.0
    vox[:, :3] *= rng.choice([1.0, 1.0, 0.0], (L.V * L.T, 3))
    vox[:, rng.integers(0, 3)] += 0.25                     # ... but never three
    for v in range(L.V):
        n = int(L.vcnt[v])
        real = list(range(n))
        if 2 <= n < L.T and v % 3 == 0:
            real[-1] = n                                   # the hole is local row n - 1
        for t in set(range(L.T)) - set(real):
            vox[v * L.T + t, :3] = 0.0
    return vox.astype(np.float32)


@gpu
@pytest.mark.parametrize('name', LAYOUTS + ['map1300'])
def test_row_compact_map_and_offsets(name):
    """R = V * T is no multiple of 256 in any case (the last block of map_count / map_write is partial): 185, 10 500, 20 650,
    1 300.  map_scan's trip over more than 1024 blocks (262k rows) is left to the full-size tests."""
    from modules import _hip
    from modules import Extension as X
    L = as_compact(layout(name))
    assert (L.V * L.T) % 256 != 0
    vox = dense_voxels(L, 9, 7)
    row_map, rows_sel, n_real, zeroed = R.compact_map(vox)
    assert n_real == L.n_real
    desc = X.FramesDesc.make(L.vox_off, L.real_off, L.T) if L.F > 1 else None
    vox_d = f32(vox)
    res = _hip.row_compact_map(vox_d, desc)
    torch.cuda.synchronize()
    assert int(res[2]) == n_real
    assert np.array_equal(res[0].cpu().numpy(), row_map)
    assert np.array_equal(res[1].cpu().numpy()[:n_real], rows_sel)
    assert np.array_equal(vox_d.cpu().numpy(), zeroed), 'channels 3.. of padding rows zeroed in place, nothing else touched'
    if desc is not None:                                   # the walk over leading, trailing and consecutive empty frames
        ref_off = R.real_offsets(row_map, L.vox_off, L.T)
        assert np.array_equal(ref_off, L.real_off)
        assert np.array_equal(res[3].cpu().numpy(), ref_off)
    voff, vcnt, row_w = R.row_offsets(row_map, L.V, L.T)
    assert np.array_equal(vcnt, L.vcnt) and np.array_equal(voff, L.voff)
    got = _hip.voxel_row_offsets(res[0], L.V, L.T, n_real, desc)
    torch.cuda.synchronize()
    assert np.array_equal(got[0].cpu().numpy(), voff)
    assert np.array_equal(got[1].cpu().numpy(), vcnt)
    assert np.array_equal(host(got[2]), row_w)
    if desc is not None:
        assert np.array_equal(host(got[3]), R.fusion_row_weights(L.vox_off, L.real_off, L.T))


# ---- 5 and 6. vfe_compact_input, vfe_compact_input_backward(_frames) ------------------------------------------------------
@gpu
@pytest.mark.parametrize('vc', [9, 7])
@pytest.mark.parametrize('name', LAYOUTS)
def test_vfe_compact_input(name, vc):
    from modules import _hip
    L = as_compact(layout(name))
    vox = dense_voxels(L, vc, 8)
    _, rows_sel, _, _ = R.compact_map(vox)
    rng = np.random.default_rng(500)
    Fc = 16
    imfeat = dyadic(rng, (L.n_real + L.F, Fc))             # every frame's shared padded row is different
    cr = DevRows(L, rows_sel)
    for pitch in (None, 24):
        ref = R.compact_input(vox, rows_sel, imfeat, L, pitch)
        out = _hip.vfe_compact_input(f32(vox), f32(imfeat), cr, pitch)
        torch.cuda.synchronize()
        assert np.array_equal(host(out), ref), pitch
        assert pitch is None or (host(out)[:, 7 + Fc:] == 0).all()


@gpu
@pytest.mark.parametrize('Fc', [16, 64, 24, 96, 1])        # LDS table: 16, 64, 1 (F <= 64 and 256 % F == 0); fallback: 24, 96
@pytest.mark.parametrize('name', LAYOUTS)
def test_vfe_compact_input_backward(name, Fc):
    from modules import _hip
    L = as_compact(layout(name))
    rng = np.random.default_rng(600 + Fc)
    g = dyadic(rng, (L.rows, 7 + Fc))                      # <= 590 padded rows of |g| <= 8: the sums are exact in f32 and f64
    ref = R.compact_input_backward(g, Fc, L)
    d = _hip.vfe_compact_input_backward(f32(g), Fc, DevRows(L))
    torch.cuda.synchronize()
    got = host(d)
    assert np.array_equal(got[:L.n_real], ref[:L.n_real]), 'real rows: copies'
    for f in range(L.F):
        assert np.array_equal(got[L.n_real + f], ref[L.n_real + f]), 'shared padded row of frame %d' % f


# ---- 7. expand_rows, expand_rows_backward --------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('C', [16, 23, 256])               # 256 / C rows per workgroup trip; 23: idle threads behind 11 * 23
@pytest.mark.parametrize('name', ['dense', 'compact', 'map1300'])
def test_expand_rows(name, C):
    from modules import _hip
    L = as_compact(layout(name))
    row_map = R.compact_map(dense_voxels(L, 9, 7))[0]
    rng = np.random.default_rng(700 + C)
    compact = dyadic(rng, (L.n_real + 1, C))
    pad_row = L.n_real
    rm_d = torch.tensor(row_map, dtype=torch.int32, device=DEV)
    out = _hip.expand_rows(f32(compact), rm_d, pad_row)
    torch.cuda.synchronize()
    assert np.array_equal(host(out), R.expand_rows(compact, row_map, pad_row))
    g = dyadic(rng, (len(row_map), C))                     # < 10 500 padded rows of |g| <= 8: below 2^24 units of 1/16
    dc = _hip.expand_rows_backward(f32(g), rm_d, pad_row, L.n_real + 1)
    torch.cuda.synchronize()
    assert np.array_equal(host(dc), R.expand_rows_backward(g, row_map, pad_row, L.n_real + 1))


@gpu
def test_expand_rows_backward_rejects_more_than_256_channels():
    """The kernel gives a workgroup 256 / C rows: C > 256 must come back as the library's argument error without a launch."""
    from modules import _hip
    from modules import Extension as X
    g = torch.zeros((8, 257), device=DEV)
    rm = torch.zeros((8,), dtype=torch.int32, device=DEV)
    with pytest.raises(X.MvxHipError, match='argument error'):
        _hip.expand_rows_backward(g, rm, 8, 9)
    torch.cuda.synchronize()


# ---- 8. weighted BatchNorm over compact rows of a frame set --------------------------------------------------------------
def rel_err(a, b):
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


@gpu
def test_weighted_batchnorm_on_compact_rows_of_a_frame_set():
    """Frame set A.  The reference is float64 BatchNorm, forward and backward, over the DENSE expansion (every padded row repeated
    T - vcnt times), frame by frame; bounds: those of test_batchnorm_relu_forward_backward (tests/test_conv3d_gpu.py) for the
    unweighted kernels.  The weighted sums of the VFE rows have one producer, the row GEMM's epilogue (frames.linear_bn ->
    _hip.linear_forward_bn_frames, finalised in the launch): its statistics are compared with those of the y it wrote.
    mvx_row_stats_frames itself takes no weights (equal shares of rows per frame, the RPN's layout) and is checked on that
    layout together with bn_finalize(F).  The empty frame has no population: nothing reads its statistics, nothing is asserted."""
    from modules import _hip
    from modules import Extension as X
    L = layout('setA')
    cr = DevRows(L)
    rng = np.random.default_rng(800)
    K, C = 16, 32
    row_w = _hip.voxel_row_offsets(torch.tensor(R.compact_map(dense_voxels(L, 9, 7))[0], dtype=torch.int32, device=DEV), L.V, L.T, L.n_real, cr.desc)[2]
    x = f32(rng.standard_normal((L.rows, K)))
    w = f32(rng.standard_normal((C, K)) * 0.5)
    b = f32(rng.standard_normal((C,)) * 0.3 + 0.3)
    y, mi = _hip.linear_forward_bn_frames(x, w, b, cr.desc, X.ROWS_VFE, row_w, 1e-6)
    torch.cuda.synchronize()
    yh, mih = host(y), host(mi)
    assert (yh >= 0).all()
    ref_mi = R.bn_forward(yh, L, 1e-6)
    live = [f for f in range(L.F) if L.vox_off[f + 1] > L.vox_off[f]]
    for f in live:
        assert rel_err(mih[f, 0], ref_mi[f, 0]) < 2e-5, 'mean of frame %d' % f
        assert rel_err(mih[f, 1], ref_mi[f, 1]) < 2e-5, '1/sqrt(var + eps) of frame %d' % f
    # backward: the gradient of a padded row arrives summed; a row that stands for no dense row (vcnt == T) carries none
    g = rng.standard_normal((L.rows, C))
    g[L.n_real:][L.vcnt == L.T] = 0.0
    ref_dz, ref_db = R.bn_relu_backward(g, yh, ref_mi, L)
    dz, db = _hip.bn_relu_backward(f32(g), y, mi, 1.0, row_w=row_w, desc=cr.desc, kind=X.ROWS_VFE)
    torch.cuda.synchronize()
    dzh = host(dz)
    none = np.isnan(ref_dz[:, 0])
    assert np.array_equal(np.nonzero(none)[0], L.n_real + np.nonzero(L.vcnt == L.T)[0]) and (dzh[none] == 0).all()
    for f in live:
        rows = sorted({r for r, _ in R.dense_expansion(L, f)})
        assert rel_err(dzh[rows], ref_dz[rows]) < 2e-5, 'dz of frame %d' % f
    assert rel_err(host(db), ref_db) < 1e-4
    # mvx_row_stats_frames + bn_finalize(F): three equal shares of rows, unweighted
    n = 1237
    z = rng.standard_normal((3 * n, C)) * np.repeat([1.0, 2.0, 0.5], n)[:, None] + np.repeat([0.3, -1.0, 4.0], n)[:, None]
    z_d = f32(z)
    mi3 = host(_hip.bn_finalize(_hip.row_stats_frames(z_d, C, 3), n, 1e-6, 3))
    ref3 = R.bn_forward(host(z_d), R.Layout(1, 3 * n, vox_off=[0, n, 2 * n, 3 * n]), 1e-6)
    for f in range(3):
        assert rel_err(mi3[f, 0], ref3[f, 0]) < 2e-5 and rel_err(mi3[f, 1], ref3[f, 1]) < 2e-5, f


# ---- 9. feature_sample_rows(_frames) at the edges ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('frames', [1, 3])
def test_feature_sample_rows_edges(frames):
    from modules import _hip
    from modules import Extension as X
    rng = np.random.default_rng(900)
    C, hw, imsize, eps = 8, ((6, 9), (3, 5)), (48.0, 72.0), 1e-3
    # projected (row, column); level 0 has 8 x 8 pixel cells, level 1 16 x 14.4
    proj = [(0.0, 0.0),            # q = -eps on both axes: trunc toward zero gives 0, the fraction is negative, not flagged
            (0.0, 30.0), (20.0, 0.0),
            (47.5, 30.0),          # trunc(q) == H - 1 on both levels: the lower taps read the zero pad
            (20.0, 71.5),          # trunc(q) == W - 1: the right taps read the zero pad
            (47.5, 71.5),
            (48.5, 30.0),          # trunc(q) == H: flagged
            (20.0, 72.5),          # trunc(q) == W: flagged
            (-17.0, 30.0),         # trunc(q) <= -1 on both levels: flagged
            (13.3, 41.7), (30.1, 8.9), (5.5, 66.6)]
    # three frames: the descriptor's frame 1 is empty, the second half of the rows belongs to frame 2 and must read frame 2's maps
    frame_of_row = np.repeat([0] if frames == 1 else [0, 2], len(proj))
    n = len(frame_of_row)
    vc = 9
    vox = rng.standard_normal((n + 5, vc)).astype(np.float32)
    rows_sel = rng.permutation(n + 5)[:n]
    for j, r in enumerate(rows_sel):
        vox[r, -2:] = proj[j % len(proj)]
    # every frame's maps differ by a constant: a row that reads another frame's maps is off by 10 or more
    maps = [[(rng.standard_normal((h, w, C)) + 10.0 * f).astype(np.float32) for h, w in hw] for f in range(frames)]
    ref, mag, flagged = R.sample_rows(vox, rows_sel, frame_of_row, maps, imsize, eps)
    assert flagged.sum() == 3 * 2 * (n // len(proj)) and not flagged[:6].any()
    desc = X.FramesDesc.make([0, 1, 1, 2], [0, len(proj), len(proj), n], 35) if frames > 1 else None
    feats = [f32(m) for fm in maps for m in fm]
    out = torch.full((n + GUARD, 2 * C), float('nan'), device=DEV)
    status = _hip.feature_sample_rows(f32(vox), torch.tensor(rows_sel, dtype=torch.int32, device=DEV), n, feats, imsize, eps, out, desc)
    torch.cuda.synchronize()
    assert int(status) == 1
    got = host(out)
    assert np.isnan(got[n:]).all()
    # the weights are the reference's f32 values; each tap is (F * a) * b (two roundings) and three additions follow: at most
    # five roundings on any path to the result, each relative to a partial sum bounded by S = sum |F_tap * weight_tap|:
    # |err| <= ((1 + u)^5 - 1) S < 8 u S
    assert (np.abs(got[:n] - ref) <= 8 * U * mag).all()
    for j in range(n):
        for lv in range(2):
            if flagged[j, lv]:
                assert (got[j, lv * C:(lv + 1) * C] == 0).all()


@gpu
def test_feature_sample_rows_status_clean_without_flagged_rows():
    from modules import _hip
    rng = np.random.default_rng(901)
    vox = rng.standard_normal((4, 9)).astype(np.float32)
    vox[:, -2:] = [(0.0, 0.0), (47.5, 71.5), (10.0, 10.0), (30.0, 60.0)]
    maps = [[rng.standard_normal((6, 9, 8)).astype(np.float32), rng.standard_normal((3, 5, 8)).astype(np.float32)]]
    ref, mag, flagged = R.sample_rows(vox, np.arange(4), np.zeros(4, int), maps, (48.0, 72.0), 1e-3)
    assert not flagged.any()
    out = torch.full((4, 16), float('nan'), device=DEV)
    status = _hip.feature_sample_rows(f32(vox), torch.arange(4, dtype=torch.int32, device=DEV), 4, [f32(m) for m in maps[0]],
                                      (48.0, 72.0), 1e-3, out)
    torch.cuda.synchronize()
    assert int(status) == 0
    assert (np.abs(host(out) - ref) <= 8 * U * mag).all()


# ---- the reference on hand-computed cases (host only) ------------------------------------------------------------------------
def test_reference_one_voxel_two_of_three_rows():
    L = R.Layout(3, 1, [2])
    assert (L.n_real, L.rows, L.stored(0), L.in_max(0), L.weight(0)) == (2, 3, [0, 1, 2], [0, 1, 2], [1, 1, 1])
    y = np.array([[1.0, 5.0], [3.0, 2.0], [2.0, 7.0]])     # rows 0, 1 real, row 2 the padded row
    mi = np.array([[1.0, 1.0], [2.0, 0.5]])                # yhat = [[0, 2], [4, .5], [2, 3]]
    out, am = R.bn_max_concat(y, mi, L)
    assert np.array_equal(out, [[0, 2, 4, 3], [4, .5, 4, 3], [2, 3, 4, 3]]) and np.array_equal(am, [[1, 2]])
    g = np.array([[1.0, 2, 10, 20], [3, 4, 30, 40], [5, 6, 50, 60]])
    assert np.array_equal(R.max_concat_backward(g, am, L), [[1, 2], [3 + 90, 4], [5, 6 + 120]])
    assert np.array_equal(R.segment_max_backward(np.array([[7.0, 9.0]]), am, L), [[0, 0], [7, 0], [0, 9]])
    voff, vcnt, row_w = R.row_offsets([0, 1, -1], 1, 3)
    assert (list(voff), list(vcnt), list(row_w)) == ([0], [2], [1, 1, 1])
    # BatchNorm over the dense expansion [1, 3, 2]: mean 2, variance 2/3
    st = R.bn_forward(y[:, :1], L, 0.0)
    assert np.allclose(st[0, :, 0], [2.0, np.sqrt(1.5)], rtol=1e-15)


def test_reference_voxel_without_real_rows():
    L = R.Layout(3, 2, [0, 3])
    assert L.stored(0) == [3] and L.in_max(0) == [3] and L.weight(0) == [3]
    assert L.stored(1) == [0, 1, 2, 4] and L.in_max(1) == [0, 1, 2] and L.weight(1) == [1, 1, 1, 0]
    y = np.array([[1.0], [2.0], [0.0], [-4.0], [9.0]])
    _, feat, am = R.bn_max(y, np.array([[0.0], [1.0]]), L)
    assert np.array_equal(feat, [[-4], [2]]) and np.array_equal(am, [[0], [1]])   # the full voxel's padded row (9) takes no part
    voff, vcnt, row_w = R.row_offsets([-1, -1, -1, 0, 1, 2], 2, 3)
    assert (list(voff), list(vcnt), list(row_w)) == ([0, 0], [0, 3], [1, 1, 1, 3, 0])
    assert list(R.fusion_row_weights([0, 0, 2], [0, 0, 3], 3)) == [1, 1, 1, 0, 3]
    assert list(R.real_offsets([-1, -1, -1, 0, 1, 2], [0, 1, 1, 2], 3)) == [0, 0, 0, 3]
    g = np.arange(5.0)[:, None] * np.ones((1, 9))
    assert np.array_equal(R.compact_input_backward(g, 2, L), [[0, 0], [1, 1], [2, 2], [7, 7]])


def test_reference_first_maximum_wins_a_tie():
    L = R.Layout(4, 1, [2])
    y = np.array([[2.0, 1.0], [2.0, 3.0], [2.0, 3.0]])     # channel 0: three equal rows; channel 1: real row 1 ties with the padded row
    _, feat, am = R.bn_max(y, np.array([[0.0, 0.0], [1.0, 1.0]]), L)
    assert np.array_equal(feat, [[2, 3]]) and np.array_equal(am, [[0, 1]])
    D = R.Layout(3, 1)
    assert np.array_equal(R.bn_max(y, np.array([[0.0, 0.0], [1.0, 1.0]]), D)[2], [[0, 1]])
    out, mag, flagged = R.sample_rows(np.array([[0, 0, 0, 4.0, 12.0]], np.float32), [0], [0], [[np.ones((2, 2, 1), np.float32)]],
                                      (8.0, 8.0), 0.0)
    # q = (1, 3): the column index 3 > W = 2 is flagged
    assert flagged[0, 0] and out[0, 0] == 0
    out, mag, flagged = R.sample_rows(np.array([[0, 0, 0, 6.0, 2.0]], np.float32), [0], [0], [[np.ones((2, 2, 1), np.float32)]],
                                      (8.0, 8.0), 0.0)
    # q = (1.5, 0.5): i = (1, 0), fractions (.5, .5); the taps of row 2 are the zero pad: 1 * .5 * .5 + 1 * .5 * .5
    assert not flagged[0, 0] and out[0, 0] == 0.5 and mag[0, 0] == 0.5
