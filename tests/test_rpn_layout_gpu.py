"""The RPN's layout kernels (csrc/rpn.hip) one by one, through the C ABI: mvx_space_to_depth_frames, mvx_d2s_bn_apply_frames and
mvx_bn_apply_strided_frames, forward and reverse, on ordinal values (element = its own flat index) against the numpy index
arithmetic of tests/rpn_layout_cases.py, and mvx_row_stats_frames with mvx_bn_finalize_frames against float64.

Every destination starts as NaN with NaN behind it; afterwards exactly the result elements differ from NaN (columns outside a
slice and rows behind the last stay NaN).  A reverse call leaves the buffer it reads unchanged bit for bit.

The normalising forms compute (v - mean_f) * inv_f in f32, two rounded operations with nothing to contract; the reference does
the same two operations in numpy float32 and the comparison is EQUALITY (it held on an MI355X for every case of this file).
Mean and inverse deviation: 2e-5 of the largest float64 magnitude, the project's bound for these quantities; the kernel sums in
f64 throughout; the largest error of the 24 cases measured on an MI355X was 5.9e-08 (C = 1024, 40 000 rows per frame)."""
import ctypes

import numpy as np
import pytest
import torch

import rpn_layout_cases as L

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
GUARD = 64
TAIL = 3                               # rows behind the last row of a sliced buffer


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _nan(n):
    return torch.full((n,), NAN, dtype=torch.float32, device=DEV)


def _dev(a):
    """A device copy of the array with GUARD NaN elements behind it -> (buffer, flat view of the data)."""
    a = np.ascontiguousarray(a, np.float32)
    buf = _nan(a.size + GUARD)
    buf[:a.size] = torch.from_numpy(a.reshape(-1))
    return buf, buf[:a.size]


def _same_bits(t, a):
    """The device tensor holds exactly the f32 array, NaN included."""
    return np.array_equal(t.cpu().numpy().view(np.int32).reshape(-1), np.ascontiguousarray(a, np.float32).view(np.int32).reshape(-1))


def _same_values(t, a):
    """Equal as numbers, with NaN exactly where the array has NaN."""
    got = t.cpu().numpy().reshape(-1)
    a = np.asarray(a, np.float32).reshape(-1)
    return np.array_equal(np.isnan(got), np.isnan(a)) and np.array_equal(got[~np.isnan(a)], a[~np.isnan(a)])


# ---- space to depth ----------------------------------------------------------------------------------------------------------
def _s2d(src, dst, case, reverse):
    from modules import Extension as X
    F, P, h, w, C = case
    rc = X.lib.mvx_space_to_depth_frames(_p(src), _p(dst), F, P, h, w, C, int(reverse), X.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('case', L.S2D_CASES, ids=str)
def test_space_to_depth(case):
    F, P, h, w, C = case
    x = L.ordinal((F * P, h, w, C))
    ref = L.space_to_depth(x, F, P)
    xbuf, xd = _dev(x)
    zbuf = _nan(x.size + GUARD)
    assert _s2d(xd, zbuf, case, 0) == 0
    assert _same_bits(zbuf[:x.size], ref) and torch.isnan(zbuf[x.size:]).all(), 'forward'
    assert _same_bits(xbuf[:x.size], x) and torch.isnan(xbuf[x.size:]).all()
    # reverse of an image with other values, then reverse(forward(x)) == x
    z2 = L.ordinal(ref.shape) * 2 + 1
    _, z2d = _dev(z2)
    back = _nan(x.size + GUARD)
    assert _s2d(z2d, back, case, 1) == 0
    assert _same_bits(back[:x.size], L.depth_to_space(z2, F, P)) and torch.isnan(back[x.size:]).all(), 'reverse'
    back2 = _nan(x.size + GUARD)
    assert _s2d(zbuf, back2, case, 1) == 0
    assert _same_bits(back2[:x.size], x) and torch.isnan(back2[x.size:]).all(), 'reverse(forward(x))'


@pytest.mark.parametrize('case', L.S2D_REJECTED, ids=str)
@pytest.mark.parametrize('reverse', [0, 1])
def test_space_to_depth_rejects(case, reverse):
    """Odd h, odd w, C % 4 != 0: the argument error, and nothing is launched."""
    F, P, h, w, C = case
    n = F * P * h * w * C
    _, src = _dev(L.ordinal((n,)))
    dst = _nan(n + GUARD)
    assert _s2d(src, dst, case, reverse) < 0
    assert torch.isnan(dst).all()


# ---- d2s_bn_apply ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s', L.D2S_S)
@pytest.mark.parametrize('shape', L.D2S_SHAPES, ids=str)
def test_d2s_bn_apply(shape, s):
    """Every (ld_out, col_offset) of rpn_layout_cases.slices: mi == NULL a bit-exact copy, mi of F distinct frames normalises each
    pixel with its own frame's row, the reverse is the exact inverse gather."""
    from modules import Extension as X
    F, h, w, C = shape
    rows_out = F * h * s * w * s
    t = L.ordinal((F * h * w, s * s * C))
    moved = L.d2s_rows(t, F, h, w, s)
    frame = np.repeat(np.arange(F), h * s * w * s)
    mi = L.mean_inv(C, F, 10 * s + C)
    _, mid = _dev(mi)
    tbuf, td = _dev(t)

    def call(tt, m, out, ld, off, reverse):
        rc = X.lib.mvx_d2s_bn_apply_frames(_p(tt), _p(m), _p(out), F, h, w, s, C, ld, off, reverse, X.stream())
        torch.cuda.synchronize()
        return rc

    for ld, off in L.slices(C):
        total = (rows_out + TAIL) * ld
        out = _nan(total)
        assert call(td, None, out, ld, off, 0) == 0
        assert _same_values(out, L.in_slice(moved, rows_out + TAIL, ld, off)), ('copy', ld, off)
        out = _nan(total)
        assert call(td, mid, out, ld, off, 0) == 0
        want = L.in_slice(L.normalise_f32(moved, mi, frame), rows_out + TAIL, ld, off)
        assert _same_values(out, want), ('normalise', ld, off)
        assert _same_bits(tbuf[:t.size], t) and torch.isnan(tbuf[t.size:]).all()
        # reverse: the slice of a buffer whose other columns hold other finite numbers, which must not be picked up
        src = L.in_slice(moved * 3 + 2, rows_out + TAIL, ld, off, fill=-7.0)
        _, srcd = _dev(src)
        back = _nan(t.size + GUARD)
        assert call(back, mid, srcd, ld, off, 1) == 0
        assert _same_bits(back[:t.size], t * 3 + 2) and torch.isnan(back[t.size:]).all(), ('reverse', ld, off)
        assert _same_bits(srcd, src), 'the reverse changed the buffer it reads'
        print('d2s %s s %d ld %d off %d: copy, normalise (f32 equality) and reverse exact' % (shape, s, ld, off))


def test_d2s_bn_apply_rejects():
    from modules import Extension as X
    t, out = _nan(64 + GUARD), _nan(256)
    for C, ld, off in ((6, 8, 0), (4, 6, 0), (4, 8, 2), (4, 8, 8), (8, 4, 0)):
        assert X.lib.mvx_d2s_bn_apply_frames(_p(t), None, _p(out), 1, 1, 1, 1, C, ld, off, 0, X.stream()) < 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- bn_apply_strided --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', L.D2S_SHAPES, ids=str)
def test_bn_apply_strided(shape):
    """[rows][C] into a column slice, the frames equal shares of the rows; mi == NULL copies; the reverse copies the slice out."""
    from modules import Extension as X
    F, h, w, C = shape
    rows = F * h * w
    y = L.ordinal((rows, C))
    frame = np.repeat(np.arange(F), h * w)
    mi = L.mean_inv(C, F, 77 + C)
    _, mid = _dev(mi)
    ybuf, yd = _dev(y)

    def call(yy, m, out, ld, off, reverse):
        rc = X.lib.mvx_bn_apply_strided_frames(_p(yy), _p(m), _p(out), rows, C, ld, off, F, reverse, X.stream())
        torch.cuda.synchronize()
        return rc

    for ld, off in L.slices(C):
        total = (rows + TAIL) * ld
        out = _nan(total)
        assert call(yd, None, out, ld, off, 0) == 0
        assert _same_values(out, L.in_slice(y, rows + TAIL, ld, off)), ('copy', ld, off)
        out = _nan(total)
        assert call(yd, mid, out, ld, off, 0) == 0
        assert _same_values(out, L.in_slice(L.normalise_f32(y, mi, frame), rows + TAIL, ld, off)), ('normalise', ld, off)
        assert _same_bits(ybuf[:y.size], y) and torch.isnan(ybuf[y.size:]).all()
        src = L.in_slice(y * 3 + 2, rows + TAIL, ld, off, fill=-7.0)
        _, srcd = _dev(src)
        back = _nan(y.size + GUARD)
        assert call(back, mid, srcd, ld, off, 1) == 0
        assert _same_bits(back[:y.size], y * 3 + 2) and torch.isnan(back[y.size:]).all(), ('reverse', ld, off)
        assert _same_bits(srcd, src)
        print('strided %s ld %d off %d: copy, normalise (f32 equality) and reverse exact' % (shape, ld, off))


def test_bn_apply_strided_rejects_rows_that_are_no_whole_frames():
    from modules import Extension as X
    _, y = _dev(L.ordinal((7, 4)))
    out = _nan(7 * 4 + GUARD)
    _, mi = _dev(L.mean_inv(4, 3, 1))
    assert X.lib.mvx_bn_apply_strided_frames(_p(y), _p(mi), _p(out), 7, 4, 4, 0, 3, 0, X.stream()) < 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- row_stats_frames + bn_finalize_frames -------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', L.STATS_CASES, ids=lambda c: 'C%d_rows%d' % c)
def test_row_stats_frames(case):
    """Three frames of their own scale and offset, mean and inverse deviation per frame against float64 (a single row per frame:
    variance 0, inverse deviation 1 / sqrt(eps)).  40 000 rows per frame pass the cap of 512 blocks per frame for C >= 48."""
    from modules import _hip
    from modules import Extension as X
    C, per = case
    F = L.STATS_F
    if per == 40000 and C >= 48:
        assert L.stats_blocks(per, C) > L.STATS_BLOCK_CAP
    g = torch.Generator().manual_seed(13 * C + per)
    y = torch.randn((F, per, C), generator=g)
    y = y * torch.tensor(L.STATS_SCALE)[:, None, None] + torch.tensor(L.STATS_OFFSET)[:, None, None]
    n = y.numel()
    ybuf = _nan(n + GUARD)
    ybuf[:n] = y.reshape(-1).to(DEV)
    ns = F * _hip.STATS_REPLICAS * 2 * C
    st = torch.full((ns + GUARD,), NAN, dtype=torch.float64, device=DEV)
    assert X.lib.mvx_row_stats_frames(_p(ybuf), _p(st), F * per, C, F, X.stream()) == 0
    mi = _nan(F * 2 * C + GUARD)
    assert X.lib.mvx_bn_finalize_frames(_p(st), float(per), L.EPS, _p(mi), C, F, X.stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(st[ns:]).all() and not torch.isnan(st[:ns]).any() and torch.isnan(mi[F * 2 * C:]).all()
    got = mi[:F * 2 * C].view(F, 2, C).cpu().double()
    errs = []
    for f in range(F):
        d = y[f].double()
        mean = d.mean(0)
        inv = 1.0 / torch.sqrt(((d - mean) ** 2).mean(0) + L.EPS)
        errs.append((float((got[f, 0] - mean).abs().max() / mean.abs().max()), float((got[f, 1] - inv).abs().max() / inv.abs().max())))
    print('row_stats_frames C %d rows %d: mean / inverse deviation per frame %s' % (C, per, ' '.join('%.2e/%.2e' % e for e in errs)))
    assert max(max(e) for e in errs) < L.BOUND
