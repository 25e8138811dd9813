"""The exact-f32 row GEMM (csrc/linear.hip, csrc/rowgemm_common.h) kernel by kernel against float64, through the C ABI
(mvx_linear_forward, mvx_linear_forward_bn, mvx_linear_wgrad) so that the test chooses leading dimensions, workspace and flags
itself; a few calls go through modules/_hip.py on non-contiguous column-slice views.  Cases, operands and the reference:
tests/rowgemm_cases.py.

Every operand is a view of a larger buffer whose unused part is NaN (columns beside the used ones, rows behind the last), and
every destination starts as NaN: afterwards exactly the result elements are finite and everything else is still NaN.  The routing
cases pass no split-K workspace, so they also show that without one nothing outside y is written.

Routing, as linear_forward_impl states it:
    vec  = x and w 16-byte aligned, ldx % 4 == 0, ldw % 4 == 0, k % 4 == 0 and (w_transposed: n % 4 == 0)
    wide = n > 64                                   -> linear_fwd<WT = w_transposed, NT = wide ? 4 : 2, VEC = vec>
    split-K: a workspace, no bias / stats / ReLU, ldy == n, fewer than 128 output blocks and k >= 8 * 32; the slabs are summed by
             slab_reduce_wide when rows * n > 2^18, else by slab_reduce
and mvx_linear_wgrad:
    vec  = x and dz 16-byte aligned, ldx % 4 == 0, lddz % 4 == 0, k % 4 == 0, n % 4 == 0   -> linear_wgrad<vec>
Each test asserts that its operands meet the condition of the instantiation it names (rowgemm_cases.fwd_inst / wgrad_vec).

Which case reaches which kernel ((K, N); rows 1, 129 and 300 each):
    linear_fwd<0, 2, 1>  head24 (24, 16), head768 (768, 16), xslice8 (24, 32) with x = buf[:, 8:32]; split-K r100k256
    linear_fwd<0, 4, 1>  tail36x192 (36, 192), wide68 (64, 68); split-K wide
    linear_fwd<0, 2, 0>  k23n32 (23, 32), xslice1 (24, 32) with x = buf[:, 1:25]; split-K scalar
    linear_fwd<0, 4, 0>  k23n128 (23, 128)
    linear_fwd<1, 2, 1>  t40x64 (40, 64), t128x32 (128, 32)
    linear_fwd<1, 4, 1>  thead (16, 768), twslice (72, 192) with ldw > n; split-K tailslab
    linear_fwd<1, 2, 0>  t24x30 (24, 30)
    linear_fwd<1, 4, 0>  t23x70 (23, 70)
    slab_reduce          split-K r100k256, tailslab, scalar; every weight gradient
    slab_reduce_wide     split-K wide (2100 x 128 outputs)
    linear_wgrad<true>   row1, rows31, rows33, strip1, blocks2x2v (k = 132), slices
    linear_wgrad<false>  vfe23 (k = 23), n30 (n = 30), xslice1 (unaligned x), blocks2x2 (k = 130)

Bounds, max error over max |float64 reference|: 2e-6, the project's bound for this kernel (tests/test_voxelnet_gpu.py), and for
K <= 40 also 4 x 2.2124e-07 (F32_MEASURED of tests/test_linear_epilogue_gpu.py).  BatchNorm sums 1e-12, mean and inverse standard
deviation 2e-5, as in that file.  Each case prints its error (-s).

Largest error per instantiation, measured on an MI355X (routing cases; the case that gave it):
    linear_fwd<0, 2, 1>  1.011e-06  head768 rows 129 (K <= 40: 1.572e-07 head24 rows 300; with an epilogue 3.096e-07)
    linear_fwd<0, 4, 1>  4.078e-07  wide68 rows 129  (K <= 40: 2.355e-07 tail36x192 rows 300)
    linear_fwd<0, 2, 0>  2.069e-07  xslice1 rows 1
    linear_fwd<0, 4, 0>  2.157e-07  k23n128 rows 129
    linear_fwd<1, 2, 1>  3.830e-07  t128x32 rows 300 (K <= 40: 2.284e-07 t40x64 rows 129)
    linear_fwd<1, 4, 1>  3.825e-07  twslice rows 300 (K <= 40: 1.711e-07 thead rows 129)
    linear_fwd<1, 2, 0>  1.942e-07  t24x30 rows 300
    linear_fwd<1, 4, 0>  1.483e-07  t23x70 rows 300
    split-K              2.542e-07  tailslab         (unsplit r100k256 with an epilogue: 5.481e-07)
    linear_wgrad<true>   3.745e-07  strip1
    linear_wgrad<false>  3.260e-07  blocks2x2
No small-K case needed more than the measured 4 x 2.2124e-07, so no comparison with the untransposed 16-byte path is made."""
import ctypes

import pytest
import torch

import rowgemm_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
GUARD = 64                              # NaN elements behind every workspace, statistics and dw buffer
EPS = 1e-6


def _p(t):
    """Pointer of the first element of a (column-slice) view."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _nan(n, dtype=torch.float32):
    return torch.full((n,), NAN, dtype=dtype, device=DEV)


def _tailed(t):
    """A contiguous copy of the 1-D tensor t with NaN behind it (bias, row weights: their loads are clamped to the last element)."""
    buf = _nan(t.numel() + 4)
    buf[:t.numel()] = t
    return buf[:t.numel()]


def _forward(x, w, wt, k, n, bias=None, relu=False, y0=0, ldy=None, stats=None, row_w=None, ws=None, ws_bytes=0, bn=None):
    """One call of mvx_linear_forward (or, with bn = (counter, count, mean_inv), mvx_linear_forward_bn) into a NaN destination
    (rows + TAIL_ROWS, ldy); the result is its columns [y0, y0 + n).  Returns (buffer, result view)."""
    from modules import _hip
    from modules import Extension as X
    rows = x.shape[0]
    ldy = n + 4 if ldy is None else ldy
    ybuf = torch.full((rows + C.TAIL_ROWS, ldy), NAN, device=DEV)
    y = ybuf[:rows, y0:y0 + n]
    flags = _hip.FLAG_RELU if relu else 0
    if bn is not None:
        rc = X.lib.mvx_linear_forward_bn(_p(x), x.stride(0), _p(w), w.stride(0), int(wt), _p(bias), _p(y), ldy, _p(stats), _p(row_w),
                                         rows, k, n, flags, _p(bn[0]), float(bn[1]), EPS, _p(bn[2]), X.stream())
    else:
        rc = X.lib.mvx_linear_forward(_p(x), x.stride(0), _p(w), w.stride(0), int(wt), _p(bias), _p(y), ldy, _p(stats), _p(row_w),
                                      rows, k, n, flags, _p(ws), ws_bytes, X.stream())
    torch.cuda.synchronize()
    assert rc == 0, 'mvx_linear_forward returned %d' % rc
    return ybuf, y


def _check_y(tag, ybuf, y, y0, ref, k):
    """Exactly the result is finite; its error against float64 is printed and held to the bound of K = k."""
    assert C.only_view_finite(ybuf, y.shape[0], y0, y.shape[1]), tag + ': something other than the rows x n result was written'
    err = C.rel(y, ref)
    print('%s: y vs float64 %.3e' % (tag, err))
    assert err < C.bound_for(k), tag
    return err


@pytest.mark.parametrize('rows', C.FWD_ROWS)
@pytest.mark.parametrize('case', C.FWD_CASES, ids=lambda c: c.name)
def test_forward_instantiations(case, rows):
    """y = x w^T without an epilogue and without a workspace, one case at least per linear_fwd<WT, NT, VEC>."""
    x, w, _ = C.fwd_operands(case, rows, DEV)
    assert C.fwd_inst(x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), case.wt, case.K, case.N) == case.inst
    ybuf, y = _forward(x, w, case.wt, case.K, case.N)
    _check_y('linear_fwd<%d, %d, %d> %s rows %d' % (case.inst + (case.name, rows)), ybuf, y, 0,
             C.fwd_reference(x, w, case.wt), case.K)


@pytest.mark.parametrize('variant', ['bias_relu', 'bias', 'none', 'yslice', 'stats', 'bn'])
@pytest.mark.parametrize('name', ['head24', 'tail36x192'])
def test_forward_epilogue(name, variant):
    """Bias and ReLU on and off, y as the column slice buf[:, 32:32 + n], the weighted BatchNorm sums of a single frame (F == 1
    accessors) through mvx_linear_forward, and their finalisation through mvx_linear_forward_bn; a narrow and a wide shape."""
    from modules import _hip
    case, rows = C.FWD_BY_NAME[name], 300
    K, N = case.K, case.N
    x, w, b = C.fwd_operands(case, rows, DEV, seed=1)
    bias = None if variant == 'none' else _tailed(b)
    relu = variant not in ('bias', 'none')
    y0, ldy = (32, N + 40) if variant == 'yslice' else (0, None)
    stats = row_w = bn = mi = None
    if variant in ('stats', 'bn'):
        # statistics f64 [MVX_REP][2][n], cleared by the call: they start as NaN, and NaN stays behind them
        stats = _nan(_hip.STATS_REPLICAS * 2 * N + GUARD, torch.float64)
        g = torch.Generator().manual_seed(5)
        rw = torch.randint(1, 5, (rows,), generator=g).float()
        rw[-3:] = torch.tensor([2000.0, 3050.0, 77.0])              # rows that stand for many
        row_w = _tailed(rw.to(DEV))
        count = float(rw.double().sum())
    if variant == 'bn':
        mi = _nan(2 * N + GUARD)
        bn = (torch.zeros((2,), dtype=torch.int32, device=DEV), count, mi)
    ybuf, y = _forward(x, w, case.wt, K, N, bias=bias, relu=relu, y0=y0, ldy=ldy, stats=stats, row_w=row_w, bn=bn)
    _check_y('%s %s' % (name, variant), ybuf, y, y0, C.fwd_reference(x, w, case.wt, bias, relu), K)
    if stats is None:
        return
    per = _hip.STATS_REPLICAS * 2 * N
    assert torch.isnan(stats[per:]).all()
    st = stats[:per].view(_hip.STATS_REPLICAS, 2, N).sum(0)
    yw = y.double() * row_w.double()[:, None]
    s1, s2 = yw.sum(0), (yw * y.double()).sum(0)
    errs = (C.rel(st[0], s1), C.rel(st[1], s2))
    print('  sums %.3e %.3e' % errs)
    assert errs[0] < 1e-12 and errs[1] < 1e-12
    if variant == 'bn':
        assert torch.isnan(mi[2 * N:]).all()
        mean = s1 / count
        inv = 1.0 / torch.sqrt((s2 / count - mean * mean).clamp_min(0.0) + EPS)
        errs = (C.rel(mi[:N], mean), C.rel(mi[N:2 * N], inv))
        print('  mean %.3e, inverse std %.3e' % errs)
        assert errs[0] < 2e-5 and errs[1] < 2e-5


@pytest.mark.parametrize('where', ['w', 'x'])
@pytest.mark.parametrize('name', ['tail36x192', 't40x64', 'k23n32', 't23x70'])
def test_forward_inf_stays_in_its_row_or_column(name, where):
    """An infinite first element -- the one that clamped loads read -- makes only its own output column (weight) or row (x)
    non-finite: the K tail of BOTH staged tiles is zero, not 0 x whatever the clamped load fetched.  Shapes with a K tail, for
    the 16-byte and the scalar reads in both weight orientations."""
    case, rows = C.FWD_BY_NAME[name], 129
    x, w, _ = C.fwd_operands(case, rows, DEV, seed=2)
    (w if where == 'w' else x)[0, 0] = float('inf')    # k = 0 of column 0 in either weight orientation, or of row 0
    assert C.fwd_inst(x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), case.wt, case.K, case.N) == case.inst
    ybuf, y = _forward(x, w, case.wt, case.K, case.N)
    assert torch.isnan(ybuf[rows:]).all() and torch.isnan(ybuf[:, case.N:]).all()
    ref = C.fwd_reference(x, w, case.wt)
    keep = torch.isfinite(ref)
    assert int((~keep).sum()) == (rows if where == 'w' else case.N)
    assert bool((torch.isfinite(y) == keep).all()), 'the infinity reached other outputs'
    zero = torch.zeros((), dtype=torch.float64, device=DEV)
    err = C.rel(torch.where(keep, y.double(), zero), torch.where(keep, ref, zero))
    print('%s inf in %s: finite part vs float64 %.3e' % (name, where, err))
    assert err < C.bound_for(case.K)


# ---- split-K ----------------------------------------------------------------------------------------------------------
def _splitk_workspace(rows, n):
    from modules import Extension as X
    nbytes = X.lib.mvx_linear_splitk_workspace_bytes(rows, n)
    assert nbytes % 4 == 0 and nbytes >= 2 * rows * n * 4
    return _nan(nbytes // 4 + GUARD), nbytes


def _splitk_operands(c, seed=3):
    case = C.Fwd(c.name, c.K, c.N, c.wt, 0, None, 0, None, c.inst)
    x, w, b = C.fwd_operands(case, c.R, DEV, seed=seed)
    assert C.fwd_inst(x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), c.wt, c.K, c.N) == c.inst
    return x, w, b


@pytest.mark.parametrize('case', C.SPLITK_CASES, ids=lambda c: c.name)
def test_splitk(case):
    """Eligible products: the workspace holds s slabs (read off its NaN pattern), the slabs add up to the product (their k ranges
    tile [0, K)), y is their sum (the reduction visits every slab and element), and a second call repeats y bit for bit."""
    R, K, N = case.R, case.K, case.N
    assert (R * N > 1 << 18) == (case.reduce == 'slab_reduce_wide')          # launch_slab_reduce's condition
    x, w, _ = _splitk_operands(case)
    ws, nbytes = _splitk_workspace(R, N)
    ybuf, y = _forward(x, w, case.wt, K, N, ldy=N, ws=ws, ws_bytes=nbytes)
    ref = C.fwd_reference(x, w, case.wt)
    _check_y('split-K %s' % case.name, ybuf, y, 0, ref, K)
    finite = torch.isfinite(ws)
    count = int(finite.sum())
    s = count // (R * N)
    print('  %d slabs' % s)
    assert count == s * R * N and 2 <= s <= 16
    assert bool(finite[:count].all()) and bool(torch.isnan(ws[count:]).all())
    slabs = ws[:count].view(s, R, N).double().sum(0)
    err = C.rel(slabs, ref)
    print('  float64 sum of the slabs vs float64 %.3e' % err)
    assert err < C.bound_for(K)
    assert float((y.double() - slabs).abs().max()) <= 1e-6 * float(y.abs().max())
    ws2, _ = _splitk_workspace(R, N)
    _, y2 = _forward(x, w, case.wt, K, N, ldy=N, ws=ws2, ws_bytes=nbytes)
    assert torch.equal(y, y2)


@pytest.mark.parametrize('form', C.SPLITK_OFF)
def test_splitk_stays_off(form):
    """The contract keeps split-K off with a bias, with ReLU, with statistics and with ldy != n: the workspace is not touched,
    the call succeeds and y is right."""
    from modules import _hip
    case = C.SPLITK_CASES[0]
    R, K, N = case.R, case.K, case.N
    x, w, b = _splitk_operands(case)
    ws, nbytes = _splitk_workspace(R, N)
    bias = _tailed(b) if form == 'bias' else None
    relu = form == 'relu'
    stats = _nan(_hip.STATS_REPLICAS * 2 * N + GUARD, torch.float64) if form == 'stats' else None
    ybuf, y = _forward(x, w, case.wt, K, N, bias=bias, relu=relu, ldy=N + 4 if form == 'ldy' else N, stats=stats, ws=ws,
                       ws_bytes=nbytes)
    assert torch.isnan(ws).all(), 'split-K ran'
    _check_y('split-K off (%s)' % form, ybuf, y, 0, C.fwd_reference(x, w, case.wt, bias, relu), K)
    if stats is not None:
        per = _hip.STATS_REPLICAS * 2 * N
        assert torch.isnan(stats[per:]).all()
        assert C.rel(stats[:per].view(-1, 2, N).sum(0)[0], y.double().sum(0)) < 1e-12


# ---- weight gradient --------------------------------------------------------------------------------------------------
def _wgrad(x, dz, k, n, flags, dw_fill, rows=None):
    """One call of mvx_linear_wgrad with a NaN workspace of mvx_linear_wgrad_workspace_bytes and NaN guards behind the workspace
    and behind dw (n * k floats, which start as ``dw_fill``: a number or a tensor); ``rows``: fewer than x holds.  Returns dw (n, k)."""
    from modules import Extension as X
    rows = x.shape[0] if rows is None else rows
    nbytes = X.lib.mvx_linear_wgrad_workspace_bytes(rows, k, n)
    assert nbytes % 4 == 0
    ws = _nan(nbytes // 4 + GUARD)
    dwbuf = _nan(n * k + GUARD)
    dwbuf[:n * k] = dw_fill
    X.check(X.lib.mvx_linear_wgrad(_p(x), x.stride(0), _p(dz), dz.stride(0), _p(dwbuf), rows, k, n, flags, _p(ws), nbytes,
                                   X.stream()), 'mvx_linear_wgrad')
    torch.cuda.synchronize()
    assert torch.isnan(ws[nbytes // 4:]).all() and torch.isnan(dwbuf[n * k:]).all()
    if rows == 0:
        assert torch.isnan(ws).all()
    return dwbuf[:n * k].view(n, k)


def _wgrad_case(name, seed=4):
    c = C.WGRAD_BY_NAME[name]
    x, dz = C.wgrad_operands(c, DEV, seed=seed)
    assert C.wgrad_vec(x.data_ptr(), x.stride(0), dz.data_ptr(), dz.stride(0), c.K, c.N) == c.vec
    return c, x, dz


@pytest.mark.parametrize('name', [c.name for c in C.WGRAD_CASES])
def test_wgrad(name):
    """dW = dz^T x into a NaN dw, and a second call bit for bit."""
    c, x, dz = _wgrad_case(name)
    dw = _wgrad(x, dz, c.K, c.N, 0, NAN)
    assert torch.isfinite(dw).all()
    err = C.rel(dw, C.wgrad_reference(x, dz))
    print('linear_wgrad<%d> %s: dw vs float64 %.3e' % (c.vec, name, err))
    assert err < C.bound_for(c.K)
    assert torch.equal(dw, _wgrad(x, dz, c.K, c.N, 0, NAN))


@pytest.mark.parametrize('name', C.WGRAD_ACCUMULATE)
def test_wgrad_accumulate(name):
    """MVX_FLAG_ACCUMULATE into a dw pre-filled with 0.5."""
    from modules import _hip
    c, x, dz = _wgrad_case(name)
    dw = _wgrad(x, dz, c.K, c.N, _hip.FLAG_ACCUMULATE, 0.5)
    err = C.rel(dw.double() - 0.5, C.wgrad_reference(x, dz))
    print('linear_wgrad<%d> %s accumulate: dw - 0.5 vs float64 %.3e' % (c.vec, name, err))
    assert err < C.bound_for(c.K)


@pytest.mark.parametrize('accumulate', [False, True])
def test_wgrad_without_rows(accumulate):
    """rows == 0: dw becomes zero, or with MVX_FLAG_ACCUMULATE stays as it is, bit for bit; the workspace is not touched."""
    from modules import _hip
    K, N = 24, 16
    g = torch.Generator().manual_seed(6)
    _, x = C.slab(1, K, 0, K + 4, g, DEV, fill=NAN)          # valid pointers to operands of which no row may be read
    _, dz = C.slab(1, N, 0, N + 4, g, DEV, fill=NAN)
    before = torch.randn((N * K,), generator=g).to(DEV)
    dw = _wgrad(x, dz, K, N, _hip.FLAG_ACCUMULATE if accumulate else 0, before if accumulate else NAN, rows=0)
    assert torch.equal(dw.reshape(-1), before if accumulate else torch.zeros_like(before))


# ---- through modules/_hip.py on column-slice views ------------------------------------------------------------------------
@pytest.mark.parametrize('name,rows', [('twslice', 300), ('thead', 1)])
def test_wrapper_transposed_read_on_views(name, rows):
    """_hip.linear_forward(..., w_transposed=True) with x, the weight and the destination all column slices of wider buffers
    (_vptr / _ld of non-contiguous views; a one-row view too)."""
    from modules import _hip
    case = C.FWD_BY_NAME[name]
    x, w, _ = C.fwd_operands(case, rows, DEV, seed=7)
    assert not (rows > 1 and x.is_contiguous()) and not w.is_contiguous()
    ybuf = torch.full((rows + C.TAIL_ROWS, case.N + 40), NAN, device=DEV)
    out = ybuf[:rows, 32:32 + case.N]
    y, stats = _hip.linear_forward(x, w, None, relu=False, want_stats=False, w_transposed=True, out=out)
    torch.cuda.synchronize()
    assert stats is None and y.data_ptr() == out.data_ptr()
    _check_y('_hip.linear_forward %s rows %d' % (name, rows), ybuf, out, 32, C.fwd_reference(x, w, 1), case.K)


def test_wrapper_splitk_on_views():
    """The wrapper's own split-K workspace (K >= 256, no epilogue) with operands that are views."""
    from modules import _hip
    case = C.SPLITK_CASES[1]
    x, w, _ = _splitk_operands(case, seed=8)
    y, _ = _hip.linear_forward(x, w, None, relu=False, want_stats=False, w_transposed=True)
    torch.cuda.synchronize()
    err = C.rel(y, C.fwd_reference(x, w, 1))
    print('_hip.linear_forward split-K %s: y vs float64 %.3e' % (case.name, err))
    assert y.shape == (case.R, case.N) and err < C.bound_for(case.K)


@pytest.mark.parametrize('name,accumulate', [('slices', False), ('xslice1', True)])
def test_wrapper_wgrad_on_views(name, accumulate):
    """_hip.linear_wgrad on column-slice views of x and dz, fresh and accumulating."""
    from modules import _hip
    c, x, dz = _wgrad_case(name, seed=9)
    assert not x.is_contiguous() and not dz.is_contiguous()
    ref = C.wgrad_reference(x, dz)
    if accumulate:
        dw = torch.full((c.N, c.K), 0.5, device=DEV)
        assert _hip.linear_wgrad(x, dz, accumulate_into=dw, split=False) is None
        torch.cuda.synchronize()
        err = C.rel(dw.double() - 0.5, ref)
    else:
        dw = _hip.linear_wgrad(x, dz, split=False)
        torch.cuda.synchronize()
        err = C.rel(dw, ref)
    print('_hip.linear_wgrad %s: dw vs float64 %.3e' % (name, err))
    assert dw.shape == (c.N, c.K) and err < C.bound_for(c.K)
