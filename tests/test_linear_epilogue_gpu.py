"""The tile epilogue that linear_fwd (csrc/linear.hip) and linear_fwd_split (csrc/linear_split.hip) share
(rowgemm_tile_epilogue, csrc/rowgemm_common.h): bias + ReLU, the stores, the per-frame weighted BatchNorm sums and their
finalisation by the last workgroup.  Through the C ABI, on a frame set whose boundaries cut the 128-row blocks: 300 rows =
[real rows of frames 0, 1, 2 | one padded row per frame] with the real rows split at 100 and 130.  The three 128-row blocks:
rows 0..127 hold two segments (frame 0, then frame 1 up to row 127); rows 128..255 hold the last two rows of frame 1 and then
frame 2; the last, partial block 256..299 holds four segments -- the end of frame 2's real rows and the three padded rows, whose
frame order starts again at 0.

f32: (K, N) = (23, 32) the scalar loads and NT = 2, (24, 128) 16-byte loads and NT = 4, (24, 192) a half-empty last column block.
Split arithmetics 3 (bf16x6), 4 (fp16x3), 2 (bf16x3) with K = 72: not 128, so the call stays on linear_fwd_split, and a K tail in
both chunk sizes (64 and 32)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROWS, REAL, VOX, T = 300, [0, 100, 130, 297], [0, 100, 230, 300], 35
EPS = 1e-6

# y against float64, max error over max |y|.  Split codes: the bounds of tests/test_rowgemm_k128_gpu.py.  f32 (code 0): four
# times what the kernel gave on these inputs before the epilogue was shared (measured on an MI355X: 1.227e-07, 2.212e-07 and
# 1.769e-07 for the three shapes; F32_MEASURED is the largest); the factor leaves room for another seed and block order.
F32_MEASURED = 2.2124e-07
Y_BOUND = {0: 4 * F32_MEASURED, 3: 2e-6, 4: 4e-6, 2: 2e-4}


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


@pytest.mark.parametrize('split,K,N', [(0, 23, 32), (0, 24, 128), (0, 24, 192), (3, 72, 128), (3, 72, 192), (4, 72, 128),
                                       (4, 72, 192), (2, 72, 128), (2, 72, 192)])
def test_shared_tile_epilogue(split, K, N):
    from modules import _hip
    from modules import Extension as X
    F = 3
    g = torch.Generator().manual_seed(100 * split + N + K)
    x = torch.randn((ROWS, K), generator=g).to(DEV)
    w = (torch.randn((N, K), generator=g) * 0.2).to(DEV)
    b = (torch.randn((N,), generator=g) * 0.1).to(DEV)
    desc = X.FramesDesc.make(VOX, REAL, T)
    count = [float((VOX[f + 1] - VOX[f]) * T) for f in range(F)]
    # real rows weigh 1, a frame's padded row stands for the rest of its population
    row_w = torch.ones((ROWS,), device=DEV)
    row_w[-F:] = torch.tensor([count[f] - (REAL[f + 1] - REAL[f]) for f in range(F)])
    ldy = N + 8                                           # the columns behind N must stay untouched
    y_buf = torch.full((ROWS, ldy), float('nan'), device=DEV)
    st = torch.zeros((F, _hip.STATS_REPLICAS, 2, N), dtype=torch.float64, device=DEV)
    cnt = torch.zeros((1,), dtype=torch.float64, device=DEV)
    mi = torch.empty((F, 2, N), device=DEV)
    flags = _hip.split_flags(split, True) | _hip.FLAG_RELU
    X.check(X.lib.mvx_linear_forward_bn_frames(X.ptr(x), K, X.ptr(w), K, 0, X.ptr(b), X.ptr(y_buf), ldy, X.ptr(st), X.ptr(row_w),
                                               ROWS, K, N, flags, X.ptr(cnt), EPS, X.ptr(mi), desc.ref(), X.ROWS_FUSION,
                                               X.stream()), 'mvx_linear_forward_bn_frames')
    torch.cuda.synchronize()
    y = y_buf[:, :N]
    assert torch.isnan(y_buf[:, N:]).all() and not torch.isnan(y).any()
    ref = torch.relu(x.double() @ w.double().t() + b.double())
    err_y = rel(y, ref)
    print('split %d K %d N %d: y vs float64 %.3e' % (split, K, N, err_y))
    assert err_y < Y_BOUND[split]
    # each frame's sums are the weighted sums of the y that was written; mean and inverse std follow from them
    yw = y.double() * row_w.double()[:, None]
    for f in range(F):
        rows_f = torch.zeros((ROWS,), dtype=torch.bool, device=DEV)
        rows_f[REAL[f]:REAL[f + 1]] = True
        rows_f[ROWS - F + f] = True
        s1, s2 = yw[rows_f].sum(0), (yw[rows_f] * y[rows_f].double()).sum(0)
        mean = s1 / count[f]
        inv = 1.0 / torch.sqrt((s2 / count[f] - mean * mean).clamp_min(0.0) + EPS)
        errs = (rel(st[f].sum(0)[0], s1), rel(st[f].sum(0)[1], s2), rel(mi[f, 0], mean), rel(mi[f, 1], inv))
        print('  frame %d: sums %.3e %.3e, mean %.3e, inverse std %.3e' % ((f,) + errs))
        assert errs[0] < 1e-12 and errs[1] < 1e-12
        assert errs[2] < 2e-5 and errs[3] < 2e-5


@pytest.mark.parametrize('split,K,N', [(0, 24, 128), (3, 72, 128)])
def test_frame_without_voxels_gets_finite_statistics(split, K, N):
    """The middle frame has no voxels: MVX_ROWS_FUSION still stores its shared padded row (weight 0, population 0).  The
    finalisation by the last workgroup gives that frame mean 0 and inverse deviation 1 / sqrt(eps) instead of 0 / 0; the live
    frames keep their statistics."""
    from modules import _hip
    from modules import Extension as X
    F = 3
    real, vox = [0, 100, 100, 297], [0, 100, 100, 170]
    g = torch.Generator().manual_seed(7 + split)
    x = torch.randn((ROWS, K), generator=g).to(DEV)
    w = (torch.randn((N, K), generator=g) * 0.2).to(DEV)
    b = (torch.randn((N,), generator=g) * 0.1).to(DEV)
    desc = X.FramesDesc.make(vox, real, T)
    count = [float((vox[f + 1] - vox[f]) * T) for f in range(F)]
    row_w = torch.ones((ROWS,), device=DEV)
    row_w[-F:] = torch.tensor([count[f] - (real[f + 1] - real[f]) for f in range(F)])
    assert count[1] == 0 and float(row_w[-2]) == 0
    y = torch.full((ROWS, N), float('nan'), device=DEV)
    st = torch.zeros((F, _hip.STATS_REPLICAS, 2, N), dtype=torch.float64, device=DEV)
    cnt = torch.zeros((1,), dtype=torch.float64, device=DEV)
    mi = torch.full((F, 2, N), float('nan'), device=DEV)
    flags = _hip.split_flags(split, True) | _hip.FLAG_RELU
    X.check(X.lib.mvx_linear_forward_bn_frames(X.ptr(x), K, X.ptr(w), K, 0, X.ptr(b), X.ptr(y), N, X.ptr(st), X.ptr(row_w),
                                               ROWS, K, N, flags, X.ptr(cnt), EPS, X.ptr(mi), desc.ref(), X.ROWS_FUSION,
                                               X.stream()), 'mvx_linear_forward_bn_frames')
    torch.cuda.synchronize()
    assert not torch.isnan(y).any() and not torch.isnan(mi).any(), 'NaN statistics for the frame without population'
    assert (mi[1, 0] == 0).all() and rel(mi[1, 1], torch.full((N,), EPS ** -0.5, dtype=torch.float64, device=DEV)) < 1e-6
    yw = y.double() * row_w.double()[:, None]
    for f in (0, 2):
        rows_f = torch.zeros((ROWS,), dtype=torch.bool, device=DEV)
        rows_f[real[f]:real[f + 1]] = True
        rows_f[ROWS - F + f] = True
        s1, s2 = yw[rows_f].sum(0), (yw[rows_f] * y[rows_f].double()).sum(0)
        mean = s1 / count[f]
        inv = 1.0 / torch.sqrt((s2 / count[f] - mean * mean).clamp_min(0.0) + EPS)
        errs = (rel(mi[f, 0], mean), rel(mi[f, 1], inv))
        print('split %d frame %d: mean %.3e, inverse std %.3e' % ((split, f) + errs))
        assert errs[0] < 2e-5 and errs[1] < 2e-5
