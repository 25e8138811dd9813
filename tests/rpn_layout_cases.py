"""Case tables and numpy references of the RPN's layout kernels (csrc/rpn.hip) for tests/test_rpn_layout_gpu.py; checked without a
GPU by tests/test_rpn_layout_host.py.  numpy only.  The references are plain index arithmetic written from the layout comments of
csrc/rpn.hip and modules/rpn_frames.py:

  space_to_depth   in [F*P][H][W][C] -> out [F][H/2][W/2][4][P][C]: pixel (y, x) of the image holds the four input pixels
                   (2y + pr, 2x + pc) as channel block p = 2 pr + pc; the P depth planes of a frame lie side by side inside a
                   block, plane-major.
  d2s              t [F][h][w][s*s][C] (the row GEMM of a transposed convolution with kernel = stride = s, block (i, j) at
                   i*s + j) -> pixel (y*s + i, x*s + j) of the [F][h*s][w*s] map, written as rows of ld floats into the columns
                   [off, off + C).
  strided          y [rows][C] -> columns [off, off + C) of rows of ld floats; the frames are equal shares of the rows.
The last two normalise on the way, out = (v - mean_f) * inv_f in f32: two rounded operations and nothing to contract, so the
reference does the same two operations in numpy float32 and the comparison is equality.

Values are ORDINAL (element = its own flat index, exact in f32 below 2^24): a misplaced element names where it came from."""
import collections

import numpy as np

EPS = 1e-6
BOUND = 2e-5                           # mean and inverse deviation against float64 (the project's bound, tests/test_conv3d_gpu.py)

# (F, planes, h, w, C) of mvx_space_to_depth_frames
S2D_CASES = [(1, 1, 2, 2, 4), (3, 2, 6, 10, 8), (2, 1, 4, 6, 64), (3, 2, 10, 14, 64)]
S2D_REJECTED = [(1, 1, 3, 4, 4), (1, 1, 4, 5, 4), (2, 2, 4, 4, 6)]      # odd h, odd w, C % 4 != 0

# (F, h, w, C) and s of mvx_d2s_bn_apply_frames; the strided form takes rows = F * h * w of the same shapes
D2S_SHAPES = [(1, 1, 1, 4), (3, 3, 5, 8), (2, 5, 3, 256)]
D2S_S = (1, 2, 4)

# mvx_row_stats_frames
STATS_C = (4, 12, 48, 256, 768, 1024)
STATS_ROWS = (1, 7, 1237, 40000)
STATS_F = 3
STATS_SCALE, STATS_OFFSET = (1.0, 2.5, 0.4), (0.3, -0.8, 1.5)
STATS_BLOCK_CAP = 512


def stats_blocks(per, C):
    """Blocks per frame that mvx_row_stats_frames wants before its cap: ceil(rows per frame / rpi), rpi = max(1, 256 / (C/4))."""
    rpi = max(1, 256 // (C // 4))
    return -(-per // rpi)


def slices(C):
    """(ld_out, col_offset) with ld_out in {C, C + 8, 768} and col_offset in {0, 4, ld_out - C}, where the slice fits."""
    out = []
    for ld in (C, C + 8, 768):
        for off in (0, 4, ld - C):
            if ld >= C and off + C <= ld and (ld, off) not in out:
                out.append((ld, off))
    return out


def ordinal(shape):
    n = int(np.prod(shape))
    assert n < 1 << 24
    return np.arange(n, dtype=np.float32).reshape(shape)


# ---- references ------------------------------------------------------------------------------------------------------------
def space_to_depth(x, F, P):
    """[F*P][H][W][C] -> [F][H/2][W/2][4*P*C]"""
    _, H, W, C = x.shape
    v = x.reshape(F, P, H // 2, 2, W // 2, 2, C)               # f d y pr x pc c
    return v.transpose(0, 2, 4, 3, 5, 1, 6).reshape(F, H // 2, W // 2, 4 * P * C)


def depth_to_space(z, F, P):
    """The way back: [F][H/2][W/2][4*P*C] -> [F*P][H][W][C]"""
    _, H2, W2, K = z.shape
    C = K // (4 * P)
    v = z.reshape(F, H2, W2, 2, 2, P, C)                       # f y x pr pc d c
    return v.transpose(0, 5, 1, 3, 2, 4, 6).reshape(F * P, 2 * H2, 2 * W2, C)


def d2s_rows(t, F, h, w, s):
    """[F][h][w][s*s][C] (any shape of that many elements) -> the rows [F*h*s*w*s][C] of the up-sampled map"""
    C = t.size // (F * h * w * s * s)
    v = t.reshape(F, h, w, s, s, C)                            # f y x i j c
    return v.transpose(0, 1, 3, 2, 4, 5).reshape(F * h * s * w * s, C)


def s2d_rows(rows, F, h, w, s):
    """The inverse gather: rows [F*h*s*w*s][C] -> [F*h*w][s*s*C]"""
    C = rows.shape[-1]
    v = rows.reshape(F, h, s, w, s, C)                         # f y i x j c
    return v.transpose(0, 1, 3, 2, 4, 5).reshape(F * h * w, s * s * C)


def normalise_f32(v, mi, frame):
    """(v - mean) * inv with the statistics mi (F, 2, C) of each row's frame: two f32 operations, rounded one by one."""
    v, mi = np.asarray(v, np.float32), np.asarray(mi, np.float32)
    d = (v - mi[frame, 0]).astype(np.float32)
    return (d * mi[frame, 1]).astype(np.float32)


def in_slice(vals, rows_total, ld, off, fill=np.nan):
    """The (rows, C) values as columns [off, off + C) of a (rows_total, ld) buffer of ``fill``."""
    buf = np.full((rows_total, ld), fill, np.float32)
    buf[:vals.shape[0], off:off + vals.shape[1]] = vals
    return buf


def mean_inv(C, F, seed):
    """Statistics of F distinct frames: a kernel that reads another frame's row of mi gives other numbers."""
    rng = np.random.default_rng(seed)
    mi = np.stack([rng.standard_normal((F, C)) * 50.0 + 100.0 * np.arange(F)[:, None], rng.uniform(0.5, 2.0, (F, C))], 1)
    return mi.astype(np.float32)


Stats = collections.namedtuple('Stats', 'C per')
STATS_CASES = [Stats(C, per) for C in STATS_C for per in STATS_ROWS]
