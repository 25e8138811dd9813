"""tests/rpn_layout_cases.py without a GPU: the numpy index arithmetic against torch's pixel_unshuffle / pixel_shuffle, against a
float64 conv_transpose2d with kernel = stride (the (i, j) order of d2s_rows), and against _to_planes of tests/test_rpn_gpu.py (the
interleave of the depth planes)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import rpn_layout_cases as L
from test_rpn_gpu import _to_planes


@pytest.mark.parametrize('case', L.S2D_CASES, ids=str)
def test_space_to_depth_is_pixel_unshuffle(case):
    F, P, h, w, C = case
    x = L.ordinal((F * P, h, w, C))
    z = L.space_to_depth(x, F, P)
    assert z.shape == (F, h // 2, w // 2, 4 * P * C)
    # the frame's planes as one NCHW image with channel d*C + c; pixel_unshuffle numbers its channels ch*4 + 2 pr + pc
    img = torch.from_numpy(x).view(F, P, h, w, C).permute(0, 1, 4, 2, 3).reshape(F, P * C, h, w)
    u = Fn.pixel_unshuffle(img, 2).view(F, P * C, 4, h // 2, w // 2).permute(0, 3, 4, 2, 1).reshape(z.shape)
    assert np.array_equal(z, u.numpy())
    assert np.array_equal(L.depth_to_space(z, F, P), x)
    assert sorted(z.reshape(-1).tolist()) == list(range(x.size))


def test_planes_interleave_is_to_planes():
    """The CML output [F*2][H][W][64] is the (F, 128, H, W) BEV map with channel = c*2 + d: block p of the space-to-depth image
    holds, at d*64 + c, channel c*2 + d of the pixel_unshuffle of that map."""
    F, P, h, w, C = L.S2D_CASES[3]
    assert (P, C) == (2, 64)
    mid = torch.from_numpy(L.ordinal((F, 128, h, w)))
    z = L.space_to_depth(_to_planes(mid).numpy(), F, P).reshape(F, h // 2, w // 2, 4, P, C)
    u = Fn.pixel_unshuffle(mid, 2).view(F, C, P, 4, h // 2, w // 2)            # channel (c*2 + d)*4 + p
    assert np.array_equal(z, u.permute(0, 4, 5, 3, 2, 1).numpy())


@pytest.mark.parametrize('s', L.D2S_S)
@pytest.mark.parametrize('shape', L.D2S_SHAPES, ids=str)
def test_d2s_is_pixel_shuffle_and_conv_transpose(shape, s):
    F, h, w, C = shape
    t = L.ordinal((F * h * w, s * s * C))
    rows = L.d2s_rows(t, F, h, w, s)
    assert rows.shape == (F * h * s * w * s, C)
    # pixel_shuffle takes channel c*s*s + i*s + j
    img = torch.from_numpy(t).view(F, h, w, s * s, C).permute(0, 4, 3, 1, 2).reshape(F, C * s * s, h, w)
    ps = Fn.pixel_shuffle(img, s).permute(0, 2, 3, 1).reshape(rows.shape)
    assert np.array_equal(rows, ps.numpy())
    assert np.array_equal(L.s2d_rows(rows, F, h, w, s), t)
    # ConvTranspose2d(ci, co, s, s): out[f, co, y*s + i, x*s + j] = sum_ci x[f, ci, y, x] W[ci, co, i, j]; as a row GEMM the
    # weight row (i*s + j)*co_n + co holds W[:, co, i, j]
    rng = np.random.default_rng(s + C)
    ci, co = 3, min(C, 8)
    x = torch.from_numpy(rng.standard_normal((F, ci, h, w)))
    W = torch.from_numpy(rng.standard_normal((ci, co, s, s)))
    Wg = W.permute(2, 3, 1, 0).reshape(s * s * co, ci)
    tg = x.permute(0, 2, 3, 1).reshape(F * h * w, ci) @ Wg.t()
    up = Fn.conv_transpose2d(x, W, stride=s).permute(0, 2, 3, 1).reshape(F * h * s * w * s, co)
    assert np.abs(L.d2s_rows(tg.numpy(), F, h, w, s) - up.numpy()).max() < 1e-12


def test_slices_and_normalise():
    assert L.slices(4) == [(4, 0), (12, 0), (12, 4), (12, 8), (768, 0), (768, 4), (768, 764)]
    assert L.slices(256) == [(256, 0), (264, 0), (264, 4), (264, 8), (768, 0), (768, 4), (768, 512)]
    mi = L.mean_inv(8, 3, 0)
    assert mi.dtype == np.float32 and len({tuple(mi[f, 0]) for f in range(3)}) == 3
    v = L.ordinal((6, 8))
    frame = np.repeat(np.arange(3), 2)
    out = L.normalise_f32(v, mi, frame)
    assert out.dtype == np.float32
    exact = (v.astype(np.float64) - mi[frame, 0]) * mi[frame, 1]
    assert np.abs(out - exact).max() <= 2 * 2.0 ** -24 * np.abs(exact).max()
    buf = L.in_slice(out, 8, 16, 4)
    assert np.isnan(buf[:, :4]).all() and np.isnan(buf[:, 12:]).all() and np.isnan(buf[6:]).all() and np.array_equal(buf[:6, 4:12], out)


def test_stats_cases():
    """40 000 rows per frame pass the cap of 512 blocks per frame wherever a block takes fewer than 79 rows per trip (C >= 48);
    at C = 4 and 12 a block takes 256 and 85.  1 237 rows pass it where a block takes one row (C >= 768)."""
    assert len(L.STATS_CASES) == 24
    capped = {(c.C, c.per) for c in L.STATS_CASES if L.stats_blocks(c.per, c.C) > L.STATS_BLOCK_CAP}
    assert capped == {(C, 40000) for C in (48, 256, 768, 1024)} | {(768, 1237), (1024, 1237)}
