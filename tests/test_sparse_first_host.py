"""CPU only: the numpy reference tests/sparse_ref.py of the sparse first CML layer against torch in float64 (conv3d of the scattered
dense grid, max_pool, autograd), the placement and exactness claims of tests/sparse_first_cases.py on the arrays the GPU tests
upload, and the argument checks of the entry points (a rejected call launches nothing, so it needs no GPU)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as tf

import sparse_first_cases as K
import sparse_ref as R

CASES = [(n, 1) for n in K.GEOMS] + [(n, 4) for n in K.GEOMS] + [('onetile', 16)]


def t64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def scattered(name, F, X):
    """The dense input [F][Cin][D][H][W] that VoxelNet.reindex would build from the voxel rows X."""
    g = K.geom(name, F)
    coords, vox_off = K.voxels(name, F)
    dense = np.zeros((F, X.shape[1], g.din, g.H, g.W))
    for v, (_, y, x, z) in enumerate(coords):
        dense[R.frame_of(v, vox_off), :, z, y, x] = X[v]
    return dense


# ---- the voxel sets -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,F', CASES)
def test_voxel_placement(name, F):
    g = K.geom(name, F)
    coords, vox_off = K.voxels(name, F)
    V = len(coords)
    assert 150 <= V <= 300 and V % 16 != 0                # V * 27 * C / 4 is no multiple of 256 for C = 16 and C = 64
    assert len(vox_off) == F + 1 and vox_off[0] == 0 and vox_off[-1] == V
    grid, occ, status = K.reference_grid(name, F)
    assert status == 0 and (grid >= 0).sum() == V == occ.sum(), 'unique sites, all in range'
    live = [f for f in range(F) if vox_off[f + 1] > vox_off[f]]
    assert sorted(set(range(F)) - set(live)) == sorted(K.EMPTY[F])
    for f in live:
        fg = grid[f * g.din:(f + 1) * g.din]
        assert fg[0, 0, 0] >= 0 and fg[-1, -1, -1] >= 0, 'corners'
        assert fg[-1, 3, 9] >= 0 and fg[0, 3, 9] >= 0, 'frame-leak pair'
        if name != 'onetile':
            assert all(fg[1, y, x] >= 0 for y in (7, 8) for x in (15, 16)) and fg[0, -1, -2] >= 0 and fg[0, 5, -1] >= 0
            z = g.din // 2
            assert fg[z, 16, 32] >= 0 and fg[z, 20, 17] >= 0 and (fg[z, 9:19, 17:48] >= 0).sum() == 1, 'lone voxel in a tile corner'
    # some site sums 27 terms: P = 1, bias = 0 counts them
    counts = R.sparse_output(np.ones((V, 27)), grid, np.zeros(1), g, False)[0]
    z0, y0, x0 = K.block_origin(name)
    d = (z0 + g.pd) // g.sd
    assert counts.max() == 27 == counts[live[0] * g.dout + d, y0 + 1, x0 + 1, 0]
    # a region of 3 x 3 tiles without a voxel in some plane.  Not on one tile; and the 3 planes x 3 x 3 tiles of 'ragged4' hold
    # the 3 x 3 x 3 block in every plane of its one frame: there the region is the empty frame of the 4-frame case.
    ty, tx = g.tiles
    if ty >= 3 and tx >= 3 and (name, F) != ('ragged4', 1):
        assert any(occ[p, i:i + 3, j:j + 3].sum() == 0 for p in range(F * g.din) for i in range(ty - 2) for j in range(tx - 2))
    # the out-of-range voxels of the index-grid test: one coordinate each, just outside
    bad, off = K.with_out_of_range(name, F)
    assert len(bad) == V + 3 and off[-1] == V + 3 and off[:-1] == vox_off[:-1]
    assert R.index_grid(bad, off, g.din, g.H, g.W)[2] == 1
    assert np.array_equal(R.index_grid(bad, off, g.din, g.H, g.W)[0], grid)
    assert bad[-3, 1] == -1 and bad[-2, 2] == g.W and bad[-1, 3] == g.din


# ---- sparse_output against conv3d ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,F', CASES)
def test_sparse_output_is_conv3d_of_the_scattered_grid(name, F):
    """Small-integer inputs: both sides are exact in float64, whatever their summation order."""
    g = K.geom(name, F)
    coords, _ = K.voxels(name, F)
    grid, _, _ = K.reference_grid(name, F)
    rng = np.random.default_rng(5)
    cin, cout = 3, 4
    X = rng.integers(-4, 5, (len(coords), cin)).astype(np.float64)
    Wt = rng.integers(-4, 5, (cout, cin, 3, 3, 3)).astype(np.float64)
    bias = rng.integers(-4, 5, cout).astype(np.float64)
    w_all = Wt.transpose(2, 3, 4, 0, 1).reshape(27 * cout, cin)         # row (kd * 9 + a * 3 + b) * cout + co = W[co][:][kd][a][b]
    out, sums = R.sparse_output(X @ w_all.T, grid, bias, g, False)
    want = tf.conv3d(t64(scattered(name, F, X)), t64(Wt), t64(bias), stride=(g.sd, 1, 1), padding=(g.pd, 1, 1))
    assert want.shape == (F, cout, g.dout, g.H, g.W)
    want = want.permute(0, 2, 3, 4, 1).reshape(F * g.dout, g.H, g.W, cout).numpy()
    assert np.array_equal(out, want)
    per_frame = want.reshape(F, -1, cout)
    assert np.array_equal(sums[:, 0], per_frame.sum(1)) and np.array_equal(sums[:, 1], (per_frame ** 2).sum(1))
    relu, rsums = R.sparse_output(X @ w_all.T, grid, bias, g, True)
    assert np.array_equal(relu, np.maximum(want, 0.0)) and np.array_equal(rsums[:, 0], np.maximum(per_frame, 0.0).sum(1))
    mag = R.sparse_output_magnitude(X @ w_all.T, grid, bias, g)
    assert (mag >= np.abs(out)).all() and np.array_equal(mag[grid_free(name, F)], np.broadcast_to(np.abs(bias), mag[grid_free(name, F)].shape))


def grid_free(name, F):
    """bool [F * dout][H][W]: sites of the first layer's output without a voxel under their taps (complement of the dilation)."""
    return K.reference_chain(name, F)[0][4][0] == 0


# ---- dilate and the tile flags against max pooling ----------------------------------------------------------------------------
def tile_pool(m):
    """[planes][H][W] 0/1 -> [planes][tiles_y][tiles_x]: any site of the 8 x 16 tile (partial tiles at the end)."""
    return tf.max_pool2d(m[:, None], (R.TH, R.TW), ceil_mode=True)[:, 0]


@pytest.mark.parametrize('name,F', CASES)
def test_dilate_is_max_pooling_per_frame(name, F):
    g = K.geom(name, F)
    H, W = g.H, g.W
    src = K.reference_grid(name, F)[0] >= 0
    for din, sd, pd, border, res in K.reference_chain(name, F):
        for mark in (False, True):
            m2, h2, t2 = res if mark == border else R.dilate(src, din, sd, pd, F, mark)
            dout = R.out_depth(din, sd, pd)
            want = tf.max_pool3d(t64(src).reshape(F, 1, din, H, W), 3, stride=(sd, 1, 1), padding=(pd, 1, 1)).reshape(F * dout, H, W)
            if mark:
                want[:, 0] = want[:, -1] = 1
                want[:, :, 0] = want[:, :, -1] = 1
            assert np.array_equal(m2, want.numpy().astype(np.uint8))
            assert np.array_equal(t2, tile_pool(want).numpy().astype(np.int32)), 'tile flags'
            grown = tf.max_pool2d(want[:, None], 3, stride=1, padding=1)[:, 0]        # a site within one step of the tile = in its halo
            assert np.array_equal(h2, tile_pool(grown).numpy().astype(np.int32)), 'halo flags'
            assert (h2 >= t2).all()
        src = res[0] != 0
    if name != 'onetile':
        # the voxel at (20, 17) reaches tile (2, 0) through its halo only
        mask, halo, tile = K.reference_chain(name, F)[0][4]
        assert (halo[:, 2, 0] > tile[:, 2, 0]).any()


@pytest.mark.parametrize('name,F', CASES)
def test_tile_dilate_and_tile_read(name, F):
    chain = K.reference_chain(name, F)
    (din1, sd1, pd1, _, l1), (din2, sd2, pd2, _, l2), (din3, sd3, pd3, _, l3) = chain
    # tile_dilate = self | max pooling over the tile grid with the layer's depth geometry
    got = R.tile_dilate(l1[2], l2[2], din2, din3, sd2, pd2, F)
    ty, tx = l1[2].shape[1:]
    pooled = tf.max_pool3d(t64(l1[2]).reshape(F, 1, din2, ty, tx), 3, stride=(sd2, 1, 1), padding=(pd2, 1, 1)).reshape(F * din3, ty, tx)
    assert np.array_equal(got, np.maximum(pooled.numpy(), l2[2]).astype(np.int32))
    assert np.array_equal(R.tile_dilate(l1[2], None, din2, din3, sd2, pd2, F), pooled.numpy().astype(np.int32))
    # tile_read: the safety property, stated from the reading side
    for (din, sd, pd, halo) in ((din2, sd2, pd2, l1[1]), (din3, sd3, pd3, l2[1])):
        dout = R.out_depth(din, sd, pd)
        read = R.tile_read(halo, din, dout, sd, pd, F)
        assert read.shape == halo.shape
        assert_read_covers(read, halo, din, dout, sd, pd, F)
        comp = R.computed_tiles(halo, din, dout, sd, pd, F)
        assert comp[:, 0].all() and comp[:, -1].all() and comp[:, :, 0].all() and comp[:, :, -1].all(), 'border units'
        if ty % 2 == 0:
            assert np.array_equal(comp[:, 0::2], comp[:, 1::2]), 'the two tile rows of a unit are computed together'
    if name == 'wide':
        read = R.tile_read(l1[1], din2, din3, sd2, pd2, F)
        assert (read == 0).any() and (read != 0).any()
        assert (read[:, 3, 4] == 0).all(), 'the tile no computed tile reads'
        # a unit computed because of its second tile row alone: without the odd tile rows' flags fewer tiles are read
        first_rows = l1[1].copy()
        first_rows[:, 1::2] = 0
        assert R.computed_tiles(l1[1], din2, din3, sd2, pd2, F)[:, 6:8, 4].any()
        assert not R.computed_tiles(first_rows, din2, din3, sd2, pd2, F)[:, 6:8, 4].any()
        assert (R.tile_read(first_rows, din2, din3, sd2, pd2, F)[:, 6:8, 3:6] < read[:, 6:8, 3:6]).any()


def assert_read_covers(read, halo, din, dout, sd, pd, F):
    """For every output plane d, valid tap kd and tile T with halo[src(d, kd)][T] != 0: every tile of the 3 x 3 neighbourhood of T
    in every valid source plane of d is flagged in ``read``."""
    _, ty, tx = halo.shape
    for f in range(F):
        for d in range(dout):
            srcs = [d * sd - pd + kd for kd in range(3) if 0 <= d * sd - pd + kd < din]
            for z in srcs:
                for i, j in np.argwhere(halo[f * din + z] != 0):
                    for z2 in srcs:
                        assert (read[f * din + z2, max(i - 1, 0):i + 2, max(j - 1, 0):j + 2] != 0).all(), (f, d, z, i, j, z2)


# ---- gather_dz against autograd -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,F', CASES)
def test_gather_dz_is_the_gradient_of_the_output_sum(name, F):
    """out = bias + index_add of P rows, the (site, row) pairs found from the OUTPUT side (every site looks up its 27 sources in the
    grid, tap by tap, as shifted views of the whole grid); d sum(out * dz) / dP must be G."""
    g = K.geom(name, F)
    coords, vox_off = K.voxels(name, F)
    grid, _, _ = K.reference_grid(name, F)
    C = 2
    rng = np.random.default_rng(11)
    dz = rng.integers(-8, 9, (F * g.dout, g.H, g.W, C)).astype(np.float64)
    site_idx, row_idx = [], []
    padded = np.full((grid.shape[0], g.H + 2, g.W + 2), -1, np.int64)
    padded[:, 1:-1, 1:-1] = grid
    sites = np.arange(F * g.dout * g.H * g.W).reshape(F * g.dout, g.H, g.W)
    for f in range(F):
        for d in range(g.dout):
            for kd in range(3):
                z = d * g.sd - g.pd + kd
                if not 0 <= z < g.din:
                    continue
                for a in range(3):
                    for b in range(3):
                        v = padded[f * g.din + z, a:a + g.H, b:b + g.W]
                        on = v >= 0
                        site_idx.append(sites[f * g.dout + d][on])
                        row_idx.append(v[on] * 27 + kd * 9 + a * 3 + b)
    site_idx, row_idx = torch.tensor(np.concatenate(site_idx)), torch.tensor(np.concatenate(row_idx))
    P = torch.zeros((len(coords) * 27, C), dtype=torch.float64, requires_grad=True)
    out = torch.zeros((sites.size, C), dtype=torch.float64).index_add(0, site_idx, P[row_idx])
    (out * t64(dz).reshape(-1, C)).sum().backward()
    assert np.array_equal(R.gather_dz(dz, coords, vox_off, g), P.grad.reshape(len(coords), 27 * C).numpy())
    # and the same pairs restate sparse_output
    Pv = rng.integers(-8, 9, (len(coords), 27 * C)).astype(np.float64)
    fwd = torch.zeros((sites.size, C), dtype=torch.float64).index_add(0, site_idx, t64(Pv).reshape(-1, C)[row_idx])
    assert np.array_equal(R.sparse_output(Pv, grid, np.zeros(C), g, False)[0].reshape(-1, C), fwd.numpy())


# ---- the exactness budget of the dyadic inputs ----------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [64, 16])
@pytest.mark.parametrize('name,F', [c for c in CASES if c[0] != 'wide'])
def test_dyadic_inputs_are_exact_in_f32(name, F, C):
    """P and bias are multiples of 1/4 with |.| <= 2, so a site's sum is a multiple of 1/4 with |acc| <= 27 * 2 + 2 = 56 = 224
    units: exact in f32 in any order.  acc^2 <= 50176 units of 1/16; a thread of mvx_sparse_conv_output adds at most 8 rows of
    them in f32: <= 401408 units, below 2^24, exact.  The f64 totals stay below 2^53 units: exact, so array_equal is the test."""
    g = K.geom(name, F)
    P, bias, dz = K.values(name, F, C, 'dyadic')
    for a in (P, bias, dz):
        assert np.array_equal(a * 4, np.round(a * 4)) and np.abs(a).max() <= 2 and np.array_equal(a, a.astype(np.float32))
    assert (bias < 0).any() and (bias > 0).any() and (bias == 0).any()
    grid, _, _ = K.reference_grid(name, F)
    mag = R.sparse_output_magnitude(P, grid, bias, g)
    assert mag.max() <= 56
    out, sums = R.sparse_output(P, grid, bias, g, False)
    assert np.array_equal(out * 4, np.round(out * 4)) and np.abs(out).max() <= 56
    assert 8 * (56 * 4) ** 2 == 401408 < 2 ** 24
    assert (np.abs(out) * 4).sum() < 2 ** 53 and ((out * 4) ** 2).sum() < 2 ** 53
    assert np.array_equal(sums * 16, np.round(sums * 16))
    # ReLU(bias) wherever no voxel lies under the taps: what the closed form of the BatchNorm sums and the unwritten tiles rely on
    free = grid_free(name, F)
    relu = R.sparse_output(P, grid, bias, g, True)[0]
    assert np.array_equal(relu[free], np.broadcast_to(np.maximum(bias, 0.0), relu[free].shape))
    assert not free.all() and (free.any() or (name, F) == ('onetile', 1))      # 210 voxels fill one frame of one tile


# ---- argument checks: rejected before any launch --------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments_before_any_launch():
    """Dummy non-null pointers and ONE bad argument per call (as tests/test_abi_and_host.py does for the convolutions): the
    argument error -1 comes back; a launch on these pointers would fault, and without a GPU it would return a HIP error."""
    from modules import Extension as X
    buf = ctypes.create_string_buffer(4096 + 64)
    p = (ctypes.addressof(buf) + 63) & ~63
    lib = X.lib
    good = dict(din=10, dout=5, h=37, w=53, cout=64, sd=2, pd=1, nf=1)

    def output_calls(din, dout, h, w, cout, sd, pd, nf, tf_ptr=p):
        return (lib.mvx_sparse_conv_output(p, p, p, p, p, din, dout, h, w, cout, sd, pd, 1, None) if nf == 1 else -1,
                lib.mvx_sparse_conv_output_frames(p, p, p, p, p, din, dout, h, w, cout, sd, pd, 1, nf, None),
                lib.mvx_sparse_conv_output_tiles_frames(p, p, p, p, p, din, dout, h, w, cout, sd, pd, 1, nf, tf_ptr, None))
    for cout in (48, 128):
        assert output_calls(**dict(good, cout=cout)) == (-1, -1, -1), cout
    for nf in (0, 17):
        assert output_calls(**dict(good, nf=nf)) == (-1, -1, -1), nf
    assert output_calls(**dict(good, dout=6)) == (-1, -1, -1)
    assert output_calls(**dict(good, dout=4)) == (-1, -1, -1)
    assert lib.mvx_sparse_conv_output_tiles_frames(p, p, p, p, p, 10, 5, 37, 53, 64, 2, 1, 1, 1, None, None) == -1
    # frame descriptors with 0 and 17 frames; a dout that does not follow from din, sd, pd
    for nf in (0, 17):
        fr = X.FramesDesc()
        fr.n_frames, fr.t = nf, 1
        assert lib.mvx_index_grid_frames(p, 1, 10, 37, 53, p, p, ctypes.addressof(fr), None) == -1
        assert lib.mvx_sparse_conv_gather_dz_frames(p, p, 1, p, 10, 5, 37, 53, 64, 2, 1, ctypes.addressof(fr), None) == -1
        assert lib.mvx_activity_dilate_frames(p, 1, 10, 5, 37, 53, 2, 1, 0, p, p, p, nf, None) == -1
        assert lib.mvx_tile_dilate_flags_frames(p, p, 10, 5, 37, 53, 2, 1, p, nf, None) == -1
        assert lib.mvx_tile_read_flags_frames(p, 10, 5, 37, 53, 2, 1, p, nf, None) == -1
    for dout in (4, 6):
        assert lib.mvx_sparse_conv_gather_dz_frames(p, p, 1, p, 10, dout, 37, 53, 64, 2, 1, None, None) == -1
        assert lib.mvx_sparse_conv_gather_dz(p, p, 1, p, 10, dout, 37, 53, 64, 2, 1, None) == -1
        assert lib.mvx_activity_dilate_frames(p, 1, 10, dout, 37, 53, 2, 1, 0, p, p, p, 1, None) == -1
        assert lib.mvx_activity_dilate(p, 1, 10, dout, 37, 53, 2, 1, 0, p, p, p, None) == -1
        assert lib.mvx_tile_dilate_flags_frames(p, p, 10, dout, 37, 53, 2, 1, p, 1, None) == -1
        assert lib.mvx_tile_read_flags_frames(p, 10, dout, 37, 53, 2, 1, p, 1, None) == -1
    for d, h, w, nf in ((0, 37, 53, 1), (10, 0, 53, 1), (10, 37, -1, 1), (10, 37, 53, 0), (-3, 37, 53, 2)):
        assert lib.mvx_index_grid_bytes_frames(d, h, w, nf) == 0
    assert lib.mvx_index_grid_bytes(0, 37, 53) == 0
    ty, tx = R.tiles_of(37, 53)
    assert lib.mvx_index_grid_bytes_frames(10, 37, 53, 4) == 4 * (40 * 37 * 53 + 40 * ty * tx + 4 + 4)
