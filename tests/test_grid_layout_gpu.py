"""csrc/scatter.hip through the C ABI: voxel rows <-> channels-last grid (mvx_scatter_voxels with its occupancy histogram and site
bits, mvx_gather_voxels) and channels-last grid <-> bird's-eye-view map (mvx_cl_to_bev_frames both ways, mvx_bev_to_cl_broadcast).
The kernels move data and count integers: every comparison is array_equal against the numpy / torch statement in this file.
Outputs carry a guard tail and start as NaN (floats) or -7 (integers), unless the call itself is to clear them."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, H, W = 3, 21, 37
GUARD = 64            # elements
POISON = -7
SENTINEL = 123.5


def dev():
    return torch.device('cuda')


def tile_shape():
    from modules import Extension as X
    th, tw = ctypes.c_int32(0), ctypes.c_int32(0)
    X.lib.mvx_conv3d_tile_shape(ctypes.byref(th), ctypes.byref(tw))
    return th.value, tw.value


def sites(C, with_bad):
    """About 300 unique sites of the D x H x W grid as coords (b, ix, iy, iz) with ix < H, iy < W, iz < D, random rows, and (with_bad)
    three rows one step outside the grid -- ix = -1, iy = W, iz = D -- at the start, in the middle and at the end."""
    g = np.random.default_rng(C)
    flat = g.choice(D * H * W, 300, replace=False)
    iz, ix, iy = np.unravel_index(flat, (D, H, W))
    coords = np.stack([np.zeros_like(ix), ix, iy, iz], 1).astype(np.int64)
    if with_bad:
        bad = np.array([[0, -1, 5, 1], [0, 4, W, 2], [0, 7, 9, D]], np.int64)
        coords = np.concatenate([bad[0:1], coords[:150], bad[1:2], coords[150:], bad[2:3]])
    feat = g.standard_normal((len(coords), C)).astype(np.float32)
    return coords, feat


def inside(coords):
    return (coords[:, 1] >= 0) & (coords[:, 1] < H) & (coords[:, 2] >= 0) & (coords[:, 2] < W) & (coords[:, 3] >= 0) & (coords[:, 3] < D)


def scatter_ref(coords, feat, grid):
    """grid [D][H][W][C] (modified), occupancy [D][ty][tx], site bits [D][H][ceil(W / 32)], status."""
    th, tw = tile_shape()
    ok = inside(coords)
    c = coords[ok]
    grid[c[:, 3], c[:, 1], c[:, 2]] = feat[ok]
    occ = np.zeros((D, -(-H // th), -(-W // tw)), np.int32)
    np.add.at(occ, (c[:, 3], c[:, 1] // th, c[:, 2] // tw), 1)
    bits = np.zeros((D, H, -(-W // 32)), np.uint32)
    np.bitwise_or.at(bits, (c[:, 3], c[:, 1], c[:, 2] >> 5), (np.uint32(1) << (c[:, 2] & 31).astype(np.uint32)))
    return grid, occ, bits, int(not ok.all())


def scatter(coords, feat, C, zero_grid, grid0, maps=True, n_voxels=None):
    """-> (rc, grid with guard, occupancy with guard, bits with guard, status[2]) as numpy."""
    from modules import Extension as X
    th, tw = tile_shape()
    n_occ, n_bits = D * -(-H // th) * -(-W // tw), D * H * -(-W // 32)
    grid = torch.full((D * H * W * C + GUARD,), grid0, dtype=torch.float32, device=dev())
    occ = torch.full((n_occ + GUARD,), POISON, dtype=torch.int32, device=dev())
    bits = torch.full((n_bits + GUARD,), POISON, dtype=torch.int32, device=dev())
    status = torch.tensor([0, POISON], dtype=torch.int32, device=dev())
    d_feat, d_coords = torch.from_numpy(feat).to(dev()), torch.from_numpy(coords).to(dev())
    V = len(coords) if n_voxels is None else n_voxels
    rc = X.lib.mvx_scatter_voxels(X.ptr(d_feat), X.ptr(d_coords), X.ptr(grid), V, C, D, H, W, int(zero_grid), X.ptr(status),
                                  X.ptr(occ) if maps else None, th, tw, X.ptr(bits) if maps else None, X.stream())
    torch.cuda.synchronize()
    return rc, grid.cpu().numpy(), occ.cpu().numpy(), bits.cpu().numpy().view(np.uint32), status.cpu().numpy()


def check_maps(occ, bits, occ_ref, bits_ref):
    assert np.array_equal(occ[:occ_ref.size], occ_ref.ravel()) and (occ[occ_ref.size:] == POISON).all()
    assert np.array_equal(bits[:bits_ref.size], bits_ref.ravel()) and (bits[bits_ref.size:].view(np.int32) == POISON).all()


@pytest.mark.parametrize('C', [4, 64, 128])
def test_scatter_with_rows_outside_the_grid(C):
    coords, feat = sites(C, True)
    assert len(coords) == 303 and inside(coords).sum() == 300
    n = D * H * W * C
    want, occ_ref, bits_ref, st = scatter_ref(coords, feat, np.zeros((D, H, W, C), np.float32))
    assert st == 1 and occ_ref.sum() == 300 and occ_ref.max() > 1
    assert sum(bin(int(b)).count('1') for b in bits_ref.ravel()) == 300 and (bits_ref[..., 1] >> (W - 32)).max() == 0
    # zero_grid = 1: the whole grid is cleared first; the three skipped rows change nothing, anywhere
    rc, grid, occ, bits, status = scatter(coords, feat, C, 1, float('nan'))
    assert rc == 0 and status.tolist() == [1, POISON]
    assert np.array_equal(grid[:n], want.ravel()) and np.isnan(grid[n:]).all()
    check_maps(occ, bits, occ_ref, bits_ref)
    # zero_grid = 0: whatever the grid held survives off the sites
    rc, grid, occ, bits, status = scatter(coords, feat, C, 0, SENTINEL)
    want_kept = scatter_ref(coords, feat, np.full((D, H, W, C), SENTINEL, np.float32))[0]
    assert rc == 0 and status.tolist() == [1, POISON]
    assert np.array_equal(grid[:n], want_kept.ravel()) and (grid[n:] == SENTINEL).all()
    assert (want_kept == SENTINEL).all(-1).sum() == D * H * W - 300
    check_maps(occ, bits, occ_ref, bits_ref)
    # without the maps: the same grid
    rc, grid, occ, bits, status = scatter(coords, feat, C, 1, float('nan'), maps=False)
    assert rc == 0 and np.array_equal(grid[:n], want.ravel()) and (occ == POISON).all() and (bits.view(np.int32) == POISON).all()


@pytest.mark.parametrize('C', [4, 64, 128])
def test_scatter_inside_the_grid_and_empty(C):
    coords, feat = sites(C, False)
    n = D * H * W * C
    want, occ_ref, bits_ref, st = scatter_ref(coords, feat, np.zeros((D, H, W, C), np.float32))
    rc, grid, occ, bits, status = scatter(coords, feat, C, 1, float('nan'))
    assert st == 0 and rc == 0 and status.tolist() == [0, POISON]
    assert np.array_equal(grid[:n], want.ravel()) and np.isnan(grid[n:]).all()
    check_maps(occ, bits, occ_ref, bits_ref)
    # n_voxels = 0: the grid and both maps are cleared, nothing else happens
    rc, grid, occ, bits, status = scatter(coords, feat, C, 1, float('nan'), n_voxels=0)
    assert rc == 0 and status.tolist() == [0, POISON]
    assert not grid[:n].any() and np.isnan(grid[n:]).all()
    check_maps(occ, bits, np.zeros_like(occ_ref), np.zeros_like(bits_ref))


@pytest.mark.parametrize('C', [4, 64, 128])
def test_gather_rows(C):
    from modules import Extension as X
    coords, _ = sites(C, True)
    V = len(coords)
    g = np.random.default_rng(100 + C)
    grid = g.standard_normal((D, H, W, C)).astype(np.float32)
    ok = inside(coords)
    want = np.zeros((V, C), np.float32)
    want[ok] = grid[coords[ok, 3], coords[ok, 1], coords[ok, 2]]
    assert (want[ok] != 0).all() and (~ok).sum() == 3
    feat = torch.full((V + 1, C), float('nan'), dtype=torch.float32, device=dev())          # one guard row
    d_grid = torch.cat([torch.from_numpy(grid).to(dev()).ravel(), torch.full((GUARD,), float('nan'), device=dev())])
    d_coords = torch.from_numpy(coords).to(dev())
    rc = X.lib.mvx_gather_voxels(X.ptr(d_grid), X.ptr(d_coords), X.ptr(feat), V, C, D, H, W, X.stream())
    torch.cuda.synchronize()
    got = feat.cpu().numpy()
    assert rc == 0 and np.array_equal(got[:V], want) and np.isnan(got[V]).all()
    # n_voxels = 0 writes nothing
    feat.fill_(float('nan'))
    assert X.lib.mvx_gather_voxels(X.ptr(d_grid), X.ptr(d_coords), X.ptr(feat), 0, C, D, H, W, X.stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(feat).all()


# ---- channels-last grid <-> bird's-eye-view map: BEV channel = c * D + d ----------------------------------------------------------
SHAPES = [(1, 2, 5, 37, 64), (3, 2, 7, 33, 48), (2, 5, 3, 70, 20)]          # (F, D, H, W, C): W and C off multiples of the 32 x 32 tile


def cl_and_bev(F, Dd, Hh, Ww, C):
    """cl [F * D][H][W][C] and the reference's view of it, bev [F][C * D][H][W] (VoxelNet.py:36: NCDHW reshaped)."""
    g = torch.Generator().manual_seed(F * 1000 + Ww)
    cl = torch.randn((F * Dd, Hh, Ww, C), generator=g)
    bev = cl.reshape(F, Dd, Hh, Ww, C).permute(0, 4, 1, 2, 3).reshape(F, C * Dd, Hh, Ww).contiguous()
    assert bev[F - 1, 3 * Dd + 1, 2, 5] == cl[(F - 1) * Dd + 1, 2, 5, 3]          # channel = c * D + d
    return cl, bev


def poisoned(n):
    return torch.full((n + GUARD,), float('nan'), dtype=torch.float32, device=dev())


@pytest.mark.parametrize('F,Dd,Hh,Ww,C', SHAPES)
def test_cl_to_bev_frames_both_directions(F, Dd, Hh, Ww, C):
    from modules import Extension as X
    cl, bev = cl_and_bev(F, Dd, Hh, Ww, C)
    n = cl.numel()
    d_cl, d_bev = cl.to(dev()), bev.to(dev())
    out = poisoned(n)
    assert X.lib.mvx_cl_to_bev_frames(X.ptr(d_cl), X.ptr(out), Dd, Hh, Ww, C, 0, F, X.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:n].cpu(), bev.ravel()) and torch.isnan(out[n:]).all()
    back = poisoned(n)
    assert X.lib.mvx_cl_to_bev_frames(X.ptr(back), X.ptr(d_bev), Dd, Hh, Ww, C, 1, F, X.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(back[:n].cpu(), cl.ravel()) and torch.isnan(back[n:]).all()
    if F == 1:                                   # the one-frame entry point is the same kernel
        out.fill_(float('nan'))
        assert X.lib.mvx_cl_to_bev(X.ptr(d_cl), X.ptr(out), Dd, Hh, Ww, C, 0, X.stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(out[:n].cpu(), bev.ravel()) and torch.isnan(out[n:]).all()


@pytest.mark.parametrize('copies', [1, 3, 16])
@pytest.mark.parametrize('F,Dd,Hh,Ww,C', SHAPES[:1] + SHAPES[2:])
def test_bev_to_cl_broadcast(F, Dd, Hh, Ww, C, copies):
    """One (C * D, H, W) map -> `copies` channels-last frames: the reverse transposition, repeated."""
    from modules import Extension as X
    cl, bev = cl_and_bev(1, Dd, Hh, Ww, C)
    n = cl.numel()
    out = poisoned(copies * n)
    d_bev = bev.to(dev())
    assert X.lib.mvx_bev_to_cl_broadcast(X.ptr(d_bev), X.ptr(out), Dd, Hh, Ww, C, copies, X.stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got[:copies * n].reshape(copies, -1), cl.ravel().expand(copies, n)) and torch.isnan(got[copies * n:]).all()
