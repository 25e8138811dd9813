"""CPU only: the input builders of tests/voxelize_cases.py give what they claim (the GPU tests upload exactly these arrays), the
batch layouts are stated once from the per-frame oracle, and the argument checks of the voxelizer and of csrc/scatter.hip return
before any launch (a rejected call needs no GPU)."""
import ctypes

import numpy as np
import pytest
import torch

import mvx_oracle as O
import voxelize_cases as K


def members(points, T=None):
    """{cell: member count} of a point set according to the oracle's index math."""
    idx = O.voxel_index(points[:, :3], K.RNG, K.SIZE)
    cells, n = np.unique(idx, axis=0, return_counts=True)
    return {tuple(c): int(k) for c, k in zip(cells.tolist(), n)}


# ---- builders -------------------------------------------------------------------------------------------------------------------
def test_crowd_has_exactly_the_member_counts():
    pts = K.crowd(1)
    assert pts.shape == (563, 6) and pts.dtype == np.float32 and sum(K.COUNTS) == 563
    m = members(pts)
    assert m == {tuple(int(c) for c in K.crowd_cell(k)): n for k, n in enumerate(K.COUNTS)}
    assert not np.array_equal(K.crowd(1), K.crowd(2)) and np.array_equal(K.crowd(1), K.crowd(1))


@pytest.mark.parametrize('T', K.T_VALUES)
def test_kept_counts_are_the_member_counts_clipped_at_T(T):
    """'single' = crowd + edges + uniform: the oracle keeps min(n, T) points of every crowd cell, and every route of the gather is
    taken: n <= 16 and n <= T (narrow group), T < n <= 16 (wide although small; T = 5 only), 16 < n <= 64 (ranked bucket),
    n > 64 (ordered walk)."""
    fs = K.case('single')
    assert fs.pcd.shape == (1, K.CAP, 6) and fs.n_points[0] == 563 + len(K.EDGE_POINTS) + 400
    frames = K.oracle_frames('single', T, 9)
    _, idx, cnt = frames[0]
    got = {tuple(i): int(c) for i, c in zip(idx.tolist(), cnt)}
    all_members = members(K.stream(fs, 0))
    for k, n in enumerate(K.COUNTS):
        cell = tuple(int(c) for c in K.crowd_cell(k))
        assert all_members[cell] == n and got[cell] == min(n, T)
    assert got[(0, 0, 0)] == min(3, T) and got[(-500, 0, 0)] == 1 and got[(0, 0, -67)] == 1
    n = np.array(list(all_members.values()))
    routes = [(n <= 16) & (n <= T), (n <= 16) & (n > T), (n > 16) & (n <= 64), n > 64]
    assert [bool(r.any()) for r in routes] == [True, T < 16, True, True]
    small = np.array([v for c, v in all_members.items() if c[0] >= 100 or c[1] >= 12])          # the uniform part
    assert ((small >= 1) & (small <= 4)).mean() > 0.9 and small.max() > 1


def test_edges_have_the_stated_indices():
    e = K.edges()
    assert np.array_equal(O.voxel_index(e[:, :3], K.RNG, K.SIZE), K.edge_indices())
    assert e[3, 0] == np.float32(K.LO[0] + 0.6) and int(0.6 / 0.2) == 2          # the f32 value decides, not the decimal
    assert np.abs(K.edge_indices()).max() < (1 << 20), 'inside the 21-bit key range: not flagged'
    assert (np.array(K.edge_indices()) == 0).all(1).sum() == 3, 'the points that share cell (0, 0, 0)'


def test_frame_sets():
    r = K.case('ragged4')
    assert r.n_points.tolist() == [1100, 0, 37, 563] and r.cap == 1100
    assert np.isnan(r.pcd[1]).all() and np.isnan(r.pcd[2, 37:]).all() and not np.isnan(r.pcd[0]).any()
    e = K.case('ends_empty')
    assert e.n_points.tolist() == [0, 700, 0]
    for name, cap in (('aligned1024', 1024), ('aligned1023', 1023)):
        a = K.case(name)
        assert a.cap == cap and a.n_points.tolist() == [cap] * 3 and a.pcd.shape == (3, cap, 6)
    m = K.case('many63')
    assert m.n_points.tolist() == list(K.MANY63_N) and m.n_points[0] == 0 and len(m.n_points) == 63
    assert m.n_points.min() == 0 and m.n_points.max() <= K.CAP and (m.n_points < 40).sum() >= 3
    blocks = -(-63 * K.CAP // 1024)
    assert blocks == 68 > 65, 'more scan blocks than the 64 predecessors of one look-back round'
    for fs in (r, e, m, K.case('single'), K.case('aligned1024')):
        for f, n in enumerate(fs.n_points):
            assert sorted(fs.perm[f, :n].tolist()) == list(range(n))
            assert (fs.perm[f, n:] == fs.cap - 1).all()


# ---- the layouts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ragged4', 'ends_empty'])
def test_concat_layout_is_the_per_frame_results_back_to_back(name):
    fs = K.case(name)
    per, cat = K.expected(name, 35, 9, 0), K.expected(name, 35, 9, 1)
    F = len(fs.n_points)
    assert np.array_equal(per.n_voxels, cat.n_voxels) and np.array_equal(per.vox_off, cat.vox_off)
    assert cat.vox_off[0] == 0 and np.array_equal(np.diff(cat.vox_off), cat.n_voxels) and cat.vox_off[-1] == len(cat.counts)
    for f in range(F):
        lo, hi = cat.vox_off[f], cat.vox_off[f + 1]
        v, i, c = O.group(fs.pcd[f, :fs.n_points[f]], fs.perm[f, :fs.n_points[f]], K.RNG, list(K.SIZE), 35)
        assert hi - lo == len(c) == per.n_voxels[f]
        assert np.array_equal(cat.voxels[lo:hi], v.astype(np.float32)) and np.array_equal(per.voxels[f], cat.voxels[lo:hi])
        assert np.array_equal(cat.coords[lo:hi, 1:], i.astype(np.int64)) and np.array_equal(per.coords[f][:, 1:], i.astype(np.int64))
        assert (cat.coords[lo:hi, 0] == f).all() and (per.coords[f][:, 0] == 0).all()
        assert np.array_equal(cat.counts[lo:hi], c) and np.array_equal(per.counts[f], c)
        assert (fs.n_points[f] == 0) == (hi == lo)
    seven = K.expected(name, 35, 7, 1)
    assert seven.voxels.shape[1:] == (35, 7) and np.array_equal(seven.coords, cat.coords) and np.array_equal(seven.counts, cat.counts)
    assert np.array_equal(seven.voxels[..., :3], cat.voxels[..., :3]) and np.array_equal(seven.voxels[..., 6], cat.voxels[..., 6])


# ---- argument errors: rejected before any launch ----------------------------------------------------------------------------------
def dummy_pointer():
    buf = ctypes.create_string_buffer(4096 + 64)
    return buf, (ctypes.addressof(buf) + 63) & ~63


def test_voxelizer_rejects_bad_arguments_before_any_launch():
    """Dummy non-null host addresses (nothing dereferences them) and ONE bad argument per call; the complete valid combination is
    never passed.  A launch on these pointers would fault, and without a GPU it would return a HIP error instead of -1."""
    from modules import Extension as X
    lib = X.lib
    keep, p = dummy_pointer()
    need = lib.mvx_voxelize_workspace_bytes(4, 1100)
    good = dict(status=p, F=4, cap=1100, ncol=6, size=(0.2, 0.2, 0.4), T=35, C=9, cap_voxels=1100, ws_bytes=need)

    def calls(status, F, cap, ncol, size, T, C, cap_voxels, ws_bytes):
        return (lib.mvx_voxelize_frames(p, p, p, None, F, cap, ncol, 0., -40., -3., size[0], size[1], size[2], T, C, cap_voxels, 1,
                                        p, p, p, p, p, status, p, ws_bytes, None),
                lib.mvx_voxelize(p, p, p, None, F, cap, ncol, 0., -40., -3., size[0], size[1], size[2], T, C, cap_voxels,
                                 p, p, p, p, status, p, ws_bytes, None))
    bad = [dict(F=0), dict(F=64), dict(F=255), dict(F=256), dict(F=-1), dict(T=0), dict(T=65), dict(C=8), dict(ncol=3),
           dict(size=(0.0, 0.2, 0.4)), dict(size=(0.2, -0.2, 0.4)), dict(size=(0.2, 0.2, 0.0)), dict(cap_voxels=0), dict(cap=0),
           dict(status=None), dict(ws_bytes=need - 1)]
    for b in bad:
        assert calls(**dict(good, **b)) == (-1, -1), b
    # 64 frames are rejected whatever the workspace: the gathers hold the F + 1 frame bases one per lane
    assert calls(**dict(good, F=64, ws_bytes=1 << 40)) == (-1, -1)
    assert calls(**dict(good, F=63, ws_bytes=lib.mvx_voxelize_workspace_bytes(63, 1100) - 1)) == (-1, -1)
    # MVX_ESIZE: cap_points * n_frames reaches 2^31, or cap_points alone exceeds 2^28
    assert calls(**dict(good, F=8, cap=1 << 28, ws_bytes=1 << 60)) == (-2, -2)
    assert calls(**dict(good, F=1, cap=(1 << 28) + 1, ws_bytes=1 << 60)) == (-2, -2)
    del keep


def test_voxelize_workspace_bytes():
    from modules import Extension as X
    q = X.lib.mvx_voxelize_workspace_bytes
    for F, cap in ((0, 1100), (-1, 1100), (63, 0), (63, -5)):
        assert q(F, cap) == 0
    assert q(63, 1100) > 0 and q(63, 1100) > q(62, 1100) > q(1, 1100) > 0
    assert 60e6 < q(63, 1100) < 80e6                  # the bucket table dominates: 63 x 4096 slots x 64 entries x 4 bytes


def test_wrappers_refuse_more_than_63_frames():
    """modules/_hip.py asserts the frame count before it touches a device."""
    from modules import _hip
    for F in (0, 64):
        x = torch.zeros((F, 8, 4), dtype=torch.float32)
        with pytest.raises(AssertionError):
            _hip.voxelize(x, None, None, K.RNG[:3], K.SIZE, 35, 9)
        with pytest.raises(AssertionError):
            _hip.voxelize_concat(x, None, None, K.RNG[:3], K.SIZE, 35, 9)


def test_header_states_the_limit_and_the_launch_count():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mvx_hip.h')).read()
    vox = text[text.index('Voxelizer.  Replaces'):text.index('size_t mvx_voxelize_workspace_bytes')]
    assert '1 <= n_frames <= 63' in vox and '255' not in vox
    assert 'Four launches' in vox and 'Three launches' not in vox


def test_grid_layout_entry_points_reject_bad_arguments_before_any_launch():
    """csrc/scatter.hip.  zero_grid = 0 throughout: the clearing of the grid comes before the tile check, and a memset on a host
    address is no argument error."""
    from modules import Extension as X
    lib = X.lib
    keep, p = dummy_pointer()
    D, H, W = 3, 21, 37
    for C in (0, 6, 63, -4):
        assert lib.mvx_scatter_voxels(p, p, p, 5, C, D, H, W, 0, p, None, 0, 0, None, None) == -1, C
        assert lib.mvx_gather_voxels(p, p, p, 5, C, D, H, W, None) == -1, C
    assert lib.mvx_scatter_voxels(p, p, None, 5, 64, D, H, W, 0, p, None, 0, 0, None, None) == -1
    assert lib.mvx_scatter_voxels(p, p, p, -1, 64, D, H, W, 0, p, None, 0, 0, None, None) == -1
    assert lib.mvx_scatter_voxels(p, p, p, 5, 64, D, 0, W, 0, p, None, 0, 0, None, None) == -1
    for th, tw in ((0, 16), (8, 0), (-8, 16)):
        assert lib.mvx_scatter_voxels(p, p, p, 5, 64, D, H, W, 0, p, p, th, tw, None, None) == -1, (th, tw)
    assert lib.mvx_gather_voxels(None, p, p, 5, 64, D, H, W, None) == -1
    for reverse in (0, 1):
        for nf in (0, 17):
            assert lib.mvx_cl_to_bev_frames(p, p, 2, 5, 37, 64, reverse, nf, None) == -1, nf
        assert lib.mvx_cl_to_bev_frames(p, p, 16, 256, 37, 64, reverse, 16, None) == -1      # d * h * n_frames = 65536 grid rows
        assert lib.mvx_cl_to_bev_frames(p, p, 2, 5, 37, 0, reverse, 1, None) == -1
        assert lib.mvx_cl_to_bev(p, p, 2, 32768, 37, 64, reverse, None) == -1
    for copies in (0, 17, -1):
        assert lib.mvx_bev_to_cl_broadcast(p, p, 2, 5, 37, 64, copies, None) == -1, copies
    assert lib.mvx_bev_to_cl_broadcast(p, p, 256, 256, 37, 64, 1, None) == -1
    assert lib.mvx_bev_to_cl_broadcast(p, None, 2, 5, 37, 64, 1, None) == -1
    del keep
