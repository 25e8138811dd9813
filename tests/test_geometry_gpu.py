"""crop / cropTensor / cropToSight / lidar2Img on the GPU against the reference fixtures."""
import numpy as np
import pytest
import torch

import mvx_oracle as O

pytestmark = pytest.mark.gpu


def test_crop_and_crop_to_sight_match_reference(golden):
    from modules.data import Preprocessing as pre
    g = golden('crop')
    raw = g['raw']
    c1 = pre.crop(raw.copy(), list(g['velorange']))
    assert np.array_equal(c1, g['crop'])                       # order-preserving, bit-exact rows
    ct = pre.cropTensor(torch.from_numpy(raw.copy()).cuda(), list(g['velorange']))
    assert np.array_equal(ct.cpu().numpy(), g['crop_tensor'])
    c2 = pre.cropToSight(c1.copy(), O.KITTI_CALIB, list(g['imsize_wh']))
    assert np.array_equal(c2, g['crop_to_sight'])
    calib32 = {k: torch.tensor(v, dtype=torch.float32) for k, v in O.KITTI_CALIB.items()}
    c2t = pre.cropToSight(torch.from_numpy(c1.copy()).cuda(), calib32, list(g['imsize_wh']))
    assert np.array_equal(c2t.cpu().numpy(), g['crop_to_sight_tensor'])
    fused = pre.cropFused(raw.copy(), list(g['velorange']), O.KITTI_CALIB, list(g['imsize_wh']))
    assert np.array_equal(fused, g['crop_to_sight'])


def test_crop_full_size_properties():
    """120k-point raw cloud (cropdata.py-sized): idempotence and agreement with the oracle."""
    from modules.data import Preprocessing as pre
    raw = O.synth_raw(1)
    a = pre.cropFused(raw.copy(), O.VELORANGE, O.KITTI_CALIB, (1224, 370))
    ref = O.crop_to_sight(O.crop(raw, O.VELORANGE), O.KITTI_CALIB, (1224, 370))
    assert np.array_equal(a, ref)
    assert np.array_equal(pre.cropFused(a.copy(), O.VELORANGE, O.KITTI_CALIB, (1224, 370)), a)
    assert pre.crop(np.zeros((0, 4), np.float32), O.VELORANGE).shape == (0, 4)


def test_lidar2img_matches_reference(golden):
    from modules.utils import lidar2Img
    g = golden('lidar2img')
    calib32 = {k: torch.tensor(v, dtype=torch.float32) for k, v in O.KITTI_CALIB.items()}
    p32 = lidar2Img(torch.from_numpy(g['pcd']), calib32, True)
    np.testing.assert_allclose(p32.numpy(), g['proj_f32'], rtol=2e-5, atol=2e-3)
    p64 = lidar2Img(g['pcd'].copy(), O.KITTI_CALIB, True)
    np.testing.assert_allclose(p64, g['proj_f64'], rtol=1e-6, atol=1e-4)   # returned through f32
    assert lidar2Img(g['pcd'].copy(), O.KITTI_CALIB, False).shape[0] <= g['pcd'].shape[0]


def test_crop_scan_carry_two_frames():
    """The shared scan of the block counts beyond its first trip of 1024 blocks, with per-frame indexing: two frames of 1026
    blocks each.  Frame 0 keeps rows in blocks 1024 and 1025, whose positions need the carry of the first trip, behind a block
    with nothing kept that ends the first trip; frame 1 ends inside block 1023, so its second trip holds only zeros and its
    count and offsets must not be touched by frame 0's."""
    from modules import _hip
    F, cap, ncol = 2, 1024 * 256 + 300, 4
    n_in = [cap, 1024 * 256 - 77]
    lo, hi = np.array(O.VELORANGE[:3]), np.array(O.VELORANGE[3:])
    g = np.random.default_rng(20)
    u = g.random((F, cap, ncol))
    u[..., 0] *= 2.0                                            # x beyond the range for about half of the points
    pcd = u.astype(np.float32)
    pcd[..., :3] = (lo + (hi - lo) * u[..., :3]).astype(np.float32)
    pcd[0, 1024 * 256 - 300:1024 * 256 + 100, 0] = np.float32(hi[0] + 1.0)      # 400 rejected rows across row 262,144
    out, n_out, src = _hip.crop_points(torch.from_numpy(pcd).cuda(), torch.tensor(n_in, dtype=torch.int32).cuda(),
                                       list(O.VELORANGE), want_index=True)
    out, n_out, src = out.cpu().numpy(), n_out.cpu().numpy(), src.cpu().numpy()
    for f in range(F):
        p = pcd[f, :n_in[f]]
        xyz = p[:, :3].astype(np.float64)                       # f32 values compared in f64, as Preprocessing.crop
        mask = np.all((lo <= xyz) & (xyz < hi), axis=1)
        n = int(mask.sum())
        assert 0.4 * n_in[f] < n < 0.6 * n_in[f]
        assert n_out[f] == n
        assert np.array_equal(out[f, :n], p[mask])
        assert np.array_equal(src[f, :n], np.flatnonzero(mask))
    assert not np.any(np.all((lo <= pcd[0, 1023 * 256:1024 * 256, :3]) & (pcd[0, 1023 * 256:1024 * 256, :3] < hi), axis=1))
    kept0 = src[0, :n_out[0]]
    assert np.any((kept0 >= 1024 * 256) & (kept0 < 1025 * 256)) and np.any(kept0 >= 1025 * 256)      # both blocks of the second trip
