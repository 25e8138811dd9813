"""The geometric augmentation's host side (no GPU): properties of the restatement tests/geom_augment_ref.py that the GPU test
compares the kernels with, the band assertions on the shared cases, the draws and the ABI entries."""
import numpy as np
import pytest

import geom_augment_cases as C
import geom_augment_ref as G


def _iou():
    import mvx_oracle as O
    return lambda a, b: O.bbox_pairwise(a, b, True)


def _frame(seed=0, n_pts=400):
    rng = np.random.default_rng(seed)
    boxes = np.array([C._car(12.0 + 9.0 * k, -6.0 + 5.0 * (k % 3), rng.uniform(-3, 3)) for k in range(5)], np.float32)
    xyz = np.concatenate([G.rot(rng.uniform(-0.45, 0.45, (40, 2)) * b[3:5], b[6]) + b[:2] for b in boxes.astype(np.float64)])
    xyz = np.concatenate([xyz, rng.uniform(-1.5, -0.2, (xyz.shape[0], 1))], 1)
    bg = rng.uniform([5, -20, -2.5], [60, 20, 0.5], (n_pts - xyz.shape[0], 3))
    pts = np.zeros((n_pts, 6), np.float32)
    pts[:, :3] = np.concatenate([xyz, bg])
    pts[:, 3] = np.arange(n_pts)
    pts[:, 4:] = rng.uniform(0, 300, (n_pts, 2))
    return pts, boxes


def test_identity_parameters_return_the_input():
    pts, boxes = _frame()
    noise = np.zeros((5, 4, 4), np.float32)
    glob = np.array([0, 1, 0, 0], np.float32)
    r = G.augment_frame(pts, boxes, noise, glob, C.VELORANGE, C.IOU_THR, _iou(), check_band=False)
    assert r['trial'].tolist() == [0] * 5 and r['kept_boxes'].tolist() == list(range(5))
    assert r['kept_points'].tolist() == list(range(pts.shape[0]))
    assert np.array_equal(r['xyz'], pts[:, :3].astype(np.float64)) and np.array_equal(r['rest'], pts[:, 3:])
    assert np.array_equal(r['box3d'][:, :6], boxes[:, :6].astype(np.float64))
    assert np.allclose(r['box3d'][:, 6], boxes[:, 6], atol=1e-12) and np.allclose(r['bev'], [G.quad(b) for b in boxes], atol=1e-12)


@pytest.mark.parametrize('flip', [0, 1])
def test_inverse_global_transform_recovers_the_per_object_result(flip):
    pts, boxes = _frame(1)
    noise, _ = G.draw_like(1, 5, 8, np.random.default_rng(3))
    glob = np.array([0.6, 1.04, flip, 0], np.float32)
    trial, move, moved, _ = G.place_frame(boxes, noise[0], C.IOU_THR, _iou(), check_band=False)
    assert (trial >= 0).any()
    obj, _ = G.object_points(pts, boxes, trial, move)
    assert np.abs(obj - pts[:, :3]).max() > 0.1                       # something moved
    out, _ = G.transform_points(pts, boxes, trial, move, glob)
    back = out.copy()
    if flip:
        back[:, 1] = -back[:, 1]
    back /= float(glob[1])
    back[:, :2] = G.rot(back[:, :2], -float(glob[0]))
    assert np.abs(back - obj).max() < 1e-12
    # the boxes follow their points: a box's corners, moved as points, are the corners of the moved box
    gb = G.global_boxes(moved, glob)
    for b0, b1 in zip(moved, gb):
        q = np.concatenate([G.quad(b0), np.full((4, 1), b0[2])], 1)
        want = G.global_points(q, glob)[:, :2]
        got = G.quad(b1)
        assert np.abs(np.sort(want, 0) - np.sort(got, 0)).max() < 1e-9
        assert -np.pi <= b1[6] < np.pi and np.allclose(b1[3:6], b0[3:6] * float(glob[1]))


def test_a_boxed_in_car_keeps_its_pose():
    c = C.build(32)
    r = c['refs'][3]
    assert r['trial'][C.C_] == -1 and not r['move'][C.C_].any()
    own = r['owner']
    mine = np.nonzero(own == C.C_)[0]
    assert mine.size > 10
    # its points take the global step alone
    want = G.global_points(c['clouds'][3][mine, :3].astype(np.float64), c['glob'][3])
    got, _ = G.transform_points(c['clouds'][3][mine], c['boxes'][3], r['trial'], r['move'], c['glob'][3])
    assert np.array_equal(want, got)


@pytest.mark.parametrize('T', [1, 16, 32])
def test_cases_satisfy_the_bands_on_the_host(T):
    """``build`` runs the restatement with its band assertions on (IoU 1e-5 from the threshold, faces 1e-3 m) and asserts the
    constructed situations; every outcome the GPU test wants to see occurs."""
    c = C.build(T)
    assert [x.shape[0] for x in c['clouds']] == list(C.N_POINTS) and [b.shape[0] for b in c['boxes']] == list(C.N_BOXES)
    trials = np.concatenate([r['trial'] for r in c['refs']])
    assert -1 in trials and 0 in trials and (T == 1 or (trials > 0).any())
    for r in c['refs']:
        assert G.in_range(r['xyz'], C.VELORANGE).all()


def test_draw_geometry_ranges_and_seed():
    from modules.augment.Geometry import GeomParams, draw_geometry
    from modules.augment import Augment as A
    p = GeomParams()
    assert p.trials == 16 and p.iou_thr == A.BEV_IOU_THR and p.scale == (0.95, 1.05) and p.flip_p == 0.5
    assert abs(p.rot_obj - np.pi / 10) < 1e-15 and abs(p.rot_glob - np.pi / 4) < 1e-15 and p.sigma == (1.0, 1.0, 1.0)
    noise, glob = draw_geometry(64, 32, p, np.random.default_rng(7))
    assert noise.shape == (64, 32, 16, 4) and noise.dtype == np.float32 and glob.shape == (64, 4) and glob.dtype == np.float32
    assert np.abs(noise[..., 3]).max() <= np.float32(np.pi / 10) and np.abs(glob[:, 0]).max() <= np.float32(np.pi / 4)
    assert 0.95 <= glob[:, 1].min() and glob[:, 1].max() <= np.float32(1.05) and set(glob[:, 2].tolist()) == {0.0, 1.0}
    assert (glob[:, 3] == 0).all() and abs(float(noise[..., :3].std()) - 1.0) < 0.02 and abs(float(noise[..., :3].mean())) < 0.02
    n2, g2 = draw_geometry(64, 32, p, np.random.default_rng(7))
    assert np.array_equal(noise, n2) and np.array_equal(glob, g2)
    n3, g3 = G.draw_like(64, 32, 16, np.random.default_rng(7))
    assert np.array_equal(noise, n3) and np.array_equal(glob, g3)          # the restated order of draws
    q = GeomParams(rot_obj=0.0, sigma=(0, 0, 0), trials=1, scale=(1, 1), rot_glob=0.0, flip_p=0.0)
    n0, g0 = draw_geometry(2, 32, q, np.random.default_rng(1))
    assert not n0.any() and g0.tolist() == [[0, 1, 0, 0]] * 2
    from modules import Extension as X
    with pytest.raises(X.MvxHipError):
        GeomParams(trials=33)


def test_entries_and_limits():
    """The new entries are exported and typed; argument errors return MVX_EINVAL before any launch."""
    from modules import Extension as X, _hip
    for name in ('mvx_geom_workspace_bytes', 'mvx_geom_place_frames', 'mvx_geom_points_frames'):
        assert name in X.PROTOTYPES and hasattr(X.lib, name)
    assert X.lib.mvx_geom_workspace_bytes(4, 20000) >= 4 * 79 * 4 and _hip.GEOM_MAX_TRIALS == 32
    r = np.asarray(C.VELORANGE, np.float64)
    rp = r.ctypes.data
    one = 1 << 20          # never dereferenced: the checks come first
    assert X.lib.mvx_geom_place_frames(one, one, 4, 33, one, 16, one, 0.05, rp, one, one, 2 * one, one, one, one, one, None) == -1
    assert X.lib.mvx_geom_place_frames(one, one, 4, 32, one, 33, one, 0.05, rp, one, one, 2 * one, one, one, one, one, None) == -1
    assert X.lib.mvx_geom_place_frames(one, one, 17, 32, one, 16, one, 0.05, rp, one, one, 2 * one, one, one, one, one, None) == -1
    assert X.lib.mvx_geom_points_frames(one, one, 4, 100, one, one, 32, one, one, one, rp, one, 2 * one, one, 1 << 20, None) == -1
