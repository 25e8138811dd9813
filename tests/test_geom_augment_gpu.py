"""Geometric augmentation on the GPU (csrc/geom_augment.hip, modules/augment/Geometry.py) against the float64 restatement
tests/geom_augment_ref.py on the cases of tests/geom_augment_cases.py.

Decisions -- the taken trial per box, the kept boxes, the kept points and their order (column 3 of a row holds its original
index), columns 3..5 -- are compared exactly: the inputs keep every decision value outside a band of its threshold (asserted
on the host).  Values are compared within bounds derived from f32 arithmetic: coordinates stay below ~115 m, where an f32
rounding is at most 4e-6 m, and a coordinate passes about ten roundings through both rotations: 1e-4 m absolute for point
and box coordinates and for bev quads; box sizes take one rounding: 1e-6 relative; r: 1e-5 rad modulo 2 pi.  (The kernels
compute in f64 and round once; the worst distances are printed per T before the assertion.)"""
import os
import sys

import numpy as np
import pytest
import torch

import geom_augment_cases as C
import geom_augment_ref as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'mvxnet-makise_amd')
TOL_M, TOL_SIZE, TOL_R = 1e-4, 1e-6, 1e-5


def _batch(clouds, dev):
    from modules.pipeline import FrameBatch
    pts = torch.full((C.F, C.CAP, 6), float('nan'), dtype=torch.float32, device=dev)          # tail rows: NaN, never read
    for f, c in enumerate(clouds):
        pts[f, :c.shape[0]] = torch.from_numpy(c).to(dev)
    n = torch.tensor([c.shape[0] for c in clouds], dtype=torch.int32, device=dev)
    return FrameBatch(pts, torch.zeros((C.F, C.CAP), dtype=torch.int32, device=dev), n, [None] * C.F)


def _run(c, dev):
    from modules.augment import Geometry
    batch = _batch(c['clouds'], dev)
    res = Geometry.augmentGeometryFrames(batch, [torch.from_numpy(b) for b in c['boxes']], c['noise'], c['glob'], iou_thr=C.IOU_THR)
    return batch, res


@pytest.mark.gpu
@pytest.mark.parametrize('T', [1, 16, 32])
def test_frame_set_matches_the_restatement(T):
    dev = torch.device('cuda')
    c = C.build(T)
    batch, res = _run(c, dev)
    worst = {'point': 0.0, 'box': 0.0, 'bev': 0.0, 'size': 0.0, 'r': 0.0}
    assert res.status == [0] * C.F and res.bbox2d is None
    moves = res.moves.cpu().numpy()
    for f in range(C.F):
        r = c['refs'][f]
        nb = c['boxes'][f].shape[0]
        # decisions: exact
        assert res.trials[f, :nb].tolist() == r['trial'].tolist() and (res.trials[f, nb:] == -1).all(), f
        assert np.array_equal(moves[f, :nb], r['move'].astype(np.float32)) and not moves[f, nb:].any()
        assert res.kept[f] == r['kept_boxes'].tolist(), f
        k = res.n_points[f]
        assert k == r['kept_points'].size == int(batch.n_points[f]), f
        rows = batch.points6[f, :k].cpu().numpy()
        assert np.array_equal(rows[:, 3].astype(np.int64), r['kept_points']), f                  # which points, in which order
        assert np.array_equal(rows[:, 3:].view(np.uint32), r['rest'].view(np.uint32)), f        # columns 3..5 bitwise
        assert G.in_range(rows[:, :3].astype(np.float64), C.VELORANGE).all(), f
        # values
        if k:
            worst['point'] = max(worst['point'], float(np.abs(rows[:, :3] - r['xyz']).max()))
        if r['kept_boxes'].size:
            b3, bev, cen = res.bbox3d[f].cpu().numpy().astype(np.float64), res.boxes[f][0].cpu().numpy(), res.boxes[f][1].cpu().numpy()
            assert b3.shape == r['box3d'].shape and bev.shape == r['bev'].shape and np.array_equal(cen, b3[:, :2].astype(np.float32))
            worst['box'] = max(worst['box'], float(np.abs(b3[:, :3] - r['box3d'][:, :3]).max()))
            worst['size'] = max(worst['size'], float((np.abs(b3[:, 3:6] - r['box3d'][:, 3:6]) / r['box3d'][:, 3:6]).max()))
            dr = b3[:, 6] - r['box3d'][:, 6]
            worst['r'] = max(worst['r'], float(np.abs(dr - 2 * np.pi * np.round(dr / (2 * np.pi))).max()))
            worst['bev'] = max(worst['bev'], float(np.abs(bev - r['bev']).max()))
            assert (b3[:, 6] >= -np.pi - TOL_R).all() and (b3[:, 6] <= np.pi + TOL_R).all()
        else:
            assert res.bbox3d[f] is None and res.boxes[f] is None
        perm = batch.perms[f, :k].cpu().numpy()
        assert sorted(perm.tolist()) == list(range(k))
    print('T=%d worst distances: %s' % (T, worst))
    assert worst['point'] <= TOL_M and worst['box'] <= TOL_M and worst['bev'] <= TOL_M, worst
    assert worst['size'] <= TOL_SIZE and worst['r'] <= TOL_R, worst


@pytest.mark.gpu
def test_second_run_is_bitwise_identical_and_single_frame_equals_frame_3():
    from modules.augment import Geometry
    dev = torch.device('cuda')
    c = C.build(16)
    b1, r1 = _run(c, dev)
    b2, r2 = _run(c, dev)
    assert np.array_equal(r1.trials, r2.trials) and r1.kept == r2.kept and r1.n_points == r2.n_points
    for f in range(C.F):
        k = r1.n_points[f]
        assert torch.equal(b1.points6[f, :k].view(torch.int32), b2.points6[f, :k].view(torch.int32))
        if r1.bbox3d[f] is not None:
            assert torch.equal(r1.bbox3d[f].view(torch.int32), r2.bbox3d[f].view(torch.int32))
            assert torch.equal(r1.boxes[f][0].view(torch.int32), r2.boxes[f][0].view(torch.int32))
    assert torch.equal(r1.moves, r2.moves)
    cloud, b3, bev = Geometry.augmentGeometry(c['clouds'][3], torch.from_numpy(c['boxes'][3]), c['noise'][3], c['glob'][3], iou_thr=C.IOU_THR)
    k = r1.n_points[3]
    assert np.array_equal(cloud.view(np.uint32), b1.points6[3, :k].cpu().numpy().view(np.uint32))
    assert torch.equal(b3, r1.bbox3d[3].cpu()) and torch.equal(bev, r1.boxes[3][0].cpu())
    # a frame without boxes or points, alone
    cloud0, b30, bev0 = Geometry.augmentGeometry(np.zeros((0, 6), np.float32), None, c['noise'][0], c['glob'][0])
    assert cloud0.shape == (0, 6) and b30 is None and bev0 is None


@pytest.mark.gpu
def test_limits_are_reported():
    from modules import Extension as X, _hip
    dev = torch.device('cuda')
    c = C.build(16)
    b3 = torch.zeros((1, 32, 7), device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    noise, glob = torch.from_numpy(c['noise'][:1]).to(dev), torch.from_numpy(c['glob'][:1]).to(dev)
    placed = _hip.geom_place(b3, torch.tensor([33], dtype=torch.int32, device=dev), noise, glob, C.VELORANGE, status)
    assert int(status[0]) == _hip.GEOM_BAD_COUNT and int(placed.n_kept[0]) == 0 and (placed.trial.cpu() == -1).all()
    with pytest.raises(X.MvxHipError):
        _hip.geom_place(torch.zeros((1, 33, 7), device=dev), torch.zeros((1,), dtype=torch.int32, device=dev),
                        torch.zeros((1, 33, 4, 4), device=dev), glob, C.VELORANGE, status)


def _tree(tmp_path, n, n_db=150):
    from modules.data import Synthetic as S
    root = str(tmp_path / 'kitti')
    S.write_kitti_tree(root, list(range(n)), points=3000, raw_points=6000)
    S.write_gt_database(root, n_db, seed=4)
    return root


@pytest.mark.gpu
def test_pasted_and_moved_batch_end_to_end(tmp_path):
    """batch_from_dataset(augment=..., geometry=...) and the whole training step on it.  The global rotation is drawn from
    +-0.1 rad here: the anchors stand at 0 and pi/2 only, and this test wants a positive anchor in every frame."""
    sys.path.insert(0, PKG)
    import modules.config as cfg
    from modules import parallel, pipeline as pl
    from modules.Calc import bbox3d2bev
    from modules.augment.Geometry import GeomParams
    from modules.augment.LoadGT import GTDatabase, getAllGT
    from modules.data import Load, Preprocessing as pre
    from modules.voxelnet import VoxelLoss
    from MVXNet import MVXNet
    import train_like
    dev = torch.device('cuda')
    root = _tree(tmp_path, 2)
    names = ['000000', '000001']
    ds = Load.createDataset(names, root=root)
    db = GTDatabase.from_gts(getAllGT(['Car'], root=root)['Car'], dev)
    anchors = pre.createAnchors(cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2, cfg.velorange, cfg.carsize)
    bevs = bbox3d2bev(anchors.reshape(anchors.shape[:2] + (-1, 7))).to(dev).contiguous()
    cap = 3000 + 12 * db.max_points
    keep0, keep1, gkeep = {}, {}, {}
    np.random.seed(0)
    pl.batch_from_dataset(ds, names, dev, bevs, train_like.fpn_maps_for, cap_points=cap,
                          augment={'db': db, 'lim': 12, 'keep': keep0, 'rng': np.random.default_rng(5)})
    np.random.seed(0)
    batch, targets = pl.batch_from_dataset(ds, names, dev, bevs, train_like.fpn_maps_for, cap_points=cap,
                                           augment={'db': db, 'lim': 12, 'keep': keep1, 'rng': np.random.default_rng(5)},
                                           geometry={'params': GeomParams(rot_glob=0.1), 'rng': np.random.default_rng(6), 'keep': gkeep})
    res, plain = keep1['result'], keep0['result']
    assert res.picked == plain.picked and sum(len(p) for p in res.picked) >= 4          # the paste's decisions do not depend on it
    assert res.status == [0, 0] and res.geometry is gkeep['result'] and res.geometry.status == [0, 0] and res.bbox2d is None
    assert (res.geometry.trials >= 0).any() and batch.n_points.cpu().tolist() == res.n_points
    for f in range(2):
        assert 0 < res.n_points[f] <= plain.n_points[f]
        assert targets[f] is not None and len(targets[f][0][0]) >= 1                     # a positive anchor
        assert targets[f][3].shape[0] == len(res.geometry.kept[f]) >= 1
        rows = batch.points6[f, :res.n_points[f], :3].cpu().numpy().astype(np.float64)
        assert G.in_range(rows, cfg.velorange).all()
    torch.manual_seed(0)
    model = MVXNet().to(dev)
    bucket = parallel.GradBucket([p for p in model.parameters() if p.requires_grad])
    bucket.zero()
    out = pl.train_step_full(model, batch, targets, VoxelLoss(), anchors.to(dev), cfg.imsize)          # raises on a status word
    torch.cuda.synchronize()
    assert len(out['loss']) == 2 and all(np.isfinite(v) for v in out['loss']) and torch.isfinite(bucket.flat).all()
    assert all(v >= 1 for v in out['voxels'])
    # geometry alone, without the paste
    np.random.seed(0)
    b2, t2 = pl.batch_from_dataset(ds, names, dev, bevs, train_like.fpn_maps_for, cap_points=cap,
                                   geometry={'params': GeomParams(rot_glob=0.1), 'rng': np.random.default_rng(6)})
    assert all(0 < int(k) <= 3000 for k in b2.n_points.cpu().tolist())


@pytest.mark.gpu
@pytest.mark.parametrize('mode,paste', [('fast', True), ('fast', False), ('module', True)])
def test_train_like_runs_with_augment_geometry(tmp_path, mode, paste):
    sys.path.insert(0, PKG)
    import train_like
    root = str(tmp_path / 'kitti')
    args = train_like.parse_args([root, '--synthetic', '8', '--augment-geometry', '--mode', mode, '--steps', '2', '--points', '3000',
                                  '--checkpoints', str(tmp_path / 'ck'), '--quiet'] + (['--augment'] if paste else []))
    np.random.seed(0)
    r = train_like.train(args)
    assert r['steps'] == 2 and len(r['losses']) == (8 if mode == 'fast' else 2) and all(np.isfinite(v) for v in r['losses'])
