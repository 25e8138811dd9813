"""GT-paste augmentation on the GPU (csrc/augment.hip, modules/augment) against the host restatement tests/augment_ref.py.

Decisions are thresholds on computed values, so the inputs (fixed seeds) are such that no decision value of the restatement
lies within a band of its threshold -- 1e-5 absolute for the IoU against 0.05, 1e-6 relative for the 2-D ratio and the ground
z; ``build_cases`` asserts that on the restatement's own values (zero values are left out), and the comparisons themselves are
exact: the bands forgive nothing."""
import os
import sys

import numpy as np
import pytest
import torch

import augment_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'mvxnet-makise_amd')
LIM = 12
SCENE = (0, 12, 13, 3, 5, 2)           # scene boxes per frame: none, exactly lim, more than lim, some


def _db(root, n, seed):
    from modules.augment.LoadGT import GTDatabase, getAllGT
    from modules.data import Synthetic as S
    S.write_gt_database(str(root), n, seed=seed)
    gts = getAllGT(['Car'], root=str(root))['Car']
    return gts, GTDatabase.from_gts(gts, 'cpu')


def _scene_frames(tmp, counts, seed=11):
    """Per frame (bbox2d, bbox3d, bev) tensors or None, the boxes drawn like the database's."""
    from modules import Calc
    from modules.data import Synthetic as S
    infos = S.write_gt_database(os.path.join(str(tmp), 'scene'), sum(counts), seed=seed, points=(5, 6))
    out, at = [], 0
    for n in counts:
        if n == 0:
            out.append(None)
            continue
        b2 = torch.stack([i['bbox2d'] for i in infos[at:at + n]])
        b3 = torch.stack([i['bbox3d'] for i in infos[at:at + n]])
        out.append((b2, b3, Calc.bbox3d2bev(b3)))
        at += n
    return out


def _clouds(F, P=20000):
    """Ring frames plus a few points outside the x/y range (and one NaN z) that the ground grid must skip."""
    from modules.data import Synthetic as S
    junk = np.array([[-1.0, 0.0, 0.99, 0.1], [70.4, 0.0, 0.99, 0.1], [10.0, 40.0, 0.99, 0.1], [10.0, -40.5, 0.99, 0.1],
                     [200.0, 0.0, 0.99, 0.1], [10.0, 0.0, np.nan, 0.1]], np.float32)
    out = []
    for f in range(F):
        p = S.synth_ring(f, P)
        # a raised platform (its cells reject the candidates centred there: the ground test must fail somewhere)
        g = np.random.default_rng(900 + f)
        slab = np.stack([g.uniform(28, 36, 16000), g.uniform(-6, 6, 16000), g.uniform(0.2, 0.45, 16000), g.random(16000)], 1)
        out.append(np.concatenate([p[:100], junk, p[100:], slab.astype(np.float32)], 0))
    return out


def build_cases(tmp, n_db=300, seed=2):
    """Inputs of the placement test and the restatement's results; asserts the bands.  Runs on the host alone."""
    import mvx_oracle as O
    import modules.config as cfg
    from modules.augment import Augment as A
    gts, db = _db(os.path.join(str(tmp), 'db'), n_db, seed)
    t = R.db_tables(db)
    scenes = _scene_frames(tmp, SCENE)
    clouds = _clouds(len(SCENE))
    F = len(SCENE)
    S = LIM
    rng = np.random.default_rng(40 + seed)
    cand = np.full((F, S, 30), -1, np.int32)
    thr = np.zeros((F, S), np.float32)
    for f in range(F):
        n0 = 0 if scenes[f] is None else scenes[f][1].shape[0]
        k = max(0, LIM - n0) if n0 <= LIM else 0
        cand[f, :k], thr[f, :k] = A.draw_slots(db.n, k, rng=rng)
    iou = lambda a, b: O.bbox_pairwise(a, b, True)
    grids = [R.ground_grid(c, cfg.velorange) for c in clouds]
    # frame 0 (no box): slot 0 offers one object 30 times, slot 1 the same object again -- all 30 fail, by its own overlap
    probe = R.place_frame(grids[0], cfg.velorange, np.zeros((0, 4)), np.zeros((0, 7)), np.zeros((0, 4, 2)), LIM, cand[0], thr[0], t, iou)
    j = int(probe['picked'][0])
    assert j >= 0
    cand[0, 0, :], cand[0, 1, :] = j, j
    refs = []
    for f in range(F):
        b2, b3, bv = (np.zeros((0, 4)), np.zeros((0, 7)), np.zeros((0, 4, 2))) if scenes[f] is None else [x.numpy() for x in scenes[f]]
        refs.append(R.place_frame(grids[f], cfg.velorange, b2, b3, bv, LIM, cand[f], thr[f], t, iou))
    assert refs[0]['picked'][0] == j and refs[0]['picked'][1] == -1 and (refs[0]['fail'][1] == 1).all()
    assert (refs[1]['picked'] == -1).all() and (refs[2]['picked'] == -1).all() and (refs[1]['fail'] == -1).all()
    # the bands, on the restatement's own values
    n_far = n_clipped = 0
    for f in range(F):
        r = refs[f]
        for s in range(S):
            for c in range(30):
                if r['fail'][s, c] < 0:
                    continue
                zg, iof, io = (float(v) for v in r['val'][s, c])
                z_lim = float(np.float32(t['box3d'][cand[f, s, c], 2]) + np.float32(0.1))
                assert abs(zg - z_lim) > 1e-6 * abs(z_lim), (f, s, c)
                if iof != 0.0 and np.isfinite(iof):
                    assert abs(iof - float(thr[f, s])) > 1e-6 * float(thr[f, s]), (f, s, c)
                if io != 0.0 and np.isfinite(io):
                    assert abs(io - 0.05) > 1e-5, (f, s, c)
                    n_far += abs(io) < 1e-4
                    n_clipped += io > 1e-4
    assert n_far > 0 and n_clipped > 0          # pairs of both kinds: bounding circles apart, and really clipped
    return dict(gts=gts, db=db, t=t, scenes=scenes, clouds=clouds, cand=cand, thr=thr, grids=grids, refs=refs)


def test_cases_satisfy_the_bands_on_the_host(tmp_path):
    """No GPU: the fixed seeds give inputs whose decision values all lie outside the bands (asserted inside)."""
    c = build_cases(tmp_path)
    fails = np.concatenate([r['fail'].reshape(-1) for r in c['refs']])
    assert {0, 1, 2, 3} <= set(fails.tolist())          # every outcome occurs


def _batch(clouds, dev, extra=0):
    from modules.pipeline import FrameBatch
    F = len(clouds)
    cap = max(c.shape[0] for c in clouds) + extra
    pts = torch.zeros((F, cap, 6), dtype=torch.float32, device=dev)
    n = torch.zeros((F,), dtype=torch.int32)
    for f, c in enumerate(clouds):
        pts[f, :c.shape[0], :c.shape[1]] = torch.from_numpy(c).to(dev)
        n[f] = c.shape[0]
    return FrameBatch(pts, torch.zeros((F, cap), dtype=torch.int32, device=dev), n.to(dev), [None] * F)


@pytest.mark.gpu
def test_ground_grid_is_bit_equal(tmp_path):
    import modules.config as cfg
    from modules import _hip
    dev = torch.device('cuda')
    clouds = _clouds(4)
    b = _batch(clouds, dev, extra=7)
    z = _hip.gt_paste_ground(b.points6, b.n_points, cfg.velorange).cpu().numpy()
    for f, c in enumerate(clouds):
        ref = R.ground_grid(c, cfg.velorange)
        assert np.array_equal(z[f], ref), f
        assert (ref > -4).sum() > 1000 and ref.max() < 0.98          # the out-of-range points (z = 0.99) did not land
    # the grid shape is a parameter
    z2 = _hip.gt_paste_ground(b.points6, b.n_points, cfg.velorange, (352, 100)).cpu().numpy()
    assert np.array_equal(z2[1], R.ground_grid(clouds[1], cfg.velorange, (352, 100)))


@pytest.mark.gpu
def test_placement_matches_the_restatement_per_candidate(tmp_path):
    import modules.config as cfg
    from modules import _hip
    from modules.augment import Augment as A
    dev = torch.device('cuda')
    c = build_cases(tmp_path)
    db = c['db'].to(dev)
    F = len(SCENE)
    b = _batch(c['clouds'], dev)
    zmax = _hip.gt_paste_ground(b.points6, b.n_points, cfg.velorange)
    b2, b3, bv, n0 = A._scene_tables(c['scenes'], _hip.GT_PASTE_MAX_BOXES, dev)
    status = torch.zeros((F,), dtype=torch.int32, device=dev)
    picked, n_out, fail, val = _hip.gt_paste_place(zmax, cfg.velorange, b2, b3, bv, n0.to(dev), LIM, torch.from_numpy(c['cand']).to(dev),
                                                   torch.from_numpy(c['thr']).to(dev), db, status, debug=True)
    picked, n_out, fail, val = picked.cpu().numpy(), n_out.cpu().numpy(), fail.cpu().numpy(), val.cpu().numpy()
    assert status.cpu().tolist() == [0] * F
    for f in range(F):
        r = c['refs'][f]
        print('frame %d: picked %s' % (f, picked[f].tolist()))
        assert picked[f].tolist() == r['picked'].tolist(), f
        assert np.array_equal(fail[f], r['fail']), f
        k = r['box3d'].shape[0]
        assert n_out[f] == k
        assert np.array_equal(b2[f, :k].cpu().numpy(), r['box2d']) and np.array_equal(b3[f, :k].cpu().numpy(), r['box3d'])
        assert np.array_equal(bv[f, :k].cpu().numpy(), r['bev'])
        live = r['fail'] >= 0
        assert np.array_equal(val[f][live][:, :2], r['val'][live][:, :2]), f           # ground z and the 2-D ratio: exact
        dv, rv = val[f][live][:, 2], r['val'][live][:, 2]
        same = dv == rv
        # where the bounding circles are apart the device has 0 and the oracle rounding noise, both far below 0.05
        assert (same | ((np.abs(dv) < 1e-4) & (np.abs(rv) < 1e-4))).all(), f
        assert (rv[same] > 1e-4).any() or f in (0, 1, 2)
    # a database smaller than 30 candidates
    gts7, db7 = _db(os.path.join(str(tmp_path), 'db7'), 7, 5)
    np.random.seed(1)
    cand7, thr7 = A.draw_slots(7, LIM)
    assert (cand7[:, 7:] == -1).all()
    t7 = R.db_tables(db7)
    import mvx_oracle as O
    ref7 = R.place_frame(c['grids'][3], cfg.velorange, *[x.numpy() for x in c['scenes'][3]], LIM, cand7, thr7, t7,
                         lambda a, b_: O.bbox_pairwise(a, b_, True))
    b2, b3, bv, n0 = A._scene_tables([c['scenes'][3]], _hip.GT_PASTE_MAX_BOXES, dev)
    st7 = torch.zeros((1,), dtype=torch.int32, device=dev)
    p7, n7, f7, v7 = _hip.gt_paste_place(zmax[3:4].contiguous(), cfg.velorange, b2, b3, bv, n0.to(dev), LIM,
                                         torch.from_numpy(cand7[None]).to(dev), torch.from_numpy(thr7[None]).to(dev), db7.to(dev), st7,
                                         debug=True)
    assert p7[0].cpu().tolist() == ref7['picked'].tolist() and np.array_equal(f7[0].cpu().numpy(), ref7['fail'])
    assert int(st7[0]) == 0 and (f7[0, :9, 7:].cpu().numpy() == -1).all()


@pytest.mark.gpu
def test_point_and_image_paste_are_bit_equal(tmp_path):
    from modules import _hip
    dev = torch.device('cuda')
    c = build_cases(tmp_path)
    db, t = c['db'].to(dev), c['t']
    F = len(SCENE)
    picked = np.stack([r['picked'] for r in c['refs']]).astype(np.int32)
    picked_d = torch.from_numpy(picked).to(dev)
    room = int(max(sum(int(t['pt_off'][i + 1] - t['pt_off'][i]) for i in p if i >= 0) for p in picked))
    for extra, want_over in ((room, False), (room // 2, True)):
        b = _batch([np.concatenate([cl, np.full((cl.shape[0], 2), 3.0, np.float32)], 1) for cl in c['clouds']], dev, extra=extra)
        before = b.points6.clone()
        status = torch.zeros((F,), dtype=torch.int32, device=dev)
        n_new = _hip.gt_paste_points(b.points6, b.n_points, picked_d, db, status).cpu().numpy()
        cap = b.points6.shape[1]
        over_any = False
        for f in range(F):
            n0 = c['clouds'][f].shape[0]
            rows, over = R.paste_points(before[f, :n0].cpu().numpy(), picked[f], t['points'], t['pt_off'], cap)
            over_any |= over
            assert n_new[f] == rows.shape[0], (f, extra)
            # bit patterns: the clouds hold a NaN on purpose
            assert np.array_equal(b.points6[f, :rows.shape[0]].cpu().numpy().view(np.uint32), rows.view(np.uint32)), (f, extra)
            assert torch.equal(b.points6[f, rows.shape[0]:].view(torch.int32), before[f, rows.shape[0]:].view(torch.int32))       # nothing behind the count is touched
            assert bool(int(status[f]) & _hip.GT_PASTE_POINTS_OVERFLOW) == over, (f, extra)
        assert over_any == want_over
    # images: patches under masks, later slots over earlier ones, clipped at the border (one object is moved half outside)
    g = np.random.default_rng(3)
    imgs = g.integers(0, 256, (F, 370, 1224, 3), dtype=np.uint8)
    bb = t['maskbbox'].copy()
    j = int(picked[0, 0])
    bb[j] += np.array([-bb[j, 0] - 5, 0, -bb[j, 0] - 5, 0], bb.dtype)                       # x1 = -5
    import copy
    db2 = copy.copy(db)
    db2.maskbbox = torch.from_numpy(bb).to(dev)
    out = _hip.gt_paste_image(torch.from_numpy(imgs).to(dev), picked_d, db2).cpu().numpy()
    changed = 0
    for f in range(F):
        ref = R.paste_image(imgs[f], picked[f], t['patch'], t['mask'], t['px_off'], bb)
        assert np.array_equal(out[f], ref), f
        changed += int((ref != imgs[f]).any())
    assert changed >= 4 and np.array_equal(out[1], imgs[1])


def _tree(tmp_path, n, n_db=150):
    from modules.data import Synthetic as S
    root = str(tmp_path / 'kitti')
    S.write_kitti_tree(root, list(range(n)), points=3000, raw_points=6000)
    S.write_gt_database(root, n_db, seed=4)
    return root


@pytest.mark.gpu
def test_augment_frames_equals_single_frame_calls(tmp_path):
    """augmentFrames on four frames = four augmentTargetClasses calls with the same np.random stream; its outputs stay on the
    device until the one packed read (Augment.augmentFrames: a single ``.cpu()`` of one int32 tensor)."""
    import inspect
    from modules import pipeline as pl
    from modules.augment import Augment as A
    from modules.augment.LoadGT import GTDatabase, getAllGT
    from modules.data import Load
    dev = torch.device('cuda')
    root = _tree(tmp_path, 4)
    names = ['%06d' % k for k in range(4)]
    ds = Load.createDataset(names, root=root)
    gts = getAllGT(['Car'], root=root)
    db = GTDatabase.from_gts(gts['Car'], dev)
    cap = 3000 + LIM * db.max_points
    pts = torch.zeros((4, cap, 6), dtype=torch.float32, device=dev)
    n = torch.tensor([d[0].shape[0] for d in ds], dtype=torch.int32, device=dev)
    for f, d in enumerate(ds):
        pts[f, :d[0].shape[0], :4] = torch.from_numpy(d[0]).to(dev)
    batch = pl.FrameBatch(pts, torch.zeros((4, cap), dtype=torch.int32, device=dev), n, [None] * 4)
    imgs = torch.from_numpy(np.stack([d[1] for d in ds])).to(dev)
    np.random.seed(3)
    res = A.augmentFrames(batch, imgs, [None if d[3] is None else (d[2], d[3], d[4]) for d in ds], db, lim=LIM)
    assert inspect.getsource(A.augmentFrames).count('.cpu()') == 1          # the one packed read
    np.random.seed(3)
    total = 0
    for f, d in enumerate(ds):
        velos, calibs, img, b3, bv = A.augmentTargetClasses(d[0], d[1], d[2], d[3], d[4], gts, ['Car'], [LIM])
        b3, bv = b3['Car'], bv['Car']
        assert torch.equal(res.bbox3d[f].cpu(), b3) and torch.equal(res.boxes[f][0].cpu(), bv), f
        assert torch.equal(res.boxes[f][1].cpu(), b3[:, :2])
        assert np.array_equal(imgs[f].cpu().numpy(), img), f
        n0 = d[0].shape[0]
        pasted = batch.points6[f, n0:res.n_points[f], :4].cpu().numpy()
        assert np.array_equal(pasted, np.concatenate(velos + [np.zeros((0, 4), np.float32)], 0)), f
        assert len(velos) == len(res.picked[f]) == b3.shape[0] - (0 if d[3] is None else d[3].shape[0])
        total += len(velos)
        perm = batch.perms[f, :res.n_points[f]].cpu().numpy()
        assert sorted(perm.tolist()) == list(range(res.n_points[f]))
    assert total >= 8 and batch.n_points.cpu().tolist() == res.n_points


@pytest.mark.gpu
def test_augmented_batch_end_to_end(tmp_path):
    """batch_from_dataset(augment=...) + the voxelizer = pre.group's contract (the C oracle) on the restatement's
    concatenated cloud under the same permutation; the whole training step runs on it."""
    sys.path.insert(0, PKG)
    import mvx_oracle as O
    import modules.config as cfg
    from modules import parallel, pipeline as pl
    from modules.Calc import bbox3d2bev
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
    cap = 3000 + LIM * db.max_points
    np.random.seed(0)
    plain, _ = pl.batch_from_dataset(ds, names, dev, bevs, train_like.fpn_maps_for, cap_points=cap)
    keep = {}
    np.random.seed(0)
    batch, targets = pl.batch_from_dataset(ds, names, dev, bevs, train_like.fpn_maps_for, cap_points=cap,
                                           augment={'db': db, 'lim': LIM, 'keep': keep})
    res = keep['result']
    t = R.db_tables(db)
    frames, status = pl.voxelize_batch(batch)
    assert int(status.max()) == 0
    for f in range(2):
        n0 = ds[f][0].shape[0]
        picked = np.asarray(res.picked[f] + [-1], np.int32)
        cloud, over = R.paste_points(plain.points6[f, :n0].cpu().numpy(), picked, t['points'], t['pt_off'], cap)
        assert not over and cloud.shape[0] == res.n_points[f] > n0
        perm = batch.perms[f, :cloud.shape[0]].cpu().numpy()
        rv, ri, _ = O.group(cloud, perm, cfg.velorange, cfg.voxelsize, cfg.samplenum)
        vox, idx = frames[f]
        assert vox.shape[1] == rv.shape[0]
        assert np.array_equal(idx[:, 1:].cpu().numpy(), ri.astype(np.int64))
        assert np.array_equal(vox[0].cpu().numpy(), rv.astype(np.float32))
        assert targets[f] is not None and targets[f][3].shape[0] == len(res.picked[f]) + (0 if ds[f][3] is None else ds[f][3].shape[0])
    torch.manual_seed(0)
    model = MVXNet().to(dev)
    bucket = parallel.GradBucket([p for p in model.parameters() if p.requires_grad])
    bucket.zero()
    out = pl.train_step_full(model, batch, targets, VoxelLoss(), anchors.to(dev), cfg.imsize)          # raises on a status word
    torch.cuda.synchronize()
    assert len(out['loss']) == 2 and all(np.isfinite(v) for v in out['loss']) and torch.isfinite(bucket.flat).all()


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['fast', 'module'])
def test_train_like_runs_with_augment(tmp_path, mode):
    sys.path.insert(0, PKG)
    import train_like
    root = str(tmp_path / 'kitti')
    args = train_like.parse_args([root, '--synthetic', '8', '--augment', '--mode', mode, '--steps', '2', '--points', '3000',
                                  '--checkpoints', str(tmp_path / 'ck'), '--quiet'])
    np.random.seed(0)
    r = train_like.train(args)
    assert r['steps'] == 2 and len(r['losses']) == (8 if mode == 'fast' else 2) and all(np.isfinite(v) for v in r['losses'])
