"""The GT-paste database builder on the GPU (csrc/gtdb.hip, modules/augment/BuildGT.py, create_gtdatabase_like.py) against the
host restatement tests/gtdb_ref.py.  Every comparison is exact: match index, flags, ROI, every mask and patch byte, pt_off and
every point in order, the pickle.

The decisions are thresholds on computed values -- the f32 IoU against 0.65, a pixel centre against an edge's crossing, a point
against a box face -- so the inputs (fixed seeds) are such that no decision value of the restatement lies within a band of its
threshold, asserted in ``build_cases`` on the restatement's own values; no case is left out.  The bands follow
tests/test_augment_gpu.py: 1e-5 absolute for the f32 IoU (some hundred f32 roundings of an IoU below 1); the two f64 tests use the
same operand order on both sides and differ by nothing, their band is 1e-9 (pixels, metres), about 1e4 f64 roundings of values
below 1300 and 80."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import gtdb_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'mvxnet-makise_amd')
SEEDS = (0, 1)
FRAMES = 10
BAND_IOU, BAND_F64 = 1e-5, 1e-9


def build_cases(tmp, seed):
    """A synthetic tree of FRAMES frames and the restatement's result on it as one batch; asserts the bands and that the
    cases the builder must handle are there.  Host only."""
    from modules.data import Synthetic as S
    root = os.path.join(str(tmp), 'kins%d' % seed)
    S.write_kins_tree(root, list(range(FRAMES)), seed=seed)
    seg = os.path.join(root, 'seglabel', 'update_train_2020.json')
    r = R.build(root, seg)
    m, L = r['margins'], r['labels']
    assert m['iou'].size > 40 and m['raster'].size > 20 and m['crop'].size > 20
    assert m['iou'].min() > BAND_IOU and m['raster'].min() > BAND_F64 and m['crop'].min() > BAND_F64
    names = [n for _, n in r['order']]
    assert len(names) == FRAMES - 1 >= 8 and '000001' not in names            # the frame without annotations is not processed
    far = names.index('000002')
    assert not (L['frame'] == far).any()                                      # all its labels fail the range test
    matched = L['best'] >= 0
    assert ((L['iou'] < 0.65) & matched & (L['iou'] > 0.3)).sum() >= 3 and (L['iou'] >= 0.65).sum() >= 20      # both sides of 0.65
    obj = L['flag'] == 3
    best = L['best'][obj].tolist()
    assert len(set(best)) < len(best)                                          # two labels take one annotation
    assert any(o['points'].shape[0] == 0 for o in r['objects']['Car'])         # an object without points
    assert any(o['points'].shape[0] > 20 for o in r['objects']['Car'])
    assert ((L['roi'][obj][:, 2] == 1223) & (L['roi'][obj][:, 3] == 369)).any()          # an ROI at the image corner
    assert all(len(r['objects'][c]) >= 2 for c in R.CLASSES)
    fill = [o['mask_px'].mean() for c in R.CLASSES for o in r['objects'][c]]
    assert min(fill) > 0.05 and max(fill) < 0.95
    return root, seg, r


@pytest.mark.parametrize('seed', SEEDS)
def test_cases_satisfy_the_bands_on_the_host(tmp_path, seed):
    """No GPU: the fixed seeds give inputs whose decision values all lie outside the bands (asserted inside)."""
    build_cases(tmp_path, seed)


def _batch(root, seg, r, dev):
    from modules.augment import BuildGT
    ann = BuildGT.readAnnotations(seg)
    frames = [BuildGT.loadFrame(root, name) for _, name in r['order']]
    return frames, [ann.by_image[i] for i, _ in r['order']]


@pytest.mark.gpu
@pytest.mark.parametrize('seed', SEEDS)
def test_match_flags_and_rois_are_exact(tmp_path, seed):
    from modules import _hip
    from modules.augment import BuildGT
    dev = torch.device('cuda')
    root, seg, r = build_cases(tmp_path, seed)
    frames, anns = _batch(root, seg, r, dev)
    t = BuildGT.pack(frames, anns, device=dev)
    best, iou, flag, roi, px_off = _hip.gtdb_match(t)
    L = r['labels']
    assert np.array_equal(best.cpu().numpy(), L['best'].astype(np.int32))
    assert np.array_equal(flag.cpu().numpy(), L['flag'].astype(np.int32))
    assert np.array_equal(iou.cpu().numpy().view(np.int32), L['iou'].astype(np.float32).view(np.int32))       # the f32 bits
    assert np.array_equal(roi.cpu().numpy(), L['roi'])
    px = np.where(L['flag'] == 3, (L['roi'][:, 2] - L['roi'][:, 0] + 1) * (L['roi'][:, 3] - L['roi'][:, 1] + 1), 0)
    assert np.array_equal(px_off.cpu().numpy(), np.concatenate([[0], np.cumsum(px)]))
    pt_off, _ = _hip.gtdb_crop_count(t, flag)
    want = iter([o['points'].shape[0] for c in R.CLASSES for o in r['objects'][c]])
    cnt = [next(want) if f == 3 else 0 for f in L['flag']]
    assert np.array_equal(pt_off.cpu().numpy(), np.concatenate([[0], np.cumsum(cnt)]))


@pytest.mark.gpu
@pytest.mark.parametrize('seed', SEEDS)
def test_masks_patches_and_points_are_exact(tmp_path, seed):
    """buildFrames on a batch of nine frames: per class every mask byte, patch byte, offset and point of the restatement, the
    points in file order; and the infos."""
    from modules.augment import BuildGT
    dev = torch.device('cuda')
    root, seg, r = build_cases(tmp_path, seed)
    frames, anns = _batch(root, seg, r, dev)
    counters = {c: 0 for c in R.CLASSES}
    built = BuildGT.buildFrames(frames, anns, device=dev, counters=counters)
    for c in R.CLASSES:
        objs, tb, infos = r['objects'][c], built[c]['tables'], built[c]['infos']
        assert tb['n'] == len(objs) == len(infos) == counters[c]
        assert np.array_equal(tb['px_off'].cpu().numpy(), np.cumsum([0] + [o['mask_px'].size for o in objs]))
        assert np.array_equal(tb['pt_off'].cpu().numpy(), np.cumsum([0] + [o['points'].shape[0] for o in objs]))
        assert np.array_equal(tb['mask'].cpu().numpy(), np.concatenate([o['mask_px'].reshape(-1) for o in objs]))
        assert np.array_equal(tb['patch'].cpu().numpy(), np.concatenate([o['patch'].reshape(-1, 3) for o in objs]))
        pts = np.concatenate([o['points'] for o in objs])
        assert np.array_equal(tb['points'].cpu().numpy().view(np.int32), pts.view(np.int32))
        assert np.array_equal(tb['maskbbox'].cpu().numpy(), np.stack([o['maskbbox'] for o in objs]))
        assert np.array_equal(tb['ann'], np.asarray([o['ann'] for o in objs]))
        for info, o in zip(infos, objs):
            assert [info[k] for k in ('velo', 'image', 'mask', 'id')] == [o[k] for k in ('velo', 'image', 'mask', 'id')]
            assert float(info['occlude']) == float(o['occlude']) and info['maskbbox'].tolist() == o['maskbbox'].tolist()
            assert np.array_equal(info['bbox2d'].numpy(), o['bbox2d']) and np.array_equal(info['bbox3d'].numpy(), o['bbox3d'])
    # the same frames again: bit for bit the same (no atomics decide anything)
    again = BuildGT.buildFrames(frames, anns, device=dev)
    for c in R.CLASSES:
        for k in ('mask', 'patch', 'points', 'pt_off', 'px_off'):
            assert torch.equal(again[c]['tables'][k], built[c]['tables'][k]), (c, k)


@pytest.mark.gpu
def test_single_frames_and_empty_batches(tmp_path):
    """Frame by frame (batches of one, the out-of-range frame among them) gives the objects of the one batch, in order."""
    from modules.augment import BuildGT
    dev = torch.device('cuda')
    root, seg, r = build_cases(tmp_path, SEEDS[0])
    frames, anns = _batch(root, seg, r, dev)
    got = {c: [] for c in R.CLASSES}
    for fr, an in zip(frames, anns):
        b = BuildGT.buildFrames([fr], [an], device=dev)
        for c in R.CLASSES:
            got[c] += BuildGT.objectsOf(b[c])
    b = BuildGT.buildFrames([frames[0]], [[]], device=dev)                     # labels, but no instance
    assert all(b[c]['tables']['n'] == 0 and b[c]['infos'] == [] for c in R.CLASSES)
    for c in R.CLASSES:
        # per class the reference numbers frame by frame, so the order is the one batch's
        assert len(got[c]) == len(r['objects'][c])
        for g, o in zip(got[c], r['objects'][c]):
            assert np.array_equal(g['velo'], o['points']) and np.array_equal(g['mask'], o['mask_px']) and np.array_equal(g['image'], o['patch'])
            assert g['id'] == o['id']


@pytest.mark.gpu
def test_script_writes_the_reference_layout(tmp_path, capsys):
    """create_gtdatabase_like.py in batches of four: the pickle and the files equal the restatement; getAllGT reads them."""
    sys.path.insert(0, PKG)
    import create_gtdatabase_like as C
    from modules.augment.LoadGT import getAllGT
    root, seg, r = build_cases(tmp_path, SEEDS[1])
    assert C.main([root, '--seg', seg, '--batch', '4', '--quiet']) == 0
    out = capsys.readouterr().out
    for c in R.CLASSES:
        objs = r['objects'][c]
        assert '%s: %d objects, %d without points' % (c, len(objs), sum(o['points'].shape[0] == 0 for o in objs)) in out
    info = pickle.load(open(os.path.join(root, 'training/gtdatabase/gtinfo.pkl'), 'rb'))
    assert set(info) == {'Car', 'Pedestrian', 'Cyclist'}
    gts = getAllGT(list(R.CLASSES), root=root)
    for c in R.CLASSES:
        assert len(info[c]) == len(r['objects'][c])
        for e, g, o in zip(info[c], gts[c], r['objects'][c]):
            assert set(e) == {'velo', 'image', 'mask', 'occlude', 'maskbbox', 'bbox2d', 'bbox3d', 'id'}
            assert [e[k] for k in ('velo', 'image', 'mask', 'id')] == [o[k] for k in ('velo', 'image', 'mask', 'id')]
            assert float(e['occlude']) == float(o['occlude']) and e['maskbbox'].tolist() == o['maskbbox'].tolist()
            assert e['maskbbox'].dtype == torch.int32 and e['bbox2d'].dtype == torch.float32
            assert np.array_equal(e['bbox2d'].numpy(), o['bbox2d']) and np.array_equal(e['bbox3d'].numpy(), o['bbox3d'])
            assert np.array_equal(g['velo'], o['points']) and np.array_equal(g['mask'], o['mask_px']) and np.array_equal(g['image'], o['patch'])
    # a class subset keeps all three keys
    assert C.main([root, '--seg', seg, '--classes', 'Car', '--quiet']) == 0
    info2 = pickle.load(open(os.path.join(root, 'training/gtdatabase/gtinfo.pkl'), 'rb'))
    assert len(info2['Car']) == len(info['Car']) and info2['Pedestrian'] == [] and info2['Cyclist'] == []


@pytest.mark.gpu
def test_built_database_feeds_the_augmentation(tmp_path):
    """End to end: the tree the script wrote, read by getAllGT, and the built tables taken directly (GTDatabase.from_built)
    give the same database and the same picks in Augment.augmentFrames."""
    sys.path.insert(0, PKG)
    import create_gtdatabase_like as C
    from modules import pipeline as pl
    from modules.augment import Augment as A, BuildGT
    from modules.augment.LoadGT import GTDatabase, getAllGT
    from modules.data import Load
    dev = torch.device('cuda')
    root, seg, r = build_cases(tmp_path, SEEDS[0])
    C.build_tree(root, seg, list(R.CLASSES), batch=8)
    db_disk = GTDatabase.from_gts(getAllGT(['Car'], root=root)['Car'], dev)
    frames, anns = _batch(root, seg, r, dev)
    built = [BuildGT.buildFrames(frames[:5], anns[:5], device=dev), BuildGT.buildFrames(frames[5:], anns[5:], device=dev)]
    db_mem = GTDatabase.from_built(built, {fr['id']: fr['calib'] for fr in frames}, dev)
    assert db_mem.n == db_disk.n == len(r['objects']['Car']) >= 20
    for k in ('box2d', 'box3d', 'bev', 'pt_off', 'points', 'px_off', 'patch', 'mask', 'maskbbox'):
        assert torch.equal(getattr(db_mem, k), getattr(db_disk, k)), k
    names = ['000000', '000003', '000004', '000005']
    ds = Load.createDataset(names, root=root)
    picks = []
    for db in (db_disk, db_mem):
        cap = max(d[0].shape[0] for d in ds) + 12 * db.max_points
        pts = torch.zeros((4, cap, 6), dtype=torch.float32, device=dev)
        for f, d in enumerate(ds):
            pts[f, :d[0].shape[0], :4] = torch.from_numpy(d[0]).to(dev)
        n = torch.tensor([d[0].shape[0] for d in ds], dtype=torch.int32, device=dev)
        batch = pl.FrameBatch(pts, torch.zeros((4, cap), dtype=torch.int32, device=dev), n, [None] * 4)
        imgs = torch.from_numpy(np.stack([d[1] for d in ds])).to(dev)
        np.random.seed(5)
        res = A.augmentFrames(batch, imgs, [None if d[3] is None else (d[2], d[3], d[4]) for d in ds], db, lim=12)
        picks.append((res.picked, res.n_points, imgs.cpu(), batch.points6.cpu()))
    assert picks[0][0] == picks[1][0] and picks[0][1] == picks[1][1] and sum(len(p) for p in picks[0][0]) >= 4
    assert torch.equal(picks[0][2], picks[1][2]) and torch.equal(picks[0][3], picks[1][3])
