"""Host checks of the GT-paste database builder (modules/augment/BuildGT.py, create_gtdatabase_like.py) without a GPU: the
restatement tests/gtdb_ref.py against values recorded from the reference's own Calc functions (tests/golden/gtdb_ref.npz,
tools/gen_gtdb_fixture.py), its box_iou against closed forms, the package's label preparation and packing against the
restatement bit for bit, and the written tree's layout against what getAllGT reads back."""
import os
import pickle

import numpy as np
import pytest
import torch

import gtdb_ref as R

FIX_FRAMES, FIX_SEED = 4, 5          # tools/gen_gtdb_fixture.py


def _tree(tmp_path, n=6, seed=0):
    from modules.data import Synthetic as S
    root = str(tmp_path / 'kins')
    S.write_kins_tree(root, list(range(n)), seed=seed, points=2000)
    return root, os.path.join(root, 'seglabel', 'update_train_2020.json')


def test_restatement_boxes_equal_the_reference_recording(tmp_path, golden):
    """bboxCam2Lidar, bbox3d2corner and bbox3d2bev of the reference, recorded on the synthetic labels.  The restatement writes
    the 4x4 product out in f32 where the reference calls a matmul, and numpy's f32 cosine where it calls torch's: a few f32
    roundings on values below 80 -- 2e-5 absolute."""
    from modules.data import Synthetic as S
    fx = golden('gtdb_ref')
    assert int(fx['n_frames']) == FIX_FRAMES and int(fx['seed']) == FIX_SEED
    root = str(tmp_path / 'kins')
    names = S.write_kins_tree(root, list(range(FIX_FRAMES)), seed=FIX_SEED, points=100)
    total = 0
    for f, name in enumerate(names):
        _, rows = R.read_labels(os.path.join(root, 'training/label_2', name + '.txt'), R.CLASSES)
        _, b2, b3 = R.cam2lidar(rows, R.read_calib(os.path.join(root, 'training/calib', name + '.txt')))
        assert np.array_equal(fx['rows_%d' % f], rows.astype(np.float32))          # the same labels went in
        assert np.abs(b3 - fx['box3d_%d' % f]).max() < 2e-5
        assert np.array_equal(b3[:, 3:6], fx['box3d_%d' % f][:, 3:6])
        assert np.abs(R.corners(fx['box3d_%d' % f]) - fx['corners_%d' % f]).max() < 2e-5
        assert np.abs(R.bev(fx['box3d_%d' % f]) - fx['bev_%d' % f]).max() < 2e-5
        total += rows.shape[0]
    assert total >= 20


def test_box_iou_closed_forms():
    w, h = 40.0, 24.0
    a = np.array([[10.0, 20.0, 10.0 + w, 20.0 + h]], np.float32)
    for dx in (0.0, 4.0, 8.0, 39.0, 40.0, 55.0):
        want = max(w - dx, 0.0) / (w + dx) if dx < w else 0.0                      # shifted copy: (w - dx) h / ((w + dx) h)
        got = R.box_iou(a, a + np.array([dx, 0, dx, 0], np.float32))[0, 0]
        assert abs(float(got) - want) < 1e-6, dx
    inner = np.array([[20.0, 25.0, 30.0, 35.0]], np.float32)                       # nested: the ratio of the areas
    assert abs(float(R.box_iou(a, inner)[0, 0]) - 100.0 / (w * h)) < 1e-7
    both = R.box_iou(np.concatenate([a, inner]), np.concatenate([inner, a, a]))
    assert both.shape == (2, 3) and both[0, 1] == 1.0 and both[0, 0] == both[1, 1]
    # the first index that reaches the maximum
    assert int(np.argmax(both[0])) == 1


def test_raster_rule_on_known_shapes():
    """Pixel-centre even-odd fill: a rectangle, a concave L, two overlapping parts (their union), a hole by self-overlap."""
    sq, _ = R.raster([[1.2, 1.2, 5.7, 1.2, 5.7, 3.7, 1.2, 3.7]], [0, 0, 7, 5])
    want = np.zeros((6, 8), np.uint8)
    want[1:4, 1:6] = 1                                                             # centres 1.5 .. 5.5 x 1.5 .. 3.5
    assert np.array_equal(sq, want)
    ell, _ = R.raster([[0.1, 0.1, 4.1, 0.1, 4.1, 2.1, 2.1, 2.1, 2.1, 4.1, 0.1, 4.1]], [0, 0, 4, 4])
    assert ell.sum() == 4 * 2 + 2 * 2 and ell[3, 3] == 0 and ell[3, 1] == 1
    two, _ = R.raster([[0.1, 0.1, 3.1, 0.1, 3.1, 3.1, 0.1, 3.1], [2.1, 0.1, 5.1, 0.1, 5.1, 3.1, 2.1, 3.1]], [0, 0, 5, 3])
    assert two[:3, :5].all() and two[3].sum() == 0                                  # the union, not the parity of the parts
    # ROI offsets: the same polygon seen through a shifted window
    part, _ = R.raster([[1.2, 1.2, 5.7, 1.2, 5.7, 3.7, 1.2, 3.7]], [2, 1, 7, 5])
    assert np.array_equal(part, want[1:6, 2:8])


def test_label_preparation_and_packing_equal_the_restatement(tmp_path):
    """BuildGT.loadFrame / pack on the CPU: the label rows (class, frame, row order), boxes, annotation boxes and edges the
    kernels will read are the restatement's, bit for bit."""
    from modules.augment import BuildGT
    root, seg = _tree(tmp_path)
    r = R.build(root, seg)
    ann = BuildGT.readAnnotations(seg)
    train = set(open(os.path.join(root, 'ImageSets/train.txt')).read().splitlines())
    order = BuildGT.frameOrder(ann, train)
    assert order == r['order'] and len(order) == 5 and order[0][1] == '000005'     # reversed in the file; frame 1 has no instance
    frames = [BuildGT.loadFrame(root, name) for _, name in order]
    t = BuildGT.pack(frames, [ann.by_image[i] for i, _ in order], device='cpu')
    L = r['labels']
    assert t.n_labels == len(L['cls']) >= 20
    assert np.array_equal(t.lab_box2d.numpy(), L['box2d']) and np.array_equal(t.lab_box3d.numpy(), L['box3d'])
    assert np.array_equal(t.lab_frame.numpy(), L['frame'])
    assert [t.classes[g % 3] for g in t.lab_group.numpy()] == L['cls'].tolist()
    assert t.lab_cs.dtype == torch.float32 and np.array_equal(t.lab_cs[:, 0].numpy(), np.cos(L['box3d'][:, 6]))
    far = [k for k, fr in enumerate(frames) if fr['id'] == '000002'][0]
    assert all(frames[far]['labels'][c]['bbox3d'].shape[0] == 0 for c in BuildGT.CLASSES)      # all labels beyond the range
    assert t.ann_off.numel() == len(order) * 3 + 1 and int(t.ann_off[-1]) == t.n_ann
    assert t.edge_off.numel() == t.n_ann + 1 and int(t.edge_off[-1]) == t.edges.shape[0]
    assert t.images.shape == (len(order), 370, 1224, 3) and t.points.shape[0] == int(t.pts_off[-1])
    # annotation boxes and edges of the objects' instances
    seg_json = __import__('json').load(open(seg))
    for o in r['objects']['Car'][:6]:
        a = o['ann']
        e = t.edges[int(t.edge_off[a]):int(t.edge_off[a + 1])].numpy()
        x1, y1, x2, y2 = t.ann_box[a].numpy()
        assert [int(x1), int(y1)] == [max(int(x1), 0), max(int(y1), 0)] and o['maskbbox'][0] == int(x1)
        src = [s for s in seg_json['annotations'] if s['i_segm'] and abs(s['i_segm'][0][0] - e[0, 0]) < 1e-12 and abs(s['i_segm'][0][1] - e[0, 1]) < 1e-12]
        assert len(src) == 1 and e.shape[0] == sum(len(p) // 2 for p in src[0]['i_segm'])
        assert np.array_equal(e[:-1, 2:], e[1:, :2]) or len(src[0]['i_segm']) > 1


def built_from_ref(r, cls):
    """The restatement's objects of a class in the layout BuildGT.buildFrames returns, on the CPU."""
    objs = r['objects'][cls]
    px = np.cumsum([0] + [o['mask_px'].size for o in objs]).astype(np.int64)
    pt = np.cumsum([0] + [o['points'].shape[0] for o in objs]).astype(np.int64)
    cat = lambda xs, shape, dt: torch.from_numpy(np.concatenate(xs, 0).astype(dt).reshape(shape) if xs else np.zeros(tuple(max(s, 0) for s in shape), dt))
    tables = {'n': len(objs), 'box2d': cat([o['bbox2d'][None] for o in objs], (-1, 4), np.float32),
              'box3d': cat([o['bbox3d'][None] for o in objs], (-1, 7), np.float32),
              'maskbbox': cat([o['maskbbox'][None] for o in objs], (-1, 4), np.int32), 'px_off': torch.from_numpy(px),
              'mask': cat([o['mask_px'].reshape(-1) for o in objs], (-1,), np.uint8),
              'patch': cat([o['patch'].reshape(-1, 3) for o in objs], (-1, 3), np.uint8), 'pt_off': torch.from_numpy(pt),
              'points': cat([o['points'] for o in objs], (-1, 4), np.float32), 'ids': [o['id'] for o in objs]}
    infos = [{'velo': o['velo'], 'image': o['image'], 'mask': o['mask'], 'occlude': torch.tensor(o['occlude']),
              'maskbbox': torch.from_numpy(o['maskbbox']), 'bbox2d': torch.from_numpy(o['bbox2d']),
              'bbox3d': torch.from_numpy(o['bbox3d']), 'id': o['id']} for o in objs]
    return {'infos': infos, 'tables': tables}


def test_written_tree_round_trips_through_getAllGT(tmp_path):
    """writeObjects + gtinfo.pkl in the reference's layout: names, keys, per-class numbering; getAllGT reads back exactly the
    built tables -- points, masks and the patch in BGR order (the PNG holds RGB)."""
    from modules.augment import BuildGT
    from modules.augment.LoadGT import GTDatabase, getAllGT
    root, seg = _tree(tmp_path)
    r = R.build(root, seg)
    built = {c: built_from_ref(r, c) for c in R.CLASSES}
    for c in R.CLASSES:
        BuildGT.writeObjects(root, c, built[c])
    with open(os.path.join(root, 'training/gtdatabase/gtinfo.pkl'), 'wb') as f:
        pickle.dump({c: built[c]['infos'] for c in R.CLASSES}, f)
    gts = getAllGT(list(R.CLASSES), root=root)
    assert sum(len(v) for v in gts.values()) >= 12 and len(gts['Car']) >= 8
    for c in R.CLASSES:
        d = os.path.join(root, 'training/gtdatabase', c)
        n = len(built[c]['infos'])
        assert sorted(os.listdir(d)) == sorted(['velo_%06d.bin' % k for k in range(n)] + ['img_%06d.png' % k for k in range(n)]
                                               + ['mask_%06d.npy' % k for k in range(n)])
        for k, (g, o) in enumerate(zip(gts[c], r['objects'][c])):
            assert np.array_equal(g['velo'], o['points']) and g['velo'].dtype == np.float32
            assert np.array_equal(g['mask'], o['mask_px']) and set(np.unique(g['mask'])) <= {0, 1}
            assert np.array_equal(g['image'], o['patch'])                           # BGR, as cv2.imread gives it
            assert [int(v) for v in g['maskbbox']] == o['maskbbox'].tolist()
            assert np.array_equal(g['bbox2d'].numpy(), o['bbox2d']) and np.array_equal(g['bbox3d'].numpy(), o['bbox3d'])
            assert g['mask'].shape == (o['maskbbox'][3] - o['maskbbox'][1] + 1, o['maskbbox'][2] - o['maskbbox'][0] + 1)
    from PIL import Image
    o = r['objects']['Car'][0]
    with Image.open(os.path.join(root, 'training/gtdatabase/Car', o['image'])) as im:
        assert np.array_equal(np.asarray(im.convert('RGB')), o['patch'][:, :, ::-1])
    # the reference's pickle keys
    info = pickle.load(open(os.path.join(root, 'training/gtdatabase/gtinfo.pkl'), 'rb'))
    assert set(info) == {'Car', 'Pedestrian', 'Cyclist'}
    assert set(info['Car'][0]) == {'velo', 'image', 'mask', 'occlude', 'maskbbox', 'bbox2d', 'bbox3d', 'id'}
    # the tables pack as loaded objects do
    calibs = {n: R.read_calib(os.path.join(root, 'training/calib', n + '.txt')) for _, n in r['order']}
    a, b = GTDatabase.from_built(built, calibs, 'cpu'), GTDatabase.from_gts(gts['Car'], 'cpu')
    for k in ('box2d', 'box3d', 'bev', 'pt_off', 'points', 'px_off', 'patch', 'mask', 'maskbbox'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_script_and_symbols_exist():
    from modules import Extension as X
    for name in ('mvx_gtdb_workspace_bytes', 'mvx_gtdb_match', 'mvx_gtdb_crop_count', 'mvx_gtdb_crop_write', 'mvx_gtdb_raster'):
        assert name in X.PROTOTYPES and hasattr(X.lib, name)
    assert X.lib.mvx_gtdb_workspace_bytes(10, 20000) >= 10 * 20 * 4
    assert X.lib.mvx_gtdb_match(None, None, None, 1, None, None, 1, None, 1, 0.65, None, None, None, None, None, None) == -1
    import create_gtdatabase_like
    assert callable(create_gtdatabase_like.build_tree)
