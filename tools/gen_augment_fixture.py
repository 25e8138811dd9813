"""Records tests/golden/augment_ref.npz from the reference implementation's own GT-paste augmentation.

    python tools/gen_augment_fixture.py <path to the reference tree> [output.npz]

The reference's modules/augment/Augment.py is imported at run time from the given tree and run unchanged on synthetic frames
and a synthetic object database (modules/data/Synthetic.write_gt_database).  Libraries this stack does not have are stood in
for before the import: ``numba.njit`` is the identity, ``torchvision.ops.boxes.box_area`` is supplied, the three OpenCV
calls it makes (``bitwise_and`` with a mask, ``add``) are numpy, ``shapely`` is an empty module, and ``cpp.bboxOverlap`` is
the C oracle's box-against-box IoU (the reference's own never loads its second box -- the one deliberate difference that
cannot be recorded otherwise).  The run is seeded per frame with ``np.random.seed(SEED0 + frame)``.

Recorded per frame f: the scene cloud and boxes that went in, the picked objects per slot (database indices), the final
boxes and bevs, the pasted image, and the rows [x y z r row col] (float32) of the pasted objects as train.py:37-42
concatenates them; the ``check`` grid of frame 1.  The database is not stored: the test regenerates it from (DB_OBJECTS,
DB_SEED)."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB_OBJECTS, DB_SEED, SCENE_SEED, SEED0, POINTS = 120, 3, 11, 100, 3000
SCENE_BOXES = (0, 3, 12, 13, 6)
IMSIZE_HW = (370, 1224)


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _read_calib(path):
    out = {}
    lines = open(path).read().splitlines()
    for row, shape in ((5, (3, 4)), (2, (3, 4)), (4, (3, 3))):
        tok = lines[row].split(' ')
        m = np.zeros((4, 4))
        m[:shape[0], :shape[1]] = np.array(tok[1:]).astype('float32').reshape(shape)
        m[3, 3] = 1
        out[tok[0][:-1]] = m
    return out


def image_of(f):
    """A smooth deterministic image (it has to compress)."""
    yy, xx = np.mgrid[0:IMSIZE_HW[0], 0:IMSIZE_HW[1]]
    return np.stack([(xx // 4 + yy // 2 + 40 * c + 17 * f) % 256 for c in range(3)], 2).astype(np.uint8)


def load_objects(root, infos, cls='Car'):
    from PIL import Image
    gts = []
    for info in infos:
        d = os.path.join(root, 'training', 'gtdatabase', cls)
        with Image.open(os.path.join(d, info['image'])) as im:
            bgr = np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])
        gts.append({'velo': np.fromfile(os.path.join(d, info['velo']), dtype='float32').reshape(-1, 4), 'image': bgr,
                    'mask': np.load(os.path.join(d, info['mask'])), 'maskbbox': info['maskbbox'], 'bbox2d': info['bbox2d'],
                    'bbox3d': info['bbox3d'], 'calib': _read_calib(os.path.join(root, 'training', 'calib', info['id'] + '.txt'))})
    return gts


def main(ref_root, out_path):
    S = _load_by_path('mvx_synthetic', os.path.join(REPO, 'mvxnet-makise_amd', 'modules', 'data', 'Synthetic.py'))
    sys.path.insert(0, os.path.join(REPO, 'oracle'))
    import mvx_oracle as O

    # ---- stand-ins, then the reference's module
    numba = types.ModuleType('numba')
    numba.njit = lambda fn: fn
    cv2 = types.ModuleType('cv2')
    cv2.bitwise_and = lambda a, b, mask=None: a * (np.asarray(mask)[..., None] != 0).astype(a.dtype)
    cv2.add = lambda a, b: np.clip(a.astype(np.int32) + b.astype(np.int32), 0, 255).astype(np.uint8)
    tv, tvo, tvb = types.ModuleType('torchvision'), types.ModuleType('torchvision.ops'), types.ModuleType('torchvision.ops.boxes')
    tvb.box_area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    shp, shg = types.ModuleType('shapely'), types.ModuleType('shapely.geometry')
    shg.Polygon = object
    ext = types.ModuleType('modules.Extension')
    ext.cpp = types.SimpleNamespace(bboxOverlap=lambda b1, b2: O.bbox_pairwise(np.asarray(b1), np.asarray(b2), True))
    sys.modules.update({'numba': numba, 'cv2': cv2, 'torchvision': tv, 'torchvision.ops': tvo, 'torchvision.ops.boxes': tvb,
                        'shapely': shp, 'shapely.geometry': shg})
    sys.argv = sys.argv[:1]
    os.chdir(ref_root)
    sys.path[:] = [ref_root] + [p for p in sys.path if 'mvxnet-makise_amd' not in p]          # `modules` is the reference's package here
    for name in [m for m in sys.modules if m == 'modules' or m.startswith('modules.')]:          # the oracle imported this package's
        del sys.modules[name]
    import modules                                                   # noqa: F401  (the reference's package)
    sys.modules['modules.Extension'] = ext
    lgt = types.ModuleType('modules.augment.LoadGT')                 # its loader needs pandas / OpenCV: objects are read by load_objects
    lgt.getAllGT = None
    sys.modules['modules.augment.LoadGT'] = lgt
    from modules.augment import Augment as RA
    from modules.Calc import bbox3d2bev
    from modules.utils import lidar2Img

    rec = {'db_objects': DB_OBJECTS, 'db_seed': DB_SEED, 'seed0': SEED0, 'n_frames': len(SCENE_BOXES)}
    with tempfile.TemporaryDirectory() as tmp:
        infos = S.write_gt_database(tmp, DB_OBJECTS, seed=DB_SEED)
        gts = load_objects(tmp, infos)
        with tempfile.TemporaryDirectory() as tmp2:
            scene_infos = S.write_gt_database(tmp2, 40, seed=SCENE_SEED, points=(5, 6))
        at = 0
        for f, nb in enumerate(SCENE_BOXES):
            pcd = S.synth_ring(f, POINTS)
            img = image_of(f)
            b2 = b3 = bev = None
            if nb:
                b2 = torch.stack([i['bbox2d'] for i in scene_infos[at:at + nb]])
                b3 = torch.stack([i['bbox3d'] for i in scene_infos[at:at + nb]])
                bev = bbox3d2bev(b3)
                at += nb
            np.random.seed(SEED0 + f)
            velos, calibs, out_img, o3, obev = RA.augmentTargetClasses(pcd, img, b2, b3, bev, {'Car': gts}, ['Car'], [12])
            o3, obev = o3['Car'], obev['Car']
            n0 = nb
            picked = []
            for k in range(o3.shape[0] - n0 if nb <= 12 else 0):
                hit = [j for j, g in enumerate(gts) if torch.equal(g['bbox3d'], o3[n0 + k])]
                picked.append(hit[0])
            rows = [np.zeros((0, 6), np.float32)]
            for ap, ac in zip(velos, calibs):
                proj = lidar2Img(ap, ac, True)[:, ::-1]
                rows.append(np.concatenate([ap, proj], axis=1).astype(np.float32))
            rec['pcd_%d' % f] = pcd
            rec['in_box2d_%d' % f] = np.zeros((0, 4), np.float32) if b2 is None else b2.numpy()
            rec['in_box3d_%d' % f] = np.zeros((0, 7), np.float32) if b3 is None else b3.numpy()
            rec['in_bev_%d' % f] = np.zeros((0, 4, 2), np.float32) if bev is None else bev.numpy()
            rec['picked_%d' % f] = np.asarray(picked, np.int32)
            rec['box3d_%d' % f] = o3.numpy()
            rec['bev_%d' % f] = obev.numpy()
            rec['img_%d' % f] = out_img
            rec['rows_%d' % f] = np.concatenate(rows, 0)
            if f == 1:
                rec['check_1'] = RA.check(pcd, RA.cfg.velorange).astype(np.float32)
            print('frame %d: %d scene boxes, %d pasted' % (f, nb, len(picked)))
    np.savez_compressed(out_path, **rec)
    print('wrote %s (%d bytes)' % (out_path, os.path.getsize(out_path)))


if __name__ == '__main__':
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    main(os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(REPO, 'tests', 'golden', 'augment_ref.npz'))
