"""The ground-truth object database of the GT-paste augmentation (reference modules/augment/LoadGT.py).

``getAllGT(['Car'])`` reads ``training/gtdatabase/gtinfo.pkl`` and every object's ``.bin`` point cloud, image patch and
``.npy`` mask in the reference's layout and returns its ``{cls: [dict, ...]}`` structure.  ``GTDatabase.from_gts`` packs one
class into the flat tables the kernels read (include/mvx_hip.h, "GT-paste augmentation").  Differences from the reference:
images are decoded with PIL into BGR (as modules/data/Load.py); the data root is an argument; points outside the crop range
or that do not project into their source image are dropped once, here (the reference fails later, in the voxelizer's index
or in featureMaping's assert); masks count as zero / non-zero."""
import os
import pickle as pkl

import numpy as np
import torch

import modules.config as cfg
from modules.data import Load


def readGTInfo(root=None):
    root = Load.dataroot if root is None else root
    with open(os.path.join(root, 'training/gtdatabase/gtinfo.pkl'), 'rb') as f:
        return pkl.load(f)


def getGTByInfo(info, cls, root=None):
    root = Load.dataroot if root is None else root
    gtroot = os.path.join(root, 'training/gtdatabase', cls)
    velo = np.fromfile(os.path.join(gtroot, info['velo']), dtype='float32').reshape((-1, 4))
    img = Load._read_image(os.path.join(gtroot, info['image']))
    mask = np.load(os.path.join(gtroot, info['mask']))
    calib = Load.readCalib(os.path.join(root, 'training/calib', info['id'] + '.txt'))
    return velo, img, mask, info['maskbbox'], info['bbox2d'], info['bbox3d'], calib


def getAllGT(targetCls, root=None, quiet=True):
    """{cls: [{'velo', 'image', 'mask', 'maskbbox', 'bbox2d', 'bbox3d', 'calib'}, ...]} (reference LoadGT.py:34-56);
    'bbox2d' / 'bbox3d' are float32 tensors."""
    gtinfo = readGTInfo(root)
    res = {}
    for c in targetCls:
        cur = []
        for i, info in enumerate(gtinfo[c]):
            if not quiet:
                print('\rLoading %s %d/%d' % (c, i + 1, len(gtinfo[c])), end=' ')
            velo, img, mask, maskbbox, bbox2d, bbox3d, calib = getGTByInfo(info, c, root)
            cur.append({'velo': velo, 'image': img, 'mask': mask, 'maskbbox': maskbbox,
                        'bbox2d': torch.as_tensor(np.asarray(bbox2d), dtype=torch.float32),
                        'bbox3d': torch.as_tensor(np.asarray(bbox3d), dtype=torch.float32), 'calib': calib})
        res[c] = cur
    return res


def project_rows_cols(velo, calib):
    """(row, col) of every point as train.py:38-40 yields them: the numpy path of lidar2Img (float64 on the float32 points,
    reference Calib.py:57-70), swapped; plus the camera depth.  Host arithmetic -- it runs once per object, at load."""
    pts = np.empty((4, velo.shape[0]), dtype='float32')
    pts[:3] = velo[:, :3].T
    pts[3] = 1
    r0, tr, p2 = (np.asarray(calib[k], dtype=np.float64) for k in ('R0_rect', 'Tr_velo_to_cam', 'P2'))
    cam = r0 @ tr @ pts
    im = p2 @ cam
    with np.errstate(divide='ignore', invalid='ignore'):
        uv = im[:2] / im[2]
    return uv[::-1].T, cam[2]


class GTDatabase:
    """One class of the database as flat tables (``n`` objects), on ``device``:
    box2d f32 (n,4), box3d f32 (n,7), bev f32 (n,4,2) = Calc.bbox3d2bev(box3d); pt_off i64 (n+1,), points f32 (sum,6) =
    [x y z r row col]; px_off i64 (n+1,), patch u8 (sum_px,3) BGR, mask u8 (sum_px,), maskbbox i32 (n,4) x1 y1 x2 y2
    inclusive, clipped to the patch that is really there.  ``gts`` keeps the source dicts and ``velo_kept`` every object's
    kept points (n,4) on the host (what the single-frame ``augment`` returns with the object's 'calib')."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @classmethod
    def from_gts(cls, gts, device, velorange=None, imsize=None):
        from modules import Calc
        rng = cfg.velorange if velorange is None else velorange
        imsize = cfg.imsize if imsize is None else imsize          # (h, w)
        lo, hi = np.asarray(rng[:3], np.float64), np.asarray(rng[3:], np.float64)
        n = len(gts)
        if n == 0:
            raise ValueError('an empty object database')
        box2d = torch.stack([torch.as_tensor(np.asarray(g['bbox2d']), dtype=torch.float32).reshape(4) for g in gts])
        box3d = torch.stack([torch.as_tensor(np.asarray(g['bbox3d']), dtype=torch.float32).reshape(-1)[:7] for g in gts])
        bev = torch.stack([Calc.bbox3d2bev(b) for b in box3d])      # per object, as locate calls it (Augment.py:44)
        pts, pt_off, dropped = [], [0], 0
        patches, masks, px_off, mbb = [], [], [0], []
        for g in gts:
            velo = np.ascontiguousarray(g['velo'], dtype=np.float32).reshape(-1, 4)
            rc, depth = project_rows_cols(velo, g['calib'])
            xyz = velo[:, :3].astype(np.float64)
            keep = np.all((lo <= xyz) & (xyz < hi), axis=1) & (depth > 0) & (rc[:, 0] >= 0) & (rc[:, 1] >= 0) \
                & (rc[:, 0] < imsize[0] - 1e-3) & (rc[:, 1] < imsize[1] - 1e-3)
            dropped += int((~keep).sum())
            pts.append(np.concatenate([velo[keep], rc[keep].astype(np.float32)], axis=1))
            pt_off.append(pt_off[-1] + int(keep.sum()))
            x1, y1, x2, y2 = (int(v) for v in g['maskbbox'])
            m = np.asarray(g['mask'])
            im = np.asarray(g['image'])
            h, w = min(y2 - y1 + 1, m.shape[0], im.shape[0]), min(x2 - x1 + 1, m.shape[1], im.shape[1])
            h, w = max(h, 0), max(w, 0)
            patches.append(np.ascontiguousarray(im[:h, :w, :3], dtype=np.uint8).reshape(-1, 3))
            masks.append((m[:h, :w] != 0).astype(np.uint8).reshape(-1))
            px_off.append(px_off[-1] + h * w)
            mbb.append([x1, y1, x1 + w - 1, y1 + h - 1])
        dev = torch.device(device)
        points = np.concatenate(pts, 0) if pt_off[-1] else np.zeros((0, 6), np.float32)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        px = np.diff(np.asarray(px_off, np.int64))
        pad = lambda a, rows: np.concatenate([a, np.zeros((rows,) + a.shape[1:], a.dtype)], 0) if a.shape[0] == 0 else a
        return cls(n=n, gts=gts, device=dev, box2d=box2d.to(dev), box3d=box3d.to(dev), bev=bev.contiguous().to(dev),
                   pt_off=to(np.asarray(pt_off, np.int64)), points=to(pad(points, 1)), px_off=to(np.asarray(px_off, np.int64)),
                   patch=to(pad(np.concatenate(patches, 0), 1)), mask=to(pad(np.concatenate(masks, 0), 1)),
                   maskbbox=to(np.asarray(mbb, np.int32)), max_patch_px=max(1, int(px.max())),
                   max_points=int(np.diff(np.asarray(pt_off)).max()), dropped_points=dropped, velo_kept=[p[:, :4] for p in pts])

    @classmethod
    def from_built(cls, built, calibs, device, name='Car', velorange=None, imsize=None):
        """The database of class ``name`` from what ``BuildGT.buildFrames`` returned (one result or a list of them, in order),
        without going through the disk: the objects' tables are read back once and packed as ``from_gts`` packs loaded
        objects (the row / col columns are the host projection with the object's own calibration, as there).  ``calibs``:
        {frame id: calib dict as Load.readCalib returns it}."""
        from modules.augment import BuildGT
        gts = []
        for b in (built if isinstance(built, (list, tuple)) else [built]):
            gts += BuildGT.objectsOf(b[name], calibs)
        return cls.from_gts(gts, device, velorange, imsize)

    def nbytes(self):
        """Resident size of the tables in bytes."""
        return sum(t.numel() * t.element_size() for t in self.__dict__.values() if isinstance(t, torch.Tensor))

    def to(self, device):
        kw = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in self.__dict__.items()}
        kw['device'] = torch.device(device)
        return GTDatabase(**kw)
