"""Synthetic KITTI-shaped inputs: there is no dataset on the GPU box.

S1 "uniform": 20,000 points uniform in the crop range (worst case, ~1 point per voxel).
S2 "ring": 64-beam spinning-lidar model over flat ground with box occluders, cropped to the
range and the camera frustum, subsampled to 20,000 points (KITTI-like occupancy).
Seeds: 1000+frame (points), 2000+frame (shuffle), 3000+frame (FPN maps).  Host-side numpy:
data generation is not part of the hot path.
"""
import numpy as np

VELORANGE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]


def _crop(pcd, rng):
    lo, hi = np.asarray(rng[:3], np.float64), np.asarray(rng[3:], np.float64)
    roi = pcd[:, :3].astype(np.float64)
    return pcd[np.all((lo <= roi) & (roi < hi), axis=1)]


def _crop_to_sight(pcd, calib, imsize_wh):
    pts = np.ones((4, pcd.shape[0]), np.float64)
    pts[:3] = pcd[:, :3].T
    cam = (calib['R0_rect'] @ calib['Tr_velo_to_cam']) @ pts
    img = calib['P2'] @ cam
    with np.errstate(divide='ignore', invalid='ignore'):
        u, v = img[0] / img[2], img[1] / img[2]
    lim = np.asarray(imsize_wh, np.float64) - 1e-3
    return pcd[(cam[2] > 0) & (u >= 0) & (v >= 0) & (u < lim[0]) & (v < lim[1])]


KITTI_CALIB = {
    # public KITTI 2011_09_26 object calibration, padded to 4x4 as
    # modules/data/Load.py:24-41 does (values parsed as float32 there).
    'P2': np.array([[721.5377, 0.0, 609.5593, 44.85728],
                    [0.0, 721.5377, 172.854, 0.2163791],
                    [0.0, 0.0, 1.0, 0.002745884],
                    [0.0, 0.0, 0.0, 1.0]], dtype=np.float32).astype(np.float64),
    'R0_rect': np.array([[0.9999239, 0.00983776, -0.007445048, 0.0],
                         [-0.009869795, 0.9999421, -0.004278459, 0.0],
                         [0.007402527, 0.004351614, 0.9999631, 0.0],
                         [0.0, 0.0, 0.0, 1.0]], dtype=np.float32).astype(np.float64),
    'Tr_velo_to_cam': np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766],
                                [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                                [0.9998621, 0.00752379, 0.01480755, -0.2717806],
                                [0.0, 0.0, 0.0, 1.0]], dtype=np.float32).astype(np.float64),
}


def synth_uniform(frame_id: int, P: int = 20000, rng=VELORANGE) -> np.ndarray:
    """S1 'uniform' frame: (P,4) f32 inside the crop range."""
    g = np.random.default_rng(1000 + frame_id)
    lo = np.asarray(rng[:3], np.float32)
    hi = np.asarray(rng[3:], np.float32)
    xyz = (g.random((P, 3)) * (hi - lo) + lo).astype(np.float32)
    xyz = np.minimum(xyz, np.nextafter(hi, -np.inf, dtype=np.float32))
    xyz = np.maximum(xyz, lo)
    r = g.random((P, 1)).astype(np.float32)
    return np.concatenate([xyz, r], axis=1)


def synth_uniform_in_sight(frame_id: int, P: int = 20000, rng=VELORANGE, calib=None, imsize_wh=(1224, 370)) -> np.ndarray:
    """S1 'uniform' for runs WITH image fusion: uniform in the crop range, restricted to the camera frustum (every point
    must project into the image, modules/imhead/Pipe.py:71), P points; still about one point per voxel."""
    calib = KITTI_CALIB if calib is None else calib
    g = np.random.default_rng(1000 + frame_id)
    lo = np.asarray(rng[:3], np.float32)
    hi = np.asarray(rng[3:], np.float32)
    parts, have = [], 0
    while have < P:
        xyz = (g.random((4 * P, 3)) * (hi - lo) + lo).astype(np.float32)
        xyz = np.maximum(np.minimum(xyz, np.nextafter(hi, -np.inf, dtype=np.float32)), lo)
        pc = np.concatenate([xyz, g.random((4 * P, 1)).astype(np.float32)], axis=1)
        pc = _crop_to_sight(_crop(pc, rng), calib, imsize_wh)
        parts.append(pc)
        have += pc.shape[0]
    return np.ascontiguousarray(np.concatenate(parts, 0)[:P])


def synth_raw_around(kept: np.ndarray, frame_id: int, total: int = 120000, rng=VELORANGE, calib=None,
                     imsize_wh=(1224, 370)) -> np.ndarray:
    """A raw (un-cropped) cloud of `total` points whose crop + cropToSight is exactly `kept`, in the same order: the kept
    points interleaved with points that fail the range crop or the frustum test (what cropdata.py / Load.py read from
    disk before cropping)."""
    calib = KITTI_CALIB if calib is None else calib
    g = np.random.default_rng(4000 + frame_id)
    need = total - kept.shape[0]
    assert need >= 0
    if need == 0:
        return np.ascontiguousarray(kept[:, :4], np.float32)
    rejected, have = [], 0
    while have < need:
        cand = np.stack([g.uniform(-80, 80, 2 * need + 16), g.uniform(-80, 80, 2 * need + 16), g.uniform(-4, 3, 2 * need + 16),
                         g.random(2 * need + 16)], axis=1).astype(np.float32)
        lo, hi = np.asarray(rng[:3], np.float64), np.asarray(rng[3:], np.float64)
        roi = cand[:, :3].astype(np.float64)
        in_range = np.all((lo <= roi) & (roi < hi), axis=1)
        bad = cand[~in_range]
        inr = cand[in_range]
        if inr.shape[0]:
            ok = _crop_to_sight(inr, calib, imsize_wh)
            # in-range points outside the frustum: everything in `inr` that is not in `ok` (rows are unique with probability 1)
            keep_rows = {r.tobytes() for r in ok}
            outside = np.array([r for r in inr if r.tobytes() not in keep_rows], np.float32).reshape(-1, 4)
            bad = np.concatenate([bad, outside], 0)
        rejected.append(bad)
        have += bad.shape[0]
    rej = np.concatenate(rejected, 0)[:need]
    slot = np.zeros(total, bool)
    slot[np.sort(g.choice(total, kept.shape[0], replace=False))] = True
    out = np.empty((total, 4), np.float32)
    out[slot] = kept[:, :4]
    out[~slot] = rej
    return out


def synth_raw(frame_id: int, P: int = 120000) -> np.ndarray:
    """Raw un-cropped cloud for the crop/cropToSight config."""
    g = np.random.default_rng(1000 + frame_id)
    x = g.uniform(-80, 80, P)
    y = g.uniform(-80, 80, P)
    z = g.uniform(-4, 3, P)
    r = g.random(P)
    return np.stack([x, y, z, r], axis=1).astype(np.float32)


def synth_ring(frame_id: int, P: int = 20000, rng=VELORANGE, calib=None,
               imsize_wh=(1224, 370)) -> np.ndarray:
    """S2 'ring' frame: 64-beam spinning-lidar model over flat ground with box
    occluders, cropped to range + camera frustum, subsampled to P points."""
    calib = KITTI_CALIB if calib is None else calib
    g = np.random.default_rng(1000 + frame_id)
    elev = np.deg2rad(np.linspace(-24.8, 2.0, 64))
    azim = np.deg2rad(np.arange(-45.0, 45.0, 0.09))
    pts = []
    nbox = 12
    bc = np.stack([g.uniform(5, 60, nbox), g.uniform(-20, 20, nbox)], 1)
    bs = np.stack([g.uniform(1.5, 4.5, nbox), g.uniform(1.5, 2.5, nbox), g.uniform(1.4, 2.5, nbox)], 1)
    h = 1.73
    for rep in range(4):                                 # several sweeps with jitter -> enough points
        az = (azim + g.normal(0, 2e-4, azim.size))[None, :]
        el = (elev + g.normal(0, 2e-4, elev.size))[:, None]
        dx, dy, dz = np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)
        with np.errstate(divide='ignore'):
            t = np.where(dz < 0, -h / dz, np.inf)
        t = np.minimum(t, 120.0)
        for k in range(nbox):                            # ray/AABB slab test
            lo = np.array([bc[k, 0] - bs[k, 0] / 2, bc[k, 1] - bs[k, 1] / 2, -h])
            hi = np.array([bc[k, 0] + bs[k, 0] / 2, bc[k, 1] + bs[k, 1] / 2, -h + bs[k, 2]])
            with np.errstate(divide='ignore', invalid='ignore'):
                t1 = np.stack([lo[0] / dx, lo[1] / dy, lo[2] / dz])
                t2 = np.stack([hi[0] / dx, hi[1] / dy, hi[2] / dz])
            tn = np.nanmax(np.minimum(t1, t2), axis=0)
            tf = np.nanmin(np.maximum(t1, t2), axis=0)
            hit = (tn <= tf) & (tn > 0)
            t = np.where(hit & (tn < t), tn, t)
        t = t * (1 + g.normal(0, 2e-3, t.shape))
        ok = np.isfinite(t) & (t < 119.0)
        p = np.stack([(t * dx)[ok], (t * dy)[ok], (t * dz)[ok], g.random(int(ok.sum()))], 1)
        pts.append(p.astype(np.float32))
    pcd = np.concatenate(pts, 0)
    pcd = _crop(pcd, rng)
    pcd = _crop_to_sight(pcd, calib, imsize_wh)
    if pcd.shape[0] >= P:
        sel = np.sort(g.choice(pcd.shape[0], P, replace=False))
        pcd = pcd[sel]
    return np.ascontiguousarray(pcd)


def synth_perm(frame_id: int, P: int) -> np.ndarray:
    return np.random.default_rng(2000 + frame_id).permutation(P).astype(np.int32)


def synth_fpn(frame_id: int, shapes=((256, 104, 336), (256, 52, 168), (256, 26, 84))):
    g = np.random.default_rng(3000 + frame_id)
    return [g.standard_normal(s, dtype=np.float32) for s in shapes]


def write_kitti_tree(root: str, frame_ids, points: int = 20000, raw_points: int = 120000, cars: int = 6, seed: int = 0):
    """A KITTI-format directory tree with synthetic frames, for the reader / training-loop tests (there is no dataset on
    the GPU box): training/{velodyne, velodyne_croped, label_2, calib, image_2} and ImageSets/train.txt, in the layout
    modules/data/Load.py:17-20 and cropdata.py:21-28 expect.  Labels hold `cars` random 'Car' boxes (camera frame, KITTI
    column order) plus one 'Pedestrian' row that the reader must skip."""
    import os
    from PIL import Image
    t = os.path.join(root, 'training')
    for d in ('velodyne', 'velodyne_croped', 'label_2', 'calib', 'image_2'):
        os.makedirs(os.path.join(t, d), exist_ok=True)
    os.makedirs(os.path.join(root, 'ImageSets'), exist_ok=True)
    names = []
    v2c = KITTI_CALIB['Tr_velo_to_cam']
    for fid in frame_ids:
        name = '%06d' % fid
        names.append(name)
        pc = synth_ring(fid, points)
        pc.tofile(os.path.join(t, 'velodyne_croped', name + '.bin'))
        synth_raw_around(pc, fid, raw_points).tofile(os.path.join(t, 'velodyne', name + '.bin'))
        g = np.random.default_rng(seed * 1000 + fid)
        img = g.integers(0, 256, (375, 1242, 3), dtype=np.uint8)
        Image.fromarray(img).save(os.path.join(t, 'image_2', name + '.png'))
        with open(os.path.join(t, 'calib', name + '.txt'), 'w') as f:
            p2 = ' '.join('%.6e' % v for v in KITTI_CALIB['P2'][:3].reshape(-1))
            r0 = ' '.join('%.6e' % v for v in KITTI_CALIB['R0_rect'][:3, :3].reshape(-1))
            tr = ' '.join('%.6e' % v for v in v2c[:3].reshape(-1))
            f.write('P0: %s\nP1: %s\nP2: %s\nP3: %s\nR0_rect: %s\nTr_velo_to_cam: %s\nTr_imu_to_velo: %s\n' % (p2, p2, p2, p2, r0, tr, tr))
        with open(os.path.join(t, 'label_2', name + '.txt'), 'w') as f:
            for k in range(cars):
                # a car in the lidar frame, written in the camera frame (inverse of modules/Calc.py bboxCam2Lidar)
                x, y, z = g.uniform(8, 60), g.uniform(-20, 20), g.uniform(-1.8, -1.2)
                l, w, h = g.uniform(3.4, 4.4), g.uniform(1.5, 1.8), g.uniform(1.4, 1.7)
                yaw = g.choice([0.0, np.pi / 2]) + g.normal(0, 0.05)
                cam = v2c @ np.array([x, y, z, 1.0])
                ry = yaw + 0.5 * np.pi
                f.write('Car 0.00 0 0.00 100.00 100.00 200.00 200.00 %.4f %.4f %.4f %.4f %.4f %.4f %.4f\n'
                        % (h, w, l, cam[0], cam[1], cam[2], ry))
            f.write('Pedestrian 0.00 0 0.00 10.00 10.00 20.00 20.00 1.70 0.60 0.80 1.00 1.50 10.00 0.10\n')
    with open(os.path.join(root, 'ImageSets', 'train.txt'), 'w') as f:
        f.write('\n'.join(names) + '\n')
    return names


def write_gt_database(root: str, n_objects: int, seed: int = 0, cls: str = 'Car', imsize_wh=(1224, 370), points=(40, 400),
                      n_calib: int = 4):
    """A synthetic ``training/gtdatabase/`` in the layout the reference's modules/augment/LoadGT.py reads, so that the GT-paste
    augmentation runs without the dataset: ``gtinfo.pkl`` = {cls: [info, ...]} and per object ``<cls>/<k>.bin`` (its points
    (n,4) f32, on the faces of its box), ``<k>.png`` (the image patch), ``<k>_mask.npy`` (u8 0/1, an ellipse) with
    ``info`` = {'velo', 'image', 'mask' (file names), 'maskbbox' (x1 y1 x2 y2 inclusive), 'bbox2d' (the projected 3-D
    corners' extent, clipped to the image), 'bbox3d' (xyzlwhr, LiDAR frame), 'id' (the source frame, whose
    ``training/calib/<id>.txt`` is written when it is missing)}.  Returns the info list."""
    import os
    import pickle
    import torch
    from PIL import Image
    g = np.random.default_rng(7000 + seed)
    t = os.path.join(root, 'training')
    odir = os.path.join(t, 'gtdatabase', cls)
    os.makedirs(odir, exist_ok=True)
    os.makedirs(os.path.join(t, 'calib'), exist_ok=True)
    ids = ['%06d' % k for k in range(n_calib)]
    for name in ids:
        path = os.path.join(t, 'calib', name + '.txt')
        if not os.path.exists(path):
            with open(path, 'w') as f:
                p2 = ' '.join('%.6e' % v for v in KITTI_CALIB['P2'][:3].reshape(-1))
                r0 = ' '.join('%.6e' % v for v in KITTI_CALIB['R0_rect'][:3, :3].reshape(-1))
                tr = ' '.join('%.6e' % v for v in KITTI_CALIB['Tr_velo_to_cam'][:3].reshape(-1))
                f.write('P0: %s\nP1: %s\nP2: %s\nP3: %s\nR0_rect: %s\nTr_velo_to_cam: %s\nTr_imu_to_velo: %s\n' % (p2, p2, p2, p2, r0, tr, tr))
    proj = KITTI_CALIB['P2'] @ KITTI_CALIB['R0_rect'] @ KITTI_CALIB['Tr_velo_to_cam']
    W, H = imsize_wh
    infos = []
    for k in range(n_objects):
        x = g.uniform(8, 62)
        y = g.uniform(-min(20.0, 0.6 * x), min(20.0, 0.6 * x))
        z = g.uniform(-1.8, -1.2)
        l, w, h = g.uniform(3.4, 4.4), g.uniform(1.5, 1.8), g.uniform(1.4, 1.7)
        yaw = g.choice([0.0, np.pi / 2]) + g.normal(0, 0.05)
        box = np.array([x, y, z, l, w, h, yaw], np.float32)
        # points on the four sides and the roof, box frame -> LiDAR frame with Calc.bbox3d2bev's rotation convention
        n = int(g.integers(points[0], points[1]))
        face = g.integers(0, 5, n)
        u, v = g.uniform(-0.5, 0.5, n), g.uniform(0, 1, n)
        px = np.where(face == 0, 0.5, np.where(face == 1, -0.5, u)) * l
        py = np.where(face == 2, 0.5, np.where(face == 3, -0.5, np.where(face < 2, u, g.uniform(-0.5, 0.5, n)))) * w
        pz = np.where(face == 4, 1.0, v) * h
        c, s = np.cos(yaw), np.sin(yaw)
        velo = np.stack([px * c + py * s + x, -px * s + py * c + y, pz + z, g.random(n)], 1).astype(np.float32)
        cx = np.array([0.5, -0.5, -0.5, 0.5, 0.5, -0.5, -0.5, 0.5]) * l
        cy = np.array([0.5, 0.5, -0.5, -0.5, 0.5, 0.5, -0.5, -0.5]) * w
        cz = np.array([0, 0, 0, 0, 1, 1, 1, 1.0]) * h
        corners = np.stack([cx * c + cy * s + x, -cx * s + cy * c + y, cz + z, np.ones(8)], 0)
        im = proj @ corners
        uu, vv = im[0] / im[2], im[1] / im[2]
        b2 = np.array([np.clip(uu.min(), 0, W - 1), np.clip(vv.min(), 0, H - 1), np.clip(uu.max(), 0, W - 1),
                       np.clip(vv.max(), 0, H - 1)], np.float32)
        x1, y1, x2, y2 = int(np.floor(b2[0])), int(np.floor(b2[1])), int(np.ceil(b2[2])), int(np.ceil(b2[3]))
        x2, y2 = min(max(x2, x1), W - 1), min(max(y2, y1), H - 1)
        ph, pw = y2 - y1 + 1, x2 - x1 + 1
        patch = g.integers(0, 256, (ph, pw, 3), dtype=np.uint8)
        yy, xx = np.mgrid[0:ph, 0:pw]
        mask = ((((xx + 0.5) / pw - 0.5) ** 2 + ((yy + 0.5) / ph - 0.5) ** 2) <= 0.25).astype(np.uint8)
        velo.tofile(os.path.join(odir, '%d.bin' % k))
        Image.fromarray(patch).save(os.path.join(odir, '%d.png' % k))
        np.save(os.path.join(odir, '%d_mask.npy' % k), mask)
        infos.append({'velo': '%d.bin' % k, 'image': '%d.png' % k, 'mask': '%d_mask.npy' % k,
                      'maskbbox': np.array([x1, y1, x2, y2], np.int64), 'bbox2d': torch.from_numpy(b2),
                      'bbox3d': torch.from_numpy(box), 'id': ids[k % n_calib]})
    with open(os.path.join(t, 'gtdatabase', 'gtinfo.pkl'), 'wb') as f:
        pickle.dump({cls: infos}, f)
    return infos


def _write_calib(path):
    with open(path, 'w') as f:
        p2 = ' '.join('%.6e' % v for v in KITTI_CALIB['P2'][:3].reshape(-1))
        r0 = ' '.join('%.6e' % v for v in KITTI_CALIB['R0_rect'][:3, :3].reshape(-1))
        tr = ' '.join('%.6e' % v for v in KITTI_CALIB['Tr_velo_to_cam'][:3].reshape(-1))
        f.write('P0: %s\nP1: %s\nP2: %s\nP3: %s\nR0_rect: %s\nTr_velo_to_cam: %s\nTr_imu_to_velo: %s\n' % (p2, p2, p2, p2, r0, tr, tr))


def _box_frame(box, xyz):
    """(u, v, dz) of points in the frame of an xyzlwhr box (the inverse of Calc.bbox3d2bev's rotation)."""
    c, s = np.cos(box[6]), np.sin(box[6])
    dx, dy = xyz[:, 0] - box[0], xyz[:, 1] - box[1]
    return dx * c - dy * s, dx * s + dy * c, xyz[:, 2] - box[2]


_KINS_DIMS = {'Car': ((3.4, 4.4), (1.5, 1.8), (1.4, 1.7)), 'Pedestrian': ((0.6, 1.0), (0.5, 0.8), (1.6, 1.9)),
              'Cyclist': ((1.5, 1.9), (0.5, 0.8), (1.6, 1.8))}
_KINS_IDS = {'Car': 4, 'Pedestrian': 2, 'Cyclist': 1}


def _kins_polygons(g, kind, ax, ay, aw, ah):
    """Instance polygons inside the box (ax, ay, aw, ah), flat [x0 y0 x1 y1 ...] lists with three decimals: 0 = one convex
    outline, 1 = one concave star, 2 = two overlapping parts, 3 = two parts with a gap."""
    def ring(cx, cy, rx, ry, n, radii):
        ang = np.linspace(0, 2 * np.pi, n, endpoint=False) + g.uniform(0, 0.3)
        xs = ax + (cx + rx * radii * np.cos(ang)) * aw
        ys = ay + (cy + ry * radii * np.sin(ang)) * ah
        return [round(round(float(v), 2) + 0.003, 3) for xy in zip(xs, ys) for v in xy]      # never on a pixel centre
    if kind == 0:
        return [ring(0.5, 0.5, 0.5, 0.5, 14, g.uniform(0.85, 1.0, 14))]
    if kind == 1:
        return [ring(0.5, 0.5, 0.5, 0.5, 12, np.where(np.arange(12) % 2 == 0, 1.0, g.uniform(0.35, 0.55, 12)))]
    if kind == 2:
        return [ring(0.32, 0.5, 0.3, 0.48, 10, g.uniform(0.9, 1.0, 10)), ring(0.68, 0.5, 0.3, 0.45, 9, g.uniform(0.9, 1.0, 9))]
    return [ring(0.22, 0.5, 0.2, 0.48, 8, g.uniform(0.9, 1.0, 8)), ring(0.78, 0.45, 0.2, 0.4, 11, g.uniform(0.6, 1.0, 11))]


def write_kins_tree(root: str, frame_ids, seg_path=None, points: int = 6000, objects=(5, 9), seed: int = 0,
                    imsize_wh=(1242, 375), rng=VELORANGE, no_annotation=(1,), out_of_range=(2,)):
    """A KITTI tree (training/{velodyne_croped, label_2, calib, image_2}, ImageSets/train.txt) whose labels -- Car, Pedestrian
    and Cyclist rows -- carry the projected 2-D boxes of their 3-D boxes (clipped to the image), plus a matching KINS-format
    annotation file ``seg_path`` (default <root>/seglabel/update_train_2020.json): per label an instance with ``a_bbox`` = the
    label's 2-D box jittered so that the IoUs lie on both sides of 0.65, and ``i_segm`` polygons of four kinds (convex,
    concave, two overlapping parts, two separate parts).  Built in on purpose, per ordinary frame: object 0 is a car at the
    right bottom corner of the image whose ROI touches the border, object 1 has no point inside its box, object 2 is
    labelled twice (two labels match one instance); some labels have no instance, some instances no label or another
    category.  The frames at positions ``no_annotation`` of ``frame_ids`` have no instance at all, those at ``out_of_range``
    only labels beyond the crop range.  The clouds hold background points plus points around every box, about half of them
    inside, in shuffled order.  The annotation file lists the frames in reversed order.  Returns the frame names."""
    import json
    import os
    from PIL import Image
    t = os.path.join(root, 'training')
    for d in ('velodyne_croped', 'label_2', 'calib', 'image_2'):
        os.makedirs(os.path.join(t, d), exist_ok=True)
    os.makedirs(os.path.join(root, 'ImageSets'), exist_ok=True)
    seg_path = os.path.join(root, 'seglabel', 'update_train_2020.json') if seg_path is None else seg_path
    os.makedirs(os.path.dirname(os.path.abspath(seg_path)), exist_ok=True)
    v2c = KITTI_CALIB['Tr_velo_to_cam']
    proj = KITTI_CALIB['P2'] @ KITTI_CALIB['R0_rect'] @ v2c
    W, H = imsize_wh
    lo, hi = np.asarray(rng[:3], np.float64), np.asarray(rng[3:], np.float64)
    names, images, anns = [], [], []
    for pos, fid in enumerate(frame_ids):
        name = '%06d' % fid
        names.append(name)
        g = np.random.default_rng(8000 + 1000 * seed + fid)
        Image.fromarray(g.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(os.path.join(t, 'image_2', name + '.png'))
        _write_calib(os.path.join(t, 'calib', name + '.txt'))
        far = pos in out_of_range
        n_obj = int(g.integers(objects[0], objects[1]))
        rows, boxes, frame_anns = [], [], []
        for k in range(n_obj):
            cls = 'Car' if k < 3 else str(g.choice(['Car', 'Pedestrian', 'Cyclist'], p=[0.5, 0.25, 0.25]))
            dl, dw, dh = _KINS_DIMS[cls]
            l, w, h = g.uniform(*dl), g.uniform(*dw), g.uniform(*dh)
            x = g.uniform(71.5, 78.0) if far else g.uniform(9, 55)
            y = g.uniform(-0.5 * x, 0.5 * x) * (0.3 if far else 1.0)
            z, yaw = g.uniform(-1.8, -1.2), g.choice([0.0, np.pi / 2]) + g.normal(0, 0.08)
            if k == 0 and not far:
                x, y, z, yaw = g.uniform(7.2, 7.6), g.uniform(-5.6, -5.3), -1.75, g.normal(0, 0.05)
            box = np.array([x, y, z, l, w, h, yaw])
            boxes.append(box)
            c, s = np.cos(yaw), np.sin(yaw)
            cx = np.array([0.5, -0.5, -0.5, 0.5, 0.5, -0.5, -0.5, 0.5]) * l
            cy = np.array([0.5, 0.5, -0.5, -0.5, 0.5, 0.5, -0.5, -0.5]) * w
            cz = np.array([0, 0, 0, 0, 1, 1, 1, 1.0]) * h
            im = proj @ np.stack([cx * c + cy * s + x, -cx * s + cy * c + y, cz + z, np.ones(8)], 0)
            uu, vv = im[0] / im[2], im[1] / im[2]
            b2 = np.array([np.clip(uu.min(), 0, W - 1), np.clip(vv.min(), 0, H - 1), np.clip(uu.max(), 0, W - 1),
                           np.clip(vv.max(), 0, H - 1)])
            cam = v2c @ np.array([x, y, z, 1.0])
            occ = int(g.integers(0, 3))
            rows.append('%s 0.00 %d 0.00 %.2f %.2f %.2f %.2f %.4f %.4f %.4f %.4f %.4f %.4f %.4f'
                        % ((cls, occ) + tuple(b2) + (h, w, l, cam[0], cam[1], cam[2], yaw + 0.5 * np.pi)))
            if k == 2:            # the same object labelled a second time, a little off
                cam2 = v2c @ np.array([x + 0.05, y, z, 1.0])
                rows.append('%s 0.00 %d 0.00 %.2f %.2f %.2f %.2f %.4f %.4f %.4f %.4f %.4f %.4f %.4f'
                            % ((cls, occ) + tuple(b2 + np.array([1.0, 0.5, 1.5, 0.0])) + (h, w, l, cam2[0], cam2[1], cam2[2], yaw + 0.5 * np.pi)))
            bw, bh = b2[2] - b2[0], b2[3] - b2[1]
            if bw < 4 or bh < 4 or (k > 2 and g.random() < 0.15):
                continue                                              # a label without an instance
            if k == 0 and not far:
                a = [b2[0], b2[1], bw + 8.0, bh + 8.0]                   # reaches over the image border
            else:
                a = [b2[0] + g.uniform(-0.2, 0.2) * bw, b2[1] + g.uniform(-0.12, 0.12) * bh, bw * g.uniform(0.85, 1.15),
                     bh * g.uniform(0.85, 1.15)]
            a = [round(float(v), 2) for v in a]
            frame_anns.append({'category_id': _KINS_IDS[cls], 'a_bbox': a, 'i_bbox': a,
                               'i_segm': _kins_polygons(g, k % 4, *a)})
        for cat in (4, 3):        # instances without a label: one of a target class, one of another category
            a = [round(float(v), 2) for v in (g.uniform(0, W - 80), g.uniform(0, H - 60), g.uniform(20, 80), g.uniform(20, 60))]
            frame_anns.append({'category_id': cat, 'a_bbox': a, 'i_bbox': a, 'i_segm': _kins_polygons(g, 0, *a)})
        with open(os.path.join(t, 'label_2', name + '.txt'), 'w') as f:
            f.write('\n'.join(rows) + '\nDontCare -1 -1 -10 500.00 100.00 520.00 120.00 -1 -1 -1 -1000 -1000 -1000 -10\n')
        # the cloud: background plus points around every box; none in or near box 1
        pts = [g.uniform(lo, hi, (points, 3))]
        for k, b in enumerate(boxes):
            if k == 1:
                continue
            m = int(g.integers(30, 200))
            u, v, dz = g.uniform(-0.7, 0.7, m) * b[3], g.uniform(-0.7, 0.7, m) * b[4], g.uniform(-0.3, b[5] + 0.3, m)
            c, s = np.cos(b[6]), np.sin(b[6])
            pts.append(np.stack([u * c + v * s + b[0], -u * s + v * c + b[1], dz + b[2]], 1))
        xyz = np.concatenate(pts, 0)
        if len(boxes) > 1:
            u, v, dz = _box_frame(boxes[1], xyz)
            xyz = xyz[~((np.abs(u) < boxes[1][3]) & (np.abs(v) < boxes[1][4]) & (dz > -1) & (dz < boxes[1][5] + 1))]
        xyz = xyz[g.permutation(xyz.shape[0])]
        pc = np.concatenate([xyz, g.random((xyz.shape[0], 1))], 1).astype(np.float32)
        _crop(pc, rng).tofile(os.path.join(t, 'velodyne_croped', name + '.bin'))
        images.append({'id': 1000 + fid, 'file_name': name + '.png', 'width': W, 'height': H})
        if pos not in no_annotation:
            anns.append([dict(a, image_id=1000 + fid) for a in frame_anns])
    flat = [a for fa in reversed(anns) for a in fa]
    for k, a in enumerate(flat):
        a['id'] = k
    with open(seg_path, 'w') as f:
        json.dump({'images': images, 'annotations': flat, 'categories': [{'id': v, 'name': k} for k, v in _KINS_IDS.items()]}, f)
    with open(os.path.join(root, 'ImageSets', 'train.txt'), 'w') as f:
        f.write('\n'.join(names) + '\n')
    return names
