"""Builds the GT-paste object database from a KITTI tree and a KINS annotation file (reference create_gtdatabase.py) on the
GPU (csrc/gtdb.hip): label boxes against instance annotations, instance polygons into masks and patches, the points inside
every oriented 3-D box.  The host parses (``json``, label / calib files, PIL images, ``.bin`` clouds) and prepares the label
rows as modules/data/Load.py does; ``buildFrames`` runs a batch of frames in four kernel calls (six launches) with one host read.

    ann = readAnnotations('update_train_2020.json')
    order = frameOrder(ann, train_set)                     # the reference's frame order
    frames = [loadFrame(root, name) for _, name in order[:8]]
    built = buildFrames(frames, [ann.by_image[i] for i, _ in order[:8]], device='cuda')
    built['Car']['infos'], built['Car']['tables']

Differences from the reference are listed in DESIGN.md 3.19 (pixel-centre even-odd fill, the cuboid itself as the crop volume,
ROIs clipped to the image, masks 0/1)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

import modules.config as cfg
from modules import _hip
from modules.data import Load

CLASSES = ('Car', 'Pedestrian', 'Cyclist')
CLS_TO_ID = {'Car': 4, 'Pedestrian': 2, 'Cyclist': 1}              # KINS category ids (create_gtdatabase.py:80)
MAX_LABELS = 65535                                                  # one grid row per label


def readAnnotations(path):
    """The KINS file: ``names`` {image id: file name} and ``by_image`` {image id: [annotation, ...]} in the file's annotation
    order (make_json_dict of the reference)."""
    with open(path, 'r') as f:
        seg = json.load(f)
    by_image = {}
    for a in seg['annotations']:
        by_image.setdefault(a['image_id'], []).append(a)
    return SimpleNamespace(names={i['id']: i['file_name'] for i in seg['images']}, by_image=by_image)


def frameOrder(ann, train_set):
    """[(image id, frame name)] of the frames the reference processes, in its order: every image that has an annotation, by
    first appearance, whose frame is in ``train_set``."""
    return [(i, ann.names[i][:6]) for i in ann.by_image if ann.names[i][:6] in train_set]


def cam2lidar_f32(rows14, calib):
    """Label rows (n, 14) -> (occluded f32 (n,), bbox2d f32 (n, 4), bbox3d f32 (n, 7) xyzlwhr in the LiDAR frame): Calc.bboxCam2Lidar
    with c2v = float32(inv(Tr_velo_to_cam)) as create_gtdatabase.py:142-151 sets it up.  The 4x4 product is written out in
    float32, left to right, so that its bits do not depend on a BLAS."""
    l = np.asarray(rows14, np.float64).astype(np.float32).reshape(-1, 14)
    m = np.linalg.inv(np.asarray(calib['Tr_velo_to_cam'], np.float64)).astype(np.float32)
    x, y, z = l[:, 10], l[:, 11], l[:, 12]
    xyz = [((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3] for k in range(3)]
    yaw = l[:, 13] - np.float32(0.5 * np.pi)
    box3d = np.stack(xyz + [l[:, 9], l[:, 8], l[:, 7], yaw], axis=1).astype(np.float32)
    return l[:, 1].copy(), l[:, 3:7].copy(), box3d


def loadFrame(root, name, classes=CLASSES, imsize=None, velorange=None):
    """One frame from the KITTI tree: the cropped cloud, the image cut to ``imsize`` (BGR), and per class the label rows in range."""
    imsize = cfg.imsize if imsize is None else imsize
    rng = np.asarray(cfg.velorange if velorange is None else velorange, np.float32)
    veloroot, _, labelroot, calibroot, imroot = Load._roots(root)
    velo = np.fromfile(os.path.join(veloroot, name + '.bin'), dtype='float32').reshape((-1, 4))
    img = Load._read_image(os.path.join(imroot, name + '.png'))[:imsize[0], :imsize[1]]
    calib = Load.readCalib(os.path.join(calibroot, name + '.txt'))
    names, rows = Load._read_class_labels(os.path.join(labelroot, name + '.txt'), classes)
    occ, b2, b3 = cam2lidar_f32(rows, calib)
    ok = np.all(b3[:, :3] < rng[None, 3:], axis=1) & np.all(b3[:, :3] >= rng[None, :3], axis=1)
    labels = {}
    for c in classes:
        sel = np.asarray([n == c for n in names], bool).reshape(-1) & ok
        labels[c] = {'occlude': occ[sel], 'bbox2d': b2[sel], 'bbox3d': b3[sel]}
    return {'id': name, 'velo': velo, 'image': img, 'calib': calib, 'labels': labels}


def annotationTables(anns, classes):
    """Per class of one frame: the mask boxes f32 (n, 4) x1 y1 x2 y2 and per annotation its polygons' edges f64 (e, 4) with the
    polygon index of every edge."""
    out = {c: {'box': [], 'edges': [], 'poly': []} for c in classes}
    ids = {CLS_TO_ID[c]: c for c in classes}
    for a in anns:
        c = ids.get(a['category_id'])
        if c is None:
            continue
        x, y, w, h = (float(v) for v in a['a_bbox'][:4])
        out[c]['box'].append([x, y, x + w, y + h])
        edges, poly = [], []
        for k, flat in enumerate(a['i_segm']):
            v = np.asarray(flat, np.float64).reshape(-1)
            v = v[:2 * (v.size // 2)].reshape(-1, 2)
            if v.shape[0] < 3:
                continue
            edges.append(np.concatenate([v, np.roll(v, -1, axis=0)], axis=1))
            poly.append(np.full((v.shape[0],), k, np.int32))
        out[c]['edges'].append(np.concatenate(edges, 0) if edges else np.zeros((0, 4), np.float64))
        out[c]['poly'].append(np.concatenate(poly, 0) if poly else np.zeros((0,), np.int32))
    return out


def pack(frames, annotations, classes=CLASSES, device='cpu', imsize=None):
    """The flat tables of a batch (include/mvx_hip.h, "Builder of the GT-paste object database") on ``device``; labels sorted
    by (class, frame, row), annotations by (frame, class).  Host work: concatenation only."""
    imsize = cfg.imsize if imsize is None else imsize
    F, C = len(frames), len(classes)
    assert F >= 1 and len(annotations) == F
    H, W = int(imsize[0]), int(imsize[1])
    at = [annotationTables(a, classes) for a in annotations]
    ann_box, edges, edge_poly, ann_off, edge_off = [], [], [], [0], [0]
    for f in range(F):
        for c in classes:
            ann_box += at[f][c]['box']
            for e, p in zip(at[f][c]['edges'], at[f][c]['poly']):
                edges.append(e)
                edge_poly.append(p)
                edge_off.append(edge_off[-1] + e.shape[0])
            ann_off.append(len(ann_box))
    lab = {k: [] for k in ('box2d', 'box3d', 'occlude', 'frame', 'group')}
    cls_off = [0]
    for ci, c in enumerate(classes):
        for f, fr in enumerate(frames):
            l = fr['labels'][c]
            n = l['bbox3d'].shape[0]
            lab['box2d'].append(l['bbox2d'])
            lab['box3d'].append(l['bbox3d'])
            lab['occlude'].append(l['occlude'])
            lab['frame'].append(np.full((n,), f, np.int32))
            lab['group'].append(np.full((n,), f * C + ci, np.int32))
        cls_off.append(sum(a.shape[0] for a in lab['frame']))
    cat = lambda xs, shape, dt: np.concatenate(xs, 0).astype(dt).reshape(shape) if xs else np.zeros(tuple(max(v, 0) for v in shape), dt)
    box3d = cat(lab['box3d'], (-1, 7), np.float32)
    images = np.zeros((F, H, W, 3), np.uint8)
    im_hw = np.zeros((F, 2), np.int32)
    for f, fr in enumerate(frames):
        im = np.asarray(fr['image'])[:H, :W, :3]
        images[f, :im.shape[0], :im.shape[1]] = im
        im_hw[f] = im.shape[:2]
    velos = [np.ascontiguousarray(fr['velo'], dtype=np.float32).reshape(-1, 4) for fr in frames]
    pts_off = np.concatenate([[0], np.cumsum([v.shape[0] for v in velos])]).astype(np.int64)
    dev = torch.device(device)
    pad = lambda a: np.concatenate([a, np.zeros((1,) + a.shape[1:], a.dtype)], 0) if a.shape[0] == 0 else a
    to = lambda a: torch.from_numpy(np.ascontiguousarray(pad(a))).to(dev)
    return SimpleNamespace(
        n_labels=box3d.shape[0], n_frames=F, n_ann=len(ann_box), classes=tuple(classes), cls_off=cls_off,
        max_frame_points=max(v.shape[0] for v in velos), ids=[fr['id'] for fr in frames],
        lab_box2d=to(cat(lab['box2d'], (-1, 4), np.float32)), lab_box3d=to(box3d),
        lab_cs=to(np.stack([np.cos(box3d[:, 6]), np.sin(box3d[:, 6])], axis=1).astype(np.float32)),
        lab_occlude=cat(lab['occlude'], (-1,), np.float32), lab_frame=to(cat(lab['frame'], (-1,), np.int32)),
        lab_group=to(cat(lab['group'], (-1,), np.int32)), ann_box=to(np.asarray(ann_box, np.float64).astype(np.float32).reshape(-1, 4)),
        ann_off=torch.from_numpy(np.asarray(ann_off, np.int32)).to(dev), edges=to(cat(edges, (-1, 4), np.float64)),
        edge_poly=to(cat(edge_poly, (-1,), np.int32)), edge_off=torch.from_numpy(np.asarray(edge_off, np.int32)).to(dev),
        images=to(images), im_hw=to(im_hw), points=to(np.concatenate(velos, 0)), pts_off=torch.from_numpy(pts_off).to(dev))


def run(t):
    """The four kernel calls on the tables of ``pack`` and the one host read between them.  Returns the per-label results on the
    host (best, iou, flag, roi, px_off, pt_off) and the packed device outputs (mask, patch, points)."""
    best, iou, flag, roi, px_off = _hip.gtdb_match(t)
    pt_off, ws = _hip.gtdb_crop_count(t, flag)
    n = t.n_labels
    host = torch.cat([best.long(), flag.long(), roi.reshape(-1).long(), px_off, pt_off]).cpu().numpy()       # the one host read
    h = SimpleNamespace(best=host[:n].astype(np.int32), flag=host[n:2 * n].astype(np.int32),
                        roi=host[2 * n:6 * n].astype(np.int32).reshape(n, 4), px_off=host[6 * n:7 * n + 1].copy(),
                        pt_off=host[7 * n + 1:8 * n + 2].copy())
    obj = h.flag == 3
    rows = int((h.roi[obj, 3] - h.roi[obj, 1] + 1).max()) if obj.any() else 1
    dev = t.points.device
    if h.px_off[-1] > 0:
        mask, patch = _hip.gtdb_raster(t, best, flag, roi, px_off, int(h.px_off[-1]), rows)
    else:                                                           # no object in the batch: nothing to launch
        mask, patch = torch.zeros((1,), dtype=torch.uint8, device=dev), torch.zeros((1, 3), dtype=torch.uint8, device=dev)
    if h.pt_off[-1] > 0:
        points = _hip.gtdb_crop_write(t, flag, pt_off, ws, int(h.pt_off[-1]))
    else:
        points = torch.zeros((1, 4), dtype=torch.float32, device=dev)
    h.iou = iou
    return h, SimpleNamespace(mask=mask, patch=patch, points=points)


def buildFrames(frames, annotations, classes=CLASSES, device=None, counters=None, imsize=None):
    """``frames``: the dicts of ``loadFrame``; ``annotations``: per frame its KINS annotation dicts, in file order.  Returns
    ``{cls: {'infos': [...], 'tables': {...}}}``: ``infos`` are the reference's gtinfo entries (occlude, maskbbox, bbox2d,
    bbox3d as tensors, id; with ``counters`` = {cls: next number} also the file names velo / image / mask, and the counters
    advance), in the reference's per-class order; ``tables`` holds the class's objects packed on the device in the layout
    csrc/augment.hip reads: box2d f32 (n, 4), box3d f32 (n, 7), maskbbox i32 (n, 4), px_off i64 (n + 1,), mask u8 (px,),
    patch u8 (px, 3) BGR, pt_off i64 (n + 1,), points f32 (rows, 4) = x y z r, plus 'label' / 'ann' (the label row and the
    annotation of every object inside the batch) and 'ids'."""
    from modules import Extension as X
    dev = torch.device(device) if device is not None else X.device()
    out = {}
    if sum(fr['labels'][c]['bbox3d'].shape[0] for fr in frames for c in classes) == 0:
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)
        for c in classes:
            out[c] = {'infos': [], 'tables': {'n': 0, 'box2d': z(0, 4), 'box3d': z(0, 7), 'maskbbox': z(0, 4, dt=torch.int32),
                                              'px_off': z(1, dt=torch.int64), 'mask': z(0, dt=torch.uint8),
                                              'patch': z(0, 3, dt=torch.uint8), 'pt_off': z(1, dt=torch.int64), 'points': z(0, 4),
                                              'label': np.zeros((0,), np.int64), 'ann': np.zeros((0,), np.int32), 'ids': []}}
        return out
    t = pack(frames, annotations, classes, dev, imsize)
    if t.n_labels > MAX_LABELS:
        raise ValueError('%d labels in one call (at most %d): use smaller batches' % (t.n_labels, MAX_LABELS))
    h, d = run(t)
    frame_of = t.lab_frame.cpu().numpy()
    for ci, c in enumerate(classes):
        l0, l1 = t.cls_off[ci], t.cls_off[ci + 1]
        sel = l0 + np.nonzero(h.flag[l0:l1] == 3)[0]
        px0, px1, pt0, pt1 = (int(v) for v in (h.px_off[l0], h.px_off[l1], h.pt_off[l0], h.pt_off[l1]))
        idx = torch.from_numpy(sel).to(dev)
        box2d, box3d = t.lab_box2d[idx], t.lab_box3d[idx]
        maskbbox = torch.from_numpy(h.roi[sel]).to(dev)
        ids = [t.ids[frame_of[k]] for k in sel]
        tables = {'n': len(sel), 'box2d': box2d, 'box3d': box3d, 'maskbbox': maskbbox,
                  'px_off': torch.from_numpy(np.concatenate([h.px_off[sel] - px0, [px1 - px0]]).astype(np.int64)).to(dev),
                  'mask': d.mask[px0:px1], 'patch': d.patch[px0:px1],
                  'pt_off': torch.from_numpy(np.concatenate([h.pt_off[sel] - pt0, [pt1 - pt0]]).astype(np.int64)).to(dev),
                  'points': d.points[pt0:pt1], 'label': sel, 'ann': h.best[sel], 'ids': ids}
        b2, b3, mb = box2d.cpu(), box3d.cpu(), maskbbox.cpu()
        infos = []
        for k, s in enumerate(sel):
            info = {}
            if counters is not None:
                info.update(velo='velo_%06d.bin' % counters[c], image='img_%06d.png' % counters[c], mask='mask_%06d.npy' % counters[c])
                counters[c] += 1
            info.update(occlude=torch.tensor(t.lab_occlude[s]), maskbbox=mb[k], bbox2d=b2[k], bbox3d=b3[k], id=ids[k])
            infos.append(info)
        out[c] = {'infos': infos, 'tables': tables}
    return out


def objectsOf(built_cls, calibs=None):
    """The objects of one class of a ``buildFrames`` result as host arrays, in order: [{'velo' (n, 4) f32, 'image' (h, w, 3) u8
    BGR, 'mask' (h, w) u8, 'maskbbox', 'bbox2d', 'bbox3d', 'id'[, 'calib']}]."""
    tb = built_cls['tables']
    px, pt = tb['px_off'].cpu().numpy(), tb['pt_off'].cpu().numpy()
    mask, patch, points, mb = (tb[k].cpu().numpy() for k in ('mask', 'patch', 'points', 'maskbbox'))
    b2, b3 = tb['box2d'].cpu(), tb['box3d'].cpu()
    out = []
    for k in range(tb['n']):
        h, w = int(mb[k, 3] - mb[k, 1] + 1), int(mb[k, 2] - mb[k, 0] + 1)
        g = {'velo': points[pt[k]:pt[k + 1]].copy(), 'image': patch[px[k]:px[k + 1]].reshape(h, w, 3).copy(),
             'mask': mask[px[k]:px[k + 1]].reshape(h, w).copy(), 'maskbbox': torch.from_numpy(mb[k].copy()),
             'bbox2d': b2[k], 'bbox3d': b3[k], 'id': tb['ids'][k]}
        if calibs is not None:
            g['calib'] = calibs[g['id']]
        out.append(g)
    return out


def writeObjects(root, cls, built_cls):
    """Writes the objects of one class under ``<root>/training/gtdatabase/<cls>/`` with the names of their infos (reference
    create_gtdatabase.py:231-233: raw f32 points, the patch as PNG, the mask as .npy)."""
    from PIL import Image
    d = os.path.join(root, 'training', 'gtdatabase', cls)
    os.makedirs(d, exist_ok=True)
    for info, g in zip(built_cls['infos'], objectsOf(built_cls)):
        g['velo'].astype(np.float32).tofile(os.path.join(d, info['velo']))
        Image.fromarray(np.ascontiguousarray(g['image'][:, :, ::-1])).save(os.path.join(d, info['image']))      # BGR -> RGB for PIL
        np.save(os.path.join(d, info['mask']), g['mask'])
