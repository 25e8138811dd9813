"""Host restatement of the GT-paste database builder (reference create_gtdatabase.py; csrc/gtdb.hip, modules/augment/BuildGT.py)
in numpy: parsing, label preparation, matching, rasterising and cutting, with the kernels' arithmetic -- f32 for the IoU, f64
in the kernels' operand order for the crossing test and the box faces.  It reads the tree itself and shares no code with the
package.  ``build`` also returns every decision value's distance to its threshold (``margins``)."""
import json
import os

import numpy as np

CLASSES = ('Car', 'Pedestrian', 'Cyclist')
CLS_TO_ID = {'Car': 4, 'Pedestrian': 2, 'Cyclist': 1}
IOU_THR = np.float32(0.65)
VELORANGE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]
IMSIZE = (370, 1224)


def read_calib(path):
    out = {}
    lines = open(path).read().splitlines()
    for row, shape in ((5, (3, 4)), (2, (3, 4)), (4, (3, 3))):
        tok = lines[row].split(' ')
        m = np.zeros((4, 4))
        m[:shape[0], :shape[1]] = np.array(tok[1:]).astype('float32').reshape(shape)
        m[3, 3] = 1
        out[tok[0][:-1]] = m
    return out


def read_image_bgr(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])


def cam2lidar(rows14, calib):
    """(occluded, bbox2d (n,4), bbox3d (n,7) xyzlwhr) in f32: Calc.bboxCam2Lidar with c2v = f32(inv(Tr)), the product left to right."""
    l = np.asarray(rows14, np.float64).astype(np.float32).reshape(-1, 14)
    m = np.linalg.inv(calib['Tr_velo_to_cam']).astype(np.float32)
    x, y, z = l[:, 10], l[:, 11], l[:, 12]
    xyz = [((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3] for k in range(3)]
    yaw = l[:, 13] - np.float32(0.5 * np.pi)
    return l[:, 1].copy(), l[:, 3:7].copy(), np.stack(xyz + [l[:, 9], l[:, 8], l[:, 7], yaw], 1).astype(np.float32)


def bev(box3d):
    """Calc.bbox3d2bev in f32: unit-square corners scaled by (l, w), times [[c, -s], [s, c]] from the right, plus (x, y)."""
    b = np.asarray(box3d, np.float32).reshape(-1, 7)
    c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
    unit = np.array([[0.5, 0.5], [-0.5, 0.5], [-0.5, -0.5], [0.5, -0.5]], np.float32)
    a, d = unit[None, :, 0] * b[:, None, 3], unit[None, :, 1] * b[:, None, 4]
    return np.stack([a * c[:, None] + d * s[:, None] + b[:, None, 0], a * -s[:, None] + d * c[:, None] + b[:, None, 1]], 2)


def corners(box3d):
    """Calc.bbox3d2corner: the top face (z + h), then the bottom face (z)."""
    b = np.asarray(box3d, np.float32).reshape(-1, 7)
    q = bev(b)
    z, h = np.broadcast_to(b[:, None, 2:3], (b.shape[0], 4, 1)), np.broadcast_to(b[:, None, 5:6], (b.shape[0], 4, 1))
    return np.concatenate([np.concatenate([q, z + h], 2), np.concatenate([q, z], 2)], 1)


def box_iou(a, b):
    """torchvision.ops.box_iou in f32: (n, 4) x (m, 4) -> (n, m)."""
    a, b = np.asarray(a, np.float32).reshape(-1, 4), np.asarray(b, np.float32).reshape(-1, 4)
    area1, area2 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt, rb = np.maximum(a[:, None, :2], b[None, :, :2]), np.minimum(a[:, None, 2:], b[None, :, 2:])
    wh = np.maximum(rb - lt, np.float32(0))
    inter = wh[..., 0] * wh[..., 1]
    with np.errstate(divide='ignore', invalid='ignore'):
        return inter / (area1[:, None] + area2[None, :] - inter)


def raster(polys, roi):
    """(mask u8 (h, w), the smallest |px - x crossing|) of the ROI x1 y1 x2 y2 (inclusive): a pixel is set when its centre is
    inside any polygon (flat coordinate lists) by the even-odd rule."""
    x1, y1, x2, y2 = (int(v) for v in roi)
    px, py = np.arange(x1, x2 + 1, dtype=np.float64) + 0.5, np.arange(y1, y2 + 1, dtype=np.float64) + 0.5
    inside = np.zeros((py.size, px.size), bool)
    margin = np.inf
    for flat in polys:
        v = np.asarray(flat, np.float64).reshape(-1)
        v = v[:2 * (v.size // 2)].reshape(-1, 2)
        if v.shape[0] < 3:
            continue
        par = np.zeros_like(inside)
        for (x0, y0), (xe, ye) in zip(v, np.roll(v, -1, axis=0)):
            rows = (y0 > py) != (ye > py)
            if not rows.any():
                continue
            xi = (xe - x0) * (py[rows] - y0) / (ye - y0) + x0
            par[rows] ^= px[None, :] < xi[:, None]
            margin = min(margin, float(np.abs(px[None, :] - xi[:, None]).min()))
        inside |= par
    return inside.astype(np.uint8), margin


def crop(velo, box3d):
    """(the rows of velo (n, 4) f32 inside the xyzlwhr f32 box, in order; the smallest distance of a coordinate to a face)."""
    b = np.asarray(box3d, np.float32)
    c, s = np.float64(np.cos(b[6])), np.float64(np.sin(b[6]))           # the f32 cosine and sine, widened
    p = velo[:, :3].astype(np.float64)
    dx, dy, dz = p[:, 0] - np.float64(b[0]), p[:, 1] - np.float64(b[1]), p[:, 2] - np.float64(b[2])
    u, v = dx * c - dy * s, dx * s + dy * c
    hl, hw, h = np.float64(b[3]) / 2.0, np.float64(b[4]) / 2.0, np.float64(b[5])
    keep = (np.abs(u) <= hl) & (np.abs(v) <= hw) & (dz >= 0.0) & (dz <= h)
    m = np.inf
    if p.shape[0]:
        m = float(min(np.abs(np.abs(u) - hl).min(), np.abs(np.abs(v) - hw).min(), np.abs(dz).min(), np.abs(dz - h).min()))
    return velo[keep], m


def read_labels(path, classes):
    names, rows = [], []
    for line in open(path):
        tok = line.split(' ')
        if tok and tok[0] in classes:
            names.append(tok[0])
            rows.append([float(t) for t in tok[1:15]])
    return names, np.asarray(rows, np.float64).reshape(-1, 14)


def frame_order(seg, train):
    names = {i['id']: i['file_name'] for i in seg['images']}
    seen = []
    for a in seg['annotations']:
        if a['image_id'] not in seen:
            seen.append(a['image_id'])
    return [(i, names[i][:6]) for i in seen if names[i][:6] in train]


def build(root, seg_path, part=None, classes=CLASSES, velorange=VELORANGE, imsize=IMSIZE):
    """The builder on the frames ``part`` (a slice of the reference's frame order; all of them by default) as ONE batch.
    Returns labels (per label, sorted by class, frame, row: cls, frame, best, iou, flag, roi -- ``best`` counts the batch's
    annotations sorted by frame, class), objects ({cls: [gtinfo entry + arrays]} in the reference's order) and margins."""
    seg = json.load(open(seg_path))
    train = set(open(os.path.join(root, 'ImageSets/train.txt')).read().splitlines())
    order = frame_order(seg, train)
    order = order if part is None else order[part]
    t = os.path.join(root, 'training')
    lo, hi = np.asarray(velorange[:3], np.float32), np.asarray(velorange[3:], np.float32)
    frames, ann_base, n_ann = [], {}, 0
    for f, (iid, name) in enumerate(order):
        img = read_image_bgr(os.path.join(t, 'image_2', name + '.png'))[:imsize[0], :imsize[1]]
        velo = np.fromfile(os.path.join(t, 'velodyne_croped', name + '.bin'), dtype='float32').reshape(-1, 4)
        calib = read_calib(os.path.join(t, 'calib', name + '.txt'))
        names, rows = read_labels(os.path.join(t, 'label_2', name + '.txt'), classes)
        occ, b2, b3 = cam2lidar(rows, calib)
        ok = np.all(b3[:, :3] < hi[None], 1) & np.all(b3[:, :3] >= lo[None], 1)
        anns = {c: [a for a in seg['annotations'] if a['image_id'] == iid and a['category_id'] == CLS_TO_ID[c]] for c in classes}
        for c in classes:
            ann_base[(f, c)] = n_ann
            n_ann += len(anns[c])
        frames.append(dict(name=name, img=img, velo=velo, names=np.asarray(names), occ=occ, b2=b2, b3=b3, ok=ok, anns=anns))
    labels = {k: [] for k in ('cls', 'frame', 'best', 'iou', 'flag', 'roi', 'box2d', 'box3d')}
    objects = {c: [] for c in classes}
    margins = {'iou': [], 'raster': [], 'crop': []}
    for c in classes:
        for f, fr in enumerate(frames):
            sel = np.nonzero((fr['names'] == c) & fr['ok'])[0] if fr['names'].size else np.zeros((0,), int)
            boxes = np.asarray([[a['a_bbox'][0], a['a_bbox'][1], a['a_bbox'][0] + a['a_bbox'][2], a['a_bbox'][1] + a['a_bbox'][3]]
                                for a in fr['anns'][c]], np.float64).astype(np.float32).reshape(-1, 4)
            ious = box_iou(fr['b2'][sel], boxes)
            H, W = fr['img'].shape[:2]
            for k, row in enumerate(sel):
                best, iou, flag, roi = -1, np.float32(0), 0, [0, 0, -1, -1]
                if boxes.shape[0]:
                    j = int(np.argmax(ious[k]))                       # the first index that reaches the maximum
                    iou = ious[k, j]
                    best = ann_base[(f, c)] + j
                    x1, y1, x2, y2 = (int(v) for v in boxes[j])       # truncation, as Tensor.int()
                    roi = [max(x1, 0), max(y1, 0), min(x2, W - 1), min(y2, H - 1)]
                    flag = int(iou >= IOU_THR) | (2 if roi[2] >= roi[0] and roi[3] >= roi[1] else 0)
                    margins['iou'].append(abs(float(iou) - 0.65))
                for key, val in (('cls', c), ('frame', f), ('best', best), ('iou', iou), ('flag', flag), ('roi', roi),
                                 ('box2d', fr['b2'][row]), ('box3d', fr['b3'][row])):
                    labels[key].append(val)
                if flag != 3:
                    continue
                mask, m = raster(fr['anns'][c][j]['i_segm'], roi)
                margins['raster'].append(m)
                patch = fr['img'][roi[1]:roi[3] + 1, roi[0]:roi[2] + 1] * mask[..., None]
                pts, m = crop(fr['velo'], fr['b3'][row])
                margins['crop'].append(m)
                n = len(objects[c])
                objects[c].append({'velo': 'velo_%06d.bin' % n, 'image': 'img_%06d.png' % n, 'mask': 'mask_%06d.npy' % n,
                                   'occlude': fr['occ'][row], 'maskbbox': np.asarray(roi, np.int32), 'bbox2d': fr['b2'][row],
                                   'bbox3d': fr['b3'][row], 'id': fr['name'], 'points': pts, 'patch': patch, 'mask_px': mask,
                                   'ann': best})
    out = {k: np.asarray(v) for k, v in labels.items()}
    out['roi'] = out['roi'].reshape(-1, 4).astype(np.int32)
    return {'labels': out, 'objects': objects, 'margins': {k: np.asarray(v, np.float64) for k, v in margins.items()}, 'order': order}
