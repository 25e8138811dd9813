"""Pictures of a frame set: a bird's-eye view and a camera view of the resident point clouds with ground-truth boxes and
detections drawn over them (csrc/render.hip).  Everything a picture needs is already on the device during a detection
step -- ``FrameBatch.points6`` (x y z r row col), the padded tensors of ``detect.postprocess(read=False)``, the GT boxes --
so a view costs three launches for all frames and no host round trip except the finished image.

  * ``draw_list``: GT boxes and detections -> the padded ``(boxes, n_boxes, colors)`` both views take.  The kernels know
    colours and priorities, not classes: ``pack_colors`` builds the words, the larger word wins a pixel.
  * ``render_bev`` / ``render_camera``: ``(image u8 (F, H, W, 3) RGB, status i32 (F,))`` on the device.
  * ``default_luts``, ``save_png``, ``save_frames``.
"""
import os

import numpy as np
import torch

import modules.config as cfg
from modules import _hip

GT_PRIO, GT_RGB = 1, (0, 255, 0)
DET_PRIO_BASE, DET_LEVELS = 2, 254          # detections: prio 2 + v, v = min(253, floor(score * 253))


def pack_colors(prio, rgb):
    """``prio << 24 | R << 16 | G << 8 | B`` as the u32 words the kernels compare, carried in an int32 tensor (a priority
    above 127 shows as a negative number; the kernels read the bits).  ``prio`` (...,) and ``rgb`` (..., 3) integers 0..255,
    tensors or Python numbers."""
    prio = torch.as_tensor(prio).to(torch.int64)
    rgb = torch.as_tensor(rgb, device=prio.device).to(torch.int64)
    if ((prio < 0) | (prio > 255)).any() or ((rgb < 0) | (rgb > 255)).any():
        raise ValueError('priorities and colour channels are 0..255')
    word = (prio << 24) | (rgb[..., 0] << 16) | (rgb[..., 1] << 8) | rgb[..., 2]
    return torch.where(word >= (1 << 31), word - (1 << 32), word).to(torch.int32)


def detection_colors():
    """u8 (254, 3): red (weakest) to yellow (strongest), G = v * 255 // 253."""
    v = torch.arange(DET_LEVELS, dtype=torch.int64)
    return torch.stack([torch.full_like(v, 255), v * 255 // (DET_LEVELS - 1), torch.zeros_like(v)], 1).to(torch.uint8)


def _padded_detections(dets, F, device):
    """(boxes (F, D, 7) f32, scores (F, D) f32, counts i32 (F,)) on ``device`` from the device dict of
    ``detect.postprocess(read=False)`` (its counts stay where they are) or from per-frame dicts with 'boxes' and 'scores'."""
    if dets is None:
        return (torch.zeros((F, 0, 7), device=device), torch.zeros((F, 0), device=device),
                torch.zeros((F,), dtype=torch.int32, device=device))
    if isinstance(dets, dict):
        assert dets['boxes'].shape[0] == F and dets['meta'].shape == (3, F)
        return dets['boxes'].to(device).float(), dets['scores'].to(device).float(), dets['meta'][0].to(device).to(torch.int32)
    assert len(dets) == F
    counts = [0 if d is None else int(d['boxes'].shape[0]) for d in dets]
    D = max(counts) if counts else 0
    boxes = torch.zeros((F, D, 7), device=device)
    scores = torch.zeros((F, D), device=device)
    for f, (d, n) in enumerate(zip(dets, counts)):
        if n:
            boxes[f, :n] = torch.as_tensor(d['boxes']).to(device).float().reshape(n, 7)
            scores[f, :n] = torch.as_tensor(d['scores']).to(device).float().reshape(n)
    return boxes, scores, torch.tensor(counts, dtype=torch.int32, device=device)


def draw_list(gt_boxes_per_frame, dets=None, device=None, cap=None):
    """The draw list of a frame set: ``(boxes f32 (F, Bcap, 7), n_boxes i32 (F,), colors i32 (F, Bcap))``.

    ``gt_boxes_per_frame``: per frame an (n, 7) LiDAR-frame xyzlwhr tensor or None -- green, priority 1.  ``dets``: the
    device dict of ``detect.postprocess(read=False)``, per-frame dicts with 'boxes' and 'scores' (``detect.unpack``), or None.
    A detection takes priority ``2 + v`` and colour ``detection_colors()[v]`` with ``v = min(253, floor(score * 253))``: the
    stronger detection is drawn over the weaker one, and every detection over the ground truth.
    A frame's slots hold its GT boxes, then its detections; ``n_boxes`` = the two counts added ON THE DEVICE (the detection
    counts of the device dict are never read on the host), and slots past the count are zeroed there, colours included.
    ``Bcap`` = the largest GT count + the detection capacity (``post_max`` for the device dict, the largest count for
    lists), or ``cap``."""
    F = len(gt_boxes_per_frame)
    if device is None:
        device = dets['boxes'].device if isinstance(dets, dict) else next(
            (torch.as_tensor(d['boxes']).device for d in (dets or []) if d is not None), torch.device('cpu'))
    device = torch.device(device)
    det_boxes, det_scores, det_counts = _padded_detections(dets, F, device)
    D = det_boxes.shape[1]
    gts = [None if g is None else torch.as_tensor(g).to(device).float().reshape(-1, 7) for g in gt_boxes_per_frame]
    g_counts = [0 if g is None else g.shape[0] for g in gts]
    Bcap = max(g_counts) + D
    if cap is not None:
        if cap < Bcap:
            raise ValueError('cap %d is below the %d slots the draw list needs' % (cap, Bcap))
        Bcap = int(cap)
    boxes = torch.zeros((F, max(Bcap, 1), 7), device=device)
    colors = torch.zeros((F, max(Bcap, 1)), dtype=torch.int32, device=device)
    v = torch.nan_to_num(torch.floor(det_scores.double() * (DET_LEVELS - 1)), nan=0.0).clamp(0, DET_LEVELS - 1).to(torch.int64)
    det_words = pack_colors(DET_PRIO_BASE + v, detection_colors().to(device)[v])
    gt_word = pack_colors(GT_PRIO, GT_RGB).to(device)
    for f, g in enumerate(gts):
        n = g_counts[f]
        if n:
            boxes[f, :n] = g
            colors[f, :n] = gt_word
        boxes[f, n:n + D] = det_boxes[f]
        colors[f, n:n + D] = det_words[f]
    n_boxes = torch.tensor(g_counts, dtype=torch.int32, device=device) + det_counts.clamp(0, D)
    live = torch.arange(boxes.shape[1], device=device)[None, :] < n_boxes[:, None]
    boxes = torch.where(live[..., None], boxes, torch.zeros_like(boxes)).contiguous()
    colors = torch.where(live, colors, torch.zeros_like(colors)).contiguous()
    return boxes, n_boxes, colors


def _ramp(i):
    """Blue - cyan - green - yellow - red over i = 0..255, four linear pieces of 64 steps, integers only."""
    seg, t = i // 64, (i % 64) * 4
    zero, full = torch.zeros_like(i), torch.full_like(i, 255)
    r = torch.where(seg < 2, zero, torch.where(seg == 2, t, full))
    g = torch.where(seg == 0, t, torch.where(seg == 3, 255 - t, full))
    b = torch.where(seg == 0, full, torch.where(seg == 1, 255 - t, zero))
    return torch.stack([r, g, b], 1).to(torch.uint8)


def default_luts():
    """{'height', 'intensity', 'depth'}: u8 (256, 3) tables on the host.  Height: blue (low) to red (high); intensity: grey
    48 + i * 207 // 255; depth: red (near) to blue (far)."""
    i = torch.arange(256, dtype=torch.int64)
    grey = (48 + i * 207 // 255).to(torch.uint8)
    return {'height': _ramp(i), 'intensity': torch.stack([grey, grey, grey], 1), 'depth': _ramp(255 - i)}


_LUTS = {}


def _lut_on(name, device, luts=None):
    if luts is not None:
        return luts[name].to(device).contiguous()
    key = (name, str(device))
    if key not in _LUTS:
        _LUTS[key] = default_luts()[name].to(device).contiguous()
    return _LUTS[key]


def _points_of(batch_or_points):
    if isinstance(batch_or_points, (tuple, list)):
        return batch_or_points
    return batch_or_points.prepared()


def _pack_rgb(rgb):
    return (int(rgb[0]) << 16) | (int(rgb[1]) << 8) | int(rgb[2])


def bev_shape(res, velorange=None):
    """(H, W) of the bird's-eye view: the x and y extent of the range over ``res`` (704 x 800 at 0.1 m)."""
    vr = cfg.velorange if velorange is None else velorange
    return int(round((vr[3] - vr[0]) / res)), int(round((vr[4] - vr[1]) / res))


def render_bev(batch_or_points, draw=None, *, res=0.1, color_by='height', cmax=8, thickness=1, background=(0, 0, 0), luts=None,
               velorange=None):
    """Bird's-eye view of every frame: ``(image u8 (F, H, W, 3) RGB, status i32 (F,))`` on the device, no host read.
    ``batch_or_points``: a ``pipeline.FrameBatch`` or ``(points6, n_points)``; ``draw``: a ``draw_list`` or None.  The range
    is ``cfg.velorange``: forward (+x) is up, +y is left, one pixel per ``res`` metres; points are coloured by 'height' (z
    over the range's z extent) or 'intensity' and shaded by the number of points in the pixel (saturating at ``cmax``).
    status: ``_hip.RENDER_BAD_BOX`` where a box was dropped (non-finite, or far outside)."""
    vr = cfg.velorange if velorange is None else velorange
    points6, n_points = _points_of(batch_or_points)
    H, W = bev_shape(res, vr)
    boxes, n_boxes, colors = draw if draw is not None else (None, None, None)
    return _hip.render_bev_frames(points6, n_points, boxes, n_boxes, colors, vr[0], vr[1], res, vr[2], vr[5], H, W,
                                  _lut_on(color_by, points6.device, luts), color_by, cmax, _pack_rgb(background), thickness)


def image_from_lidar(calibs):
    """f64 (F, 4, 4): ``P2 @ Tr_velo_to_cam`` of every frame's calibration dict."""
    return torch.stack([torch.as_tensor(np.asarray(c['P2'], dtype=np.float64) @ np.asarray(c['Tr_velo_to_cam'], dtype=np.float64))
                        for c in calibs])


def stack_images(images, imsize):
    """Per-frame (h, w, 3) u8 arrays -> one (F, H, W, 3) array of ``imsize``, cropped or zero-padded at the bottom / right."""
    H, W = int(imsize[0]), int(imsize[1])
    out = np.zeros((len(images), H, W, 3), np.uint8)
    for f, im in enumerate(images):
        im = np.asarray(im)[:H, :W]
        out[f, :im.shape[0], :im.shape[1]] = im
    return out


def render_camera(batch_or_points, draw, calibs, images=None, *, imsize=None, matrices=None, z_near=0.5, depth_max=None,
                  point_radius=1, thickness=1, images_bgr=True, luts=None):
    """Camera view of every frame: ``(image u8 (F, H, W, 3) RGB, status i32 (F,))`` on the device.  Points are drawn at the
    (row, col) the loader projected them to (columns 4 and 5 of ``points6``), nearest point on top, coloured by depth;
    ``images``: per-frame (h, w, 3) u8 arrays or one (F, H, W, 3) array / device tensor, in the loader's BGR order unless
    ``images_bgr=False``; None: black.

    Boxes go through ``matrices`` f64 (F, 4, 4), by default ``P2 @ Tr_velo_to_cam`` -- WITHOUT ``R0_rect``, although the
    points were projected with ``P2 @ R0_rect @ Tr_velo_to_cam``.  The loader takes the label boxes to the LiDAR frame with
    the inverse of ``Tr_velo_to_cam`` alone (Load.createDataset, like the reference), and ``detect.kitti_lines`` takes
    detections back the same way: a box in this project's "LiDAR frame" is therefore placed where the label file put it only
    by that matrix.  The picture shows the consequence -- boxes sit where the labels are in the image, and the points of the
    same object are off by the rectifying rotation (a fraction of a degree on KITTI) -- instead of hiding it."""
    points6, n_points = _points_of(batch_or_points)
    dev = points6.device
    H, W = (int(v) for v in (cfg.imsize if imsize is None else imsize))
    mats = image_from_lidar(calibs) if matrices is None else torch.as_tensor(matrices)
    mats = mats.to(dev, torch.float64).contiguous()
    if images is not None and not isinstance(images, torch.Tensor):
        images = torch.from_numpy(stack_images(images, (H, W)))
    if images is not None:
        images = images.to(dev).contiguous()
    boxes, n_boxes, colors = draw if draw is not None else (None, None, None)
    vr = cfg.velorange
    return _hip.render_camera_frames(points6, n_points, boxes, n_boxes, colors, mats, H, W, _lut_on('depth', dev, luts), z_near,
                                     float(vr[3]) if depth_max is None else depth_max, point_radius, images, images_bgr, thickness)


def points_from_dataset(group, device, cap_points=None):
    """``(points6 f32 (B, cap, 6), n_points i32 (B,))`` on ``device`` from frames of ``Load.createDataset``: x y z r and the
    (row, col) of train.py:31-34 -- the projection ``pipeline.batch_from_dataset`` makes, without the training targets."""
    from modules.data.Preprocessing import _calib_products
    cap = max(d[0].shape[0] for d in group) if cap_points is None else cap_points
    pts6 = torch.zeros((len(group), max(cap, 1), 6), dtype=torch.float32, device=device)
    n = []
    for k, d in enumerate(group):
        P = d[0].shape[0]
        n.append(P)
        if P:
            src = torch.from_numpy(np.ascontiguousarray(d[0], dtype=np.float32)).to(device)
            pts6[k, :P, :4] = src
            m, p2 = _calib_products(d[5], True)
            _hip.lidar2img(src, m, p2, math_f32=True, out=pts6[k, :P], col_offset=4, swap_rc=True)
    return pts6, torch.tensor(n, dtype=torch.int32, device=device)


def save_png(path, rgb):
    """One (H, W, 3) u8 RGB image (tensor or array) as a PNG file."""
    from PIL import Image
    a = rgb.detach().cpu().numpy() if isinstance(rgb, torch.Tensor) else np.asarray(rgb)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError('save_png takes an (H, W, 3) uint8 image')
    Image.fromarray(np.ascontiguousarray(a), 'RGB').save(path)


def save_frames(out_dir, names, bev=None, cam=None):
    """``<name>_bev.png`` / ``<name>_cam.png`` of every frame: one device-to-host copy per view.  Returns the paths."""
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for tag, imgs in (('bev', bev), ('cam', cam)):
        if imgs is None:
            continue
        host = imgs.cpu()
        for name, im in zip(names, host):
            paths.append(os.path.join(out_dir, '%s_%s.png' % (name, tag)))
            save_png(paths[-1], im)
    return paths
