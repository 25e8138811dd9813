"""Pictures of KITTI frames: a bird's-eye view and a camera view of every frame with the ground-truth boxes of ``label_2``
(green) and, optionally, detections (red, weak, to yellow, strong) drawn on the GPU (modules/render.py, csrc/render.hip).

Detections come from KITTI result files (``--results DIR``, as detect_like.py writes them, taken back to the LiDAR frame with
``Calc.bboxCam2Lidar``) or from running the model (``--checkpoint FILE``).  Writes ``<name>_bev.png`` and ``<name>_cam.png``.

    python visualize_like.py <dataroot> --results <dataroot>/results/data --split val --out pictures
    python visualize_like.py <dataroot> --checkpoint checkpoints/epoch10.pkl --frames 8
    python visualize_like.py /tmp/kitti --synthetic 3          # a synthetic tree, ground truth only
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SET = 4          # frames rendered per launch


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('dataroot')
    ap.add_argument('--results', default=None, help='directory of KITTI result files (<name>.txt) to draw as detections')
    ap.add_argument('--checkpoint', default=None, help='state dict written by train_like.py: detections from running the model')
    ap.add_argument('--dir-offset', type=float, default=math.pi / 4,
                    help='a checkpoint of train_like.py --direction (it holds backbone.rpn.dir.weight): the --dir-offset it was trained with')
    ap.add_argument('--bn-stats', choices=['auto', 'batch'], default='auto',
                    help='auto: a checkpoint of train_like.py --bn-track (it holds running_mean keys) runs in eval mode on its '
                         'running statistics; batch: every frame\'s own statistics even then')
    ap.add_argument('--iou-alpha', type=float, default=0.5,
                    help='a checkpoint of train_like.py --iou-head (it holds backbone.rpn.iou.weight): scores are cls^(1-a) iou^a')
    ap.add_argument('--split', default='train', help='ImageSets/<split>.txt')
    ap.add_argument('--out', default=None, help='picture directory (default <dataroot>/pictures)')
    ap.add_argument('--view', choices=['bev', 'camera', 'both'], default='both')
    ap.add_argument('--frames', type=int, default=0, help='render the first N frames of the split (default 0: all)')
    ap.add_argument('--res', type=float, default=0.1, help='metres per pixel of the bird\'s-eye view')
    ap.add_argument('--thickness', type=int, default=1, choices=[1, 2, 3], help='line thickness in pixels')
    ap.add_argument('--synthetic', type=int, default=0, help='write a synthetic KITTI tree with this many frames into dataroot first')
    from detect_like import add_tta_arguments
    add_tta_arguments(ap)                        # with --checkpoint: the views' detections fused (modules/tta.py)
    return ap.parse_args(argv)


def read_result_boxes(path, calib):
    """The 'Car' rows of a KITTI result file -> {'boxes' (n, 7) LiDAR xyzlwhr, 'scores' (n,)}; a missing file has no rows."""
    from modules import Calc
    rows = []
    if os.path.exists(path):
        with open(path, 'r') as f:
            for line in f:
                tok = line.split()
                if len(tok) >= 16 and tok[0] == 'Car':
                    rows.append([float(v) for v in tok[8:16]])
    rows = torch.tensor(rows, dtype=torch.float32).reshape(-1, 8)
    c2v = torch.linalg.inv(torch.as_tensor(calib['Tr_velo_to_cam']).float())
    return dict(boxes=Calc.bboxCam2Lidar(rows[:, :7], c2v), scores=rows[:, 7].clone())


def _model_detector(args, device, data, names):
    """Frames -> (FrameBatch, per-frame detections) through the model of ``--checkpoint``, as detect_like.py runs it."""
    import modules.config as cfg
    from modules import bn_running as bnr
    from modules import Extension as X
    from modules import pipeline as pl
    from modules.Calc import bbox3d2bev
    from modules.data import Preprocessing as pre
    from modules.detect import detect_frame_set
    from MVXNet import MVXNet
    from train_like import fpn_maps_for
    anchors = pre.createAnchors(cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2, cfg.velorange, cfg.carsize)
    anchor_bevs = bbox3d2bev(anchors.reshape(anchors.shape[:2] + (-1, 7))).to(device).contiguous()
    anchors = anchors.to(device)
    torch.manual_seed(0)
    state = torch.load(args.checkpoint, map_location=device)
    direction = 'backbone.rpn.dir.weight' in state                            # written by train_like.py --direction
    tracked = bnr.checkpoint_tracks(state) and args.bn_stats != 'batch'      # written by train_like.py --bn-track
    if bnr.checkpoint_tracks(state) and not tracked:
        state = bnr.strip_running(state)
    cfg.config['bntrack'] = tracked             # main() restores it
    iou_head = 'backbone.rpn.iou.weight' in state                             # written by train_like.py --iou-head
    model = (MVXNet(direction=True, iou=True) if iou_head else MVXNet(direction=True) if direction else MVXNet()).to(device)
    model.load_state_dict(state)
    if tracked:
        model.eval()                            # detect_frame_set then normalises with the running statistics
    kw = dict(dir_offset=args.dir_offset) if direction else {}
    if iou_head:
        kw['iou_alpha'] = args.iou_alpha
    from modules import tta
    tta_kw, n_views = tta.options(args)
    kw.update(tta_kw)
    cap = max(d[0].shape[0] for d in data)

    def run(group, gnames):
        batch, _ = pl.batch_from_dataset(group, gnames, device, anchor_bevs, fpn_maps_for, cap_points=cap)
        return batch, detect_frame_set(model, batch, anchors, cfg.imsize, **kw)
    run.per_set = max(1, min(SET, X.MAX_FRAMES // n_views))              # F * V frames go through one forward
    return run


def main(args):
    import modules.config as cfg
    old = cfg.config.get('bntrack', False)
    try:
        return _main(args)
    finally:
        cfg.config['bntrack'] = old             # a tracked checkpoint switches it on for the run


def _main(args):
    import modules.config as cfg
    from modules import Extension as X
    from modules import render
    from modules.data import Load as load

    device = X.device()
    torch.cuda.set_device(device)
    if args.synthetic:
        from modules.data import Synthetic
        Synthetic.write_kitti_tree(args.dataroot, list(range(args.synthetic)))
    with open(os.path.join(args.dataroot, 'ImageSets', args.split + '.txt'), 'r') as f:
        names = [n for n in f.read().splitlines() if n]
    if args.frames > 0:
        names = names[:args.frames]
    data = load.createDataset(names, root=args.dataroot)
    out_dir = args.out or os.path.join(args.dataroot, 'pictures')
    detector = _model_detector(args, device, data, names) if args.checkpoint else None
    paths, dropped = [], 0
    per_set = detector.per_set if detector is not None else SET
    for lo in range(0, len(data), per_set):
        group, gnames = data[lo:lo + per_set], names[lo:lo + per_set]
        dets = None
        if detector is not None:
            points, dets = detector(group, gnames)
        else:
            points = render.points_from_dataset(group, device)
            if args.results:
                dets = [read_result_boxes(os.path.join(args.results, n + '.txt'), d[5]) for n, d in zip(gnames, group)]
        draw = render.draw_list([d[3] for d in group], dets, device=device)
        bev = cam = None
        status = []
        if args.view in ('bev', 'both'):
            bev, st = render.render_bev(points, draw, res=args.res, thickness=args.thickness)
            status.append(st)
        if args.view in ('camera', 'both'):
            cam, st = render.render_camera(points, draw, [d[5] for d in group], [d[1] for d in group], thickness=args.thickness)
            status.append(st)
        paths += render.save_frames(out_dir, gnames, bev, cam)
        dropped += int(np.count_nonzero(torch.stack(status).cpu().numpy()))
    print('%d frames, %d pictures -> %s%s' % (len(data), len(paths), out_dir,
                                             '' if not dropped else ' (%d views dropped a box: non-finite or far outside)' % dropped))
    return paths


if __name__ == '__main__':
    a = parse_args()
    sys.argv = sys.argv[:1]              # modules.config parses argv at import (reference modules/config/Parser.py:12)
    main(a)
