"""Detection counterpart of train_like.py: boxes for every frame of a KITTI split from a checkpoint, written as KITTI
``label_2`` result files (one per frame) for the devkit.

Frames are read with ``Load.createDataset``, grouped into frame sets with ``pipeline.batch_from_dataset`` and run through
``detect.detect_frame_set`` (the training step's forward on this library's kernels, then decoding and rotated BEV NMS on the
GPU).  The feature maps come from the same stand-in as train_like.py when torchvision is absent.

    python detect_like.py <dataroot> --checkpoint checkpoints/epoch10.pkl [--split val] [--out results/data]
    python detect_like.py /tmp/kitti --synthetic 8          # a synthetic tree, an untrained (seeded) model
    python detect_like.py <dataroot> --split val --eval     # then score the files against the split's label_2 (eval_like.py)
    python detect_like.py <dataroot> --render pictures      # and a bird's-eye and a camera picture of every frame (visualize_like.py)
    python detect_like.py <dataroot> --tta identity flip     # test-time augmentation: the views' detections fused (modules/tta.py)
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('dataroot')
    ap.add_argument('--checkpoint', default=None, help='state dict written by train_like.py (default: the seeded, untrained model)')
    ap.add_argument('--split', default='train', help='ImageSets/<split>.txt')
    ap.add_argument('--out', default=None, help='result directory (default <dataroot>/results/data)')
    ap.add_argument('--synthetic', type=int, default=0, help='write a synthetic KITTI tree with this many frames into dataroot first')
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--frames', type=int, default=4, help='frames per frame set (with --tta of V views at most 16 // V)')
    ap.add_argument('--need-crop', action='store_true')
    ap.add_argument('--score-thr', type=float, default=0.05)
    ap.add_argument('--iou-thr', type=float, default=0.01)
    ap.add_argument('--pre-max', type=int, default=1000)
    ap.add_argument('--post-max', type=int, default=100)
    ap.add_argument('--decode', choices=['loss', 'reference'], default='loss')
    ap.add_argument('--dir-offset', type=float, default=math.pi / 4,
                    help='a checkpoint of train_like.py --direction (it holds backbone.rpn.dir.weight): the --dir-offset it was trained with')
    ap.add_argument('--bn-stats', choices=['auto', 'batch'], default='auto',
                    help='auto: a checkpoint of train_like.py --bn-track (it holds running_mean keys) runs in eval mode on its '
                         'running statistics; batch: every frame\'s own statistics even then (for comparison)')
    ap.add_argument('--iou-alpha', type=float, default=0.5,
                    help='a checkpoint of train_like.py --iou-head (it holds backbone.rpn.iou.weight): the scores are '
                         'cls^(1-a) iou^a with this a in [0, 1] (0 = the plain score; 0.5 is a design choice, not a measured optimum)')
    ap.add_argument('--eval', action='store_true', help='score the written files against the split\'s label_2 (KITTI AP on the GPU)')
    ap.add_argument('--classes', nargs='+', default=['Car'], help='classes scored by --eval')
    ap.add_argument('--extractor-weights', default=None,
                    help='state dict of the frozen ResNet50-FPN extractor (torchvision key names): images go through the HIP extractor')
    ap.add_argument('--render', default=None, metavar='DIR',
                    help='also write <name>_bev.png and <name>_cam.png of every frame (ground truth green, detections red to yellow)')
    add_tta_arguments(ap)
    return ap.parse_args(argv)


def add_tta_arguments(ap):
    """The test-time augmentation switches (also of visualize_like.py --checkpoint); ``modules.tta.options`` reads them."""
    ap.add_argument('--tta', nargs='+', default=None, metavar='NAME',
                    help='test-time augmentation: fuse the detections of these views (identity, flip, rot+, rot-, flip+rot+, flip+rot-)')
    ap.add_argument('--tta-rot', type=float, default=math.pi / 8, help='angle of the named rotations of --tta')
    ap.add_argument('--fuse-iou', type=float, default=0.5, help='--tta: a view votes for a cluster above this BEV IoU with its head')
    ap.add_argument('--min-views', type=int, default=1, help='--tta: clusters with fewer voting views are dropped')


def main(args):
    import modules.config as cfg
    old = cfg.config.get('bntrack', False)
    try:
        return _main(args)
    finally:
        cfg.config['bntrack'] = old             # a tracked checkpoint switches it on for the run


def _main(args):
    import modules.config as cfg
    from modules import bn_running as bnr
    from modules import Extension as X
    from modules import pipeline as pl
    from modules.Calc import bbox3d2bev
    from modules.data import Load as load, Preprocessing as pre
    from modules.detect import detect_frame_set, write_kitti_results
    from MVXNet import MVXNet
    from train_like import extractor_fpn_fn, fpn_maps_for

    device = X.device()
    torch.cuda.set_device(device)
    if args.synthetic:
        from modules.data import Synthetic
        Synthetic.write_kitti_tree(args.dataroot, list(range(args.synthetic)), points=args.points)
    with open(os.path.join(args.dataroot, 'ImageSets', args.split + '.txt'), 'r') as f:
        names = [n for n in f.read().splitlines() if n]
    data = load.createDataset(names, needCrop=args.need_crop, root=args.dataroot)
    out_dir = args.out or os.path.join(args.dataroot, 'results', 'data')
    os.makedirs(out_dir, exist_ok=True)

    anchors = pre.createAnchors(cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2, cfg.velorange, cfg.carsize)
    anchorBevs = bbox3d2bev(anchors.reshape(anchors.shape[:2] + (-1, 7))).to(device).contiguous()
    anchors = anchors.to(device)
    torch.manual_seed(0)
    state = torch.load(args.checkpoint, map_location=device) if args.checkpoint else None
    direction = state is not None and 'backbone.rpn.dir.weight' in state      # written by train_like.py --direction
    tracked = bnr.checkpoint_tracks(state) and args.bn_stats != 'batch'      # written by train_like.py --bn-track
    if bnr.checkpoint_tracks(state) and not tracked:
        state = bnr.strip_running(state)
    cfg.config['bntrack'] = tracked
    iou_head = state is not None and 'backbone.rpn.iou.weight' in state       # written by train_like.py --iou-head
    if iou_head:
        model = MVXNet(direction=True, iou=True).to(device)
        print('IoU head of the checkpoint: scores rectified with iou_alpha=%g' % args.iou_alpha)
    else:
        model = (MVXNet(direction=True) if direction else MVXNet()).to(device)
    if state is not None:
        model.load_state_dict(state)
    if tracked:
        model.eval()                            # detect_frame_set then normalises with the running statistics
        print('running BatchNorm statistics of the checkpoint (eval mode; --bn-stats batch: per-frame statistics)')
    fpn_fn = fpn_maps_for
    if args.extractor_weights:
        model.head.extractor.load_weights(args.extractor_weights).to(device)
        fpn_fn = extractor_fpn_fn(model.head.extractor, {n: d[1] for d, n in zip(data, names)})
    kw = dict(score_thr=args.score_thr, iou_thr=args.iou_thr, pre_max=args.pre_max, post_max=args.post_max, decode=args.decode)
    if direction:
        kw['dir_offset'] = args.dir_offset
    if iou_head:
        kw['iou_alpha'] = args.iou_alpha
    from modules import tta
    tta_kw, n_views = tta.options(args)
    kw.update(tta_kw)
    per_set = max(1, min(args.frames, X.MAX_FRAMES // n_views))          # F * V frames go through one forward
    cap = max(args.points, max(d[0].shape[0] for d in data))
    t0, n_boxes = time.perf_counter(), 0
    for lo in range(0, len(data), per_set):
        group, gnames = data[lo:lo + per_set], names[lo:lo + per_set]
        batch, _ = pl.batch_from_dataset(group, gnames, device, anchorBevs, fpn_fn, cap_points=cap)
        dets = detect_frame_set(model, batch, anchors, cfg.imsize, **kw)
        for name, d, frame in zip(gnames, dets, group):
            write_kitti_results(os.path.join(out_dir, name + '.txt'), d, frame[5], cfg.imsize)
            n_boxes += d['boxes'].shape[0]
        if args.render:                  # straight from the device tensors of the step just run
            from modules import render
            draw = render.draw_list([frame[3] for frame in group], dets, device=device)
            bev, _ = render.render_bev(batch, draw)
            cam, _ = render.render_camera(batch, draw, [frame[5] for frame in group], [frame[1] for frame in group])
            render.save_frames(args.render, gnames, bev, cam)
    dt = time.perf_counter() - t0
    print('%d frames, %d boxes -> %s (%.1f frames/s including file I/O)' % (len(data), n_boxes, out_dir, len(data) / max(dt, 1e-9)))
    if args.eval:
        import json
        from eval_like import run
        print(json.dumps(run(args.dataroot, out_dir, names, args.classes)))


if __name__ == '__main__':
    a = parse_args()
    sys.argv = sys.argv[:1]              # modules.config parses argv at import (reference modules/config/Parser.py:12)
    main(a)
