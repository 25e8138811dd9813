"""Cost of the IoU-aware confidence head on device events, on the benchmark's 4-frame S2 batch
(bench.make_batch), in the manner of tools/time_direction.py:
  * train_step   -- pipeline.train_step_full with FocalLoss(direction=True) on MVXNet(direction=True) against
                    FocalLoss(direction=True, iou=True) on MVXNet(direction=True, iou=True), convmath bf16x6, same seed, same
                    batch and targets;
  * postprocess  -- modules.detect.postprocess alone on each model's heads (20 columns both; the IoU model rectifies);
  * loss         -- the loss entry alone on the step's heads and packed targets, mvx_focal_loss_dir_frames against
                    mvx_focal_loss_iou_frames: the difference is the new launch (focal_iou) at this batch's positive count.
The variants alternate in blocks of --iters calls, --rounds times, so that drift of the machine hits both alike.  Prints one
JSON line (milliseconds per call: the median over all rounds, and the per-round medians as the spread).
``--variants direction`` measures the direction model alone: the form that also runs on a tree without the IoU head (the
yardstick: the parent commit's direction model, run from its own checkout in alternation with this one)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'mvxnet-makise_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--variants', default='direction,iou')
    ap.add_argument('--label', default='')
    args = ap.parse_args()
    sys.argv = sys.argv[:1]
    import torch
    import bench
    import modules.config as cfg
    import modules.pipeline as pl
    from MVXNet import MVXNet
    from modules import Calc, parallel
    from modules.data import Preprocessing as pre
    from modules.detect import postprocess
    from modules.voxelnet.FocalLoss import FocalLoss

    dev = torch.device('cuda')
    cfg.config['convmath'] = 'bf16x6'
    frames = [0, 1, 2, 3]
    batch = bench.make_batch(frames, dev, 20000, 'S2')
    anchors = pre.createAnchors(cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2, cfg.velorange, cfg.carsize)
    bevs = Calc.bbox3d2bev(anchors.reshape(anchors.shape[:2] + (-1, 7))).to(dev).contiguous()
    anchors = anchors.to(dev)
    gt = bench.synthetic_gt()
    lists = Calc.classifyAnchorsFrames([(Calc.bbox3d2bev(gt), gt[:, [0, 1]])] * len(frames), bevs, cfg.velorange, 0.45, 0.6)
    targets = [(t[0], t[1], t[2], gt.to(dev)) for t in lists]

    variants = {}
    for name in args.variants.split(','):
        iou = name == 'iou'
        torch.manual_seed(0)
        model = (MVXNet(direction=True, iou=True) if iou else MVXNet(direction=True)).to(dev)
        bucket = parallel.GradBucket([p for p in model.parameters() if p.requires_grad])
        crit = FocalLoss(direction=True, iou=True) if iou else FocalLoss(direction=True)
        keep = {}

        def train(model=model, bucket=bucket, crit=crit, keep=keep):
            bucket.zero()
            return pl.train_step_full(model, batch, targets, crit, anchors, cfg.imsize, keep=keep)

        def post(keep=keep, iou=iou):
            F, h1, w1 = keep['geom'][0], keep['geom'][5], keep['geom'][6]
            return postprocess(keep['heads'], anchors, F, h1, w1, **(dict(iou=True) if iou else {}))

        def loss(crit=crit, keep=keep):
            F, h1, w1 = keep['geom'][0], keep['geom'][5], keep['geom'][6]
            return crit.heads_loss_frames(keep['heads'], F, h1, w1, targets, anchors)

        variants[name] = dict(train=train, post=post, loss=loss, keep=keep)

    def block(fn, n):
        ms = []
        for _ in range(n):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            ms.append(s.elapsed_time(e))
        return ms

    out = {'label': args.label, 'frames': len(frames), 'convmath': 'bf16x6', 'iters': args.iters, 'rounds': args.rounds,
           'positives_per_frame': [int(len(t[0][0])) for t in targets]}
    for what in ('train', 'post', 'loss'):
        for v in variants.values():
            block(v[what], args.warmup)
        samples = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, v in variants.items():
                samples[name].append(block(v[what], args.iters))
        for name, rounds in samples.items():
            out['%s_%s_ms' % (what, name)] = round(statistics.median([x for r in rounds for x in r]), 4)
            out['%s_%s_round_medians_ms' % (what, name)] = [round(statistics.median(r), 4) for r in rounds]
        if len(variants) == 2:
            out['%s_ratio' % what] = round(out['%s_iou_ms' % what] / out['%s_direction_ms' % what], 4)
    out['heads_columns'] = {name: int(v['keep']['heads'].shape[1]) for name, v in variants.items()}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
