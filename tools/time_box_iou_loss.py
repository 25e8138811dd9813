"""Cost of the rotated 3D IoU regression loss on device events, on the benchmark's 4-frame S2 batch
(bench.make_batch) with the benchmark's synthetic targets, in the manner of tools/time_iou_head.py:
  * launch      -- mvx_box_iou_loss_frames alone (forward + gradient into a d_heads) at the full grid, 4 x 176 x 200 x 2
                   anchors: on the heads of the untrained model (most positives decode off their box: little clipping) and on
                   zero regression rows (every positive decodes onto its anchor and overlaps its box: every entry clips);
                   per call, from --iters calls between two events;
  * loss        -- FocalLoss.heads_loss_frames with and without iou_loss on the step's heads;
  * train_step  -- pipeline.train_step_full with FocalLoss() against FocalLoss(iou_loss=True) on MVXNet(), convmath bf16x6,
                   same seed, batch and targets.
The variants alternate in blocks of --iters calls, --rounds times.  Prints one JSON line (milliseconds per call: the median over
all rounds, and the per-round medians as the spread)."""
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
    args = ap.parse_args()
    sys.argv = sys.argv[:1]
    import torch
    import bench
    import modules.config as cfg
    import modules.pipeline as pl
    from MVXNet import MVXNet
    from modules import Calc, _hip, parallel
    from modules.data import Preprocessing as pre
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
    for name in ('focal', 'iou_loss'):
        torch.manual_seed(0)
        model = MVXNet().to(dev)
        bucket = parallel.GradBucket([p for p in model.parameters() if p.requires_grad])
        crit = FocalLoss(iou_loss=(name == 'iou_loss'))
        keep = {}

        def train(model=model, bucket=bucket, crit=crit, keep=keep):
            bucket.zero()
            return pl.train_step_full(model, batch, targets, crit, anchors, cfg.imsize, keep=keep)

        def loss(crit=crit, keep=keep):
            F, h1, w1 = keep['geom'][0], keep['geom'][5], keep['geom'][6]
            return crit.heads_loss_frames(keep['heads'], F, h1, w1, targets, anchors)

        variants[name] = dict(train=train, loss=loss, keep=keep, crit=crit)

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

    out = {'frames': len(frames), 'convmath': 'bf16x6', 'iters': args.iters, 'rounds': args.rounds,
           'positives_per_frame': [int(len(t[0][0])) for t in targets]}
    for what in ('train', 'loss'):
        for v in variants.values():
            block(v[what], args.warmup)
        samples = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, v in variants.items():
                samples[name].append(block(v[what], args.iters))
        for name, rounds in samples.items():
            out['%s_%s_ms' % (what, name)] = round(statistics.median([x for r in rounds for x in r]), 4)
            out['%s_%s_round_medians_ms' % (what, name)] = [round(statistics.median(r), 4) for r in rounds]
        out['%s_ratio' % what] = round(out['%s_iou_loss_ms' % what] / out['%s_focal_ms' % what], 4)
    out['mean_iou_of_the_positives'] = [round(v, 4) for v in variants['iou_loss']['crit'].last_box_iou[:, 1].tolist()]

    # the launch alone: --iters calls between two events, so that the events' own cost does not hide a launch of a few us
    keep = variants['iou_loss']['keep']
    F, h1, w1 = keep['geom'][0], keep['geom'][5], keep['geom'][6]
    packed, _ = FocalLoss.pack_targets(targets, dev)
    anc = anchors.detach().float().contiguous()
    for label, heads in (('model_heads', keep['heads']), ('zero_rows', torch.zeros_like(keep['heads']))):
        d = torch.zeros_like(heads)

        def launch(heads=heads, d=d):
            return _hip.box_iou_loss_frames(heads, F, h1, w1, 2, packed.pos_idx, packed.gi, packed.counts, packed.gts, packed.gt_off,
                                            anc, 1.0, d_heads=d)
        for _ in range(args.warmup):
            launch()
        rounds = []
        for _ in range(args.rounds):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.iters):
                res = launch()
            e.record()
            torch.cuda.synchronize()
            rounds.append(s.elapsed_time(e) / args.iters)
        out['launch_%s_ms' % label] = round(statistics.median(rounds), 5)
        out['launch_%s_rounds_ms' % label] = [round(r, 5) for r in rounds]
        out['launch_%s_mean_iou' % label] = [round(v, 4) for v in res[0][:, 1].tolist()]
    print(json.dumps(out))


if __name__ == '__main__':
    main()
