"""Times the detection output on device events, on the benchmark's 4-frame S2 batch (bench.make_batch):
  * detect_step  -- modules.detect.detect_frame_set (frame-set forward + RPN + postprocess, default thresholds);
  * postprocess  -- modules.detect.postprocess alone on that step's heads (4 frames, defaults);
  * train_step   -- pipeline.train_step_full on the same batch, convmath bf16x6.
Prints one JSON line (milliseconds per call, medians over --iters calls after --warmup)."""
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
    args = ap.parse_args()
    sys.argv = sys.argv[:1]
    import torch
    import bench
    import modules.config as cfg
    import modules.pipeline as pl
    from MVXNet import MVXNet
    from modules import Calc, parallel
    from modules.data import Preprocessing as pre
    from modules.detect import detect_frame_set, postprocess
    from modules.voxelnet import VoxelLoss

    dev = torch.device('cuda')
    cfg.config['convmath'] = 'bf16x6'
    frames = [0, 1, 2, 3]
    batch = bench.make_batch(frames, dev, 20000, 'S2')
    torch.manual_seed(0)
    model = MVXNet().to(dev)
    bucket = parallel.GradBucket([p for p in model.parameters() if p.requires_grad])
    anchors = pre.createAnchors(cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2, cfg.velorange, cfg.carsize)
    bevs = Calc.bbox3d2bev(anchors.reshape(anchors.shape[:2] + (-1, 7))).to(dev).contiguous()
    anchors = anchors.to(dev)
    gt = bench.synthetic_gt()
    lists = Calc.classifyAnchorsFrames([(Calc.bbox3d2bev(gt), gt[:, [0, 1]])] * len(frames), bevs, cfg.velorange, 0.45, 0.6)
    targets = [(t[0], t[1], t[2], gt.to(dev)) for t in lists]
    crit = VoxelLoss()
    keep = {}

    def detect():
        return detect_frame_set(model, batch, anchors, cfg.imsize, keep=keep)

    def post():
        F, h1, w1 = keep['geom']
        return postprocess(keep['heads'], anchors, F, h1, w1)

    def train():
        bucket.zero()
        return pl.train_step_full(model, batch, targets, crit, anchors, cfg.imsize)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.iters):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            ms.append(s.elapsed_time(e))
        return statistics.median(ms), min(ms), max(ms)

    det, pp, tr = timed(detect), timed(post), timed(train)
    dets = detect()
    F = len(frames)
    print(json.dumps({
        'frames': F, 'convmath': 'bf16x6', 'iters': args.iters,
        'detect_step_ms': round(det[0], 3), 'detect_step_min_max_ms': [round(det[1], 3), round(det[2], 3)],
        'detect_frames_per_s': round(F / det[0] * 1e3, 1),
        'postprocess_ms': round(pp[0], 4), 'postprocess_min_max_ms': [round(pp[1], 4), round(pp[2], 4)],
        'train_step_ms': round(tr[0], 3), 'train_frames_per_s': round(F / tr[0] * 1e3, 1),
        'detect_over_train': round(det[0] / tr[0], 3),
        'boxes_per_frame': [int(d['boxes'].shape[0]) for d in dets],
        'candidates_per_frame': [int(d['n_candidates']) for d in dets]}))


if __name__ == '__main__':
    main()
