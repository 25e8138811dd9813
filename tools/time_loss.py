"""Times the two losses of the frame-set heads on device events, on --frames (4) frames of the 176 x 200 x 2 head map with
--positives (40) positive and 150 further not-negative anchors per frame, lists on the device as Calc.classifyAnchorsFrames
returns them:
  * voxel -- pipeline.heads_loss with VoxelLoss (a Python loop over the frames: sigmoid, per-frame index blocks, two launches
             and a memset per frame, the sigmoid's derivative);
  * focal -- FocalLoss.heads_loss_frames (pack_targets + one library call: three launches and a memset for any F).
Each call is timed from an event before its first host instruction to an event after its last launch (host work that the
device waits for is part of the figure), median over --iters calls after --warmup.  Prints one JSON line: milliseconds per
call and the library's kernel launches per call (mvx_launch_count: memsets and torch's own kernels are not counted), the
latter also for one frame."""
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
    ap.add_argument('--frames', type=int, default=4)
    ap.add_argument('--positives', type=int, default=40)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    args = ap.parse_args()
    sys.argv = sys.argv[:1]
    import numpy as np
    import torch
    import modules.config as cfg
    import modules.pipeline as pl
    from modules import _hip
    from modules.data import Preprocessing as pre
    from modules.voxelnet import VoxelLoss
    from modules.voxelnet.FocalLoss import FocalLoss

    dev = torch.device('cuda')
    l, w, A = cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2, 2
    anchors = pre.createAnchors(l, w, cfg.velorange, cfg.carsize).to(dev)
    an = anchors.detach().float().reshape(l, w, A, 7)
    rng = np.random.default_rng(0)
    g = torch.Generator(device=dev).manual_seed(0)

    def make(F):
        heads = torch.randn((F * l * w, 8 * A), generator=g, device=dev)
        targets = []
        for _ in range(F):
            pick = rng.permutation(l * w * A)[:args.positives + 150]
            xyz = [torch.from_numpy(c).to(dev) for c in (pick // (w * A), (pick // A) % w, pick % A)]
            pi = tuple(c[:args.positives] for c in xyz)
            gts = an[pi[0][:8], pi[1][:8], pi[2][:8]].clone()                 # 8 boxes: anchors, moved and resized a little
            gts[:, :3] += 0.3
            gts[:, 3:6] *= 1.1
            gi = torch.from_numpy(rng.integers(0, 8, args.positives)).to(dev)
            targets.append((pi, tuple(xyz), gi, gts))
        return heads, targets

    voxel, focal = VoxelLoss(), FocalLoss()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        l0 = _hip.X.lib.mvx_launch_count()
        fn()
        launches = _hip.X.lib.mvx_launch_count() - l0
        ms = []
        for _ in range(args.iters):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            ms.append(s.elapsed_time(e))
        return {'ms': round(statistics.median(ms), 4), 'min_max_ms': [round(min(ms), 4), round(max(ms), 4)], 'launches': int(launches)}

    out = {'frames': args.frames, 'head_map': [l, w, A], 'positives_per_frame': args.positives, 'iters': args.iters,
           'device': torch.cuda.get_device_name(dev)}
    for F in sorted({1, args.frames}):
        heads, targets = make(F)
        res = {'voxel': timed(lambda: pl.heads_loss(heads, F, l, w, targets, voxel, anchors)),
               'focal': timed(lambda: focal.heads_loss_frames(heads, F, l, w, targets, anchors))}
        packed, _ = focal.pack_targets(targets, dev)
        res['focal_kernels_only'] = timed(lambda: _hip.focal_loss_frames(
            heads, F, l, w, A, packed.pos_idx, packed.neg_idx, packed.gi, packed.counts, packed.gts, packed.gt_off,
            an, focal.alpha, focal.gamma, focal.cls_weight, focal.reg_weight))
        out['F=%d' % F] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
