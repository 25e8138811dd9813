"""Times the test-time augmentation on device events, on the benchmark's 4-frame S2 batch (bench.make_batch) and a seeded,
untrained model, for V = 1, 2 and 4 views:
  * fuse        -- the three launches of tta.fuse_views alone (read=False) on that step's 4 V padded lists;
  * postprocess -- modules.detect.postprocess alone on the 4 V frames' heads, for comparison;
  * detect_tta  -- modules.detect.detect_frame_set(tta=views): expand_batch, the forward over 4 V frames, postprocess, fusion;
  * detect      -- detect_frame_set(tta=None) of the same process.
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

VIEW_SETS = {1: ['identity'], 2: ['identity', 'flip'], 4: ['identity', 'flip', 'rot+', 'rot-']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    sys.argv = sys.argv[:1]
    import torch
    import bench
    import modules.config as cfg
    from MVXNet import MVXNet
    from modules import detect, tta
    from modules.data import Preprocessing as pre

    dev = torch.device('cuda')
    cfg.config['convmath'] = 'bf16x6'
    frames = [0, 1, 2, 3]
    F = len(frames)
    batch = bench.make_batch(frames, dev, 20000, 'S2')
    torch.manual_seed(0)
    model = MVXNet().to(dev)
    anchors = pre.createAnchors(cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2, cfg.velorange, cfg.carsize).to(dev)

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
        return round(statistics.median(ms), 4)

    out = {'frames': F, 'convmath': 'bf16x6', 'iters': args.iters,
           'detect_ms': timed(lambda: detect.detect_frame_set(model, batch, anchors, cfg.imsize)), 'views': {}}
    for V, names in VIEW_SETS.items():
        rows = tta.views(names)
        keep = {}
        dets, live, _ = detect._detect_dev(model, tta.expand_batch(batch, rows), anchors, cfg.imsize, None, keep, {})
        full = detect.pad_frames(dets, live, F * V)
        heads, (n, h1, w1) = keep['heads'], keep['geom']
        fused = tta.fuse_views(full, rows, F, iou_thr=detect.DEFAULTS['iou_thr'])
        out['views'][V] = {
            'names': names,
            'fuse_ms': timed(lambda: tta.fuse_views(full, rows, F, iou_thr=detect.DEFAULTS['iou_thr'], read=False)),
            'postprocess_ms': timed(lambda: detect.postprocess(heads, anchors, n, h1, w1, read=False)),
            'detect_tta_ms': timed(lambda: detect.detect_frame_set(model, batch, anchors, cfg.imsize, tta=rows)),
            'merged_per_frame': [int(full['meta'][0, f * V:(f + 1) * V].sum()) for f in range(F)],
            'fused_per_frame': [int(d['boxes'].shape[0]) for d in fused],
            'mean_views_per_box': round(float(torch.cat([d['n_views'] for d in fused]).float().mean()), 3)}
        out['views'][V]['detect_tta_over_detect'] = round(out['views'][V]['detect_tta_ms'] / out['detect_ms'], 3)
        out['views'][V]['frames_per_s'] = round(F / out['views'][V]['detect_tta_ms'] * 1e3, 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
