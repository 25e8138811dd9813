"""Times the KITTI object evaluation (modules/kitti_eval.py, csrc/kitti_eval.hip) on a seeded synthetic split of the size of
KITTI val: --frames frames (3,769), --dets detections per frame (100 = post_max), 0..12 labelled objects per frame.
Reports per-stage device times from hipEvents (medians over --iters evaluations after --warmup), the end-to-end time of
``evaluate`` (host layout and upload included), and -- for contrast -- the host reference (tests/kitti_eval_ref.py) on the
first --ref-frames frames.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'mvxnet-makise_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def synthetic_split(F, dets, seed=0):
    """(gt_annos, dt_annos): per frame 0..12 objects (Car / Van / Pedestrian / DontCare) and ``dets`` detections -- jittered
    copies of the labels and clutter, scores on a 0.01 grid."""
    g = np.random.default_rng(seed)
    names = np.array(['Car', 'Car', 'Car', 'Van', 'Pedestrian', 'DontCare'])
    gts, dts = [], []
    for _ in range(F):
        n = int(g.integers(0, 13))
        x1, y1 = g.uniform(0, 1100, n), g.uniform(120, 250, n)
        gt = dict(name=names[g.integers(0, len(names), n)], truncated=g.choice([0.0, 0.1, 0.3, 0.6], n),
                  occluded=g.integers(0, 4, n).astype(np.float64), alpha=g.uniform(-3, 3, n),
                  bbox=np.stack([x1, y1, x1 + g.uniform(20, 160, n), y1 + g.uniform(15, 150, n)], 1),
                  hwl=np.stack([g.uniform(1.4, 1.8, n), g.uniform(1.5, 1.9, n), g.uniform(3.4, 4.8, n)], 1),
                  location=np.stack([g.uniform(-25, 25, n), g.uniform(1.2, 2.0, n), g.uniform(5, 70, n)], 1),
                  rotation_y=g.uniform(-3.1, 3.1, n), score=np.zeros(n))
        src = g.integers(0, max(n, 1), dets) if n else np.zeros(dets, np.int64)
        copy = (g.uniform(size=dets) < 0.5) & (n > 0)
        j = g.uniform(0, 0.5, dets)[:, None]
        base = {k: (v[src] if n else np.zeros((dets,) + v.shape[1:])) for k, v in gt.items() if k != 'name'}
        cx1, cy1 = g.uniform(0, 1100, dets), g.uniform(120, 250, dets)
        clutter = dict(bbox=np.stack([cx1, cy1, cx1 + g.uniform(20, 150, dets), cy1 + g.uniform(15, 120, dets)], 1),
                       hwl=np.tile([1.6, 1.7, 4.0], (dets, 1)),
                       location=np.stack([g.uniform(-25, 25, dets), np.full(dets, 1.6), g.uniform(5, 70, dets)], 1),
                       rotation_y=g.uniform(-3.1, 3.1, dets), alpha=g.uniform(-3, 3, dets))
        dt = {}
        for k in ('bbox', 'hwl', 'location', 'rotation_y', 'alpha'):
            jit = base[k] + g.normal(0, 1, base[k].shape) * (j * (20 if k == 'bbox' else 0.3) if base[k].ndim == 2 else j[:, 0] * 0.3)
            c = copy[:, None] if base[k].ndim == 2 else copy
            dt[k] = np.where(c, jit, clutter[k])
        dt['name'] = np.where(g.uniform(size=dets) < 0.8, 'Car', 'Pedestrian')
        dt['truncated'] = np.full(dets, -1.0)
        dt['occluded'] = np.full(dets, -1.0)
        dt['score'] = np.round(g.uniform(0, 1, dets), 2)
        gts.append(gt)
        dts.append(dt)
    return gts, dts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=3769)
    ap.add_argument('--dets', type=int, default=100)
    ap.add_argument('--classes', nargs='+', default=['Car', 'Pedestrian', 'Cyclist'])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--ref-frames', type=int, default=40, help='frames of the host reference run (0: skip)')
    args = ap.parse_args()
    sys.argv = sys.argv[:1]
    import torch
    from modules import kitti_eval as ke

    dev = torch.device('cuda')
    gts, dts = synthetic_split(args.frames, args.dets)
    classes = tuple(args.classes)
    stage_names = ('overlaps', 'tp_scores+sort', 'thresholds', 'counts')
    stages, total = [], []
    for it in range(args.warmup + args.iters):
        events = []
        t0 = time.perf_counter()
        res = ke.evaluate(gts, dts, classes, dev, events)
        t1 = time.perf_counter()
        if it >= args.warmup:
            stages.append([events[k].elapsed_time(events[k + 1]) for k in range(len(events) - 1)])
            total.append((t1 - t0) * 1e3)
    med = [statistics.median(s[k] for s in stages) for k in range(len(stage_names))]
    inp = ke.EvalInput(gts, dts, classes)
    out = dict(frames=args.frames, dets_per_frame=args.dets, gt_rows=int(inp.off[1, -1]), dontcare_rows=int(inp.off[2, -1]),
               pairs=inp.n_pairs, curves=len(inp.keys), device_ms=dict(zip(stage_names, [round(v, 3) for v in med])),
               device_total_ms=round(sum(med), 3), evaluate_ms=round(statistics.median(total), 1),
               car_moderate_3d_r40=res['ap']['Car'][0]['3d']['R40'][1])
    if args.ref_frames:
        import kitti_eval_ref as R
        n = min(args.ref_frames, args.frames)
        t0 = time.perf_counter()
        R.evaluate(gts[:n], dts[:n], classes)
        dt = time.perf_counter() - t0
        out.update(ref_frames=n, ref_s=round(dt, 2), ref_s_per_frame=round(dt / n, 4))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
