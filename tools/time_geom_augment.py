"""Times the geometric augmentation on a 4-frame batch of S2 ring frames (20,000 points each) with twelve boxes per frame:
  * device_ms   -- the three launches (placement, point count, point write) between device events, draws given;
  * place_ms / points_ms -- the placement alone and the two point launches alone, the same way;
  * host_draw_ms -- draw_geometry for the batch (32 box slots, 16 trials);
  * kept        -- boxes and points per frame behind the filter.
Prints one JSON line (medians over --iters calls after --warmup)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'mvxnet-makise_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--trials', type=int, default=16)
    args = ap.parse_args()
    sys.argv = sys.argv[:1]
    import numpy as np
    import torch
    import modules.config as cfg
    from modules import _hip
    from modules.augment import Geometry as G
    from modules.data import Synthetic as S

    dev = torch.device('cuda')
    F, NB, P = 4, 12, 20000
    rng = np.random.default_rng(0)
    clouds = [S.synth_ring(f, P) for f in range(F)]
    pts = torch.zeros((F, P, 6), dtype=torch.float32, device=dev)
    for f, c in enumerate(clouds):
        pts[f, :c.shape[0], :4] = torch.from_numpy(c).to(dev)
    n_pts = torch.tensor([c.shape[0] for c in clouds], dtype=torch.int32, device=dev)
    # twelve cars per frame on a loose grid in front of the sensor
    boxes = []
    for f in range(F):
        b = [[x + rng.uniform(-1, 1), y + rng.uniform(-1, 1), -1.6, 3.9, 1.6, 1.56, rng.uniform(-np.pi, np.pi)]
             for x in (10, 20, 30, 40) for y in (-10, 0, 10)]
        boxes.append(torch.tensor(b, dtype=torch.float32))
    b3, n_box = G.box_table(boxes, dev)
    params = G.GeomParams(trials=args.trials)
    noise, glob = G.draw_geometry(F, b3.shape[1], params, rng)
    noise_d, glob_d = torch.from_numpy(noise).to(dev), torch.from_numpy(glob).to(dev)
    status = torch.zeros((F,), dtype=torch.int32, device=dev)
    state = {}

    def place():
        state['placed'] = _hip.geom_place(b3, n_box, noise_d, glob_d, cfg.velorange, status, iou_thr=params.iou_thr)

    def points():
        state['out'] = _hip.geom_points(pts, n_pts, b3, n_box, state['placed'], glob_d, cfg.velorange)

    def both():
        place(), points()

    def timed(fn):
        ms = []
        for k in range(args.warmup + args.iters):
            if fn is points:
                place()
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                ms.append(s.elapsed_time(e))
        return round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)

    res = {'frames': F, 'points': P, 'boxes_per_frame': NB, 'trials': args.trials, 'iters': args.iters}
    for name, fn in (('device', both), ('place', place), ('points', points)):
        med, lo, hi = timed(fn)
        res[name + '_ms'] = med
        res[name + '_min_max_ms'] = [lo, hi]
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        G.draw_geometry(F, b3.shape[1], params, rng)
        ts.append((time.perf_counter() - t0) * 1e3)
    res['host_draw_ms'] = round(statistics.median(ts), 3)
    res['kept'] = {'boxes': state['placed'].n_kept.cpu().tolist(), 'points': state['out'][1].cpu().tolist(),
                   'moved_boxes': (state['placed'].trial >= 0).sum(1).cpu().tolist()}
    assert status.cpu().tolist() == [0] * F
    print(json.dumps(res))


if __name__ == '__main__':
    main()
