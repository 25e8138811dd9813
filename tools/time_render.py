"""Times the two rendered views on device events, on the benchmark's 4-frame S2 batch (bench.make_batch) with 100 boxes per
frame:
  * render_bev     -- modules.render.render_bev, 704 x 800 (0.1 m per pixel), three launches for the four frames;
  * render_camera  -- modules.render.render_camera, 370 x 1224, over a camera image and over black;
  * draw_list      -- modules.render.draw_list from a padded device dict (torch glue, no kernel of the library);
  * image_to_host  -- the device-to-host copy of one view's images.
Prints one JSON line (milliseconds per call for all four frames, medians over --iters windows of --calls calls after --warmup)."""
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
    ap.add_argument('--iters', type=int, default=20, help='timed windows')
    ap.add_argument('--calls', type=int, default=50, help='calls per window')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--boxes', type=int, default=100)
    args = ap.parse_args()
    sys.argv = sys.argv[:1]
    import numpy as np
    import torch
    import bench
    import modules.config as cfg
    from modules import render
    from modules.data import Synthetic

    dev = torch.device('cuda')
    frames = [0, 1, 2, 3]
    F = len(frames)
    batch = bench.make_batch(frames, dev, 20000, 'S2')
    points = batch.prepared()
    g = np.random.default_rng(0)
    vr = cfg.velorange
    n_gt = args.boxes // 5
    box = lambda n: np.stack([g.uniform(vr[0] + 3, vr[3] - 3, n), g.uniform(vr[1] + 3, vr[4] - 3, n), g.uniform(-1.8, -1.2, n),
                              g.uniform(3.4, 4.4, n), g.uniform(1.5, 1.8, n), g.uniform(1.4, 1.7, n), g.uniform(-3.1, 3.1, n)], 1)
    gts = [torch.from_numpy(box(n_gt).astype(np.float32)) for _ in frames]
    n_det = args.boxes - n_gt
    dets = dict(boxes=torch.from_numpy(np.stack([box(n_det) for _ in frames]).astype(np.float32)).to(dev),
                scores=torch.from_numpy(g.uniform(0.05, 1.0, (F, n_det)).astype(np.float32)).to(dev),
                meta=torch.tensor([[n_det] * F, [n_det] * F, [0] * F], dtype=torch.int32, device=dev))
    draw = render.draw_list(gts, dets)
    calibs = [Synthetic.KITTI_CALIB] * F
    images = torch.from_numpy(g.integers(0, 256, (F, int(cfg.imsize[0]), int(cfg.imsize[1]), 3), dtype=np.uint8)).to(dev)
    mats = render.image_from_lidar(calibs).to(dev)
    keep = {}

    def bev():
        keep['bev'] = render.render_bev(points, draw)

    def cam_image():
        keep['cam'] = render.render_camera(points, draw, calibs, images, matrices=mats)

    def cam_black():
        render.render_camera(points, draw, calibs, None, matrices=mats)

    def make_list():
        render.draw_list(gts, dets)

    def to_host():
        keep['bev'][0].cpu()

    def timed(fn):
        """Windows of --calls calls between two device events (one call is tens of microseconds: a window per call would
        measure the event pair); milliseconds per call."""
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.iters):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.calls):
                fn()
            e.record()
            torch.cuda.synchronize()
            ms.append(s.elapsed_time(e) / args.calls)
        return [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)]

    out = {'frames': F, 'boxes_per_frame': args.boxes, 'points_per_frame': points[1].tolist(), 'iters': args.iters, 'calls_per_window': args.calls,
           'bev_shape': list(render.bev_shape(0.1)), 'camera_shape': [int(v) for v in cfg.imsize]}
    for name, fn in (('render_bev', bev), ('render_camera_image', cam_image), ('render_camera_black', cam_black),
                     ('draw_list', make_list), ('image_to_host_bev', to_host)):
        out[name + '_ms_median_min_max'] = timed(fn)
    out['status'] = [keep['bev'][1].tolist(), keep['cam'][1].tolist()]
    print(json.dumps(out))


if __name__ == '__main__':
    main()
