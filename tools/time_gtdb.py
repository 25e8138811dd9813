"""Times the GT-paste database builder (csrc/gtdb.hip, modules/augment/BuildGT.py) on a synthetic split
(modules/data/Synthetic.write_kins_tree, --frames frames of --points background points, one batch):
  * match_ms / count_ms / raster_ms / write_ms -- each call alone between device events, inputs resident;
  * device_ms       -- the four calls (six launches) and the host read between them (BuildGT.run), the same way;
  * build_ms        -- buildFrames on parsed frames (upload, launches, read, per-class tables and infos), wall clock;
  * parse_ms        -- json / label / PIL / .bin parsing of the batch, wall clock (host work the builder keeps);
  * restatement_ms  -- tests/gtdb_ref.py on the same frames, wall clock: the only baseline there is, the reference's own script
                       needs open3d, pycocotools, OpenCV and pandas.
Prints one JSON line (medians over --iters calls after --warmup); per-frame figures divide by the frames processed."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'mvxnet-makise_amd'), os.path.join(ROOT, 'tests'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--no-restatement', action='store_true')
    args = ap.parse_args()
    sys.argv = sys.argv[:1]
    import numpy as np
    import torch
    from modules import _hip
    from modules.augment import BuildGT
    from modules.data import Synthetic as S

    dev = torch.device('cuda')
    with tempfile.TemporaryDirectory() as tmp:
        S.write_kins_tree(tmp, list(range(args.frames)), points=args.points, no_annotation=(), out_of_range=())
        seg = os.path.join(tmp, 'seglabel', 'update_train_2020.json')
        train = set(open(os.path.join(tmp, 'ImageSets/train.txt')).read().splitlines())

        def parse():
            ann = BuildGT.readAnnotations(seg)
            order = BuildGT.frameOrder(ann, train)
            return [BuildGT.loadFrame(tmp, n) for _, n in order], [ann.by_image[i] for i, _ in order]

        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            frames, anns = parse()
            ts.append((time.perf_counter() - t0) * 1e3)
        res = {'frames': len(frames), 'points_per_frame': int(np.mean([f['velo'].shape[0] for f in frames])), 'iters': args.iters,
               'parse_ms': round(statistics.median(ts), 2)}
        if not args.no_restatement:
            import gtdb_ref as R
            t0 = time.perf_counter()
            r = R.build(tmp, seg)
            res['restatement_ms'] = round((time.perf_counter() - t0) * 1e3, 2)
    t = BuildGT.pack(frames, anns, device=dev)
    h, d = BuildGT.run(t)
    res.update(labels=t.n_labels, objects=int((h.flag == 3).sum()), mask_px=int(h.px_off[-1]), object_points=int(h.pt_off[-1]),
               edges=int(t.edges.shape[0]))
    best, iou, flag, roi, px_off = _hip.gtdb_match(t)
    pt_off, ws = _hip.gtdb_crop_count(t, flag)
    rows = int((h.roi[h.flag == 3, 3] - h.roi[h.flag == 3, 1] + 1).max())

    def timed(fn):
        ms = []
        for k in range(args.warmup + args.iters):
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                ms.append(s.elapsed_time(e))
        return round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)

    for name, fn in (('match', lambda: _hip.gtdb_match(t)), ('count', lambda: _hip.gtdb_crop_count(t, flag)),
                     ('raster', lambda: _hip.gtdb_raster(t, best, flag, roi, px_off, int(h.px_off[-1]), rows)),
                     ('write', lambda: _hip.gtdb_crop_write(t, flag, pt_off, ws, int(h.pt_off[-1]))),
                     ('device', lambda: BuildGT.run(t))):
        med, lo, hi = timed(fn)
        res[name + '_ms'] = med
        res[name + '_min_max_ms'] = [lo, hi]
    ts = []
    for k in range(args.warmup + args.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        built = BuildGT.buildFrames(frames, anns, device=dev)
        torch.cuda.synchronize()
        if k >= args.warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    res['build_ms'] = round(statistics.median(ts), 3)
    res['build_ms_per_frame'] = round(res['build_ms'] / len(frames), 3)
    res['device_ms_per_frame'] = round(res['device_ms'] / len(frames), 4)
    if not args.no_restatement:
        res['restatement_ms_per_frame'] = round(res['restatement_ms'] / len(frames), 2)
        same = all(np.array_equal(built[c]['tables']['mask'].cpu().numpy(),
                                  np.concatenate([o['mask_px'].reshape(-1) for o in r['objects'][c]] + [np.zeros((0,), np.uint8)]))
                   and np.array_equal(built[c]['tables']['points'].cpu().numpy(),
                                      np.concatenate([o['points'] for o in r['objects'][c]] + [np.zeros((0, 4), np.float32)]))
                   for c in BuildGT.CLASSES)
        res['restatement_equal'] = bool(same)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
