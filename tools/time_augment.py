"""Times the GT-paste augmentation on a 4-frame batch of S2 ring frames (20,000 points each) with a synthetic object database:
  * device_ms        -- the four launches (ground grid, placement, point paste, image paste) between device events, draws given;
  * per kernel       -- each launch alone, the same way;
  * host_draw_ms     -- the host's draws for the batch, in the reference's order (np.random, a permutation of the database per
                        slot) and with a Generator, for --objects and for a KITTI-sized database of 14,357 cars;
  * restatement_ms   -- tests/augment_ref.py on the same four frames and draws (the CPU baseline), wall clock;
  * db_bytes         -- resident size of the database's tables, and that scaled to 14,357 objects.
Prints one JSON line (medians over --iters calls after --warmup)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'mvxnet-makise_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

KITTI_CARS = 14357


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--objects', type=int, default=500)
    ap.add_argument('--no-restatement', action='store_true')
    args = ap.parse_args()
    sys.argv = sys.argv[:1]
    import numpy as np
    import torch
    import modules.config as cfg
    from modules import _hip
    from modules.augment import Augment as A
    from modules.augment.LoadGT import GTDatabase, getAllGT
    from modules.data import Synthetic as S

    dev = torch.device('cuda')
    F, LIM = 4, 12
    with tempfile.TemporaryDirectory() as tmp:
        S.write_gt_database(tmp, args.objects, seed=0)
        gts = getAllGT(['Car'], root=tmp)['Car']
    db = GTDatabase.from_gts(gts, dev)
    clouds = [S.synth_ring(f, 20000) for f in range(F)]
    cap = 20000 + LIM * db.max_points
    pts0 = torch.zeros((F, cap, 6), dtype=torch.float32, device=dev)
    for f, c in enumerate(clouds):
        pts0[f, :c.shape[0], :4] = torch.from_numpy(c).to(dev)
    n0 = torch.tensor([c.shape[0] for c in clouds], dtype=torch.int32, device=dev)
    # two scene boxes per frame, taken from the database itself
    scenes = [(db.box2d[2 * f:2 * f + 2].cpu(), db.box3d[2 * f:2 * f + 2].cpu(), db.bev[2 * f:2 * f + 2].cpu()) for f in range(F)]
    S_max = LIM - 2
    g = np.random.default_rng(0)
    cand = np.stack([A.draw_slots(db.n, S_max, rng=g)[0] for _ in range(F)])
    thr = np.stack([A.draw_slots(db.n, S_max, rng=g)[1] for _ in range(F)])
    cand_d, thr_d = torch.from_numpy(cand).to(dev), torch.from_numpy(thr).to(dev)
    img0 = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (F, 370, 1224, 3), dtype=np.uint8)).to(dev)
    b2_0, b3_0, bv_0, ns = A._scene_tables(scenes, _hip.GT_PASTE_MAX_BOXES, dev)
    ns = ns.to(dev)
    status = torch.zeros((F,), dtype=torch.int32, device=dev)
    state = {}

    def reset():
        state.update(pts=pts0.clone(), img=img0.clone(), b2=b2_0.clone(), b3=b3_0.clone(), bv=bv_0.clone())

    def ground():
        state['z'] = _hip.gt_paste_ground(state['pts'], n0, cfg.velorange)

    def place():
        state['picked'], _ = _hip.gt_paste_place(state['z'], cfg.velorange, state['b2'], state['b3'], state['bv'], ns, LIM, cand_d, thr_d,
                                                 db, status)

    def points():
        _hip.gt_paste_points(state['pts'], n0, state['picked'], db, status)

    def image():
        _hip.gt_paste_image(state['img'], state['picked'], db)

    def all_four():
        ground(), place(), points(), image()

    def timed(fn):
        ms = []
        for k in range(args.warmup + args.iters):
            reset()                                   # outside the timed window: fresh tables, the same work every call
            if fn is not ground and fn is not all_four:
                ground()
            if fn in (points, image):
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

    res = {'frames': F, 'objects': db.n, 'iters': args.iters, 'slots_per_frame': S_max}
    for name, fn in (('device', all_four), ('ground', ground), ('place', place), ('points', points), ('image', image)):
        med, lo, hi = timed(fn)
        res[name + '_ms'] = med
        res[name + '_min_max_ms'] = [lo, hi]
    res['pasted_per_frame'] = [int((row >= 0).sum()) for row in state['picked'].cpu().numpy()]

    def draw_ms(n_db, rng):
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _f in range(F):
                A.draw_slots(n_db, S_max, rng=rng)
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ts), 3)

    res['host_draw_ms'] = {'np_random_%d' % db.n: draw_ms(db.n, None), 'generator_%d' % db.n: draw_ms(db.n, np.random.default_rng(0)),
                           'np_random_%d' % KITTI_CARS: draw_ms(KITTI_CARS, None),
                           'generator_%d' % KITTI_CARS: draw_ms(KITTI_CARS, np.random.default_rng(0))}
    res['db_bytes'] = db.nbytes()
    res['db_bytes_scaled_to_%d' % KITTI_CARS] = int(db.nbytes() / db.n * KITTI_CARS)
    if not args.no_restatement:
        import augment_ref as R
        import mvx_oracle as O
        t = R.db_tables(db)
        imgs = img0.cpu().numpy()
        t0 = time.perf_counter()
        same = True
        for f in range(F):
            zm = R.ground_grid(clouds[f], cfg.velorange)
            r = R.place_frame(zm, cfg.velorange, *[x.numpy() for x in scenes[f]], LIM, cand[f], thr[f], t,
                              lambda a, b: O.bbox_pairwise(a, b, True))
            R.paste_points(np.zeros((clouds[f].shape[0], 6), np.float32), r['picked'], t['points'], t['pt_off'], cap)
            R.paste_image(imgs[f], r['picked'], t['patch'], t['mask'], t['px_off'], t['maskbbox'])
            same = same and r['picked'].tolist() == state['picked'][f].cpu().tolist()
        res['restatement_ms'] = round((time.perf_counter() - t0) * 1e3, 2)
        res['restatement_picks_equal'] = same
    print(json.dumps(res))


if __name__ == '__main__':
    main()
