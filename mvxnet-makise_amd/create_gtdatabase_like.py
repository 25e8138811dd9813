"""The reference's database builder (create_gtdatabase.py) on this package's kernels: for every frame of the KINS annotation
file that is in ``ImageSets/train.txt`` match the label boxes to the instance annotations, rasterise the instances' polygons
and cut the points inside every 3-D box (csrc/gtdb.hip), then write ``training/gtdatabase/<Class>/{velo,img,mask}_%06d.*``
and ``gtinfo.pkl`` in the reference's layout -- what ``modules.augment.LoadGT.getAllGT`` and ``train_like.py --augment`` read.

    python create_gtdatabase_like.py <dataroot> [--seg PATH] [--classes Car Pedestrian Cyclist] [--batch N] [--synthetic N]

``--seg`` defaults to ``<dataroot>/seglabel/update_train_2020.json``.  ``--synthetic N`` first writes a synthetic KITTI tree of
N frames with a matching annotation file (modules/data/Synthetic.write_kins_tree).  Needs json, PIL and numpy only.
"""
import argparse
import os
import pickle
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def build_tree(dataroot, seg, classes, batch=8, device=None, quiet=True):
    """Builds and writes the database; returns ({cls: infos}, {cls: objects without points})."""
    from modules.augment import BuildGT
    with open(os.path.join(dataroot, 'ImageSets/train.txt'), 'r') as f:
        train = set(f.read().splitlines())
    ann = BuildGT.readAnnotations(seg)
    order = BuildGT.frameOrder(ann, train)
    gtinfo = {c: [] for c in BuildGT.CLASSES}                       # all three keys, always (create_gtdatabase.py:89-93)
    counters = {c: 0 for c in classes}
    empty = {c: 0 for c in classes}
    for lo in range(0, len(order), batch):
        part = order[lo:lo + batch]
        frames = [BuildGT.loadFrame(dataroot, name, classes) for _, name in part]
        built = BuildGT.buildFrames(frames, [ann.by_image[i] for i, _ in part], classes, device=device, counters=counters)
        for c in classes:
            gtinfo[c] += built[c]['infos']
            BuildGT.writeObjects(dataroot, c, built[c])
            pt = built[c]['tables']['pt_off'].cpu().numpy()
            empty[c] += int((pt[1:] == pt[:-1]).sum())
        if not quiet:
            print('\rCreating ground truth database: %d/%d' % (min(lo + batch, len(order)), len(order)), end='')
    for c in BuildGT.CLASSES:
        os.makedirs(os.path.join(dataroot, 'training/gtdatabase', c), exist_ok=True)
    with open(os.path.join(dataroot, 'training/gtdatabase/gtinfo.pkl'), 'wb') as f:
        pickle.dump(gtinfo, f)
    return gtinfo, empty


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('dataroot')
    ap.add_argument('--seg', default=None, help='the KINS annotation file')
    ap.add_argument('--classes', nargs='+', default=['Car', 'Pedestrian', 'Cyclist'], choices=['Car', 'Pedestrian', 'Cyclist'])
    ap.add_argument('--batch', type=int, default=8, help='frames per kernel pass')
    ap.add_argument('--synthetic', type=int, default=0, help='write a synthetic tree and annotation file of this many frames first')
    ap.add_argument('--quiet', action='store_true')
    a = ap.parse_args(argv)
    sys.argv = sys.argv[:1]              # modules.config parses argv at import (reference modules/config/Parser.py:12)
    seg = a.seg if a.seg else os.path.join(a.dataroot, 'seglabel/update_train_2020.json')
    if a.synthetic:
        from modules.data import Synthetic
        Synthetic.write_kins_tree(a.dataroot, list(range(a.synthetic)), seg_path=seg)
    t0 = time.perf_counter()
    gtinfo, empty = build_tree(a.dataroot, seg, list(a.classes), max(1, a.batch), quiet=a.quiet)
    if not a.quiet:
        print()
    for c in a.classes:
        print('%s: %d objects, %d without points' % (c, len(gtinfo[c]), empty[c]))
    print('%.2f s' % (time.perf_counter() - t0))
    return 0


if __name__ == '__main__':
    sys.exit(main())
