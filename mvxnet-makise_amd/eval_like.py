"""KITTI object evaluation of result files: AP for 2D bbox, BEV and 3D plus AOS (easy / moderate / hard, R11 and R40),
computed on the GPU by modules/kitti_eval.py (csrc/kitti_eval.hip).

    python eval_like.py <dataroot> --results <dataroot>/results/data [--split val] [--classes Car Pedestrian] [--json]

Labels are read from <dataroot>/training/label_2, the frame names from ImageSets/<split>.txt; a missing result file is an
error.  Prints the familiar table and one JSON line with the AP values and the time of file parsing and of the device
stages (hipEvents) separately.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('dataroot')
    ap.add_argument('--results', required=True, help='directory of KITTI result files, one <name>.txt per frame')
    ap.add_argument('--split', default='val', help='ImageSets/<split>.txt')
    ap.add_argument('--classes', nargs='+', default=['Car'])
    ap.add_argument('--json', action='store_true', help='print only the JSON line')
    return ap.parse_args(argv)


def run(dataroot, results, names, classes, quiet=False):
    """Evaluate ``results`` against the split's labels; prints the table (unless ``quiet``) and returns the JSON record."""
    from modules import Extension as X
    from modules import kitti_eval as ke
    dev = X.device()
    t0 = time.perf_counter()
    gt, dt = ke.read_dirs(os.path.join(dataroot, 'training', 'label_2'), results, names)
    t_parse = time.perf_counter() - t0
    events = []
    res = ke.evaluate(gt, dt, tuple(classes), dev, events)
    torch.cuda.synchronize(dev)
    stages = [events[k].elapsed_time(events[k + 1]) for k in range(len(events) - 1)]
    if not quiet:
        print(ke.format_table(res))
    return dict(frames=len(names), classes=list(classes), parse_s=round(t_parse, 4), device_ms=round(sum(stages), 3),
                stage_ms=dict(zip(('overlaps', 'tp_scores+sort', 'thresholds', 'counts'), [round(s, 3) for s in stages])),
                ap=ke.summary(res))


def main(args):
    with open(os.path.join(args.dataroot, 'ImageSets', args.split + '.txt'), 'r') as f:
        names = [n for n in f.read().splitlines() if n]
    rec = run(args.dataroot, args.results, names, args.classes, quiet=args.json)
    print(json.dumps(rec))


if __name__ == '__main__':
    a = parse_args()
    sys.argv = sys.argv[:1]              # modules.config parses argv at import (reference modules/config/Parser.py:12)
    main(a)
