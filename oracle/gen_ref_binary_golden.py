"""tests/golden/ref_*.npz: what the reference's own compiled extension returns for the inputs of
tests/test_ref_extension.py.  TEST INFRASTRUCTURE ONLY.

Needs ``oracle/_ref/voxelutil*.so`` (``make -C oracle ref`` with the reference tree present); only the
resulting data files are committed.

  ref_group_<kind>_<fid>.npz   `_group(points, indices, 35)` of a 20,000-point synthetic frame: voxel, x, y, z,
                               cnt, and the SHA-256 of the inputs (mvx_oracle.ref_binary_frame)
  ref_classify_anchors.npz     `_classifyAnchors` over the full 176 x 200 x 2 anchor grid for random car boxes:
                               per seed the boxes (gt<seed>), the positive / negative index triples (p<seed>_<k>,
                               n<seed>_<k>) and the ground-truth ids (g<seed>)

Usage:  python oracle/gen_ref_binary_golden.py
"""
import glob
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), 'tests', 'golden')
sys.path.insert(0, HERE)
import mvx_oracle as O  # noqa: E402

GROUP_FRAMES = [('uniform', 3), ('ring', 3), ('uniform', 4), ('ring', 4)]
ANCHOR_SEEDS = (0, 1, 2)


def load_binary():
    so = glob.glob(os.path.join(HERE, '_ref', 'voxelutil*.so'))
    assert so, 'run `make -C oracle ref` first'
    spec = importlib.util.spec_from_file_location('voxelutil', so[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def save(name, **arrs):
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **arrs)
    print('%-28s %8.1f KB' % (name, os.path.getsize(path) / 1024))


def main():
    ref = load_binary()
    for kind, fid in GROUP_FRAMES:
        s, idx = O.ref_binary_frame(kind, fid)
        voxel, (x, y, z), cnt = ref._group(s, idx, 35)
        save('ref_group_%s_%d' % (kind, fid), voxel=voxel, x=x, y=y, z=z, cnt=cnt,
             input_sha256=np.array(O.array_digest(s, idx)))

    anchors = O.create_anchors(176, 200)
    bevs = O.bbox3d2bev(anchors.reshape(176, 200, 2, 7))
    arrs = {}
    for seed in ANCHOR_SEEDS:
        gt = O.ref_binary_boxes(seed)
        bev = O.bbox3d2bev(gt).numpy()
        nls, nws = O.anchor_center_cells(gt[:, :2], bevs.shape, O.VELORANGE)
        rp, rn, rg = ref._classifyAnchors(bev, bevs.numpy(), nls.numpy(), nws.numpy(), 0.45, 0.6)
        arrs['gt%d' % seed] = gt.numpy()
        for k in range(3):
            arrs['p%d_%d' % (seed, k)] = np.asarray(rp[k])
            arrs['n%d_%d' % (seed, k)] = np.asarray(rn[k])
        arrs['g%d' % seed] = np.asarray(rg)
    save('ref_classify_anchors', **arrs)


if __name__ == '__main__':
    main()
