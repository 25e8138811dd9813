"""The reference's OWN compiled extension as the checker.

``tests/golden/ref_*.npz`` hold what the reference's cpp/voxelutil.cpp, compiled as it is by ``oracle/Makefile`` (plain g++ with
the real pybind11 headers), returned for the inputs below (``oracle/gen_ref_binary_golden.py``; nothing of the reference's SOURCE
is in the repository).  They stand beside the other committed fixtures:

  * CPU (-m "not gpu"): the plain-C restatement of the oracle (oracle/group_c.c, oracle/anchors_c.c) against the real `_group`,
    `_classifyAnchors` at the benchmark's size -- the restatement is pinned by the reference's
    binary, not only by the small fixtures made from it;
  * GPU (-m gpu): the HIP library behind the same pybind signatures (modules.Extension.cpp) against the same binary."""
import numpy as np
import pytest

import mvx_oracle as O


def _group_ref(golden, kind, fid):
    """(points, indices) of the frame and the binary's `_group(points, indices, 35)` as (voxel, (x, y, z), cnt)."""
    s, idx = O.ref_binary_frame(kind, fid)
    g = golden('ref_group_%s_%d' % (kind, fid))
    assert O.array_digest(s, idx) == str(g['input_sha256']), 'the synthetic frame is not the one the fixture was made from'
    return s, idx, (g['voxel'], (g['x'], g['y'], g['z']), g['cnt'])


def _targets_ref(golden, seed):
    """(gt boxes, the binary's `_classifyAnchors` as ((px, py, pz), (nx, ny, nz), gi)) for one seed."""
    g = golden('ref_classify_anchors')
    gt = O.ref_binary_boxes(seed)
    assert np.array_equal(gt.numpy(), g['gt%d' % seed]), 'the boxes are not the ones the fixture was made from'
    return gt, (tuple(g['p%d_%d' % (seed, k)] for k in range(3)), tuple(g['n%d_%d' % (seed, k)] for k in range(3)),
                g['g%d' % seed])


@pytest.mark.parametrize('kind', ['uniform', 'ring'])
def test_c_oracle_voxelizer_equals_the_reference_binary_at_full_size(golden, kind):
    """oracle/group_c.c (through mvx_oracle.group) == cpp/voxelutil.cpp `_group` on a 20,000-point frame: voxel order, counts
    and the xyz / reflectance payload, bit for bit (voxelutil.cpp:325-360 fills columns 0:3 and 6)."""
    s, idx, (voxel, (x, y, z), cnt) = _group_ref(golden, kind, 3)
    pcd6 = np.concatenate([s, np.zeros((s.shape[0], 2), np.float32)], 1)
    v9, ui, c = O.group(pcd6, np.arange(s.shape[0], dtype=np.int32), O.VELORANGE, O.voxelsize(), 35)
    assert np.array_equal(np.stack([x, y, z], 1), ui.astype(np.int64))
    assert np.array_equal(cnt, c)
    assert np.array_equal(voxel[..., :3], v9[..., :3].astype(np.float32)) and np.array_equal(voxel[..., 6], v9[..., 6].astype(np.float32))
    assert not voxel[..., 3:6].any()


def test_c_oracle_targets_equal_the_reference_binary(golden):
    """oracle/anchors_c.c == the reference binary's bboxOverlap / bboxIntersection / _classifyAnchors on random car boxes over the
    full 176 x 200 x 2 anchor grid."""
    anchors = O.create_anchors(176, 200)
    bevs = O.bbox3d2bev(anchors.reshape(176, 200, 2, 7))
    for seed in (0, 1, 2):
        gt, (rp, rn, rg) = _targets_ref(golden, seed)
        pi, ni, gi = O.classify_anchors(O.bbox3d2bev(gt), gt[:, :2], bevs, O.VELORANGE, 0.45, 0.6)
        for got, want in zip(list(pi) + list(ni) + [gi], list(rp) + list(rn) + [rg]):
            assert np.array_equal(np.asarray(got), np.asarray(want))
    # bboxOverlap / bboxIntersection of the binary are NOT compared: the reference fills r2[j] where r2[k] is meant
    # (voxelutil.cpp:107-109,128-130), so box 2 is read from stale static scratch and the result is
    # undefined; its IoU arithmetic is pinned through _classifyAnchors above and tests/test_targets_oracle.py


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['uniform', 'ring'])
def test_hip_group_equals_the_reference_binary_at_full_size(golden, kind):
    """modules.Extension.cpp._group (HIP voxelizer behind the pybind signature) == the reference binary, 20,000 points."""
    from modules.Extension import cpp
    s, idx, (rv, (rx, ry, rz), rc) = _group_ref(golden, kind, 4)
    voxel, (x, y, z), cnt = cpp._group(s, idx, 35)
    assert np.array_equal(x, rx) and np.array_equal(y, ry) and np.array_equal(z, rz) and np.array_equal(cnt, rc)
    assert voxel.dtype == rv.dtype and np.array_equal(voxel, rv)


@pytest.mark.gpu
def test_hip_targets_equal_the_reference_binary(golden):
    from modules.Extension import cpp
    anchors = O.create_anchors(176, 200)
    bevs = O.bbox3d2bev(anchors.reshape(176, 200, 2, 7))
    for seed in (0, 1):
        gt, want = _targets_ref(golden, seed)
        bev = O.bbox3d2bev(gt).numpy()
        nls, nws = O.anchor_center_cells(gt[:, :2], bevs.shape, O.VELORANGE)
        got = cpp._classifyAnchors(bev, bevs.numpy(), nls.numpy(), nws.numpy(), 0.45, 0.6)
        for a, b in zip(list(got[0]) + list(got[1]) + [got[2]], list(want[0]) + list(want[1]) + [want[2]]):
            assert np.array_equal(a, b)
