"""CPU-only checks of the detection output (csrc/detect.hip, modules/detect.py): the C ABI's size query and its argument
checks before any launch, and the KITTI box export (camera-frame conversion, result files read back by the loader)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch


def test_detect_symbols_and_workspace_query():
    from modules import Extension as X
    from modules import detect  # noqa: F401  (importable without a GPU)
    assert X.ABI_VERSION == 10 and X.lib.mvx_abi_version() == 10
    lib = ctypes.CDLL(X.LIB_PATH)
    for name in ('mvx_detect_workspace_bytes', 'mvx_detect_frames'):
        assert hasattr(lib, name) and name in X.PROTOTYPES
    one = X.lib.mvx_detect_workspace_bytes(1, 70400, 1000)
    four = X.lib.mvx_detect_workspace_bytes(4, 70400, 1000)
    assert one > 1000 * 16 * 8 + 70400 * 4          # mask rows + the key array at least
    assert four > 3 * one
    assert X.lib.mvx_detect_workspace_bytes(16, 70400, 4096) > X.lib.mvx_detect_workspace_bytes(16, 70400, 1000)


def _call(**over):
    """mvx_detect_frames with plausible arguments (fake, never dereferenced device addresses: every case here must be
    refused by the host-side checks before anything is launched)."""
    from modules import Extension as X
    fake = ctypes.c_void_p(1 << 20)
    a = dict(cls=fake, reg=fake, anchors=fake, n_frames=4, l=176, w=200, A=2, score_thr=0.05, iou_thr=0.01, pre_max=1000,
             post_max=100, decode=0, boxes=fake, scores=fake, idx=fake, counts=fake, ncand=fake, status=fake, ws=fake,
             ws_bytes=1 << 40)
    a.update(over)
    return X.lib.mvx_detect_frames(a['cls'], 3520 * 16, 3200, 16, 1, a['reg'], 3520 * 16, 3200, 16, 1, a['anchors'], a['n_frames'],
                                   a['l'], a['w'], a['A'], a['score_thr'], a['iou_thr'], a['pre_max'], a['post_max'], a['decode'],
                                   a['boxes'], a['scores'], a['idx'], a['counts'], a['ncand'], a['status'], None, None, None,
                                   a['ws'], a['ws_bytes'], None)


@pytest.mark.parametrize('over', [
    dict(pre_max=4097), dict(pre_max=0), dict(post_max=1001), dict(post_max=0), dict(iou_thr=0.0), dict(iou_thr=1.0),
    dict(iou_thr=5e-4), dict(score_thr=1.0), dict(score_thr=-0.1), dict(n_frames=0), dict(n_frames=17), dict(boxes=None),
    dict(scores=None), dict(idx=None), dict(counts=None), dict(ncand=None), dict(status=None), dict(cls=None),
    dict(anchors=None), dict(ws=None), dict(decode=2), dict(ws_bytes=1024),
], ids=lambda o: '-'.join('%s=%s' % kv for kv in o.items()))
def test_detect_frames_rejects_bad_arguments_before_any_launch(over):
    assert _call(**over) == -1


def _calib():
    from modules.data import Synthetic as S
    return {k: torch.Tensor(np.asarray(v)) for k, v in S.KITTI_CALIB.items()}


def test_boxes_lidar_to_camera_inverts_bboxCam2Lidar():
    from modules import Calc
    from modules.detect import boxes_lidar_to_camera
    calib = _calib()                                    # the loader's layout: 4x4 float32 tensors
    g = np.random.default_rng(5)
    n = 64
    boxes = torch.tensor(np.stack([g.uniform(0, 70, n), g.uniform(-40, 40, n), g.uniform(-3, 1, n), g.uniform(3, 5, n),
                                   g.uniform(1.4, 2, n), g.uniform(1.3, 1.9, n), g.uniform(-math.pi, math.pi, n)], 1),
                         dtype=torch.float32)
    cam = boxes_lidar_to_camera(boxes, calib)
    c2v = torch.linalg.inv(calib['Tr_velo_to_cam'])
    back = Calc.bboxCam2Lidar(cam.float(), c2v)
    assert torch.allclose(back, boxes, atol=1e-5, rtol=0), float((back - boxes).abs().max())


def test_write_kitti_results_reads_back_through_the_loader(tmp_path):
    import modules.config as cfg
    from modules.data import Load, Synthetic as S
    from modules.detect import kitti_lines, write_kitti_results
    names = S.write_kitti_tree(str(tmp_path), [0, 1], points=500, raw_points=1000)
    g = np.random.default_rng(9)
    label_dir = os.path.join(str(tmp_path), 'training', 'label_2')
    sent = {}
    for k, name in enumerate(names):
        n = 5 - 2 * k                                   # 5 boxes, then 3
        boxes = torch.tensor(np.stack([g.uniform(5, 65, n), g.uniform(-35, 35, n), g.uniform(-2.5, 0.5, n), g.uniform(3, 5, n),
                                       g.uniform(1.4, 2, n), g.uniform(1.3, 1.9, n), g.uniform(-3, 3, n)], 1), dtype=torch.float32)
        scores = torch.tensor(g.uniform(0.05, 1, n), dtype=torch.float32)
        calib = Load.readCalib(os.path.join(str(tmp_path), 'training', 'calib', name + '.txt'))
        calib = {kk: torch.Tensor(v) for kk, v in calib.items()}
        write_kitti_results(os.path.join(label_dir, name + '.txt'), {'boxes': boxes, 'scores': scores}, calib, cfg.imsize)
        sent[name] = (boxes, scores)
        for line in kitti_lines({'boxes': boxes, 'scores': scores}, calib, cfg.imsize):
            tok = line.split(' ')
            assert tok[:3] == ['Car', '-1', '-1'] and len(tok) == 16
            x1, y1, x2, y2 = [float(v) for v in tok[4:8]]
            assert 0 <= x1 <= x2 <= cfg.imsize[1] - 1 and 0 <= y1 <= y2 <= cfg.imsize[0] - 1
            h, w, l, x, y, z, ry = [float(v) for v in tok[8:15]]
            assert abs(float(tok[3]) - (ry - math.atan2(x, z))) < 0.02
    data = Load.createDataset(names, root=str(tmp_path))
    for name, d in zip(names, data):
        boxes, scores = sent[name]
        got = d[3]
        assert got is not None and got.shape == boxes.shape
        # the format's 2 decimals (h w l x y z ry), then the reader's f32 rotation back into the LiDAR frame
        assert torch.allclose(got, boxes, atol=1.2e-2, rtol=0), float((got - boxes).abs().max())
    open(os.path.join(label_dir, names[0] + '.txt'), 'w').close()
    write_kitti_results(os.path.join(label_dir, names[0] + '.txt'), {'boxes': torch.zeros((0, 7)), 'scores': torch.zeros((0,))},
                        _calib(), cfg.imsize)
    assert open(os.path.join(label_dir, names[0] + '.txt')).read() == ''
