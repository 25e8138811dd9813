"""CPU-only checks of the renderer: the segment rule of the reference (tests/render_ref.py), the draw list and the colour
words on CPU tensors, the tables, the PNG writer, the argument checks of the two entry points before any launch, the command
line of visualize_like.py, and that the seeded rejection of tests/render_cases.py reaches its box counts."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import abi_header
import render_cases as C
import render_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _segments(seed=0, n=300):
    g = np.random.default_rng(seed)
    segs = [tuple(int(v) for v in g.integers(-40, 40, 4)) for _ in range(n)]
    segs += [(0, 0, 0, 0), (3, -2, 3, 9), (-5, 4, 6, 4), (1, 1, 8, 8), (2, 9, 9, 2), (0, 0, 1, 100000), (-70000, 5, 90000, -3)]
    return segs


def test_segment_rule_properties():
    for r0, c0, r1, c1 in _segments():
        px = R.segment_pixels(r0, c0, r1, c1)
        n = max(abs(r1 - r0), abs(c1 - c0))
        assert len(px) == n + 1 and len(set(px)) == n + 1
        assert (r0, c0) in (px[0], px[-1]) and (r1, c1) in (px[0], px[-1])
        for a, b in zip(px, px[1:]):
            assert abs(a[0] - b[0]) <= 1 and abs(a[1] - b[1]) <= 1
        assert px == R.segment_pixels(r1, c1, r0, c0)                 # (A, B) and (B, A): the same pixels in the same order


def test_segment_rule_is_exact_on_axes_and_diagonals():
    assert R.segment_pixels(3, -2, 3, 4) == [(3, c) for c in range(-2, 5)]
    assert R.segment_pixels(6, 4, -1, 4) == [(r, 4) for r in range(-1, 7)]
    assert R.segment_pixels(1, 1, 5, 5) == [(k, k) for k in range(1, 6)]
    assert R.segment_pixels(2, 9, 9, 2) == [(2 + k, 9 - k) for k in range(8)]
    assert R.segment_pixels(7, 7, 7, 7) == [(7, 7)]
    # ties round half up along the sign of the minor step: (0,0)-(2,1) passes (1, 1), and so does its mirror image
    assert R.segment_pixels(0, 0, 2, 1) == [(0, 0), (1, 1), (2, 1)]
    assert R.segment_pixels(0, 0, 2, -1) == [(0, 0), (1, -1), (2, -1)]


def test_clipped_drawing_equals_the_unclipped_pixels_inside_the_image():
    H, W = 23, 31
    for T in (1, 2, 3):
        for r0, c0, r1, c1 in _segments(seed=T, n=120):
            plane = np.zeros((H, W), np.int64)
            R.draw_segment(plane, r0, c0, r1, c1, T, 7)
            want = np.zeros((H, W), np.int64)
            for r, c in R.segment_pixels(r0, c0, r1, c1):
                if 0 <= r < H and 0 <= c < W:
                    for dr in range(-(T // 2), T - (T // 2)):
                        for dc in range(-(T // 2), T - (T // 2)):
                            if 0 <= r + dr < H and 0 <= c + dc < W:
                                want[r + dr, c + dc] = 7
            assert np.array_equal(plane, want), (T, r0, c0, r1, c1)
    klo, khi = R.clipped_k_range(5, -100000, 7, 100000, H, W)[:2]
    assert khi - klo + 1 == W                                         # 10^5 px off-screen: max(H, W) steps at most


def test_pack_colors_words():
    from modules import render
    w = render.pack_colors(torch.tensor([1, 2, 127, 128, 255]), torch.tensor([[0, 255, 0], [255, 0, 0], [1, 2, 3], [4, 5, 6], [255, 255, 255]]))
    assert w.dtype == torch.int32
    assert (w.numpy().view(np.uint32).tolist() ==
            [0x0100FF00, 0x02FF0000, 0x7F010203, 0x80040506, 0xFFFFFFFF])
    assert int(render.pack_colors(1, (0, 255, 0))) == 0x0100FF00
    with pytest.raises(ValueError):
        render.pack_colors(256, (0, 0, 0))
    with pytest.raises(ValueError):
        render.pack_colors(1, (0, 0, 300))


def _words(colors):
    return colors.numpy().view(np.uint32)


def test_draw_list_priorities_and_masking_on_cpu_tensors():
    from modules import render
    g = torch.Generator().manual_seed(0)
    gts = [torch.rand((2, 7), generator=g), None, torch.rand((1, 7), generator=g)]
    scores = torch.tensor([[0.0, 0.5, 1.0, 0.999, 7.0], [0.3, 0.2, 0.1, 0.0, 0.0], [0.9, 0.9, 0.9, 0.9, 0.9]])
    dev = dict(boxes=torch.rand((3, 5, 7), generator=g), scores=scores, anchor_idx=torch.zeros((3, 5), dtype=torch.int32),
               meta=torch.tensor([[5, 2, 0], [9, 9, 9], [0, 0, 0]], dtype=torch.int32))
    boxes, n_boxes, colors = render.draw_list(gts, dev)
    assert boxes.shape == (3, 7, 7) and colors.shape == (3, 7) and boxes.dtype == torch.float32 and colors.dtype == torch.int32
    assert n_boxes.dtype == torch.int32 and n_boxes.tolist() == [7, 2, 1]
    w = _words(colors)
    assert w[0, 0] == w[0, 1] == w[2, 0] == 0x0100FF00                 # GT: green, priority 1
    prio = lambda s: 2 + min(253, int(np.floor(np.float64(np.float32(s)) * 253)))
    for k, s in enumerate(scores[0].tolist()):
        v = prio(s) - 2
        assert w[0, 2 + k] == (prio(s) << 24) | (255 << 16) | ((v * 255 // 253) << 8), (k, s)
    assert (w[0, 2] >> 24, w[0, 4] >> 24, w[0, 6] >> 24) == (2, 255, 255) and w[0, 4] & 0xFFFFFF == 0xFFFF00
    assert torch.equal(boxes[0, :2], gts[0]) and torch.equal(boxes[0, 2:], dev['boxes'][0])
    # slots behind the count: zero boxes, zero words
    assert not w[1, 2:].any() and not boxes[1, 2:].any() and torch.equal(boxes[1, :2], dev['boxes'][1, :2])
    assert not w[2, 1:].any() and not boxes[2, 1:].any()
    # the same list from unpacked per-frame dicts, padded to the same capacity
    counts = dev['meta'][0].tolist()
    lists = [dict(boxes=dev['boxes'][f, :n], scores=dev['scores'][f, :n]) for f, n in enumerate(counts)]
    b2, n2, c2 = render.draw_list(gts, lists, cap=7)
    assert torch.equal(b2, boxes) and torch.equal(n2, n_boxes) and torch.equal(c2, colors)
    b3, n3, c3 = render.draw_list(gts, None)
    assert b3.shape == (3, 2, 7) and n3.tolist() == [2, 0, 1] and not _words(c3)[1].any()
    with pytest.raises(ValueError):
        render.draw_list(gts, lists, cap=3)


def test_default_luts_and_detection_colors():
    from modules import render
    luts = render.default_luts()
    assert sorted(luts) == ['depth', 'height', 'intensity']
    for t in luts.values():
        assert t.shape == (256, 3) and t.dtype == torch.uint8
    assert luts['height'][0].tolist() == [0, 0, 255] and luts['height'][255].tolist() == [255, 3, 0]
    assert luts['height'][128].tolist() == [0, 255, 0] and luts['depth'][0].tolist() == luts['height'][255].tolist()
    assert luts['intensity'][0].tolist() == [48] * 3 and luts['intensity'][255].tolist() == [255] * 3
    d = render.detection_colors()
    assert d.shape == (254, 3) and d[0].tolist() == [255, 0, 0] and d[253].tolist() == [255, 255, 0]
    assert render.bev_shape(0.1) == (704, 800)


def test_save_png_round_trip(tmp_path):
    from PIL import Image
    from modules import render
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (13, 17, 3), dtype=np.uint8))
    path = str(tmp_path / 'a.png')
    render.save_png(path, img)
    with Image.open(path) as im:
        assert im.mode == 'RGB' and im.size == (17, 13)
        assert np.array_equal(np.asarray(im), img.numpy())
    with pytest.raises(ValueError):
        render.save_png(path, img[..., 0])
    paths = render.save_frames(str(tmp_path / 'out'), ['000000', '000001'], bev=torch.stack([img, img]), cam=None)
    assert [os.path.basename(p) for p in paths] == ['000000_bev.png', '000001_bev.png'] and all(os.path.exists(p) for p in paths)


# one bad argument each -> MVX_EINVAL; a parameter an entry point does not have is skipped for it
RENDER_BAD_ARGUMENTS = (
    ('points6', None), ('n_points', None), ('boxes', None), ('n_boxes', None), ('colors', None), ('lut', None), ('lut_depth', None),
    ('image_from_lidar', None), ('out', None), ('status', None), ('workspace', None),
    ('n_frames', 0), ('n_frames', 17), ('h', 0), ('h', 4097), ('w', 0), ('w', 4097), ('res', 0.0), ('res', -0.1), ('z1', -3.0),
    ('z1', -4.0), ('cmax', 0), ('thickness', 0), ('thickness', 4), ('point_radius', -1), ('point_radius', 3),
    ('workspace_bytes', 1024), ('ld', 5), ('cap_points', 0), ('z_near', 0.0), ('depth_max', 0.0), ('color_by', 2))


def test_render_entry_points_reject_bad_arguments_before_any_launch():
    """16-byte-aligned dummy pointers and ONE bad argument: the call comes back with MVX_EINVAL -- a launch on these host
    pointers would fault, and without a GPU the memset in front of it would return a HIP error instead."""
    from modules import Extension as X
    buf = ctypes.create_string_buffer(4096 + 64)
    dummy = (ctypes.addressof(buf) + 63) & ~63
    good = dict(ld=6, n_frames=2, cap_points=100, cap_boxes=4, x0=0.0, y0=-40.0, res=0.1, z0=-3.0, z1=1.0, h=37, w=45, color_by=0,
                cmax=8, background=0, thickness=1, z_near=0.5, depth_max=70.4, point_radius=1, image_is_bgr=1,
                workspace_bytes=1 << 40, stream=None)
    assert X.lib.mvx_render_workspace_bytes(2, 37, 45) >= 3 * 2 * 37 * 45 * 4
    for bad in ((0, 37, 45), (17, 37, 45), (2, 0, 45), (2, 37, 4097)):
        assert X.lib.mvx_render_workspace_bytes(*bad) == 0
    calls = 0
    for name in ('mvx_render_bev_frames', 'mvx_render_camera_frames'):
        names = abi_header.parameter_names(name)
        assert len(names) == len(X.PROTOTYPES[name][1])
        for param, value in RENDER_BAD_ARGUMENTS:
            if param not in names:
                continue
            args = [value if q == param else good[q] if q in good else dummy for q in names]
            assert getattr(X.lib, name)(*args) == -1, (name, param, value)
            calls += 1
    assert calls == 26 + 25
    # without boxes the three box pointers may be null: the check that fails is the (too small) workspace, not them
    names = abi_header.parameter_names('mvx_render_bev_frames')
    args = [None if q in ('boxes', 'n_boxes', 'colors') else 0 if q == 'cap_boxes' else 16 if q == 'workspace_bytes' else
            good[q] if q in good else dummy for q in names]
    assert X.lib.mvx_render_bev_frames(*args) == -1


def test_wrapper_constants_match_the_header():
    import re
    from modules import _hip
    header = open(os.path.join(REPO, 'include', 'mvx_hip.h')).read()
    for name, val in (('MVX_RENDER_MAX_SIDE', _hip.RENDER_MAX_SIDE), ('MVX_RENDER_BAD_BOX', _hip.RENDER_BAD_BOX),
                      ('MVX_RENDER_BY_HEIGHT', _hip.RENDER_COLOR_BY['height']), ('MVX_RENDER_BY_INTENSITY', _hip.RENDER_COLOR_BY['intensity'])):
        assert int(re.search(r'#define %s (\d+)' % name, header).group(1)) == val, name
    assert R.BAD_BOX == _hip.RENDER_BAD_BOX


def test_visualize_like_parse_args():
    import visualize_like as V
    a = V.parse_args(['/data/kitti'])
    assert (a.dataroot, a.results, a.checkpoint, a.split, a.out, a.view, a.frames, a.res, a.thickness, a.synthetic) == \
        ('/data/kitti', None, None, 'train', None, 'both', 0, 0.1, 1, 0)
    a = V.parse_args(['/d', '--results', 'r', '--checkpoint', 'c.pkl', '--split', 'val', '--out', 'o', '--view', 'bev', '--frames', '5',
                      '--res', '0.2', '--thickness', '3', '--synthetic', '2'])
    assert (a.results, a.checkpoint, a.split, a.out, a.view, a.frames, a.res, a.thickness, a.synthetic) == \
        ('r', 'c.pkl', 'val', 'o', 'bev', 5, 0.2, 3, 2)
    for bad in (['/d', '--view', 'side'], ['/d', '--thickness', '4'], []):
        with pytest.raises(SystemExit):
            V.parse_args(bad)
    import detect_like as D
    assert D.parse_args(['/d']).render is None and D.parse_args(['/d', '--render', 'pics']).render == 'pics'


def test_read_result_boxes_inverts_the_result_writer(tmp_path):
    import modules.config as cfg
    import visualize_like as V
    from modules.data import Synthetic as S
    from modules.detect import write_kitti_results
    calib = {k: torch.as_tensor(v, dtype=torch.float32) for k, v in S.KITTI_CALIB.items()}
    dets = dict(boxes=torch.tensor([[12.0, 1.5, -1.6, 4.1, 1.7, 1.5, 0.3], [30.0, -4.0, -1.4, 3.8, 1.6, 1.6, -1.2]]),
                scores=torch.tensor([0.9, 0.25]))
    path = str(tmp_path / 'r.txt')
    write_kitti_results(path, dets, calib, cfg.imsize)
    got = V.read_result_boxes(path, calib)
    assert got['boxes'].shape == (2, 7) and torch.allclose(got['boxes'], dets['boxes'], atol=2e-2)        # two decimals in the file
    assert torch.allclose(got['scores'], dets['scores'], atol=1e-4)
    empty = V.read_result_boxes(str(tmp_path / 'missing.txt'), calib)
    assert empty['boxes'].shape == (0, 7) and empty['scores'].shape == (0,)


def test_case_generators_reach_their_box_counts():
    """The seeded rejection finds every box (a draw fails with probability ~ 4e-5), the final sets keep the margin, and the
    planted situations are really there: a corner behind z_near, a box wholly behind, a projection beyond 10^5 px."""
    b = C.bev_case()
    assert len(b['tries']) == 7 and max(b['tries']) <= 3
    assert b['boxes'].shape == (3, 9, 7) and b['n_boxes'].tolist() == [0, 1, 7] and b['n_points'].tolist() == [0, 1, 300]
    assert np.isnan(b['boxes'][2, 6]).any() and np.isfinite(b['boxes'][2, :6]).all()
    for f in range(3):
        for k in range(b['n_boxes'][f]):
            if np.isfinite(b['boxes'][f, k]).all():
                assert C.margin_ok(R.bev_endpoints(b['boxes'][f, k], b['x0'], b['y0'], b['res']))
    cells = lambda k: [(np.floor(e[0]), np.floor(e[1])) for sg in R.bev_endpoints(b['boxes'][2, k], b['x0'], b['y0'], b['res']) for e in sg]
    inside = lambda ij: 0 <= ij[0] < b['H'] and 0 <= ij[1] < b['W']
    assert not any(inside(ij) for ij in cells(0))                      # wholly outside
    assert any(inside(ij) for ij in cells(1)) and not all(inside(ij) for ij in cells(1))
    assert len(set(cells(2))) == 1                                     # zero size: one pixel
    c = C.camera_case()
    assert len(c['tries']) == 6 and max(c['tries']) <= 3 and c['n_boxes'].tolist() == [4, 2]
    segs = [R.camera_endpoints(c['boxes'][0, k], c['mats'][0], c['z_near']) for k in range(4)]
    assert len(segs[0]) == 14 and 0 < len(segs[1]) <= 14 and len(segs[2]) == 0 and len(segs[3]) >= 1
    m = c['mats'][0]
    w_of = lambda box: [float(m[2] @ np.append(p, 1.0)) for p in _corners(box)]
    assert 0 < sum(w < c['z_near'] for w in w_of(c['boxes'][0, 1])) < 8
    far = max(abs(v) for sg in segs[3] for e in sg for v in e)
    assert 1e5 < far < 2 ** 24
    for f in range(2):
        for k in range(c['n_boxes'][f]):
            assert C.margin_ok(R.camera_endpoints(c['boxes'][f, k], c['mats'][f], c['z_near']))


def _corners(box):
    from modules import Calc
    return Calc.bbox3d2corner(torch.as_tensor(np.asarray(box, dtype=np.float64))[None])[0].numpy()
