"""Frame rendering on the GPU (csrc/render.hip, modules/render.py) against the numpy restatement tests/render_ref.py: every
comparison is torch.equal on the u8 image and on the status words -- no tolerance.  The inputs are the seeded cases of
tests/render_cases.py (boxes built by rejection: every pre-floor endpoint coordinate at least 1e-6 px from an integer,
asserted on the final set)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_cases as C
import render_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GT_GREEN = (0, 255, 0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _draw(c):
    return _dev(c['boxes']), _dev(c['n_boxes']), _dev(C.as_i32(c['colors']))


@pytest.fixture(scope='module')
def bev():
    c = C.bev_case()
    for f in range(3):                                                  # asserted on the final set: nothing excluded afterwards
        for k in range(c['n_boxes'][f]):
            if np.isfinite(c['boxes'][f, k]).all():
                assert C.margin_ok(R.bev_endpoints(c['boxes'][f, k], c['x0'], c['y0'], c['res'])), (f, k)
    return c


@pytest.fixture(scope='module')
def camera():
    c = C.camera_case()
    for f in range(2):
        for k in range(c['n_boxes'][f]):
            assert C.margin_ok(R.camera_endpoints(c['boxes'][f, k], c['mats'][f], c['z_near'])), (f, k)
    return c


def _bev_gpu(c, color_by, T, points6=None):
    from modules import _hip
    pts = _dev(c['points6'] if points6 is None else points6)
    return _hip.render_bev_frames(pts, _dev(c['n_points']), *_draw(c), c['x0'], c['y0'], c['res'], c['z0'], c['z1'], c['H'], c['W'],
                                  _dev(c['lut']), color_by, c['cmax'], c['background'], T)


def _bev_ref(c, color_by, T):
    return R.render_bev(c['points6'], c['n_points'], c['boxes'], c['n_boxes'], c['colors'], c['x0'], c['y0'], c['res'], c['z0'], c['z1'],
                        c['H'], c['W'], c['lut'], color_by, c['cmax'], c['background'], T)


@pytest.mark.parametrize('color_by,T', [('height', 1), ('intensity', 3), ('height', 2)])
def test_bev_equals_the_reference(bev, color_by, T):
    img, status = _bev_gpu(bev, color_by, T)
    want, want_status = _bev_ref(bev, color_by, T)
    assert img.shape == (3, 37, 45, 3) and img.dtype == torch.uint8
    assert torch.equal(status.cpu(), torch.from_numpy(want_status)) and want_status.tolist() == [0, 0, R.BAD_BOX]
    assert torch.equal(img.cpu(), torch.from_numpy(want))
    # what the case plants is really in the picture
    bg = torch.tensor([9, 17, 33], dtype=torch.uint8)
    assert (img[0].cpu() == bg).all()                                   # no point, no box: background only
    assert int((img[1].cpu() != bg).any(-1).sum()) > 4                  # one point (if in range) and one box
    H, W = bev['H'], bev['W']
    lut = bev['lut'].astype(np.int64)
    if T == 1:                                                          # thin lines leave the planted pixels free, or the box won them
        i, j = C.SATURATED_CELL
        px = want[2, H - 1 - i, W - 1 - j]
        ov_free = not _on_a_box(bev, T, 2, H - 1 - i, W - 1 - j)
        if ov_free and color_by == 'height':
            z = bev['points6'][2, 10:50, 2].astype(np.float64)
            zq = max(R.clampq((v - bev['z0']) / (bev['z1'] - bev['z0']) * 65535.0, 65535) for v in z)
            assert px.tolist() == [int(lut[zq >> 8, ch]) * 255 // 255 for ch in range(3)]        # count 40 >= cmax: full shade
    # the point on the lower bounds is drawn (bottom right pixel), the ones on the upper bounds are not
    if not _on_a_box(bev, T, 2, H - 1, W - 1):
        assert want[2, H - 1, W - 1].tolist() != [9, 17, 33]


def _on_a_box(c, T, f, r, col):
    """Does the reference's overlay of frame f cover pixel (r, col)?  (an image with black points and no LUT would do too)"""
    blank = np.zeros_like(c['points6'])
    img, _ = R.render_bev(blank, np.zeros_like(c['n_points']), c['boxes'], c['n_boxes'], c['colors'], c['x0'], c['y0'], c['res'],
                          c['z0'], c['z1'], c['H'], c['W'], c['lut'], 'height', c['cmax'], 0, T)
    return bool(img[f, r, col].any())


def test_bev_ties_and_order(bev):
    """Equal z, different r: the larger r colours the pixel by intensity; a higher point wins whatever its r."""
    H, W, lut = bev['H'], bev['W'], bev['lut'].astype(np.int64)
    img, _ = _bev_gpu(bev, 'intensity', 1)
    img = img.cpu().numpy()
    for (i, j), r_win in ((C.TIE_CELL, 0.7), (C.ORDER_CELL, 0.1)):
        if _on_a_box(bev, 1, 2, H - 1 - i, W - 1 - j):
            continue
        iq = R.clampq(float(np.float64(np.float32(r_win))) * 255.0, 255)
        shade = 64 + 191 * 2 // bev['cmax']
        assert img[2, H - 1 - i, W - 1 - j].tolist() == [int(lut[iq, ch]) * shade // 255 for ch in range(3)]


def test_bev_without_boxes_and_slots_behind_the_counts(bev):
    """No draw list at all; and with one, the garbage behind n_boxes / n_points changes nothing when it is replaced."""
    from modules import _hip
    pts, n = _dev(bev['points6']), _dev(bev['n_points'])
    args = (bev['x0'], bev['y0'], bev['res'], bev['z0'], bev['z1'], bev['H'], bev['W'], _dev(bev['lut']), 'height', bev['cmax'],
            bev['background'], 1)
    img0, st0 = _hip.render_bev_frames(pts, n, None, None, None, *args)
    want, _ = R.render_bev(bev['points6'], bev['n_points'], None, None, None, bev['x0'], bev['y0'], bev['res'], bev['z0'], bev['z1'],
                           bev['H'], bev['W'], bev['lut'], 'height', bev['cmax'], bev['background'], 1)
    assert torch.equal(img0.cpu(), torch.from_numpy(want)) and st0.tolist() == [0, 0, 0]
    other = dict(bev)
    other['boxes'], other['colors'], other['points6'] = bev['boxes'].copy(), bev['colors'].copy(), bev['points6'].copy()
    for f in range(3):
        other['boxes'][f, bev['n_boxes'][f]:] = 7.0
        other['colors'][f, bev['n_boxes'][f]:] = 0xFFFFFFFF
        other['points6'][f, bev['n_points'][f]:, :4] = (5.0, 1.0, 0.0, 0.5)
    a, sa = _bev_gpu(bev, 'height', 1)
    b, sb = _bev_gpu(other, 'height', 1)
    assert torch.equal(a, b) and torch.equal(sa, sb)


def _cam_gpu(c, R_pt, T, images, bgr, points6=None):
    from modules import _hip
    pts = _dev(c['points6'] if points6 is None else points6)
    return _hip.render_camera_frames(pts, _dev(c['n_points']), *_draw(c), _dev(c['mats']), c['H'], c['W'], _dev(c['lut']),
                                     z_near=c['z_near'], depth_max=c['depth_max'], point_radius=R_pt,
                                     images=None if images is None else _dev(images), images_bgr=bgr, thickness=T)


@pytest.mark.parametrize('R_pt,T,with_image,bgr', [(0, 1, False, False), (2, 1, True, True), (1, 3, True, False)])
def test_camera_equals_the_reference(camera, R_pt, T, with_image, bgr):
    c = camera
    images = c['images'] if with_image else None
    img, status = _cam_gpu(c, R_pt, T, images, bgr)
    want, want_status = R.render_camera(c['points6'], c['n_points'], c['boxes'], c['n_boxes'], c['colors'], c['mats'], c['z_near'],
                                        c['depth_max'], c['H'], c['W'], c['lut'], R_pt, images, bgr, T)
    assert img.shape == (2, 29, 41, 3) and img.dtype == torch.uint8
    assert torch.equal(status.cpu(), torch.from_numpy(want_status)) and want_status.tolist() == [0, 0]
    assert torch.equal(img.cpu(), torch.from_numpy(want))


def test_camera_planted_situations(camera):
    """The box wholly behind the camera draws nothing; the one that runs 10^5 px off the screen draws inside it; the nearer of
    two points on a pixel colours it."""
    c = camera

    def only(k):
        d = dict(c)
        d['colors'] = np.zeros_like(c['colors'])
        d['colors'][0, k] = c['colors'][0, k]
        d['n_points'] = np.zeros_like(c['n_points'])
        img, status = _cam_gpu(d, 0, 1, None, False)
        want, _ = R.render_camera(c['points6'], d['n_points'], d['boxes'], d['n_boxes'], d['colors'], c['mats'], c['z_near'],
                                  c['depth_max'], c['H'], c['W'], c['lut'], 0, None, False, 1)
        got = img.cpu().numpy()
        assert np.array_equal(got, want) and status.tolist() == [0, 0]
        return int(got[0].any(-1).sum())

    assert only(0) > 10 and only(1) > 0 and only(2) == 0 and only(3) > 0
    img, _ = _cam_gpu(c, 0, 1, None, False)
    dq = R.clampq(float(np.float64(np.float32(8.0))) / c['depth_max'] * 65535.0, 65535)
    want, _ = R.render_camera(c['points6'], c['n_points'], None, None, None, c['mats'], c['z_near'], c['depth_max'], c['H'], c['W'],
                              c['lut'], 0, None, False, 1)
    assert want[0, 10, 20].tolist() == c['lut'][dq >> 8].tolist()      # rows 10.5 / 10.2, cols 20.5 / 20.9: pixel (10, 20)


def test_rendering_is_deterministic_and_independent_of_the_point_order(bev, camera):
    g = np.random.default_rng(5)
    for c, run in ((bev, lambda c, p: _bev_gpu(c, 'height', 2, points6=p)), (camera, lambda c, p: _cam_gpu(c, 2, 2, c['images'], True, points6=p))):
        a, sa = run(c, None)
        b, sb = run(c, None)
        assert torch.equal(a, b) and torch.equal(sa, sb)
        perm = c['points6'].copy()
        for f, n in enumerate(c['n_points']):
            perm[f, :n] = perm[f, g.permutation(n)]
        p, sp = run(c, perm)
        assert torch.equal(a, p) and torch.equal(sa, sp)


def test_draw_list_from_the_device_dict_equals_the_unpacked_lists():
    """postprocess(read=False) -> draw_list without reading the counts == draw_list of the unpacked per-frame lists."""
    import modules.config as cfg
    from modules import render
    from modules.data import Preprocessing as pre
    from modules.detect import postprocess, unpack
    F, l, w = 3, 22, 25
    g = np.random.default_rng(3)
    anchors = pre.createAnchors(l, w, cfg.velorange, cfg.carsize)
    heads = np.zeros((F, l * w, 16), np.float32)
    heads[..., :2] = g.normal(-2.0, 2.0, (F, l * w, 2))
    heads[2, :, :2] = -20.0                                             # a frame without detections
    heads[..., 2:] = g.normal(0.0, 0.3, (F, l * w, 14))
    dev = postprocess(_dev(heads).reshape(F * l * w, 16), anchors, F, l, w, score_thr=0.3, iou_thr=0.1, pre_max=200, post_max=40,
                      read=False)
    gts = [torch.rand((3, 7)), None, torch.rand((1, 7))]
    boxes, n_boxes, colors = render.draw_list(gts, dev)
    lists = unpack(dev)
    counts = [d['boxes'].shape[0] for d in lists]
    assert max(counts) > 1 and counts[2] == 0
    b2, n2, c2 = render.draw_list(gts, lists, cap=boxes.shape[1])
    assert boxes.is_cuda and boxes.shape == (F, 3 + 40, 7)
    assert torch.equal(boxes, b2) and torch.equal(n_boxes, n2) and torch.equal(colors, c2)
    assert n_boxes.tolist() == [3 + counts[0], counts[1], 1]
    prio = (colors.cpu().numpy().view(np.uint32) >> 24).astype(np.int64)
    assert (prio[0, :3] == 1).all() and (prio[0, 3:3 + counts[0]] >= 2).all() and not prio[0, 3 + counts[0]:].any()
    s = lists[0]['scores'].cpu().numpy().astype(np.float64)
    assert prio[0, 3:3 + counts[0]].tolist() == [2 + min(253, int(v)) for v in np.floor(s * 253)]


def _run(script, *argv):
    p = subprocess.run([sys.executable, os.path.join(REPO, 'mvxnet-makise_amd', script)] + list(argv), capture_output=True, text=True,
                       timeout=900, cwd=REPO)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert('RGB'))


def test_visualize_like_and_detect_like_render_end_to_end(tmp_path):
    import modules.config as cfg
    root, pics = str(tmp_path / 'kitti'), str(tmp_path / 'pics')
    _run('visualize_like.py', root, '--synthetic', '3', '--view', 'both', '--out', pics)
    files = sorted(os.listdir(pics))
    assert files == ['%06d_%s.png' % (k, v) for k in range(3) for v in ('bev', 'cam')]
    for f in files:
        im = _png(os.path.join(pics, f))
        assert im.shape == ((704, 800, 3) if f.endswith('_bev.png') else (int(cfg.imsize[0]), int(cfg.imsize[1]), 3)), f
        assert int((im == np.array(GT_GREEN, np.uint8)).all(-1).sum()) > 20, f          # the GT boxes are in the picture
    # detect_like.py --render: the pictures next to result files that do not change (same process, same shuffle seed)
    import detect_like as D
    root2 = str(tmp_path / 'kitti2')
    np.random.seed(0)
    D.main(D.parse_args([root2, '--synthetic', '2', '--points', '3000', '--out', str(tmp_path / 'plain')]))
    np.random.seed(0)
    D.main(D.parse_args([root2, '--points', '3000', '--out', str(tmp_path / 'drawn'), '--render', str(tmp_path / 'pics2')]))
    assert sorted(os.listdir(str(tmp_path / 'pics2'))) == ['%06d_%s.png' % (k, v) for k in range(2) for v in ('bev', 'cam')]
    for name in ('000000.txt', '000001.txt'):
        with open(str(tmp_path / 'plain' / name), 'rb') as a, open(str(tmp_path / 'drawn' / name), 'rb') as b:
            assert a.read() == b.read(), name
    assert _png(str(tmp_path / 'pics2' / '000000_bev.png')).shape == (704, 800, 3)


def _inside_or_on(outline):
    """Pixels of a bool mask that a 4-connected walk from outside the mask's bounding box cannot reach: the closed outline and
    what it encloses."""
    rows, cols = np.nonzero(outline)
    r0, r1, c0, c1 = rows.min() - 1, rows.max() + 2, cols.min() - 1, cols.max() + 2
    assert r0 >= 0 and c0 >= 0 and r1 <= outline.shape[0] and c1 <= outline.shape[1], 'the outline touches the image border'
    wall = outline[r0:r1, c0:c1]
    seen = np.zeros_like(wall)
    stack = [(0, 0)]
    seen[0, 0] = True
    while stack:
        r, c = stack.pop()
        for rr, cc in ((r + 1, c), (r - 1, c), (r, c + 1), (r, c - 1)):
            if 0 <= rr < wall.shape[0] and 0 <= cc < wall.shape[1] and not seen[rr, cc] and not wall[rr, cc]:
                seen[rr, cc] = True
                stack.append((rr, cc))
    out = np.zeros_like(outline)
    out[r0:r1, c0:c1] = ~seen
    return out


def test_boxes_sit_on_their_point_clusters():
    """Full-size views through modules.render (range and sizes from the configuration): points sampled inside two rotated boxes
    fall on or inside the drawn outline of their box in both views -- a flipped axis, a transposed image or a yaw of the wrong
    sign between the point rule and the box rule would put them outside."""
    import modules.config as cfg
    from modules import render
    from modules.data import Synthetic as S
    g = np.random.default_rng(2)
    gt = np.array([[20.0, 5.0, -1.5, 4.0, 1.8, 1.5, 0.4], [35.0, -8.0, -1.6, 4.2, 1.7, 1.6, -1.1]], np.float32)
    M = S.KITTI_CALIB['P2'] @ S.KITTI_CALIB['R0_rect'] @ S.KITTI_CALIB['Tr_velo_to_cam']
    n_each = 400
    clusters = []
    for b in gt.astype(np.float64):
        u, v = g.uniform(-0.4, 0.4, n_each) * b[3], g.uniform(-0.4, 0.4, n_each) * b[4]
        c, s = np.cos(b[6]), np.sin(b[6])
        xyz = np.stack([u * c + v * s + b[0], -u * s + v * c + b[1], b[2] + g.uniform(0.1, 0.9, n_each) * b[5]], 1).astype(np.float32)
        cam = np.concatenate([xyz.astype(np.float64), np.ones((n_each, 1))], 1) @ M.T
        clusters.append(np.concatenate([xyz, g.uniform(0, 1, (n_each, 1)).astype(np.float32),
                                        (cam[:, 1:2] / cam[:, 2:3]).astype(np.float32), (cam[:, 0:1] / cam[:, 2:3]).astype(np.float32)], 1))
    pts = _dev(np.concatenate(clusters)[None])
    none = (pts, torch.zeros((1,), dtype=torch.int32, device=DEV))
    H, W = render.bev_shape(0.1)
    assert (H, W) == (704, 800)
    for k in range(2):
        draw = render.draw_list([torch.from_numpy(gt[k:k + 1])], None, device=DEV)
        bev, st = render.render_bev(none, draw)
        cam, st2 = render.render_camera(none, draw, None, matrices=M[None])
        assert bev.shape == (1, H, W, 3) and cam.shape == (1, int(cfg.imsize[0]), int(cfg.imsize[1]), 3) and st.tolist() == st2.tolist() == [0]
        p = clusters[k].astype(np.float64)
        region = _inside_or_on((bev[0].cpu().numpy() == np.array(GT_GREEN, np.uint8)).all(-1))
        rows = H - 1 - np.floor((p[:, 0] - cfg.velorange[0]) / 0.1).astype(int)
        cols = W - 1 - np.floor((p[:, 1] - cfg.velorange[1]) / 0.1).astype(int)
        assert region[rows, cols].all() and 600 < region.sum() < 900, (k, int(region.sum()))       # a box of about 40 x 18 px
        region = _inside_or_on((cam[0].cpu().numpy() == np.array(GT_GREEN, np.uint8)).all(-1))
        assert region[np.floor(p[:, 4]).astype(int), np.floor(p[:, 5]).astype(int)].all(), k
    # and the points themselves are where that rule says, in both views
    both = (pts, torch.tensor([2 * n_each], dtype=torch.int32, device=DEV))
    bev, _ = render.render_bev(both, None)
    lit = (bev[0].cpu().numpy() != 0).any(-1)
    p = np.concatenate(clusters).astype(np.float64)
    want = np.zeros_like(lit)
    want[H - 1 - np.floor((p[:, 0] - cfg.velorange[0]) / 0.1).astype(int), W - 1 - np.floor((p[:, 1] - cfg.velorange[1]) / 0.1).astype(int)] = True
    assert np.array_equal(lit, want)
