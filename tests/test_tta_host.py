"""CPU-only checks of the test-time augmentation (modules/tta.py, csrc/tta.hip): the float64 reference against itself and
against Geometry.transform_boxes, the case builder's margins, the view parser, expand_batch's refusals and the C ABI's
declarations and argument checks before any launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

import abi_header
import tta_cases as C
import tta_ref as R


def test_reference_is_self_consistent():
    case = C.build()
    out = R.fuse(case['boxes'], case['scores'], case['counts'], case['views'], case['F'], C.IOU_THR, C.FUSE_IOU)
    V, post_max = case['views'].shape[0], case['post_max']
    for f, fr in enumerate(out):
        mb, ms, prov = fr['merged']
        assert len(prov) == int(case['counts'][f * V:(f + 1) * V].sum()) and not fr['bad']
        iou, heads, voters = fr['iou'], fr['all_heads'], fr['voters']
        for a in heads:                                 # the heads are a greedy NMS of the union: none suppresses another
            for b in heads:
                assert a == b or iou[min(a, b), max(a, b)] <= C.IOU_THR
        assert heads == R.D.greedy_nms(R.D.corners(mb), C.IOU_THR, len(prov) + 1)
        for h in heads:
            seen = [prov[j] // post_max for j in voters[h]]
            assert len(seen) == len(set(seen)) and voters[h][0] == h and voters[h] == sorted(voters[h])
        assert (np.diff(fr['scores']) < 0).all()
        # every planted box comes out once, within the jitter, and nothing else does
        g = case['ground'][f]
        assert fr['boxes'].shape[0] == g.shape[0]
        d = np.linalg.norm(fr['boxes'][:, None, :2] - g[None, :, :2].astype(np.float64), axis=2)
        assert sorted(d.argmin(1).tolist()) == list(range(g.shape[0])) and d.min(1).max() < 0.2
        near = g[d.argmin(1)]
        assert R.yaw_distance(fr['boxes'][:, 6], near[:, 6]).max() < 0.05      # also across the +-pi seam
    f0 = out[0]
    k0 = int(np.linalg.norm(f0['boxes'][:, :2] - case['ground'][0][0, :2], axis=1).argmin())
    k1 = int(np.linalg.norm(f0['boxes'][:, :2] - case['ground'][0][1, :2], axis=1).argmin())
    k2 = int(np.linalg.norm(f0['boxes'][:, :2] - case['ground'][0][2, :2], axis=1).argmin())
    assert f0['n_views'][k0] == V               # V + 1 sightings above fuse_iou, two of them of view 0: one vote per view
    h0 = f0['heads'][k0]
    assert sum(1 for j in range(h0 + 1, len(f0['merged'][2])) if f0['iou'][h0, j] > C.FUSE_IOU) == V
    assert f0['n_views'][k1] == 1 and f0['src'][k1] // post_max == 1
    assert f0['n_views'][k2] == V - 1           # the shifted sighting belongs to the cluster and does not vote
    assert out[1]['n_views'].max() == V - 1     # the empty view
    two = R.fuse(case['boxes'], case['scores'], case['counts'], case['views'], case['F'], C.IOU_THR, C.FUSE_IOU, min_views=2)
    assert two[0]['boxes'].shape[0] == f0['boxes'].shape[0] - 1 and (two[0]['n_views'] >= 2).all()


def test_one_identity_view_is_a_no_op():
    case = C.build(views=np.array([[0, 1, 0, 0]], np.float32), n_ground=(10,), post_max=16)
    fr = R.fuse(case['boxes'], case['scores'], case['counts'], case['views'], 1, C.IOU_THR, C.FUSE_IOU)[0]
    keep = R.D.greedy_nms(R.D.corners(case['boxes'][0, :case['counts'][0]]), C.IOU_THR, 100)
    assert fr['src'].tolist() == keep
    assert np.array_equal(fr['boxes'].astype(np.float32), case['boxes'][0, keep])
    assert np.array_equal(fr['scores'].astype(np.float32), case['scores'][0, keep])


def test_inverse_after_forward_returns_the_planted_boxes():
    from modules.augment.Geometry import transform_boxes
    g = C.planted(24, 5)
    for row in ([0.0, 1.0, 0.0, 0.0], [0.3, 1.05, 1.0, 0.0], [-0.7, 0.9, 0.0, 0.0], [0.0, 1.0, 1.0, 0.0], [math.pi / 8, 1.0, 1.0, 0.0]):
        fwd = np.asarray(g, np.float64)                                        # the forward step in float64, unrounded
        G = np.asarray(row, np.float32).astype(np.float64)
        c, s = math.cos(G[0]), math.sin(G[0])
        out = fwd.copy()
        out[:, 0] = G[1] * (c * fwd[:, 0] + s * fwd[:, 1])
        out[:, 1] = G[1] * (-s * fwd[:, 0] + c * fwd[:, 1]) * (-1 if G[2] else 1)
        out[:, 2:6] = G[1] * fwd[:, 2:6]
        out[:, 6] = (fwd[:, 6] + G[0]) * (-1 if G[2] else 1)
        assert np.abs(out[:, :6] - transform_boxes(g, row)[:, :6]).max() < 1e-5        # ... is Geometry.transform_boxes
        back = inverse64(out, row)
        assert np.abs(back[:, :6] - g[:, :6]).max() < 1e-6
        assert R.yaw_distance(back[:, 6], g[:, 6]).max() < 1e-6


def inverse64(boxes64, row):
    """tta_ref.inverse_boxes without its f32 reading of the input."""
    b = np.asarray(boxes64, np.float64)
    row = np.asarray(row, np.float32).astype(np.float64)
    x, y, r = b[:, 0], b[:, 1], b[:, 6]
    if row[2]:
        y, r = -y, -r
    c, s = math.cos(row[0]), math.sin(row[0])
    out = b / row[1]
    out[:, 0], out[:, 1] = (c * x - s * y) / row[1], (s * x + c * y) / row[1]
    out[:, 6] = R.wrap(r - row[0], 2 * math.pi)
    return out


def test_reference_inverse_matches_the_unrounded_inverse():
    g = C.planted(24, 6)
    from modules.augment.Geometry import transform_boxes
    for row in ([0.3, 1.05, 1.0, 0.0], [-0.2, 0.95, 0.0, 0.0]):
        back = R.inverse_boxes(transform_boxes(g, row), row)                   # through the f32 boxes a view's list holds
        assert np.abs(back[:, :3] - g[:, :3]).max() < 1e-4
        assert (np.abs(back[:, 3:6] - g[:, 3:6]) / g[:, 3:6]).max() < 1e-6
        assert R.yaw_distance(back[:, 6], g[:, 6]).max() < 1e-5


def test_case_margins_hold():
    for case in (C.build(), C.build(seed=1, n_ground=(12,), post_max=16)):
        out = C.check_margins(case)
        assert len(out) == case['F']
    worst = min(float(np.abs(fr['iou'][np.triu_indices(fr['iou'].shape[0], 1)] - t).min()) for fr in out for t in (C.IOU_THR, C.FUSE_IOU))
    assert worst >= C.MARGIN
    n0 = int(C.build()['counts'][:3].sum())
    assert n0 > 64                              # the merged list of frame 0 crosses a 64-bit mask word


def test_views_parses_names_and_rows():
    from modules import tta
    from modules import Extension as X
    v = tta.views(['identity', 'flip', 'rot+', 'rot-', 'flip+rot+', 'flip+rot-'])
    assert v.dtype == np.float32 and v.shape == (6, 4)
    r = np.float32(math.pi / 8)
    assert v.tolist() == [[0, 1, 0, 0], [0, 1, 1, 0], [r, 1, 0, 0], [-r, 1, 0, 0], [r, 1, 1, 0], [-r, 1, 1, 0]]
    assert tta.views(['rot+'], rot=0.25)[0, 0] == np.float32(0.25)
    mixed = tta.views(['identity', (0.1, 1.05, 1), [-0.2, 0.95, 0, 0]])
    assert np.array_equal(mixed, np.array([[0, 1, 0, 0], [0.1, 1.05, 1, 0], [-0.2, 0.95, 0, 0]], np.float32))
    assert np.array_equal(tta.views(mixed), mixed) and np.array_equal(tta.views('flip'), tta.views(['flip']))
    for bad in (['mirror'], [], ['identity'] * 9, [(0.1, 0.0, 0)], [(0.1, 1.0)], [(float('nan'), 1.0, 0)], [(0.1, 1.0, 0, 2.0)]):
        with pytest.raises(X.MvxHipError):
            tta.views(bad)


def test_expand_batch_and_fuse_views_refuse_bad_arguments():
    from modules import tta
    from modules import Extension as X
    from modules.pipeline import FrameBatch
    batch = FrameBatch(torch.zeros((9, 8, 6)), None, torch.zeros((9,), dtype=torch.int32), [None] * 9)
    with pytest.raises(X.MvxHipError, match=r'9 frames x 2 views = 18 .* 16'):
        tta.expand_batch(batch, ['identity', 'flip'])
    with pytest.raises(X.MvxHipError):
        tta.expand_batch(batch, ['sideways'])
    dets = dict(boxes=torch.zeros((4, 8, 7)), scores=torch.zeros((4, 8)), meta=torch.zeros((3, 4), dtype=torch.int32))
    for kw in (dict(F=3), dict(iou_thr=0.6), dict(fuse_iou=1.0), dict(min_views=3), dict(min_views=0), dict(out_max=17), dict(out_max=0),
               dict(iou_thr=1e-4)):
        a = dict(F=2, iou_thr=0.1, fuse_iou=0.5, min_views=1, out_max=None)
        a.update(kw)
        with pytest.raises(X.MvxHipError):
            tta.fuse_views(dets, ['identity', 'flip'], a.pop('F'), **a)


def test_detect_frame_set_refuses_ready_with_tta():
    from modules import Extension as X
    from modules.detect import detect_frame_set
    from modules.pipeline import FrameBatch
    batch = FrameBatch(torch.zeros((1, 8, 6)), None, torch.zeros((1,), dtype=torch.int32), [None])
    with pytest.raises(X.MvxHipError, match='ready'):
        detect_frame_set(None, batch, None, (370, 1224), ready=object(), tta=['identity'])


def test_header_entries_parse_and_match_the_prototypes():
    from modules import Extension as X
    decl = abi_header.declarations()
    for name in ('mvx_tta_workspace_bytes', 'mvx_tta_fuse_frames'):
        res, params = decl[name]
        assert (res, [t for _, t in params]) == X.PROTOTYPES[name], name
        assert hasattr(ctypes.CDLL(X.LIB_PATH), name)
    assert abi_header.parameter_names('mvx_tta_fuse_frames')[:4] == ['boxes', 'scores', 'counts', 'views']
    assert abi_header.parameter_names('mvx_tta_fuse_frames')[-3:] == ['workspace', 'workspace_bytes', 'stream']
    text = open(abi_header.HEADER).read()
    for name, value in (('MVX_TTA_MAX_VIEWS', 8), ('MVX_TTA_MAX_BOXES', 1024), ('MVX_TTA_NONFINITE', 2)):
        assert '#define %s %d\n' % (name, value) in text
    from modules import _hip
    assert (_hip.TTA_MAX_VIEWS, _hip.TTA_MAX_BOXES, _hip.TTA_NONFINITE) == (8, 1024, 2)
    one, four = X.lib.mvx_tta_workspace_bytes(1, 4, 100), X.lib.mvx_tta_workspace_bytes(4, 4, 100)
    assert one >= 2 * 400 * 7 * 8 and four == 4 * one and one % 256 == 0
    assert X.lib.mvx_tta_workspace_bytes(1, 8, 129) == 0


def _call(**over):
    """mvx_tta_fuse_frames with plausible arguments and fake, never dereferenced device addresses: every case must be refused
    by the host-side checks before anything is launched."""
    from modules import Extension as X
    fake = ctypes.c_void_p(1 << 20)
    a = dict(boxes=fake, scores=fake, counts=fake, views=fake, F=4, V=4, post_max=100, iou_thr=0.01, fuse_iou=0.5, min_views=1,
             out_max=100, full_turn=0, ob=fake, osc=fake, onv=fake, osrc=fake, ocnt=fake, status=fake, ws=fake, ws_bytes=1 << 40)
    a.update(over)
    return X.lib.mvx_tta_fuse_frames(a['boxes'], a['scores'], a['counts'], a['views'], a['F'], a['V'], a['post_max'], a['iou_thr'],
                                     a['fuse_iou'], a['min_views'], a['out_max'], a['full_turn'], a['ob'], a['osc'], a['onv'],
                                     a['osrc'], a['ocnt'], a['status'], a['ws'], a['ws_bytes'], None)


@pytest.mark.parametrize('over', [
    dict(F=0), dict(F=17), dict(V=0), dict(V=9), dict(post_max=0), dict(post_max=257), dict(iou_thr=5e-4), dict(iou_thr=0.6),
    dict(fuse_iou=1.0), dict(min_views=0), dict(min_views=5), dict(out_max=0), dict(out_max=401), dict(boxes=None), dict(scores=None),
    dict(counts=None), dict(views=None), dict(ob=None), dict(osc=None), dict(onv=None), dict(osrc=None), dict(ocnt=None),
    dict(status=None), dict(ws=None), dict(ws=ctypes.c_void_p((1 << 20) + 64)), dict(ws_bytes=1024),
], ids=lambda o: '-'.join('%s=%s' % kv for kv in o.items()))
def test_tta_fuse_frames_rejects_bad_arguments_before_any_launch(over):
    assert _call(**over) == -1
