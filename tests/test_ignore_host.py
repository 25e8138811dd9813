"""CPU-only checks of the ignore pass (csrc/ignore.hip, Calc.IgnoreRegions): the C ABI's declarations against the
prototype table and its argument checks, the rule itself (tests/ignore_ref.ignore_rule) on hand-written tables, one per clause,
the conditions the GPU fixtures must meet, the label reader, the geometry helpers and the command-line switches."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import abi_header
import ignore_cases as IC
import ignore_ref as IR

ENTRIES = ('mvx_box_point_counts_frames', 'mvx_ignore_anchors_frames_workspace_bytes', 'mvx_ignore_anchors_frames')


def test_header_matches_the_prototype_table_and_the_abi_is_still_10():
    from modules import Extension as X
    assert X.ABI_VERSION == 10 and X.lib.mvx_abi_version() == 10
    lib = ctypes.CDLL(X.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name) and name in X.PROTOTYPES
        res, params = abi_header.declarations()[name]
        assert X.PROTOTYPES[name][0] is res, name
        assert X.PROTOTYPES[name][1] == [t for _, t in params], name
    assert len(abi_header.parameter_names('mvx_ignore_anchors_frames')) == 30
    assert len(abi_header.parameter_names('mvx_box_point_counts_frames')) == 10
    q = X.lib.mvx_ignore_anchors_frames_workspace_bytes
    assert q(4, 176, 200, 2) >= 4 * 176 * 200 * 2 * 4 + 4 * 16 and q(0, 176, 200, 2) <= 256
    assert q(4, 176, 200, 2) < X.lib.mvx_assign_anchors_frames_workspace_bytes(60, 4, 176, 200, 2)      # a 4-byte map against an 8-byte one


GOOD = dict(cap=100, n_frames=2, min_points=5, l=24, w=20, anchors_per_loc=2, ioa_thr=0.5, cap_out=960, workspace_bytes=1 << 40,
            cap_points=100, ld=6, n_boxes_total=3, stream=None)
BAD = (('pos_idx', None), ('neg_idx', None), ('gi', None), ('counts', None), ('anchors', None), ('anchor_quads', None), ('pos_out', None),
       ('neg_out', None), ('gi_out', None), ('counts_out', None), ('stats', None), ('status', None), ('workspace', None),
       ('gt_off', None), ('rect_off', None), ('img_from_lidar', None), ('ign_off', None),
       ('n_frames', 0), ('n_frames', 17), ('anchors_per_loc', 0), ('anchors_per_loc', 5), ('cap', 0), ('cap_out', 0), ('ioa_thr', 0.0),
       ('ioa_thr', -0.5), ('ioa_thr', 1.5), ('min_points', -1), ('workspace_bytes', 1024), ('l', 0), ('w', 0),
       ('points6', None), ('n_points', None), ('boxes', None), ('cap_points', 0), ('ld', 2), ('n_boxes_total', -1))


def test_each_bad_argument_is_refused_before_any_launch():
    """Dummy host pointers and ONE bad argument: MVX_EINVAL.  A launch on these pointers would fault, and without a GPU the memset
    in front of the launches would return a HIP error instead of -1."""
    from modules import Extension as X
    buf = ctypes.create_string_buffer(4096 + 64)
    dummy = (ctypes.addressof(buf) + 63) & ~63
    calls = 0
    for name in ('mvx_ignore_anchors_frames', 'mvx_box_point_counts_frames'):
        names = abi_header.parameter_names(name)
        for param, value in BAD:
            if param not in names:
                continue
            args = [value if q == param else GOOD[q] if q in GOOD else dummy for q in names]
            assert getattr(X.lib, name)(*args) == -1, (name, param, value)
            calls += 1
    assert calls == 30 + 10
    # every source is optional: with all of them null the check that fails is the (too small) workspace, not they
    names = abi_header.parameter_names('mvx_ignore_anchors_frames')
    absent = ('gt_off', 'gt_points', 'rects', 'rect_off', 'img_from_lidar', 'ign_quads', 'ign_off')
    args = [None if q in absent else 16 if q == 'workspace_bytes' else GOOD[q] if q in GOOD else dummy for q in names]
    assert X.lib.mvx_ignore_anchors_frames(*args) == -1
    # no box at all: nothing to count, nothing touched, no launch
    names = abi_header.parameter_names('mvx_box_point_counts_frames')
    args = [0 if q == 'n_boxes_total' else GOOD[q] if q in GOOD else None for q in names]
    assert X.lib.mvx_box_point_counts_frames(*args) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the rule on hand-written tables: 6 anchors, centres at pixel (10 a, 5), one rectangle over anchors 2..4
# ---------------------------------------------------------------------------------------------------------------------------
def _centres(depth=None):
    px = 10.0 * np.arange(6)
    return px, np.full((6,), 5.0), np.ones((6,)) if depth is None else np.asarray(depth, np.float64)


RECT = [[15.0, 0.0, 45.0, 10.0]]
AREA = np.full((6,), 4.0, np.float32)


def _rule(**k):
    r = IR.ignore_rule(6, **k)
    return r['pos'].tolist(), r['gi'].tolist(), r['notneg'].tolist(), r['stats']


def test_rule_demotion():
    # box 1 holds 4 points, one fewer than asked: its positive (anchor 3) is demoted and stays not negative; no rematch
    got = _rule(pos=[1, 3], gi=[0, 1], notneg=[1, 3, 4], gt_points=[5, 4], min_points=5)
    assert got == ([1], [0], [1, 3, 4], [1, 0, 0, 1])
    # exactly min_points: kept; no counts given: nothing is sparse
    assert _rule(pos=[1, 3], gi=[0, 1], notneg=[1, 3, 4], gt_points=[5, 5], min_points=5) == ([1, 3], [0, 1], [1, 3, 4], [0, 0, 0, 0])
    assert _rule(pos=[1, 3], gi=[0, 1], notneg=[1, 3, 4], min_points=5) == ([1, 3], [0, 1], [1, 3, 4], [0, 0, 0, 0])
    # a sparse box without a positive still counts as sparse
    assert _rule(pos=[1], gi=[0], notneg=[1], gt_points=[9, 0, 2], min_points=3)[3] == [0, 0, 0, 2]


def test_rule_rectangle_only():
    assert _rule(pos=[0], gi=[0], notneg=[0], centres=_centres(), rects=RECT) == ([0], [0], [0, 2, 3, 4], [0, 3, 0, 0])
    # edges inclusive
    assert _rule(pos=[], gi=[], notneg=[], centres=_centres(), rects=[[20.0, 5.0, 40.0, 5.0]])[2] == [2, 3, 4]


def test_rule_box_only():
    inter = np.array([[0.0, 2.0, 1.9, 0.0, 0.0, 4.0]], np.float32)          # ioa 0.5 exactly, just below, 1.0
    assert _rule(pos=[0], gi=[0], notneg=[0], inter=inter, area=AREA) == ([0], [0], [0, 1, 5], [0, 0, 2, 0])
    # intersection over the ANCHOR's area: a box however large shields the anchor it covers
    assert _rule(pos=[], gi=[], notneg=[], inter=inter, area=AREA, ioa_thr=1.0)[2] == [5]


def test_rule_both_sources_and_the_precedence_of_the_rectangle():
    inter = np.array([[0.0, 3.0, 3.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 4.0, 4.0]], np.float32)
    got = _rule(pos=[0], gi=[0], notneg=[0], centres=_centres(), rects=RECT, inter=inter, area=AREA)
    assert got == ([0], [0], [0, 1, 2, 3, 4, 5], [0, 3, 2, 0])              # 2 and 4 count for the rectangle, 1 and 5 for the boxes


def test_rule_leaves_what_is_already_not_negative():
    inter = np.array([[4.0, 4.0, 0.0, 0.0, 0.0, 0.0]], np.float32)
    got = _rule(pos=[3], gi=[0], notneg=[0, 2, 3], centres=_centres(), rects=RECT, inter=inter, area=AREA)
    assert got == ([3], [0], [0, 1, 2, 3, 4], [0, 1, 1, 0])                # new: 4 by the rectangle, 1 by the box
    # a demoted positive is not counted again by a rectangle over it
    got = _rule(pos=[3], gi=[0], notneg=[3], gt_points=[0], min_points=1, centres=_centres(), rects=RECT)
    assert got == ([], [], [2, 3, 4], [1, 2, 0, 1])


def test_rule_depth_not_positive():
    got = _rule(pos=[], gi=[], notneg=[], centres=_centres([1.0, 1.0, 0.0, -2.0, 1.0, 1.0]), rects=RECT)
    assert got == ([], [], [4], [0, 1, 0, 0])
    an = np.array([[-3.0, 0.0, -1.0, 3.9, 1.6, 1.56, 0.0], [0.27, 0.0, -1.0, 3.9, 1.6, 1.56, 0.0], [12.0, 0.5, -1.0, 3.9, 1.6, 1.56, 0.0]], np.float32)
    px, py, d = IR.project(an, IC.MATRIX)
    assert d[0] < 0 and abs(d[1] - 0.002745884) < 1e-6 and d[2] > 11 and np.isnan(px[0]) and np.isfinite(px[2])
    # by hand: camera (x, y, z) = (-0.5, 1 - 0.78 - 0.08, 12 - 0.27)
    assert abs(px[2] - ((721.5377 * -0.5 + 609.5593 * 11.73 + 44.85728) / (11.73 + 0.002745884))) < 1e-3
    assert abs(py[2] - ((721.5377 * 0.14 + 172.854 * 11.73 + 0.2163791) / (11.73 + 0.002745884))) < 1e-3


def test_rule_empty_frame():
    assert _rule(pos=[], gi=[], notneg=[]) == ([], [], [], [0, 0, 0, 0])
    assert _rule(pos=[], gi=[], notneg=[], gt_points=[], min_points=5, centres=_centres(), rects=np.zeros((0, 4)),
                 inter=np.zeros((0, 6), np.float32), area=AREA) == ([], [], [], [0, 0, 0, 0])
    # with no source the lists come back as they went in
    assert _rule(pos=[1, 4], gi=[2, 0], notneg=[0, 1, 4]) == ([1, 4], [2, 0], [0, 1, 4], [0, 0, 0, 0])


def test_area32_is_the_shoelace_magnitude_either_way_round():
    q = np.array([[[2.0, 1.0], [-2.0, 1.0], [-2.0, -1.0], [2.0, -1.0]]], np.float32)
    assert IR.area32(q).tolist() == [8.0] and IR.area32(q[:, ::-1]).tolist() == [8.0]


# ---------------------------------------------------------------------------------------------------------------------------
# conditions on the GPU fixtures that need no GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, rects', [(n, r) for n, r in IC.RECTS.items()] + [('44x50x2', [IC.RECT_ALL])])
def test_no_anchor_centre_projects_onto_a_rectangle_edge(name, rects):
    g = IC.grid(name)
    px, py, d = IR.project(g['anchors'].reshape(-1, 7), IC.MATRIX)
    hit, margin = IR.in_rects(px, py, d, rects)
    print('%s %s: %d of %d centres inside, the nearest %.3g px from an edge' % (name, rects, hit.sum(), hit.size, margin))
    assert margin > 1e-6
    if name == '24x20x2behind':
        assert (d <= 0).any() and (d > 0).any() and hit.any() and not hit[d <= 0].any()
    elif rects == [IC.RECT_ALL]:
        assert hit.sum() > 4 * 256                      # the not-negative list crosses several block boundaries
    else:
        assert 0 < hit.sum() < hit.size


def test_no_point_of_the_count_fixture_lies_on_a_box_face():
    fx = IC.point_fixture()
    counts, margin = IR.point_counts64(fx['points'], fx['n_points'], fx['boxes'], fx['gt_off'])
    print('point counts %s, the nearest point %.3g m from a face' % (counts.tolist(), margin))
    assert margin > 1e-6 and (counts[:5] > 100).all() and counts[5] == 1
    # the rows beyond n_points lie inside a box: reading them would change the count
    full, _ = IR.point_counts64(fx['points'], np.full((3,), fx['points'].shape[1]), fx['boxes'], fx['gt_off'])
    assert (full[[0, 3, 5]] > counts[[0, 3, 5]]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# Python layers
# ---------------------------------------------------------------------------------------------------------------------------
def test_label_reader_on_a_written_label_file(tmp_path):
    from modules import Calc
    from modules.data import Load
    root = tmp_path / 'kitti'
    (root / 'training' / 'label_2').mkdir(parents=True)
    (root / 'training' / 'calib').mkdir(parents=True)
    rows = ['Car 0.00 0 -1.6 100.0 150.0 200.0 220.0 1.5 1.6 3.9 1.0 1.7 15.0 -1.5',
            'Van 0.00 1 1.2 300.5 160.0 420.0 240.0 2.2 1.9 5.1 -3.0 1.8 20.0 0.3',
            'DontCare -1 -1 -10 503.89 169.71 590.61 190.13 -1 -1 -1 -1000 -1000 -1000 -10',
            'Truck 0.00 0 0.1 10.0 20.0 30.0 40.0 3.0 2.6 10.0 4.0 1.9 30.0 1.6',
            'DontCare -1 -1 -10 0.00 1.50 20.25 30.75 -1 -1 -1 -1000 -1000 -1000 -10']
    (root / 'training' / 'label_2' / '000007.txt').write_text('\n'.join(rows) + '\n')
    (root / 'training' / 'label_2' / '000008.txt').write_text(rows[0] + '\n')
    tr = IC.TR[:3].reshape(-1)
    calib = ['P0: ' + ' '.join(['0'] * 12), 'P1: ' + ' '.join(['0'] * 12), 'P2: ' + ' '.join('%.9g' % v for v in IC.P2.reshape(-1)),
             'P3: ' + ' '.join(['0'] * 12), 'R0_rect: 1 0 0 0 1 0 0 0 1', 'Tr_velo_to_cam: ' + ' '.join('%.9g' % v for v in tr),
             'Tr_imu_to_velo: ' + ' '.join(['0'] * 12)]
    for n in ('000007', '000008'):
        (root / 'training' / 'calib' / (n + '.txt')).write_text('\n'.join(calib) + '\n')
    (r7, b7), (r8, b8) = Load.readIgnoreLabels(['000007', '000008'], root=str(root))
    assert r7.dtype == torch.float32 and np.allclose(r7.numpy(), [[503.89, 169.71, 590.61, 190.13], [0.0, 1.5, 20.25, 30.75]])
    assert tuple(b7.shape) == (1, 7) and tuple(r8.shape) == (0, 4) and tuple(b8.shape) == (0, 7)
    # the van: camera (x, y, z) = (-3, 1.8, 20) -> LiDAR (z + 0.27, -x, -y - 0.08), sizes l w h, yaw - pi/2
    assert np.allclose(b7.numpy(), [[20.27, 3.0, -1.88, 5.1, 1.9, 2.2, 0.3 - np.pi / 2]], atol=1e-5)
    c2v = torch.linalg.inv(torch.Tensor(IC.TR))
    want = Calc.bboxCam2Lidar(torch.Tensor([[2.2, 1.9, 5.1, -3.0, 1.8, 20.0, 0.3]]), c2v)
    assert torch.equal(b7, want)
    (_, both), _ = Load.readIgnoreLabels(['000007', '000008'], root=str(root), classes=('Van', 'Truck'))
    assert tuple(both.shape) == (2, 7) and np.allclose(both[1, 3:6].numpy(), [10.0, 2.6, 3.0])
    (_, none), _ = Load.readIgnoreLabels(['000007', '000008'], root=str(root), classes=())
    assert tuple(none.shape) == (0, 7)


def test_cli_switches_and_errors():
    import train_like as T
    a = T.parse_args(['root', '--mode', 'fast', '--targets', 'maxiou', '--ignore-dontcare', '--ignore-classes', 'Van', 'Truck',
                      '--min-gt-points', '5'])
    assert a.ignore_dontcare and a.ignore_classes == ['Van', 'Truck'] and a.ignore_ioa == 0.5 and a.min_gt_points == 5 and a.ignore
    d = T.parse_args(['root'])
    assert not d.ignore_dontcare and d.ignore_classes == [] and d.ignore_ioa == 0.5 and d.min_gt_points == 0 and not d.ignore
    assert T.parse_args(['root', '--mode', 'fast', '--targets', 'maxiou', '--ignore-classes', 'Van', '--ignore-ioa', '0.3']).ignore_ioa == 0.3
    for flags in (['--ignore-dontcare'], ['--ignore-classes', 'Van'], ['--ignore-ioa', '0.4'], ['--min-gt-points', '3']):
        with pytest.raises(SystemExit):
            T.parse_args(['root', '--mode', 'fast'] + flags)                              # the reference assigner
        with pytest.raises(SystemExit):
            T.parse_args(['root', '--mode', 'fast', '--targets', 'reference'] + flags)
    for flags in (['--ignore-ioa', '0'], ['--ignore-ioa', '1.5'], ['--min-gt-points', '-1']):
        with pytest.raises(SystemExit):
            T.parse_args(['root', '--mode', 'fast', '--targets', 'maxiou', '--ignore-dontcare'] + flags)


def test_global_matrix_and_its_inverse():
    from modules.augment import Geometry
    for row in ([0.3, 1.04, 0.0, 0.0], [-0.7, 0.96, 1.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 1.0, 1.0, 0.0]):
        G = Geometry.global_matrix(np.array(row, np.float32))
        assert G.dtype == np.float64 and G.shape == (4, 4) and np.array_equal(G[3], [0, 0, 0, 1])
        assert np.abs(G @ np.linalg.inv(G) - np.eye(4)).max() < 1e-14
        assert abs(abs(np.linalg.det(G[:3, :3])) - np.float64(np.float32(row[1])) ** 3) < 1e-12
        assert (np.linalg.det(G[:3, :3]) < 0) == bool(row[2])
    assert np.array_equal(Geometry.global_matrix([0.0, 1.0, 0.0, 0.0]), np.eye(4))
    # by hand: p_xy @ R(phi), R = [[c, -s], [s, c]] on row vectors, then the scale, then the flip of y
    phi, k = np.float64(np.float32(0.3)), np.float64(np.float32(1.04))
    p = Geometry.global_matrix(np.array([0.3, 1.04, 1.0, 0.0], np.float32)) @ np.array([2.0, 1.0, -0.5, 1.0])
    assert np.allclose(p[:3], [k * (2 * np.cos(phi) + np.sin(phi)), -k * (-2 * np.sin(phi) + np.cos(phi)), -0.5 * k], atol=1e-14)
    b = Geometry.transform_boxes(np.array([[2.0, 1.0, -0.5, 3.9, 1.6, 1.5, 3.0]], np.float32), np.array([0.3, 1.04, 1.0, 0.0], np.float32))
    assert b.dtype == np.float32 and np.allclose(b[0, :3], p[:3], atol=1e-6) and np.allclose(b[0, 3:6], k * np.array([3.9, 1.6, 1.5]), atol=1e-6)
    assert abs(b[0, 6] - (-(3.0 + phi) + 2 * np.pi)) < 1e-6                             # wrapped into [-pi, pi)


def test_python_keywords_and_the_holder():
    from modules import Calc, pipeline
    from modules.data import Prefetch
    assert inspect.signature(Calc.assignAnchorsFrames).parameters['ignore'].default is None
    assert inspect.signature(pipeline.batch_from_dataset).parameters['ignore'].default is None
    assert inspect.signature(Prefetch.PrefetchLoader.__init__).parameters['ignore'].default is None
    with pytest.raises(ValueError):
        Calc.IgnoreRegions(2, rects=[None])
    with pytest.raises(ValueError):
        Calc.IgnoreRegions(1, ioa_thr=0.0)
    with pytest.raises(ValueError):
        Calc.IgnoreRegions(1, min_points=-1)
    with pytest.raises(ValueError):
        Calc.IgnoreRegions(1, anchors=torch.zeros((2, 2, 2, 7)), rects=[torch.zeros((1, 4))])          # rectangles and no matrix
    with pytest.raises(ValueError):
        Calc.IgnoreRegions(1, rects=[torch.zeros((1, 4))], matrix=[np.eye(4)[:3]])                     # ... and no anchors
    reg = Calc.IgnoreRegions(3, quads=[None, torch.zeros((2, 4, 2)), torch.zeros((0, 4, 2))])
    assert [reg.has_source(k) for k in range(3)] == [False, True, False]
    # frames without boxes and without a source need no device
    info = {}
    anchors = torch.zeros((2, 2, 2, 4, 2))
    assert Calc.assignAnchorsFrames([None, (torch.zeros((0, 4, 2)), None)], anchors, info=info, ignore=Calc.IgnoreRegions(2)) == [None, None]
    assert info['ignore_stats'] == [0, 0, 0, 0]
    # an assigner without the keyword cannot take ignore regions
    assert not pipeline.assigner_takes_ignore(lambda frames: None) and not pipeline.assigner_takes_ignore(None)
    assert pipeline.assigner_takes_ignore(lambda frames, ignore=None: None) and pipeline.assigner_takes_ignore(lambda frames, **k: None)
    with pytest.raises(ValueError):
        pipeline.batch_from_dataset([], [], 'cpu', None, None, 10, ignore={'labels': []})
    with pytest.raises(ValueError):
        pipeline.batch_from_dataset([], [], 'cpu', None, None, 10, assigner=lambda frames: None, ignore={'labels': []})
