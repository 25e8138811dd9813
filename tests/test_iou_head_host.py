"""The IoU-aware confidence head without a GPU: the float64 reference (tests/iou_head_ref.py) against direction_ref and
against autograd, the exact clip on boxes with known answers, the conditions of the cases, the model's optional fourth head
and its state-dict keys, the switches of the Python layers, and the two new entry points of the built library."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import abi_header
import direction_ref as DR
import iou_head_cases as IC
import iou_head_ref as IR

CASES = [('case1', False), ('case1', True), ('case4', False), ('case5', False), ('case3', False)]


# ---- the reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['case1', 'case4', 'case5'])
def test_reference_with_zero_weight_is_direction_ref(name):
    case = IC.with_iou(name)
    got = IR.iou_head_ref(case, iou_weight=0.0)
    want = DR.direction_ref(case)
    assert torch.equal(got[0][:, :3], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert float(got[0][:, 3].abs().max()) == 0.0 and float(got[3].abs().max()) == 0.0
    on = IR.iou_head_ref(case)                      # and with it on, the other three terms are still direction_ref's bit for bit
    assert torch.equal(on[0][:, :3], want[0]) and torch.equal(on[1], want[1]) and torch.equal(on[2], want[2])
    assert on[0].shape == (case['F'], 4) and float(on[0][:, 3].max()) > 0.0


def test_iou_of_a_box_with_itself_is_one_and_of_disjoint_boxes_zero():
    rng = np.random.default_rng(7)
    for _ in range(20):
        b = np.array([rng.uniform(-20, 20), rng.uniform(-20, 20), rng.uniform(-2, 0), rng.uniform(3, 5), rng.uniform(1.4, 2),
                      rng.uniform(1.3, 1.9), rng.uniform(-4, 4)])
        q, _ = IR.iou3d(b, b)
        assert abs(q - 1.0) < 1e-12
        far = b.copy()
        far[0] += 9.0                               # disjoint in the BEV though the circles of long boxes may touch
        assert IR.iou3d(b, far)[0] == 0.0
        above = b.copy()
        above[2] += b[5] + 0.01                     # same footprint, stacked: no vertical overlap
        q, (gap, ih, inter) = IR.iou3d(b, above)
        assert q == 0.0 and gap <= 0 and ih < 0 and abs(inter - b[3] * b[4]) < 1e-9


def test_clip_area_of_known_rectangles():
    unit = np.array([0, 0, 0, 2.0, 1.0, 1.0, 0.0])
    half = unit.copy()
    half[0] = 1.0                                   # shifted by half its length: overlap 1 x 1 x 1 of volumes 2 + 2
    assert abs(IR.iou3d(unit, half)[0] - 1.0 / 3.0) < 1e-12
    turned = unit.copy()
    turned[6] = math.pi / 2                         # a 2 x 1 and a 1 x 2 rectangle share the unit square
    assert abs(IR.clip_area(IR.quad64(unit), IR.quad64(turned)) - 1.0) < 1e-12
    diamond = np.array([0, 0, 0, math.sqrt(2), math.sqrt(2), 1.0, math.pi / 4])      # |x| + |y| <= 1
    square = np.array([0, 0, 0, 1.5, 1.5, 1.0, 0.0])                                 # minus four corner triangles of legs 0.5
    assert abs(IR.clip_area(IR.quad64(diamond), IR.quad64(square)) - 1.75) < 1e-12
    assert abs(IR.clip_area(IR.quad64(square), IR.quad64(diamond)[::-1]) - 1.75) < 1e-12      # either order, either orientation


@pytest.mark.parametrize('name,saturated', CASES)
def test_analytic_gradient_matches_autograd(name, saturated):
    case = IC.with_iou(name, saturated)
    losses, _, _, d_iou, q = IR.iou_head_ref(case, iou_weight=0.7)
    a_losses, a_iou = IR.iou_head_autograd(case, iou_weight=0.7, q=q)
    np.testing.assert_allclose(losses[:, 3].numpy(), a_losses.numpy(), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(d_iou.numpy(), a_iou.numpy(), rtol=1e-10, atol=1e-12)
    assert bool(torch.isfinite(losses).all()) and float(d_iou.abs().max()) > 0.0


@pytest.mark.parametrize('name,saturated', CASES)
def test_cases_meet_their_conditions(name, saturated):
    case = IC.with_iou(name, saturated)
    bad, recs = IC.conditions(case)
    assert bad == [] and len(recs) == len(case['recs'])
    qs = np.array([r['q'] for r in recs])
    assert ((qs >= 0) & (qs <= 1)).all()
    zero = [r for r in recs if IR.must_be_zero(r)]
    assert all(r['q'] == 0.0 for r in zero) and len(zero) >= 3
    if name == 'case3':                             # the strided loop: more than one workgroup per frame, a ragged tail
        n = int(case['counts'][0, 0])
        assert n > 256 and n % 128 != 0 and case['gi'].shape[1] > 256
    if name == 'case1':                             # duplicates, an empty frame, a frame without positives
        assert tuple(case['pos'][0, :, 0]) == tuple(case['pos'][0, :, 1]) and case['gi'][0, 0] != case['gi'][0, 1]
        assert tuple(case['counts'][1]) == (0, 0) and case['counts'][2, 0] == 0
    if saturated:
        assert set(np.unique(case['iou'])) == {-90.0, -20.0, 0.0, 20.0, 90.0}


def test_q_in_f32_arithmetic_is_close_to_the_exact_clip():
    case = IC.with_iou('case5')
    q32 = IR.q_f32(case, case['recs'])
    q64 = np.array([r['q'] for r in case['recs']])
    ok = ~np.isnan(q32)
    assert ok.sum() >= 16 and float(np.abs(q32[ok] - q64[ok]).max()) < 1e-4


def test_decode_case_meets_its_conditions():
    import mvx_oracle as O
    case = IC.decode_case()
    assert IC._decode_ok(case, 0.5, O)
    for f in range(case['F']):
        c, u = case['cls'][f].reshape(-1), case['iou'][f].reshape(-1)
        sp = case['special'][f]
        keep, scores, n = IR.candidates(c, u, 0.5, case['score_thr'], 1000)
        assert n == len(keep) == 4 and sp['nan'] not in keep and sp['low'] not in keep
        pos = {int(a): i for i, a in enumerate(keep)}
        lo, hi = sorted(sp['tie'])
        assert pos[lo] + 1 == pos[hi] and scores[pos[lo]] == scores[pos[hi]]         # the index tie: lowest first
        assert (np.diff(scores) <= 0).all()
        only_u, _, _ = IR.candidates(c, u, 1.0, case['score_thr'], 1000)               # a = 1: the IoU logit alone
        assert list(u[only_u]) == sorted(u[only_u], reverse=True)
    assert IC.decode_heads(case).shape == (60, 20)


# ---- the model --------------------------------------------------------------------------------------------------------------
IOU_KEYS = ['backbone.rpn.iou.weight', 'backbone.rpn.iou.bias']


@functools.lru_cache(maxsize=None)
def _models():
    from MVXNet import MVXNet
    torch.manual_seed(0)
    plain = MVXNet()
    torch.manual_seed(0)
    direct = MVXNet(direction=True)
    torch.manual_seed(0)
    return plain, direct, MVXNet(direction=True, iou=True)


def test_state_dict_keys_of_the_three_models():
    plain, direct, both = _models()
    pk, dk, bk = (list(m.state_dict()) for m in (plain, direct, both))
    assert not any('.iou.' in k for k in pk + dk) and not hasattr(plain.backbone.rpn, 'iou') and not hasattr(direct.backbone.rpn, 'iou')
    assert [k for k in bk if k not in dk] == IOU_KEYS and [k for k in bk if k in dk] == dk
    assert [k for k in dk if k not in pk] == ['backbone.rpn.dir.weight', 'backbone.rpn.dir.bias']
    h = both.backbone.rpn.iou
    assert isinstance(h, torch.nn.Conv2d) and tuple(h.weight.shape) == (2, 768, 1, 1) and tuple(h.bias.shape) == (2,)
    assert float(h.bias.detach().abs().max()) == 0.0                               # initWeights, like dir
    bound = math.sqrt(6.0 / (768 + 2))
    assert 0.5 * bound < float(h.weight.detach().abs().max()) <= bound
    assert [n for n, _ in both.backbone.rpn.named_children()][-4:] == ['cls', 'reg', 'dir', 'iou']
    with pytest.raises(RuntimeError):
        both.load_state_dict(direct.state_dict())
    with pytest.raises(RuntimeError):
        direct.load_state_dict(both.state_dict())


def test_iou_head_needs_the_direction_head():
    from MVXNet import MVXNet
    from modules.Extension import MvxHipError
    from modules.voxelnet import Pipe
    from modules.voxelnet.FocalLoss import FocalLoss
    from modules.voxelnet.VoxelNet import VoxelNet
    for build in (lambda: Pipe.RPN(iou=True), lambda: VoxelNet(iou=True), lambda: MVXNet(iou=True), lambda: FocalLoss(iou=True)):
        with pytest.raises(MvxHipError, match='direction=True'):
            build()
    assert hasattr(Pipe.RPN(direction=True, iou=True), 'iou')
    plain = FocalLoss()
    assert plain.iou is False and plain.iou_weight == 1.0
    crit = FocalLoss(direction=True, iou=True, iou_weight=0.5)
    assert crit.iou is True and crit.direction is True and crit.iou_weight == 0.5


def test_postprocess_iou_switch_without_the_columns_is_an_error():
    from modules import detect
    from modules.Extension import MvxHipError
    anchors = torch.zeros((2, 3, 14))
    with pytest.raises(MvxHipError, match='iou=True'):
        detect.postprocess(torch.zeros((6, 16)), anchors, 1, 2, 3, iou=True)
    with pytest.raises(MvxHipError, match='iou=True'):
        detect.postprocess((torch.zeros((1, 2, 2, 3)), torch.zeros((1, 14, 2, 3)), torch.zeros((1, 2, 2, 3))), anchors, 1, 2, 3, iou=True)
    with pytest.raises(MvxHipError, match='iou_alpha'):
        detect.postprocess(torch.zeros((6, 20)), anchors, 1, 2, 3, iou=True, iou_alpha=1.5)
    views = detect._views(torch.zeros((6, 20)), 1, 2, 3)
    assert len(views) == 4 and views[3].shape == (1, 2, 3, 2) and detect._views(torch.zeros((6, 16)), 1, 2, 3)[2:] == (None, None)


def test_train_like_iou_head_needs_direction(capsys):
    import train_like
    ok = train_like.parse_args(['root', '--direction', '--iou-head', '--mode', 'fast', '--loss', 'focal', '--iou-weight', '0.5'])
    assert ok.iou_head and ok.direction and ok.iou_weight == 0.5
    d = train_like.parse_args(['root'])
    assert not d.iou_head and d.iou_weight == 1.0
    with pytest.raises(SystemExit) as e:
        train_like.parse_args(['root', '--iou-head', '--mode', 'fast', '--loss', 'focal'])
    assert e.value.code == 2 and '--iou-head needs --direction' in capsys.readouterr().err
    import detect_like
    import visualize_like
    assert detect_like.parse_args(['root']).iou_alpha == 0.5 and detect_like.parse_args(['root', '--iou-alpha', '0.25']).iou_alpha == 0.25
    assert visualize_like.parse_args(['root', '--iou-alpha', '1']).iou_alpha == 1.0


# ---- the library ------------------------------------------------------------------------------------------------------------
NEW = ('mvx_focal_loss_iou_frames_workspace_bytes', 'mvx_focal_loss_iou_frames', 'mvx_detect_frames_iou')


def test_new_entry_points_resolve_with_their_prototypes():
    from modules import Extension as X
    i32, i64, f32, p, sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    want = {
        NEW[0]: (i64, [i32] * 5 + [i64]),
        NEW[1]: (i32, [p, i32, p, i32, p, i32, i32, i32, i32, i32, p, p, p, i64, p, p, i32, p, p] + [f32] * 7
                 + [p, i32, p, i32, p, i32, p, p, p, i64, p]),
        NEW[2]: (i32, [p] + [i64] * 4 + [p] + [i64] * 4 + [p] + [i64] * 4 + [f32, p] + [i64] * 4 + [f32, p] + [i32] * 4 + [f32, f32]
                 + [i32] * 3 + [p] * 10 + [sz, p]),
    }
    lib = ctypes.CDLL(X.LIB_PATH)
    for name, (res, args) in want.items():
        fn = getattr(X.lib, name)
        assert hasattr(lib, name) and fn.restype is res and list(fn.argtypes) == args, name
    # pure host code: the direction entry's workspace plus F * min(ceil(cap / 128), 64) doubles
    base = X.lib.mvx_focal_loss_dir_frames_workspace_bytes(3, 6, 5, 2, 20)
    for cap, nq in ((1, 1), (128, 1), (129, 2), (301, 3), (128 * 64, 64), (10 ** 6, 64)):
        assert X.lib.mvx_focal_loss_iou_frames_workspace_bytes(3, 6, 5, 2, 20, cap) == base + 3 * nq * 8, cap
    assert X.lib.mvx_focal_loss_iou_frames_workspace_bytes(3, 6, 5, 2, 18, 12) == 0         # rows are float4 multiples
    assert X.lib.mvx_focal_loss_iou_frames_workspace_bytes(3, 6, 5, 2, 20, 0) == 0


def test_header_matches_the_prototypes_of_the_new_entry_points():
    from modules import Extension as X
    for name in NEW:
        ret, params = abi_header.declarations()[name]
        assert ret is (ctypes.c_int64 if name.endswith('_bytes') else ctypes.c_int32)
        assert [t for _, t in params] == list(X.PROTOTYPES[name][1]), name
    old, new = abi_header.parameter_names('mvx_detect_frames_dir'), abi_header.parameter_names('mvx_detect_frames_iou')
    assert [n for n in new if n not in old] == ['iou', 'iou_sf', 'iou_sl', 'iou_sw', 'iou_sa', 'iou_alpha']
    assert [n for n in new if n in old] == old
    old, new = abi_header.parameter_names('mvx_focal_loss_dir_frames'), abi_header.parameter_names('mvx_focal_loss_iou_frames')
    assert [n for n in new if n not in old] == ['iou', 'iou_ld', 'iou_weight', 'd_iou', 'd_iou_ld', 'q_out']
    assert [n for n in new if n in old] == old


def test_loss_entry_rejects_bad_arguments_before_any_launch():
    """Dummy aligned host pointers and ONE bad argument: MVX_EINVAL (-1) -- a launch on these pointers would fault."""
    from modules import Extension as X
    buf = ctypes.create_string_buffer(4096 + 64)
    dummy = (ctypes.addressof(buf) + 63) & ~63
    names = abi_header.parameter_names('mvx_focal_loss_iou_frames')
    need = X.lib.mvx_focal_loss_iou_frames_workspace_bytes(2, 6, 5, 2, 20, 8)
    good = dict(heads_ld=20, dir_ld=20, iou_ld=20, n_frames=2, l=6, w=5, anchors_per_loc=2, cap=8, gt_ld=7, alpha=0.25, gamma=2.0,
                cls_weight=1.0, reg_weight=2.0, dir_weight=0.2, dir_offset=math.pi / 4, iou_weight=1.0, d_heads_ld=20, d_dir_ld=20,
                d_iou_ld=20, workspace_bytes=need, stream=None)
    bad = [('heads', None), ('dir', None), ('iou', None), ('heads_ld', 18), ('heads_ld', 12), ('d_heads_ld', 18), ('d_heads_ld', 12),
           ('dir_ld', 1), ('iou_ld', 1), ('d_dir_ld', 1), ('d_iou_ld', 1), ('d_dir', None), ('d_iou', None), ('d_heads', None),
           ('dir', dummy + 2), ('iou', dummy + 2), ('d_iou', dummy + 1), ('q_out', dummy + 2), ('d_heads', dummy + 8), ('n_frames', 17),
           ('n_frames', 0), ('anchors_per_loc', 5), ('workspace_bytes', need - 1), ('workspace', None), ('losses', None), ('gt_ld', 6),
           ('cap', 0), ('cap', 1 << 31), ('alpha', 1.5), ('gamma', -1.0), ('dir_weight', -0.1), ('dir_offset', float('nan')),
           ('iou_weight', -0.1), ('iou_weight', float('nan')), ('pos_idx', None), ('gi', None), ('counts', None), ('anchors', None)]
    # the workspace of the direction entry alone is too small: the F * nq partials are part of the contract
    bad.append(('workspace_bytes', X.lib.mvx_focal_loss_dir_frames_workspace_bytes(2, 6, 5, 2, 20)))
    for param, value in bad:
        assert param in names
        args = [value if n == param else good[n] if n in good else dummy for n in names]
        assert X.lib.mvx_focal_loss_iou_frames(*args) == -1, (param, value)


def test_detect_entry_rejects_bad_arguments_before_any_launch():
    """Fake, never dereferenced device addresses and ONE bad argument: every call is refused before anything is launched."""
    from modules import Extension as X
    fake = 1 << 20
    names = abi_header.parameter_names('mvx_detect_frames_iou')
    good = dict(cls_sf=3520 * 20, cls_sl=4000, cls_sw=20, cls_sa=1, reg_sf=3520 * 20, reg_sl=4000, reg_sw=20, reg_sc=1,
                dir_sf=3520 * 20, dir_sl=4000, dir_sw=20, dir_sa=1, dir_offset=math.pi / 4, iou_sf=3520 * 20, iou_sl=4000, iou_sw=20,
                iou_sa=1, iou_alpha=0.5, n_frames=4, l=176, w=200, anchors_per_loc=2, score_thr=0.05, iou_thr=0.01, pre_max=1000,
                post_max=100, decode=0, dbg_idx=None, dbg_boxes=None, dbg_corners=None, workspace_bytes=1 << 40, stream=None)
    bad = [('iou_alpha', -0.01), ('iou_alpha', 1.01), ('iou_alpha', float('nan')), ('iou_alpha', float('inf')),
           ('dir_offset', float('nan')), ('pre_max', 4097), ('pre_max', 0), ('post_max', 1001), ('iou_thr', 0.0), ('iou_thr', 1.0),
           ('score_thr', 1.0), ('score_thr', -0.1), ('n_frames', 0), ('n_frames', 17), ('boxes', None), ('scores', None),
           ('anchor_idx', None), ('counts', None), ('n_candidates', None), ('status', None), ('cls', None), ('reg', None),
           ('anchors', None), ('workspace', None), ('decode', 2), ('workspace_bytes', 1024), ('dbg_idx', fake)]
    for param, value in bad:
        assert param in names
        args = [value if n == param else good[n] if n in good else fake for n in names]
        assert X.lib.mvx_detect_frames_iou(*args) == -1, (param, value)
    # with a = 0 the head is not read: the bad alpha is still refused when the head is null
    args = [float('nan') if n == 'iou_alpha' else None if n == 'iou' else good[n] if n in good else fake for n in names]
    assert X.lib.mvx_detect_frames_iou(*args) == -1
