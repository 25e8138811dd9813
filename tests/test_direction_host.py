"""The direction classifier and the sine angle loss without a GPU: the float64 reference (tests/direction_ref.py) against
focal_ref and against autograd, the encode -> decode round trip of the yaw, the model's optional third head and its
state-dict keys, and the two new entry points of the built library."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import abi_header
import direction_cases as DC
import direction_ref as DR
import focal_cases as C
import focal_ref as R


@functools.lru_cache(maxsize=None)
def _case(name, saturated=False):
    return DC.with_direction(name, saturated=saturated)


@pytest.mark.parametrize('name', ['case1', 'case4', 'case5'])
def test_reference_with_direction_off_is_focal_ref(name):
    case = _case(name)
    got = DR.direction_ref(case, direction=False)
    want = R.focal_ref(case)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # and with it on, the classification loss and gradient columns are still focal_ref's, bit for bit
    on = DR.direction_ref(case)
    A = case['A']
    assert torch.equal(on[0][:, 0], want[0][:, 0]) and torch.equal(on[1][:, :A], want[1][:, :A])
    assert on[0].shape == (case['F'], 3)


@pytest.mark.parametrize('name,saturated', [('case1', False), ('case1', True), ('case4', False), ('case5', False), ('case3', False)])
@pytest.mark.parametrize('dir_offset', DC.OFFSETS)
def test_analytic_gradients_match_autograd(name, saturated, dir_offset):
    case = _case(name, saturated)
    losses, d_heads, d_dir, _ = DR.direction_ref(case, dir_offset=dir_offset)
    a_losses, a_heads, a_dir = DR.direction_autograd(case, dir_offset=dir_offset)
    np.testing.assert_allclose(losses.numpy(), a_losses.numpy(), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(d_heads.numpy(), a_heads.numpy(), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(d_dir.numpy(), a_dir.numpy(), rtol=1e-10, atol=1e-10)
    assert bool(torch.isfinite(losses).all()) and float(losses[:, 2].max()) > 0.0
    assert float(d_dir.abs().max()) > 0.0


def test_case1_counts_duplicates_and_skips_frames_without_positives():
    case = _case('case1')
    losses, d_heads, d_dir, (positive, _) = DR.direction_ref(case)
    assert float(losses[1, 1]) == 0.0 and float(losses[1, 2]) == 0.0 and float(losses[2, 2]) == 0.0
    d4 = d_dir.reshape(case['F'], case['l'], case['w'], case['A'])
    assert float(d4[torch.from_numpy(~positive)].abs().max()) == 0.0
    # anchor (1,2,0) is listed twice with two boxes: its direction gradient is the sum of both entries'
    x = float(case['dir'].reshape(case['F'], case['l'], case['w'], case['A'])[0, 1, 2, 0])
    bits = DR.direction_bit(case['gts'][[0, 1], 6], math.pi / 4)
    want = 0.2 / 4 * sum(1.0 / (1.0 + math.exp(-x)) - int(b) for b in bits)
    assert math.isclose(float(d4[0, 1, 2, 0]), want, rel_tol=1e-12)


def test_angle_term_vanishes_at_multiples_of_pi():
    """A regression that is k half turns off costs nothing on the angle column and has no gradient there."""
    base = _case('case4')
    F, l, w, A = base['F'], base['l'], base['w'], base['A']
    for k in (-3, -1, 0, 1, 2):
        case = dict(base)
        heads = np.asarray(base['heads'], np.float64).reshape(F, l, w, 8 * A).copy()
        an = base['anchors'].astype(np.float64)
        for f in range(F):
            px, py, pz, rows, _ = DR._entries(base, f)
            for x, y, z, g in zip(px, py, pz, rows):
                t = R.regression_targets(torch.from_numpy(base['gts'][g:g + 1, :7].astype(np.float64)), torch.from_numpy(an[x, y, z][None]))
                heads[f, x, y, A + 7 * z:A + 7 * z + 7] = t[0].numpy()
                heads[f, x, y, A + 7 * z + 6] += k * math.pi
        case['heads'] = heads.reshape(F * l * w, 8 * A)
        losses, d_heads, _, _ = DR.direction_ref(case)
        assert float(losses[:, 1].abs().max()) < 1e-24, k
        assert float(d_heads[:, A:].abs().max()) < 1e-12, k


def _grid():
    """Yaws over [-3 pi / 2, pi / 2], with points 1e-3 on either side of every bin boundary of both offsets."""
    pts = list(np.linspace(-1.5 * math.pi, 0.5 * math.pi, 97))
    for off in DC.OFFSETS:
        for k in range(-3, 3):
            b = off + k * math.pi
            if -1.5 * math.pi <= b - 1e-3 and b + 1e-3 <= 0.5 * math.pi:
                pts += [b - 1e-3, b + 1e-3]
    return np.array(pts)


@pytest.mark.parametrize('dir_offset', DC.OFFSETS)
@pytest.mark.parametrize('shift', [0.0, math.pi, -math.pi])
def test_encode_decode_round_trip(dir_offset, shift):
    """theta' = g6 (mod 2 pi) for a perfect regression or one half a turn off, given the box's own bit; in [-pi, pi)."""
    g6 = _grid()
    g6 = g6[DR.fold_margin(g6, dir_offset) >= 0.5e-3]          # the boundary itself belongs to neither side
    assert g6.shape[0] >= 97
    for an6 in (0.0, math.pi / 2):
        theta = (g6 - an6) + shift + an6                       # encode, the regression's error, decode
        bit = DR.direction_bit(g6, dir_offset)
        got = DR.fold_yaw(theta, np.where(bit == 1, 3.0, -3.0), dir_offset)
        assert (got >= -math.pi).all() and (got < math.pi).all()
        err = DR.wrap_pi(got - g6)
        assert np.abs(err).max() < 1e-9, (dir_offset, shift, an6)
        # the wrong bit is exactly half a turn away
        wrong = DR.fold_yaw(theta, np.where(bit == 1, -3.0, 3.0), dir_offset)
        assert np.abs(np.abs(DR.wrap_pi(wrong - g6)) - math.pi).max() < 1e-9


def test_decode_cases_meet_their_conditions():
    for off in DC.OFFSETS:
        case = DC.decode_case(off)
        assert len(case['planted']) == 2 and all(len(fr) == 6 for fr in case['planted'])
        assert {p['bit'] for fr in case['planted'] for p in fr} == {0, 1}
        assert DC.decode_heads(case).shape == (60, 20) and DC.decode_heads(case, with_dir=False).shape == (60, 16)


# ---- the model ------------------------------------------------------------------------------------------------------------
DIR_KEYS = ['backbone.rpn.dir.weight', 'backbone.rpn.dir.bias']


@functools.lru_cache(maxsize=None)
def _models():
    from MVXNet import MVXNet
    torch.manual_seed(0)
    plain = MVXNet()
    torch.manual_seed(0)
    again = MVXNet()
    torch.manual_seed(0)
    return plain, again, MVXNet(direction=True)


def test_state_dict_keys():
    from modules.voxelnet import Pipe
    plain, again, direct = _models()
    keys = list(plain.state_dict())
    assert not any('.dir.' in k for k in keys) and not hasattr(plain.backbone.rpn, 'dir')
    assert [n for n, _ in plain.backbone.rpn.named_children()] == ['blk1', 'blk2', 'blk3', 'deconv1', 'deconv2', 'deconv3', 'cls', 'reg']
    dkeys = list(direct.state_dict())
    assert [k for k in dkeys if k not in keys] == DIR_KEYS and [k for k in dkeys if k in keys] == keys
    d = direct.backbone.rpn.dir
    assert isinstance(d, torch.nn.Conv2d) and tuple(d.weight.shape) == (2, 768, 1, 1) and tuple(d.bias.shape) == (2,)
    assert float(d.bias.abs().max()) == 0.0                                      # initWeights, like cls and reg
    bound = math.sqrt(6.0 / (768 + 2))
    assert 0.5 * bound < float(d.weight.abs().max()) <= bound
    assert list(Pipe.RPN().state_dict()) == [k[len('backbone.rpn.'):] for k in keys if k.startswith('backbone.rpn.')]


def test_plain_checkpoint_round_trip_is_unchanged():
    plain, again, direct = _models()
    sd = plain.state_dict()
    for k, v in again.state_dict().items():                                      # the same seed builds the same plain model
        assert torch.equal(v, sd[k]), k
    fresh = {k: v.clone() + 1.0 if v.is_floating_point() else v.clone() for k, v in sd.items()}
    res = again.load_state_dict(fresh)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in again.state_dict().items():
        assert torch.equal(v, fresh[k]), k
    with pytest.raises(RuntimeError):                                            # a plain checkpoint lacks the two keys
        direct.load_state_dict(sd)
    with pytest.raises(RuntimeError):
        plain.load_state_dict(direct.state_dict())


def test_head_layout_recognises_both_widths():
    from modules import rpn_frames as rf
    from modules.Extension import MvxHipError
    assert [rf.head_layout(n) for n in (8, 16, 24, 32)] == [(1, False), (2, False), (3, False), (4, False)]
    assert [rf.head_layout(n) for n in (12, 20, 28, 36)] == [(1, True), (2, True), (3, True), (4, True)]
    for bad in (4, 18, 27, 40, 44):
        with pytest.raises(MvxHipError):
            rf.head_layout(bad)
    heads = torch.arange(2 * 3 * 20, dtype=torch.float32).reshape(6, 20)
    score, reg = rf.split_heads(heads, 1, 2, 3)
    assert score.shape == (1, 2, 2, 3) and reg.shape == (1, 14, 2, 3)
    assert torch.equal(reg[0, :, 0, 0], heads[0, 2:16])


def test_focal_loss_direction_arguments():
    from modules.voxelnet.FocalLoss import FocalLoss
    plain = FocalLoss()
    assert plain.direction is False and plain.dir_weight == 0.2 and plain.dir_offset == math.pi / 4
    d = FocalLoss(direction=True, dir_weight=0.5, dir_offset=0.0)
    assert d.direction is True and d.dir_weight == 0.5 and d.dir_offset == 0.0


def test_train_like_direction_needs_fast_mode_and_focal_loss(capsys):
    import train_like
    ok = train_like.parse_args(['root', '--direction', '--mode', 'fast', '--loss', 'focal', '--dir-weight', '0.3', '--dir-offset', '0.5'])
    assert ok.direction and ok.dir_weight == 0.3 and ok.dir_offset == 0.5
    assert not train_like.parse_args(['root']).direction
    for argv in (['root', '--direction', '--mode', 'fast', '--loss', 'voxel'], ['root', '--direction', '--loss', 'focal'],
                 ['root', '--direction', '--mode', 'module']):
        with pytest.raises(SystemExit) as e:
            train_like.parse_args(argv)
        assert e.value.code == 2
        assert '--direction needs --mode fast --loss focal' in capsys.readouterr().err


# ---- the library ----------------------------------------------------------------------------------------------------------
def test_new_entry_points_resolve_with_their_prototypes():
    from modules import Extension as X
    i32, i64, f32, p, sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    want = {
        'mvx_focal_loss_dir_frames_workspace_bytes': (i64, [i32] * 5),
        'mvx_focal_loss_dir_frames': (i32, [p, i32, p, i32, i32, i32, i32, i32, p, p, p, i64, p, p, i32, p, p] + [f32] * 6
                                      + [p, i32, p, i32, p, p, i64, p]),
        'mvx_detect_frames_dir': (i32, [p] + [i64] * 4 + [p] + [i64] * 4 + [p] + [i64] * 4 + [f32, p] + [i32] * 4 + [f32, f32]
                                  + [i32] * 3 + [p] * 10 + [sz, p]),
    }
    for name, (res, args) in want.items():
        fn = getattr(X.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    # pure host code: the workspace of the wide rows is the plain one plus the partial sums of the extra float4 per row
    plain = X.lib.mvx_focal_loss_frames_workspace_bytes(3, 6, 5, 2)
    assert X.lib.mvx_focal_loss_dir_frames_workspace_bytes(3, 6, 5, 2, 16) == plain
    assert X.lib.mvx_focal_loss_dir_frames_workspace_bytes(3, 6, 5, 2, 20) >= plain
    assert X.lib.mvx_focal_loss_dir_frames_workspace_bytes(3, 6, 5, 2, 18) == 0         # rows are float4 multiples
    assert X.lib.mvx_focal_loss_dir_frames_workspace_bytes(3, 6, 5, 2, 12) == 0         # narrower than [cls | reg]


def test_header_matches_the_prototypes_of_the_new_entry_points():
    from modules import Extension as X
    for name in ('mvx_focal_loss_dir_frames_workspace_bytes', 'mvx_focal_loss_dir_frames', 'mvx_detect_frames_dir'):
        ret, params = abi_header.declarations()[name]
        assert ret is (ctypes.c_int64 if name.endswith('_bytes') else ctypes.c_int32)
        assert [t for _, t in params] == list(X.PROTOTYPES[name][1]), name
    old = abi_header.parameter_names('mvx_detect_frames')
    new = abi_header.parameter_names('mvx_detect_frames_dir')
    assert [n for n in new if n not in old] == ['dir', 'dir_sf', 'dir_sl', 'dir_sw', 'dir_sa', 'dir_offset']
    assert [n for n in new if n in old] == old


def test_loss_entry_rejects_bad_arguments_before_any_launch():
    """Dummy aligned host pointers and ONE bad argument: MVX_EINVAL (-1) -- a launch on these pointers would fault."""
    from modules import Extension as X
    buf = ctypes.create_string_buffer(4096 + 64)
    dummy = (ctypes.addressof(buf) + 63) & ~63
    names = abi_header.parameter_names('mvx_focal_loss_dir_frames')
    need = X.lib.mvx_focal_loss_dir_frames_workspace_bytes(2, 6, 5, 2, 20)
    good = dict(heads_ld=20, dir_ld=20, n_frames=2, l=6, w=5, anchors_per_loc=2, cap=8, gt_ld=7, alpha=0.25, gamma=2.0,
                cls_weight=1.0, reg_weight=2.0, dir_weight=0.2, dir_offset=math.pi / 4, d_heads_ld=20, d_dir_ld=20,
                workspace_bytes=need, stream=None)
    bad = [('heads', None), ('dir', None), ('heads_ld', 18), ('heads_ld', 12), ('d_heads_ld', 18), ('d_heads_ld', 12), ('dir_ld', 1),
           ('d_dir_ld', 1), ('d_dir', None), ('d_heads', None), ('dir', dummy + 2), ('d_heads', dummy + 8), ('n_frames', 17),
           ('anchors_per_loc', 5), ('workspace_bytes', need - 1), ('workspace', None), ('losses', None), ('gt_ld', 6), ('cap', 0),
           ('alpha', 1.5), ('gamma', -1.0), ('dir_weight', -0.1), ('dir_offset', float('nan'))]
    for param, value in bad:
        assert param in names
        args = [value if n == param else good[n] if n in good else dummy for n in names]
        assert X.lib.mvx_focal_loss_dir_frames(*args) == -1, (param, value)
