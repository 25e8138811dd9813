"""The rotated 3D IoU regression loss without a GPU: the two float64 restatements of tests/box_iou_ref.py
against each other (autograd against central differences of the world-coordinate clip), the kernel's own algorithm restated in
float64 against both and in f32 against the bars the GPU tests derive from it, the rejection rule of the cases, the switches of
the Python layers, and the new entry point of the built library (prototype, header, argument checks)."""
import ctypes
import math

import numpy as np
import pytest

import abi_header
import box_iou_cases as BC
import box_iou_ref as BR
import iou_head_ref as IR

NAME = 'mvx_box_iou_loss_frames'


# ---- the restatements -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('where', ['near', 'far'])
def test_autograd_restatement_agrees_with_central_differences_of_the_exact_clip(where):
    case = BC.pair_case(where)
    ref = BC.reference(where)
    out_b, grad_b, q_b = BR.loss_autograd(case, BC.WEIGHT)
    assert np.array_equal(grad_b, ref['grad'])
    np.testing.assert_allclose(q_b, ref['q'], rtol=0, atol=1e-12)
    np.testing.assert_allclose(out_b, ref['out'], rtol=1e-12, atol=1e-14)
    fd = BR.central_differences(case, BC.WEIGHT)
    err = float(np.abs(fd - grad_b).max())
    print('%s: autograd vs central differences %.2e, largest gradient %.3f' % (where, err, ref['grad_max']))
    assert err < 1e-6 and ref['grad_max'] > 0.1                  # the finite-difference noise of h = 1e-6
    listed = np.zeros(grad_b.shape, bool)
    for r in case['recs']:
        row, col = (r['f'] * case['l'] + r['x']) * case['w'] + r['y'], case['A'] + 7 * r['z']
        listed[row, col:col + 7] = True
        g = np.abs(grad_b[row, col:col + 7])
        assert g[[0, 1, 3, 4, 5, 6]].min() > 0                   # every pair has a gradient (z: only when a face is the min / max)
    assert float(np.abs(grad_b[~listed]).max()) == 0.0


@pytest.mark.parametrize('where', ['near', 'far'])
def test_kernel_algorithm_in_float64_is_the_reference_and_in_f32_within_the_bars(where):
    case = BC.pair_case(where)
    ref = BC.reference(where)
    q, out, grad = BR.kernel_restated(case, BC.WEIGHT, np.float64)
    taken = ref['q'] >= 0
    assert np.array_equal(q >= 0, taken) and int(taken.sum()) == sum(BC.QUOTA)
    print('%s: float64 restatement of the kernel: q %.2e, gradient %.2e, out %.2e; f32: q %.2e, gradient %.2e (of %.3f)'
          % (where, np.abs(q - ref['q']).max(), np.abs(grad - ref['grad']).max(), np.abs(out - ref['out']).max(),
             ref['worst_q'], ref['worst_grad'], ref['grad_max']))
    np.testing.assert_allclose(q, ref['q'], rtol=0, atol=1e-11)
    np.testing.assert_allclose(grad, ref['grad'], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(out, ref['out'], rtol=1e-11, atol=0)
    assert 0 < ref['q_bar'] <= BC.Q_BAR_MAX and 0 < ref['grad_bar'] <= BC.GRAD_BAR_MAX * ref['grad_max']
    assert BC.reference(where, 20)['q_bar'] == ref['q_bar']     # the row stride changes nothing


def test_pair_cases_meet_the_rejection_rule_and_their_shape():
    for where in ('near', 'far'):
        case = BC.pair_case(where)
        assert (case['F'], case['l'], case['w'], case['A']) == (3, 6, 5, 2) and case['gi'].shape[1] == BC.CAP > max(BC.QUOTA)
        assert [int(c) for c in case['counts'][:, 0]] == list(BC.QUOTA) and case['kept'] == sum(BC.QUOTA) <= case['drawn']
        seen = set()
        for r in case['recs']:
            reg, _ = BR.reg_row(case, r['f'], r['x'], r['y'], r['z'])
            b, g = BR.decode64(reg, case['anchors'][r['x'], r['y'], r['z']]), case['gts'][r['row']].astype(np.float64)
            assert BC.violations(b, g) == [] and IR.iou3d(b, g)[0] > 0.02
            assert (r['f'], r['x'], r['y'], r['z']) not in seen and r['row'] not in seen
            seen.update([(r['f'], r['x'], r['y'], r['z']), r['row']])
        xy = case['anchors'][..., :2].reshape(-1, 2)
        if where == 'far':
            assert abs(xy[:, 0].mean() - 69) < 0.5 and abs(xy[:, 1].mean() + 39) < 0.5
        wide = BC.pair_case(where, 20)
        assert wide['heads'].shape[1] == 20 and np.array_equal(wide['heads'][:, :16], case['heads'])
    # the rule rejects what it should
    b = np.array([0, 0, 0, 4.0, 2.0, 1.5, 0.3])
    assert BC.violations(b, b + np.array([0.5, 0.3, 0.2, 0, 0, 0.3, 0.2])) == []
    assert len(BC.violations(b, b)) == 3
    assert BC.violations(b, b + np.array([0.5, 0.3, 0.2, 0, 0, 0.3, math.pi / 2 + 0.005])) != []
    assert BC.violations(b, b + np.array([0.5, 0.3, 0.005, 0, 0, 0.3, 0.2])) != []


def test_edge_case_is_what_it_says():
    case = BC.edge_case()
    s = case['slots']
    q, out = BR.q_ref(case)
    k = lambda name: q[0, s[name]]
    assert k('exact') == 1.0 and abs(k('half_turn') - 1.0) < 1e-6
    assert k('touching') == k('apart') == k('no_vertical') == k('overflow') == 0.0
    assert k('outside_grid') == k('gi_high') == k('gi_negative') == -1.0 and (q[0, len(s):] == -1.0).all()
    assert k('twice_a') == k('twice_b') and 0.3 < k('twice_a') < 0.9 and 0.3 < k('plain') < 0.9
    taken = q[0][q[0] >= 0]
    assert len(taken) == 9 and abs(out[0, 0] - (9 - taken.sum()) / 12) < 1e-12 and abs(out[0, 1] - taken.mean()) < 1e-12
    q32, _, g32 = BR.kernel_restated(case, 1.0, np.float32)
    assert q32[0, s['touching']] == 0.0 and q32[0, s['exact']] == 1.0 and np.isfinite(g32).all()      # exactly, in f32


# ---- the Python layers ------------------------------------------------------------------------------------------------------------
def test_focal_loss_switch():
    from modules.Extension import MvxHipError
    from modules.voxelnet.FocalLoss import FocalLoss
    plain = FocalLoss()
    assert plain.iou_loss is False and plain.iou_loss_weight == 1.0 and plain.last_box_iou is None
    for kw in ({}, {'direction': True}, {'direction': True, 'iou': True}):
        crit = FocalLoss(iou_loss=True, iou_loss_weight=0.5, **kw)
        assert crit.iou_loss is True and crit.iou_loss_weight == 0.5 and crit.direction == bool(kw.get('direction'))
        assert crit.iou == bool(kw.get('iou')) and crit.last_box_iou is None
    for bad in (-0.1, float('nan')):
        with pytest.raises(MvxHipError, match='iou_loss_weight'):
            FocalLoss(iou_loss=True, iou_loss_weight=bad)
    with pytest.raises(MvxHipError, match='direction=True'):
        FocalLoss(iou=True, iou_loss=True)                       # the IoU head's own condition stays


def test_train_like_iou_loss_needs_the_fast_focal_path(capsys):
    import train_like
    ok = train_like.parse_args(['root', '--mode', 'fast', '--loss', 'focal', '--iou-loss', '--iou-loss-weight', '0.5'])
    assert ok.iou_loss and ok.iou_loss_weight == 0.5 and not ok.direction and not ok.iou_head
    both = train_like.parse_args(['root', '--mode', 'fast', '--loss', 'focal', '--direction', '--iou-head', '--iou-loss'])
    assert both.iou_loss and both.iou_head and both.iou_loss_weight == 1.0
    d = train_like.parse_args(['root'])
    assert not d.iou_loss and d.iou_loss_weight == 1.0
    for argv, text in ((['root', '--iou-loss'], '--iou-loss needs --mode fast --loss focal'),
                       (['root', '--mode', 'fast', '--iou-loss'], '--iou-loss needs --mode fast --loss focal'),
                       (['root', '--mode', 'fast', '--loss', 'voxel', '--iou-loss'], '--iou-loss needs --mode fast --loss focal'),
                       (['root', '--mode', 'fast', '--loss', 'focal', '--iou-loss', '--iou-loss-weight', '-1'],
                        '--iou-loss-weight must not be negative')):
        with pytest.raises(SystemExit) as e:
            train_like.parse_args(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err


# ---- the library ------------------------------------------------------------------------------------------------------------------
def test_entry_point_resolves_with_its_prototype_and_the_header_agrees():
    from modules import Extension as X
    i32, i64, f32, p = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    want = [p, i32, i32, i32, i32, i32, p, p, i64, p, p, i32, p, p, f32, p, i32, p, i32, p, p, p]
    fn = getattr(X.lib, NAME)
    assert hasattr(ctypes.CDLL(X.LIB_PATH), NAME) and fn.restype is i32 and list(fn.argtypes) == want
    ret, params = abi_header.declarations()[NAME]
    assert ret is i32 and [t for _, t in params] == list(X.PROTOTYPES[NAME][1]) == want
    assert abi_header.parameter_names(NAME) == ['heads', 'heads_ld', 'n_frames', 'l', 'w', 'anchors_per_loc', 'pos_idx', 'gi', 'cap',
                                                'counts', 'gts', 'gt_ld', 'gt_off', 'anchors', 'weight', 'd_heads', 'd_heads_ld',
                                                'loss_add', 'loss_add_ld', 'out', 'q_out', 'stream']
    assert X.ABI_VERSION == 10 and X.lib.mvx_abi_version() == 10             # an addition: not bumped


def test_entry_rejects_bad_arguments_before_any_launch():
    """Fake, never dereferenced device addresses and ONE bad argument: MVX_EINVAL (-1) before anything is launched."""
    from modules import Extension as X
    fake = 1 << 20
    names = abi_header.parameter_names(NAME)
    good = dict(heads_ld=20, n_frames=3, l=6, w=5, anchors_per_loc=2, cap=48, gt_ld=7, weight=1.0, d_heads_ld=24, loss_add_ld=4,
                stream=None)
    bad = [('heads', None), ('pos_idx', None), ('gi', None), ('counts', None), ('gts', None), ('gt_off', None), ('anchors', None),
           ('out', None), ('cap', 0), ('cap', -3), ('cap', 1 << 31), ('gt_ld', 6), ('anchors_per_loc', 0), ('anchors_per_loc', 5),
           ('n_frames', 0), ('n_frames', 17), ('l', 0), ('w', -1), ('heads_ld', 12), ('heads_ld', 18), ('d_heads_ld', 15),
           ('heads_ld', (1 << 31) // 90 + 3), ('d_heads_ld', (1 << 31) // 90 + 1), ('weight', -0.5), ('weight', float('nan')),
           ('loss_add_ld', 0), ('cap', (1 << 31) // 3 + 1), ('heads', fake + 8), ('heads', fake + 2), ('pos_idx', fake + 4),
           ('gi', fake + 4), ('counts', fake + 2), ('gts', fake + 1), ('gt_off', fake + 2), ('anchors', fake + 3),
           ('d_heads', fake + 2), ('loss_add', fake + 1), ('out', fake + 2), ('q_out', fake + 3)]
    for param, value in bad:
        assert param in names
        args = [value if n == param else good[n] if n in good else fake for n in names]
        assert getattr(X.lib, NAME)(*args) == -1, (param, value)
    # what is optional may be null together with a stride of 0 -- still refused for another reason, so nothing is launched
    args = [None if n in ('d_heads', 'loss_add', 'q_out') else 0 if n in ('d_heads_ld', 'loss_add_ld', 'cap') else good[n] if n in good
            else fake for n in names]
    assert getattr(X.lib, NAME)(*args) == -1
