"""Host side of the focal loss (no GPU): the C entry's declaration, size query and argument checks, the packing of the
per-frame targets, the float64 reference's simplest closed form, and train_like.py's flags."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import abi_header
import focal_cases as C
import focal_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'mvxnet-makise_amd')


def test_header_matches_the_prototypes():
    from modules import Extension as X
    for name, ret_type in (('mvx_focal_loss_frames_workspace_bytes', ctypes.c_int64), ('mvx_focal_loss_frames', ctypes.c_int32)):
        ret, params = abi_header.declarations()[name]
        assert name in X.PROTOTYPES and hasattr(X.lib, name)
        assert X.PROTOTYPES[name][0] is ret_type and ret is ret_type
        assert [t for _, t in params] == list(X.PROTOTYPES[name][1]), name
    names = abi_header.parameter_names('mvx_focal_loss_frames')
    for n in ('heads', 'n_frames', 'anchors_per_loc', 'pos_idx', 'neg_idx', 'gi', 'cap', 'counts', 'gts', 'gt_ld', 'gt_off', 'anchors',
              'alpha', 'gamma', 'cls_weight', 'reg_weight', 'd_heads', 'losses', 'workspace', 'workspace_bytes', 'stream'):
        assert n in names, n
    assert X.lib.mvx_abi_version() == 10


def test_workspace_query():
    from modules import Extension as X
    q = X.lib.mvx_focal_loss_frames_workspace_bytes
    full = q(4, 176, 200, 2)
    assert full >= 4 * 176 * 200 * 2              # at least the flag byte per anchor
    assert q(1, 176, 200, 2) < full
    assert q(0, 176, 200, 2) == 0 and q(17, 176, 200, 2) == 0
    assert q(4, 176, 200, 0) == 0 and q(4, 176, 200, 5) == 0
    assert q(16, 2, 3, 1) > 0 and q(1, 1, 1, 4) > 0


def test_entry_rejects_bad_arguments_before_any_launch():
    """Dummy 64-byte aligned host pointers and ONE bad argument: the call must come back with MVX_EINVAL (-1) -- a launch on
    these pointers would fault, and without a GPU it would return a HIP error instead."""
    from modules import Extension as X
    buf = ctypes.create_string_buffer(4096 + 64)
    dummy = (ctypes.addressof(buf) + 63) & ~63
    names = abi_header.parameter_names('mvx_focal_loss_frames')
    need = X.lib.mvx_focal_loss_frames_workspace_bytes(2, 6, 5, 2)
    good = dict(n_frames=2, l=6, w=5, anchors_per_loc=2, cap=8, gt_ld=7, alpha=0.25, gamma=2.0, cls_weight=1.0, reg_weight=2.0,
                workspace_bytes=need, stream=None)
    bad = [('heads', None), ('n_frames', 17), ('n_frames', 0), ('anchors_per_loc', 5), ('anchors_per_loc', 0), ('workspace_bytes', need - 1),
           ('workspace_bytes', 0), ('workspace', None), ('losses', None), ('counts', None), ('gt_off', None), ('pos_idx', None),
           ('gt_ld', 6), ('cap', 0), ('alpha', 1.5), ('gamma', -1.0)]
    for param, value in bad:
        assert param in names
        args = [value if n == param else good[n] if n in good else dummy for n in names]
        assert X.lib.mvx_focal_loss_frames(*args) == -1, (param, value)


def test_pack_targets_shapes_offsets_and_counts():
    from modules.voxelnet.FocalLoss import FocalLoss
    cpu = torch.device('cpu')
    g0, g2, g3 = torch.arange(14.).reshape(2, 7), torch.arange(7.).reshape(1, 7) + 100, torch.arange(21.).reshape(3, 7) + 200
    t0 = ((np.array([1, 2, 3]), np.array([4, 5, 6]), np.array([0, 1, 0])),
          ([1, 2, 3, 9, 9], [4, 5, 6, 8, 8], [0, 1, 0, 1, 1]), np.array([1, 0, 1]), g0)
    empty = np.zeros((0,), np.int64)
    t2 = ((empty, empty, empty), (torch.tensor([7, 8]), torch.tensor([1, 0]), torch.tensor([1, 1])), empty, g2)       # no positive
    t3 = ((torch.tensor([5]), torch.tensor([4]), torch.tensor([1])), (torch.tensor([5]), torch.tensor([4]), torch.tensor([1])),
          torch.tensor([2]), g3)
    packed, has_reg = FocalLoss.pack_targets([t0, None, t2, t3], cpu)
    assert has_reg == [True, False, False, True]
    cap = 5
    assert packed.pos_idx.shape == (4, 3, cap) and packed.neg_idx.shape == (4, 3, cap) and packed.gi.shape == (4, cap)
    assert packed.pos_idx.dtype == packed.neg_idx.dtype == packed.gi.dtype == torch.int64
    assert packed.counts.dtype == packed.gt_off.dtype == torch.int32 and packed.gts.dtype == torch.float32
    assert packed.counts.tolist() == [[3, 5], [0, 0], [0, 2], [1, 1]]
    assert packed.gt_off.tolist() == [0, 2, 2, 3, 6]
    assert torch.equal(packed.gts, torch.cat([g0, g2, g3]))
    assert packed.pos_idx[0, :, :3].tolist() == [[1, 2, 3], [4, 5, 6], [0, 1, 0]]
    assert packed.neg_idx[0].tolist() == [[1, 2, 3, 9, 9], [4, 5, 6, 8, 8], [0, 1, 0, 1, 1]]
    assert packed.gi[0, :3].tolist() == [1, 0, 1]
    assert packed.neg_idx[2, :, :2].tolist() == [[7, 8], [1, 0], [1, 1]]
    assert packed.pos_idx[3, :, :1].tolist() == [[5], [4], [1]] and packed.gi[3, :1].tolist() == [2]
    for t in packed:
        assert t.is_contiguous()
    # no frame with a box at all: one dummy row keeps the pointer valid, every count is zero
    packed, has_reg = FocalLoss.pack_targets([None, None], cpu)
    assert has_reg == [False, False] and packed.gts.shape == (1, 7) and packed.gt_off.tolist() == [0, 0, 0]
    assert packed.counts.tolist() == [[0, 0], [0, 0]] and packed.pos_idx.shape == (2, 3, 1)


def test_reference_without_lists_is_half_the_logit_bce():
    case = C.case1()
    case['counts'] = np.zeros_like(case['counts'])
    losses, d, (positive, ignored) = R.focal_ref(case, alpha=0.5, gamma=0.0, cls_weight=1.0, reg_weight=2.0)
    assert not positive.any() and not ignored.any()
    F, A = case['F'], case['A']
    x = torch.from_numpy(case['heads'].astype(np.float64)).reshape(F, -1, 8 * A)[:, :, :A]
    for f in range(F):
        want = 0.5 * torch.nn.functional.binary_cross_entropy_with_logits(x[f], torch.zeros_like(x[f]), reduction='sum') / 1
        assert abs(float(losses[f, 0]) - float(want)) <= 1e-12 * float(want)
        assert float(losses[f, 1]) == 0.0
    assert float(d[:, A:].abs().max()) == 0.0
    # the set semantics: an anchor listed twice as positive counts once, a positive listed in neg is not ignored
    _, _, (positive, ignored) = R.focal_ref(C.case1())
    assert positive.sum() == 3 and ignored.sum() == 7 and not (positive & ignored).any()


def test_train_like_flags():
    sys.path.insert(0, PKG)
    import train_like
    d = train_like.parse_args(['/nowhere'])
    assert d.loss == 'voxel' and d.mode == 'module'
    a = train_like.parse_args(['/nowhere', '--loss', 'focal', '--mode', 'fast', '--focal-alpha', '0.5', '--focal-gamma', '1.5',
                               '--focal-reg-weight', '1'])
    assert (a.loss, a.focal_alpha, a.focal_gamma, a.focal_reg_weight) == ('focal', 0.5, 1.5, 1.0)
    f = train_like.parse_args(['/nowhere', '--loss', 'focal', '--mode', 'fast'])
    assert (f.focal_alpha, f.focal_gamma, f.focal_reg_weight) == (0.25, 2.0, 2.0)
    for bad in (['--loss', 'focal', '--mode', 'module'], ['--loss', 'focal'], ['--loss', 'bce', '--mode', 'fast']):
        with pytest.raises(SystemExit):
            train_like.parse_args(['/nowhere'] + bad)


def test_forward_raises_and_names_the_frames_call():
    from modules.voxelnet.FocalLoss import FocalLoss
    import modules.voxelnet as vn
    crit = FocalLoss()
    assert (crit.alpha, crit.gamma, crit.cls_weight, crit.reg_weight) == (0.25, 2.0, 1.0, 2.0)
    with pytest.raises(NotImplementedError, match='heads_loss_frames'):
        crit(None, None, None, None, torch.zeros(2, 2, 2), None, torch.zeros(2, 2, 2, 7), 2)
    assert hasattr(crit, 'heads_loss_frames')
    assert not isinstance(getattr(vn, 'FocalLoss', None), type)          # the package does not re-export the class
