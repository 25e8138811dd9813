"""tests/bn_rows_cases.py without a GPU: the float64 reference over the dense expansion against torch.autograd in float64 on the
expanded tensor, for every layout kind; against tests/rows_ref.py where a layout can be written as a rows_ref.Layout; and the
case tables against the situations they name."""
import numpy as np
import pytest
import torch

import bn_rows_cases as B
import rows_ref as R


def _autograd(lay, y, g, C):
    """BatchNorm (batch statistics, biased variance, eps, no affine) behind a ReLU on the dense expansion of every frame, by
    torch in float64.  The pre-activation z is any tensor with relu(z) = y: z = y where y > 0 and -1 elsewhere.
    -> mi (F, 2, C), dz (rows, C) folded on the stored rows (NaN for a row that stands for none), dbias (C,)"""
    mi = np.full((lay.F, 2, C), np.nan)
    dz = np.full((lay.rows, C), np.nan)
    db = np.zeros((C,))
    for f in range(lay.F):
        idx, share = lay.expansion(f)
        if not len(idx):
            continue
        yd = torch.tensor(y[idx], dtype=torch.float64)
        z = torch.where(yd > 0, yd, -torch.ones_like(yd)).requires_grad_(True)
        a = torch.relu(z)
        yh = torch.nn.functional.batch_norm(a, None, None, training=True, eps=B.EPS)
        yh.backward(torch.tensor(g[idx] * share[:, None], dtype=torch.float64))
        mean = a.detach().mean(0)
        mi[f] = mean.numpy(), (1.0 / torch.sqrt(a.detach().var(0, unbiased=False) + B.EPS)).numpy()
        full = np.zeros((lay.rows, C))
        np.add.at(full, idx, z.grad.numpy())
        r = lay.frame_rows(f)
        r = r[lay.weight[r] > 0]
        dz[r] = full[r]
        db += z.grad.numpy().sum(0)
    return mi, dz, db


@pytest.mark.parametrize('kind', B.KINDS)
def test_reference_matches_autograd(kind):
    lay = B.layout(kind)
    C = 8
    y, g, mi32 = B.operands(lay, C, seed=1)
    y, g = y.astype(np.float64), g.astype(np.float64)
    mi = B.bn_forward(lay, y)
    ref_mi, ref_dz, ref_db = _autograd(lay, y, g, C)
    live = lay.pop > 0
    assert live.sum() >= min(2, lay.F) and (kind.endswith('_empty') or kind == 'vfe') == (not live.all())
    assert np.isnan(mi[~live]).all() and B.rel(mi[live], ref_mi[live]) < 1e-12
    # what the operands hand to the kernel is this, rounded to f32 (frames without population: finite stand-ins)
    assert np.isfinite(mi32).all() and B.rel(mi32[live], mi[live]) < 1e-7
    dz, db = B.bn_relu_backward(lay, g, y, np.where(np.isnan(mi), 0.0, mi))
    assert np.array_equal(np.isnan(dz[:, 0]), lay.weight == 0)
    assert B.rel(dz, ref_dz) < 1e-11 and B.rel(db, ref_db) < 1e-11


def test_fusion_reference_matches_rows_ref():
    """A fusion set whose frames share one population is a rows_ref.Layout of one 'voxel' of T = population rows per frame: its
    real rows, then its padded row."""
    lay = B.fusion([300, 120, 77], [10, 10, 10], 35)
    L = R.Layout(350, 3, [300, 120, 77], [0, 1, 2, 3])
    assert L.rows == lay.rows and list(L.real_off) == lay.real_off
    y, g, _ = B.operands(lay, 8, seed=2)
    mi = B.bn_forward(lay, y)
    assert B.rel(mi, R.bn_forward(y, L, B.EPS)) < 1e-12
    dz, db = B.bn_relu_backward(lay, g, y, mi)
    rdz, rdb = R.bn_relu_backward(g, y, mi, L)
    assert B.rel(dz, rdz) < 1e-11 and B.rel(db, rdb) < 1e-11


def test_vfe_layout_is_the_rows_ref_layout():
    lay = B.layout('vfe')
    L = lay.vfe
    for f in range(L.F):
        pairs = R.dense_expansion(L, f)
        idx, _ = lay.expansion(f)
        assert sorted(r for r, w in pairs for _ in range(w)) == sorted(idx.tolist())
    assert (lay.weight == 0).sum() >= 5 and lay.pop[1] == 0


@pytest.mark.parametrize('s', B.C_TABLE, ids=B.shape_id)
def test_c_table_reaches_what_it_names(s):
    B.check_shape(s)
    lay = B.table_layout(s)
    assert lay.rows == s.per * s.F
    if s.F > 1:
        assert B.spanning_blocks(lay, s.C) >= 1
    if s.C == 16:
        assert B.spanning_blocks(lay, s.C) == 2


@pytest.mark.parametrize('C', B.KIND_C)
@pytest.mark.parametrize('kind', [k for k in B.KINDS if k != 'single'])
def test_every_kind_has_a_block_that_spans_two_segments(kind, C):
    lay = B.layout(kind)
    assert lay.F == 3 and B.spanning_blocks(lay, C) >= 1


def test_geometry_examples():
    """Worked by hand from bn_relu_backward_impl."""
    assert B.geometry(3711, 16) == B.Geometry(4, 64, 8, 512, 8, 'shuffle')
    assert B.geometry(8193, 768) == B.Geometry(192, 1, 1024, 12, 683, 'serial')
    assert B.geometry(41, 1028) == B.Geometry(257, 1, 6, 8, 6, 'columns')
    assert B.geometry(0, 16).blocks == 0
    assert B.last_trip_is_partial(3711, 16) and not B.last_trip_is_partial(512, 16)


def test_operands_put_the_largest_dz_in_the_last_row():
    lay = B.layout('grid')
    y, g, mi = B.operands(lay, 16, seed=3, peak_last=True)
    dz, _ = B.bn_relu_backward(lay, g, y, mi)
    assert int(np.abs(dz).max(1).argmax()) == lay.rows - 1
