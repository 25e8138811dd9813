"""The case table of the exact-f32 row GEMM tests (tests/rowgemm_cases.py) without a GPU: every instantiation has a case, every
case's layout meets the routing condition of the instantiation it names, and the operand and reference helpers do what the GPU
test relies on."""
import numpy as np
import torch

import rowgemm_cases as C

BASE = 1 << 12                        # an allocation's address: 16-byte aligned, as torch's device allocations are


def _fwd_layout(c):
    ldx = c.ldx if c.ldx is not None else c.K + 4
    ldw = c.ldw if c.ldw is not None else (c.N if c.wt else c.K) + 4
    return BASE + 4 * c.x0, ldx, BASE + 4 * c.w0, ldw


def test_every_instantiation_has_a_case():
    insts = {c.inst for c in C.FWD_CASES}
    assert insts == {(wt, nt, vec) for wt in (0, 1) for nt in (2, 4) for vec in (0, 1)}
    assert {c.vec for c in C.WGRAD_CASES} == {0, 1}
    assert {c.reduce for c in C.SPLITK_CASES} == {'slab_reduce', 'slab_reduce_wide'}
    assert {C.WGRAD_BY_NAME[n].vec for n in C.WGRAD_ACCUMULATE} == {0, 1}


def test_layouts_meet_their_routing_condition():
    for c in C.FWD_CASES:
        xa, ldx, wa, ldw = _fwd_layout(c)
        assert ldx >= c.x0 + c.K and ldw >= c.w0 + (c.N if c.wt else c.K), c.name
        assert C.fwd_inst(xa, ldx, wa, ldw, c.wt, c.K, c.N) == c.inst, c.name
    for c in C.SPLITK_CASES:
        assert C.fwd_inst(BASE, c.K + 4, BASE, (c.N if c.wt else c.K) + 4, c.wt, c.K, c.N) == c.inst, c.name
        assert c.K >= 8 * C.BK and (c.R * c.N > 1 << 18) == (c.reduce == 'slab_reduce_wide'), c.name
    for c in C.WGRAD_CASES:
        ldx = c.ldx if c.ldx is not None else c.K + 4
        lddz = c.lddz if c.lddz is not None else c.N + 4
        assert C.wgrad_vec(BASE + 4 * c.x0, ldx, BASE + 4 * c.z0, lddz, c.K, c.N) == c.vec, c.name
        # a kernel that mixed the two leading dimensions up would read other elements
        assert ldx != lddz, c.name


def test_bounds():
    assert C.bound_for(24) == 4 * 2.2124e-07 and C.bound_for(40) == C.bound_for(24) and C.bound_for(41) == 2e-6


def test_operands_and_reference():
    c = C.FWD_BY_NAME['twslice']
    x, w, b = C.fwd_operands(c, 5, 'cpu')
    assert x.shape == (5, c.K) and w.shape == (c.K, c.N) and w.stride(0) == c.ldw and not w.is_contiguous()
    assert torch.isfinite(x).all() and torch.isfinite(w).all()
    buf, v = C.slab(3, 4, 2, 8, torch.Generator().manual_seed(0), 'cpu')
    assert buf.shape == (3 + C.TAIL_ROWS, 8) and C.only_view_finite(buf, 3, 2, 4)
    buf[4, 0] = 1.0
    assert not C.only_view_finite(buf, 3, 2, 4)
    ref = C.fwd_reference(x, w, 1, b, relu=True).numpy()
    want = np.maximum(np.einsum('rk,kn->rn', x.double().numpy(), w.double().numpy()) + b.double().numpy(), 0.0)
    assert np.allclose(ref, want, rtol=1e-14, atol=1e-14)
    g = C.WGRAD_BY_NAME['slices']
    xs, dz = C.wgrad_operands(g, 'cpu')
    assert xs.stride(0) == g.ldx and dz.stride(0) == g.lddz
    assert np.allclose(C.wgrad_reference(xs, dz).numpy(), np.einsum('rn,rk->nk', dz.double().numpy(), xs.double().numpy()),
                       rtol=1e-13, atol=1e-13)
