"""Case table, operands and float64 reference of the exact-f32 row GEMM tests (tests/test_rowgemm_f32_gpu.py; the table itself is
checked without a GPU by tests/test_rowgemm_cases_host.py).  torch only; every function works on any device.

Operands live inside larger buffers whose unused part is NaN (``slab``): the columns beside the used ones, and a few rows behind
the last one.  The kernels clamp an out-of-range load to the operand's first element and zero the K tail when it is staged
(csrc/linear.hip), so a correct kernel lets no slack value reach an output."""
import collections

import torch

NAN = float('nan')
BK = 32                                # K chunk of linear_fwd (csrc/linear.hip): split-K needs k >= 8 chunks
TAIL_ROWS = 3                          # poisoned rows behind every operand and result

# ---- bounds (max error over max |reference|, against float64) -------------------------------------------------------------
BOUND = 2e-6                           # the project's bound for this kernel (tests/test_voxelnet_gpu.py, test_rowgemm_k128_gpu.py)
F32_MEASURED = 2.2124e-07              # tests/test_linear_epilogue_gpu.py: K = 23 / 24, measured before the epilogue was shared
SMALL_K, SMALL_K_BOUND = 40, 4 * F32_MEASURED


def bound_for(k):
    """The bound of a case whose K is ``k``: 2e-6, and for K <= 40 the measured small-K value times four."""
    return min(BOUND, SMALL_K_BOUND) if k <= SMALL_K else BOUND


# ---- forward cases ------------------------------------------------------------------------------------------------------
# K, N; wt: the weight is stored (K, N) and read transposed; x0 / ldx: first column and width of the buffer that x is a column
# slice of (ldx None: k + 4); w0 / ldw the same for the weight; inst: the linear_fwd<WT, NT, VEC> that the dispatch must choose.
Fwd = collections.namedtuple('Fwd', 'name K N wt x0 ldx w0 ldw inst')


def _f(name, K, N, wt, inst, x0=0, ldx=None, w0=0, ldw=None):
    return Fwd(name, K, N, wt, x0, ldx, w0, ldw, inst)


FWD_CASES = [
    # WT = 0, NT = 2, 16-byte: the heads (the second 32-column tile entirely off), and x an aligned slice with ldx > k
    _f('head24', 24, 16, 0, (0, 2, 1)),
    _f('head768', 768, 16, 0, (0, 2, 1)),
    _f('xslice8', 24, 32, 0, (0, 2, 1), x0=8, ldx=40),
    # WT = 0, NT = 4, 16-byte: a K tail of 4 in the second chunk + a half-empty last column block; just wide (60 of 128 off)
    _f('tail36x192', 36, 192, 0, (0, 4, 1)),
    _f('wide68', 64, 68, 0, (0, 4, 1)),
    # WT = 0, scalar loads: K = 23 narrow and wide; K % 4 == 0 from an unaligned base
    _f('k23n32', 23, 32, 0, (0, 2, 0)),
    _f('k23n128', 23, 128, 0, (0, 4, 0)),
    _f('xslice1', 24, 32, 0, (0, 2, 0), x0=1, ldx=28),
    # WT = 1, NT = 2, 16-byte
    _f('t40x64', 40, 64, 1, (1, 2, 1)),
    _f('t128x32', 128, 32, 1, (1, 2, 1)),
    # WT = 1, NT = 4, 16-byte: the heads' input gradient; the weight a column slice (ldw > n)
    _f('thead', 16, 768, 1, (1, 4, 1)),
    _f('twslice', 72, 192, 1, (1, 4, 1), w0=8, ldw=208),
    # WT = 1, scalar loads: n % 4 != 0 (NT = 2), k % 4 != 0 (NT = 4)
    _f('t24x30', 24, 30, 1, (1, 2, 0)),
    _f('t23x70', 23, 70, 1, (1, 4, 0)),
]
FWD_ROWS = (1, 129, 300)               # a single row; a full block + a block of one row; a ragged last block
FWD_BY_NAME = {c.name: c for c in FWD_CASES}

# (R, K, N, wt) of the split-K cases: eligible by the header's contract (no bias / ReLU / stats, ldy == n, skinny, long k)
SplitK = collections.namedtuple('SplitK', 'name R K N wt inst reduce')
SPLITK_CASES = [
    SplitK('r100k256', 100, 256, 16, 0, (0, 2, 1), 'slab_reduce'),
    SplitK('tailslab', 300, 300, 192, 1, (1, 4, 1), 'slab_reduce'),                # K = 9 chunks + 12: the last slab ends in a tail
    SplitK('scalar', 130, 301, 64, 0, (0, 2, 0), 'slab_reduce'),
    SplitK('wide', 2100, 256, 128, 0, (0, 4, 1), 'slab_reduce_wide'),              # rows * n > 2^18
]
SPLITK_OFF = ('bias', 'relu', 'stats', 'ldy')          # forms of r100k256 in which the contract keeps split-K off

# ---- weight-gradient cases ----------------------------------------------------------------------------------------------
# R, K, N; x0 / ldx, z0 / lddz as above; vec: linear_wgrad<true> (16-byte loads) or linear_wgrad<false>
Wgrad = collections.namedtuple('Wgrad', 'name R K N x0 ldx z0 lddz vec')


def _g(name, R, K, N, vec, x0=0, ldx=None, z0=0, lddz=None):
    return Wgrad(name, R, K, N, x0, ldx, z0, lddz, vec)


WGRAD_CASES = [
    _g('row1', 1, 24, 16, 1),
    _g('rows31', 31, 24, 16, 1),                       # around the 32-row LDS step
    _g('rows33', 33, 24, 16, 1),
    _g('strip1', 129, 128, 64, 1),                     # strips of 128 rows: the second holds one row; waves wn = 1 off (N = 64)
    # 2 x 2 output blocks with ragged edges, waves wk = 1 of the last K block off: K = 130 is no multiple of 4 and takes the
    # scalar loads, K = 132 is its 16-byte sibling
    _g('blocks2x2', 300, 130, 200, 0),
    _g('blocks2x2v', 300, 132, 200, 1),
    _g('slices', 517, 40, 768, 1, x0=8, ldx=56, z0=16, lddz=800),
    _g('vfe23', 300, 23, 32, 0),                       # the VFE first layer
    _g('n30', 300, 24, 30, 0),
    _g('xslice1', 129, 24, 32, 0, x0=1, ldx=28),
]
WGRAD_BY_NAME = {c.name: c for c in WGRAD_CASES}
WGRAD_ACCUMULATE = ('rows33', 'blocks2x2', 'vfe23')


# ---- routing, restated from linear_forward_impl / mvx_linear_wgrad ----------------------------------------------------------
def aligned16(addr):
    return addr % 16 == 0


def fwd_inst(x_addr, ldx, w_addr, ldw, wt, k, n):
    """(WT, NT, VEC) of the linear_fwd instantiation that linear_forward_impl launches."""
    vec = aligned16(x_addr) and aligned16(w_addr) and ldx % 4 == 0 and ldw % 4 == 0 and k % 4 == 0 and (not wt or n % 4 == 0)
    wide = n > 64
    return (int(bool(wt)), 4 if wide else 2, int(vec))


def wgrad_vec(x_addr, ldx, z_addr, lddz, k, n):
    return int(aligned16(x_addr) and aligned16(z_addr) and ldx % 4 == 0 and lddz % 4 == 0 and k % 4 == 0 and n % 4 == 0)


# ---- operands -----------------------------------------------------------------------------------------------------------
def slab(rows, cols, col0, ld, gen, device, scale=1.0, fill=None):
    """A (rows, cols) view at column ``col0`` of a NaN buffer (rows + TAIL_ROWS, ld); the view holds ``scale`` * randn (drawn
    on the CPU from ``gen``) or, with ``fill``, that constant.  Returns (buffer, view)."""
    assert col0 + cols <= ld
    buf = torch.full((rows + TAIL_ROWS, ld), NAN, dtype=torch.float32, device=device)
    view = buf[:rows, col0:col0 + cols]
    if fill is not None:
        view.fill_(fill)
    elif rows:
        view.copy_((torch.randn((rows, cols), generator=gen) * scale).to(device))
    return buf, view


def only_view_finite(buf, view_rows, col0, cols):
    """True when exactly the (view_rows, cols) block at column col0 of ``buf`` is finite and everything else is NaN."""
    want = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    want[:view_rows, col0:col0 + cols] = True
    return bool((torch.isfinite(buf) == want).all()) and bool(torch.isnan(buf[~want]).all())


def fwd_operands(c, rows, device, seed=0):
    """x (rows, K) and the weight -- (N, K), or (K, N) for c.wt -- as views of poisoned buffers, and a bias (N,)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * c.K + c.N + rows)
    ldx = c.ldx if c.ldx is not None else c.K + 4
    _, x = slab(rows, c.K, c.x0, ldx, g, device)
    wr, wc = (c.K, c.N) if c.wt else (c.N, c.K)
    ldw = c.ldw if c.ldw is not None else wc + 4
    _, w = slab(wr, wc, c.w0, ldw, g, device, scale=0.2)
    b = (torch.randn((c.N,), generator=g) * 0.1).to(device)
    return x, w, b


def fwd_reference(x, w, wt, bias=None, relu=False):
    """float64: [ReLU](x w^T + b), w stored (N, K) -- or (K, N) with ``wt``."""
    w64 = w.double() if wt else w.double().t()
    y = x.double() @ w64
    if bias is not None:
        y = y + bias.double()
    return torch.relu(y) if relu else y


def wgrad_operands(c, device, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * c.K + c.N + c.R)
    _, x = slab(c.R, c.K, c.x0, c.ldx if c.ldx is not None else c.K + 4, g, device)
    _, dz = slab(c.R, c.N, c.z0, c.lddz if c.lddz is not None else c.N + 4, g, device)
    return x, dz


def wgrad_reference(x, dz):
    """float64: dW (N, K) = dz^T x."""
    return dz.double().t() @ x.double()


def rel(a, b):
    """max |a - b| over max |b|, in float64."""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))
