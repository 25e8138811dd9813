"""The kernels in front of the middle network -- mvx_index_grid, mvx_sparse_conv_output (plain, _frames, _tiles_frames, with and
without MVX_FLAG_NO_BG_FILL), the closed-form BatchNorm share, mvx_sparse_conv_gather_dz (csrc/sparseconv.hip) and
mvx_activity_dilate, mvx_tile_dilate_flags, mvx_tile_read_flags (csrc/activity.hip) -- one by one against the numpy reference
tests/sparse_ref.py, which tests/test_sparse_first_host.py holds against torch in float64.

Every kernel gets its INPUT from the reference (never from another kernel's output) and writes into a buffer pre-filled with a
recognisable pattern and followed by guard elements.  The integer kernels are compared with array_equal.  The two f32 kernels run
on DYADIC inputs (multiples of 1/4, |.| <= 2: every sum is exact in f32 and in the f64 totals, see
test_dyadic_inputs_are_exact_in_f32), so they are array_equal too; one random-input variant each uses a derived bound.

Voxel sets and geometries: tests/sparse_first_cases.py (frames stacked along depth, empty frames, voxels on both sides of every
tile edge, a 27-term site, a voxel pair that a leak between frames would meet)."""
import functools

import numpy as np
import pytest
import torch

import sparse_first_cases as K
import sparse_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24                          # unit roundoff of f32
POISON = 0x7FC0BEEF                     # a quiet NaN with a payload: what an unwritten f32 element must still hold
GUARD = 3                               # rows (sites, voxels, planes) behind every output that must stay untouched
FLAG_RELU, FLAG_NO_BG_FILL = 1, 2048
REP = 32                                # MVX_STATS_REPLICAS

FIRST = ['model', 'vec4', 'ragged4', 'onetile']            # the first-layer geometries; 'wide' serves the tile bookkeeping only
CASES = [(n, F) for n in FIRST for F in (1, 4)] + [('onetile', 16)]
TILE_CASES = CASES + [('wide', 1), ('wide', 4)]
RANDOM_CASES = [('model', 4), ('ragged4', 1), ('onetile', 16)]


def dev(a, dtype):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def poisoned(n):
    return torch.full((n,), POISON, dtype=torch.int32, device=DEV).view(torch.float32)


def bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def marked(n, dtype, value):
    return torch.full((n,), value, dtype=dtype, device=DEV)


def descriptor(name, F):
    from modules import Extension as X
    _, vox_off = K.voxels(name, F)
    return X.FramesDesc.make(vox_off, [0] * (F + 1), 1) if F > 1 else None


def desc_ref(desc):
    from modules import _hip
    return _hip._desc_ref(desc)


def grid_buffer(name, F):
    """The buffer mvx_index_grid_frames fills, built from the REFERENCE: site grid, occupancy counts, 4 + F scratch words."""
    from modules import Extension as X
    g = K.geom(name, F)
    grid, occ, _ = K.reference_grid(name, F)
    buf = dev(np.concatenate([grid.ravel(), occ.ravel(), np.zeros(4 + F, np.int32)]), torch.int32)
    assert buf.numel() * 4 == X.lib.mvx_index_grid_bytes_frames(g.din, g.H, g.W, F)
    return buf


# ---- 1. mvx_index_grid_frames ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,F', CASES)
def test_index_grid(name, F):
    from modules import _hip
    g = K.geom(name, F)
    grid, occ, _ = K.reference_grid(name, F)
    n, m = grid.size, occ.size

    def run(coords, vox_off):
        from modules import Extension as X
        desc = X.FramesDesc.make(vox_off, [0] * (F + 1), 1) if F > 1 else None
        buf, status = _hip.index_grid(dev(coords, torch.int64).reshape(-1, 4), (g.din, g.H, g.W), desc)
        torch.cuda.synchronize()
        buf = buf.cpu().numpy()
        assert buf.size == n + m + 4 + F
        return buf[:n].reshape(grid.shape), buf[n:n + m].reshape(occ.shape), int(status.item())
    coords, vox_off = K.voxels(name, F)
    got_grid, got_occ, status = run(coords, vox_off)
    assert status == 0
    assert np.array_equal(got_grid, grid), 'site grid'
    assert np.array_equal(got_occ, occ), 'coarse occupancy'
    # three voxels just outside the grid (iy = -1, ix = W, iz = D): reported and dropped before any store
    got_grid, got_occ, status = run(*K.with_out_of_range(name, F))
    assert status & 1
    assert np.array_equal(got_grid, grid) and np.array_equal(got_occ, occ)
    # no voxel at all
    got_grid, got_occ, status = run(np.zeros((0, 4), np.int64), [0] * (F + 1))
    assert status == 0 and (got_grid == -1).all() and (got_occ == 0).all()


# ---- 2. mvx_activity_dilate_frames -------------------------------------------------------------------------------------------------
def run_dilate(src, is_index, din, H, W, sd, pd, mark, F):
    """-> (mask, halo flags, tile flags) as numpy, written into marked buffers with guard elements (asserted untouched), and
    equal to what the _hip wrapper returns."""
    from modules import _hip
    from modules import Extension as X
    dout = R.out_depth(din, sd, pd)
    ty, tx = R.tiles_of(H, W)
    nm, nf = F * dout * H * W, F * dout * ty * tx
    mask = marked(nm + GUARD * W, torch.uint8, 0xAB)
    hflag, tflag = marked(nf + GUARD * tx, torch.int32, -7), marked(nf + GUARD * tx, torch.int32, -7)
    X.check(X.lib.mvx_activity_dilate_frames(X.ptr(src), int(is_index), din, dout, H, W, sd, pd, int(mark), X.ptr(mask), X.ptr(hflag),
                                             X.ptr(tflag), F, X.stream()), 'mvx_activity_dilate_frames')
    wm, wh, wt = _hip.activity_dilate(src, is_index, din, H, W, sd, pd, mark, want_tile_flags=True, F=F)
    torch.cuda.synchronize()
    assert torch.equal(wm.ravel(), mask[:nm]) and torch.equal(wh.ravel(), hflag[:nf]) and torch.equal(wt.ravel(), tflag[:nf])
    assert (mask[nm:] == 0xAB).all() and (hflag[nf:] == -7).all() and (tflag[nf:] == -7).all(), 'guard elements'
    return (mask[:nm].cpu().numpy().reshape(F * dout, H, W), hflag[:nf].cpu().numpy().reshape(F * dout, ty, tx),
            tflag[:nf].cpu().numpy().reshape(F * dout, ty, tx))


@pytest.mark.parametrize('name,F', TILE_CASES)
def test_activity_dilate(name, F):
    """Layer 1 from the index grid, layers 2 and 3 of the chain from the reference's u8 mask of the layer before, each with and
    without the border mark: mask, halo flags and tile flags."""
    g = K.geom(name, F)
    src_ref = K.reference_grid(name, F)[0] >= 0
    src_dev = grid_buffer(name, F)
    for li, (din, sd, pd, border, res) in enumerate(K.reference_chain(name, F)):
        for mark in (False, True):
            want = res if mark == border else R.dilate(src_ref, din, sd, pd, F, mark)
            got = run_dilate(src_dev, li == 0, din, g.H, g.W, sd, pd, mark, F)
            for what, a, b in zip(('mask', 'halo flags', 'tile flags'), got, want):
                assert np.array_equal(a, b), (what, li, mark)
        if li == 0:
            # the first layer from a u8 mask too (the model only dilates the index grid with this depth geometry)
            occupied = dev(src_ref, torch.uint8)
            for mark in (False, True):
                want = res if mark == border else R.dilate(src_ref, din, sd, pd, F, mark)
                got = run_dilate(occupied, False, din, g.H, g.W, sd, pd, mark, F)
                assert all(np.array_equal(a, b) for a, b in zip(got, want)), ('u8 source', mark)
        src_ref = res[0] != 0
        src_dev = dev(res[0], torch.uint8)


# ---- 3. mvx_tile_dilate_flags_frames, mvx_tile_read_flags_frames -----------------------------------------------------------------
def run_tile_flags(fn_name, n_out, tx, *args):
    from modules import Extension as X
    out = marked(n_out + GUARD * tx, torch.int32, -7)
    lead, tail = args
    X.check(getattr(X.lib, fn_name)(*lead, X.ptr(out), *tail, X.stream()), fn_name)
    torch.cuda.synchronize()
    assert (out[n_out:] == -7).all(), 'guard elements'
    return out[:n_out].cpu().numpy()


@pytest.mark.parametrize('name,F', TILE_CASES)
def test_tile_dilate_and_tile_read_flags(name, F):
    """On the flags of the three-layer chain (the first layer's geometry, then conv2 (1, 0) and conv3 (2, 1)).  'wide' is the one
    image large enough for a tile that no computed tile reads (see sparse_first_cases.GEOMS): there `read` must hold zeros."""
    from modules import _hip
    from modules import Extension as X
    g = K.geom(name, F)
    ty, tx = g.tiles
    (_, _, _, _, l1), (din2, sd2, pd2, _, l2), (din3, sd3, pd3, _, l3) = K.reference_chain(name, F)
    d4 = R.out_depth(din3, sd3, pd3)
    # the tiles layer 2's restricted backward touches: layer 1's tile flags dilated through conv2, or layer 2's own
    t1, t2 = dev(l1[2], torch.int32), dev(l2[2], torch.int32)
    for self_ref, self_dev in ((l2[2], t2), (None, None)):
        want = R.tile_dilate(l1[2], self_ref, din2, din3, sd2, pd2, F)
        got = run_tile_flags('mvx_tile_dilate_flags_frames', want.size, tx, (X.ptr(t1), X.ptr(self_dev), din2, din3, g.H, g.W, sd2, pd2), (F,))
        assert np.array_equal(got.reshape(want.shape), want), 'tile_dilate_flags'
        assert np.array_equal(_hip.tile_dilate_flags(t1, self_dev, din2, g.H, g.W, sd2, pd2, F=F).cpu().numpy().ravel(), got)
    # conv3's geometry on layer 2's flags as well (stride 2)
    want = R.tile_dilate(l2[2], l3[2], din3, d4, sd3, pd3, F)
    t3 = dev(l3[2], torch.int32)
    got = run_tile_flags('mvx_tile_dilate_flags_frames', want.size, tx, (X.ptr(t2), X.ptr(t3), din3, d4, g.H, g.W, sd3, pd3), (F,))
    assert np.array_equal(got.reshape(want.shape), want), 'tile_dilate_flags, stride 2'
    # what conv2 reads of layer 1's output and conv3 of layer 2's
    some_unread = False
    for halo, din, dout, sd, pd in ((l1[1], din2, din3, sd2, pd2), (l2[1], din3, d4, sd3, pd3)):
        want = R.tile_read(halo, din, dout, sd, pd, F)
        h = dev(halo, torch.int32)
        got = run_tile_flags('mvx_tile_read_flags_frames', want.size, tx, (X.ptr(h), din, dout, g.H, g.W, sd, pd), (F,))
        got = got.reshape(want.shape)
        assert np.array_equal(got, want), 'tile_read_flags'
        assert np.array_equal(_hip.tile_read_flags(h, din, g.H, g.W, sd, pd, F=F).cpu().numpy().reshape(want.shape), got)
        # independent of the reference: every tile with a flagged source halo makes its 3 x 3 neighbourhood readable in every
        # source plane of the output plane that reads it
        for f in range(F):
            for d in range(dout):
                srcs = [d * sd - pd + kd for kd in range(3) if 0 <= d * sd - pd + kd < din]
                for z in srcs:
                    for i, j in np.argwhere(halo[f * din + z] != 0):
                        for z2 in srcs:
                            assert (got[f * din + z2, max(i - 1, 0):i + 2, max(j - 1, 0):j + 2] != 0).all(), (f, d, z, i, j, z2)
        some_unread |= bool((got == 0).any())
    if name == 'wide':
        assert some_unread, 'a kernel that flags everything'


# ---- 4. mvx_sparse_conv_output, _frames, _tiles_frames + the closed-form BatchNorm share -------------------------------------------
@functools.lru_cache(None)
def output_reference(name, F, C, kind, relu):
    g = K.geom(name, F)
    P, bias, _ = K.values(name, F, C, kind)
    return R.sparse_output(P, K.reference_grid(name, F)[0], bias, g, relu)


def coarse_tiles(name, F):
    """[F * dout][tiles_y][tiles_x]: the output tiles whose 3 x 3 tile neighbourhood holds a voxel in a valid source plane: what
    the plain entry builds (a superset of the first layer's tile flags)."""
    g = K.geom(name, F)
    _, occ, _ = K.reference_grid(name, F)
    ty, tx = g.tiles
    on = np.zeros((F * g.dout, ty, tx), np.int32)
    for f in range(F):
        for d in range(g.dout):
            for z, _ in R.sources(d, g.din, g.sd, g.pd):
                for i, j in np.argwhere(occ[f * g.din + z] > 0):
                    on[f * g.dout + d, max(i - 1, 0):i + 2, max(j - 1, 0):j + 2] = 1
    return on


class OutputRun:
    """One `out` tensor (pre-filled with the poison pattern before every run, guard sites behind it) for every entry point."""

    def __init__(self, name, F, C, kind):
        self.name, self.F, self.C = name, F, C
        self.g = g = K.geom(name, F)
        P, bias, _ = K.values(name, F, C, kind)
        self.P, self.bias = dev(P, torch.float32), dev(bias, torch.float32)
        self.buf = grid_buffer(name, F)
        self.sites = F * g.dout * g.H * g.W
        self.out = poisoned((self.sites + GUARD * g.W) * C)
        self.tflag_ref = K.reference_chain(name, F)[0][4][2]
        self.tflag = dev(self.tflag_ref, torch.int32)

    def run(self, entry, relu, want_stats, skip_fill):
        """-> (out f32 [F * dout][H][W][C] as numpy, its bits, stats summed over the replicas [F][2][C] or None)"""
        from modules import Extension as X
        g, C, F = self.g, self.C, self.F
        self.out.view(torch.int32).fill_(POISON)
        stats = torch.full((F, REP, 2, C), 7.0, dtype=torch.float64, device=DEV) if want_stats else None      # cleared by the call
        flags = (FLAG_RELU if relu else 0) | (FLAG_NO_BG_FILL if skip_fill else 0)
        head = (X.ptr(self.P), X.ptr(self.buf), X.ptr(self.bias), X.ptr(self.out), X.ptr(stats), g.din, g.dout, g.H, g.W, C, g.sd, g.pd,
                flags)
        if entry == 'plain':
            assert F == 1
            code = X.lib.mvx_sparse_conv_output(*head, X.stream())
        elif entry == 'frames':
            code = X.lib.mvx_sparse_conv_output_frames(*head, F, X.stream())
        else:
            code = X.lib.mvx_sparse_conv_output_tiles_frames(*head, F, X.ptr(self.tflag), X.stream())
        X.check(code, entry)
        torch.cuda.synchronize()
        assert (bits(self.out[self.sites * C:]) == POISON).all(), 'guard sites'
        body = self.out[:self.sites * C].reshape(F * g.dout, g.H, g.W, C)
        return body.cpu().numpy().astype(np.float64), bits(body), None if stats is None else stats.sum(1).cpu().numpy()


def check_written(got, got_bits, ref, written, what):
    """Equal to the reference on the written sites, the poison pattern bit for bit on the others."""
    assert np.array_equal(got[written], ref[written]), what
    assert (got_bits[~written] == POISON).all(), what + ': unwritten sites'


@pytest.mark.parametrize('C', [64, 16])
@pytest.mark.parametrize('name,F', CASES)
def test_sparse_conv_output_exact(name, F, C):
    """Dyadic P and bias (both signs): `out` array_equal on every written site, unflagged tiles and guard sites still poisoned,
    the BatchNorm sums (kernel share + closed form of the ReLU(bias) sites) array_equal per frame."""
    from modules import _hip
    run = OutputRun(name, F, C, 'dyadic')
    g = run.g
    flagged = R.tile_sites(run.tflag_ref, g.H, g.W)
    coarse = R.tile_sites(coarse_tiles(name, F), g.H, g.W)
    everywhere = np.ones_like(flagged)
    assert (coarse >= flagged).all() and (name == 'onetile' or not flagged.all())
    assert name in ('onetile', 'ragged4') or not coarse.all()           # 3 x 3 tiles or fewer: every tile has an occupied neighbour
    for relu in (True, False):
        ref, ref_sums = output_reference(name, F, C, 'dyadic', relu)
        bias = K.values(name, F, C, 'dyadic')[1]
        fill = np.maximum(bias, 0.0) if relu else bias
        assert np.array_equal(ref[~flagged], np.broadcast_to(fill, ref[~flagged].shape)), 'the reference off the flagged tiles'
        results = {}
        for entry in (('plain', 'frames', 'tiles') if F == 1 else ('frames', 'tiles')):
            for want_stats in (True, False):
                for skip_fill in (False, True):
                    got, got_bits, sums = run.run(entry, relu, want_stats, skip_fill)
                    written = everywhere if not skip_fill else flagged if entry == 'tiles' else coarse
                    check_written(got, got_bits, ref, written, '%s relu=%d stats=%d skip=%d' % (entry, relu, want_stats, skip_fill))
                    if want_stats:
                        assert np.array_equal(sums, ref_sums), (entry, relu, skip_fill)
                    results[entry, skip_fill] = got_bits
        # the coarse-occupancy path and the tile-flag path: the same bits on the flagged tiles
        assert np.array_equal(results['frames', False][flagged], results['tiles', True][flagged])
        assert np.array_equal(results['frames', False], results['tiles', False])
    if F == 1:                                              # the wrappers return the same bits
        ref, ref_sums = output_reference(name, F, C, 'dyadic', True)
        out, stats = _hip.sparse_conv_output(run.P, run.buf, (g.din, g.H, g.W), run.bias, C, g.sd, g.pd)
        assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(stats.sum(0).cpu().numpy(), ref_sums[0])
    out, stats = _hip.sparse_conv_output_tiles(run.P, run.buf, (g.din, g.H, g.W), run.bias, C, g.sd, g.pd, run.tflag, F)
    ref, ref_sums = output_reference(name, F, C, 'dyadic', True)
    assert np.array_equal(out.cpu().numpy()[flagged], ref[flagged]) and np.array_equal(stats.sum(1).cpu().numpy(), ref_sums)


@pytest.mark.parametrize('C', [64, 16])
@pytest.mark.parametrize('name,F', RANDOM_CASES)
def test_sparse_conv_output_random(name, F, C):
    """Standard-normal P and bias.  Per element: the kernel adds its n <= 27 terms and the bias one by one in f32 (n roundings),
    so |out - exact| <= gamma_28 (|b| + sum |terms|) with gamma_28 = 28 u / (1 - 28 u); the bound used is 28 u (|b| + sum |terms|)
    with the magnitude sum of the reference, u = 2^-24 (gamma_28 exceeds 28 u by 28 u gamma_28 < 2e-6 of it, while the true
    worst case of the up to 28 additions is 27 roundings: 27 (1 + 2e-6) < 28).  ReLU does not increase a difference.
    BatchNorm sums: a thread adds at most 8 f32 values (rows of its tile column) and at most 8 squares in f32, the rest is f64.
    With e_i the element bound above and g = gamma_8 = 8 u / (1 - 8 u) (7 additions, and one rounding of each square):
      |sum - exact|    <= sum_i [e_i + g (|ref_i| + e_i)]                         + 2^-40 sum_i |ref_i|
      |sumsq - exact|  <= sum_i [(2 |ref_i| + e_i) e_i + g (|ref_i| + e_i)^2]     + 2^-40 sum_i ref_i^2
    over the sites of the frame; the last terms cover the f64 additions (atomics in any order, the closed form n * v, n * v * v).
    Observed on an MI355X (printed per run): element error at most 0.091 of its bound, error of the sums at most 0.038 of theirs."""
    run = OutputRun(name, F, C, 'random')
    g = run.g
    P, bias, _ = K.values(name, F, C, 'random')
    grid = K.reference_grid(name, F)[0]
    e = 28 * U * R.sparse_output_magnitude(P, grid, bias, g)
    flagged = R.tile_sites(run.tflag_ref, g.H, g.W)
    gam = 8 * U / (1 - 8 * U)
    worst_el, worst_st = 0.0, 0.0
    for relu in (True, False):
        ref, ref_sums = output_reference(name, F, C, 'random', relu)
        a = np.abs(ref)
        per = lambda x: x.reshape(F, -1, C).sum(1)
        b1 = per(e + gam * (a + e)) + 2.0 ** -40 * per(a)
        b2 = per((2 * a + e) * e + gam * (a + e) ** 2) + 2.0 ** -40 * per(a * a)
        bound_sums = np.stack([b1, b2], axis=1)
        for entry, skip_fill in (('frames', False), ('tiles', True)):
            got, got_bits, sums = run.run(entry, relu, True, skip_fill)
            written = flagged if skip_fill else np.ones_like(flagged)
            err = np.abs(got[written] - ref[written])
            frac_el = float((err / e[written]).max())
            frac_st = float((np.abs(sums - ref_sums) / bound_sums).max())
            print('sparse_conv_output %s F=%d C=%d relu=%d %s: element error / bound = %.3f, stats error / bound = %.3f'
                  % (name, F, C, relu, entry, frac_el, frac_st))
            worst_el, worst_st = max(worst_el, frac_el), max(worst_st, frac_st)
            assert (err <= e[written]).all(), (entry, relu)
            assert (got_bits[~written] == POISON).all()
            assert (np.abs(sums - ref_sums) <= bound_sums).all(), (entry, relu)
    assert worst_el > 0.0, 'random inputs round somewhere'


# ---- 5. mvx_sparse_conv_gather_dz_frames -------------------------------------------------------------------------------------------
def run_gather(name, F, C, kind):
    from modules import _hip
    from modules import Extension as X
    g = K.geom(name, F)
    coords, vox_off = K.voxels(name, F)
    V = len(coords)
    assert (V * 27 * C // 4) % 256 != 0                     # the last workgroup is partly filled
    dz = dev(K.values(name, F, C, kind)[2], torch.float32)
    cd = dev(coords, torch.int64)
    desc = descriptor(name, F)
    G = poisoned((V + GUARD) * 27 * C)
    X.check(X.lib.mvx_sparse_conv_gather_dz_frames(X.ptr(dz), X.ptr(cd), V, X.ptr(G), g.din, g.dout, g.H, g.W, C, g.sd, g.pd,
                                                   desc_ref(desc), X.stream()), 'mvx_sparse_conv_gather_dz_frames')
    W = _hip.sparse_conv_gather_dz(dz, cd, g.din, g.sd, g.pd, desc)
    torch.cuda.synchronize()
    assert (bits(G[V * 27 * C:]) == POISON).all(), 'guard rows'
    body = G[:V * 27 * C].reshape(V, 27 * C)
    assert torch.equal(body, W)
    want = R.gather_dz(K.values(name, F, C, kind)[2], coords, vox_off, g)
    assert np.array_equal(body.cpu().numpy().astype(np.float64), want)
    assert (want != 0).any() and (want.reshape(V, 27, C) == 0).all(2).any(), 'taps with and without an output site'


@pytest.mark.parametrize('C', [64, 16])
@pytest.mark.parametrize('name,F', CASES)
def test_sparse_conv_gather_dz_exact(name, F, C):
    run_gather(name, F, C, 'dyadic')


@pytest.mark.parametrize('C', [64, 16])
@pytest.mark.parametrize('name,F', RANDOM_CASES)
def test_sparse_conv_gather_dz_random(name, F, C):
    """A pure copy: array_equal on standard-normal dz as well."""
    run_gather(name, F, C, 'random')
