"""CPU side of tests/test_background_gpu.py.

1. The float64 reference (tests/background_ref.py, tests/background_cases.py) has the properties the GPU test relies on, on exactly
   the arrays that test uploads: off the site masks every layer output is one value per (frame, plane, channel); off the tiles
   of conv2's restricted backward its dense gradient is an affine function of the incoming one; the cases have the unflagged tiles, the partial
   tiles, the empty frame and the straddling tile runs they are there for.
2. Sensitivity.  This file restates the CLOSED FORMS of the library (csrc/activity.hip, csrc/conv3d.hip) in numpy float64, holds
   them against the dense reference, and then breaks them one structural mistake at a time.  Every mistake must move a quantity
   the GPU test checks by more than 10 x the tolerance the GPU test uses for it: a kernel with that mistake cannot pass.  The
   ratios are printed (pytest -s); their minima are in DESIGN.md section 4.
3. Argument checks of the entry points that return before any launch."""
import ctypes
import functools

import numpy as np
import pytest

import background_cases as BC
import background_ref as B
import sparse_ref as R

C = BC.C
NAMES = sorted(BC.CASES)
MUTATIONS = ('drop_tile', 'neighbour_plane_c', 'frame0_mean_inv', 'partial_tile_128', 'drop_border_correction', 'interior_for_class',
             'skipped_tap_left_out', 'src_plane_shift')
FACTOR = 10.0


# ---- 1. properties of the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_background_is_one_value_per_plane_and_channel(name):
    wi, t = BC.wiring(name), BC.dense(name)
    scale = max(float(np.abs(t[k]).max()) for k in ('x1', 'x2', 'x3'))
    print('%s: largest deviation of a background site from its plane value %.3g (scale %.3g)' % (name, t['bg_dev'], scale))
    assert t['bg_dev'] <= 1e-12 * scale
    for k in ('c1', 'ybg1', 'c2', 'ybg2', 'c3', 'ybg3'):
        assert np.isfinite(t[k]).all(), k                       # every plane has a background site
    for k in ('ybg1', 'ybg2'):                                  # both branches of [y_bg > 0] in the bias gradient
        zero = float((t[k] == 0).mean())
        assert 0.3 < zero < 0.7, (k, zero)
    # off the tiles of conv2's restricted backward its output is the background, so the dense gradient of its pre-activation
    # is an affine function of the incoming one with per-plane coefficients: dz2 - [y_bg > 0] inv g2 is ONE value per
    # (plane, channel) there (dz2 itself is not: the upstream gradient is arbitrary), and the sum over those tiles follows from
    # the sum of g2 and the number of sites -- what lets the kernels work from plane sums alone
    off = ~B.tile_sites(wi.conv2.bflag_out, wi.H, wi.W)
    inv = np.repeat(t['mi2'][:, 1], wi.conv2.dout, axis=0)
    slope = (t['ybg2'] > 0) * inv
    val, dev = B.background_value(t['dz2'] - slope[:, None, None] * t['g2'], ~off)
    assert dev <= 1e-11 * float(np.abs(t['dz2']).max())
    n_off = off.sum((1, 2))
    closed = slope * B.region_sums(t['g2'], off) + np.nan_to_num(val) * n_off[:, None]
    assert np.allclose(t['inact2'], closed, rtol=1e-9, atol=1e-9 * float(np.abs(t['inact2']).max()))
    on = B.region_sums(t['dz2'], ~off)
    assert np.allclose(on + t['inact2'], B.plane_sums(t['dz2']), rtol=0, atol=1e-10 * float(np.abs(t['dz2']).max()) * wi.H * wi.W)


def test_cases_hold_what_they_are_there_for():
    counts = {}
    for name in NAMES:
        wi = BC.wiring(name)
        counts[name] = tuple((int((L.tflag_out == 0).sum()), L.tflag_out.size) for L in wi.layers)
    assert counts == {'wide': ((81, 189), (54, 126)), 'model': ((36, 240), (24, 160))}
    wide, model = BC.wiring('wide'), BC.wiring('model')
    assert (wide.F, wide.H, wide.W, wide.D1, wide.conv2.dout, wide.conv3.dout) == (1, 72, 112, 5, 3, 2)
    assert (model.F, model.H % R.TH, model.W % R.TW) == (4, 5, 5)                    # partial last tile row and column
    # only 'wide' has tiles nobody reads, and unflagged tiles off bflag2 with both tiles of a vertical pair unflagged
    assert all((L.read_in == 0).any() for L in wide.layers) and not any((L.read_in == 0).any() for L in model.layers)
    # the empty frame: no flagged tile in layer 1, so the whole plane is "inactive" there; the other frames have some
    t1 = model.conv2.tflag_in.reshape(model.F, -1)
    assert not t1[1].any() and all(t1[f].any() for f in (0, 2, 3))
    for wi in (wide, model):
        for L in wi.layers:
            # what the kernels assume of their flags: border tiles carry gradient / are computed; gradients live where they are read
            border = np.zeros(L.tflag_out.shape[1:], bool)
            border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
            assert (L.tflag_out[:, border] != 0).all()
            assert ((L.bflag_in != 0) | (L.tflag_in == 0)).all()
    # the shares of the depth taps are never zero where a source plane exists
    for name in NAMES:
        for li in (0, 1):
            L, F = BC.wiring(name).layers[li], BC.wiring(name).F
            ref, _ = BC.table(name, li)
            P = F * L.dout
            taps = ref[P:4 * P].reshape(P, 3, C)
            for p in range(P):
                for kd in range(3):
                    has = 0 <= (p % L.dout) * L.sd - L.pd + kd < L.din
                    assert (taps[p, kd] != 0).all() if has else (taps[p, kd] == 0).all(), (name, li, p, kd)


def test_the_batchnorm_case_straddles_planes_and_frames():
    bc = BC.bn_case()
    F, D, H, W, Cn = BC.BN_SHAPE
    ty, tx = R.tiles_of(H, W)
    flags = bc.flags.reshape(F * D, -1)
    assert (ty * tx) % 2 == 1 and flags.size == 2166 and int((flags != 0).sum()) >= 2049
    border = np.ones((ty, tx), bool)
    border[1:-1, 1:-1] = False
    assert (bc.flags[:, border] != 0).all()
    # bnb_tiles: min(2048, tiles) workgroups take contiguous runs of ceil(n_act / 2048) listed tiles
    n_act = int((flags != 0).sum())
    per = -(-n_act // 2048)
    assert per == 2
    plane_of = np.repeat(np.arange(F * D), ty * tx)[flags.ravel() != 0]
    runs = [plane_of[j:j + per] for j in range(0, n_act, per)]
    assert any(r[0] != r[-1] for r in runs), 'a run in two planes (flush inside a run)'
    assert any(r[0] // D != r[-1] // D for r in runs), 'a run in two frames'
    assert -(-flags.size // 1024) > 1                           # bnb_tile_list: more than one flag per thread
    assert 256 // (Cn // 4) != R.TW and 256 // (C // 4) == R.TW   # the generic site loop here, the eight-row path at C = 64
    assert 0.3 < float((bc.ybg == 0).mean()) < 0.7


# ---- 2. the closed forms, restated, and their mutants ---------------------------------------------------------------------------------
def src_plane(d, L, kd, shift=0):
    z = d * L.sd - L.pd + kd + shift
    return z if 0 <= z < L.din else -1


def first_tile(flags, pick):
    """(plane, ty, tx) of a flagged tile: the pick-th from the END (the last frame, away from the full voxel block)."""
    idx = np.argwhere(np.asarray(flags) != 0)
    return tuple(int(v) for v in idx[-1 - pick])


def without_tile(flags, tile):
    out = np.array(flags)
    out[tile] = 0
    return out


def closed_table(w, c_in, L, F, mut=None):
    """mvx_conv3d_background_taps_frames: totals | depth taps | border classes."""
    P = F * L.dout
    tot, tap, cls = np.zeros((P, C)), np.zeros((P, 3, C)), np.zeros((P, 9, C))
    shift = 1 if mut == 'src_plane_shift' and L.sd == 2 else 0
    for p in range(P):
        f, d = divmod(p, L.dout)
        for kd in range(3):
            z = src_plane(d, L, kd, shift)
            if z < 0:
                continue
            part = np.einsum('ncab,c->abn', w[:, :, kd], c_in[f * L.din + z])
            tap[p, kd] = part.sum((0, 1))
            for q in range(9):
                ry, rx = divmod(q, 3)
                for a in range(3):
                    for b in range(3):
                        if not ((ry == 0 and a == 0) or (ry == 2 and a == 2) or (rx == 0 and b == 0) or (rx == 2 and b == 2)):
                            cls[p, q] += part[a, b]
        tot[p] = tap[p].sum(0)
        if mut == 'interior_for_class':
            cls[p, :] = tot[p]
    return np.concatenate([tot, tap.reshape(P * 3, C), cls.reshape(P * 9, C)])


def frame_rows(mi, planes, mut=None):
    """(mean, inv) per global plane; the mutant gives frame 1 the statistics of frame 0."""
    mi = np.array(mi)
    if mut == 'frame0_mean_inv' and mi.shape[0] > 1:
        mi[1] = mi[0]
    return np.repeat(mi[:, 0], planes, axis=0), np.repeat(mi[:, 1], planes, axis=0)


def neighbour(c, planes, mut=None):
    """c per global plane; the mutant reads the next plane of the frame (the previous one in the last)."""
    if mut != 'neighbour_plane_c':
        return c
    idx = np.arange(c.shape[0])
    nb = np.where(idx % planes == planes - 1, idx - 1, idx + 1)
    return c[nb]


def closed_bn_apply_tiles(y, mi, c_bg, tflag, F, mut=None, tile=None):
    P, H, W, _ = y.shape
    m, inv = frame_rows(mi, P // F, mut)
    flags = without_tile(tflag, tile) if mut == 'drop_tile' else tflag
    on = B.tile_sites(flags, H, W)
    return np.where(on[..., None], (y - m[:, None, None]) * inv[:, None, None], neighbour(c_bg, P // F, mut)[:, None, None])


def closed_tap_sums(dz, flags, inactive, mut=None, tile=None):
    """mvx_plane_tap_sums, tile form: the nine region sums over the flagged tiles, the closed-form share of the rest, and the
    inclusion-exclusion of region_tap_sums."""
    P, H, W, _ = dz.shape
    use = without_tile(flags, tile) if mut == 'drop_tile' else flags
    v = np.where(B.tile_sites(use, H, W)[..., None], np.nan_to_num(dz), 0.0)
    k = [v.sum((1, 2)) + inactive, v[:, 0].sum(1), v[:, H - 1].sum(1), v[:, :, 0].sum(1), v[:, :, W - 1].sum(1),
         v[:, 0, 0], v[:, 0, W - 1], v[:, H - 1, 0], v[:, H - 1, W - 1]]
    T = np.empty((P, 9, dz.shape[3]))
    for a in range(3):
        for b in range(3):
            t = k[0].copy()
            if a == 0 and not (mut == 'drop_border_correction' and b == 1):
                t -= k[1]
            if a == 2:
                t -= k[2]
            if b == 0:
                t -= k[3]
            if b == 2:
                t -= k[4]
            if a == 0 and b == 0:
                t += k[5]
            if a == 0 and b == 2:
                t += k[6]
            if a == 2 and b == 0:
                t += k[7]
            if a == 2 and b == 2:
                t += k[8]
            T[:, a * 3 + b] = t
    return T


def closed_input_grad_sums(w, T, L, F, mut=None):
    """A[z][c] = sum over the (output plane d, kd) that read input plane z, taps and output channels of W T[d]."""
    A = np.zeros((F * L.din, w.shape[1]))
    shift = 1 if mut == 'src_plane_shift' and L.sd == 2 else 0
    for f in range(F):
        for d in range(L.dout):
            for kd in range(3):
                z = src_plane(d, L, kd, shift)
                if z >= 0:
                    A[f * L.din + z] += np.einsum('nck,kn->c', w[:, :, kd].reshape(w.shape[0], w.shape[1], 9), T[f * L.dout + d])
    return A


def closed_wgrad(x, c_in, dz, T, L, F, mut=None, tile=None, hflag=None):
    """mvx_conv3d_wgrad_bg: (x - c_in) (x) dz over the (output tile, depth tap) pairs whose source tile has its halo flag set --
    the difference vanishes in the halo of every other tile -- plus the rank-one term c_in (x) tap sums.  A wrong constant c'
    leaves (c_in - c') (x) dz behind on the pairs that are NOT visited."""
    dzv = np.nan_to_num(dz)
    if mut == 'drop_tile':
        p, i, j = tile
        dzv = dzv.copy()
        dzv[p, i * R.TH:(i + 1) * R.TH, j * R.TW:(j + 1) * R.TW] = 0.0
    dw = B.wgrad(np.nan_to_num(x) - c_in[:, None, None, :], dzv, L.sd, L.pd, F)
    shift = 1 if mut == 'src_plane_shift' and L.sd == 2 else 0
    wrong = neighbour(c_in, L.din, mut) - c_in
    for f in range(F):
        for d in range(L.dout):
            p = f * L.dout + d
            for kd in range(3):
                z = src_plane(d, L, kd, shift)
                if z >= 0:
                    dw[:, :, kd] += np.einsum('c,kn->nck', c_in[f * L.din + z], T[p]).reshape(C, C, 3, 3)
                if mut == 'neighbour_plane_c' and z >= 0:
                    unvisited = B.tile_sites(hflag[f * L.din + z][None] == 0, dz.shape[1], dz.shape[2])
                    left = B.tap_sums(np.nan_to_num(dz[p:p + 1]) * unvisited[..., None])[0]
                    dw[:, :, kd] -= np.einsum('c,kn->nck', wrong[f * L.din + z], left).reshape(C, C, 3, 3)
    return dw


def wgrad_tile(L):
    """An output tile (plane, ty, tx) whose middle depth tap reads a tile that holds non-background sites."""
    for p, i, j in np.argwhere(L.tflag_out != 0)[::-1]:
        f, d = divmod(int(p), L.dout)
        z = src_plane(d, L, 1)
        if z >= 0 and L.tflag_in[f * L.din + z, i, j]:
            return int(p), int(i), int(j)
    raise AssertionError('no such tile')


def closed_bn_backward(dyhat, y, mi, c_bg, ybg, A, flags, F, mut=None, tile=None):
    """mvx_bn_relu_backward_tiles_frames -> (dz on the flagged tiles (0 elsewhere), dbias, dz_inactive_sums), from the header of
    bnb_tiles / bnb_finalize_ab / bnb_dbias in csrc/activity.hip."""
    P, H, W, Cn = y.shape
    D = P // F
    m, inv = frame_rows(mi, D, mut)
    cb = neighbour(c_bg, D, mut)
    listed = without_tile(flags, tile) if mut == 'drop_tile' else flags
    on = B.tile_sites(listed, H, W)[..., None]
    g = np.where(on, np.nan_to_num(dyhat), 0.0)
    yh = (y - m[:, None, None]) * inv[:, None, None]
    P1 = g.sum((1, 2))
    Q1 = (g * (yh - cb[:, None, None])).sum((1, 2)).reshape(F, D, Cn).sum(1)
    N = D * H * W
    a = A.reshape(F, D, Cn).sum(1) / N
    b = (Q1 + (cb * A).reshape(F, D, Cn).sum(1)) / N
    ap, bp = np.repeat(a, D, axis=0), np.repeat(b, D, axis=0)
    dz = np.where(on & (y > 0), inv[:, None, None] * (g - (ap[:, None, None] + yh * bp[:, None, None])), 0.0)
    ty, tx = R.tiles_of(H, W)
    rows = np.minimum(R.TH, H - np.arange(ty) * R.TH)[:, None]
    cols = np.minimum(R.TW, W - np.arange(tx) * R.TW)[None, :]
    sites = np.full((ty, tx), R.TH * R.TW) if mut == 'partial_tile_128' else rows * cols
    n_inact = ((np.asarray(flags) == 0) * sites).sum((1, 2))
    inact = np.where(ybg > 0, inv * ((A - P1) - n_inact[:, None] * (ap + cb * bp)), 0.0)
    return dz, dz.sum((0, 1, 2)) + inact.sum(0), inact


RATIOS = {}


def note(mut, quantity, case, mutated, ref, tol):
    """The mutant must leave the tolerance by FACTOR somewhere."""
    diff, tol = np.abs(np.asarray(mutated) - ref), np.broadcast_to(tol, np.shape(ref))
    exact = tol == 0                                            # elements that must be matched exactly: any change there counts as infinite
    ratio = np.inf if (diff[exact] > 0).any() else float((diff[~exact] / tol[~exact]).max())
    RATIOS.setdefault(mut, []).append((ratio, quantity, case))
    print('  %-24s %-34s %-8s moves the reference by %10.3g x the tolerance' % (mut, quantity, case, ratio))
    assert ratio > FACTOR, (mut, quantity, case, ratio)


def agree(closed, ref, what, rtol=1e-9):
    err = float(np.abs(closed - ref).max())
    assert err <= rtol * float(np.abs(ref).max()), (what, err)


@functools.lru_cache(None)
def table_and_constants(name):
    wi = BC.wiring(name)
    for li in (0, 1):
        L, _, c_in, w, b, y, mi, x_out, c_out, ybg_out, _, _ = BC.layer_tensors(name, li)
        ref, tol = BC.table(name, li)
        agree(closed_table(w, c_in, L, wi.F), ref, 'table')
        case = '%s/conv%d' % (name, li + 2)
        note('interior_for_class', 'background_taps (classes)', case, closed_table(w, c_in, L, wi.F, 'interior_for_class'), ref, tol)
        if L.sd == 2:
            note('src_plane_shift', 'background_taps', case, closed_table(w, c_in, L, wi.F, 'src_plane_shift'), ref, tol)
        # bn_background and bn_apply_tiles of this layer's output
        P = wi.F * L.dout
        bg_pre = B.f32(ref[:P])
        mi32 = B.f32(mi)
        _, c_ref, c_tol = BC.bn_background(bg_pre, b, mi32, L.dout, True)
        out_ref, out_tol = BC.bn_apply(y, mi32)
        c32 = B.f32(c_ref)
        tile = first_tile(L.tflag_out, 0)
        agree(closed_bn_apply_tiles(y, mi32, c32, L.tflag_out, wi.F), out_ref, 'bn_apply_tiles', 1e-6)      # c32 is rounded
        for mut in ('drop_tile', 'neighbour_plane_c') + (('frame0_mean_inv',) if wi.F > 1 else ()):
            note(mut, 'bn_apply_tiles', case, closed_bn_apply_tiles(y, mi32, c32, L.tflag_out, wi.F, mut, tile), out_ref, out_tol)
        if wi.F > 1:
            m, inv = frame_rows(mi32, L.dout, 'frame0_mean_inv')
            note('frame0_mean_inv', 'bn_background', case, (np.maximum(bg_pre + b, 0) - m) * inv, c_ref, c_tol)


@functools.lru_cache(None)
def forward_with_tap_constants(name):
    """The two rewrites of MVX_FLAG_BG_TAPS, as exact statements about the dense convolution: in an interior tile a depth tap whose
    source halo flag is clear contributes its constant at every site; in a border tile without any flagged source the pre-activation
    is the class constant of the site.  Leaving the constant out / taking the interior one must be visible."""
    wi, inp = BC.wiring(name), BC.inputs(name)
    seen = set()
    for li in (0, 1):
        L, x, c_in, w, b, *_ = BC.layer_tensors(name, li)
        F, H, W = wi.F, wi.H, wi.W
        y_ref = BC.forward(name, li)[0]
        tol = BC.CONV_TOL[3] * float(np.abs(y_ref).max())                # the tightest of the arithmetics
        table = BC.table(name, li)[0]
        P = F * L.dout
        tot, tap, cls = table[:P], table[P:4 * P].reshape(P, 3, C), table[4 * P:].reshape(P, 9, C)
        z = B.conv_relu(x, w, b, L.sd, L.pd, F, relu=False)
        ty, tx = R.tiles_of(H, W)
        border = np.ones((ty, tx), bool)
        border[1:-1, 1:-1] = False
        skipped_out, class_out = z.copy(), z.copy()
        ry = np.where(np.arange(H) == 0, 0, np.where(np.arange(H) == H - 1, 2, 1))
        rx = np.where(np.arange(W) == 0, 0, np.where(np.arange(W) == W - 1, 2, 1))
        q_of = 3 * ry[:, None] + rx[None, :]                     # position class of every site
        n_skip = n_idle = 0
        for kd in range(3):
            wk = np.zeros_like(w)
            wk[:, :, kd] = w[:, :, kd]
            zk = B.conv_relu(x, wk, None, L.sd, L.pd, F, relu=False)
            for p in range(P):
                f, d = divmod(p, L.dout)
                src = src_plane(d, L, kd)
                if src < 0:
                    continue
                flags = [L.hflag_in[f * L.din + s] != 0 for s in (src_plane(d, L, k) for k in range(3)) if s >= 0]
                any_flag = np.logical_or.reduce(flags)
                skip = ~border & any_flag & (L.hflag_in[f * L.din + src] == 0)         # computed interior tile, this tap not executed
                sites = B.tile_sites(skip[None], H, W)[0]
                if sites.any():
                    n_skip += int(skip.sum())
                    assert np.abs(zk[p][sites] - tap[p, kd]).max() <= 1e-12 * float(np.abs(z).max())
                    skipped_out[p][sites] -= tap[p, kd]
        for p in range(P):
            f, d = divmod(p, L.dout)
            flags = [L.hflag_in[f * L.din + s] != 0 for s in (src_plane(d, L, k) for k in range(3)) if s >= 0]
            idle = border & ~np.logical_or.reduce(flags)
            sites = B.tile_sites(idle[None], H, W)[0]
            n_idle += int(idle.sum())
            if sites.any():
                assert np.abs(z[p][sites] - (cls[p][q_of[sites]] + b)).max() <= 1e-12 * float(np.abs(z).max())
                class_out[p][sites] = tot[p] + b
        case = '%s/conv%d' % (name, li + 2)
        print('  %s: %d (tile, tap) pairs skipped in computed interior tiles, %d idle border tiles' % (case, n_skip, n_idle))
        if n_skip:
            note('skipped_tap_left_out', 'conv3d_forward_bg (taps)', case, np.maximum(skipped_out, 0), y_ref, tol)
            seen.add('skip')
        if n_idle:
            note('interior_for_class', 'conv3d_forward_bg (taps)', case, np.maximum(class_out, 0), y_ref, tol)
            seen.add('idle')
    assert seen == {'skip', 'idle'}, seen


@functools.lru_cache(None)
def closed_form_sums(name):
    """plane_tap_sums (tile form), conv3d_input_grad_sums and conv3d_wgrad_bg."""
    wi, inp, t = BC.wiring(name), BC.inputs(name), BC.dense(name)
    F, H, W = wi.F, wi.H, wi.W
    # tap sums of the dyadic gradient, tile form on conv2's backward tiles: exact, tolerance zero -> any change is infinite; use
    # the random-input bound of the GPU test instead (u |ref| + four times an f32 evaluation's distance)
    L2 = wi.conv2
    dz2 = B.f32(t['dz2'])
    ref = B.tap_sums(dz2)
    T32 = B.tap_sums(dz2.astype(np.float32))
    tol = 4 * np.abs(T32 - ref).max() + BC.U * np.abs(ref)
    off = ~B.tile_sites(L2.bflag_out, H, W)
    inact = B.region_sums(dz2, off)
    agree(closed_tap_sums(BC.poison(dz2, ~off), L2.bflag_out, inact), ref, 'tap sums')
    tile = first_tile(L2.bflag_out, 3)
    for mut in ('drop_tile', 'drop_border_correction'):
        note(mut, 'plane_tap_sums (tiles)', name, closed_tap_sums(BC.poison(dz2, ~off), L2.bflag_out, inact, mut, tile), ref, tol)
    dy = BC.dyadic_dz(name, 0)
    assert np.array_equal(closed_tap_sums(dy, L2.bflag_out, B.region_sums(dy, off)), B.tap_sums(dy))       # dyadic: exact
    assert np.array_equal(B.tap_sums(dy), B.tap_sums(dy).astype(np.float32))
    # input gradient sums, stride 1 and stride 2
    for li in (0, 1):
        L = wi.layers[li]
        T, ref, tol = BC.input_grad_sums(name, li)
        agree(closed_input_grad_sums(inp.w[li], T, L, F), ref, 'input_grad_sums')
        if L.sd == 2:
            note('src_plane_shift', 'conv3d_input_grad_sums', '%s/conv%d' % (name, li + 2),
                 closed_input_grad_sums(inp.w[li], T, L, F, 'src_plane_shift'), ref, tol)
        note('drop_border_correction', 'conv3d_input_grad_sums', '%s/conv%d' % (name, li + 2),
             closed_input_grad_sums(inp.w[li], closed_tap_sums(BC.dyadic_dz(name, li), np.ones_like(L.tflag_out), 0.0,
                                                                'drop_border_correction'), L, F), ref, tol)
    # weight gradient
    for li in (0, 1):
        L, x, c_in, w, b, y, mi, x_out, c_out, ybg_out, dz, _ = BC.layer_tensors(name, li)
        ref = BC.wgrad(name, li)
        tol = BC.CONV_TOL[3] * float(np.abs(ref).max())
        T = B.f32(B.tap_sums(dz))
        agree(closed_wgrad(x, c_in, dz, T, L, F), ref, 'wgrad_bg', 1e-6)                                  # T and c_in are rounded
        tile = wgrad_tile(L)
        case = '%s/conv%d' % (name, li + 2)
        muts = ('drop_tile', 'neighbour_plane_c') + (('src_plane_shift',) if L.sd == 2 else ())
        for mut in muts:
            note(mut, 'conv3d_wgrad_bg', case, closed_wgrad(x, c_in, dz, T, L, F, mut, tile, L.hflag_in), ref, tol)
        note('drop_border_correction', 'conv3d_wgrad_bg', case,
             closed_wgrad(x, c_in, dz, closed_tap_sums(dz, np.ones_like(L.tflag_out), 0.0, 'drop_border_correction'), L, F), ref, tol)


def bn_backward_inputs(which):
    """(label, dyhat, y, mi, c, ybg, flags, F, reference dict) of the three BatchNorm-backward cases of the GPU test."""
    if which == 'alone':
        bc = BC.bn_case()
        return 'alone', bc.dyhat, bc.y, bc.mi, bc.c, bc.ybg, bc.flags, bc.F, bc.ref
    name, li = which
    wi, t = BC.wiring(name), BC.dense(name)
    n = li + 2
    ref = BC.bn_backward(name, li)
    return ('%s/layer%d' % (name, n), B.f32(t['g%d' % n]), B.f32(t['y%d' % n]), B.f32(t['mi%d' % n]), B.f32(t['c%d' % n]),
            B.f32(t['ybg%d' % n]), ref['flags'], wi.F, ref)


BN_CASES = ['alone', ('model', -1), ('model', 0), ('wide', -1), ('wide', 0)]


@functools.lru_cache(None)
def batchnorm_backward(which):
    label, dyhat, y, mi, c, ybg, flags, F, ref = bn_backward_inputs(which)
    print('  %s: f32 restatement, relative to the largest element: %s' % (label, ref['f32']))
    A = B.f32(ref['A'])
    on = ~ref['off']
    args = (BC.poison(dyhat, on), y, mi, c, ybg, A, flags, F)
    dz, dbias, inact = closed_bn_backward(*args)
    scale = float(np.abs(ref['dz']).max())
    # the closed form on f32-rounded A, c and (mean, inv) against dense float64: the roundings of its inputs, no more
    assert np.abs(dz - ref['dz'] * on[..., None]).max() <= 1e-5 * scale
    assert np.abs(inact - ref['inact']).max() <= ref['tol_inact'] and np.abs(dbias - ref['dbias']).max() <= ref['tol_dbias']
    if which != 'alone' and which[0] == 'model':
        # the empty frame of layer 1 has no flagged tile: the sums over the "other" tiles are the dense plane sums
        if which[1] == -1:
            wi = BC.wiring('model')
            rows = slice(wi.D1, 2 * wi.D1)
            assert not flags[rows].any() and np.array_equal(ref['inact'][rows], ref['plane'][rows])
    tile = first_tile(flags, 5)
    partial = bool(((np.asarray(flags) == 0)[:, -1, :].any() or (np.asarray(flags) == 0)[:, :, -1].any())
                   and (y.shape[1] % R.TH or y.shape[2] % R.TW))
    muts = ['drop_tile', 'neighbour_plane_c'] + (['frame0_mean_inv'] if F > 1 else []) + (['partial_tile_128'] if partial else [])
    for mut in muts:
        mdz, mdb, min_ = closed_bn_backward(*args, mut, tile)
        # judged on the tiles the mutant still writes (a dropped tile is simply not written: the sentinel check sees that)
        keep = B.tile_sites(without_tile(flags, tile), y.shape[1], y.shape[2])[..., None] if mut == 'drop_tile' else True
        r = [float((np.abs(mdz - dz) * keep).max() / ref['tol_dz']), float(np.abs(mdb - dbias).max() / ref['tol_dbias']),
             float(np.abs(min_ - inact).max() / ref['tol_inact'])]
        best = int(np.argmax(r))
        RATIOS.setdefault(mut, []).append((r[best], 'bn_relu_backward_tiles', label))
        print('  %-24s bn_relu_backward_tiles %-14s dz %9.3g  dbias %9.3g  inactive sums %9.3g  x the tolerance' % ((mut, label) + tuple(r)))
        assert r[best] > FACTOR, (mut, label, r)


@pytest.mark.parametrize('name', NAMES)
def test_table_and_constants_sensitivity(name):
    table_and_constants(name)


@pytest.mark.parametrize('name', NAMES)
def test_forward_with_tap_constants_sensitivity(name):
    forward_with_tap_constants(name)


@pytest.mark.parametrize('name', NAMES)
def test_closed_form_sums_sensitivity(name):
    closed_form_sums(name)


@pytest.mark.parametrize('which', BN_CASES, ids=str)
def test_batchnorm_backward_sensitivity(which):
    batchnorm_backward(which)


def test_every_mutation_moves_a_checked_quantity():
    """Each structural mistake of the list moved at least one quantity by more than 10 x its tolerance (the workers are cached:
    after the tests above this only reads their results)."""
    for name in NAMES:
        table_and_constants(name), forward_with_tap_constants(name), closed_form_sums(name)
    for which in BN_CASES:
        batchnorm_backward(which)
    for mut in MUTATIONS:
        assert mut in RATIOS, mut
        print('  %-24s minimum ratio %.3g (%s, %s)' % ((mut,) + min(RATIOS[mut])))


# ---- 3. argument checks that return before any launch ---------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments_before_any_launch():
    """Dummy host pointers: a launch (or the memset in front of it) on them would fault or give a HIP error; the argument error
    MVX_EINVAL (-1) must come first."""
    from modules import Extension as X
    dummy = (ctypes.c_double * 64)()
    p = ctypes.addressof(dummy)
    big = 1 << 40
    for flags, inact in ((p, None), (None, p)):
        assert X.lib.mvx_plane_tap_sums(p, 3, 9, 17, 64, flags, inact, p, p, big, None) == -1
    good = dict(planes=3, h=9, w=17, channels=64, n_frames=2)

    def bnb(workspace_bytes=big, **kw):
        a = dict(good, **kw)
        return X.lib.mvx_bn_relu_backward_tiles_frames(p, p, p, p, p, p, p, a['planes'], a['h'], a['w'], a['channels'], p, p, p, p, 0, p,
                                                       workspace_bytes, a['n_frames'], None)
    assert bnb(channels=6) == -1 and bnb(channels=62) == -1
    assert bnb(planes=17) == -1
    need = X.lib.mvx_bn_relu_backward_tiles_workspace_bytes_frames(3, 9, 17, 64, 2)
    assert need > 0 and bnb(workspace_bytes=need - 1) == -1
    assert X.lib.mvx_bn_relu_backward_tiles(p, p, p, p, p, p, p, 17, 9, 17, 64, p, p, p, 0, p, big, None) == -1
    for bad in ((0, 64), (3, 0), (-1, 64), (3, -4)):
        assert X.lib.mvx_plane_tap_sums_workspace_bytes(*bad) == 0
    for bad in ((0, 9, 17, 64), (3, 0, 17, 64), (3, 9, 0, 64), (3, 9, 17, 0), (-3, 9, 17, 64), (3, 9, -17, 64)):
        assert X.lib.mvx_bn_relu_backward_tiles_workspace_bytes(*bad) == 0
        assert X.lib.mvx_bn_relu_backward_tiles_workspace_bytes_frames(*bad, 2) == 0
        assert X.lib.mvx_conv3d_wgrad_bg_workspace_bytes(*bad, 64) == 0
        assert X.lib.mvx_conv3d_wgrad_bg_workspace_bytes_frames(*bad, 64, 2) == 0
    assert X.lib.mvx_bn_relu_backward_tiles_workspace_bytes(3, 9, 17, 64) > 0 and X.lib.mvx_conv3d_wgrad_bg_workspace_bytes(3, 9, 17, 64, 64) > 0
    assert X.lib.mvx_bn_relu_backward_tiles_workspace_bytes_frames(3, 9, 17, 64, 0) == 0
    assert X.lib.mvx_conv3d_wgrad_bg_workspace_bytes_frames(3, 9, 17, 64, 64, 0) == 0
