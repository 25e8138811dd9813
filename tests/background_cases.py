"""Inputs and float64 expectations of tests/test_background_host.py and tests/test_background_gpu.py: the CML background chain
behind a synthetic first layer, on the voxel sets of tests/sparse_first_cases.py, and a stand-alone BatchNorm-backward case.
Flags are wired exactly as frames.grid_activity wires them.  Every expectation is a dense float64 operation (background_ref) on
the f32-valued arrays the GPU test uploads; every tolerance is derived there or here, none comes from a kernel."""
import functools
import types

import numpy as np

import background_ref as B
import sparse_first_cases as K
import sparse_ref as R

C = 64
CASES = {'wide': ('wide', 1), 'model': ('model', 4)}       # name -> (geometry of sparse_first_cases, frames); 'model': frame 1 empty
# relative to the tensor maximum, per arithmetic (False: exact f32; 2: bf16x3; 3: bf16x6; 4: fp16x3): the bounds
# tests/test_conv3d_gpu.py::test_conv3d_bf16x3_split_accuracy holds the dense kernels to
CONV_TOL = {False: 1e-5, 2: 2e-5, 3: 4e-6, 4: 4e-6}
U = B.U


class Layer(types.SimpleNamespace):
    """One convolution of the chain: depth geometry, the activity of its input (mask / halo / tile flags, the tiles its input's
    gradient lives on, the tiles of its input that it reads) and of its output."""


@functools.lru_cache(None)
def wiring(name):
    gname, F = CASES[name]
    ch = K.reference_chain(gname, F)
    g = K.geom(gname, F)
    (_, _, _, _, (mask1, halo1, tile1)), (d1, sd2, pd2, _, (mask2, halo2, tile2)), (d2, sd3, pd3, _, (mask3, halo3, tile3)) = ch
    d3 = R.out_depth(d2, sd3, pd3)
    bflag2 = R.tile_dilate(tile1, tile2, d1, d2, sd2, pd2, F)
    reads = [R.tile_read(halo1, d1, d2, sd2, pd2, F), R.tile_read(halo2, d2, d3, sd3, pd3, F)]
    conv2 = Layer(din=d1, dout=d2, sd=sd2, pd=pd2, mask_in=mask1, hflag_in=halo1, tflag_in=tile1, bflag_in=tile1, read_in=reads[0],
                  mask_out=mask2, tflag_out=tile2, bflag_out=bflag2)
    conv3 = Layer(din=d2, dout=d3, sd=sd3, pd=pd3, mask_in=mask2, hflag_in=halo2, tflag_in=tile2, bflag_in=bflag2, read_in=reads[1],
                  mask_out=mask3, tflag_out=tile3, bflag_out=None)
    return types.SimpleNamespace(F=F, H=g.H, W=g.W, D1=d1, conv2=conv2, conv3=conv3, layers=(conv2, conv3))


def normal32(rng, shape, scale=1.0, shift=0.0):
    return (rng.standard_normal(shape) * scale + shift).astype(np.float32).astype(np.float64)


@functools.lru_cache(None)
def inputs(name):
    """f32-valued float64: z1 (random on mask1, one constant per (plane, channel) elsewhere, both signs: about half of the
    background is exactly 0 behind the ReLU), the weights and biases of conv2 / conv3, the upstream gradient G of x3."""
    wi = wiring(name)
    rng = np.random.default_rng(len(name) * 13 + wi.F)
    P1 = wi.F * wi.D1
    k1 = normal32(rng, (P1, C), 0.7)
    z1 = normal32(rng, (P1, wi.H, wi.W, C), 1.0, 0.2)
    z1 = np.where(wi.conv2.mask_in[..., None] != 0, z1, k1[:, None, None, :])
    w2, w3 = (normal32(rng, (C, C, 3, 3, 3), 1.0 / np.sqrt(27 * C)) for _ in range(2))
    b2, b3 = normal32(rng, (C,), 0.5), normal32(rng, (C,), 0.5)
    G = normal32(rng, (wi.F * wi.conv3.dout, wi.H, wi.W, C))
    return types.SimpleNamespace(z1=z1, k1=k1, w2=w2, b2=b2, w3=w3, b3=b3, G=G, w=(w2, w3), b=(b2, b3))


@functools.lru_cache(None)
def dense(name):
    """The float64 chain and what is read off it.  Keys: y1 x1 mi1 .. y3 x3 mi3, g3 dz3 g2 dz2 g1 dz1 (gradients of x / of the
    pre-activation), dw2 db2 dw3 db3; c1 ybg1 c2 ybg2 c3 ybg3 (background of x / y per plane), A2 A1 (plane sums of g2 / g1),
    inact2 (dz2 over the tiles off bflag2), T3 T2 (tap sums), bg_dev (largest deviation of a background site from its plane's
    value over all six tensors)."""
    wi, inp = wiring(name), inputs(name)
    t = B.chain(inp.z1, inp.w2, inp.b2, inp.w3, inp.b3, inp.G, wi.F, (wi.conv2.sd, wi.conv2.pd), (wi.conv3.sd, wi.conv3.pd))
    dev = 0.0
    for li, mask in ((1, wi.conv2.mask_in), (2, wi.conv2.mask_out), (3, wi.conv3.mask_out)):
        for key, src in (('c%d' % li, 'x%d' % li), ('ybg%d' % li, 'y%d' % li)):
            t[key], d = B.background_value(t[src], mask)
            dev = max(dev, d)
    t['bg_dev'] = dev
    t['A2'], t['A1'] = B.plane_sums(t['g2']), B.plane_sums(t['g1'])
    t['inact2'] = B.region_sums(t['dz2'], ~B.tile_sites(wi.conv2.bflag_out, wi.H, wi.W))
    t['T3'], t['T2'] = B.tap_sums(t['dz3']), B.tap_sums(t['dz2'])
    return t


def layer_tensors(name, li):
    """(layer, x_in, c_in, w, b, y, mi, x_out, c_out, ybg_out, dz, g_in) of conv2 (li = 0) / conv3 (li = 1), f32-VALUED float64
    (what a kernel under test is given), dense."""
    wi, inp, t = wiring(name), inputs(name), dense(name)
    n = li + 1
    keys = ('x%d' % n, 'c%d' % n, None, None, 'y%d' % (n + 1), 'mi%d' % (n + 1), 'x%d' % (n + 1), 'c%d' % (n + 1), 'ybg%d' % (n + 1),
            'dz%d' % (n + 1), 'g%d' % n)
    vals = [B.f32(t[k]) if k else None for k in keys]
    vals[2], vals[3] = inp.w[li], inp.b[li]
    return (wi.layers[li],) + tuple(vals)


def poison(a, sites):
    """a with NaN off the sites bool (planes, H, W)."""
    return np.where(np.asarray(sites)[..., None], a, np.nan)


# ---- expectations per kernel: (reference, tolerance), from f32-valued inputs ------------------------------------------------------------
@functools.lru_cache(None)
def table(name, li):
    """mvx_conv3d_background_taps_frames of conv2 / conv3 -> (reference (F * dout * 13, cout), bound)."""
    L, _, c_in, w, *_ = layer_tensors(name, li)
    F = wiring(name).F
    ref = B.bg_table(w, c_in, L.din, L.sd, L.pd, F)
    mag = B.bg_table(np.abs(w), np.abs(c_in), L.din, L.sd, L.pd, F)
    return ref, B.single_rounding_bound(ref, mag, 27 * C + 64)


def bn_background(bg_pre, bias, mi, planes, relu):
    """-> (y_bg, c_out, bound of c_out): y_bg = [ReLU](bg_pre + bias) and c = (y_bg - mean) * inv per frame.  f32 roundings: the
    sum, the difference, the product: at most 3 u (|v| + |m|) inv."""
    F = mi.shape[0]
    v = (0.0 if bg_pre is None else bg_pre) + (0.0 if bias is None else bias)[None, :] + np.zeros((F * planes, mi.shape[2]))
    if relu:
        v = np.maximum(v, 0.0)
    m, inv = np.repeat(mi[:, 0], planes, axis=0), np.repeat(mi[:, 1], planes, axis=0)
    return v, (v - m) * inv, 3 * U * (np.abs(v) + np.abs(m)) * inv


def bn_apply(y, mi):
    """-> ((y - mean) * inv per frame, bound 3 u (|y| + |m|) inv)."""
    F, P = mi.shape[0], y.shape[0]
    m = np.repeat(mi[:, 0], P // F, axis=0)[:, None, None, :]
    inv = np.repeat(mi[:, 1], P // F, axis=0)[:, None, None, :]
    return (y - m) * inv, 3 * U * (np.abs(y) + np.abs(m)) * inv


@functools.lru_cache(None)
def forward(name, li):
    """conv -> ReLU of conv2 / conv3 on the f32-valued input -> (y, per-frame sums (F, 2, C), mean_inv (F, 2, C))."""
    L, x, _, w, b, *_ = layer_tensors(name, li)
    F = wiring(name).F
    y = B.conv_relu(x, w, b, L.sd, L.pd, F)
    per = y.reshape(F, -1, C)
    return y, np.stack([per.sum(1), (per * per).sum(1)], 1), B.mean_inv(y, F)


def mean_inv_bound(y, mi, tol_y):
    """Bound of the (mean, inverse std) a kernel forms from ITS output, every element within tol_y of y: |d mean| <= tol_y,
    |d var| <= (2 rms + tol_y) tol_y + 2 |mean| tol_y (Cauchy-Schwarz on the second moment), d inv = inv^3 d var / 2; plus the
    rounding of the result to f32."""
    F = mi.shape[0]
    rms = np.sqrt((y.reshape(F, -1, y.shape[-1]) ** 2).mean(1))
    m, inv = mi[:, 0], mi[:, 1]
    dvar = (2 * rms + tol_y) * tol_y + 2 * np.abs(m) * tol_y
    return np.stack([tol_y + U * np.abs(m), 0.5 * inv ** 3 * dvar + U * inv], 1)


@functools.lru_cache(None)
def dyadic_dz(name, li):
    L = wiring(name).layers[li]
    wi = wiring(name)
    return K.dyadic(np.random.default_rng(31 + li + wi.F), (wi.F * L.dout, wi.H, wi.W, C))


@functools.lru_cache(None)
def input_grad_sums(name, li):
    """On dyadic dz (its tap sums are exact in f32) -> (T, reference = plane sums of the dense input gradient, bound)."""
    wi, inp = wiring(name), inputs(name)
    L, dz = wi.layers[li], dyadic_dz(name, li)
    ref = B.plane_sums(B.dgrad(dz, inp.w[li], L.din, L.sd, L.pd, wi.F))
    mag = B.plane_sums(B.dgrad(np.abs(dz), np.abs(inp.w[li]), L.din, L.sd, L.pd, wi.F))
    return B.tap_sums(dz), ref, B.single_rounding_bound(ref, mag, 27 * C + wi.H * wi.W)


@functools.lru_cache(None)
def dgrad(name, li):
    """dense input gradient of conv2 / conv3 from the f32-valued dz."""
    L, *_, dz, _ = layer_tensors(name, li)
    return B.dgrad(dz, inputs(name).w[li], L.din, L.sd, L.pd, wiring(name).F)


@functools.lru_cache(None)
def wgrad(name, li):
    L, x, *_, dz, _ = layer_tensors(name, li)
    return B.wgrad(x, dz, L.sd, L.pd, wiring(name).F)


def rank_one(c_in, T, L, F):
    """|c_in| (x) |tap sums| (cout, cin, 3, 3, 3): the magnitude of the closed-form term the background-aware weight gradient adds
    to its gathered part -- the two can cancel, so roundings of the result scale with it, not with the gradient."""
    r = np.zeros((T.shape[2], c_in.shape[1], 3, 9))
    for f in range(F):
        for d in range(L.dout):
            for kd in range(3):
                z = d * L.sd - L.pd + kd
                if 0 <= z < L.din:
                    r[:, :, kd] += np.einsum('c,kn->nck', np.abs(c_in[f * L.din + z]), np.abs(T[f * L.dout + d]))
    return r.reshape(T.shape[2], c_in.shape[1], 3, 3, 3)


@functools.lru_cache(None)
def bn_backward(name, li):
    """BatchNorm + ReLU backward of layer 1 (li = -1) / conv2's output (li = 0) on f32-valued (dyhat, y): dict of dz, dbias,
    inact (sums over the tiles off the flags), the flags, and the three restatement bounds (tol_dz, tol_dbias, tol_inact)."""
    wi, t = wiring(name), dense(name)
    n = li + 2
    flags = wi.conv2.bflag_in if li < 0 else wi.conv2.bflag_out
    return _bn_backward(B.f32(t['g%d' % n]), B.f32(t['y%d' % n]), flags, wi.F)


@functools.lru_cache(None)
def bn_backward_dense(name):
    """The dense BatchNorm + ReLU backward behind conv3 (upstream gradient G), with the same restatement bounds."""
    wi, t = wiring(name), dense(name)
    return _bn_backward(B.f32(t['g3']), B.f32(t['y3']), np.ones_like(wi.conv3.tflag_out), wi.F)


def _bn_backward(dyhat, y, flags, F):
    off = ~B.tile_sites(flags, y.shape[1], y.shape[2])
    dz = B.bn_relu_backward(dyhat, y, F)
    dz32 = B.bn_relu_backward(dyhat, y, F, dtype=B.torch.float32).astype(np.float32)      # the plain f32 evaluation, f32 sums
    db32 = dz32.sum((0, 1, 2), dtype=np.float32)
    inact32 = (dz32 * off[..., None]).sum((1, 2), dtype=np.float32)
    res = dict(dz=dz, dbias=dz.sum((0, 1, 2)), inact=B.region_sums(dz, off), flags=flags, off=off, A=B.plane_sums(dyhat),
               plane=B.plane_sums(dz))
    res['tol_dz'] = B.restatement_bound(dz32, dz)
    res['tol_dbias'] = B.restatement_bound(db32, res['dbias'])
    res['tol_inact'] = B.restatement_bound(inact32, res['inact'])
    # the measured f32 distances, relative to the largest element
    res['f32'] = dict(dz=B.rel_err(dz32, dz), dbias=B.rel_err(db32, res['dbias']), inact=B.rel_err(inact32, res['inact']))
    return res


# ---- the stand-alone BatchNorm backward -----------------------------------------------------------------------------------------------
BN_SHAPE = (2, 3, 152, 304, 16)                    # F, planes, H, W, C: 19 x 19 tiles
BN_UNFLAGGED = (18, 19, 19, 20, 17, 17)            # interior tiles per plane: 2,056 of 2,166 flagged, odd counts up to a plane / frame end


@functools.lru_cache(None)
def bn_case():
    """Synthetic flags (every border tile, 2,056 of 2,166 tiles), y = ReLU(z) with z random on the flagged tiles and one constant
    per (plane, channel) of both signs elsewhere, a dense random dyhat.  -> namespace(flags, y, dyhat, ybg, c, mi, ref)."""
    F, D, H, W, Cn = BN_SHAPE
    ty, tx = R.tiles_of(H, W)
    rng = np.random.default_rng(77)
    flags = np.ones((F * D, ty, tx), np.int32)
    for p, n in enumerate(BN_UNFLAGGED):
        pick = rng.choice((ty - 2) * (tx - 2), n, replace=False)
        flags[p, 1 + pick // (tx - 2), 1 + pick % (tx - 2)] = 0
    on = B.tile_sites(flags, H, W)
    k = normal32(rng, (F * D, Cn), 0.7)
    z = np.where(on[..., None], normal32(rng, (F * D, H, W, Cn), 1.5, 0.2), k[:, None, None, :])
    y = np.maximum(z, 0.0)
    dyhat = normal32(rng, (F * D, H, W, Cn))
    mi = B.f32(B.mean_inv(y, F))
    ybg = np.maximum(k, 0.0)
    c = B.f32((ybg - np.repeat(mi[:, 0], D, 0)) * np.repeat(mi[:, 1], D, 0))
    return types.SimpleNamespace(F=F, D=D, H=H, W=W, C=Cn, flags=flags, y=y, dyhat=dyhat, ybg=ybg, c=c, mi=mi,
                                 ref=_bn_backward(dyhat, y, flags, F))
