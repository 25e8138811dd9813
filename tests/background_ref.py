"""Float64 reference of the CML background rewrite (csrc/activity.hip, the closed-form kernels of csrc/conv3d.hip): the DENSE
operation plus masking, torch-CPU autograd and numpy.  Nothing here restates a closed form of the library: the constants of the
background, the plane sums, the sums over the unflagged tiles and the border classes are READ OFF dense tensors (a convolution
of a constant image, a sum over sites).  tests/test_background_host.py checks the properties these read-offs rely on, and holds
its own restatement of the closed forms against them.

Layout: channels-last numpy arrays (F * planes, H, W, C), the frames stacked along depth as in the library; `cl` / `nc` convert
from and to torch's (F, C, D, H, W).  BatchNorm: per frame over D * H * W, biased variance, eps 1e-6, no affine."""
import numpy as np
import torch
import torch.nn.functional as Fn

import sparse_ref as R

EPS = 1e-6
U = 2.0 ** -24                                    # unit roundoff of f32
TH, TW = R.TH, R.TW


def f32(a):
    """The values an upload as f32 holds, as float64."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def nc(a, F, dtype=torch.float64):
    a = torch.as_tensor(np.ascontiguousarray(a)).to(dtype)
    FD, H, W, C = a.shape
    return a.reshape(F, FD // F, H, W, C).permute(0, 4, 1, 2, 3).contiguous()


def cl(t):
    F, C, D, H, W = t.shape
    return t.detach().permute(0, 2, 3, 4, 1).reshape(F * D, H, W, C).double().numpy().copy()


def conv(x, w, b, sd, pd):
    return Fn.conv3d(x, w, b, (sd, 1, 1), (pd, 1, 1))


def bn(y):
    """-> (normalised y, mean [F][C], 1 / sqrt(var + eps) [F][C])."""
    m = y.mean((2, 3, 4), keepdim=True)
    inv = (((y - m) ** 2).mean((2, 3, 4), keepdim=True) + EPS).rsqrt()
    return (y - m) * inv, m.flatten(1), inv.flatten(1)


def mean_inv(y_cl, F):
    """f64 (F, 2, C): what mvx_bn_finalize forms from the sums of y."""
    _, m, inv = bn(nc(y_cl, F))
    return torch.stack([m, inv], 1).numpy()


# ---- the dense chain behind a synthetic first layer ----------------------------------------------------------------------------------
def chain(z1, w2, b2, w3, b3, G, F, geom2, geom3):
    """x1 = BN(ReLU(z1)); conv2 -> ReLU -> BN; conv3 -> ReLU -> BN; loss = sum(G * x3).  geom = (sd, pd).  Returns every tensor of
    the forward and every gradient of the backward, channels-last float64."""
    t = {}
    z1t = nc(z1, F).requires_grad_(True)
    w2t, b2t, w3t, b3t = (torch.as_tensor(np.asarray(a, np.float64)).requires_grad_(True) for a in (w2, b2, w3, b3))
    y1 = torch.relu(z1t)
    x1, m1, i1 = bn(y1)
    z2 = conv(x1, w2t, b2t, *geom2)
    y2 = torch.relu(z2)
    x2, m2, i2 = bn(y2)
    z3 = conv(x2, w3t, b3t, *geom3)
    y3 = torch.relu(z3)
    x3, m3, i3 = bn(y3)
    loss = (nc(G, F) * x3).sum()
    g = torch.autograd.grad(loss, [z1t, x1, z2, x2, z3, w2t, b2t, w3t, b3t])
    for k, v in dict(y1=y1, x1=x1, y2=y2, x2=x2, y3=y3, x3=x3, dz1=g[0], g1=g[1], dz2=g[2], g2=g[3], dz3=g[4]).items():
        t[k] = cl(v)
    for k, (m, i) in dict(mi1=(m1, i1), mi2=(m2, i2), mi3=(m3, i3)).items():
        t[k] = torch.stack([m, i], 1).detach().numpy()
    for k, v in dict(dw2=g[5], db2=g[6], dw3=g[7], db3=g[8]).items():
        t[k] = v.numpy()
    t['g3'] = np.asarray(G, np.float64)
    return t


# ---- the dense operations of single kernels, on the (f32-valued) inputs the kernel gets -----------------------------------------------
def conv_relu(x_cl, w, b, sd, pd, F, relu=True):
    z = conv(nc(x_cl, F), torch.as_tensor(np.asarray(w, np.float64)), None if b is None else torch.as_tensor(np.asarray(b, np.float64)),
             sd, pd)
    return cl(torch.relu(z) if relu else z)


def dgrad(dz_cl, w, din, sd, pd, F):
    """dense input gradient (F * din, H, W, cin) of the convolution."""
    dz = nc(dz_cl, F)
    w = torch.as_tensor(np.asarray(w, np.float64))
    size = (F, w.shape[1], din, dz.shape[3], dz.shape[4])
    return cl(torch.nn.grad.conv3d_input(size, w, dz, (sd, 1, 1), (pd, 1, 1)))


def wgrad(x_cl, dz_cl, sd, pd, F):
    """dense weight gradient (cout, cin, 3, 3, 3), summed over the frames."""
    x, dz = nc(x_cl, F), nc(dz_cl, F)
    return torch.nn.grad.conv3d_weight(x, (dz.shape[1], x.shape[1], 3, 3, 3), dz, (sd, 1, 1), (pd, 1, 1)).numpy()


def bn_relu_backward(dyhat_cl, y_cl, F, dtype=torch.float64):
    """dense dz of ReLU -> BatchNorm given dL/d(BN output) and the ReLU output y, by autograd in `dtype` (float32: what a plain
    f32 evaluation gives, the yardstick of the kernels' tolerances)."""
    z = nc(y_cl, F, dtype).requires_grad_(True)                 # ReLU(y) = y and [z > 0] = [y > 0]
    yh, _, _ = bn(torch.relu(z))
    (dz,) = torch.autograd.grad((nc(dyhat_cl, F, dtype) * yh).sum(), [z])
    return cl(dz)


# ---- reading restricted quantities off dense tensors ---------------------------------------------------------------------------------
def tile_sites(flags, H, W):
    return R.tile_sites(flags, H, W)


def background_value(t_cl, mask):
    """-> (value (planes, C) at the first site of each plane with mask == 0 (NaN where a plane has none), the largest distance of
    any other such site from it)."""
    P, H, W, C = t_cl.shape
    val, dev = np.full((P, C), np.nan), 0.0
    for p in range(P):
        rows = t_cl[p][np.asarray(mask[p]) == 0]
        if len(rows):
            val[p] = rows[0]
            dev = max(dev, float(np.abs(rows - rows[0]).max()))
    return val, dev


def plane_sums(t_cl):
    return t_cl.sum((1, 2))


def region_sums(t_cl, sites):
    """sum over the sites bool (planes, H, W) -> (planes, C)."""
    return (t_cl * np.asarray(sites)[..., None]).sum((1, 2))


def tap_sums(dz_cl):
    """(planes, 9, C): per in-plane tap (a, b), the sum of dz over the sites whose tap source (y + a - 1, x + b - 1) lies inside
    the image (the border rule of mvx_plane_tap_sums in the header)."""
    P, H, W, C = dz_cl.shape
    T = np.empty((P, 9, C))
    for a in range(3):
        ys = slice(max(0, 1 - a), H - max(0, a - 1))
        for b in range(3):
            xs = slice(max(0, 1 - b), W - max(0, b - 1))
            T[:, a * 3 + b] = dz_cl[:, ys, xs].sum((1, 2))
    return T


def bg_table(w, c_in, din, sd, pd, F):
    """The table of mvx_conv3d_background_taps_frames, (F * dout * 13, cout) float64: totals | three depth taps | nine border
    classes, each read off the dense convolution of a constant image.  On a 3 x 3 image with c_in[plane] at every site, site
    (ry, rx) is an image corner / edge / interior site of class 3 * ry + rx, and (1, 1) is the interior."""
    w = torch.as_tensor(np.asarray(w, np.float64))
    cin = w.shape[1]
    img = torch.as_tensor(np.asarray(c_in, np.float64)).reshape(F, din, cin).permute(0, 2, 1)[:, :, :, None, None].expand(F, cin, din, 3, 3)
    z = conv(img, w, None, sd, pd)                                       # (F, cout, dout, 3, 3)
    P, cout = F * z.shape[2], w.shape[0]
    totals = z[:, :, :, 1, 1].permute(0, 2, 1).reshape(P, cout)
    classes = z.permute(0, 2, 3, 4, 1).reshape(P * 9, cout)
    taps = []
    for kd in range(3):
        wk = torch.zeros_like(w)
        wk[:, :, kd] = w[:, :, kd]
        taps.append(conv(img, wk, None, sd, pd)[:, :, :, 1, 1].permute(0, 2, 1).reshape(P, cout))
    taps = torch.stack(taps, 1).reshape(P * 3, cout)
    return torch.cat([totals, taps, classes]).numpy()


# ---- bounds ------------------------------------------------------------------------------------------------------------------------
def single_rounding_bound(ref, magnitude, n):
    """|f32(s) - ref| for s an f64 accumulation of n terms rounded once to f32: one ulp of f32 (2 u relative) and the f64
    accumulation errors of the kernel and of this reference, n * 2^-53 * sum |terms| each."""
    return 2 * U * np.abs(ref) + 2 * n * 2.0 ** -53 * np.asarray(magnitude)


def restatement_bound(f32_result, ref):
    """Four times the distance of a plain f32 evaluation from float64 (the factor covers another summation order) plus one
    rounding of the largest element."""
    return 4 * float(np.abs(np.asarray(f32_result) - ref).max()) + U * float(np.abs(ref).max())


def rel_err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(1e-300, np.abs(b).max()))
