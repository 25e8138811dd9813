"""CPU oracle for the MVXNet hot path -- TEST INFRASTRUCTURE ONLY.

This file is a CPU restatement (numpy for the integer / index work, torch-CPU
functional ops for the floating-point layers) of the reference algorithm on
the hot path.  It exists so that the HIP path can be checked; it is never the
thing shipped or measured.  Only ``tests/``, ``__graft_entry__.smoke()`` and
``bench.py``'s ``cpu_baseline`` leg may import it.

Parity pin: the reference ships no tests or golden vectors,
so this oracle is pinned by fixtures generated *from the reference itself*
run in the build container (``oracle/gen_golden.py`` -> ``tests/golden/*.npz``)
and checked in ``tests/test_oracle_golden.py``.

Every function cites the reference lines it follows (paths relative to the
reference root).
"""
from __future__ import annotations

import math
from typing import Dict, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

# ----------------------------------------------------------------------------
# configuration constants (config.yml:3-26, modules/config/Config.py:7-13)
# ----------------------------------------------------------------------------
VELORANGE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]
VOXELSHAPE = [352, 400, 10]
SAMPLENUM = 35
IMSIZE_HW = [370, 1224]
EPS = 1e-6


def voxelsize(velorange=VELORANGE, voxelshape=VOXELSHAPE):
    """modules/config/Config.py:7 -- python-float (f64) true division."""
    return [(velorange[i + 3] - velorange[i]) / voxelshape[i] for i in range(3)]


# ----------------------------------------------------------------------------
# a1: crop / cropTensor  (modules/data/Preprocessing.py:12-17, :19-24)
# ----------------------------------------------------------------------------
def crop_mask(pcd: np.ndarray, rng: Sequence[float], bounds_f32: bool = False) -> np.ndarray:
    """Boolean keep-mask ``low <= xyz < high``.

    numpy path compares the f32 coordinates promoted to f64 with f64 bounds
    (Preprocessing.py:13-16); the torch path rounds the bounds to f32 first
    (Preprocessing.py:20-23) -> ``bounds_f32=True``.
    """
    low = np.asarray(rng[0:3], dtype=np.float64)
    high = np.asarray(rng[3:6], dtype=np.float64)
    if bounds_f32:
        low = low.astype(np.float32).astype(np.float64)
        high = high.astype(np.float32).astype(np.float64)
    roi = pcd[:, :3].astype(np.float64)
    return np.all((low <= roi) & (roi < high), axis=1)


def crop(pcd: np.ndarray, rng: Sequence[float], bounds_f32: bool = False) -> np.ndarray:
    return pcd[crop_mask(pcd, rng, bounds_f32)]


# ----------------------------------------------------------------------------
# a2: cropToSight  (modules/data/Preprocessing.py:26-55)
# ----------------------------------------------------------------------------
def project_cam(pcd: np.ndarray, calib: Dict[str, np.ndarray], dtype=np.float64):
    """(R0_rect @ Tr_velo_to_cam) @ [x y z 1]^T, then P2 @ cam.

    Returns (cam_z, u, v) in ``dtype``.  Association order follows
    Preprocessing.py:46,50 (left-associated matmuls).
    """
    pts = np.ones((4, pcd.shape[0]), dtype=np.float32)
    pts[:3] = pcd[:, :3].T
    r0 = np.asarray(calib['R0_rect'], dtype=dtype)
    tr = np.asarray(calib['Tr_velo_to_cam'], dtype=dtype)
    p2 = np.asarray(calib['P2'], dtype=dtype)
    cam = (r0 @ tr) @ pts.astype(dtype)
    img = p2 @ cam
    with np.errstate(divide='ignore', invalid='ignore'):
        u = img[0] / img[2]
        v = img[1] / img[2]
    return cam[2], u, v


def crop_to_sight_mask(pcd, calib, imsize_wh, dtype=np.float64):
    """Keep-mask of cropToSight; ``imsize_wh`` is (w, h) (Preprocessing.py:28).

    numpy path -> f64 math (calib is f64, cropdata.py:46-56); torch path -> f32.
    """
    lim = np.asarray(imsize_wh, dtype=dtype) - dtype(1e-3)
    z, u, v = project_cam(pcd, calib, dtype)
    front = z > 0
    inside = (u >= 0) & (v >= 0) & (u < lim[0]) & (v < lim[1])
    return front & inside


def crop_to_sight(pcd, calib, imsize_wh, dtype=np.float64):
    return pcd[crop_to_sight_mask(pcd, calib, imsize_wh, dtype)]


# ----------------------------------------------------------------------------
# a3: lidar2Img(uncheck=True)  (modules/utils/Calib.py:47-69)
# ----------------------------------------------------------------------------
def lidar2img(pcd: np.ndarray, calib, dtype=np.float32) -> np.ndarray:
    """(P,2) projected (u, v) = (width coord, height coord); no filtering.

    train.py:31-33 runs this in torch f32 and then swaps to (row, col).
    """
    _, u, v = project_cam(pcd, calib, dtype)
    return np.stack([u, v], axis=1)


# ----------------------------------------------------------------------------
# a4: group  (modules/data/Preprocessing.py:75-116) -- the voxelizer train.py uses
# ----------------------------------------------------------------------------
def voxel_index(xyz: np.ndarray, rng, size) -> np.ndarray:
    """int32 voxel index, f64 true division, truncation toward zero
    (Preprocessing.py:87-90)."""
    low = np.asarray(rng[0:3], dtype=np.float64)
    size = np.asarray(size, dtype=np.float64)
    return ((xyz.astype(np.float64) - low) / size).astype(np.int32)


def _first_appearance(idx: np.ndarray):
    """voxel id per stream point in first-appearance order, plus the rank of
    each point inside its voxel in stream order."""
    n = idx.shape[0]
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), 0
    uniq, first, inv = np.unique(idx, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(first, kind='stable')            # unique-row -> appearance order
    vid_of_uniq = np.empty_like(order)
    vid_of_uniq[order] = np.arange(order.size)
    vid = vid_of_uniq[inv]
    srt = np.argsort(vid, kind='stable')                # stream order kept inside a voxel
    counts = np.bincount(vid, minlength=order.size)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    rank = np.empty(n, np.int64)
    rank[srt] = np.arange(n) - np.repeat(start, counts)
    return vid, rank, order.size


def group(pcd: np.ndarray, perm: np.ndarray, rng, size, T: int
          ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """9-channel voxelizer.

    ``pcd`` (P,6) [x y z r row col]; ``perm`` is the shuffle permutation that
    the reference draws with np.random.shuffle (Preprocessing.py:86) -- an
    explicit input here.  Returns (voxel f64 (V,T,9), uidx f64
    (V,3), cnt int64 (V,)) exactly as Preprocessing.py:105-116: first <=T
    points per voxel in stream order, voxels in first-appearance order,
    centroid over kept points, cols 3:6 = xyz - centroid for all T rows.
    """
    s = pcd[perm]
    idx = voxel_index(s[:, :3], rng, size)
    vid, rank, V = _first_appearance(idx)
    voxel = np.zeros((V, T, 9), dtype=np.float64)
    keep = rank < T
    sv, sr = vid[keep], rank[keep]
    sk = s[keep].astype(np.float64)
    voxel[sv, sr, 0] = sk[:, 0]
    voxel[sv, sr, 1] = sk[:, 1]
    voxel[sv, sr, 2] = sk[:, 2]
    voxel[sv, sr, 6] = sk[:, 3]
    voxel[sv, sr, 7] = sk[:, 4]
    voxel[sv, sr, 8] = sk[:, 5]
    cnt = np.minimum(np.bincount(vid, minlength=V), T).astype(np.int64)
    uidx = np.zeros((V, 3), dtype=np.float64)
    firstpos = np.nonzero(rank == 0)[0]
    uidx[vid[firstpos]] = idx[firstpos]
    if V:
        center = voxel[..., :3].sum(axis=1) / cnt[:, None].astype(np.float64)
        voxel[..., 3:6] = voxel[..., :3] - center[:, None, :]
    return voxel, uidx, cnt


# ----------------------------------------------------------------------------
# a5: group_ + native _group  (Preprocessing.py:57-73, cpp/voxelutil.cpp:325-360)
# ----------------------------------------------------------------------------
def group7(pcd: np.ndarray, perm: np.ndarray, rng, size, T: int):
    """Legacy 7-channel path.  ``pcd`` (P,>=4) f32.  The native part returns
    f32 (V,T,7) with xyz->0:3, r->6 (voxelutil.cpp:345-357); python adds the
    centroid columns: f32 sum over T / int64 cnt (-> f64) and f32 store
    (Preprocessing.py:71-72)."""
    s = pcd[perm]
    idx = voxel_index(s[:, :3], rng, size)
    vid, rank, V = _first_appearance(idx)
    voxel = np.zeros((V, T, 7), dtype=np.float32)
    keep = rank < T
    sv, sr = vid[keep], rank[keep]
    voxel[sv, sr, 0:3] = s[keep, 0:3]
    voxel[sv, sr, 6] = s[keep, 3]
    cnt = np.minimum(np.bincount(vid, minlength=V), T).astype(np.int64)
    uidx = np.zeros((V, 3), dtype=np.int64)
    firstpos = np.nonzero(rank == 0)[0]
    uidx[vid[firstpos]] = idx[firstpos]
    if V:
        center = voxel[..., :3].sum(axis=1) / cnt[:, None]
        voxel[..., 3:6] = voxel[..., :3] - center[:, None, :]
    return voxel, uidx, cnt


# ----------------------------------------------------------------------------
# a6: featureMaping  (modules/imhead/Pipe.py:23-82)
# ----------------------------------------------------------------------------
def feature_mapping(voxels: torch.Tensor, features: Sequence[torch.Tensor],
                    imsize_hw: torch.Tensor, eps: float = EPS):
    """One frame.  ``voxels`` (V,T,9) is MODIFIED IN PLACE like the reference
    (rows with x==y==z==0 get all 9 channels zeroed, Pipe.py:54-59).
    ``features`` = levels of (C,H,W) maps (un-padded).  Returns (V,T,C*levels).

    Sampling (Pipe.py:61-75): q = proj/region - eps, i = trunc(q), f = q - i,
    out = F[i,j] fx fy + F[i+1,j] (1-fx) fy + F[i,j+1] fx (1-fy)
        + F[i+1,j+1] (1-fx)(1-fy)   -- weights as written, not textbook bilinear.
    """
    V, T, _ = voxels.shape
    xyz = voxels[..., :3].reshape(-1, 3)
    zero = torch.all(xyz == 0, dim=1)
    proj = voxels[..., -2:].reshape(-1, 2)
    proj[zero] = 0
    voxels[zero.reshape(V, T)] = 0
    outs = []
    for feat in features:
        C, H, W = feat.shape
        region = imsize_hw / torch.tensor([float(H), float(W)], dtype=imsize_hw.dtype)
        fp = F.pad(feat, (0, 1, 0, 1))
        q = proj / region - eps
        i = q.long()
        fx = (q[:, 0] - i[:, 0])[None]
        fy = (q[:, 1] - i[:, 1])[None]
        r, c = i[:, 0], i[:, 1]
        if r.numel():
            assert int(r.max()) + 1 < fp.shape[-2] and int(c.max()) + 1 < fp.shape[-1]
        o = fp[:, r, c] * fx * fy
        o = o + fp[:, r + 1, c] * (1 - fx) * fy
        o = o + fp[:, r, c + 1] * fx * (1 - fy)
        o = o + fp[:, r + 1, c + 1] * (1 - fx) * (1 - fy)
        outs.append(o)
    out = torch.cat(outs, dim=0).T.reshape(V, T, -1).clone()
    out[zero.reshape(V, T)] = 0
    return out


# ----------------------------------------------------------------------------
# a9: FCN / CRB blocks  (modules/layers/Blocks.py:5-29)
# ----------------------------------------------------------------------------
def _bn_rows(y: torch.Tensor, eps: float) -> torch.Tensor:
    """BatchNorm with batch statistics over every leading dim, per last-dim
    channel, biased variance, no affine (Blocks.py:10; config.yml:19-20).

    A (V,T,C) input is normalised through the same permuted (1,C,V,T) view the
    reference builds (Blocks.py:15-18), so torch-CPU takes the same kernel and
    the fp32 rounding matches the fixtures; in float64 the layout is immaterial.
    """
    if y.dim() == 3:
        out = F.batch_norm(y[None].permute(0, 3, 1, 2), None, None, None, None, True, 0.0, eps)
        return out.permute(0, 2, 3, 1)[0]
    c = y.shape[-1]
    flat = y.reshape(-1, c).T[None]                      # (1, C, R)
    out = F.batch_norm(flat, None, None, None, None, True, 0.0, eps)
    return out[0].T.reshape(y.shape)


def fcn(x, w, b, eps=EPS):
    """Linear -> ReLU -> BN (Blocks.py:14-18)."""
    return _bn_rows(F.relu(F.linear(x, w, b)), eps)


def crb2d_1x1(x, w, b, eps=EPS):
    """CRB2d with a 1x1 kernel on channel-last rows (Blocks.py:31-40, used by
    imhead/Pipe.py:89,91): identical arithmetic to a Linear layer."""
    if x.dim() == 3:                                     # same NCHW view as imhead/Pipe.py:97-99
        y = F.relu(F.conv2d(x[None].permute(0, 3, 1, 2), w, b))
        y = F.batch_norm(y, None, None, None, None, True, 0.0, eps)
        return y.permute(0, 2, 3, 1)[0]
    return _bn_rows(F.relu(F.linear(x, w.reshape(w.shape[0], -1), b)), eps)


def crb3d(x, w, b, stride, pad, eps=EPS):
    """Conv3d -> ReLU -> BN3d on NCDHW (Blocks.py:20-29)."""
    y = F.relu(F.conv3d(x, w, b, stride, pad))
    return F.batch_norm(y, None, None, None, None, True, 0.0, eps)


# ----------------------------------------------------------------------------
# a10/a11: VFE, SVFE, head FCN + max  (modules/voxelnet/Pipe.py:5-29, VoxelNet.py:27-33)
# ----------------------------------------------------------------------------
def vfe(x, w, b, eps=EPS):
    """x (V,T,cin) -> (V,T,2*cout); max over all T rows, no mask (Pipe.py:14-18)."""
    y = fcn(x, w, b, eps)
    s = y.max(dim=1, keepdim=True)[0].expand(-1, y.shape[1], -1)
    return torch.cat([y, s], dim=-1)


def svfe(x, p, prefix='svfe.', eps=EPS):
    x = vfe(x, p[prefix + 'vfe1.fcn.fc.weight'], p[prefix + 'vfe1.fcn.fc.bias'], eps)
    return vfe(x, p[prefix + 'vfe2.fcn.fc.weight'], p[prefix + 'vfe2.fcn.fc.bias'], eps)


def voxel_features(x, p, eps=EPS):
    """(V,T,23) -> (V,128): SVFE -> FCN(128,128) -> max over T (VoxelNet.py:27-33)."""
    x = svfe(x, p, 'svfe.', eps)
    x = fcn(x, p['fcn.fc.weight'], p['fcn.fc.bias'], eps)
    return x.max(dim=1)[0]


# ----------------------------------------------------------------------------
# a12: reindex  (modules/voxelnet/VoxelNet.py:16-22)
# ----------------------------------------------------------------------------
def reindex(x, idx, voxelshape=VOXELSHAPE):
    """(V,128), idx (V,4) long [b ix iy iz] -> (1,128,D,H,W) with D=shape[2],
    H=shape[0], W=shape[1]."""
    res = torch.zeros((1, x.shape[1], voxelshape[2], voxelshape[0], voxelshape[1]), dtype=x.dtype)
    res[idx[:, 0], :, idx[:, 3], idx[:, 1], idx[:, 2]] = x
    return res


# ----------------------------------------------------------------------------
# a13: CML  (modules/voxelnet/Pipe.py:31-43)
# ----------------------------------------------------------------------------
CML_GEOM = (
    ('cml.conv1.conv', (2, 1, 1), (1, 1, 1)),
    ('cml.conv2.conv', (1, 1, 1), (0, 1, 1)),
    ('cml.conv3.conv', (2, 1, 1), (1, 1, 1)),
)


def cml(x, p, eps=EPS):
    for name, stride, pad in CML_GEOM:
        x = crb3d(x, p[name + '.weight'], p[name + '.bias'], stride, pad, eps)
    return x


def voxelnet_middle(x, idx, p, voxelshape=VOXELSHAPE, eps=EPS):
    """VoxelNet.forward up to the RPN input (VoxelNet.py:27-36):
    (V,T,23), (V,4) -> (1,128,H,W) with channel = c*2+d."""
    f = voxel_features(x, p, eps)
    g = reindex(f, idx, voxelshape)
    y = cml(g, p, eps)
    return y.reshape(1, -1, voxelshape[0], voxelshape[1])


# ----------------------------------------------------------------------------
# f1: RPN  (modules/voxelnet/Pipe.py:45-75; CRB2d / DeCRB2d of modules/layers/Blocks.py:31-51)
# ----------------------------------------------------------------------------
def crb2d(x, w, b, stride, pad, eps=EPS):
    """Conv2d -> ReLU -> BN2d on NCHW (Blocks.py:31-40)."""
    y = F.relu(F.conv2d(x, w, b, stride, pad))
    return F.batch_norm(y, None, None, None, None, True, 0.0, eps)


def decrb2d(x, w, b, stride, pad, eps=EPS):
    """ConvTranspose2d -> ReLU -> BN2d on NCHW (Blocks.py:42-51)."""
    y = F.relu(F.conv_transpose2d(x, w, b, stride, pad))
    return F.batch_norm(y, None, None, None, None, True, 0.0, eps)


def rpn(x, p, prefix='rpn.', eps=EPS):
    """(1,128,H,W) -> (score (1,2,H/2,W/2), reg (1,14,H/2,W/2)) (Pipe.py:45-75)."""
    def blk(x, name, n):
        for i in range(n):
            x = crb2d(x, p['%s%s.%d.conv.weight' % (prefix, name, i)], p['%s%s.%d.conv.bias' % (prefix, name, i)], 2 if i == 0 else 1, 1, eps)
        return x
    x1 = blk(x, 'blk1', 4)
    x2 = blk(x1, 'blk2', 6)
    x3 = blk(x2, 'blk3', 6)
    ups = [decrb2d(x1, p[prefix + 'deconv1.deconv.weight'], p[prefix + 'deconv1.deconv.bias'], 1, 1, eps),
           decrb2d(x2, p[prefix + 'deconv2.deconv.weight'], p[prefix + 'deconv2.deconv.bias'], 2, 0, eps),
           decrb2d(x3, p[prefix + 'deconv3.deconv.weight'], p[prefix + 'deconv3.deconv.bias'], 4, 0, eps)]
    up = torch.cat(ups, dim=1)
    score = torch.sigmoid(F.conv2d(up, p[prefix + 'cls.weight'], p[prefix + 'cls.bias']))
    return score, F.conv2d(up, p[prefix + 'reg.weight'], p[prefix + 'reg.bias'])


def rpn_params(golden_rpn_shapes, dtype=torch.float32):
    """The deterministic RPN tensors the reference fixtures were generated with (make_rpn_param per state-dict key)."""
    out = {}
    for name, shape in zip(golden_rpn_shapes['names'], golden_rpn_shapes['shapes']):
        shape = tuple(int(v) for v in shape if v != 0)
        out[str(name)] = make_rpn_param(str(name), shape).to(dtype)
    return out


# ----------------------------------------------------------------------------
# a7: ImageFeatureFusion  (modules/imhead/Pipe.py:84-104)
# ----------------------------------------------------------------------------
def image_feature_fusion(x, p, prefix='', eps=EPS):
    """(V,T,768) -> (V,T,16)."""
    x = fcn(x, p[prefix + 'fcn1.fc.weight'], p[prefix + 'fcn1.fc.bias'], eps)
    x = crb2d_1x1(x, p[prefix + 'conv1.conv.weight'], p[prefix + 'conv1.conv.bias'], eps)
    x = fcn(x, p[prefix + 'fcn2.fc.weight'], p[prefix + 'fcn2.fc.bias'], eps)
    x = crb2d_1x1(x, p[prefix + 'conv2.conv.weight'], p[prefix + 'conv2.conv.bias'], eps)
    x = fcn(x, p[prefix + 'fcn3.fc.weight'], p[prefix + 'fcn3.fc.bias'], eps)
    return x


# ----------------------------------------------------------------------------
# a8: MVXNet.forward glue minus the frozen extractor  (MVXNet.py:21-27, Head.py:14-22)
# ----------------------------------------------------------------------------
def mvx_point_features(voxels, features, imsize_hw, p, eps=EPS):
    """voxels (V,T,9) (modified in place), FPN levels -> (V,T,23)."""
    imf = feature_mapping(voxels, features, imsize_hw, eps)
    imf = image_feature_fusion(imf, p, 'head.fusion.', eps)
    return torch.cat([voxels[..., :7], imf], dim=-1)


# ----------------------------------------------------------------------------
# deterministic parameters and synthetic frames
# ----------------------------------------------------------------------------
PARAM_SHAPES = {
    'backbone.svfe.vfe1.fcn.fc.weight': (16, 23), 'backbone.svfe.vfe1.fcn.fc.bias': (16,),
    'backbone.svfe.vfe2.fcn.fc.weight': (64, 32), 'backbone.svfe.vfe2.fcn.fc.bias': (64,),
    'backbone.fcn.fc.weight': (128, 128), 'backbone.fcn.fc.bias': (128,),
    'backbone.cml.conv1.conv.weight': (64, 128, 3, 3, 3), 'backbone.cml.conv1.conv.bias': (64,),
    'backbone.cml.conv2.conv.weight': (64, 64, 3, 3, 3), 'backbone.cml.conv2.conv.bias': (64,),
    'backbone.cml.conv3.conv.weight': (64, 64, 3, 3, 3), 'backbone.cml.conv3.conv.bias': (64,),
    'head.fusion.fcn1.fc.weight': (768, 768), 'head.fusion.fcn1.fc.bias': (768,),
    'head.fusion.conv1.conv.weight': (128, 768, 1, 1), 'head.fusion.conv1.conv.bias': (128,),
    'head.fusion.fcn2.fc.weight': (128, 128), 'head.fusion.fcn2.fc.bias': (128,),
    'head.fusion.conv2.conv.weight': (16, 128, 1, 1), 'head.fusion.conv2.conv.bias': (16,),
    'head.fusion.fcn3.fc.weight': (16, 16), 'head.fusion.fcn3.fc.bias': (16,),
}


def lcg_uniform(n: int, seed: int) -> np.ndarray:
    """torch-independent integer PRNG -> uniform f64 in [-1, 1).  A 64-bit LCG
    (Knuth MMIX constants) so fixtures can be regenerated anywhere."""
    a = np.uint64(6364136223846793005)
    c = np.uint64(1442695040888963407)
    out = np.empty(n, dtype=np.float64)
    # vectorised jump-free generation: iterate in python for small n only
    s = np.uint64(seed * 2654435761 % (1 << 63) + 1)
    with np.errstate(over='ignore'):
        for i in range(n):
            s = s * a + c
            out[i] = float(int(s >> np.uint64(11))) / float(1 << 53)
    return out * 2.0 - 1.0


def fast_uniform(n: int, seed: int) -> np.ndarray:
    """Counter-based integer hash (splitmix64) -> uniform f64 in [-1,1);
    vectorised, used for the larger parameter tensors."""
    with np.errstate(over='ignore'):
        z = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) / float(1 << 53) * 2.0 - 1.0


def make_params(seed: int = 7, dtype=torch.float32, names=None) -> Dict[str, torch.Tensor]:
    """Deterministic weights: uniform(-k, k), k = 1/sqrt(fan_in) (the scale of
    PyTorch's default Linear/Conv init), from the integer hash above."""
    out = {}
    for j, (name, shape) in enumerate(PARAM_SHAPES.items()):
        if names is not None and name not in names:
            continue
        n = int(np.prod(shape))
        if name.endswith('weight'):
            fan_in = int(np.prod(shape[1:]))
        else:
            fan_in = int(np.prod(PARAM_SHAPES[name[:-4] + 'weight'][1:]))
        k = 1.0 / math.sqrt(fan_in)
        vals = fast_uniform(n, seed * 1000 + j) * k
        out[name] = torch.from_numpy(vals.reshape(shape)).to(dtype)
    return out


def make_rpn_param(name: str, shape) -> torch.Tensor:
    """Deterministic RPN tensor (modules/voxelnet/Pipe.py:45-75 shapes) for fixtures."""
    n = int(np.prod(shape))
    seed = 500 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003
    fan = int(np.prod(shape[1:])) if len(shape) > 1 else 64
    return torch.from_numpy((fast_uniform(n, seed) / math.sqrt(max(1, fan))).reshape(shape)).float()


def strip_prefix(p: Dict[str, torch.Tensor], prefix: str) -> Dict[str, torch.Tensor]:
    return {k[len(prefix):]: v for k, v in p.items() if k.startswith(prefix)}


# ----------------------------------------------------------------------------
# anchors, target assignment, loss
# ----------------------------------------------------------------------------
CARSIZE = [3.9, 1.6, 1.56]


def create_anchors(l: int, w: int, rng=VELORANGE, size=CARSIZE) -> torch.Tensor:
    """(l, w, 14): two 7-dof anchors (yaw 0, pi/2) per BEV cell, z = -1
    (modules/data/Preprocessing.py:118-142)."""
    ls, ws = (rng[3] - rng[0]) / l, (rng[4] - rng[1]) / w
    x = torch.linspace(rng[0] + ls / 2, rng[3] - ls / 2, l)
    y = torch.linspace(rng[1] + ws / 2, rng[4] - ws / 2, w)
    gx, gy = torch.meshgrid(x, y, indexing='ij')
    cols = [gx[..., None], gy[..., None], torch.full((l, w, 1), -1.0), torch.Tensor(size).tile((l, w, 1))]
    a0 = torch.concat(cols + [torch.zeros((l, w, 1))], dim=2)
    a1 = torch.concat(cols + [torch.full((l, w, 1), torch.pi / 2)], dim=2)
    return torch.concat([a0, a1], dim=2)


def bbox3d2bev(boxes: torch.Tensor) -> torch.Tensor:
    """(..., 7) xyzlwhr -> BEV corner points (..., 4, 2) (modules/Calc.py:15-38): unit square corners
    scaled by (l, w), multiplied from the RIGHT by [[cos, -sin], [sin, cos]], shifted by (x, y)."""
    shape = boxes.shape[:-1]
    b = boxes.reshape(-1, boxes.shape[-1])
    unit = torch.Tensor([[0.5, 0.5], [-0.5, 0.5], [-0.5, -0.5], [0.5, -0.5]])
    res = torch.tile(unit, (b.shape[0], 1, 1)) * b[:, None, [3, 4]]
    c, s_ = torch.cos(b[:, 6]).reshape(-1, 1), torch.sin(b[:, 6]).reshape(-1, 1)
    rot = torch.concat([c, -s_, s_, c], dim=1).reshape(-1, 2, 2)
    res = res @ rot + b[:, None, [0, 1]]
    return res.reshape(shape + (4, 2)) if len(shape) else res[0]


_ORACLE_C = None


def _oracle_c():
    global _ORACLE_C
    if _ORACLE_C is None:
        import ctypes
        _ORACLE_C = ctypes.CDLL(_os.path.join(_os.path.dirname(_os.path.abspath(__file__)), 'liboracle_c.so'))
        _ORACLE_C.oracle_anchor_stale_reads.restype = ctypes.c_int64
    return _ORACLE_C


def _f32p(a):
    import ctypes
    return a.ctypes.data_as(ctypes.c_void_p)


def bbox_pairwise(b1: np.ndarray, b2: np.ndarray, iou: bool) -> np.ndarray:
    """IoU (``cpp.bboxOverlap``) or intersection area (``cpp.bboxIntersection``) of every BEV box pair,
    (N,4,2) x (M,4,2) -> (N,M) f32, with the corner-index fix described in oracle/anchors_c.c
    (cpp/voxelutil.cpp:96-136)."""
    import ctypes
    b1 = np.ascontiguousarray(b1, np.float32)
    b2 = np.ascontiguousarray(b2, np.float32)
    out = np.empty((b1.shape[0], b2.shape[0]), np.float32)
    _oracle_c().oracle_bbox_pairwise(_f32p(b1), ctypes.c_int64(b1.shape[0]), _f32p(b2), ctypes.c_int64(b2.shape[0]),
                                     ctypes.c_int(1 if iou else 0), _f32p(out))
    return out


def classify_anchors_cells(gts: np.ndarray, anchors: np.ndarray, nls: np.ndarray, nws: np.ndarray,
                           neg_thr: float, pos_thr: float):
    """``cpp._classifyAnchors`` (cpp/voxelutil.cpp:138-316): gts (G,4,2) f32, anchors (L,W,A,4,2) f32,
    centre cells nls/nws i64 (G,) -> ((px,py,pz), (nx,ny,nz), gi) int64 arrays in the reference's order."""
    import ctypes
    gts = np.ascontiguousarray(gts, np.float32)
    anchors = np.ascontiguousarray(anchors, np.float32)
    nls = np.ascontiguousarray(nls, np.int64)
    nws = np.ascontiguousarray(nws, np.int64)
    L, W, A = anchors.shape[:3]
    G = gts.shape[0]
    cap = max(1, L * W * A * max(1, G))
    cap = min(cap, 1 << 24)
    bufs = [np.empty(cap, np.int64) for _ in range(7)]
    counts = np.zeros(2, np.int64)
    _oracle_c().oracle_classify_anchors(_f32p(gts), ctypes.c_int64(G), _f32p(anchors), ctypes.c_int64(L), ctypes.c_int64(W),
                                        ctypes.c_int64(A), _f32p(nls), _f32p(nws), ctypes.c_float(neg_thr),
                                        ctypes.c_float(pos_thr), *[_f32p(b) for b in bufs], _f32p(counts))
    npos, nneg = int(counts[0]), int(counts[1])
    return (tuple(b[:npos].copy() for b in bufs[0:3]), tuple(b[:nneg].copy() for b in bufs[3:6]), bufs[6][:npos].copy())


def anchor_center_cells(gt_centers: torch.Tensor, anchors_shape, rng=VELORANGE):
    """Centre cell of every ground truth (modules/Calc.py:91-94), torch f32 arithmetic then .long()."""
    l = (rng[3] - rng[0]) / anchors_shape[0]
    w = (rng[4] - rng[1]) / anchors_shape[1]
    nls = ((gt_centers[:, 0] - rng[0] - l / 2) / l + 0.5).long()
    nws = ((gt_centers[:, 1] - rng[1] - w / 2) / w + 0.5).long()
    return nls, nws


def classify_anchors(gts_bev: torch.Tensor, gt_centers: torch.Tensor, anchor_bevs: torch.Tensor, rng, neg_thr, pos_thr):
    """modules/Calc.py:88-96."""
    nls, nws = anchor_center_cells(gt_centers, anchor_bevs.shape, rng)
    return classify_anchors_cells(gts_bev.numpy(), anchor_bevs.numpy(), nls.numpy(), nws.numpy(), neg_thr, pos_thr)


def make_loss_inputs(L: int, W: int, seed: int):
    """Deterministic RPN outputs for the loss fixtures: score (L,W,2) in (0,1), reg (L,W,14)."""
    score = torch.sigmoid(torch.from_numpy(fast_uniform(L * W * 2, seed).reshape(L, W, 2)).float() * 3)
    reg = torch.from_numpy(fast_uniform(L * W * 14, seed + 10).reshape(L, W, 14)).float() * 0.5
    return score, reg


def voxel_loss(pi, ni, gi, gts, score, reg, anchors, anchors_per_loc, a=1.5, b=1.0, eps=EPS):
    """VoxelLoss.forward (modules/voxelnet/Loss.py:15-45).  score (L,W,A), reg (L,W,7A); pi / ni index triples,
    gi ground-truth id per positive; returns (clsLoss, regLoss or None)."""
    if pi is None:
        return -torch.log(1 - score + eps).mean(), None
    pi = tuple(torch.as_tensor(np.asarray(t)).long() for t in pi)
    ni = tuple(torch.as_tensor(np.asarray(t)).long() for t in ni)
    gi = torch.as_tensor(np.asarray(gi)).long()
    pos = -torch.log(score[pi] + eps).sum()
    neg_all = -torch.log(1 - score + eps)
    size_sum = neg_all.shape[0] * neg_all.shape[1] * neg_all.shape[2]
    neg = neg_all.sum() - neg_all[ni].sum()            # a cell listed twice in ni is subtracted twice, as in the reference
    pos = pos / (pi[0].shape[0] + eps)
    neg = neg / (size_sum - ni[0].shape[0] + eps)
    cls = a * pos + b * neg
    if len(pi[0]) == 0:
        return cls, None
    g = gts[gi]
    an = anchors.reshape((anchors.shape[0], anchors.shape[1], anchors_per_loc, 7))[pi]
    d = torch.sqrt(an[:, 3] ** 2 + an[:, 4] ** 2)[:, None]
    t = torch.empty_like(g)
    t[:, [0, 1]] = (g[:, [0, 1]] - an[:, [0, 1]]) / d
    t[:, 2] = (g[:, 2] - an[:, 2]) / an[:, 5]
    t[:, 3:6] = torch.log(g[:, 3:6] / an[:, 3:6])
    t[:, 6] = g[:, 6] - an[:, 6]
    r = reg.reshape((reg.shape[0], reg.shape[1], anchors_per_loc, 7))[pi]
    return cls, F.smooth_l1_loss(r, t)                 # nn.SmoothL1Loss(): mean over N*7, beta = 1


# Synthetic KITTI-shaped frames and the calibration live in the package (bench.py uses them and
# may not import oracle/); re-exported here for the tests.
import os as _os
import sys as _sys
_PKG = _os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), 'mvxnet-makise_amd')
if _PKG not in _sys.path:
    _sys.path.insert(0, _PKG)
from modules.data.Synthetic import (KITTI_CALIB, synth_fpn, synth_perm, synth_raw, synth_ring,  # noqa: E402,F401
                                    synth_uniform)


# Inputs of the fixtures made from the reference's compiled extension (oracle/gen_ref_binary_golden.py ->
# tests/golden/ref_*.npz, checked in tests/test_ref_extension.py)
def ref_binary_frame(kind: str, fid: int, n: int = 20000):
    """(points (n,4) f32 in shuffled order, their voxel indices (n,3) i32): the `_group` arguments of a synthetic frame."""
    pc4 = synth_uniform(fid, n) if kind == 'uniform' else synth_ring(fid, n)
    perm = synth_perm(fid, pc4.shape[0])
    s = np.ascontiguousarray(pc4[perm][:, :4], np.float32)
    idx = voxel_index(s[:, :3], VELORANGE, voxelsize())
    return s, np.ascontiguousarray(idx, np.int32)


def ref_binary_boxes(seed: int, n: int = 8) -> torch.Tensor:
    """n random car boxes (xyzlwhr, f32) inside the range: the ground truth of the `_classifyAnchors` fixtures."""
    g = np.random.default_rng(seed)
    gt = np.stack([g.uniform(5, 65, n), g.uniform(-35, 35, n), g.uniform(-1.8, -0.6, n), g.uniform(3.4, 4.4, n),
                   g.uniform(1.5, 1.8, n), g.uniform(1.4, 1.7, n), g.uniform(-1.6, 1.6, n)], 1).astype(np.float32)
    return torch.from_numpy(gt)


def array_digest(*arrays) -> str:
    """SHA-256 over dtype, shape and bytes of each array: pins a regenerated input to the one a fixture was made from."""
    import hashlib
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(('%s%s' % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()
