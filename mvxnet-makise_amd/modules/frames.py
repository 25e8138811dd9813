"""Frame sets: all frames of a step through ONE launch per layer.

The reference is strictly batch-1 (config.yml:18; modules/voxelnet/VoxelNet.py:19; MVXNet.py:23-24), so a batch of
B frames means B independent forwards with per-frame BatchNorm statistics and summed parameter gradients
(SURVEY.md 8e).  ``modules/tape.py`` runs them one after the other (about 170 launches per frame); this module runs the
same chain -- MVXNet.middle on compact rows: fusion sampling + fusion MLP (imhead/Pipe.py:23-104), the concat of
MVXNet.py:26, SVFE + FCN + max (voxelnet/Pipe.py:5-29, VoxelNet.py:27-33), reindex + CML (VoxelNet.py:16-36,
voxelnet/Pipe.py:31-43) -- ONCE for the whole frame set through the ``*_frames`` entry points of the C ABI: row
matrices hold the frames back to back, grids stack them along the depth axis, every per-frame quantity carries a
leading frame dimension.  Same kernels, same arithmetic per frame; parameter gradients are summed over the frames by
the reductions themselves.

Weight-gradient kernels go to the side stream (modules/_hip.py), everything else stays on the caller's stream.
"""
import os

import torch

import modules.config as cfg
from modules import _hip
from modules import bn_running as bnr
from modules import Extension as X
from modules.layers.Blocks import conv_background_on, conv_split_math

R = _hip.STATS_REPLICAS


class FrameSet:
    """Voxels of F frames back to back + the compact-row bookkeeping every layer needs.

    voxels f32 (Vt, T, 9), coords i64 (Vt, 4); vox_off / real_off: host lists (F+1)."""

    def __init__(self, voxels, coords, vox_off, T):
        self.voxels, self.coords = voxels, coords
        self.vox_off = [int(v) for v in vox_off]
        self.F, self.T = len(vox_off) - 1, int(T)
        self.Vt = self.vox_off[-1]
        self.real_off = None
        self.desc = None
        self.sampled = None          # (FPN features of the real rows, status word) when sampled with the preparation (sample_rows)
        self.grid = None             # voxel index grid + activity masks / tile flags of the three CML layers (grid_activity), same

    # -- step 1 (enqueue only): dense-row -> compact-row map of all frames, real-row offsets stay on the device
    def enqueue_map(self):
        rows = self.Vt * self.T
        vox2d = self.voxels.view(rows, self.voxels.shape[-1])
        self.vox2d = vox2d
        d0 = X.FramesDesc.make(self.vox_off, [0] * (self.F + 1), self.T)
        self.row_map, self.rows_sel, self.n_real_dev, self.real_off_dev = _hip.row_compact_map(vox2d, d0)
        return self.real_off_dev

    # -- step 2 (after ONE host read of real_off_dev): the descriptor and the per-voxel offsets
    def finish_map(self, real_off):
        self.real_off = [int(v) for v in real_off]
        self.Rt = self.real_off[-1]
        self.n_real, self.V = self.Rt, self.Vt             # the names of _hip.CompactRows: the wrappers take either
        self.desc = X.FramesDesc.make(self.vox_off, self.real_off, self.T)
        # row_w: MVX_ROWS_VFE layout (Rt + Vt,); fusion_row_w: MVX_ROWS_FUSION layout (Rt + F,)
        self.voff, self.vcnt, self.row_w, self.fusion_row_w = _hip.voxel_row_offsets(self.row_map, self.Vt, self.T, self.Rt, self.desc)
        return self

    @property
    def rows(self):
        return self.Rt + self.Vt

    def hand_over(self, stream, fenced=False):
        """The set was built on another stream (input preparation): keep its tensors alive for ``stream`` too.
        ``fenced`` (modules/pipeline.py): the consumer records an end-of-step event and the preparation stream waits for it before
        it allocates again, so the tensors only have to stay referenced until the step function returns -- no
        ``record_stream``, whose release depends on when the allocator next polls its events (the peak crept 4 % over 1,000
        identical steps and the pools held 2.6 x the live bytes, profiles/r05b_soak_hot.txt)."""
        kept = []
        for t in (self.voxels, self.coords, self.row_map, self.rows_sel, self.n_real_dev, self.real_off_dev, self.voff,
                  self.vcnt, self.row_w, self.fusion_row_w) + (tuple(self.sampled) if self.sampled is not None else ()) + \
                 (tuple(self.grid['tensors']) if self.grid is not None else ()):
            planes = getattr(t, '_mvx_planes', None)                 # the sampled features' planes of bf16 pieces (sample_rows)
            amax = _hip.amax_of(t)
            for u in (t, planes, amax):
                if u is None:
                    continue
                if fenced:
                    kept.append(u)
                else:
                    u.record_stream(stream)
        self._kept = kept                                            # sampled / grid are dropped mid-step: their tensors stay here


BEV_FUSED = True      # conv3's BatchNorm apply writes the (F, C * D, H, W) map itself (tests set False to compare)
# DIAGNOSTIC ONLY (tools/knockout.sh): comma-separated kernel classes that are NOT launched, to measure what each class costs
# on the critical path of a step (step time with the class removed).  Results are garbage; bench.py marks such a run invalid.
# A knocked-out call hands back an uninitialised tensor of the shape the kernel would have written (_knocked).
KNOCKOUT = frozenset(k for k in os.environ.get('MVX_KNOCKOUT', '').split(',') if k)


def _knocked(like=None, shape=None, dtype=torch.float32):
    return torch.empty_like(like) if shape is None else torch.empty(shape, dtype=dtype, device=like.device)


def linear_bn(x, w, b, fs, kind, row_w, eps, tag='fusion', foreign=False, bn=None):
    """rows -> (y = ReLU(x w^T + b), mean_inv (F,2,N)) with per-frame statistics formed inside the launch, in the arithmetic of
    _hip.row_split(tag).  ``foreign``: x was not produced by this library (the sampled image features): _hip.foreign_split.
    ``bn``: the layer's BatchNorm module (bnr.site); an eval forward on running statistics runs the GEMM without its sums --
    the same products -- unless x exists as planes of bf16 pieces only (the GEMM on pre-cut operands has its sums built in)."""
    N = w.shape[0]
    if 'lin_fwd' in KNOCKOUT:
        return _knocked(x, (x.shape[0], N)), _knocked(x, (fs.F, 2, N))
    split = _hip.row_split(tag)
    if bnr.eval_mode() and not (getattr(x, '_mvx_planes', None) is not None and _hip.precut_ok(split, x.shape[0], x.shape[1], N)):
        y, _ = _hip.linear_forward(x, w.reshape(N, -1), b, relu=True, want_stats=False, split=split, foreign=foreign)
        return y, bnr.site(bn, None, kind, x.shape[0])
    y, mi = _hip.linear_forward_bn_frames(x, w.reshape(N, -1), b, fs.desc, kind, row_w, eps, split, foreign)
    return y, bnr.site(bn, mi, kind, x.shape[0])


def bn_apply(y, mi, fs, kind):
    if 'bn_apply_rows' in KNOCKOUT:
        return y
    return _hip.bn_apply(y, mi, desc=fs.desc, kind=kind)


def bn_relu_backward(dyhat, y, mi, fs, kind, row_w, dbias_into, dz=None, planes=False):
    """dz (may alias dyhat); the bias gradient is ADDED to ``dbias_into`` (summed over the frames).  ``planes``: dz is
    written as three planes of bf16 pieces, int16 (3, rows, C), instead of f32 (a layer whose dz only feeds its own weight
    gradient on pre-cut operands: _hip.linear_wgrad_pre)."""
    if planes:
        if 'bn_bwd_rows' in KNOCKOUT:
            return _knocked(y, (3, y.numel() // mi.shape[-1], mi.shape[-1]), torch.int16)
        return _hip.bn_relu_backward_planes(dyhat, y, mi, dbias_into, row_w, fs.desc, kind)
    if ('bn_bwd_rows' if kind != X.ROWS_GRID else 'bn_bwd_grid') in KNOCKOUT:
        return dz if dz is not None else _knocked(y)
    return _hip.bn_relu_backward(dyhat, y, mi, 1.0, dz=dz, row_w=row_w, dbias_out=dbias_into, desc=fs.desc, kind=kind)[0]


def bn_relu_backward_planes_parts(dyhat, y, mi, fs, kind, row_w, dbias_into, nparts):
    """``bn_relu_backward(..., planes=True)`` enqueued range by range: yields ``(planes, row_lo, row_hi)`` per part
    (_hip.bn_relu_backward_planes_parts)."""
    if 'bn_bwd_rows' in KNOCKOUT:
        rows = y.numel() // mi.shape[-1]
        yield _knocked(y, (3, rows, mi.shape[-1]), torch.int16), 0, rows
        return
    yield from _hip.bn_relu_backward_planes_parts(dyhat, y, mi, dbias_into, row_w, fs.desc, kind, nparts)


# (The BatchNorm-backward reduction folded into the epilogue of the producing input-gradient kernel -- VERDICT r03 #1a, built and
# measured in round 4: hot 413.0 vs 418.0 frames/s, full 190.9 vs 190.8, its kernel variants spilling -- was removed in round 5.)


_GRAD_TARGETS = None        # id(parameter) -> buffer the gradient is ADDED into instead of .grad (a second lane of frame sets)


class grad_targets:
    """``with grad_targets(mapping)``: parameter gradients of the enclosed calls are added into ``mapping[id(p)]`` instead of
    ``p.grad`` (modules/pipeline.py: the second lane accumulates into its own flat buffer, so two lanes never write the
    same memory concurrently).  ``None`` = the parameters' own .grad."""

    def __init__(self, mapping):
        self.mapping = mapping

    def __enter__(self):
        global _GRAD_TARGETS
        self.old, _GRAD_TARGETS = _GRAD_TARGETS, self.mapping
        return self

    def __exit__(self, *exc):
        global _GRAD_TARGETS
        _GRAD_TARGETS = self.old
        return False


def _grad_of(p):
    if _GRAD_TARGETS is not None:
        return _GRAD_TARGETS[id(p)]
    if p.grad is None or not p.grad.is_contiguous():
        raise X.MvxHipError('the frame-set path adds gradients into existing contiguous .grad buffers (GradBucket)')
    return p.grad


# ---------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------
class _Saved:
    pass


def middle_forward(model, fs, fpn_levels, imsize, status_sink):
    """Forward of MVXNet.middle for the whole frame set.  ``fpn_levels``: per frame [f0, f1, f2] (1,C,H,W).
    Returns (mid (F,128,H,W), saved state for the backward)."""
    feat, S = rows_forward(model, fs, fpn_levels, imsize, status_sink)
    return cml_forward(model, fs, feat, S, status_sink), S


def sample_rows(head, fs, fpn_levels, imsize):
    """FPN features of the real rows of all frames (imhead/Pipe.py:23-82), each from its own frame's maps:
    ([real rows | one zero row per frame] x (levels * C), status word).  Depends on the inputs only, so the training
    pipeline runs it on the preparation stream for the NEXT step (pipeline.prepare_frame_set(..., sample=...)): 0.21 ms of
    HBM-bound work per 4-frame step that then runs beside MFMA-bound kernels instead of in front of the first GEMM."""
    dev = fs.voxels.device
    F, Rt = fs.F, fs.Rt
    levels = [f[0].permute(1, 2, 0).contiguous() for lv in fpn_levels for f in head.extractor(lv)]
    L = len(levels) // F
    C = levels[0].shape[2]
    compact = torch.empty((Rt + F, L * C), dtype=torch.float32, device=dev)
    compact[Rt:].zero_()                                   # the shared padded rows (Pipe.py:80)
    # fp16x3: the image features come from outside this library -- their range (max |value|) is formed by the sampler while it
    # writes them, so that the first fusion layer can scale them (forward: the coarse scale, _hip.foreign_split)
    amax = torch.zeros((1,), dtype=torch.float32, device=dev) if _hip.split_pieces() == 4 else None
    # the first fusion layer and its weight gradient read their input as planes of bf16 pieces
    # (csrc/rowgemm_pre.hip): the sampler writes them beside the f32 rows while the values are in registers
    w0 = head.fusion._layers()[0][0]
    planes = None
    want_planes = _hip.precut_ok(_hip.split_pieces(), Rt + F, L * C, w0.shape[0]) and _hip.split_pieces() == 3
    if want_planes:
        planes = torch.empty((3, Rt + F, L * C), dtype=torch.int16, device=dev)
        planes[:, Rt:].zero_()
    out = compact
    if planes is not None:
        # with the first fusion layer on planes too nobody reads the f32 rows: they are not written (245 MB per
        # 4-frame step); `compact` stays as the rows' handle (shape, planes, range tag).  MVX_POISON_BG=1 (tests) fills it with
        # NaN instead, which any read would carry into the results
        K0, N0 = L * C, w0.shape[0]
        planes_only = bool(not KNOCKOUT and
                           _hip.precut_ok(_hip.row_split('fusion_%dx%d' % (N0, K0)), Rt + F, K0, N0) and
                           _hip.precut_ok(_hip.row_split('wgrad'), Rt + F, K0, N0))       # both readers take the planes
        if planes_only:
            out = None
            if os.environ.get('MVX_POISON_BG'):
                compact[:Rt].fill_(float('nan'))
    if 'sample' in KNOCKOUT:
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
    else:
        status = _hip.feature_sample_rows(fs.vox2d, fs.rows_sel, Rt, levels, imsize, cfg.eps, out, fs.desc, amax, planes)
    _hip.tag_amax(compact, amax)
    if planes is not None:
        compact._mvx_planes = planes
    return compact, status


def rows_forward(model, fs, fpn_levels, imsize, status_sink, imfeat=None):
    """The row part of the chain: fusion sampling + fusion MLP -> concat -> SVFE -> FCN + max: voxel features
    (Vt,128) of all frames.  ``imfeat`` (Rt+F, 16), if given, stands for the fusion branch's output (VFE-only runs)."""
    head, bb = model.head, model.backbone
    dev = fs.voxels.device
    F, T, Rt, Vt = fs.F, fs.T, fs.Rt, fs.Vt
    _hip.require_no_bnaffine()
    S = _Saved()
    S.fs = fs
    eps = cfg.eps
    S.fusion = []
    if imfeat is not None:
        x = imfeat
        return _vfe_forward(bb, fs, x, S, eps)
    # ---- fusion sampling (imhead/Pipe.py:23-82): real rows of all frames, each from its own frame's maps -- done with the
    # input preparation when the frame set was prepared a step ahead (sample_rows: no parameter is involved)
    if fs.sampled is not None:
        compact, status = fs.sampled
        fs.sampled = None
    else:
        compact, status = sample_rows(head, fs, fpn_levels, imsize)
    status_sink.append(status)
    if _hip.split_pieces() == 4:
        status_sink.append(_hip.fp16_weight_status(dev))    # fp16x3: the weight-range guard's word (modules/_hip.py guard_fp16_weight)
    # ---- fusion MLP (imhead/Pipe.py:84-104) on [real rows | one shared padded row per frame]
    x = compact
    for i, ((w, b), bn) in enumerate(zip(head.fusion._layers(), head.fusion._bns())):
        y, mi = linear_bn(x, w, b, fs, X.ROWS_FUSION, fs.fusion_row_w, eps, 'fusion_%dx%d' % (w.shape[0], w[0].numel()),
                          foreign=(i == 0), bn=bn)
        S.fusion.append((x, w, b, y, mi))
        x = bn_apply(y, mi, fs, X.ROWS_FUSION)
    return _vfe_forward(bb, fs, x, S, eps)


def _vfe_forward(bb, fs, x, S, eps):
    dev = fs.voxels.device
    F, T, Rt, Vt = fs.F, fs.T, fs.Rt, fs.Vt
    # ---- concat with the 7 geometric channels (MVXNet.py:26): [real rows | one padded row per voxel]
    Fc = x.shape[1]
    # rows of 7 + Fc = 23 floats are written with a pitch of 24 (one zero column): the first VFE layer and its weight gradient then
    # read them with 16-byte loads (k = 24 against a weight padded with a zero column: the same sums) instead of falling to the
    # scalar-load forms of their kernels (config 2: 106 / 170 us for 11 / 50 MB)
    ldr = (7 + Fc + 3) & ~3
    rows23 = _hip.vfe_compact_input(fs.vox2d, x, fs, pitch=ldr)
    S.fc = Fc
    # ---- SVFE (voxelnet/Pipe.py:5-29) and FCN + max (VoxelNet.py:27-33)
    S.vfe = []
    x = rows23
    for vfe in (bb.svfe.vfe1, bb.svfe.vfe2):
        w, b = vfe.fcn.fc.weight, vfe.fcn.fc.bias
        y, mi = linear_bn(x, _hip.padded_weight(w.reshape(w.shape[0], -1), x.shape[1]), b, fs, X.ROWS_VFE, fs.row_w, eps, 'vfe',
                          bn=vfe.fcn.bn)
        out, am = _hip.vfe_bn_max_concat(y, mi, Vt, T, fs)
        S.vfe.append((x, w, b, y, mi, am))
        x = out
    w, b = bb.fcn.fc.weight, bb.fcn.fc.bias
    y, mi = linear_bn(x, w, b, fs, X.ROWS_VFE, fs.row_w, eps, 'vfe', bn=bb.fcn.bn)
    feat, am = _hip.bn_segment_max(y, mi, Vt, T, fs)
    S.head = (x, w, b, y, mi, am)
    return feat, S


def grid_activity(model, fs):
    """Everything of the CML forward that depends on the voxel COORDINATES only (no parameter, no activation): the voxel index
    grid of the sparse first layer and the site-level activity of the three layers' outputs -- masks, halo / tile flags, the
    tile set of layer 2's restricted backward (csrc/activity.hip; VoxelNet.py:16-22, voxelnet/Pipe.py:36-42).  ~0.2 ms of small
    dependent launches in front of the first convolution: the training pipeline runs it with the input preparation of the NEXT
    step on the preparation stream (pipeline.prepare_frame_set(..., grid=model)), like the FPN sampling."""
    bb = model.backbone
    dev = fs.voxels.device
    F, Vt = fs.F, fs.Vt
    D0, H, W = cfg.voxelshape[2], cfg.voxelshape[0], cfg.voxelshape[1]
    idx_grid, st2 = _hip.index_grid(fs.coords, (D0, H, W), fs.desc)
    tensors = [idx_grid, st2]
    layers = []
    src, is_index, din = idx_grid, True, D0
    for li, m in enumerate((bb.cml.conv1, bb.cml.conv2, bb.cml.conv3)):
        lay = _hip.activity_dilate(src, is_index, din, H, W, m._sd, m._pd, li > 0, want_tile_flags=True, F=F)      # (mask, hflag, tflag)
        layers.append(lay)
        tensors += lay
        src, is_index, din = lay[0], False, _hip.conv_out_depth(din, m._sd, m._pd)
    # the tiles layer 2's own restricted backward touches (from layer 1's and layer 2's tile flags)
    c2 = bb.cml.conv2
    d1 = _hip.conv_out_depth(D0, bb.cml.conv1._sd, bb.cml.conv1._pd)
    bflag2 = _hip.tile_dilate_flags(layers[0][2], layers[1][2], d1, H, W, c2._sd, c2._pd, F=F)
    tensors.append(bflag2)
    # which tiles of conv1's / conv2's normalised OUTPUT the next layer reads (its forward gather and weight gradient: the 3 x 3
    # tile neighbourhoods of the output tiles it computes): bn_apply_bg leaves the other background tiles unwritten
    reads = []
    din = d1
    for li, m in enumerate((bb.cml.conv2, bb.cml.conv3)):
        reads.append(_hip.tile_read_flags(layers[li][1], din, H, W, m._sd, m._pd, F=F))
        din = _hip.conv_out_depth(din, m._sd, m._pd)
    tensors += reads
    return dict(idx_grid=idx_grid, status=st2, layers=layers, bflag2=bflag2, reads=reads, tensors=tensors)


def cml_forward(model, fs, feat, S, status_sink, want_bev=True):
    """reindex + CML + the BEV reshape (VoxelNet.py:16-36) for the whole frame set: (Vt,128) -> (F,128,H,W).
    The channels-last CML output [F*D3][H][W][64] stays in ``S.x3`` (what modules/rpn_frames.py reads); with
    ``want_bev=False`` the (F,128,H,W) map is not materialised and None is returned."""
    bb = model.backbone
    dev = fs.voxels.device
    F, T, Rt, Vt = fs.F, fs.T, fs.Rt, fs.Vt
    eps = cfg.eps
    _hip.require_no_bnaffine()
    bn_eval = bnr.eval_mode()         # running statistics: the layers run without their sums where an entry point has that form
    # ---- reindex + conv1 through the voxel-GEMM factorisation (VoxelNet.py:16-22, voxelnet/Pipe.py:36)
    D0, H, W = cfg.voxelshape[2], cfg.voxelshape[0], cfg.voxelshape[1]
    c1, c2, c3 = bb.cml.conv1, bb.cml.conv2, bb.cml.conv3
    w1, b1 = c1.conv.weight, c1.conv.bias
    cout, cin = w1.shape[0], w1.shape[1]
    w_all = w1.permute(2, 3, 4, 0, 1).reshape(27 * cout, cin).contiguous()
    P, _ = _hip.linear_forward(feat, w_all, None, relu=False, want_stats=False, split=_hip.row_split('conv1'))
    ga = fs.grid if fs.grid is not None else grid_activity(model, fs)      # made with the input preparation when the set was prepared a step ahead
    fs.grid = None
    idx_grid = ga['idx_grid']
    status_sink.append(ga['status'])
    D1 = _hip.conv_out_depth(D0, c1._sd, c1._pd)
    # voxel-free tiles of y1 are never read (bn_apply_bg / the tile-restricted BatchNorm backward walk the flagged tiles only):
    # they are not written either (MVX_FLAG_NO_BG_FILL: 742 -> ~300 MB of stores per 4-frame step).  MVX_POISON_BG=1 (tests)
    # fills them with NaN instead, which any read would carry into the results
    y1 = torch.full((F * D1, H, W, cout), float('nan'), dtype=torch.float32, device=dev) if os.environ.get('MVX_POISON_BG') else None
    if 'sparse_out' in KNOCKOUT:
        y1, stats = _knocked(feat, (F * D1, H, W, cout)), torch.zeros((F, R, 2, cout), dtype=torch.float64, device=dev)
    else:
        # only the tiles of y1 that hold a site next to a voxel are built: the flags of this layer's output from grid_activity
        y1, stats = _hip.sparse_conv_output_tiles(P, idx_grid, (D0, H, W), b1, cout, c1._sd, c1._pd, ga['layers'][0][2], F, out=y1)
    # (the sums are built into the sparse output kernel: an eval forward leaves them unused and skips their finaliser)
    mi1 = bnr.site(c1.bn, None if bn_eval else _hip.bn_finalize(stats, D1 * H * W, eps, F), X.ROWS_GRID, F * D1 * H * W)

    def dilate(li):
        return ga['layers'][li]

    def background(bg_pre, bias, mi, planes, C_):
        return _hip.bn_background(bg_pre, bias, mi, planes, C_, want_y=True, F=F)

    def bn_apply_bg(y, mi, c_bg, tflag, read=None):
        """BatchNorm apply of a layer output with a background (_hip.bn_apply_tiles).  ``read``: tile flags of what the consuming
        layer reads (grid_activity): the background tiles outside that set are not written (MVX_POISON_BG=1, tests: they hold NaN)."""
        if 'bn_apply_cml' in KNOCKOUT:
            return y
        out = torch.full_like(y, float('nan')) if (read is not None and os.environ.get('MVX_POISON_BG')) else None
        return _hip.bn_apply_tiles(y, mi, c_bg, tflag, F, read, out)

    mask1, hflag1, tflag1 = dilate(0)
    cc1, ybg1 = background(None, b1, mi1, D1, cout)
    x1 = bn_apply_bg(y1, mi1, cc1, tflag1, ga['reads'][0])
    S.conv1 = dict(feat=feat, w=w1, b=b1, w_all=w_all, y=y1, mi=mi1, c=cc1, ybg=ybg1, tflag=tflag1, D0=D0, D1=D1)

    # ---- conv2, conv3 on the MFMA gather kernel with the background rewrite (voxelnet/Pipe.py:37-42)
    split = conv_split_math()                # convmath: bf16x3 -> the split-MFMA forms of the three conv2 / conv3 kernels
    if not conv_background_on():
        raise X.MvxHipError('the frame-set path needs convbackground (the default configuration)')
    S.split = split
    S.convs = []
    x_in, din, c_in, mask_in, hflag_in, tflag_in = x1, D1, cc1, mask1, hflag1, tflag1
    bflag_in = tflag1                                     # tiles on which the gradient of x_in is produced / consumed
    for li, m in enumerate((c2, c3)):
        w, b = m.conv.weight, m.conv.bias
        co, ci = w.shape[0], w.shape[1]
        sd, pd = m._sd, m._pd
        dout = _hip.conv_out_depth(din, sd, pd)
        wpk = m._packer(False, split)
        # background constants of this layer: [planes][co] totals, followed by the per-depth-tap ones the exact-f32 gather
        # uses to skip the depth taps whose source halo holds no active site (FLAG_BG_TAPS)
        bg_pre = _hip.conv3d_background_taps(w, c_in, din, sd, pd, F)[:F * dout]      # totals | 3 depth taps | 9 border classes
        mask_o, hflag_o, tflag_o = dilate(li + 1)
        if 'gather_fwd' in KNOCKOUT and not split:
            y, mi = _knocked(x_in, (F * dout, H, W, co)), _knocked(x_in, (F, 2, co))
        else:
            y, mi = _hip.conv3d_forward_bg(x_in, wpk, b, co, sd, pd, _hip.Background(c_in, mask_in, hflag_in), mask_o, bg_pre,
                                           want_stats=not bn_eval, finalize_eps=eps, split=split, F=F, bg_taps=True)
        mi = bnr.site(m.bn, None if bn_eval else mi, X.ROWS_GRID, F * dout * H * W)
        c_o, ybg_o = background(bg_pre, b, mi, dout, co)         # the background of this layer's output
        if want_bev and li == 1 and co <= 64 and 'bn_apply_cml' not in KNOCKOUT and BEV_FUSED:
            # the last layer's normalised output goes straight into the reference's (F, C * D, H, W) layout
            # (mvx_bn_apply_tiles_bev_frames): no channels-last copy of it, no transposition pass
            mid = _hip.bn_apply_tiles_bev(y, mi, c_o, tflag_o, F)
            x_out = None
        else:
            # conv2's output is read by conv3 only; conv3's (channels-last form: --mode full) by the RPN, everywhere
            x_out = bn_apply_bg(y, mi, c_o, tflag_o, ga['reads'][1] if li == 0 else None)
        rec = dict(x=x_in, w=w, b=b, y=y, mi=mi, din=din, dout=dout, sd=sd, pd=pd, m=m, c_in=c_in, hflag_in=hflag_in,
                   bflag_in=bflag_in, split=split)
        if li == 0:
            # the tiles this layer's own restricted backward touches
            bflag_o = ga['bflag2']
            rec.update(c_out=c_o, ybg_out=ybg_o, bflag_out=bflag_o)
            c_in, bflag_in = c_o, bflag_o
        S.convs.append(rec)
        x_in, din, mask_in, hflag_in, tflag_in = x_out, dout, mask_o, hflag_o, tflag_o
    D3 = din
    S.D3, S.H, S.W, S.C3 = D3, H, W, co
    S.x3 = x_in                                # None when the last layer wrote the (F, C * D, H, W) map itself
    if not want_bev:
        return None
    if x_in is None:
        return mid
    return _hip.cl_to_bev(x_in, F)


def _wgrad_bg_flops(rec, F):
    """EXECUTED FLOPs of a background-aware weight-gradient launch as a zero-argument callable (timing runs only; evaluated
    after the timed region): the kernel runs the (plane, tile) steps whose source halo holds a non-background site, every
    step = 8 x 16 sites x Cin x Cout x 9 taps.  Only the flag tensor is captured, not the activations."""
    din, dout, sd, pd = rec['din'], rec['dout'], rec['sd'], rec['pd']
    hflag = rec['hflag_in']
    co, ci = rec['w'].shape[0], rec['w'].shape[1]

    def count():
        hf = hflag.view(F, din, -1).ne(0)
        steps = 0
        for kd in range(3):
            for d in range(dout):
                ds = d * sd - pd + kd
                if 0 <= ds < din:
                    steps = steps + hf[:, ds].sum()
        return float(steps) * (2.0 * 128 * ci * co * 9)
    return count


def _wgrad_bg(rec, dz, tap_sums, F, H, W):
    if 'wgrad_bg' in KNOCKOUT:
        return
    fl = _wgrad_bg_flops(rec, F) if _hip.KERNEL_TIMERS is not None else 0      # a callable, evaluated after the timed region
    # on the side stream (_hip.ASYNC_WGRAD); split arithmetic: conv3d_wgrad4s (csrc/conv3d.hip) behind the same entry point
    _hip.conv3d_wgrad_bg(rec['x'], dz, rec['sd'], rec['pd'], _hip.Background(rec['c_in'], None, rec['hflag_in']), tap_sums,
                         accumulate_into=_grad_of(rec['w']), split=rec.get('split'), F=F, flops=fl)


def _linear_wgrad_side(x, dz, w):
    """dW += dz^T x over the rows of ALL frames, on the side stream."""
    if 'lin_wgrad' in KNOCKOUT:
        return
    _hip.linear_wgrad(x, dz, accumulate_into=_grad_of(w).view(w.shape[0], -1))


def middle_backward(model, S, grad_mid):
    """Backward of the chain for the whole frame set.  ``grad_mid`` (F or 1, 128, H, W) = dL/d(mid); parameter gradients
    are ADDED into the existing .grad buffers (summed over the frames)."""
    old_async, _hip.ASYNC_WGRAD = _hip.ASYNC_WGRAD, True
    try:
        rows_backward(model, S, cml_backward(model, S, grad_mid))
    finally:
        _hip.ASYNC_WGRAD = old_async


_MUTATE = {}        # TESTS ONLY (tests/test_fullsize_gpu.py): name -> factor applied to a closed-form term of the restricted
                    # backward, to prove that the parity tests would notice a 1 % error in it.  Empty in every product run.


def _mut(name, t):
    return _hip.mutate(_MUTATE, name, t) if _MUTATE else t


def cml_backward(model, S, grad_mid, g_cl=None):
    """Backward of cml_forward: returns dL/d(voxel features) (Vt,128).  ``g_cl``: the gradient already in the
    channels-last layout of ``S.x3`` ([F*D3][H][W][64], from modules/rpn_frames.py) instead of ``grad_mid`` (F or 1,128,H,W)."""
    fs = S.fs
    F, T, Rt, Vt = fs.F, fs.T, fs.Rt, fs.Vt
    H, W, D3, C3 = S.H, S.W, S.D3, S.C3
    dev = fs.voxels.device
    gm = grad_mid.contiguous() if g_cl is None else None
    if g_cl is not None:
        g = g_cl
    elif gm.shape[0] == 1 and F > 1:
        # one gradient map for every frame: transposed once, written F times (instead of a transposition and a repeat of it)
        g = _hip.bev_to_cl_broadcast(gm, D3, F)
    else:
        g = _hip.bev_to_cl(gm, D3)

    def tap_sums(dz, tile_flags=None, inactive=None):
        if 'tap_sums' in KNOCKOUT:
            return _knocked(dz, (dz.shape[0], 9, dz.shape[3]))
        return _hip.plane_tap_sums(dz, tile_flags, inactive)

    def tap_sums_side(name, dz, tile_flags=None, inactive=None):
        """The tap sums of a layer on the SIDE stream, in front of their first reader (the layer's weight gradient); returns
        (T, event): the main stream goes straight from the BatchNorm backward to the input-gradient gather and waits for the
        event only in front of input_grad_sums.  (T, None): computed inline."""
        if not _hip.ASYNC_WGRAD or 'tap_sums' in KNOCKOUT:
            return _mut(name, tap_sums(dz, tile_flags, inactive)), None
        main = torch.cuda.current_stream(dev)
        with _hip._SideStream(dz, tile_flags, inactive):
            Tt = _mut(name, tap_sums(dz, tile_flags, inactive))
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
        Tt.record_stream(main)                  # allocated on the side stream's pool, read by input_grad_sums on the main stream
        return Tt, ev

    def dgrad_tiles(rec, dz, bflag):
        split = rec.get('split') or 0
        wpd = rec['m']._packer(True, split)
        if 'gather_dgrad' in KNOCKOUT and not split:
            return _knocked(dz, (F * rec['din'], H, W, rec['w'].shape[1]))
        return _hip.conv3d_dgrad_tiles(dz, wpd, rec['din'], rec['w'].shape[1], rec['sd'], rec['pd'], bflag, split, F)

    def input_grad_sums(rec, Tt):
        return _hip.conv3d_input_grad_sums(rec['w'], Tt, rec['din'], rec['sd'], rec['pd'], F)

    def bn_bwd_tiles(gin, y, mi, c_bg, y_bg, A, bflag, bias, want_inactive):
        if 'bn_bwd_tiles' in KNOCKOUT:
            return _knocked(y), (_knocked(y, (y.shape[0], y.shape[3])) if want_inactive else None)
        bg = _hip.Background(c_bg, None, None, y_bg=y_bg, bflag=bflag)
        out = _hip.bn_relu_backward_tiles(gin, y, mi, bg, A, _grad_of(bias), want_inactive, F)
        return out[0], (out[2] if want_inactive else None)       # (dz, sums of dz over the other tiles)

    # ---- conv3: dense gradient in, restricted gradient + closed-form plane sums out
    r3, r2 = S.convs[1], S.convs[0]
    dz3 = bn_relu_backward(g, r3['y'], r3['mi'], fs, X.ROWS_GRID, None, _grad_of(r3['b']))
    T3, ev3 = tap_sums_side('T3', dz3)
    _wgrad_bg(r3, dz3, T3, F, H, W)
    g2 = dgrad_tiles(r3, dz3, r3['bflag_in'])
    if ev3 is not None:
        torch.cuda.current_stream(dev).wait_event(ev3)
    A2 = _mut('A2', input_grad_sums(r3, T3))
    # ---- conv2
    dz2, inact2 = bn_bwd_tiles(g2, r2['y'], r2['mi'], r2['c_out'], r2['ybg_out'], A2, r2['bflag_out'], r2['b'], True)
    inact2 = _mut('inact2', inact2)
    T2, ev2 = tap_sums_side('T2', dz2, r2['bflag_out'], inact2)
    _wgrad_bg(r2, dz2, T2, F, H, W)
    g1 = dgrad_tiles(r2, dz2, r2['bflag_in'])
    if ev2 is not None:
        torch.cuda.current_stream(dev).wait_event(ev2)
    A1 = _mut('A1', input_grad_sums(r2, T2))
    # ---- conv1 (voxel-GEMM factorisation): gradient only next to the voxels
    c1 = S.conv1
    w1 = c1['w']
    cout, cin = w1.shape[0], w1.shape[1]
    dz1, _ = bn_bwd_tiles(g1, c1['y'], c1['mi'], c1['c'], c1['ybg'], A1, c1['tflag'], c1['b'], False)
    cm = model.backbone.cml.conv1
    G = _hip.sparse_conv_gather_dz(dz1, fs.coords, c1['D0'], cm._sd, cm._pd, fs.desc)      # its rows are rows of dz1: keeps the range tag
    # conv1's weight gradient ((27 * cout, cin) = G^T feat, then reordered into the parameter's layout): off the main stream like
    # the other weight gradients -- the main stream goes on to the input gradient
    with _hip._SideStream(c1['feat'], G):
        dw_all = _hip.linear_wgrad(c1['feat'], G)
    with _hip._SideStream(dw_all):
        _grad_of(w1).add_(dw_all.reshape(3, 3, 3, cout, cin).permute(3, 4, 0, 1, 2))
    # dfeat = G w_all: the weight as a row-major [cin][27 cout] matrix, so that both operands are read along k
    dfeat, _ = _hip.linear_forward(G, c1['w_all'].t().contiguous(), None, relu=False, want_stats=False, label='linear_dgrad',
                                   split=_hip.row_split('dgrad'))
    return dfeat


def _rows_dgrad(dz, w2):
    """dx = dz w (rows x K): the input gradient of a row layer."""
    if 'lin_dgrad' in KNOCKOUT:
        return torch.empty((dz.shape[0], w2.shape[1]), dtype=torch.float32, device=dz.device)
    gx, _ = _hip.linear_forward(dz, _hip.transposed_weight(w2), None, relu=False, want_stats=False, label='linear_dgrad',
                                split=_hip.row_split('dgrad'))
    return gx


def rows_backward(model, S, dfeat):
    """Backward of rows_forward from dL/d(voxel features) (Vt,128); needs _hip.ASYNC_WGRAD set by the caller."""
    fs = S.fs
    F, T, Rt, Vt = fs.F, fs.T, fs.Rt, fs.Vt
    dev = dfeat.device
    # ---- FCN + max
    x, w, b, y, mi, am = S.head
    Cn = w.shape[0]
    dyh = _hip.segment_max_backward(dfeat, am, Vt, T, fs)
    dz = bn_relu_backward(dyh, y, mi, fs, X.ROWS_VFE, fs.row_w, _grad_of(b), dz=dyh)
    _linear_wgrad_side(x, dz, w)
    gx = _rows_dgrad(dz, w)
    # ---- VFE 2, VFE 1
    for x, w, b, y, mi, am in reversed(S.vfe):
        Cn = w.shape[0]
        dyh = _hip.vfe_max_concat_backward(gx, am, Vt, T, fs)
        dz = bn_relu_backward(dyh, y, mi, fs, X.ROWS_VFE, fs.row_w, _grad_of(b), dz=dyh)
        w2 = w.reshape(w.shape[0], -1)
        if x.shape[1] != w2.shape[1] and 'lin_wgrad' not in KNOCKOUT:
            # rows with a padded pitch (23 -> 24): the gradient of the padded weight, its real columns added into the parameter's
            with _hip._SideStream(x, dz):
                dwp = _hip.linear_wgrad(x, dz)
                _grad_of(w).view(w2.shape).add_(dwp[:, :w2.shape[1]])
        else:
            _linear_wgrad_side(x, dz, w)
        gx = _rows_dgrad(dz, w)
    # ---- concat backward: gradient of the fused image features ([real rows | shared padded row per frame])
    Fc = S.fc
    gim = _hip.vfe_compact_input_backward(gx, Fc, fs)
    # ---- fusion MLP, last layer first; the sampled features carry no gradient
    gx = gim
    for i in range(len(S.fusion) - 1, -1, -1):
        x, w, b, y, mi = S.fusion[i]
        xp = getattr(x, '_mvx_planes', None)
        if i == 0 and xp is not None and _hip.precut_ok(_hip.row_split('wgrad'), x.shape[0], x.shape[1], w.shape[0]):
            # the step's last and largest weight gradient on pre-cut operands: the BatchNorm backward writes dz as planes (no other
            # reader: the sampled features carry no gradient), the weight gradient moves both operands by DMA (rowgemm_pre.hip)
            # in ONE row range: more ranges, each weight gradient on the side stream beside the apply pass of the next range, measured
            # slower (463.7 / 463.1 frames/s in one part, 460.7 / 460.9 in two, 455.4 / 455.3 in four; bf16x6, 40 steps): the
            # HBM-bound apply pass and the MFMA-bound product slow each other down by more than the overlap hides
            for dzp, lo, hi in bn_relu_backward_planes_parts(gx, y, mi, fs, X.ROWS_FUSION, fs.fusion_row_w, _grad_of(b), 1):
                _hip.mark_tail(dev)
                if 'lin_wgrad' not in KNOCKOUT:
                    _hip.linear_wgrad_pre(xp, dzp, accumulate_into=_grad_of(w).view(w.shape[0], -1), rows=(lo, hi))
            break
        dz = bn_relu_backward(gx, y, mi, fs, X.ROWS_FUSION, fs.fusion_row_w, _grad_of(b))
        if i == 0:
            _hip.mark_tail(dev)          # the step's last weight gradient follows: everything else of the bucket may go out (parallel.py)
        _linear_wgrad_side(x, dz, w)
        if i > 0:
            gx = _rows_dgrad(dz, w.reshape(w.shape[0], -1))          # dL/dyhat of layer i - 1
