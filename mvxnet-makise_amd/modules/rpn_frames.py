"""Region proposal network on frame sets: RPN.forward and its backward (modules/voxelnet/Pipe.py:45-75) for all frames
of a step, on the HIP kernels -- no MIOpen, no autograd.

    blk1 = CRB2d(128,128,3,2,1) + 3 x CRB2d(128,128,3,1,1)        -> x1 (H/2 x W/2)
    blk2 = CRB2d(128,128,3,2,1) + 5 x CRB2d(128,128,3,1,1)        -> x2 (H/4 x W/4)
    blk3 = CRB2d(128,256,3,2,1) + 5 x CRB2d(256,256,3,1,1)        -> x3 (H/8 x W/8)
    up   = cat(DeCRB2d(128,256,3,1,1)(x1), DeCRB2d(128,256,2,2,0)(x2), DeCRB2d(256,256,4,4,0)(x3))
    score, reg = sigmoid(Conv2d(768,2,1)(up)), Conv2d(768,14,1)(up)

every CRB2d / DeCRB2d = conv -> ReLU -> BatchNorm with per-frame batch statistics (Blocks.py:31-51).  How each piece runs:
  * 3x3 stride-1 blocks (and deconv1, a stride-1 transposed convolution = a convolution with the flipped, transposed
    kernel): the MFMA gather / wgrad kernels of csrc/conv3d.hip, one plane per frame (mvx_conv2d_*_frames);
  * the three stride-2 blocks: the same kernels with a 2x2 tap window on the space-to-depth image of the input (the weight
    is rearranged, include/mvx_hip.h); the first one reads the CML output planes directly, so the (1,128,H,W) reshape of
    VoxelNet.py:36 is never materialised on this path;
  * deconv2 / deconv3 (kernel = stride): row GEMMs (csrc/linear.hip) whose output is normalised and pixel-shuffled into
    its channel slice of the 768-channel concat buffer by one pass (csrc/rpn.hip);
  * the two heads: one row GEMM with 16 output columns; with the optional direction head (``RPN(direction=True)``) the same
    GEMM with 20: [cls 2 | reg 14 | dir 2 | two zero columns], so that rows stay multiples of 16 bytes and the 768-channel
    concat buffer is read once; the IoU head (``RPN(direction=True, iou=True)``) puts its two logits where the zero columns
    stand: [cls 2 | reg 14 | dir 2 | iou 2].
Maps are channels-last [F][h][w][c].  Parameter gradients are ADDED into the existing .grad buffers, weight-gradient
kernels run on the side stream.
"""
import torch

import modules.config as cfg
from modules import _hip
from modules import bn_running as bnr
from modules import Extension as X

TAPS2 = _hip.FLAG_TAPS2


def _split():
    """convmath: bf16x3 / bf16x6 -> the 3x3 convolutions run on the split-MFMA kernels (csrc/conv3d_split.hip): the number of
    bf16 pieces per operand (0 = exact-f32 kernels)."""
    return _hip.split_pieces()


_GRAD_TARGETS = None        # id(parameter) -> tensor the gradient is ADDED into instead of .grad (the autograd wrapper)


class grad_targets:
    """``with grad_targets({id(p): buffer})``: rpn_backward adds every parameter gradient into the given buffers instead of
    the parameters' .grad (modules/voxelnet/Pipe.py RPNFunction hands them to the autograd engine)."""

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


_S2D_INDEX = {}


def _s2d_index(cout, cin, planes, dev):
    """Gather index / mask that rearrange a stride-2 kernel W (cout, cin, 3, 3) into the 2x2-window kernel over the
    space-to-depth channels: W2[co][(p, d, c)][ta][tb] = W[co][c*planes + d][a][b] with a -> (ta, pr): 0 -> (0,1), 1 -> (1,0),
    2 -> (1,1) (b likewise), zeros elsewhere.  cin = planes * C: with planes > 1 the reference channel index is c*planes + d
    (VoxelNet.py:36), the space-to-depth image holds the planes side by side (d-major)."""
    key = (cout, cin, planes, str(dev))
    hit = _S2D_INDEX.get(key)
    if hit is None:
        C = cin // planes
        amap = {0: (0, 1), 1: (1, 0), 2: (1, 1)}
        idx = torch.zeros((4 * cin, 3, 3), dtype=torch.int64)
        mask = torch.zeros((4 * cin, 3, 3), dtype=torch.float32)
        ch = torch.arange(cin)
        d, c = ch // C, ch % C                       # s2d channel (within a parity block) = d*C + c
        ref = c * planes + d                         # the reference's channel
        for a in range(3):
            for b in range(3):
                (ta, pr), (tb, pc) = amap[a], amap[b]
                p = pr * 2 + pc
                idx[p * cin + ch, ta, tb] = ref * 9 + a * 3 + b
                mask[p * cin + ch, ta, tb] = 1.0
        hit = (idx.reshape(-1).to(dev), mask.reshape(-1).to(dev), mask.reshape(-1).bool().nonzero().reshape(-1).to(dev))
        _S2D_INDEX[key] = hit
    return hit


def _s2d_weight(w, planes):
    cout, cin = w.shape[0], w.shape[1]
    idx, mask, _ = _s2d_index(cout, cin, planes, w.device)
    return (w.reshape(cout, cin * 9)[:, idx] * mask).view(cout, 4 * cin, 3, 3)


def _s2d_weight_grad(dw2, w, planes):
    """ADD the gradient of the rearranged kernel back into the layout of ``w``'s gradient."""
    cout, cin = w.shape[0], w.shape[1]
    idx, _, valid = _s2d_index(cout, cin, planes, w.device)
    _grad_of(w).view(cout, cin * 9).index_add_(1, idx[valid], dw2.reshape(cout, -1)[:, valid])


class _Packs:
    """Kernel-layout copies of the (possibly rearranged) convolution weights of one RPN, refreshed when a parameter changes."""

    def __init__(self):
        self.cache = {}

    def get(self, key, w, make, for_dgrad):
        split = _split()
        tag = (w._version, w.data_ptr())
        hit = self.cache.get((key, for_dgrad, split))
        if hit is None or hit[0] != tag:
            w2 = make().detach()
            if split:                      # bf16x3: the 2-D kernel as the middle depth slice of a 3-D one, hi/lo split pack
                w3 = torch.zeros(w2.shape[:2] + (3, 3, 3), dtype=torch.float32, device=w2.device)
                w3[:, :, 1] = w2
                hit = (tag, _hip.conv3d_pack(w3, for_dgrad, split=split))
            else:
                hit = (tag, _hip.conv3d_pack(w2, for_dgrad))
            self.cache[(key, for_dgrad, split)] = hit
        return hit[1]


def _packs_of(rpn):
    pk = rpn.__dict__.get('_mvx_packs')
    if pk is None:
        pk = _Packs()
        object.__setattr__(rpn, '_mvx_packs', pk)
    return pk


def _desc(F):
    return X.FramesDesc.make([0] * (F + 1), [0] * (F + 1), 1)


# The convolution wrappers of _hip in this RPN's arithmetic (_split) and with its gradient targets (_grad_of).
def _conv(x, wpk, bias, F, h, w, cin, cout, flags, eps, bn=None):
    """y = ReLU(conv(x) + b) with per-frame statistics finalised in the launch -> (y, mean_inv (F,2,cout)); ``bn``: the layer's
    BatchNorm module as a site of the step (bnr.site: with running statistics in eval mode the kernel's own sums stay
    unused); None: a stand-alone block (modules/layers/Block2d.py), batch statistics."""
    if bn is None:
        return _hip.conv2d_forward(x, wpk, bias, F, h, w, cin, cout, flags, eps, _split())
    ev = bnr.eval_mode()
    y, mi = _hip.conv2d_forward(x, wpk, bias, F, h, w, cin, cout, flags, eps, _split(), want_mi=not ev)
    return y, bnr.site(bn, None if ev else mi, X.ROWS_GRID, F * h * w)


def _bn_apply(y, mi, F):
    return _hip.bn_apply(y, mi, desc=_desc(F), kind=X.ROWS_GRID, timed=False)


def _bn_bwd(g, y, mi, F, bias):
    return _hip.bn_relu_backward(g, y, mi, 1.0, dbias_out=_grad_of(bias), desc=_desc(F), kind=X.ROWS_GRID, timed=False)[0]


def _retag(t, like):
    """A view of a tagged gradient keeps the tag."""
    return _hip.tag_amax(t, _hip.amax_of(like))


def _dgrad(dz, wpd, F, h, w, cin, cout, flags):
    return _hip.conv2d_dgrad(dz, wpd, F, h, w, cin, cout, flags, _split())


def _wgrad(x, dz, F, h, w, cin, cout, flags, into=None):
    """dW (cout, cin, 3, 3) over all frames, on the side stream; ADDED into ``into`` or returned."""
    return _hip.conv2d_wgrad(x, dz, F, h, w, cin, cout, flags, into, _split())


def _s2d(x, F, planes, h, w, C):
    return _hip.space_to_depth(x, F, planes, h, w, C)


def _d2s(xs, F, planes, h, w, C):
    return _hip.space_to_depth(xs, F, planes, h, w, C, reverse=True)


def rpn_forward(rpn, x_cl, F, planes, H, W, Cp):
    """x_cl: the normalised CML output, channels-last planes [F*planes][H][W][Cp] (BEV channel c*planes + d).
    Returns (heads (F*H/2*W/2, 16) = [cls logits (2) | reg (14)] per BEV cell, saved state); with a direction head the rows
    are 20 wide, [cls (2) | reg (14) | dir logits (2) | 0 0] (``head_layout``), and with the IoU head on top of it
    [cls (2) | reg (14) | dir logits (2) | iou logits (2)]: the width does not tell the two apart, the model does."""
    dev = x_cl.device
    eps = cfg.eps
    _hip.require_no_bnaffine()
    bn_eval = bnr.eval_mode()
    pk = _packs_of(rpn)
    S = {'F': F, 'geom': (planes, H, W, Cp), 'blocks': []}
    x, h, w, C, pl = x_cl, H, W, Cp, planes
    for bi, blk in enumerate((rpn.blk1, rpn.blk2, rpn.blk3)):
        layers = []
        for li, m in enumerate(blk):
            wt, b = m.conv.weight, m.conv.bias
            cout = wt.shape[0]
            if li == 0:                                   # stride 2: 2x2 window on the space-to-depth image
                xs = _s2d(x, F, pl, h, w, C)
                h, w = h // 2, w // 2
                cin = 4 * pl * C
                wpk = pk.get(('s2', bi), wt, lambda wt=wt, pl=pl: _s2d_weight(wt, pl), False)
                y, mi = _conv(xs, wpk, b, F, h, w, cin, cout, TAPS2, eps, m.bn)
                layers.append(dict(kind='s2', x=xs, y=y, mi=mi, m=m, cin=cin, cout=cout, h=h, w=w, planes=pl, cfull=C, bi=bi))
                pl = 1
            else:
                cin = C
                wpk = pk.get(('s1', bi, li), wt, lambda wt=wt: wt, False)
                y, mi = _conv(x, wpk, b, F, h, w, cin, cout, 0, eps, m.bn)
                layers.append(dict(kind='s1', x=x, y=y, mi=mi, m=m, cin=cin, cout=cout, h=h, w=w, bi=bi, li=li))
            x = _bn_apply(y, mi, F)
            C = cout
        S['blocks'].append(dict(layers=layers, out=x, h=h, w=w, C=C))
    (x1, h1, w1), (x2, h2, w2), (x3, h3, w3) = [(b['out'], b['h'], b['w']) for b in S['blocks']]
    rows = F * h1 * w1
    up = torch.empty((rows, 768), dtype=torch.float32, device=dev)
    # deconv1: stride-1 transposed convolution = convolution with the flipped kernel, channel axes swapped
    d1 = rpn.deconv1
    wc = pk.get(('d1',), d1.deconv.weight, lambda: d1.deconv.weight.flip(2, 3).transpose(0, 1).contiguous(), False)
    y, mi = _conv(x1, wc, d1.deconv.bias, F, h1, w1, 128, 256, 0, eps, d1.bn)
    _hip.bn_apply_strided(y, mi, up, rows, 256, 768, 0, F)
    S['d1'] = dict(x=x1, y=y, mi=mi)
    # deconv2 / deconv3: kernel = stride -> row GEMM + normalising pixel shuffle into the concat slice
    S['dk'] = []
    for xk, hk, wk, m, s, off in ((x2, h2, w2, rpn.deconv2, 2, 256), (x3, h3, w3, rpn.deconv3, 4, 512)):
        wt, b = m.deconv.weight, m.deconv.bias                    # (Cin, Cout, s, s)
        cin, cout = wt.shape[0], wt.shape[1]
        w_all = wt.permute(2, 3, 1, 0).reshape(s * s * cout, cin).contiguous()     # row (i*s+j)*Cout + co
        xr = xk.view(F * hk * wk, cin)
        t, _ = _hip.linear_forward(xr, w_all, b.repeat(s * s), relu=True, want_stats=False, split=_hip.row_split('rpn'))
        # (statistics and finaliser are launches of their own here: an eval forward on running statistics has neither)
        mi = bnr.site(m.bn, None if bn_eval else _hip.bn_finalize(_hip.row_stats_frames(t, cout, F), hk * wk * s * s, eps, F),
                      X.ROWS_GRID, F * hk * wk * s * s)
        _hip.d2s_bn_apply(t, mi, up, F, hk, wk, s, cout, 768, off)
        S['dk'].append(dict(x=xr, t=t, mi=mi, m=m, s=s, off=off, h=hk, w=wk, w_all=w_all, cin=cin, cout=cout))
    # heads (Pipe.py:64-65,74): one GEMM, 16 columns
    dirh = getattr(rpn, 'dir', None)
    if dirh is None:
        w_heads = torch.cat([rpn.cls.weight.view(2, 768), rpn.reg.weight.view(14, 768)]).contiguous()
        b_heads = torch.cat([rpn.cls.bias, rpn.reg.bias])
    elif getattr(rpn, 'iou', None) is None:         # + the direction logits and two zero rows: 20 columns
        w_heads = torch.cat([rpn.cls.weight.view(2, 768), rpn.reg.weight.view(14, 768), dirh.weight.view(2, 768),
                             torch.zeros((2, 768), dtype=torch.float32, device=dev)]).contiguous()
        b_heads = torch.cat([rpn.cls.bias, rpn.reg.bias, dirh.bias, torch.zeros((2,), dtype=torch.float32, device=dev)])
    else:                                           # the IoU logits where the zero rows stand: the same 20 columns
        w_heads = torch.cat([rpn.cls.weight.view(2, 768), rpn.reg.weight.view(14, 768), dirh.weight.view(2, 768),
                             rpn.iou.weight.view(2, 768)]).contiguous()
        b_heads = torch.cat([rpn.cls.bias, rpn.reg.bias, dirh.bias, rpn.iou.bias])
    heads, _ = _hip.linear_forward(up, w_heads, b_heads, relu=False, want_stats=False)
    S.update(up=up, w_heads=w_heads, h1=h1, w1=w1)
    return heads, S


def head_layout(width):
    """Row width of a head output -> (A, has_dir): 8A columns [A cls | 7A reg], or with the direction head 9A rounded up to a
    multiple of 4, [A cls | 7A reg | A dir | zeros] (8, 16, 24, 32 against 12, 20, 28, 36: never ambiguous for A <= 4)."""
    if width % 8 == 0 and 1 <= width // 8 <= 4:
        return width // 8, False
    A = width // 9
    if 1 <= A <= 4 and (9 * A + 3) // 4 * 4 == width:
        return A, True
    raise X.MvxHipError('a head row of %d columns is neither [A cls | 7A reg] nor that plus A direction logits' % width)


def split_heads(heads, F, h1, w1):
    """(score (F,2,h1,w1) = sigmoid(cls), reg (F,14,h1,w1)) as views of the channels-last head output (no copies of reg), of
    either width."""
    A, _ = head_layout(heads.shape[-1])
    v = heads.view(F, h1, w1, heads.shape[-1])
    return torch.sigmoid(v[..., :A]).permute(0, 3, 1, 2), v[..., A:8 * A].permute(0, 3, 1, 2)


_MUTATE = {}        # TESTS ONLY (tests/test_rpn_gpu.py): name -> factor applied to one term of the RPN backward, to prove that the
                    # full-size gradient check would notice a 1 % error in it.  Empty in every product run.


def _mut(name, t):
    return _hip.mutate(_MUTATE, name, t) if _MUTATE else t


def rpn_backward(rpn, S, d_heads):
    """Backward from dL/d(heads) (F*h1*w1, 16 or 20, as rpn_forward returned them); returns dL/d(x_cl) in the layout of rpn_forward's input.
    Needs _hip.ASYNC_WGRAD semantics: weight gradients are produced on the side stream (join before the optimizer)."""
    F = S['F']
    planes, H, W, Cp = S['geom']
    pk = _packs_of(rpn)
    cap = S.get('capture')          # tests: list receiving (layer key, upstream gradient, input gradient) per conv layer
    up, w_heads, h1, w1 = S['up'], S['w_heads'], S['h1'], S['w1']
    dev = up.device
    rows = up.shape[0]
    d_heads = d_heads.contiguous()
    if _split() == 4 and _hip.amax_of(d_heads) is None:
        _hip.tensor_amax(d_heads)        # fp16x3: the loss gradient's range (9 MB: 5 us), else its weight gradient runs in bf16x6
    # heads
    # (the row-GEMM weight gradients of the heads and of deconv2 / deconv3 run on the side stream like the convolutions': they
    # were 0.41 ms of main-queue time per --mode full step)
    with _hip._SideStream(up, d_heads):
        dwh = _hip.linear_wgrad(up, d_heads)                               # (16 or 20, 768)
    with _hip._SideStream(dwh, d_heads):
        _grad_of(rpn.cls.weight).view(2, 768).add_(dwh[:2])
        _grad_of(rpn.reg.weight).view(14, 768).add_(dwh[2:16])
        db = d_heads.sum(0)
        _grad_of(rpn.cls.bias).add_(db[:2])
        _grad_of(rpn.reg.bias).add_(db[2:16])
        if w_heads.shape[0] == 20:                  # the direction head (its two pad columns of d_heads are zero)
            _grad_of(rpn.dir.weight).view(2, 768).add_(dwh[16:18])
            _grad_of(rpn.dir.bias).add_(db[16:18])
            if getattr(rpn, 'iou', None) is not None:      # the IoU head: columns 18..19 are its logits, not padding
                _grad_of(rpn.iou.weight).view(2, 768).add_(dwh[18:20])
                _grad_of(rpn.iou.bias).add_(db[18:20])
    g_up, _ = _hip.linear_forward(d_heads, w_heads, None, relu=False, want_stats=False, w_transposed=True)      # (rows, 768)
    g_up = _mut('heads_dgrad', g_up)
    # deconv2 / deconv3
    g_in = {}
    for rec in S['dk']:
        m, s, off, hk, wk, cin, cout = rec['m'], rec['s'], rec['off'], rec['h'], rec['w'], rec['cin'], rec['cout']
        gt = torch.empty_like(rec['t'])
        _hip.d2s_bn_apply(gt, None, g_up, F, hk, wk, s, cout, 768, off, reverse=True)
        dz0 = _bn_bwd(gt.view(-1, cout), rec['t'].view(-1, cout), rec['mi'], F, m.deconv.bias)
        dz = _retag(dz0.view(rec['t'].shape), dz0)
        with _hip._SideStream(rec['x'], dz):
            dw_all = _hip.linear_wgrad(rec['x'], dz)                       # (s*s*cout, cin)
        with _hip._SideStream(dw_all):
            _grad_of(m.deconv.weight).add_(dw_all.view(s, s, cout, cin).permute(3, 2, 0, 1))
        # input gradient with the weight as a row-major [cin][s*s*cout] matrix (both operands read along k)
        gx, _ = _hip.linear_forward(dz, rec['w_all'].t().contiguous(), None, relu=False, want_stats=False, label='linear_dgrad',
                                    split=_hip.row_split('dgrad'))
        g_in[s] = _mut('deconv%d_dgrad' % s, gx).view(F, hk, wk, cin)
    # deconv1
    d1 = rpn.deconv1
    g1 = torch.empty((rows, 256), dtype=torch.float32, device=dev)
    _hip.bn_apply_strided(g1, None, g_up, rows, 256, 768, 0, F, reverse=True)
    r1 = S['d1']
    dz = _bn_bwd(g1.view(F, h1, w1, 256), r1['y'], r1['mi'], F, d1.deconv.bias)
    dwc = _wgrad(r1['x'], dz, F, h1, w1, 128, 256, 0)                      # gradient of the flipped / transposed kernel
    with _hip._SideStream(dwc):
        _grad_of(d1.deconv.weight).add_(dwc.transpose(0, 1).flip(2, 3))
    wcd = pk.get(('d1',), d1.deconv.weight, lambda: d1.deconv.weight.flip(2, 3).transpose(0, 1).contiguous(), True)
    g_x1 = _mut('deconv1_dgrad', _dgrad(dz, wcd, F, h1, w1, 128, 256, 0))
    # blocks, last first; x2 and x1 collect the gradients of both their consumers
    g_next = {2: g_in[4], 1: g_in[2], 0: g_x1}
    g = g_next[2]
    for bi in (2, 1, 0):
        if bi < 2:
            g = g_next[bi] + g                      # deconv path + the next block's stride-2 layer
        sums = None                                 # BatchNorm-backward sums of the layer about to be processed, when its producer made them
        layers = S['blocks'][bi]['layers']
        for rec in reversed(layers):
            m = rec['m']
            wt = m.conv.weight
            h, w, cin, cout = rec['h'], rec['w'], rec['cin'], rec['cout']
            g_up_layer = g
            dz = _mut('bn_bwd_b%d' % bi, _bn_bwd(g, rec['y'], rec['mi'], F, m.conv.bias))
            if rec['kind'] == 's1':
                _wgrad(rec['x'], dz, F, h, w, cin, cout, 0, into=_grad_of(wt))
                wpd = pk.get(('s1', rec['bi'], rec['li']), wt, lambda wt=wt: wt, True)
                g = _mut('s1_dgrad_b%d' % bi, _dgrad(dz, wpd, F, h, w, cin, cout, 0))
            else:
                pl, Cf = rec['planes'], rec['cfull']
                dw2 = _wgrad(rec['x'], dz, F, h, w, cin, cout, TAPS2)
                with _hip._SideStream(dw2):
                    _s2d_weight_grad(dw2, wt, pl)
                wpd = pk.get(('s2', rec['bi']), wt, lambda wt=wt, pl=pl: _s2d_weight(wt, pl), True)
                gs = _mut('s2_dgrad_b%d' % bi, _dgrad(dz, wpd, F, h, w, cin, cout, TAPS2))             # gradient of the space-to-depth image
                g = _d2s(gs, F, pl, 2 * h, 2 * w, Cf)
                if pl == 1:
                    g = g.view(F, 2 * h, 2 * w, Cf)
            if cap is not None:
                cap.append(((rec['bi'], rec.get('li', 0)), g_up_layer.clone(), g.clone()))
    return g                                       # [F*planes][H][W][Cp]
