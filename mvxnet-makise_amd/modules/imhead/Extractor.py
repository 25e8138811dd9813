"""The frozen image extractor on this library's kernels: torchvision's ``fasterrcnn_resnet50_fpn_v2`` trunk (reference
modules/imhead/Pipe.py:8-21) -- GeneralizedRCNNTransform (eval), ResNet50 v1.5 body, FPN levels '0', '1', '2' -- without
torchvision.  Forward only, channels-last frame sets (F, h, w, C):

  * preparation, stem (7x7 / 2 + max pool), the bottleneck's skip, the stride-2 row gather and the FPN's top-down merge are the
    kernels of csrc/extractor.hip;
  * every 1x1 convolution is a row GEMM (``_hip.linear_forward``), every 3x3 one a launch of the conv2d kernels
    (``_hip.conv2d_forward_plain``; stride 2 = the 2x2 window on the space-to-depth image, as the RPN does it), both in the
    configured ``convmath`` (fp16x3 runs bf16x6 here: the activations of a frozen foreign network carry no range tag);
  * BatchNorm (eval, eps 1e-5) is folded into weight and bias once per load, in float64;
  * what nobody reads is not computed: ``fpn.layer_blocks.3``, the ``pool`` level, the RPN and ROI heads.

Weights come as a state dict with torchvision's key names (``body.conv1.weight`` ... ``fpn.layer_blocks.2.1.bias``), bare or
below ``backbone.`` or ``head.extractor.backbone.`` (a checkpoint written by the reference's train.py)."""
import torch
from torch import nn

from modules import _hip

BN_EPS = 1e-5
PREFIXES = ('head.extractor.backbone.', 'backbone.', '')
LAYERS = ((3, 64), (4, 128), (6, 256), (3, 512))          # ResNet50: blocks, bottleneck width (output = 4 x width)
_BN = ('weight', 'bias', 'running_mean', 'running_var')

prepared_size = _hip.prepared_size


def expected_shapes():
    """torchvision key -> shape of everything the three read levels depend on."""
    s = {}

    def conv_bn(conv, bn, co, ci, k):
        s[conv + '.weight'] = (co, ci, k, k)
        for t in _BN:
            s[bn + '.' + t] = (co,)

    conv_bn('body.conv1', 'body.bn1', 64, 3, 7)
    cin = 64
    for li, (n, width) in enumerate(LAYERS, 1):
        for b in range(n):
            p = 'body.layer%d.%d.' % (li, b)
            conv_bn(p + 'conv1', p + 'bn1', width, cin, 1)
            conv_bn(p + 'conv2', p + 'bn2', width, width, 3)
            conv_bn(p + 'conv3', p + 'bn3', 4 * width, width, 1)
            if b == 0:
                conv_bn(p + 'downsample.0', p + 'downsample.1', 4 * width, cin, 1)
            cin = 4 * width
    for i, (_, width) in enumerate(LAYERS):
        conv_bn('fpn.inner_blocks.%d.0' % i, 'fpn.inner_blocks.%d.1' % i, 256, 4 * width, 1)
    for i in range(3):
        conv_bn('fpn.layer_blocks.%d.0' % i, 'fpn.layer_blocks.%d.1' % i, 256, 256, 3)
    return s


def clean_state_dict(src):
    """A state dict or a path to one -> {torchvision key: CPU tensor} of exactly ``expected_shapes()``.  Keys may carry one of
    PREFIXES; anything else in the file (RPN / ROI heads, ``num_batches_tracked``, the rest of a model checkpoint) is ignored.
    Missing keys and wrong shapes raise ONE ValueError that lists all of them."""
    if not isinstance(src, dict):
        src = torch.load(src, map_location='cpu', weights_only=True)
    want = expected_shapes()
    got = {}
    for prefix in PREFIXES:                       # longest first: a bare key never shadows a prefixed one
        for k, v in src.items():
            if k.startswith(prefix) and k[len(prefix):] in want and k[len(prefix):] not in got:
                got[k[len(prefix):]] = v
    bad = ['missing: %s' % k for k in want if k not in got]
    bad += ['shape of %s: %s, expected %s' % (k, tuple(got[k].shape), want[k]) for k in want
            if k in got and tuple(got[k].shape) != want[k]]
    if bad:
        raise ValueError('extractor weights: %d problem(s)\n  %s' % (len(bad), '\n  '.join(bad)))
    return {k: got[k].detach().to('cpu') for k in want}


def fold_bn(w, gamma, beta, mean, var, eps=BN_EPS):
    """Eval BatchNorm behind a bias-free convolution as (weight, bias) in float64: w * g / sqrt(var + eps) and
    beta - mean * g / sqrt(var + eps)."""
    k = gamma.double() / torch.sqrt(var.double() + eps)
    return w.double() * k.view(-1, 1, 1, 1), beta.double() - mean.double() * k


def _folded(sd, conv, bn):
    w, b = fold_bn(sd[conv + '.weight'], *(sd[bn + '.' + t] for t in _BN))
    return w.float(), b.float()


def buffer_tree(sd):
    """The tensors as buffers of a module tree that has their dotted names (``state_dict()`` gives the keys back)."""
    root = nn.Module()
    for k, v in sd.items():
        parts = k.split('.')
        m = root
        for p in parts[:-1]:
            if p not in m._modules:
                m.add_module(p, nn.Module())
            m = m._modules[p]
        m.register_buffer(parts[-1], v.clone())
    return root


def _conv_split():
    sp = _hip.split_pieces()
    return 3 if sp == 4 else sp


def _row_split():
    sp = _hip.row_split('extractor')
    return 3 if sp == 4 else sp


class _Row:
    """1x1 convolution + folded BatchNorm = a row GEMM on the (F*h*w, cin) view of the map."""

    def __init__(self, w, b, dev):
        self.w = w.reshape(w.shape[0], w.shape[1]).contiguous().to(dev)
        self.b = b.contiguous().to(dev)

    def __call__(self, x, relu):
        F, h, w, c = x.shape
        y, _ = _hip.linear_forward(x.view(F * h * w, c), self.w, self.b, relu=relu, want_stats=False, split=_row_split())
        return y.view(F, h, w, self.w.shape[0])


class _Conv3:
    """3x3 convolution (padding 1, stride 1 or 2) + folded BatchNorm on the conv2d kernels; the kernel-layout pack of the weight
    is made once per arithmetic."""

    def __init__(self, w, b, stride, dev):
        from modules.rpn_frames import _s2d_weight
        self.cout, self.cin, self.stride = w.shape[0], w.shape[1], stride
        w = w.to(dev)
        self.w = (_s2d_weight(w, 1) if stride == 2 else w).contiguous()
        self.b = b.contiguous().to(dev)
        self.packs = {}

    def _pack(self, split):
        pk = self.packs.get(split)
        if pk is None:
            if split:                       # the split pack takes a 3-D kernel: the 2-D one is its middle depth slice
                w3 = torch.zeros(self.w.shape[:2] + (3, 3, 3), dtype=torch.float32, device=self.w.device)
                w3[:, :, 1] = self.w
                pk = _hip.conv3d_pack(w3, False, split=split)
            else:
                pk = _hip.conv3d_pack(self.w, False)
            self.packs[split] = pk
        return pk

    def __call__(self, x, relu):
        F, h, w, c = x.shape
        split = _conv_split()
        if self.stride == 2:
            x = _hip.space_to_depth(x, F, 1, h, w, c)
            return _hip.conv2d_forward_plain(x, self._pack(split), self.b, F, h // 2, w // 2, 4 * c, self.cout, _hip.FLAG_TAPS2, relu,
                                             split)
        return _hip.conv2d_forward_plain(x, self._pack(split), self.b, F, h, w, c, self.cout, 0, relu, split)


class FrozenResNet50FPN:
    """The network on one device, built from a cleaned state dict (folding and packing happen here, once)."""

    def __init__(self, sd, device, min_size=800, max_size=1333):
        self.device = torch.device(device)
        self.min_size, self.max_size = min_size, max_size
        dev = self.device
        w, b = _folded(sd, 'body.conv1', 'body.bn1')
        self.stem_w = w.permute(2, 3, 1, 0).contiguous().to(dev)          # [ky][kx][ci][co]
        self.stem_b = b.contiguous().to(dev)
        self.stages = []
        for li, (n, _) in enumerate(LAYERS, 1):
            blocks = []
            for bi in range(n):
                p = 'body.layer%d.%d.' % (li, bi)
                stride = 2 if (bi == 0 and li > 1) else 1
                blk = {'conv1': _Row(*_folded(sd, p + 'conv1', p + 'bn1'), dev),
                       'conv2': _Conv3(*_folded(sd, p + 'conv2', p + 'bn2'), stride, dev),
                       'conv3': _Row(*_folded(sd, p + 'conv3', p + 'bn3'), dev), 'stride': stride, 'down': None}
                if bi == 0:
                    blk['down'] = _Row(*_folded(sd, p + 'downsample.0', p + 'downsample.1'), dev)
                blocks.append(blk)
            self.stages.append(blocks)
        self.inner = [_Row(*_folded(sd, 'fpn.inner_blocks.%d.0' % i, 'fpn.inner_blocks.%d.1' % i), dev) for i in range(4)]
        self.outer = [_Conv3(*_folded(sd, 'fpn.layer_blocks.%d.0' % i, 'fpn.layer_blocks.%d.1' % i), 1, dev) for i in range(3)]

    # the pieces, as tools/time_extractor.py times them
    def prepare(self, images):
        return _hip.image_prepare(images, self.min_size, self.max_size)[0]

    def stem(self, x4):
        return _hip.maxpool3s2(_hip.stem_conv7(x4, self.stem_w, self.stem_b))

    def stage(self, i, x):
        for blk in self.stages[i]:
            y = blk['conv3'](blk['conv2'](blk['conv1'](x, True), True), False)
            if blk['down'] is not None:
                x = blk['down'](_hip.gather_stride2(x) if blk['stride'] == 2 else x, False)
            x = _hip.add_relu(y, x)
        return x

    def fpn(self, c):
        """c = [C2, C3, C4, C5] -> the levels '0', '1', '2' (layer_blocks.3 and the pool level have no reader)."""
        last = self.inner[3](c[3], False)
        outs = [None, None, None]
        for i in (2, 1, 0):
            last = _hip.topdown_merge(self.inner[i](c[i], False), last)
            outs[i] = self.outer[i](last, False)
        return outs

    def maps(self, images):
        """u8 (F, H, W, 3) or f32 (F, 3, H, W) -> [P2, P3, P4] as (F, h, w, 256) frame sets."""
        x = self.stem(self.prepare(images))
        c = []
        for i in range(4):
            x = self.stage(i, x)
            c.append(x)
        return self.fpn(c)
