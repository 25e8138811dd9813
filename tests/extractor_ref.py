"""Restatement on the CPU, with torch.nn.functional, of what the frozen image extractor computes (torchvision's
``fasterrcnn_resnet50_fpn_v2`` trunk in eval mode: GeneralizedRCNNTransform, ResNet50 v1.5 body, FPN levels '0', '1', '2'), in
float64 or float32, from a state dict with torchvision's key names.  BatchNorm is applied UNFOLDED (``F.batch_norm`` on the
running statistics), so the library's folding is checked against it.  Also the seeded test weights."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
EPS = 1e-5
LAYERS = ((3, 64), (4, 128), (6, 256), (3, 512))


def conv_bn_names():
    """(conv key, bn key, cout, cin, kernel) of every layer, torchvision names, in network order; also the unread ones."""
    out = [('body.conv1', 'body.bn1', 64, 3, 7)]
    cin = 64
    for li, (n, width) in enumerate(LAYERS, 1):
        for b in range(n):
            p = 'body.layer%d.%d.' % (li, b)
            out.append((p + 'conv1', p + 'bn1', width, cin, 1))
            out.append((p + 'conv2', p + 'bn2', width, width, 3))
            out.append((p + 'conv3', p + 'bn3', 4 * width, width, 1))
            if b == 0:
                out.append((p + 'downsample.0', p + 'downsample.1', 4 * width, cin, 1))
            cin = 4 * width
    for i, (_, width) in enumerate(LAYERS):
        out.append(('fpn.inner_blocks.%d.0' % i, 'fpn.inner_blocks.%d.1' % i, 256, 4 * width, 1))
    for i in range(4):
        out.append(('fpn.layer_blocks.%d.0' % i, 'fpn.layer_blocks.%d.1' % i, 256, 256, 3))
    return out


@functools.lru_cache(maxsize=None)
def seeded_state_dict(seed=7):
    """float64 weights: He-scaled convolutions, BatchNorm with gamma ~ 1 (0.25 on the last BatchNorm of a bottleneck, so the
    skip sums do not grow over 16 blocks), beta and mean within 0.1, variance in [0.5, 1.5]: activations stay O(1)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for conv, bn, co, ci, k in conv_bn_names():
        sd[conv + '.weight'] = torch.randn((co, ci, k, k), generator=g, dtype=torch.float64) * math.sqrt(2.0 / (ci * k * k))
        scale = 0.25 if bn.endswith('bn3') else 1.0
        sd[bn + '.weight'] = scale * (1.0 + 0.1 * (2 * torch.rand((co,), generator=g, dtype=torch.float64) - 1))
        sd[bn + '.bias'] = 0.1 * (2 * torch.rand((co,), generator=g, dtype=torch.float64) - 1)
        sd[bn + '.running_mean'] = 0.1 * (2 * torch.rand((co,), generator=g, dtype=torch.float64) - 1)
        sd[bn + '.running_var'] = 0.5 + torch.rand((co,), generator=g, dtype=torch.float64)
        if bn.startswith('fpn.'):
            sd[bn + '.num_batches_tracked'] = torch.tensor(0)
    return sd


def f32_state_dict(seed=7):
    return {k: (v.float() if v.is_floating_point() else v) for k, v in seeded_state_dict(seed).items()}


def sizes(h, w, min_size, max_size):
    """(oh, ow, ph, pw): torchvision holds the scale in float32 and interpolate floors dim * scale."""
    s = float(torch.min(torch.tensor(float(min_size)) / torch.tensor(float(min(h, w))),
                        torch.tensor(float(max_size)) / torch.tensor(float(max(h, w)))))
    oh, ow = int(math.floor(h * s)), int(math.floor(w * s))
    return oh, ow, int(math.ceil(oh / 32) * 32), int(math.ceil(ow / 32) * 32)


def prepare(img, min_size, max_size):
    """img (F, 3, H, W) in [0, 1] of the wanted dtype -> normalised, resized, zero-padded (F, 3, ph, pw)."""
    dt = img.dtype
    x = (img - torch.tensor(MEAN, dtype=dt).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=dt).view(1, 3, 1, 1)
    oh, ow, ph, pw = sizes(img.shape[2], img.shape[3], min_size, max_size)
    x = F.interpolate(x, size=(oh, ow), mode='bilinear', align_corners=False)      # size given = the scale recomputed from the sizes
    out = torch.zeros((img.shape[0], 3, ph, pw), dtype=dt)
    out[:, :, :oh, :ow] = x
    return out


def _cb(sd, x, conv, bn, stride=1, padding=0, relu=False):
    dt = x.dtype
    y = F.conv2d(x, sd[conv + '.weight'].to(dt), None, stride, padding)
    y = F.batch_norm(y, sd[bn + '.running_mean'].to(dt), sd[bn + '.running_var'].to(dt), sd[bn + '.weight'].to(dt),
                     sd[bn + '.bias'].to(dt), False, 0.0, EPS)
    return F.relu(y) if relu else y


def stem(sd, x):
    return F.max_pool2d(_cb(sd, x, 'body.conv1', 'body.bn1', 2, 3, True), 3, 2, 1)


def body(sd, x):
    """pooled stem output -> [C2, C3, C4, C5]"""
    c = []
    for li, (n, _) in enumerate(LAYERS, 1):
        for b in range(n):
            p = 'body.layer%d.%d.' % (li, b)
            s = 2 if (b == 0 and li > 1) else 1
            y = _cb(sd, x, p + 'conv1', p + 'bn1', relu=True)
            y = _cb(sd, y, p + 'conv2', p + 'bn2', s, 1, True)             # v1.5: the stride sits on the 3x3
            y = _cb(sd, y, p + 'conv3', p + 'bn3')
            if b == 0:
                x = _cb(sd, x, p + 'downsample.0', p + 'downsample.1', s)
            x = F.relu(y + x)
        c.append(x)
    return c


def fpn(sd, c):
    """[C2..C5] -> levels '0', '1', '2' (torchvision's FeaturePyramidNetwork: conv + BatchNorm without activation, nearest)."""
    last = _cb(sd, c[3], 'fpn.inner_blocks.3.0', 'fpn.inner_blocks.3.1')
    outs = [None] * 3
    for i in (2, 1, 0):
        lat = _cb(sd, c[i], 'fpn.inner_blocks.%d.0' % i, 'fpn.inner_blocks.%d.1' % i)
        last = lat + F.interpolate(last, size=lat.shape[-2:], mode='nearest')
        outs[i] = _cb(sd, last, 'fpn.layer_blocks.%d.0' % i, 'fpn.layer_blocks.%d.1' % i, 1, 1)
    return outs


def forward(sd, img, min_size, max_size):
    """-> dict(prepared, stem, c = [C2..C5], p = [P2, P3, P4]), all NCHW in img's dtype."""
    with torch.no_grad():
        x = prepare(img, min_size, max_size)
        s = stem(sd, x)
        c = body(sd, s)
        return {'prepared': x, 'stem': s, 'c': c, 'p': fpn(sd, c)}


def sample_images(n=3, h=40, w=75, seed=11):
    """u8 (n, h, w, 3) distinct frames."""
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def reference(dtype_name='float64', n=3, min_size=48, max_size=96):
    """The restatement on the test images, computed once per process and shared (treat as read-only)."""
    dt = getattr(torch, dtype_name)
    img = sample_images(n).permute(0, 3, 1, 2).to(dt) / 255
    return forward(seeded_state_dict(), img, min_size, max_size)
