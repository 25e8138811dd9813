"""The frozen image extractor on the GPU (csrc/extractor.hip, modules/imhead/Extractor.py) against the float64 restatement of
tests/extractor_ref.py: each new kernel alone, the whole network in ``bf16x6`` and ``f32``, frame independence, the module
interface, and the map geometry at KITTI size."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extractor_ref as R                                        # noqa: E402

pytestmark = pytest.mark.gpu
BAR = 1e-4              # of each map's largest magnitude: the project's feature bar (tests/test_configs_gpu.py)
MIN_SIZE, MAX_SIZE = 48, 96          # 40x75 -> scale 1.2 -> 48x90 -> padded 64x96


def _dev():
    return torch.device('cuda:0')


def _rel(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


def _cl(t):
    """NCHW reference map -> channels-last (F, h, w, C)."""
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.fixture(scope='module')
def extractor():
    from modules.imhead.Pipe import ImageFeatureExtractor
    ex = ImageFeatureExtractor()
    ex.load_weights(R.f32_state_dict(), MIN_SIZE, MAX_SIZE)
    return ex.to(_dev())


@pytest.fixture
def convmath(request):
    import modules.config as cfg
    old = cfg.config.get('convmath', 'f32')
    cfg.config['convmath'] = request.param
    yield request.param
    cfg.config['convmath'] = old


@pytest.mark.parametrize('layout', ['u8_hwc', 'f32_chw'])
def test_image_prepare(layout):
    """Bound: the kernel holds the coordinate scale and the source coordinate in float32 as torch does: a source coordinate
    below 75 carries an error of a few 2^-24 * 75 = 1.4e-5, which moves a sample by that fraction of the difference of two
    neighbours (at most 1 / 0.224 = 4.5 after the normalisation): 6e-5 absolute, 2.4e-5 of the largest magnitude 2.6; the
    float32 products add 1e-6.  5e-5 of the largest magnitude.  Padding must be exactly zero."""
    from modules import _hip
    img = R.sample_images(3)
    ref = R.reference('float64')['prepared']
    if layout == 'u8_hwc':
        x = img.to(_dev())
    else:
        x = (img.permute(0, 3, 1, 2).float() / 255).contiguous().to(_dev())
    out, (oh, ow) = _hip.image_prepare(x, MIN_SIZE, MAX_SIZE)
    assert (oh, ow) == (48, 90) and out.shape == (3, 64, 96, 4)
    err = _rel(out[..., :3], _cl(ref))
    print('image_prepare %s: %.2e of the largest magnitude' % (layout, err))
    assert err < 5e-5
    o = out.cpu()
    assert float(o[:, 48:].abs().max()) == 0.0 and float(o[:, :, 90:].abs().max()) == 0.0 and float(o[..., 3].abs().max()) == 0.0


def test_stem_and_pool():
    """7x7 / 2 convolution (folded BatchNorm, ReLU) + max pool on the float64 prepared image, against the unfolded restatement."""
    from modules import _hip
    from modules.imhead import Extractor as E
    sd, ref = R.seeded_state_dict(), R.reference('float64')
    w, b = E.fold_bn(sd['body.conv1.weight'], *(sd['body.bn1.' + t] for t in ('weight', 'bias', 'running_mean', 'running_var')))
    x4 = torch.zeros((3, 64, 96, 4), dtype=torch.float32)
    x4[..., :3] = _cl(ref['prepared']).float()
    conv = _hip.stem_conv7(x4.to(_dev()), w.float().permute(2, 3, 1, 0).contiguous().to(_dev()), b.float().to(_dev()))
    assert conv.shape == (3, 32, 48, 64)
    out = _hip.maxpool3s2(conv)
    assert out.shape == (3, 16, 24, 64)
    err = _rel(out, _cl(ref['stem']))
    print('stem + pool: %.2e of the largest magnitude' % err)
    assert err < BAR


@pytest.mark.parametrize('hw', [(2, 3), (4, 6), (8, 12)])
@pytest.mark.parametrize('C', [64, 256])
def test_elementwise_glue(hw, C):
    """Skip epilogue, stride-2 row gather, top-down merge: one float32 addition per element at most, which is correctly rounded,
    so the results equal the float64 restatement rounded to float32 EXACTLY."""
    from modules import _hip
    from modules import Extension as X
    import torch.nn.functional as Fn
    h, w = hw
    g = torch.Generator().manual_seed(h * 100 + C)
    a, b = torch.randn((3, h, w, C), generator=g), torch.randn((3, h, w, C), generator=g)
    top = torch.randn((3, h, w, C), generator=g)
    lat = torch.randn((3, 2 * h, 2 * w, C), generator=g)
    da, db, dtop, dlat = (t.to(_dev()) for t in (a, b, top, lat))
    assert torch.equal(_hip.add_relu(da, db).cpu(), Fn.relu(a.double() + b.double()).float())
    assert torch.equal(_hip.gather_stride2(da).cpu(), a[:, ::2, ::2].contiguous())
    up = Fn.interpolate(top.double().permute(0, 3, 1, 2), size=(2 * h, 2 * w), mode='nearest').permute(0, 2, 3, 1)
    assert torch.equal(_hip.topdown_merge(dlat, dtop).cpu(), (lat.double() + up).float())
    with pytest.raises(X.MvxHipError):                # a lateral map that is not exactly twice the top one
        _hip.topdown_merge(dlat[:, :2 * h - 1].contiguous(), dtop)


def _run(extractor, n):
    maps = extractor._network(_dev()).maps(R.sample_images(3)[:n].contiguous().to(_dev()))
    torch.cuda.synchronize()
    return maps


@pytest.mark.parametrize('convmath', ['bf16x6', 'f32'], indirect=True)
def test_whole_network_and_frame_independence(extractor, convmath):
    """F = 3 distinct frames and F = 1: maps 16x24, 8x12, 4x6 (deepest stage 2x3) within 1e-4 of each map's largest magnitude of
    the float64 restatement; frame k of the set equals the single-frame call bit for bit; a repeated call is bit-identical."""
    ref = R.reference('float64')
    m3 = _run(extractor, 3)
    assert [tuple(m.shape) for m in m3] == [(3, 16, 24, 256), (3, 8, 12, 256), (3, 4, 6, 256)]
    for i, m in enumerate(m3):
        err = _rel(m, _cl(ref['p'][i]))
        print('%s P%d (F = 3): %.2e of the largest magnitude %.3g' % (convmath, i + 2, err, float(ref['p'][i].abs().max())))
        assert err < BAR, (convmath, i, err)
    m1 = _run(extractor, 1)
    for i, m in enumerate(m1):
        err = _rel(m, _cl(ref['p'][i][:1]))
        print('%s P%d (F = 1): %.2e' % (convmath, i + 2, err))
        assert err < BAR, (convmath, i, err)
        assert torch.equal(m[0], m3[i][0]), 'frame 0 of the set differs from the single-frame call (level %d)' % i
    again = _run(extractor, 3)
    assert all(torch.equal(a, b) for a, b in zip(again, m3))
    one = extractor._network(_dev()).maps(R.sample_images(3)[2:3].contiguous().to(_dev()))
    assert all(torch.equal(a[0], b[2]) for a, b in zip(one, m3)), 'frame 2 of the set differs from the single-frame call'


def _small_model_inputs(dev):
    from modules import _hip
    import modules.config as cfg
    g = np.random.default_rng(0)
    lo, hi = np.array(cfg.velorange[:3]), np.array(cfg.velorange[3:])
    pts = (g.random((600, 3)) * (hi - lo) * 0.999 + lo).astype(np.float32)
    proj = np.stack([g.uniform(0, 39, 600), g.uniform(0, 74, 600)], 1).astype(np.float32)
    pcd = np.concatenate([pts, g.random((600, 1)).astype(np.float32), proj], 1)
    perm = g.permutation(600).astype(np.int32)
    res = _hip.voxelize(torch.from_numpy(pcd).to(dev)[None], torch.from_numpy(perm).to(dev)[None], None, cfg.velorange[:3],
                        cfg.voxelsize, 35, 9)
    V = int(res.n_voxels[0])
    return res.voxels[0, :V].unsqueeze(0).clone(), res.coords[0, :V].clone()


def test_module_interface():
    """Before load_weights: the key list is today's and an image raises the old error.  A checkpoint with
    ``head.extractor.backbone.*`` keys loads; after it MVXNet.forward on the image equals forward on the extractor's own maps."""
    import modules.config as cfg
    from MVXNet import MVXNet
    dev = _dev()
    old, old_range = list(cfg.config['voxelshape']), list(cfg.config['velorange'])
    cfg.config['voxelshape'] = [16, 24, 10]
    cfg.config['velorange'] = [0.0, -2.4, -3.0, 3.2, 2.4, 1.0]
    cfg.config['voxelsize'] = [(cfg.config['velorange'][k + 3] - cfg.config['velorange'][k]) / cfg.config['voxelshape'][k] for k in range(3)]
    try:
        torch.manual_seed(0)
        model = MVXNet().to(dev)
        keys = list(model.state_dict())
        assert not any('extractor' in k for k in keys)
        voxels, idx = _small_model_inputs(dev)
        image = (R.sample_images(1).permute(0, 3, 1, 2).float() / 255).to(dev)
        imsize = torch.tensor([40.0, 75.0], device=dev)
        try:
            import torchvision  # noqa: F401
        except ImportError:
            with pytest.raises(RuntimeError, match='torchvision is not installed'):
                model(voxels.clone(), image, idx, [None], imsize)
        ckpt = {k: v.clone() for k, v in model.state_dict().items()}
        ckpt.update({'head.extractor.backbone.' + k: v for k, v in R.f32_state_dict().items()})
        model.load_state_dict(ckpt, strict=True)
        model.head.extractor.min_size, model.head.extractor.max_size = MIN_SIZE, MAX_SIZE
        assert len(model.state_dict()) == len(keys) + 300
        with torch.no_grad():
            maps = model.head.extractor(image)
            assert [tuple(m.shape) for m in maps] == [(1, 256, 16, 24), (1, 256, 8, 12), (1, 256, 4, 6)]
            assert all(m[0].permute(1, 2, 0).is_contiguous() for m in maps)           # _channels_last_levels does not copy
            s1, r1 = model(voxels.clone(), image, idx, [None], imsize)
            s2, r2 = model(voxels.clone(), maps, idx, [None], imsize)
        assert torch.isfinite(s1).all() and torch.equal(s1, s2) and torch.equal(r1, r2)
        frames = model.head.extractor.extract_frames(R.sample_images(1).to(dev))
        assert all(torch.equal(a, b) for a, b in zip(frames[0], maps))                 # u8 entry = f32 / 255 entry
    finally:
        cfg.config['voxelshape'] = old
        cfg.config['velorange'] = old_range
        cfg.config['voxelsize'] = [(old_range[k + 3] - old_range[k]) / old[k] for k in range(3)]


def test_geometry_at_kitti_size():
    """One 370 x 1224 u8 frame with the default sizes: finite maps of 104x336, 52x168, 26x84 (no numeric reference)."""
    from modules.imhead.Pipe import ImageFeatureExtractor
    ex = ImageFeatureExtractor().load_weights(R.f32_state_dict()).to(_dev())
    img = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (1, 370, 1224, 3), dtype=np.uint8)).to(_dev())
    maps = ex.extract_frames(img)[0]
    assert [tuple(m.shape) for m in maps] == [(1, 256, 104, 336), (1, 256, 52, 168), (1, 256, 26, 84)]
    assert all(bool(torch.isfinite(m).all()) for m in maps)
