"""Host side of the frozen image extractor (modules/imhead/Extractor.py): size arithmetic, a hand-computed resize, BatchNorm
folding, the weight loader, and that float32 arithmetic can reach the bar of the GPU test at the test weights.  No GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extractor_ref as R                                        # noqa: E402
from modules.imhead import Extractor as E                        # noqa: E402

BAR = 1e-4              # of each map's largest magnitude: the project's feature bar (tests/test_configs_gpu.py)


def test_size_arithmetic_kitti():
    oh, ow, ph, pw = E.prepared_size(370, 1224)
    assert oh == 402 and ow in (1332, 1333) and (ph, pw) == (416, 1344)
    assert [(ph // s, pw // s) for s in (4, 8, 16)] == [(104, 336), (52, 168), (26, 84)]
    assert E.prepared_size(40, 75, 48, 96) == (48, 90, 64, 96)
    assert R.sizes(40, 75, 48, 96) == (48, 90, 64, 96) and R.sizes(370, 1224, 800, 1333)[2:] == (416, 1344)
    assert E.prepared_size(375, 1242) == R.sizes(375, 1242, 800, 1333)          # the other KITTI size


def test_hand_computed_bilinear_and_padding():
    """2x3 image, min_size 4, max_size 6: scale 2 -> 4x6 -> padded 32x32.  align_corners=False with scale 0.5: output column x
    reads source 0.5 * (x + 0.5) - 0.5 = -0.25 (clamped to 0), 0.25, 0.75, 1.25, 1.75, 2.25 (column 2 with weight 1); rows
    -0.25 -> 0, 0.25, 0.75, 1.25 -> row 1.  Values are 10 * row + column before the normalisation, which is affine and the
    same for every pixel of a channel, so it commutes with the interpolation."""
    img = torch.tensor([[0., 1., 2.], [10., 11., 12.]], dtype=torch.float64)
    x = img.view(1, 1, 2, 3).repeat(1, 3, 1, 1)
    assert R.sizes(2, 3, 4, 6) == (4, 6, 32, 32) == E.prepared_size(2, 3, 4, 6)
    out = R.prepare(x, 4, 6)
    cols = [0.0, 0.25, 0.75, 1.25, 1.75, 2.0]
    rows = [0.0, 2.5, 7.5, 10.0]
    for c in range(3):
        want = torch.tensor([[(r + q - R.MEAN[c]) / R.STD[c] for q in cols] for r in rows], dtype=torch.float64)
        assert torch.allclose(out[0, c, :4, :6], want, rtol=0, atol=1e-12)
    assert out.shape == (1, 3, 32, 32)
    assert float(out[:, :, 4:].abs().max()) == 0.0 and float(out[:, :, :, 6:].abs().max()) == 0.0      # zeros, not -mean/std


def test_folded_weights_equal_unfolded_batchnorm():
    sd = R.seeded_state_dict()
    g = torch.Generator().manual_seed(1)
    for conv, bn, stride, pad in (('body.conv1', 'body.bn1', 2, 3), ('body.layer2.0.conv2', 'body.layer2.0.bn2', 2, 1),
                                  ('body.layer1.0.downsample.0', 'body.layer1.0.downsample.1', 1, 0),
                                  ('fpn.layer_blocks.1.0', 'fpn.layer_blocks.1.1', 1, 1)):
        cin = sd[conv + '.weight'].shape[1]
        x = torch.randn((2, cin, 9, 11), generator=g, dtype=torch.float64)
        want = R._cb(sd, x, conv, bn, stride, pad)
        w, b = E.fold_bn(sd[conv + '.weight'], sd[bn + '.weight'], sd[bn + '.bias'], sd[bn + '.running_mean'], sd[bn + '.running_var'])
        assert w.dtype == torch.float64 and b.dtype == torch.float64
        got = torch.nn.functional.conv2d(x, w, b, stride, pad)
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), conv


@pytest.mark.parametrize('prefix', ['', 'backbone.', 'head.extractor.backbone.'])
def test_loader_accepts_prefixes_and_ignores_other_keys(prefix, tmp_path):
    sd = R.f32_state_dict()
    src = {prefix + k: v for k, v in sd.items()}
    src.update({'rpn.head.conv.0.0.weight': torch.zeros(3), 'roi_heads.box_predictor.cls_score.bias': torch.zeros(2),
                'head.fusion.fcn1.fc.weight': torch.zeros(4), prefix + 'body.bn1.num_batches_tracked': torch.tensor(5)})
    got = E.clean_state_dict(src)
    want = E.expected_shapes()
    assert set(got) == set(want) and len(want) == 53 * 5 + 7 * 5
    assert all(torch.equal(got[k], sd[k]) for k in want)
    assert not any(k.startswith('fpn.layer_blocks.3') or k.endswith('num_batches_tracked') for k in got)
    path = os.path.join(str(tmp_path), 'w.pt')
    torch.save(src, path)
    from_file = E.clean_state_dict(path)
    assert all(torch.equal(from_file[k], sd[k]) for k in want)


def test_loader_lists_every_missing_or_misshapen_key():
    sd = dict(R.f32_state_dict())
    del sd['body.layer2.0.downsample.1.running_var']
    del sd['fpn.inner_blocks.0.0.weight']
    sd['body.conv1.weight'] = torch.zeros(64, 3, 3, 3)
    sd['fpn.layer_blocks.2.1.bias'] = torch.zeros(128)
    with pytest.raises(ValueError) as e:
        E.clean_state_dict(sd)
    msg = str(e.value)
    for k in ('body.layer2.0.downsample.1.running_var', 'fpn.inner_blocks.0.0.weight', 'body.conv1.weight', 'fpn.layer_blocks.2.1.bias'):
        assert k in msg, k
    assert '4 problem' in msg


def test_module_keeps_its_keys_until_weights_are_loaded():
    from MVXNet import MVXNet
    m = MVXNet()
    before = list(m.state_dict())
    assert not any('extractor' in k for k in before)
    ckpt = dict(m.state_dict())
    ckpt.update({'head.extractor.backbone.' + k: v for k, v in R.f32_state_dict().items()})
    ckpt['head.extractor.backbone.fpn.layer_blocks.3.0.weight'] = torch.zeros(256, 256, 3, 3)       # unread: dropped, not an error
    m.load_state_dict(ckpt, strict=True)
    after = list(m.state_dict())
    want = ['head.extractor.backbone.' + k for k in E.expected_shapes()]
    assert sorted(after) == sorted(before + want)
    assert torch.equal(m.state_dict()['head.extractor.backbone.fpn.layer_blocks.2.1.bias'], R.f32_state_dict()['fpn.layer_blocks.2.1.bias'])
    assert list(MVXNet().state_dict()) == before                   # a fresh model is unaffected
    m2 = MVXNet()
    m2.load_state_dict(m.state_dict())                             # its own checkpoint round-trips


def test_float32_restatement_reaches_the_bar():
    """The 1e-4 bar of the GPU test is reachable by float32 arithmetic at the test weights: the float32 restatement against
    the float64 one, every read map."""
    r64, r32 = R.reference('float64'), R.reference('float32')
    for name, a, b in [('prepared', r32['prepared'], r64['prepared']), ('stem', r32['stem'], r64['stem'])] + \
            [('p%d' % i, r32['p'][i], r64['p'][i]) for i in range(3)]:
        err = float((a.double() - b).abs().max() / b.abs().max())
        print('%s: float32 vs float64 restatement %.2e of the largest magnitude %.3g' % (name, err, float(b.abs().max())))
        assert err < BAR, (name, err)
    assert [tuple(p.shape[-2:]) for p in r64['p']] == [(16, 24), (8, 12), (4, 6)] and tuple(r64['c'][3].shape[-2:]) == (2, 3)
