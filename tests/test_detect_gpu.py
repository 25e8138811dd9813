"""Detection output on the GPU (csrc/detect.hip, modules/detect.py, MVXNet.detect): candidate order, selection, decoding,
corners and NMS exactly against a host reference (tests/detect_ref.py on the C oracle's IoU); planted boxes found once each;
the forward of the detection step equal to the training step's; MVXNet.detect on the single-node forward."""
import math

import numpy as np
import pytest
import torch

import detect_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')
L1, W1, A = 176, 200, 2


def _anchors(l=L1, w=W1):
    import modules.config as cfg
    from modules.data import Preprocessing as pre
    return pre.createAnchors(l, w, cfg.velorange, cfg.carsize)           # (l, w, 14) = [l][w][A][7]


def _avoid_band(logits, thr):
    """Logits whose sigmoid is not within 1e-6 of the threshold (selection must not hinge on the last bit of exp)."""
    p = torch.sigmoid(torch.from_numpy(logits))
    bad = (p - thr).abs() < 1e-6
    logits[bad.numpy()] += 0.01
    return logits


def _synthetic_heads(F, seed):
    """(F*L1*W1, 16) heads: logits quantised to 1/8 (many exact ties, also at the selection threshold), one frame mostly far
    below the threshold (fewer candidates than pre_max), regressions ~ N(0, 0.3)."""
    g = np.random.default_rng(seed)
    lg = np.round(g.normal(0.0, 2.0, (F, L1 * W1, A)) * 8) / 8
    lg[F - 1] -= 6.0
    heads = np.zeros((F, L1 * W1, 16), np.float32)
    heads[..., :A] = lg
    heads[..., A:] = g.normal(0.0, 0.3, (F, L1 * W1, 14))
    return heads


def test_candidates_decode_corners_and_nms_match_the_reference():
    from modules import Calc
    from modules.detect import postprocess
    F, thr, pre_max, post_max, iou_thr = 3, 0.4, 500, 60, 0.1
    heads = _synthetic_heads(F, 1)
    heads[..., :A] = _avoid_band(heads[..., :A].copy(), thr)
    anchors = _anchors()
    anc = anchors.reshape(-1, 7).numpy()
    h_dev = torch.from_numpy(heads).to(DEV).reshape(F * L1 * W1, 16)
    for mode in ('loss', 'reference'):
        out = postprocess(h_dev, anchors, F, L1, W1, score_thr=thr, iou_thr=iou_thr, pre_max=pre_max, post_max=post_max,
                          decode=mode, read=False, debug=True)
        meta = out['meta'].cpu().numpy()
        cand, cboxes, ccorn = out['cand_idx'].cpu().numpy(), out['cand_boxes'].cpu().numpy(), out['cand_corners'].cpu().numpy()
        for f in range(F):
            logits = heads[f, :, :A].reshape(-1)                     # anchor index n = (x*w + y)*A + a
            ref_idx, n_above = R.candidates(logits, thr, pre_max)
            K = len(ref_idx)
            assert meta[1, f] == n_above and meta[2, f] == (1 if n_above > pre_max else 0)
            assert np.array_equal(cand[f, :K], ref_idx) and (cand[f, K:] == -1).all(), (mode, f)
            reg = heads[f, :, A:].reshape(-1, A * 7)[ref_idx // A].reshape(-1, A, 7)[np.arange(K), ref_idx % A]
            want = R.decode(reg, anc[ref_idx], mode)
            got = cboxes[f, :K].astype(np.float64)
            # 1e-6 relative to the operands: in 'reference' mode r * |(x_a, y_a)| and the anchor centre may cancel
            err = np.abs(got - want) / R.decode_scale(reg, anc[ref_idx], mode)
            assert err.max() <= 1e-6, (mode, f, err.max())
            if mode == 'reference':
                ref_t = Calc.decodeRegression(torch.from_numpy(reg), torch.from_numpy(anc[ref_idx])).numpy()
                assert (np.abs(got - ref_t) / R.decode_scale(reg, anc[ref_idx], mode)).max() <= 1e-6
            want_c = R.corners(cboxes[f, :K])
            assert np.all(np.abs(ccorn[f, :K] - want_c) <= 1e-5 * np.maximum(np.abs(want_c), 1.0)), (mode, f)
            keep = R.greedy_nms(ccorn[f, :K].astype(np.float32), iou_thr, post_max)
            n = meta[0, f]
            assert n == len(keep), (mode, f, n, len(keep))
            assert np.array_equal(out['anchor_idx'][f, :n].cpu().numpy(), ref_idx[keep])
            assert torch.equal(out['boxes'][f, :n].cpu(), torch.from_numpy(cboxes[f, keep]))
            want_s = torch.sigmoid(torch.from_numpy(logits[ref_idx[keep]]))
            assert torch.allclose(out['scores'][f, :n].cpu(), want_s, rtol=1e-6, atol=0)
            assert (out['anchor_idx'][f, n:] == -1).all()
        assert meta[1, F - 1] < pre_max and meta[1, 0] > pre_max      # both the selection and the "take all" path ran


def _planted(boxes_per_frame, background=-10.0):
    """NCHW maps (F,2,L1,W1) / (F,14,L1,W1): every box encoded (VoxelLoss's targets) into the 3x3 cells x 2 orientations
    around its centre cell, logits 2 + 0.05 * (member number) with the maximum at a known member."""
    anchors = _anchors()
    F = len(boxes_per_frame)
    cls = np.full((F, A, L1, W1), background, np.float32)
    reg = np.zeros((F, 7 * A, L1, W1), np.float32)
    best = []
    for f, boxes in enumerate(boxes_per_frame):
        best.append([])
        for b, (gt, top) in enumerate(boxes):
            x = int((gt[0] - 0.0) / 0.4)
            y = int((gt[1] + 40.0) / 0.4)
            m = 0
            for dx in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for a in range(A):
                        an = anchors[x + dx, y + dy, 7 * a:7 * a + 7].numpy()
                        reg[f, 7 * a:7 * a + 7, x + dx, y + dy] = R.encode(gt, an)
                        cls[f, a, x + dx, y + dy] = top - 0.05 * ((m * 7) % 18)
                        if (m * 7) % 18 == 0:
                            best[-1].append(((x + dx) * W1 + (y + dy)) * A + a)
                        m += 1
    return torch.from_numpy(cls).to(DEV), torch.from_numpy(reg).to(DEV), best


def _bev_iou(b1, b2):
    import mvx_oracle as O
    return float(O.bbox_pairwise(R.corners([b1]), R.corners([b2]), True)[0, 0])


GTS = [(np.array([20.0, -10.0, -1.0, 3.9, 1.6, 1.5, 0.1]), 3.0), (np.array([40.0, 12.0, -0.8, 4.2, 1.7, 1.6, 1.65]), 2.5),
       (np.array([55.0, -25.0, -1.2, 3.6, 1.5, 1.4, -0.4]), 2.0), (np.array([12.0, 30.0, -1.1, 4.0, 1.65, 1.55, 3.0]), 1.5)]
DX = 4.0 * 0.7 / 1.3                                               # two 4 m boxes side by side at BEV IoU 0.3
PAIR = [(np.array([30.0, -2.0, -1.0, 4.0, 1.6, 1.5, 0.0]), 2.0), (np.array([30.0 + DX, -2.0, -1.0, 4.0, 1.6, 1.5, 0.0]), 1.0)]


def test_planted_boxes():
    from modules.detect import postprocess
    anchors = _anchors()
    cls, reg, best = _planted([GTS, PAIR, []])
    assert abs(_bev_iou(PAIR[0][0], PAIR[1][0]) - 0.3) < 1e-3

    def run(maps, **kw):
        return postprocess(maps, anchors, maps[0].shape[0], L1, W1, **kw)

    d = run((cls, reg))
    assert [x['boxes'].shape[0] for x in d] == [4, 1, 0]              # default iou_thr 0.01: the pair's lower box goes too
    for k, (gt, top) in enumerate(GTS):
        assert torch.allclose(d[0]['boxes'][k].cpu().double(), torch.from_numpy(gt), rtol=1e-5, atol=1e-5), k
        assert int(d[0]['anchor_idx'][k]) == best[0][k]
        assert math.isclose(float(d[0]['scores'][k]), float(torch.sigmoid(torch.tensor(top, dtype=torch.float32))), rel_tol=1e-6)
    assert d[0]['status'] == 0 and d[0]['n_candidates'] == 4 * 18 and d[2]['n_candidates'] == 0
    # the pair: both survive at 0.5, the higher one alone at 0.2
    d5 = run((cls, reg), iou_thr=0.5)
    assert d5[1]['boxes'].shape[0] == 2 and d5[1]['anchor_idx'].tolist() == best[1]
    d2 = run((cls, reg), iou_thr=0.2)
    assert d2[1]['anchor_idx'].tolist() == best[1][:1]
    # post_max truncates (the best boxes first); pre_max truncation sets status bit 1
    dp = run((cls, reg), post_max=2)
    assert dp[0]['anchor_idx'].tolist() == best[0][:2]
    dt = run((cls, reg), pre_max=10, post_max=10)
    assert dt[0]['status'] & 1 and not dt[2]['status'] & 1 and dt[0]['n_candidates'] == 72
    # frames permuted -> outputs permuted; two runs bitwise equal
    perm = [2, 0, 1]
    dq = run((cls[perm].contiguous(), reg[perm].contiguous()))
    for i, f in enumerate(perm):
        for k in ('boxes', 'scores', 'anchor_idx'):
            assert torch.equal(dq[i][k], d[f][k])
    raw1 = postprocess((cls, reg), anchors, 3, L1, W1, read=False)
    raw2 = postprocess((cls, reg), anchors, 3, L1, W1, read=False)
    for k in ('boxes', 'scores', 'anchor_idx', 'meta'):
        assert torch.equal(raw1[k], raw2[k])
    # a non-finite decoded box is dropped and reported
    reg_bad = reg.clone()
    n0 = best[0][0]
    reg_bad[0, (n0 % A) * 7 + 3, n0 // A // W1, n0 // A % W1] = 200.0      # exp(200) * l_a = inf at the first box's best anchor
    db = run((cls, reg_bad))
    assert db[0]['status'] & 2 and best[0][0] not in db[0]['anchor_idx'].tolist()


def test_detect_step_matches_the_training_forward_and_leaves_parameters_alone():
    import bench
    import modules.config as cfg
    import modules.pipeline as pl
    from MVXNet import MVXNet
    from modules import Calc, parallel
    from modules.detect import detect_frame_set, postprocess
    from modules.voxelnet import VoxelLoss
    frames = [0, 1, 2, 3]
    batch = bench.make_batch(frames, DEV, 20000, 'S2')
    torch.manual_seed(0)
    model = MVXNet().to(DEV)
    bucket = parallel.GradBucket([p for p in model.parameters() if p.requires_grad])
    bucket.zero()
    anchors = _anchors(cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2)
    params = {k: p.detach().clone() for k, p in model.named_parameters()}
    grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    keep = {}
    dets = detect_frame_set(model, batch, anchors, cfg.imsize, keep=keep, score_thr=0.3)
    heads = keep['heads'].clone()
    torch.cuda.synchronize()
    assert len(dets) == 4
    for k, p in model.named_parameters():
        assert torch.equal(p.detach(), params[k]), k
        if k in grads:
            assert torch.equal(p.grad, grads[k]), k
    F, h1, w1 = keep['geom']
    again = postprocess(keep['heads'], anchors, F, h1, w1, score_thr=0.3)
    for a, b in zip(dets, again):
        assert torch.equal(a['boxes'], b['boxes']) and torch.equal(a['anchor_idx'], b['anchor_idx'])
    gt = bench.synthetic_gt()
    bevs = Calc.bbox3d2bev(anchors.reshape(anchors.shape[:2] + (-1, 7))).to(DEV).contiguous()
    lists = Calc.classifyAnchorsFrames([(Calc.bbox3d2bev(gt), gt[:, [0, 1]])] * 4, bevs, cfg.velorange, 0.45, 0.6)
    targets = [(t[0], t[1], t[2], gt.to(DEV)) for t in lists]
    keep2 = {}
    pl.train_step_full(model, batch, targets, VoxelLoss(), anchors.to(DEV), cfg.imsize, keep=keep2)
    torch.cuda.synchronize()
    assert torch.equal(heads, keep2['heads'])


def test_mvxnet_detect_is_postprocess_of_the_forward_logits(golden):
    import modules.config as cfg
    from MVXNet import MVXNet
    from modules import whole
    from modules.detect import postprocess
    g = golden('mvxnet_small')
    old = list(cfg.config['voxelshape'])
    cfg.config['voxelshape'] = [int(v) for v in g['voxelshape']]
    try:
        torch.manual_seed(4)
        model = MVXNet().to(DEV)
        feats = [torch.from_numpy(g[k])[None].to(DEV) for k in ('f0', 'f1', 'f2')]
        idx = torch.from_numpy(g['idx']).to(DEV)
        imsize = torch.from_numpy(g['imsize_hw']).to(DEV)
        h1, w1 = cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2
        anchors = _anchors(h1, w1)

        def vox():
            return torch.from_numpy(g['voxels'].copy())[None].to(DEV)
        det = model.detect(vox(), feats, idx, [None], imsize, anchors, score_thr=0.2, iou_thr=0.1)
        with torch.no_grad():
            heads = whole.forward_heads(model, vox(), feats, idx, imsize)
            score, _ = model(vox(), feats, idx, [None], imsize)
        ref = postprocess(heads, anchors, 1, h1, w1, score_thr=0.2, iou_thr=0.1)[0]
        assert det['boxes'].shape[0] > 0
        for k in ('boxes', 'scores', 'anchor_idx'):
            assert torch.equal(det[k], ref[k]), k
        assert det['n_candidates'] == ref['n_candidates']
        sig = torch.sigmoid(heads.view(1, h1, w1, 16)[..., :2]).permute(0, 3, 1, 2)
        assert torch.equal(score, sig)
    finally:
        cfg.config['voxelshape'] = old
