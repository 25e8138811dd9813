"""MVXNet top module with the reference's interface (MVXNet.py:13-27):
``forward(voxels (1,N,T,9), imgs, idx (N,4), calibs, imsize) -> (score, reg)``, and ``detect`` (same inputs + the anchor
grid) -> the frame's boxes after decoding and NMS (modules/detect.py; the reference has no detection output)."""
import torch
from torch import nn

from modules import _hip
from modules.imhead import ImageHead
from modules.voxelnet import VoxelNet

__all__ = ['MVXNet']


def initWeights(m):
    # the reference re-initialises nn.Conv2d only (MVXNet.py:8-11): Linear / Conv3d /
    # ConvTranspose2d keep PyTorch's defaults
    if isinstance(m, nn.Conv2d):
        nn.init.xavier_uniform_(m.weight.data)
        m.bias.data.zero_()


class MVXNet(nn.Module):

    def __init__(self, direction=False, iou=False):
        """``direction``: the RPN carries the direction classifier ``backbone.rpn.dir`` (voxelnet/Pipe.py RPN); ``iou`` (with
        ``direction``): and the IoU-aware confidence head ``backbone.rpn.iou``."""
        super().__init__()
        self.head = ImageHead()
        self.backbone = VoxelNet(direction=direction, iou=iou)
        self.backbone.apply(initWeights)

    def load_state_dict(self, state_dict, strict=True, **kw):
        """As nn.Module.load_state_dict; a checkpoint that carries the frozen extractor (``head.extractor.backbone.*``, what the
        reference's train.py writes) also loads it (``ImageFeatureExtractor.load_weights``): the tensors the three FPN levels
        read are kept, the rest of that subtree (RPN / ROI heads, unread FPN blocks) is dropped."""
        pre = 'head.extractor.'
        if any(k.startswith(pre + 'backbone.') for k in state_dict):
            self.head.extractor.load_weights({k: v for k, v in state_dict.items() if k.startswith(pre + 'backbone.')})
            dev = next(self.parameters()).device
            self.head.extractor.to(dev)
            kept = {pre + k for k in self.head.extractor.state_dict()}
            state_dict = {k: v for k, v in state_dict.items() if not k.startswith(pre) or k in kept}
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def prepack(self):
        """Pack the dense-conv weights on the CURRENT stream for the arithmetic in use, so frames that
        run on other streams find them ready (modules/pipeline.py)."""
        from modules.layers.Blocks import CRB3d, conv_split_math
        split = conv_split_math()
        for m in self.backbone.cml.modules():
            if isinstance(m, CRB3d):
                m._packer(False, split)
                m._packer(True, split)

    def point_features(self, voxels, imgs, calibs, imsize):
        """(1,N,T,9) -> (1,N,T,23): 7 geometric channels + 16 fused image channels
        (MVXNet.py:25-26).  Padded rows of ``voxels`` are zeroed in place by the head."""
        imfeatures = self.head(imgs, voxels, calibs, imsize)
        return torch.concat([voxels[..., :7], imfeatures], dim=-1)

    def middle(self, voxels, imgs, idx, calibs, imsize, compact=True, prepared=None, status_sink=None):
        """Hot path up to the RPN input.  ``compact=True`` evaluates the fusion MLP and the VFE stack on
        real rows + one padded row per voxel instead of all N*T rows -- identical results because
        inside MVXNet all padded rows of a voxel are identical; ``compact=False`` runs the
        reference's dense formulation."""
        _hip.require_plain_batchnorm('MVXNet.middle')      # bntrack lives on the frame-set path (modules/bn_running.py)
        if not compact:
            return self.backbone.middle(self.point_features(voxels, imgs, calibs, imsize), idx)
        from modules.voxelnet.Pipe import CompactInputFunction
        imfeat, cr, vox2d = self.head.forward_compact(imgs, voxels, calibs, imsize, prepared, status_sink)
        rows = CompactInputFunction.apply(imfeat, vox2d, cr)
        return self.backbone.middle(rows, idx, compact_rows=cr)

    def forward(self, voxels, imgs, idx, calibs, imsize, compact=True):
        """(1,N,T,9) voxels, image or FPN maps, (N,4) indices -> (score (1,2,H/2,W/2), reg (1,14,H/2,W/2)) (MVXNet.py:21-27).
        ``compact=True`` (default) evaluates the fusion MLP and the VFE stack on the real rows + one padded row per voxel
        and the first CML layer on the voxel rows: exact for ANY input, because featureMaping zeroes every row whose
        x = y = z = 0 in place (imhead/Pipe.py:54-59), which makes all such rows of a voxel identical from there on
        (SURVEY Q5).  On the GPU the whole forward is then ONE autograd node over the frame-set kernels (modules/whole.py);
        ``compact='modules'`` keeps the same arithmetic on the per-module autograd path (modules.voxelnet / imhead / layers),
        ``compact=False`` is the reference's dense (1,N,T,23) formulation."""
        _hip.require_plain_batchnorm('MVXNet.forward')      # bntrack lives on the frame-set path (modules/bn_running.py)
        if not compact:
            return self.backbone(self.point_features(voxels, imgs, calibs, imsize), idx)
        if compact != 'modules':
            from modules import whole
            if whole.supported(self, voxels, idx):
                return whole.forward(self, voxels, imgs, idx, imsize)
        from modules.voxelnet.Pipe import CompactInputFunction
        imfeat, cr, vox2d = self.head.forward_compact(imgs, voxels, calibs, imsize)
        rows = CompactInputFunction.apply(imfeat, vox2d, cr)
        return self.backbone(rows, idx, compact_rows=cr)

    def detect(self, voxels, imgs, idx, calibs, imsize, anchors, **kw):
        """Boxes of one frame, with forward's inputs (MVXNet.py:21-27) and the anchor grid (h1, w1, 14)
        (Preprocessing.createAnchors): the forward on the single HIP node up to the raw head logits, then
        ``modules.detect.postprocess`` (keyword arguments as there: score_thr, iou_thr, pre_max, post_max, decode).
        A model with the direction head decodes through it (``direction`` / ``dir_offset`` of postprocess): yaws in [-pi, pi);
        one with the IoU head ranks and scores by cls^(1-a) iou^a (``iou_alpha`` of postprocess, default 0.5).
        Returns ``{boxes (n,7) xyzlwhr LiDAR frame, scores (n,), anchor_idx (n,), n_candidates, status}``."""
        from modules import detect, whole
        from modules import Extension as X
        import modules.config as cfg
        _hip.require_plain_batchnorm('MVXNet.detect')      # bntrack lives on the frame-set path (modules/bn_running.py)
        if not whole.supported(self, voxels, idx):
            raise X.MvxHipError('MVXNet.detect runs on the single-node HIP path: f32 contiguous (1,N,T,9) voxels and (N,4) i64 '
                                'indices on the GPU, the background rewrite and the HIP RPN on, map sides divisible by 8')
        with torch.no_grad():
            heads = whole.forward_heads(self, voxels, imgs, idx, imsize)
            kw.setdefault('iou', hasattr(self.backbone.rpn, 'iou'))
            return detect.postprocess(heads, anchors, 1, cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2, **kw)[0]
