"""2-D box helper with the reference's name (modules/utils/Bbox.py)."""
import torch


def bboxIntersection(bboxes1: torch.Tensor, bboxes2: torch.Tensor) -> torch.Tensor:
    """Intersection area of every pair of axis-aligned xyxy boxes, (N,4) x (M,4) -> (N,M), in the tensors' dtype and on
    their device.  A handful of label boxes: plain tensor operations; the augmentation's own test runs inside
    csrc/augment.hip."""
    a, b = bboxes1[:, None, :], bboxes2[None, :, :]
    w = torch.minimum(a[..., 2], b[..., 2]) - torch.maximum(a[..., 0], b[..., 0])
    h = torch.minimum(a[..., 3], b[..., 3]) - torch.maximum(a[..., 1], b[..., 1])
    return w.clamp(min=0) * h.clamp(min=0)
