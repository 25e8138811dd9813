"""Float64 restatement of the running-statistics kernels (csrc/bn_running.hip), shared by the host and the GPU tests.

The reference runs batch 1, one forward per frame, so a step of F frames is F sequential updates of
``nn.BatchNorm*d(track_running_stats=True)``: running_mean moves towards the frame's mean, running_var towards its UNBIASED
variance, num_batches_tracked counts the forwards."""
import numpy as np
import torch


def fold(mean_inv, pops, rm, rv, eps, momentum):
    """mean_inv (F,2,C) = (mean, 1/sqrt(biased var + eps)) per frame, pops[f] the frame's population (0 = the frame takes no
    part), rm / rv (C,) the buffers before the step -> (rm, rv, frames folded) in float64."""
    mi = torch.as_tensor(mean_inv).detach().cpu().double()
    rm = torch.as_tensor(rm).detach().cpu().double().clone()
    rv = torch.as_tensor(rv).detach().cpu().double().clone()
    m, live = float(momentum), 0
    for f, n in enumerate(pops):
        if n <= 0:
            continue
        var = (1.0 / (mi[f, 1] * mi[f, 1]) - eps).clamp_min(0.0)
        rm = (1.0 - m) * rm + m * mi[f, 0]
        if n > 1:
            rv = (1.0 - m) * rv + m * (var * float(n) / (n - 1.0))
        live += 1
    return rm, rv, live


def mean_inv_of(rm, rv, eps, F):
    """(F,2,C) f32: (running_mean, the float64 1/sqrt(running_var + eps) rounded once), the same for every frame."""
    rm = torch.as_tensor(rm).detach().cpu().float()
    inv = (1.0 / torch.sqrt(torch.as_tensor(rv).detach().cpu().double() + eps)).float()
    return torch.stack([rm, inv])[None].repeat(F, 1, 1).contiguous()


def mean_inv_from_frames(y, eps):
    """y (F,n,C) float64 -> mean_inv (F,2,C) float64 from each frame's own (biased) statistics."""
    mean = y.mean(dim=1)
    var = y.var(dim=1, unbiased=False)
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], dim=1)


def torch_fold(frames, rm, rv, eps, momentum):
    """The yardstick: ``torch.nn.BatchNorm2d(C, affine=False).double()`` on the CPU, fed the live frames (each (h,w,C) or None)
    one at a time in order, from the given buffers -> (running_mean, running_var, num_batches_tracked)."""
    C = rm.numel()
    bn = torch.nn.BatchNorm2d(C, eps=eps, momentum=momentum, affine=False).double()
    bn.running_mean.copy_(torch.as_tensor(rm).double())
    bn.running_var.copy_(torch.as_tensor(rv).double())
    bn.train()
    for y in frames:
        if y is not None:
            bn(y.double().permute(2, 0, 1)[None])
    return bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)


def ulp_distance(a, b):
    """Largest distance in units of the last place between two f32 tensors of the same sign pattern."""
    ia = np.asarray(a.detach().cpu().contiguous().numpy()).view(np.int32).astype(np.int64)
    ib = np.asarray(b.detach().cpu().contiguous().numpy()).view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max())
