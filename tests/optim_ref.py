"""Float64 restatement of the fused AdamW's contract (include/mvx_hip.h, "Fused AdamW") in plain numpy: scale by the sample
count, global gradient norm, clip coefficient, skip on a non-finite gradient, decoupled weight decay, moments, bias correction.
Written from the formulas, not from the kernel."""
import numpy as np


class RefAdamW:
    """State: lists of float64 arrays p, m, v (one per parameter), step count t, skipped count."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-2, max_norm=0.0, guard=True):
        self.p = [np.asarray(p, dtype=np.float64).copy() for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.lr, self.betas, self.eps, self.wd = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.max_norm, self.guard = float(max_norm), bool(guard)
        self.t = 0
        self.skipped = 0
        self.norm = self.coef = 0.0

    def step(self, grads, count=None, lr=None):
        lr = self.lr if lr is None else float(lr)
        g = [np.asarray(x, dtype=np.float64) for x in grads]
        gscale = 1.0 if count is None else 1.0 / max(float(count), 1.0)
        with np.errstate(over='ignore', invalid='ignore'):
            self.norm = float(np.sqrt(sum(float((x * x).sum()) for x in g))) * gscale
        self.coef = min(1.0, self.max_norm / (self.norm + 1e-6)) if self.max_norm > 0 else 1.0
        bad = any(not np.isfinite(x).all() for x in g) or not np.isfinite(self.norm)
        if self.guard and bad:
            self.skipped += 1
            return False
        self.t += 1
        b1, b2 = self.betas
        step_size = lr / (1.0 - b1 ** self.t)
        bc2_sqrt = np.sqrt(1.0 - b2 ** self.t)
        for i, x in enumerate(g):
            x = x * (gscale * self.coef)
            self.p[i] *= 1.0 - lr * self.wd
            self.m[i] += (x - self.m[i]) * (1.0 - b1)
            self.v[i] = self.v[i] * b2 + (1.0 - b2) * x * x
            self.p[i] -= step_size * self.m[i] / (np.sqrt(self.v[i]) / bc2_sqrt + self.eps)
        return True


def max_dist(ref_arrays, arrays):
    """Largest absolute distance between float64 reference arrays and (f32) arrays of the same shapes."""
    return max(float(np.abs(r - np.asarray(a, dtype=np.float64)).max()) for r, a in zip(ref_arrays, arrays))
