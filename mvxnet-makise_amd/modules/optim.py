"""AdamW on the library's own kernels (csrc/optim.hip): one streaming pass over the flat gradient bucket of
modules/parallel.py per step, with global gradient-norm clipping and a guard against non-finite gradients that runs on the
device -- a step whose gradient holds an inf or a NaN changes nothing and is counted, without a host read.  Checkpoints have
torch.optim.AdamW's format, so ``epoch{n}_opt.pkl`` files go both ways between the two optimizers.

    opt = optim.AdamW(params, lr=1e-3, max_norm=10.0)         # or bucket=GradBucket(...): the gradients ARE the bucket
    opt.zero_grad(); loss.backward(); opt.step(lr=optim.lr_at(k, 1e-3, 'cosine', warmup, total))
"""
import math

import numpy as np
import torch

CHUNK = 4096          # MVX_OPTIM_CHUNK of include/mvx_hip.h: elements per workgroup of the update kernel


def lr_at(k, base, schedule, warmup, total, lr_min=0.0):
    """Learning rate of the k-th ``step()`` call (k counts host calls from 0, skipped steps included, like torch's
    schedulers).  'constant': base.  'cosine': linear warm-up base * (k + 1) / warmup over the first ``warmup`` calls, then
    half a cosine from base down to lr_min at ``total``."""
    if schedule == 'constant':
        return float(base)
    if schedule != 'cosine':
        raise ValueError('unknown learning-rate schedule %r (constant | cosine)' % (schedule,))
    if k < warmup:
        return base * (k + 1) / warmup
    return lr_min + 0.5 * (base - lr_min) * (1.0 + math.cos(math.pi * (k - warmup) / max(1, total - warmup)))


def bucket_order(params, late=()):
    """The trainable parameters in the order of GradBucket's buffer: early ones first, then the ``late`` ones."""
    late_ids = {id(p) for p in late}
    ps = [p for p in params if p.requires_grad]
    return [p for p in ps if id(p) not in late_ids] + [p for p in ps if id(p) in late_ids]


def chunk_table(params, late=(), chunk=CHUNK):
    """Chunk table of the update kernel as an int64 array (n_chunks, 3): {address of the chunk's first element in its
    parameter, offset of that element in the flat bucket layout, element count <= chunk}.  Parameters are cut separately, so
    a chunk never straddles two of them.  Pure host code."""
    rows, off = [], 0
    for p in bucket_order(params, late):
        base, n = p.data_ptr(), p.numel()
        for s in range(0, n, chunk):
            rows.append((base + 4 * s, off + s, min(chunk, n - s)))
        off += n
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3)


class AdamW:
    """torch.optim.AdamW's update (decoupled weight decay, bias correction) as one library call per step.

    ``bucket``: the ``parallel.GradBucket`` that already holds the parameters' gradients, or None to make one (every
    parameter's ``.grad`` then becomes a view of its flat buffer).  ``max_norm`` > 0 clips the global gradient norm like
    ``torch.nn.utils.clip_grad_norm_``; ``guard`` skips a step with a non-finite gradient on the device (parameters, moments
    and the step count stay as they are; ``skipped_steps()`` counts it).  With ``guard=False`` a non-finite gradient goes into
    the weights as it does with torch.  ``exp_avg`` / ``exp_avg_sq`` are flat buffers in the bucket's layout."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=None, weight_decay=1e-2, max_norm=0.0, guard=True, bucket=None,
                 amsgrad=False, maximize=False):
        from modules import parallel
        if amsgrad or maximize:
            raise ValueError('optim.AdamW supports neither amsgrad nor maximize')
        if eps is None:
            import modules.config as cfg
            eps = cfg.eps
        self.all_params = list(params)
        self.params = [p for p in self.all_params if p.requires_grad]
        if not self.params:
            raise ValueError('optim.AdamW got no trainable parameter')
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_contiguous() or not p.is_cuda:
                raise ValueError('optim.AdamW needs contiguous float32 parameters on the GPU')
        if bucket is None:
            bucket = parallel.GradBucket(self.params)
        elif {id(p) for p in bucket.params} != {id(p) for p in self.params} or len(bucket.params) != len(self.params):
            raise ValueError('the GradBucket does not hold exactly the trainable parameters given to the optimizer')
        self.bucket = bucket
        self.max_norm, self.guard = float(max_norm), bool(guard)
        self.param_groups = [{'params': self.all_params, 'lr': lr, 'betas': tuple(betas), 'eps': eps, 'weight_decay': weight_decay,
                              'amsgrad': False, 'maximize': False, 'foreach': None, 'capturable': False, 'differentiable': False,
                              'fused': None, 'decoupled_weight_decay': True}]
        dev = bucket.flat.device
        n = bucket.flat.numel()
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self._state = torch.zeros(8, dtype=torch.float64, device=dev)      # [t, skipped, norm, coef, skip flag, ...]
        self._offsets, off = {}, 0
        for p in bucket.params:
            self._offsets[id(p)] = off
            off += p.numel()
        self._ptrs = [p.data_ptr() for p in bucket.params]
        self._table = torch.from_numpy(chunk_table(bucket.params)).to(dev)      # built once, lives on the device

    # ---- the step ------------------------------------------------------------------------------------------------
    def zero_grad(self, set_to_none=False):
        if set_to_none:
            raise ValueError('the gradients are views of the GradBucket: they are zeroed, never dropped')
        self.bucket.zero()

    def step(self, lr=None, count=None):
        """One update on the current stream; ``lr``: the value for this call (default: ``param_groups[0]['lr']``).
        ``count``: a one-element f32 device tensor, e.g. ``bucket.count_slot()`` after ``all_reduce_mean(frames_local=,
        divide=False)``: the gradient is scaled by 1 / max(count, 1) inside the update (read on the device)."""
        from modules import _hip
        self.bucket.check_views()
        if [p.data_ptr() for p in self.bucket.params] != self._ptrs:
            raise RuntimeError('a parameter moved after the optimizer was built (model.to(), a new .data): rebuild optim.AdamW')
        g = self.param_groups[0]
        _hip.optim_adamw_step(self._table, self.bucket.flat, self.exp_avg, self.exp_avg_sq, count, self._state,
                              g['lr'] if lr is None else lr, g['betas'][0], g['betas'][1], g['eps'], g['weight_decay'],
                              self.max_norm, self.guard)
        # the kernel wrote the weights behind torch's back: the packed-weight caches key on (_version, data_ptr)
        torch.autograd.graph.increment_version(self.bucket.params)

    # ---- diagnostics: one host read each, on demand ------------------------------------------------------------------
    def _read(self, k):
        return float(self._state.cpu()[k])

    def diagnostics(self):
        """{'step', 'skipped', 'norm', 'coef'} of the state block with ONE host read."""
        st = self._state.cpu().tolist()
        return {'step': int(st[0]), 'skipped': int(st[1]), 'norm': st[2], 'coef': st[3]}

    def steps(self):
        return int(self._read(0))

    def skipped_steps(self):
        return int(self._read(1))

    def last_norm(self):
        return self._read(2)

    def last_coef(self):
        return self._read(3)

    # ---- checkpoints in torch.optim.AdamW's format -----------------------------------------------------------------
    def _slice(self, flat, p):
        off = self._offsets[id(p)]
        return flat[off:off + p.numel()].view_as(p)

    def moments(self, p):
        """(exp_avg, exp_avg_sq) of parameter ``p`` as views of the flat buffers, in the parameter's shape."""
        return self._slice(self.exp_avg, p), self._slice(self.exp_avg_sq, p)

    def state_dict(self):
        t = self._read(0)
        state = {}
        for i, p in enumerate(self.all_params):
            if p.requires_grad and t > 0:
                state[i] = {'step': torch.tensor(t, dtype=torch.float32), 'exp_avg': self._slice(self.exp_avg, p).clone(),
                            'exp_avg_sq': self._slice(self.exp_avg_sq, p).clone()}
        group = {k: v for k, v in self.param_groups[0].items() if k != 'params'}
        group['params'] = list(range(len(self.all_params)))
        return {'state': state, 'param_groups': [group]}

    def load_state_dict(self, sd):
        groups = sd['param_groups']
        if len(groups) != 1 or len(groups[0]['params']) != len(self.all_params):
            raise ValueError('optim.AdamW holds one parameter group of %d parameters' % len(self.all_params))
        if groups[0].get('amsgrad') or groups[0].get('maximize'):
            raise ValueError('optim.AdamW supports neither amsgrad nor maximize')
        index_of = {key: i for i, key in enumerate(groups[0]['params'])}
        steps = set()
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        for key, st in sd['state'].items():
            p = self.all_params[index_of[key]]
            if not p.requires_grad:
                continue
            if tuple(st['exp_avg'].shape) != tuple(p.shape):
                raise ValueError('optimizer state %r has shape %s, the parameter %s' % (key, tuple(st['exp_avg'].shape), tuple(p.shape)))
            self._slice(self.exp_avg, p).copy_(st['exp_avg'])
            self._slice(self.exp_avg_sq, p).copy_(st['exp_avg_sq'])
            steps.add(float(st['step']))
        if len(steps) > 1:
            raise ValueError('optim.AdamW keeps ONE step count; the checkpoint holds %s' % sorted(steps))
        if steps and len(sd['state']) < len(self.params):
            raise ValueError('the checkpoint has optimizer state for only %d of %d parameters' % (len(sd['state']), len(self.params)))
        for k in ('lr', 'betas', 'eps', 'weight_decay'):
            if k in groups[0]:
                self.param_groups[0][k] = tuple(groups[0][k]) if k == 'betas' else groups[0][k]
        host = self._state.cpu()
        host[0] = steps.pop() if steps else 0.0
        self._state.copy_(host)
