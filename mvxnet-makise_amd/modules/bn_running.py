"""``bntrack``: running BatchNorm statistics on the frame-set path (config.yml:20; the reference passes the switch to every
``nn.BatchNorm*d(track_running_stats=cfg.bntrack)``, Blocks.py:10,25).

Every BatchNorm site of modules/frames.py and modules/rpn_frames.py hands its consumer one tensor, mean_inv f32 (F,2,C).  A
step function opens ``step(model)``; each site then passes through ``site(bn, mean_inv, kind, rows)``:

  * training (``model.training``): the site is recorded and ``StepSites.update`` folds all of them into the modules' buffers
    with ONE launch behind the forward (csrc/bn_running.hip) -- F sequential PyTorch updates in frame order, because the
    reference runs batch 1.  The arithmetic of the step is untouched;
  * eval: ``StepSites.fill`` writes (running_mean, 1/sqrt(running_var + eps)) for every BatchNorm module of the model with ONE
    launch before the first layer, and ``site`` hands that tensor out in place of the batch statistics.

With ``bntrack`` off nothing here runs: ``current()`` is None and the sites keep the tensors they computed.
"""
import torch
from torch.nn.modules.batchnorm import _BatchNorm

import modules.config as cfg
from modules import _hip
from modules import Extension as X

# The StepSites of the frame-set step being enqueued.  ONE per process: the step functions enqueue from a single thread, and a
# frame-set forward started from another Python thread while a step is open would register its sites here.  The loader thread
# of modules/data/Prefetch.py prepares inputs only (no BatchNorm site), so it never does.
_STEP = None


def current():
    """The step's site list when ``bntrack`` is on (None when it is off).  A frame-set forward outside a step function -- the
    per-frame autograd paths run the same kernels one frame at a time -- is refused."""
    if not cfg.config.get('bntrack', False):
        return None
    if _STEP is None:
        _hip.require_plain_batchnorm('a forward outside the frame-set step functions (MVXNet.forward, modules/whole.py, modules/tape.py)')
    return _STEP


def site(bn, mi, kind, rows):
    """BatchNorm site ``bn`` of the step: ``mi`` (F,2,C) as the layer computed it (None in an eval forward), the layout of its
    row matrix (X.ROWS_*) and its row count over all frames.  Returns the mean_inv the consumers read."""
    st = current()
    return mi if st is None else st.site(bn, mi, kind, rows)


def eval_mode():
    """Does the step being enqueued normalise with the running statistics?"""
    st = current()
    return st is not None and st.eval


_BUFFERS = ('.running_mean', '.running_var', '.num_batches_tracked')
_FROZEN = 'head.extractor.'      # the frozen image extractor keeps BatchNorm buffers of its own in every checkpoint that carries it


def _own_buffer(key):
    """Is ``key`` a running buffer of one of the model's OWN BatchNorm modules?  The frozen extractor's subtree
    (``head.extractor.backbone.body.bn1.running_mean`` ...: imhead/Extractor.py) says nothing about ``bntrack``."""
    return key.endswith(_BUFFERS) and not key.startswith(_FROZEN)


def checkpoint_tracks(state):
    """Does a state dict hold running statistics of the model's own BatchNorm modules (a model trained with ``bntrack``)?"""
    return state is not None and any(k.endswith('.running_mean') and _own_buffer(k) for k in state)


def strip_running(state):
    """The state dict without the running buffers of the model's own BatchNorm modules: what an untracked model loads.  The
    frozen extractor's tensors stay."""
    return {k: v for k, v in state.items() if not _own_buffer(k)}


def load_state(model, state):
    """``model.load_state_dict(state)`` for a tracked model that may be resumed from a checkpoint written without running
    statistics: the buffers then stay at their initial 0 / 1.  Returns True when that happened; every other mismatch raises as
    ever."""
    if not _hip.bn_tracking() or checkpoint_tracks(state):
        model.load_state_dict(state)
        return False
    res = model.load_state_dict(state, strict=False)
    odd = [k for k in res.missing_keys if not _own_buffer(k)] + list(res.unexpected_keys)
    if odd:
        raise RuntimeError('state dict does not fit the model beyond the running BatchNorm buffers: %s' % odd[:8])
    return True


def set_momentum(model, momentum):
    """``bn.momentum`` of every BatchNorm module (torch's default 0.1); None, the cumulative average, is not supported."""
    if momentum is None or not 0.0 <= float(momentum) <= 1.0:
        raise X.MvxHipError('BatchNorm momentum must lie in 0..1 (None, the cumulative average, is not supported)')
    for m in model.modules():
        if isinstance(m, _BatchNorm):
            m.momentum = float(momentum)


class StepSites:
    def __init__(self, training):
        self.eval = not training
        self.sites = []             # (BatchNorm module, mean_inv, row kind, rows)
        self.filled = None          # eval: id(module) -> mean_inv (F,2,C) from the buffers
        self.table = None

    def site(self, bn, mi, kind, rows):
        if self.eval:
            mi = self.filled[id(bn)]
        self.sites.append((bn, mi, kind, int(rows)))
        return mi

    def _table(self, entries):
        # the table holds addresses: the tensors stay referenced by this object until the step function returns
        self.table = _hip.bn_site_table([(mi, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, kind, rows)
                                         for bn, mi, kind, rows in entries])
        return self.table

    def fill(self, model, F):
        """Eval: mean_inv of EVERY BatchNorm module of ``model`` from its buffers, for F frames, in one launch."""
        bns = [m for m in model.modules() if isinstance(m, _BatchNorm)]
        dev = bns[0].running_mean.device
        flat = torch.empty((sum(F * 2 * m.num_features for m in bns),), dtype=torch.float32, device=dev)
        self.filled, off = {}, 0
        for m in bns:
            n = F * 2 * m.num_features
            self.filled[id(m)] = flat[off:off + n].view(F, 2, m.num_features)
            off += n
        _hip.bn_running_mean_inv_sites(self._table([(m, self.filled[id(m)], X.ROWS_GRID, 0) for m in bns]), F, cfg.eps)

    def update(self, F, desc=None):
        """Training: fold the recorded sites into their modules' buffers, one launch on the current stream."""
        _hip.bn_running_update_sites(self._table(self.sites), F, cfg.eps, desc)

    def records(self, F, desc=None):
        """Tests: per recorded site (module, mean_inv, per-frame populations as the fold takes them)."""
        out = []
        for bn, mi, kind, rows in self.sites:
            if kind == X.ROWS_GRID:
                pop = [rows // F] * F
            else:
                pop = [(desc.vox_off[f + 1] - desc.vox_off[f]) * desc.t for f in range(F)]
            out.append((bn, mi, pop))
        return out


class step:
    """``with step(model) as st``: the frame-set forward enclosed registers its BatchNorm sites in ``st`` (None with ``bntrack``
    off).  ``train_entry``: the entry point is a training step, refused on an eval model."""

    def __init__(self, model, train_entry=True):
        self.st = None
        if _hip.bn_tracking():
            if train_entry and not model.training:
                raise X.MvxHipError('bntrack: a training step on a model in eval mode (model.train() first; detect.detect_frame_set '
                                    'is the eval forward)')
            self.st = StepSites(model.training)

    def __enter__(self):
        global _STEP
        self.old, _STEP = _STEP, self.st
        return self.st

    def __exit__(self, *exc):
        global _STEP
        _STEP = self.old
        return False
