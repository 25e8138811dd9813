"""Typed torch-tensor wrappers over the C ABI (plumbing only: allocation, pointers, stream)."""
import collections
import ctypes
import math
import os

import torch

from modules import Extension as X

VoxelizeResult = collections.namedtuple('VoxelizeResult', 'voxels coords counts n_voxels status')

_ws_cache = {}
STATS_REPLICAS = 32      # MVX_STATS_REPLICAS of include/mvx_hip.h
FLAG_RELU, FLAG_PREZEROED, FLAG_ACCUMULATE, FLAG_CONV2D = 1, 2, 4, 8      # MVX_FLAG_* of include/mvx_hip.h
FLAG_SPLIT = 64                                                          # MVX_FLAG_SPLIT: bf16x3 arithmetic of the wide row GEMMs
FLAG_SPLIT3 = 128                                                        # MVX_FLAG_SPLIT3: three bf16 pieces per operand (bf16x6, fp32-grade)
FLAG_AMAX_COARSE = 1024                                                  # MVX_FLAG_AMAX_COARSE: the bound x is a foreign forward input (8-binade scale steps)
FLAG_NO_BG_FILL = 2048                                                   # MVX_FLAG_NO_BG_FILL: voxel-free tiles of the sparse conv1 output are not written
FLAG_SPLIT_F16 = 512                                                     # MVX_FLAG_SPLIT_F16: two fp16 pieces per operand (fp16x3)


def split_flags(split, row=False):
    """``split``: 0 / False = exact-f32 MFMA, 2 / True = bf16x3, 3 = bf16x6 -> the flag bits of a call (row GEMMs also need
    MVX_FLAG_SPLIT, and so do the convolution weight gradients, which run behind the f32 entry points; the *_split
    convolution entry points -- forward, input gradient, weight packing -- only look at MVX_FLAG_SPLIT3 / MVX_FLAG_SPLIT_F16)."""
    if not split:
        return 0
    return (FLAG_SPLIT if row else 0) | (FLAG_SPLIT3 if int(split) == 3 else 0) | (FLAG_SPLIT_F16 if int(split) == 4 else 0)


def amax_of(t):
    """The 1-element float32 tensor holding max |t| that a producer kernel wrote (``tag_amax``), or None."""
    return getattr(t, '_mvx_amax', None)


def tag_amax(t, amax):
    """Attach the device-side max |t| (1-element float32 tensor, kept alive by the attribute) to ``t``: the fp16x3 kernels scale
    the operand by it (include/mvx_hip.h: mvx_split_operand_amax).  A ``.view()`` of t does not carry the tag: re-tag it."""
    if t is not None and amax is not None:
        t._mvx_amax = amax
    return t


def new_amax(device):
    """A 1-element float32 tensor for a producer kernel to write max |dz| into.  Its OWN allocation, not a slot of the
    accumulator arena: side-stream weight-gradient kernels read it after the arena of their lane has been cleared for the next
    frame."""
    return torch.empty((1,), dtype=torch.float32, device=device)


def tensor_amax(t):
    """Measure max |t| on the device (one pass over t) and tag t with it."""
    am = torch.empty((1,), dtype=torch.float32, device=t.device)
    X.call('mvx_tensor_amax', t, t.numel(), am, 0)
    return tag_amax(t, am)


def bind_amax(split, a=None, b=None):
    """fp16x3 (split code 4): bind the operand ranges of the NEXT split launch to the tags of tensors a / b (untagged: not
    scaled).  The entry point that follows consumes the binding."""
    if split and int(split) == 4:
        X.lib.mvx_split_operand_amax(X.ptr(amax_of(a)) if a is not None else None, X.ptr(amax_of(b)) if b is not None else None)


def foreign_split(split, x=None):
    """Arithmetic of a FORWARD row GEMM whose input was not produced by this library (sampled image features, the input of a
    stand-alone FCN).  fp16x3 needs the input's range there, and a scale taken over whatever tensor the executor happens to
    hold (one frame, a frame set) makes two executors round differently -- enough to flip ReLUs between them
    (tools/dbg_fp16_seeds.py: 3e-2 on 4 of 6 seeds).  So: a foreign input WITH a range tag runs fp16x3 with the COARSE scale
    (MVX_FLAG_AMAX_COARSE: 8-binade steps, the same for a frame and its set unless their maxima straddle a step); one without a
    tag runs bf16x6, which has the range of f32.  Returns (split code, extra flags)."""
    if split and int(split) == 4:
        return (4, FLAG_AMAX_COARSE) if (x is not None and amax_of(x) is not None) else (3, 0)
    return split, 0


class foreign_input_math:
    """Scope of ONE stand-alone block call (CRB3d / CRB2d / DeCRB2d through the nn.Module interface) on a tensor this library
    did not produce: under ``convmath: fp16x3`` the block runs in bf16x6 -- an input of unknown range has no place in fp16's
    five exponent bits (1e-3-sized inputs would keep ~15 bits, 1e5-sized ones overflow, and the BatchNorm behind the
    convolution would hide both), bf16 pieces have the range of f32.  Tensors produced by this library's blocks
    (outputs of a BatchNorm: bounded by sqrt(N)) carry ``_mvx_lib`` and keep fp16x3.  ``math``: re-enter the arithmetic a
    forward call chose (its backward)."""

    def __init__(self, x=None, math=None):
        self.x, self.math, self.old = x, math, None

    def __enter__(self):
        import modules.config as cfg
        cur = cfg.config.get('convmath', 'f32')
        want = self.math
        if want is None:
            want = 'bf16x6' if (cur == 'fp16x3' and not getattr(self.x, '_mvx_lib', False)) else cur
        if want != cur:
            self.old, cfg.config['convmath'] = cur, want
        return want

    def __exit__(self, *exc):
        if self.old is not None:
            import modules.config as cfg
            cfg.config['convmath'] = self.old
        return False


def mark_lib(t):
    """``t`` is the output of one of this library's BatchNorms (see foreign_input_math)."""
    t._mvx_lib = True
    return t


# The 1 % mutation hooks of the gradient tests (frames._MUTATE, rpn_frames._MUTATE) only act in a process started with
# MVX_ALLOW_MUTATION=1 (tests/conftest.py sets it): a product run cannot switch them on by accident.
MUTATION_ALLOWED = os.environ.get('MVX_ALLOW_MUTATION') == '1'


def mutate(table, name, t):
    """``t * table[name]`` when the test hook names this term (and keeps t's range tag, scaled: the mutated tensor then takes
    the same arithmetic path -- fp16x3 with its amax -- as the unmutated one); ``t`` otherwise."""
    f = table.get(name)
    if f is None or t is None:
        return t
    if not MUTATION_ALLOWED:
        raise X.MvxHipError('gradient mutation hooks are test-only: start the process with MVX_ALLOW_MUTATION=1')
    t2 = t * f
    am = amax_of(t)
    if am is not None:
        tag_amax(t2, am * abs(float(f)))
    return t2


# ---- fp16x3: the weight-range guard.  Weights are cut times 2^8 (csrc/split_common.h), so a weight at or above 255.9 would
# overflow its high fp16 piece into inf -- silently, behind a BatchNorm that hides the scale.  Every weight
# tensor an fp16x3 kernel is about to read is checked ON THE DEVICE once per parameter version (a tiny kernel; no host read) into
# a per-device status word that joins the step's other status words (modules/frames.py) and is decoded by raise_on_status:
# the step that used such a weight is reported, loudly, at its status check.
STATUS_F16_WEIGHT_RANGE = 8
_W16_STATUS = {}


def fp16_weight_status(device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _W16_STATUS.get(idx)
    if st is None:
        st = _W16_STATUS[idx] = torch.zeros((1,), dtype=torch.int32, device=torch.device('cuda', idx))
    return st


def guard_fp16_weight(w):
    """Range check of a weight tensor for the fp16-piece arithmetic, once per version of the parameter it views."""
    base = w._base if w._base is not None else w
    seen = base.__dict__.setdefault('_mvx_w16', {})
    tag = (base._version, w.data_ptr())
    if seen.get(tuple(w.shape)) != tag:
        seen[tuple(w.shape)] = tag
        wc = w.detach()
        wc = wc if wc.is_contiguous() else wc.contiguous()
        X.call('mvx_split_f16_weight_check', wc, wc.numel(), fp16_weight_status(w.device))


def raise_on_status(word):
    """Decode the OR of a step's device status words (one host read by the caller)."""
    word = int(word)
    if word & STATUS_F16_WEIGHT_RANGE:
        raise X.MvxHipError('convmath fp16x3: a weight reached |w| >= 255.9 (or is not finite): its fp16 pieces overflow.  The results '
                            'of this step are invalid; use convmath bf16x6 (three bf16 pieces: the exponent range of f32)')
    if word & 1:
        raise AssertionError('projected point outside the feature map (imhead/Pipe.py:71)')
    if word:
        raise X.MvxHipError('a kernel reported a data-dependent error (status %d)' % word)


def grad_split(split, dz):
    """Arithmetic of a row GEMM whose operand ``dz`` is a gradient: fp16x3 needs its range (a tag), else bf16x6 stands in (the
    row kernels split both operands in the kernel, so any arithmetic can run any call)."""
    if split and int(split) == 4 and amax_of(dz) is None:
        return 3
    return split


def split_pieces():
    """convmath of config.yml -> 0 (f32: exact-f32 MFMA), 2 (bf16x3) or 3 (bf16x6)."""
    import modules.config as cfg
    m = cfg.config.get('convmath', 'f32')
    if m not in ('f32', 'bf16x3', 'bf16x6', 'fp16x3'):
        raise X.MvxHipError('convmath must be f32, bf16x3, bf16x6 or fp16x3, not %r' % (m,))
    return {'f32': 0, 'bf16x3': 2, 'bf16x6': 3, 'fp16x3': 4}[m]
FLAG_BG_TAPS = 32

# When True, the backward of the hot-path layers adds weight / bias gradients straight into the existing
# ``.grad`` buffers inside the reduction kernels (and returns None to autograd), instead of producing a
# temporary that autograd adds afterwards.  Set by the training pipeline (modules/pipeline.py).
GRAD_SINK = False


# When True (and gradients go straight into .grad, see GRAD_SINK), weight-gradient kernels are enqueued
# on a second HIP stream: their results are only needed at the optimizer step, so they overlap with the
# rest of the backward pass (their MFMA work fills the CUs while BatchNorm / gather kernels wait on HBM).
ASYNC_WGRAD = False
_SIDE = {}


def side_stream(device):
    st = _SIDE.get(device.index)
    if st is None:
        st = torch.cuda.Stream(device=device, priority=0)
        _SIDE[device.index] = st
    return st


_KEEP = {}          # device index -> tensors read by side-stream kernels since the last join
_COMM = {}
_TAIL = {}          # device index -> [event on the side stream before the step's last weight gradient, event at the end of the main stream's backward]


def comm_stream(device):
    """Stream of the data-parallel exchange (modules/parallel.py: the early part of the gradient bucket goes out on it while
    the step's last weight gradient is still running)."""
    st = _COMM.get(device.index)
    if st is None:
        st = _COMM[device.index] = torch.cuda.Stream(device)
    return st


def mark_tail(device):
    """Called by the backward right BEFORE it enqueues the step's last weight-gradient kernel on the side stream: every other
    parameter gradient of the side stream is complete when this event fires."""
    if device.index in _SIDE:
        ev = torch.cuda.Event()
        ev.record(_SIDE[device.index])
        _TAIL[device.index] = [ev, None]


def tail_events(device):
    """The pair of the step that has just been enqueued, consumed by the caller (None: no tail was marked)."""
    t = _TAIL.pop(device.index, None)
    return tuple(t) if t is not None and t[1] is not None else None


def drop_tail(device=None):
    """Forget the tail pair: a gradient has been (or will be) written on the main stream AFTER join_side_stream recorded the end
    of the backward -- lane gradients added into the bucket, autograd's AccumulateGrad of returned views -- so the early part
    of the exchange must wait for the whole main stream (parallel.py falls back to ``comm.wait_stream(main)``)."""
    if device is None:
        _TAIL.clear()
    else:
        _TAIL.pop(device.index, None)


def join_side_stream(device=None):
    """Make the current stream wait for every weight-gradient kernel enqueued on the side stream."""
    for idx, st in _SIDE.items():
        if device is None or device.index == idx:
            cur = torch.cuda.current_stream(st.device)
            t = _TAIL.get(idx)
            if t is not None:
                if t[1] is None:                    # the main stream's own gradient work ends here (before it waits for the tail)
                    ev = torch.cuda.Event()
                    ev.record(cur)
                    t[1] = ev
                else:                               # a mark of an earlier join: stale
                    del _TAIL[idx]
            cur.wait_stream(st)
            keep = _KEEP.pop(idx, None)             # dropped AFTER the wait has been enqueued (see _SideStream)
            del keep


class _SideStream:
    """Run the enclosed launches on the side stream, ordered after everything already enqueued on the
    current stream; the tensors they read are kept alive until the owning stream joins the side stream."""

    def __init__(self, *tensors):
        self.tensors = [t for t in tensors if t is not None]
        # the side-stream kernels also read the range tags of their operands (fp16x3: amax_of): separate allocations
        self.tensors += [a for a in (amax_of(t) for t in self.tensors) if a is not None]

    def __enter__(self):
        dev = self.tensors[0].device
        self.side = side_stream(dev)
        self.side.wait_stream(torch.cuda.current_stream(dev))
        # keep the tensors alive until the owning stream has JOINED the side stream (join_side_stream drops the list after
        # its wait): their blocks then return to the owning stream's pool in stream order.  record_stream instead parks a
        # block until an event of the side stream has been seen to complete, which is timing dependent: the hot loop held
        # 40 GB reserved for 8 GB allocated and its peak crept 6.6 % over 1,500 identical steps (profiles/r03_soak.txt)
        _KEEP.setdefault(dev.index, []).extend(self.tensors)
        self.ctx = torch.cuda.stream(self.side)
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc)


class _Inline:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _wgrad_scope(accumulate_into, *tensors):
    if ASYNC_WGRAD and accumulate_into is not None:
        return _SideStream(*tensors)
    return _Inline()


class ZeroArena:
    """One f64 buffer cleared with ONE fill per frame, from which every BatchNorm accumulator of the
    frame is carved (the C entry points then skip their own memsets: MVX_FLAG_PREZEROED)."""

    def __init__(self, device, doubles=1 << 19):
        self.buf = torch.empty((doubles,), dtype=torch.float64, device=device)
        self.off = doubles                 # exhausted until begin()

    def begin(self):
        self.buf.zero_()
        self.off = 0

    def take(self, n):
        n_al = (n + 31) & ~31
        if self.off + n_al > self.buf.numel():
            return None
        view = self.buf[self.off:self.off + n]
        self.off += n_al
        return view


_ARENAS = {}          # one arena per (device, stream): frames in flight on different streams never share one
_ARENA_ON = False


def _arena_key(device):
    return (device.index, X.raw_stream(device.index))


def arena_begin(device, doubles=1 << 19):
    """Start a frame (or a frame set) on the current stream: clear its accumulator arena (created on first use; grown
    when a larger one is asked for)."""
    global _ARENA_ON
    key = _arena_key(device)
    if key not in _ARENAS or _ARENAS[key].buf.numel() < doubles:
        with torch.cuda.device(device):
            _ARENAS[key] = ZeroArena(device, doubles)
    _ARENAS[key].begin()
    _ARENA_ON = True


def arena_end():
    global _ARENA_ON
    _ARENA_ON = False
    for a in _ARENAS.values():
        a.off = a.buf.numel()


def _acc_f64(shape, device):
    """(accumulator tensor, flag): carved from the frame arena (pre-zeroed) or freshly allocated."""
    n = 1
    for d in shape:
        n *= int(d)
    if _ARENA_ON:
        a = _ARENAS.get(_arena_key(device))
        if a is not None:
            v = a.take(n)
            if v is not None:
                return v.view(shape), FLAG_PREZEROED
    return torch.empty(shape, dtype=torch.float64, device=device), 0

# Optional live kernel timing (bench.py): name -> list of (start_event, end_event, algorithmic_flops).
# Events are recorded on the current stream, the stream every kernel of this library is launched on.
KERNEL_TIMERS = None


_EVENT_POOL = []          # timing events are recycled: creating one costs tens of microseconds of host time


def _timing_event():
    return _EVENT_POOL.pop() if _EVENT_POOL else torch.cuda.Event(enable_timing=True)


def recycle_timing_events(timers):
    """Hand the events of a finished (and read) KERNEL_TIMERS dict back to the pool."""
    for evs in timers.values():
        for s_, e_, _ in evs:
            _EVENT_POOL.append(s_)
            _EVENT_POOL.append(e_)


_STREAM_OBJS = {}


def _current_stream_obj():
    """torch.cuda.current_stream() without its ~10 us of Python per call (Event.record() without a stream argument pays it
    too): the Stream object of the current raw stream, looked up once per (device, raw stream)."""
    idx = torch.cuda.current_device()
    key = (idx, X.raw_stream(idx))
    st = _STREAM_OBJS.get(key)
    if st is None:
        st = torch.cuda.current_stream()
        _STREAM_OBJS[key] = st
    return st


TIMER_NAMES = None     # bench.py: with KERNEL_TIMERS on, only these timer names record events (None = all).  Two event records per
                       # library call are ~180 markers in a hot step: 0.5 ms of an 8.2 ms step (tools/soak_plain.py runs 7.65)


class _Timed:
    def __init__(self, name, flops):
        self.name, self.flops = name, flops

    def __enter__(self):
        self.on = KERNEL_TIMERS is not None and (TIMER_NAMES is None or self.name in TIMER_NAMES)
        if self.on:
            self.s = _timing_event()
            self.e = _timing_event()
            self.s.record(_current_stream_obj())
        return self

    def __exit__(self, *exc):
        if self.on and KERNEL_TIMERS is not None:
            self.e.record(_current_stream_obj())
            KERNEL_TIMERS.setdefault(self.name, []).append((self.s, self.e, self.flops))
        return False


def _timed_bytes(name, nbytes):
    """Timer for an HBM-bound stage: the third tuple field carries ALGORITHMIC bytes (negative marks bytes)."""
    if KERNEL_TIMERS is None:
        return _Timed('hbm:' + name, 0)
    # a data-dependent byte count (e.g. bytes of the flagged tiles) is passed as a zero-argument CALLABLE that the
    # consumer of the timers evaluates after the run (timer_value): neither a host read nor an extra launch inside the step
    return _Timed('hbm:' + name, nbytes if (callable(nbytes) or isinstance(nbytes, torch.Tensor)) else float(nbytes))


def timer_value(v):
    """The FLOP / byte figure of a timer entry as a float: numbers as they are, device scalars read, callables evaluated
    (data-dependent counts are deferred until after the timed region)."""
    if callable(v):
        v = v()
    return float(v)


def require_no_bnaffine():
    """The kernels normalise without affine parameters -- the reference's configuration (config.yml:19: bnaffine False;
    Blocks.py:10,25).  With them switched on, bn.weight / bn.bias would enter the optimizer with permanently zero gradients,
    silently: refuse instead.  (``bntrack`` is honoured on the frame-set path: modules/bn_running.py.)"""
    import modules.config as cfg
    if bool(cfg.config.get('bnaffine', False)):
        raise X.MvxHipError('bnaffine is not supported by the HIP BatchNorm kernels (no affine parameters: the reference\'s '
                            'config.yml:19); set it to False')


def bn_tracking():
    """config.yml ``bntrack``: the BatchNorm modules carry running statistics (nn.BatchNorm*d(track_running_stats=True))."""
    import modules.config as cfg
    return bool(cfg.config.get('bntrack', False))


def require_plain_batchnorm(what='this path'):
    """The per-frame autograd paths (MVXNet.forward, modules/tape.py, modules/whole.py, the stand-alone blocks) normalise with
    the batch statistics only and never touch a running buffer: with ``bntrack`` the buffers would not move in training and
    would not be read in eval, silently: refuse instead and name the path that honours it."""
    require_no_bnaffine()
    if bn_tracking():
        raise X.MvxHipError('bntrack: %s normalises with batch statistics only; running statistics are kept and read on the '
                            'frame-set path (pipeline.train_step_full / train_step_frame_set / train_step_rows_only, '
                            'detect.detect_frame_set; train_like.py --mode fast)' % what)


# ---------------------------------------------------------------------------------------------
# Running BatchNorm statistics of a step's sites (csrc/bn_running.hip; modules/bn_running.py)
# ---------------------------------------------------------------------------------------------
def bn_site_table(sites):
    """The host table of mvx_bn_site_t from ``(mean_inv (F,2,C), running_mean (C,), running_var (C,), num_batches_tracked i64
    (), momentum, row kind, rows)`` per site.  The tensors must outlive the launches that read the table."""
    table = (X.BnSite * len(sites))()
    for k, (mi, rm, rv, nbt, momentum, kind, rows) in enumerate(sites):
        C = rm.numel()
        if momentum is None:
            raise X.MvxHipError('BatchNorm momentum None (the cumulative average) is not supported by the running-statistics fold')
        if not (mi.dtype == rm.dtype == rv.dtype == torch.float32 and nbt.dtype == torch.int64 and mi.dim() == 3 and
                mi.shape[1:] == (2, C) and rv.numel() == C and nbt.numel() == 1 and mi.is_cuda and rm.is_cuda and rv.is_cuda and
                nbt.is_cuda and mi.is_contiguous() and rm.is_contiguous() and rv.is_contiguous()):
            raise X.MvxHipError('a BatchNorm site needs mean_inv f32 (F,2,C) and the f32 / i64 running buffers of C channels, '
                                'contiguous on the device')
        s = table[k]
        s.mean_inv, s.running_mean, s.running_var, s.num_batches_tracked = mi.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr()
        s.rows, s.momentum, s.channels, s.row_kind = int(rows), float(momentum), C, int(kind)
    return table


def bn_running_update_sites(table, F, eps, desc=None, live_mask=None):
    """Fold every site's per-frame (mean, inverse deviation) into its running buffers, frame after frame, in one launch
    (mvx_bn_running_update_sites).  ``desc``: the frame set's descriptor (the row layouts take their populations from it);
    ``live_mask``: bit f clear = frame f folds nothing (default: every frame)."""
    mask = (1 << F) - 1 if live_mask is None else int(live_mask)
    if len(table):
        X.call('mvx_bn_running_update_sites', table, len(table), _desc_ref(desc), F, mask, float(eps))


def bn_running_mean_inv_sites(table, F, eps):
    """Every site's mean_inv (F,2,C) = (running_mean, 1/sqrt(running_var + eps)) in one launch (mvx_bn_running_mean_inv_sites)."""
    if len(table):
        X.call('mvx_bn_running_mean_inv_sites', table, len(table), F, float(eps))


def conv_flops(d_out_planes, d_src_planes, H, W, cin, cout, sd, pd, dgrad=False):
    """Executed multiply-add FLOPs of one gather launch: depth taps that fall outside the source
    volume are skipped by the kernel and are NOT counted (in-plane zero padding is computed and
    is counted)."""
    taps = 0
    for d in range(d_out_planes):
        for kd in range(3):
            if not dgrad:
                s = d * sd - pd + kd
                taps += 0 <= s < d_src_planes
            else:
                t = d + pd - kd
                taps += t >= 0 and t % sd == 0 and t // sd < d_src_planes
    return 2.0 * taps * 9 * H * W * cin * cout


def _per_frame(F, *shape):
    """Shape of a per-frame quantity: ``F=None`` is ONE frame without the frame axis, an int a frame set with it in front."""
    return shape if F is None else (F,) + shape


def workspace(nbytes, dev, tag):
    """Grow-only scratch buffer per (device, tag); stream-ordered reuse on the current stream."""
    key = (dev.index, tag, X.raw_stream(dev.index))    # one buffer per (tag, stream): no cross-stream reuse
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
        _ws_cache[key] = buf
    return buf


def voxelize(pcd, perm, n_points, lo, size, T, out_channels, cap_voxels=None, ext_idx=None):
    """pcd f32 (F,capP,ncol) on the GPU; perm i32 (F,capP) or None; n_points i32 (F,) or None
    (= every frame full).  Returns capacity-sized outputs plus device-side counts."""
    assert pcd.dim() == 3 and pcd.dtype == torch.float32
    F, cap, ncol = pcd.shape
    assert 1 <= F <= 63, 'the voxelizer takes 1..63 frames per call (include/mvx_hip.h)'
    dev = pcd.device
    if n_points is None:
        n_points = torch.full((F,), cap, dtype=torch.int32, device=dev)
    cap_voxels = cap if cap_voxels is None else int(cap_voxels)
    voxels = torch.empty((F, cap_voxels, T, out_channels), dtype=torch.float32, device=dev)
    coords = torch.empty((F, cap_voxels, 4), dtype=torch.int64, device=dev)
    counts = torch.empty((F, cap_voxels), dtype=torch.int32, device=dev)
    n_vox = torch.empty((F,), dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    nbytes = X.lib.mvx_voxelize_workspace_bytes(F, cap)
    ws = workspace(nbytes, dev, 'voxelize')
    # algorithmic bytes: points + permutation read; the voxel payload is priced at ~V = P/4 voxels per frame
    with _timed_bytes('voxelize', F * cap * (ncol * 4 + 4) + F * (cap // 4) * (T * out_channels * 4 + 36)):
        rc = X.lib.mvx_voxelize(X.ptr(pcd), X.ptr(perm), X.ptr(n_points), X.ptr(ext_idx), F, cap, ncol,
                                float(lo[0]), float(lo[1]), float(lo[2]),
                                float(size[0]), float(size[1]), float(size[2]),
                                int(T), int(out_channels), cap_voxels,
                                X.ptr(voxels), X.ptr(coords), X.ptr(counts), X.ptr(n_vox), X.ptr(status),
                                X.ptr(ws), ws.numel(), X.stream())
    X.check(rc, 'mvx_voxelize')
    return VoxelizeResult(voxels, coords, counts, n_vox, status)


def voxelize_concat(pcd, perm, n_points, lo, size, T, out_channels):
    """The batch layout: voxels of all frames back to back.  Returns (voxels (F*cap,T,C), coords (F*cap,4) with the frame
    index in column 0, counts, n_voxels i32 (F,), vox_off i32 (F+1,), status) -- capacity-sized, offsets on the device."""
    assert pcd.dim() == 3 and pcd.dtype == torch.float32
    F, cap, ncol = pcd.shape
    assert 1 <= F <= 63, 'the voxelizer takes 1..63 frames per call (include/mvx_hip.h)'
    dev = pcd.device
    if n_points is None:
        n_points = torch.full((F,), cap, dtype=torch.int32, device=dev)
    total = F * cap
    voxels = torch.empty((total, T, out_channels), dtype=torch.float32, device=dev)
    coords = torch.empty((total, 4), dtype=torch.int64, device=dev)
    counts = torch.empty((total,), dtype=torch.int32, device=dev)
    n_vox = torch.empty((F,), dtype=torch.int32, device=dev)
    vox_off = torch.empty((F + 1,), dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = workspace(X.lib.mvx_voxelize_workspace_bytes(F, cap), dev, 'voxelize')
    with _timed_bytes('voxelize', F * cap * (ncol * 4 + 4) + F * (cap // 4) * (T * out_channels * 4 + 36)):
        rc = X.lib.mvx_voxelize_frames(X.ptr(pcd), X.ptr(perm), X.ptr(n_points), None, F, cap, ncol,
                                       float(lo[0]), float(lo[1]), float(lo[2]), float(size[0]), float(size[1]), float(size[2]),
                                       int(T), int(out_channels), total, 1, X.ptr(voxels), X.ptr(coords), X.ptr(counts),
                                       X.ptr(n_vox), X.ptr(vox_off), X.ptr(status), X.ptr(ws), ws.numel(), X.stream())
    X.check(rc, 'mvx_voxelize_frames')
    return voxels, coords, counts, n_vox, vox_off, status


# ---------------------------------------------------------------------------------------------
# dense grid scatter / gather
# ---------------------------------------------------------------------------------------------
_TILE = None


def conv_tile_shape():
    global _TILE
    if _TILE is None:
        import ctypes
        th, tw = ctypes.c_int32(0), ctypes.c_int32(0)
        X.lib.mvx_conv3d_tile_shape(ctypes.byref(th), ctypes.byref(tw))
        _TILE = (th.value, tw.value)
    return _TILE


def scatter_voxels(feat, coords, dhw, grid=None, zero=True, want_occupancy=False):
    D, H, W = dhw
    V, C = feat.shape
    if grid is None:
        grid = torch.empty((D, H, W, C), dtype=torch.float32, device=feat.device)
    status = torch.zeros((1,), dtype=torch.int32, device=feat.device)
    th, tw = conv_tile_shape()
    occ = bits = None
    if want_occupancy:
        occ = torch.empty((D, -(-H // th), -(-W // tw)), dtype=torch.int32, device=feat.device)
        bits = torch.empty((D, H, -(-W // 32)), dtype=torch.int32, device=feat.device)
    X.call('mvx_scatter_voxels', feat, coords, grid, V, C, D, H, W, int(zero), status, occ, th, tw, bits)
    if want_occupancy:
        return grid, status, (occ, bits)
    return grid, status


def gather_voxels(grid, coords, V):
    D, H, W, C = grid.shape
    feat = torch.empty((V, C), dtype=torch.float32, device=grid.device)
    X.call('mvx_gather_voxels', grid, coords, feat, V, C, D, H, W)
    return feat


def cl_to_bev(cl, F=None):
    """channels-last (D,H,W,C) -> (C*D,H,W) contiguous, channel = c*D + d; a frame set (F*D,H,W,C) -> (F,C*D,H,W)."""
    FD, H, W, C = cl.shape
    D = FD // (F or 1)
    bev = torch.empty(_per_frame(F, C * D, H, W), dtype=torch.float32, device=cl.device)
    with _timed_bytes('cl_bev_transpose', 2 * cl.numel() * 4):
        X.call('mvx_cl_to_bev_frames', cl, bev, D, H, W, C, 0, F or 1)
    return bev


def bev_to_cl(bev, D):
    """(C*D,H,W) -> channels-last (D,H,W,C); a frame set (F,C*D,H,W) -> (F*D,H,W,C)."""
    F = bev.shape[0] if bev.dim() == 4 else 1
    CD, H, W = bev.shape[-3:]
    C = CD // D
    cl = torch.empty((F * D, H, W, C), dtype=torch.float32, device=bev.device)
    X.call('mvx_cl_to_bev_frames', cl, bev, D, H, W, C, 1, F)
    return cl


def bev_to_cl_broadcast(bev, D, F):
    """ONE map (1,C*D,H,W) -> channels-last (F*D,H,W,C): transposed once, written F times."""
    CD, H, W = bev.shape[-3:]
    C = CD // D
    cl = torch.empty((F * D, H, W, C), dtype=torch.float32, device=bev.device)
    X.call('mvx_bev_to_cl_broadcast', bev, cl, D, H, W, C, F)
    return cl


# ---------------------------------------------------------------------------------------------
# BatchNorm (batch statistics) + ReLU
# ---------------------------------------------------------------------------------------------
def row_stats(y2d):
    rows, C = y2d.shape
    stats = torch.empty((STATS_REPLICAS, 2, C), dtype=torch.float64, device=y2d.device)
    X.call('mvx_row_stats', y2d, stats, rows, C)
    return stats


def row_stats_frames(y, C, F):
    """BatchNorm sums f64 (F,R,2,C) of a frame set: y holds its rows of C channels frame after frame."""
    stats = torch.empty((F, STATS_REPLICAS, 2, C), dtype=torch.float64, device=y.device)
    X.call('mvx_row_stats_frames', y, stats, y.numel() // C, C, F)
    return stats


def bn_finalize(stats, count, eps, F=None):
    """(mean, 1/sqrt(var + eps)) f32 (2,C) from the sums of one frame; (F,2,C) from those of a frame set."""
    C = stats.shape[-1]
    mi = torch.empty(_per_frame(F, 2, C), dtype=torch.float32, device=stats.device)
    X.call('mvx_bn_finalize_frames', stats, float(count), float(eps), mi, C, F or 1)
    return mi


def _desc_ref(desc):
    return desc.ref() if desc is not None else None


def bn_apply(y, mi, out=None, desc=None, kind=X.ROWS_SINGLE, timed=True):
    """``desc`` / ``kind``: the frames of a frame set and its row layout (X.FramesDesc, X.ROWS_*), mi (F,2,C) then."""
    C = mi.shape[-1]
    rows = y.numel() // C
    if out is None:
        out = torch.empty_like(y)
    with _timed_bytes('bn_apply', 2 * y.numel() * 4) if timed else _Inline():
        X.call('mvx_bn_apply_frames', y, mi, out, rows, C, _desc_ref(desc), kind)
    return out


def bn_apply_strided(x, mi, buf, rows, C, ld, off, F, reverse=False):
    """x (rows,C) normalised per frame into columns off..off+C of the (rows,ld) buffer ``buf``; ``reverse``: that column slice of
    buf copied out into x (mi unused: the gradient of the concat)."""
    X.call('mvx_bn_apply_strided_frames', x, mi, buf, rows, C, ld, off, F, int(reverse))


def d2s_bn_apply(t, mi, buf, F, h, w, s, cout, ld, off, reverse=False):
    """t (F*h*w, s*s*cout) normalised per frame and pixel-shuffled into columns off..off+cout of the (F*h*s*w*s, ld) buffer
    ``buf``; ``reverse``: the inverse shuffle of that slice of buf into t (mi unused)."""
    X.call('mvx_d2s_bn_apply_frames', t, mi, buf, F, h, w, s, cout, ld, off, int(reverse))


def space_to_depth(x, F, planes, h, w, C, reverse=False):
    """[F*planes][h][w][C] -> [F][h/2][w/2][4*planes*C] (2x2 parity blocks side by side); ``reverse``: the way back."""
    shape = (F * planes, h, w, C) if reverse else (F, h // 2, w // 2, 4 * planes * C)
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
    X.call('mvx_space_to_depth_frames', x, out, F, planes, h, w, C, int(reverse))
    return out


def bn_relu_backward(dyhat, y, mi, count, want_dbias=True, dz=None, row_w=None, dbias_out=None, desc=None, kind=X.ROWS_SINGLE,
                     timed=True):
    """dbias_out: existing gradient buffer to ADD the bias gradient to (returns None for dbias then).  ``desc`` / ``kind``: a frame
    set (per-frame counts come from its descriptor; dbias is summed over the frames)."""
    C = mi.shape[-1]
    rows = y.numel() // C
    if dz is None:
        dz = torch.empty_like(y)
    flags = 0
    if dbias_out is not None:
        dbias, flags = dbias_out, FLAG_ACCUMULATE
    else:
        dbias = torch.empty((C,), dtype=torch.float32, device=y.device) if want_dbias else None
    scratch, fz = _bn_backward_scratch(C, desc, y.device)
    amax = new_amax(y.device)
    with _timed_bytes('bn_relu_backward', 5 * y.numel() * 4) if timed else _Inline():      # reduce reads 2 tensors, apply reads 2 + writes 1
        X.call('mvx_bn_relu_backward_frames', dyhat, y, mi, float(count), dz, dbias, scratch, row_w, rows, C, flags | fz,
               _desc_ref(desc), kind, amax)
    tag_amax(dz, amax)                                   # max |dz|: the range the fp16x3 kernels scale dz by
    return dz, (None if dbias_out is not None else dbias)


def _bn_backward_scratch(C, desc, device):
    return _acc_f64((X.lib.mvx_bn_backward_scratch_bytes_frames(C, desc.n_frames if desc is not None else 1) // 8,), device)


def bn_relu_backward_planes(dyhat, y, mi, dbias_out, row_w, desc, kind):
    """bn_relu_backward of a frame set with dz written as three planes of bf16 pieces, int16 (3, rows, C), instead of f32 (a
    layer whose dz only feeds its own weight gradient on pre-cut operands: linear_wgrad_pre)."""
    C = mi.shape[-1]
    rows = y.numel() // C
    dzp = torch.empty((3, rows, C), dtype=torch.int16, device=y.device)
    scratch, fz = _bn_backward_scratch(C, desc, y.device)
    with _timed_bytes('bn_relu_backward', 5.5 * y.numel() * 4):
        X.call('mvx_bn_relu_backward_planes_frames', dyhat, y, mi, 1.0, dzp, dbias_out, scratch, row_w, rows, C,
               FLAG_ACCUMULATE | fz, desc.ref(), kind, None)
    return dzp


def bn_relu_backward_planes_parts(dyhat, y, mi, dbias_out, row_w, desc, kind, nparts):
    """Generator form of bn_relu_backward_planes: the apply pass is enqueued range by range; every iteration enqueues one part
    and yields ``(planes, row_lo, row_hi)`` -- the rows whose planes that part writes -- so the caller can put the weight gradient
    of those rows on the side stream before the next part is enqueued (mvx_bn_relu_backward_planes_part_frames).  The bias
    gradient is complete after the last part."""
    C = mi.shape[-1]
    rows = y.numel() // C
    dzp = torch.empty((3, rows, C), dtype=torch.int16, device=y.device)
    scratch, fz = _bn_backward_scratch(C, desc, y.device)
    rng = (ctypes.c_int64 * 2)()
    for part in range(nparts):
        with _timed_bytes('bn_relu_backward', 5.5 * y.numel() * 4 / nparts):
            X.call('mvx_bn_relu_backward_planes_part_frames', dyhat, y, mi, 1.0, dzp, dbias_out, scratch, row_w, rows, C,
                   FLAG_ACCUMULATE | fz, desc.ref(), kind, part, nparts, rng)
        if rng[1] > rng[0]:
            yield dzp, int(rng[0]), int(rng[1])


# ---------------------------------------------------------------------------------------------
# dense 3x3x3 convolution (channels-last, one frame)
# ---------------------------------------------------------------------------------------------
def conv3d_pack(weight, for_dgrad, split=False):
    """Kernel-layout weights; split=True: pre-split (hi, lo) bf16 pairs for the bf16x3 kernels.  A 2-D kernel
    (cout,cin,3,3) is packed as the middle depth slice of a 3-D one (exact-f32 kernels only): nn.Conv2d 3x3 / stride 1 /
    padding 1 then runs on the conv3d kernels with a depth-1 tensor and pad_d = 1."""
    cout, cin = weight.shape[0], weight.shape[1]
    two_d = tuple(weight.shape[2:]) == (3, 3)
    assert two_d or tuple(weight.shape[2:]) == (3, 3, 3)
    assert not (two_d and split)
    if split:
        sf = split_flags(split)
        if int(split) == 4:
            guard_fp16_weight(weight)
        wpk = torch.empty((X.lib.mvx_conv3d_packed_weight_bytes_split(cout, cin, sf) // 2,), dtype=torch.int16, device=weight.device)
        X.call('mvx_conv3d_pack_weights_split', weight.contiguous(), wpk, cout, cin, int(for_dgrad), sf)
        return wpk
    wpk = torch.empty((27 * cout * cin,), dtype=torch.float32, device=weight.device)
    X.call('mvx_conv3d_pack_weights', weight.contiguous(), wpk, cout, cin, int(for_dgrad) | (2 if two_d else 0))
    return wpk


def conv_out_depth(din, sd, pd):
    return (din + 2 * pd - 3) // sd + 1


def conv3d_forward(x, wpk, bias, cout, sd, pd, relu=True, want_stats=True, split=False):
    """Dense forward of one frame; split=True: bf16x3 kernel (wpk from conv3d_pack(..., split=True))."""
    din, H, W, cin = x.shape
    dout = conv_out_depth(din, sd, pd)
    out = torch.empty((dout, H, W, cout), dtype=torch.float32, device=x.device)
    stats, fz = _acc_f64((STATS_REPLICAS, 2, cout), x.device) if want_stats else (None, 0)
    flags = (FLAG_RELU if relu else 0) | fz | split_flags(split)
    if split:
        with _Timed('conv3d_gather_split', conv_flops(dout, din, H, W, cin, cout, sd, pd) if KERNEL_TIMERS is not None else 0):
            X.call('mvx_conv3d_forward_split', x, wpk, bias, out, stats, din, dout, H, W, cin, cout, sd, pd, flags)
        return out, stats
    with _Timed('conv3d_gather', conv_flops(dout, din, H, W, cin, cout, sd, pd) if KERNEL_TIMERS is not None else 0):
        X.call('mvx_conv3d_forward', x, wpk, bias, out, stats, din, dout, H, W, cin, cout, sd, pd, flags, _work_counter(x.device))
    return out, stats


def conv3d_dgrad(dz, wpk_d, din, cin, sd, pd, split=False):
    dout, H, W, cout = dz.shape
    dx = torch.empty((din, H, W, cin), dtype=torch.float32, device=dz.device)
    if split:
        with _Timed('conv3d_gather_split', conv_flops(din, dout, H, W, cout, cin, sd, pd, True) if KERNEL_TIMERS is not None else 0):
            bind_amax(split, dz)
            X.call('mvx_conv3d_dgrad_split', dz, wpk_d, dx, din, dout, H, W, cin, cout, sd, pd, split_flags(split))
        return dx
    with _Timed('conv3d_gather', conv_flops(din, dout, H, W, cout, cin, sd, pd, True) if KERNEL_TIMERS is not None else 0):
        X.call('mvx_conv3d_dgrad', dz, wpk_d, dx, din, dout, H, W, cin, cout, sd, pd, _work_counter(dz.device))
    return dx


def conv3d_wgrad(x, dz, sd, pd, split=False, accumulate_into=None, two_d=False):
    """accumulate_into: existing (cout,cin,3,3,3) gradient buffer to ADD to (returns None then).
    two_d: the gradient of a 2-D kernel (cout,cin,3,3) (depth-1 tensors, pad_d = 1).
    split: the split arithmetic of conv3d_wgrad4s, which takes cin in multiples of 64."""
    din, H, W, cin = x.shape
    dout, _, _, cout = dz.shape
    if accumulate_into is not None:
        dw, flags = accumulate_into, FLAG_ACCUMULATE
    else:
        shape = (cout, cin, 3, 3) if two_d else (cout, cin, 3, 3, 3)
        dw, flags = torch.empty(shape, dtype=torch.float32, device=x.device), 0
    if two_d:
        assert not split and din == 1 and dout == 1 and pd == 1
        flags |= FLAG_CONV2D
    if split and cin % 64:
        raise ValueError('conv3d_wgrad: split arithmetic needs cin %% 64 == 0 (got cin = %d)' % cin)
    flags |= split_flags(split, True)
    nbytes = X.lib.mvx_conv3d_wgrad_workspace_bytes(H, W, cin, cout)
    with _wgrad_scope(accumulate_into, x, dz) as scope:
        ws = workspace(nbytes, x.device, 'wgrad_side' if isinstance(scope, _SideStream) else 'wgrad')
        with _Timed('conv3d_wgrad', conv_flops(dout, din, H, W, cin, cout, sd, pd) if KERNEL_TIMERS is not None else 0):
            bind_amax(split, x, dz)
            X.call('mvx_conv3d_wgrad', x, dz, dw, din, dout, H, W, cin, cout, sd, pd, flags, ws, ws.numel())
    return None if accumulate_into is not None else dw


# ---------------------------------------------------------------------------------------------
# 3x3 2-D convolutions of a frame set on the same kernels: maps channels-last [F][h][w][c], one plane per frame; ``flags``:
# FLAG_TAPS2 = a 2x2 tap window (the stride-2 layers on the space-to-depth image); wpk from conv3d_pack
# ---------------------------------------------------------------------------------------------
FLAG_TAPS2 = 16          # MVX_FLAG_TAPS2


def _conv2d_flops(F, h, w, cin, cout, flags):
    if KERNEL_TIMERS is None:
        return 0
    return 2.0 * F * h * w * cin * cout * (2.25 if flags & FLAG_TAPS2 else 9)     # 2x2 window: 9 of the 16 (tap, parity) blocks run


def conv2d_forward(x, wpk, bias, F, h, w, cin, cout, flags, eps, split=False, want_mi=True):
    """y = ReLU(conv(x) + b) -> (y, mean_inv (F,2,cout)): per-frame statistics finalised in the launch (split kernels: behind it).
    ``want_mi=False`` (an eval forward on running statistics): the split kernels' finaliser launch is left out and mean_inv is
    not to be read; the sums built into the kernels are formed as ever."""
    dev = x.device
    y = torch.empty((F, h, w, cout), dtype=torch.float32, device=dev)
    stats, fz = _acc_f64((F, STATS_REPLICAS, 2, cout), dev)
    fin = _fin_slot(dev, fz)
    if fin is None:
        fin = torch.zeros((1,), dtype=torch.float64, device=dev)
    mi = torch.empty((F, 2, cout), dtype=torch.float32, device=dev)
    with _Timed('rpn_conv', _conv2d_flops(F, h, w, cin, cout, flags)):
        if split:                              # split arithmetic (bf16x3 / bf16x6), same window / structural-zero skipping
            X.call('mvx_conv2d_forward_split_frames', x, wpk, bias, y, stats, h, w, cin, cout,
                   FLAG_RELU | fz | flags | split_flags(split), F)
        else:
            X.call('mvx_conv2d_forward_frames', x, wpk, bias, y, stats, h, w, cin, cout, FLAG_RELU | fz | flags, fin, float(eps),
                   mi, _work_counter(dev), F)
    if split and want_mi:
        X.call('mvx_bn_finalize_frames', stats, float(h * w), float(eps), mi, cout, F)
    return y, mi


def conv2d_dgrad(dz, wpk_d, F, h, w, cin, cout, flags, split=False):
    dx = torch.empty((F, h, w, cin), dtype=torch.float32, device=dz.device)
    with _Timed('rpn_conv', _conv2d_flops(F, h, w, cin, cout, flags)):
        if split:
            bind_amax(split, dz)
            X.call('mvx_conv2d_dgrad_split_frames', dz, wpk_d, dx, h, w, cin, cout, flags | split_flags(split), F)
        else:
            X.call('mvx_conv2d_dgrad_frames', dz, wpk_d, dx, h, w, cin, cout, flags, _work_counter(dz.device), F)
    return dx


def conv2d_wgrad(x, dz, F, h, w, cin, cout, flags, accumulate_into=None, split=False):
    """dW (cout, cin, 3, 3) summed over the frames, on the side stream; ADDED into ``accumulate_into`` or returned."""
    dev = x.device
    # split arithmetic: the same entry point and workgroup decomposition (conv3d_wgrad4s, csrc/conv3d.hip) -- MVX_FLAG_SPLIT[3]
    sp = split_flags(split, True)
    nbytes = X.lib.mvx_conv2d_wgrad_workspace_bytes_frames(h, w, cin, cout, F)
    dw = accumulate_into if accumulate_into is not None else torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=dev)
    with _SideStream(x, dz, dw), _Timed('rpn_wgrad', _conv2d_flops(F, h, w, cin, cout, flags)):
        ws = workspace(nbytes, dev, 'rpn_wgrad_side')
        bind_amax(split, None, dz)
        X.call('mvx_conv2d_wgrad_frames', x, dz, dw, h, w, cin, cout,
               flags | sp | (FLAG_ACCUMULATE if accumulate_into is not None else 0), ws, ws.numel(), F)
    return dw


# ---------------------------------------------------------------------------------------------
# background rewrite of the CML stack (csrc/activity.hip)
# ---------------------------------------------------------------------------------------------
class Background:
    """What a CML activation looks like away from the voxels: per (plane, channel) constant ``c`` f32 (D,C)
    (``y_bg``: its value before the BatchNorm), site mask u8 (D,H,W) of the sites that do NOT hold it, per-tile
    flags i32 (D,tiles): ``hflag`` = the tile's halo holds such a site, ``tflag`` = the tile itself does.
    ``back``: dict the CONSUMER's backward fills for the producer's backward ('plane_grad_sums'), or None when
    the producer cannot use it (then the consumer computes a dense input gradient)."""
    __slots__ = ('c', 'y_bg', 'mask', 'hflag', 'tflag', 'bflag', 'back')

    def __init__(self, c, mask, hflag, tflag=None, y_bg=None, back=None, bflag=None):
        self.c, self.mask, self.hflag, self.tflag, self.y_bg, self.back = c, mask, hflag, tflag, y_bg, back
        # tiles on which this tensor's GRADIENT is produced/consumed by the restricted backward (defaults to tflag)
        self.bflag = bflag if bflag is not None else tflag


EXEC_STAGES = None       # device u64 counter of executed gather stages while KERNEL_TIMERS is on (bench roofline)
STAGE_FLOP = 2.0 * 9 * 128 * 32 * 64


def n_tiles(H, W):
    return ((H + 7) // 8) * ((W + 15) // 16)


def _exec_stages(device):
    """The EXEC_STAGES counter while KERNEL_TIMERS is on (created on first use), else None."""
    global EXEC_STAGES
    if KERNEL_TIMERS is None:
        return None
    if EXEC_STAGES is None:
        EXEC_STAGES = torch.zeros((1,), dtype=torch.int64, device=device)
    return EXEC_STAGES


# The wrappers of this section serve one frame and a frame set: ``F`` frames stacked along the depth axis ((F*D,H,W,C) where one
# frame is (D,H,W,C)); ``din`` / ``planes`` arguments stay PER FRAME.
def activity_dilate(src, src_is_index, din, H, W, sd, pd, mark_border, want_tile_flags=False, F=1):
    """(mask u8 (dout,H,W), halo flags i32 (dout,tiles)[, tile flags]) of a layer output from its input's activity."""
    dout = conv_out_depth(din, sd, pd)
    mask = torch.empty((F * dout, H, W), dtype=torch.uint8, device=src.device)
    hflag = torch.empty((F * dout, n_tiles(H, W)), dtype=torch.int32, device=src.device)
    tflag = torch.empty_like(hflag) if want_tile_flags else None
    X.call('mvx_activity_dilate_frames', src, 1 if src_is_index else 0, din, dout, H, W, sd, pd, 1 if mark_border else 0, mask,
           hflag, tflag, F)
    return (mask, hflag, tflag) if want_tile_flags else (mask, hflag)


def conv3d_background(w, c_in, din, sd, pd):
    cout, cin = w.shape[0], w.shape[1]
    dout = conv_out_depth(din, sd, pd)
    bg_pre = torch.empty((dout, cout), dtype=torch.float32, device=w.device)
    X.call('mvx_conv3d_background', w.contiguous(), c_in, din, dout, cin, cout, sd, pd, bg_pre)
    return bg_pre


def conv3d_background_taps(w, c_in, din, sd, pd, F=1):
    """Background constants of a layer, f32 (F*dout*13, cout): the [planes][cout] totals of conv3d_background, followed by the
    per-depth-tap ones (3) and the border classes (9) that the gather kernels use under FLAG_BG_TAPS."""
    cout, cin = w.shape[0], w.shape[1]
    dout = conv_out_depth(din, sd, pd)
    bg_all = torch.empty((F * dout * 13, cout), dtype=torch.float32, device=w.device)
    X.call('mvx_conv3d_background_taps_frames', w, c_in, din, dout, cin, cout, sd, pd, bg_all, F)
    return bg_all


def bn_background(bg_pre, bias, mi, planes, channels, relu=True, want_y=False, F=1):
    c_out = torch.empty((F * planes, channels), dtype=torch.float32, device=mi.device)
    y_bg = torch.empty_like(c_out) if want_y else None
    X.call('mvx_bn_background_frames', bg_pre, bias, mi, planes, channels, FLAG_RELU if relu else 0, y_bg, c_out, F)
    return (c_out, y_bg) if want_y else c_out


def bn_apply_tiles(y, mi, c_bg, tflag, F=1, read=None, out=None):
    """BatchNorm apply of a layer output with a background: tiles without a non-background site (``tflag`` 0) take the normalised
    constant ``c_bg`` without being read (bit-identical to bn_apply).  ``read``: tile flags of what the consuming layer reads
    (tile_read_flags): the background tiles outside that set are not written.  ``out``: written into (default: a new tensor)."""
    FD, H, W, C = y.shape
    if out is None:
        out = torch.empty_like(y)
    # algorithmic bytes (timing runs only): flagged tiles are read and written, the others only written
    nbytes = (lambda: (tflag.ne(0).sum() + (torch.logical_or(tflag.ne(0), read.ne(0)).sum() if read is not None else tflag.numel()))
              * (128 * C * 4)) if KERNEL_TIMERS is not None else 0
    with _timed_bytes('bn_apply', nbytes):
        if read is not None:
            X.call('mvx_bn_apply_tiles_read_frames', y, mi, c_bg, tflag, read, out, FD // F, H, W, C, F)
        else:
            X.call('mvx_bn_apply_tiles_frames', y, mi, c_bg, tflag, out, FD // F, H, W, C, F)
    return out


def bn_apply_tiles_bev(y, mi, c_bg, tflag, F=1):
    """bn_apply_tiles + cl_to_bev in one pass: the normalised (F*D,H,W,C) output written as the (F, C*D, H, W) map."""
    FD, H, W, C = y.shape
    D = FD // F
    bev = torch.empty((F, C * D, H, W), dtype=torch.float32, device=y.device)
    nbytes = (lambda: (tflag.ne(0).sum() + tflag.numel()) * (128 * C * 4)) if KERNEL_TIMERS is not None else 0
    with _timed_bytes('bn_apply', nbytes):
        X.call('mvx_bn_apply_tiles_bev_frames', y, mi, c_bg, tflag, bev, D, H, W, C, F)
    return bev


def plane_tap_sums(dz, tile_flags=None, inactive_sums=None):
    """f32 (planes, 9, C): border-corrected per-tap sums of dz over each plane (mvx_plane_tap_sums); with
    ``tile_flags`` dz is only read on the flagged tiles and ``inactive_sums`` (planes, C) stands for the rest."""
    D, H, W, C = dz.shape
    T = torch.empty((D, 9, C), dtype=torch.float32, device=dz.device)
    ws = workspace(X.lib.mvx_plane_tap_sums_workspace_bytes(D, C), dz.device, 'tap_sums')
    X.call('mvx_plane_tap_sums', dz, D, H, W, C, tile_flags, inactive_sums, T, ws, ws.numel())
    return T


def tile_dilate_flags(in_tflag, self_tflag, din, H, W, sd, pd, F=1):
    dout = conv_out_depth(din, sd, pd)
    out = torch.empty((F * dout, n_tiles(H, W)), dtype=torch.int32, device=in_tflag.device)
    X.call('mvx_tile_dilate_flags_frames', in_tflag, self_tflag, din, dout, H, W, sd, pd, out, F)
    return out


def tile_read_flags(hflag, din, H, W, sd, pd, F=1):
    """Which tiles of a layer's normalised INPUT the layer reads (its forward gather and weight gradient: the 3 x 3 tile
    neighbourhoods of the output tiles it computes), from the input's halo flags i32 (F*din, tiles)."""
    dout = conv_out_depth(din, sd, pd)
    out = torch.empty_like(hflag)
    X.call('mvx_tile_read_flags_frames', hflag, din, dout, H, W, sd, pd, out, F)
    return out


def conv3d_input_grad_sums(w, T, din, sd, pd, F=1):
    cout, cin = w.shape[0], w.shape[1]
    A = torch.empty((F * din, cin), dtype=torch.float32, device=w.device)
    X.call('mvx_conv3d_input_grad_sums_frames', w.contiguous(), T, din, T.shape[0] // F, cin, cout, sd, pd, A, F)
    return A


def conv3d_dgrad_tiles(dz, wpk_d, din, cin, sd, pd, tflag, split=False, F=1):
    """Input gradient on the flagged tiles only; the rest of the returned tensor is NOT initialised."""
    FD, H, W, cout = dz.shape
    dout = FD // F
    dx = torch.empty((F * din, H, W, cin), dtype=torch.float32, device=dz.device)
    counter = _exec_stages(dz.device)
    with _Timed('conv3d_gather_tiles', F * conv_flops(din, dout, H, W, cout, cin, sd, pd, True) if KERNEL_TIMERS is not None else 0):   # dense-equivalent
        if split:
            bind_amax(split, dz)
            X.call('mvx_conv3d_dgrad_tiles_split_frames', dz, wpk_d, dx, din, dout, H, W, cin, cout, sd, pd, split_flags(split),
                   tflag, counter, F)
        else:
            X.call('mvx_conv3d_dgrad_tiles_frames', dz, wpk_d, dx, din, dout, H, W, cin, cout, sd, pd, tflag, counter,
                   _work_counter(dz.device), F)
    return dx


def bn_relu_backward_tiles(dyhat, y, mi, bg, plane_grad_sums, dbias_out=None, want_inactive_sums=False, F=1):
    """BatchNorm+ReLU backward of a layer output with Background ``bg`` (its c, y_bg and bflag are read); dyhat valid on bg.bflag
    tiles only.  Returns (dz valid on those tiles only, dbias[, sums of dz over the other tiles (planes, C)])."""
    FD, H, W, C = y.shape
    dz = torch.empty_like(y)
    if dbias_out is not None:
        db, flags = dbias_out, FLAG_ACCUMULATE
    else:
        db, flags = torch.empty((C,), dtype=torch.float32, device=y.device), 0
    ws = workspace(X.lib.mvx_bn_relu_backward_tiles_workspace_bytes_frames(FD // F, H, W, C, F), y.device, 'bn_tiles')
    inact = torch.empty((FD, C), dtype=torch.float32, device=y.device) if want_inactive_sums else None
    amax = new_amax(y.device)                            # max |dz| over the written tiles (zeroed by the call)
    # algorithmic bytes (timing runs only): the flagged 8x16 tiles, two passes reading dyhat and y, the second writing dz
    bflag = bg.bflag
    nbytes = (lambda: bflag.ne(0).sum() * (128 * C * 4 * 5)) if KERNEL_TIMERS is not None else 0
    with _timed_bytes('bn_relu_backward_tiles', nbytes):
        X.call('mvx_bn_relu_backward_tiles_frames', dyhat, y, mi, bg.c, bg.y_bg, plane_grad_sums, bflag, FD // F, H, W, C, dz, db,
               inact, amax, flags, ws, ws.numel(), F)
    tag_amax(dz, amax)
    db = None if dbias_out is not None else db
    return (dz, db, inact) if want_inactive_sums else (dz, db)


def conv3d_forward_bg(x, wpk, bias, cout, sd, pd, bg_in, out_mask, bg_pre, relu=True, want_stats=True, finalize_eps=None,
                      split=False, F=None, bg_taps=False):
    """finalize_eps: also form the BatchNorm mean / inverse std (returns (y, mean_inv) then): in the kernel, or with the split
    kernels (wpk from conv3d_pack(..., split=...)) by a launch of bn_finalize behind it.  Of ``bg_in`` the halo flags are read.
    ``F``: a frame set (statistics per frame: (F,R,2,cout) / (F,2,cout)); ``bg_taps``: bg_pre is the head of a
    conv3d_background_taps table (FLAG_BG_TAPS)."""
    nf = F or 1
    FD, H, W, cin = x.shape
    din = FD // nf
    dout = conv_out_depth(din, sd, pd)
    out = torch.empty((nf * dout, H, W, cout), dtype=torch.float32, device=x.device)
    stats, fz = _acc_f64(_per_frame(F, STATS_REPLICAS, 2, cout), x.device) if want_stats else (None, 0)
    flags = (FLAG_RELU if relu else 0) | fz | split_flags(split) | (FLAG_BG_TAPS if bg_taps else 0)
    fin, mi, npos = None, None, float(dout * H * W)
    if finalize_eps is not None and want_stats:
        fin = _fin_slot(x.device, fz)
        if fin is None:
            fin = torch.zeros((1,), dtype=torch.float64, device=x.device)
        mi = torch.empty(_per_frame(F, 2, cout), dtype=torch.float32, device=x.device)
    counter = _exec_stages(x.device)
    with _Timed('conv3d_gather_bg', nf * conv_flops(dout, din, H, W, cin, cout, sd, pd) if KERNEL_TIMERS is not None else 0):   # dense-equivalent
        if split:
            X.call('mvx_conv3d_forward_bg_split_frames', x, wpk, bias, out, stats, din, dout, H, W, cin, cout, sd, pd, flags,
                   bg_in.hflag, out_mask, bg_pre, 1, counter, nf)
        else:
            X.call('mvx_conv3d_forward_bg_frames', x, wpk, bias, out, stats, din, dout, H, W, cin, cout, sd, pd, flags,
                   bg_in.hflag, out_mask, bg_pre, 1, counter, fin, npos, float(finalize_eps or 0.0), mi, _work_counter(x.device),
                   nf)
    if split and mi is not None:
        X.call('mvx_bn_finalize_frames', stats, npos, float(finalize_eps), mi, cout, nf)
    return (out, mi) if mi is not None else (out, stats)


def conv3d_wgrad_bg(x, dz, sd, pd, bg_in, tap_sums=None, accumulate_into=None, split=False, F=1, flops=0):
    """Of ``bg_in`` the constants c and the halo flags are read.  ``flops``: the figure of the timer (a number, or a callable
    evaluated after the timed region: the executed steps depend on the flags)."""
    FD, H, W, cin = x.shape
    din = FD // F
    dout, cout = dz.shape[0] // F, dz.shape[3]
    if accumulate_into is not None:
        dw, flags = accumulate_into, FLAG_ACCUMULATE
    else:
        dw, flags = torch.empty((cout, cin, 3, 3, 3), dtype=torch.float32, device=x.device), 0
    flags |= split_flags(split, True)              # split arithmetic: conv3d_wgrad4s behind the same entry point
    nbytes = X.lib.mvx_conv3d_wgrad_bg_workspace_bytes_frames(dout, H, W, cin, cout, F)
    if tap_sums is None:
        tap_sums = plane_tap_sums(dz)
    # every tensor the side-stream kernels read must be kept alive until that stream is joined (_SideStream), not only x and
    # dz: the tap sums and the background description are temporaries of the frame's own stream
    with _wgrad_scope(accumulate_into, x, dz, tap_sums, bg_in.c, bg_in.hflag) as scope:
        ws = workspace(nbytes, x.device, 'wgrad_bg_side' if isinstance(scope, _SideStream) else 'wgrad_bg')
        with _Timed('conv3d_wgrad_bg', flops):
            bind_amax(split, None, dz)
            X.call('mvx_conv3d_wgrad_bg_frames', x, dz, dw, din, dout, H, W, cin, cout, sd, pd, flags, bg_in.hflag, bg_in.c,
                   tap_sums, ws, ws.numel(), F)
    return None if accumulate_into is not None else dw


# ---------------------------------------------------------------------------------------------
# row-wise linear layers (2-D views with explicit leading dimensions)
# ---------------------------------------------------------------------------------------------
def _ld(t):
    assert t.dim() == 2 and t.stride(1) == 1, 'need a row-major 2-D view'
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _vptr(t):
    """Pointer of a (possibly column-sliced) row-major view."""
    if t is None:
        return None
    if not t.is_cuda:
        raise X.MvxHipError('libmvx_hip needs device tensors (no CPU fallback)')
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


def _fin_slot(device, zeroed):
    """u32 counter for the in-kernel BatchNorm finalisation: from the frame arena when the statistics came from it
    (pre-zeroed), else a fresh buffer the C entry clears."""
    if zeroed:
        a = _ARENAS.get(_arena_key(device))
        v = a.take(1) if a is not None else None
        if v is not None:
            return v
    return None


def _work_counter(device):
    """Zeroed u32 slot for the persistent convolution launches: from the frame arena, else a fresh zero."""
    if _ARENA_ON:
        a = _ARENAS.get(_arena_key(device))
        v = a.take(1) if a is not None else None
        if v is not None:
            return v
    return torch.zeros((1,), dtype=torch.float64, device=device)


ROW_SPLIT = ('dgrad', 'wgrad', 'rpn')


def row_split(tag):
    """Does the wide row GEMM ``tag`` run in bf16x3 arithmetic (csrc/linear_split.hip)?  Under ``convmath: bf16x3``, when an
    entry of ROW_SPLIT is a prefix of the tag.  Tags: 'fusion_<N>x<K>' (forward of a fusion MLP layer), 'vfe', 'conv1',
    'rpn' (forward of the wide VFE layer, of conv1's per-voxel GEMM, of the RPN's deconvolution GEMMs), 'dgrad' (every
    input-gradient row GEMM), 'wgrad' (every weight-gradient row GEMM).

    Default: the input and weight gradients and the RPN's forward GEMMs only.  A forward layer in split arithmetic carries ~5e-6 relative
    error (exact-f32 MFMA: ~8e-7) and the BatchNorm chain behind the FIRST layers of the network amplifies it 5-7x on the
    way to the BEV map.  Measured on one full-size frame against the float64 oracle and on bench.py --convmath bf16x3
    (tools/split_accuracy.py -> profiles/r03_split_accuracy.json; profiles/r03_split_speed.txt):

        forward rows in bf16x3          BEV map   cls logits  hot frames/s  full frames/s   (input gradients split, weight gradients f32)
        none (convolutions only)        7.6e-6    1.36e-4     443           200
        rpn                             7.6e-6    1.37e-4       (within noise of the row above)
        conv1                           1.3e-5    1.49e-4
        vfe                             1.1e-5    1.82e-4
        fusion_768x768                  3.1e-5    4.5e-4      466           202
        fusion (all five layers)        4.4e-5    6.1e-4
        fusion,vfe,conv1,rpn            4.8e-5    6.3e-4      472           208

    i.e. the 768 -> 768 layer, the only one whose speed matters (81 % of the row-GEMM flops of a step, +5 % frames/s), is
    also the one that costs a factor 3-4 in accuracy of every later map: it stays on the exact-f32 kernel.  The weight-gradient GEMMs ('wgrad', linear_wgrad_split: 0.955 -> 0.517 ms for the
    768 x 768 layer over 80 k rows) touch no forward map and are split by default: hot 443 -> 470, full 200 -> 210 frames/s.

    Returns the number of bf16 pieces (0 = exact-f32 kernel, 2 = bf16x3, 3 = bf16x6).  Under ``convmath: bf16x6`` the split is
    fp32-grade (three pieces = the whole f32 mantissa), so every tag uses it."""
    np_ = split_pieces()
    if np_ == 2:
        return 2 if any(tag.startswith(k) for k in ROW_SPLIT) else 0
    if np_ in (3, 4):
        return np_
    return 0


def transposed_weight(w2):
    """Row-major W^T of a (N, K) weight view, cached ON the parameter it views (so it dies with the model) and keyed by the
    parameter's version counter and the view's address: an optimizer step, load_state_dict or .to() makes the copy stale
    and it is made again.  (Not a module-level cache keyed by address: a new model may reuse a freed model's addresses at
    version 0.)  The input-gradient GEMM then reads both operands with 16-byte loads along k -- the transposed-read form of
    the f32 kernel collects its weight tile with 4-byte loads and ran at 0.43 matrix-pipe busy against 0.61 for the forward
    form -- and the split row GEMM reads row-major weights only (csrc/linear_split.hip)."""
    base = w2._base if w2._base is not None else w2
    cache = base.__dict__.setdefault('_mvx_wt', {})
    tag = (base._version, w2.data_ptr())
    hit = cache.get(tuple(w2.shape))
    if hit is None or hit[0] != tag:
        hit = (tag, w2.detach().t().contiguous())
        cache[tuple(w2.shape)] = hit
    return hit[1]


def padded_weight(w2, k):
    """(N, k) copy of a (N, K <= k) weight view with zero columns appended, cached on the parameter like transposed_weight: the
    operand of a row layer whose input rows were written with a pitch of k floats (frames._vfe_forward: 23 -> 24)."""
    if w2.shape[1] == k:
        return w2
    base = w2._base if w2._base is not None else w2
    cache = base.__dict__.setdefault('_mvx_wpad', {})
    tag = (base._version, w2.data_ptr())
    hit = cache.get((tuple(w2.shape), k))
    if hit is None or hit[0] != tag:
        wp = torch.zeros((w2.shape[0], k), dtype=w2.dtype, device=w2.device)
        wp[:, :w2.shape[1]] = w2.detach()
        hit = (tag, wp)
        cache[(tuple(w2.shape), k)] = hit
    return hit[1]


# ---------------------------------------------------------------------------------------------
# Row GEMMs on pre-cut operands (csrc/rowgemm_pre.hip): the operands are PLANES of 16-bit pieces, int16 (pieces, rows, k),
# written by their producers; the GEMM moves them global -> LDS by DMA.  Used for the wide layers whose shape fills its
# 256 x 256 tiles (n a multiple of 256: the 768 -> 768 fusion layer, 70 % of the row-GEMM work of a step) in the bf16x6
# arithmetic; every other call keeps the in-kernel-cut kernels.
# The FORWARD on pre-cut operands: its products and their accumulation order are those of linear_fwd_split (y is bit-identical)
# and its BatchNorm sums are formed term by term in f64 from an LDS copy of the tile (csrc/rowgemm_pre.hip), equal to that
# kernel's to f64 rounding -- the four-term f32 partial sums of its first form (1e-9 off: enough to move a mean by an ulp between
# executors that tile the rows differently) are gone, and with them the reason it was opt-in.
# ---------------------------------------------------------------------------------------------
# MVX_FLAG_PRE_XCD_STRIPS of mvx_linear_wgrad_pre: every block of a row strip on the same XCD (developer knob, A/B runs)
PRE_XCD_STRIPS = 4096 if os.environ.get('MVX_PRE_XCD', '0') != '0' else 0


def precut_ok(split, rows, K, N):
    return bool(split and int(split) == 3 and N % 256 == 0 and K % 16 == 0 and rows >= 2048 and
                3 * rows * max(K, N) * 2 < (1 << 32))


def split_rows(x, split, scale=1.0):
    """f32 (rows, k) -> planes int16 (pieces, rows, k) (mvx_split_rows).  For tensors whose producer does not write planes."""
    rows, K = x.shape
    flags = split_flags(split, True)
    planes = torch.empty((3 if int(split) == 3 else 2, rows, K), dtype=torch.int16, device=x.device)
    X.call('mvx_split_rows', _vptr(x), _ld(x), rows, K, planes, flags, float(scale))
    return planes


def weight_planes(w2, split):
    """Planes of a (N, K) weight view, cached ON the parameter it views and keyed by its version counter (see transposed_weight):
    cut once per optimizer step instead of in every workgroup of every launch."""
    base = w2._base if w2._base is not None else w2
    cache = base.__dict__.setdefault('_mvx_wp', {})
    tag = (base._version, w2.data_ptr())
    key = (tuple(w2.shape), int(split))
    hit = cache.get(key)
    if hit is None or hit[0] != tag:
        hit = (tag, split_rows(w2.detach().contiguous(), split))
        cache[key] = hit
    return hit[1]


def linear_forward_pre(x_planes, w_planes, bias, y, stats, row_w, flags, counter, eps, mi, desc, kind):
    """y = [ReLU](x w^T + b) with per-frame BatchNorm sums / finalisation from operand planes (mvx_linear_forward_pre_frames)."""
    _, rows, K = x_planes.shape
    N = w_planes.shape[1]
    with _Timed('linear_fwd', 2.0 * rows * K * N if KERNEL_TIMERS is not None else 0):
        X.call('mvx_linear_forward_pre_frames', x_planes, w_planes, bias, _vptr(y), _ld(y), stats, row_w, rows, K, N, flags, 1.0,
               counter, float(eps), mi, desc.ref() if desc is not None else None, kind)


def linear_wgrad_pre(x_planes, dz_planes, accumulate_into=None, rows=None):
    """dW (N, K) (+)= dz^T x from operand planes (mvx_linear_wgrad_pre); on the side stream like linear_wgrad.  ``rows=(lo, hi)``:
    only those rows of the planes (mvx_linear_wgrad_pre_rows)."""
    pieces, plane_rows, K = x_planes.shape
    N = dz_planes.shape[2]
    lo, hi = rows if rows is not None else (0, plane_rows)
    # the kernel adds through 16-byte vectors: a gradient view that starts elsewhere (a GradBucket lays parameters back to back,
    # and a model with the direction head has 18 bias floats in front of the late part) gets the product through a buffer
    via = accumulate_into is not None and accumulate_into.data_ptr() % 16 != 0
    if accumulate_into is not None and not via:
        assert accumulate_into.is_contiguous() and accumulate_into.numel() == N * K
        dw, flags = accumulate_into, FLAG_ACCUMULATE
    else:
        dw, flags = torch.empty((N, K), dtype=torch.float32, device=x_planes.device), 0
    flags |= split_flags(3 if pieces == 3 else 4, True) | PRE_XCD_STRIPS
    nbytes = max(X.lib.mvx_linear_wgrad_pre_workspace_bytes(plane_rows, K, N), X.lib.mvx_linear_wgrad_pre_workspace_bytes(hi - lo, K, N))
    with _wgrad_scope(accumulate_into, x_planes, dz_planes) as scope:
        ws = workspace(nbytes, x_planes.device, 'lwgrad_pre_side' if isinstance(scope, _SideStream) else 'lwgrad_pre')
        with _Timed('linear_wgrad', 2.0 * (hi - lo) * K * N if KERNEL_TIMERS is not None else 0):
            X.call('mvx_linear_wgrad_pre_rows', x_planes, dz_planes, dw, plane_rows, lo, hi, K, N, flags, 1.0, ws, ws.numel())
        if via:
            if isinstance(scope, _SideStream):       # the buffer lives until the owning stream has joined (see _SideStream)
                _KEEP.setdefault(dw.device.index, []).append(dw)
            assert accumulate_into.is_contiguous() and accumulate_into.numel() == N * K
            accumulate_into.view(N, K).add_(dw)
    return None if accumulate_into is not None else dw


def rows_dgrad(dz, w2, label='linear_dgrad'):
    """dx = dz w2 of a row layer with weight (N, K): in bf16x3 arithmetic (``row_split('dgrad')``) through the cached
    transposed copy, otherwise through the f32 kernel's transposed-weight read."""
    if row_split('dgrad'):
        dx, _ = linear_forward(dz, transposed_weight(w2), None, relu=False, want_stats=False, label=label, split=row_split('dgrad'))
    else:
        dx, _ = linear_forward(dz, w2, None, relu=False, want_stats=False, w_transposed=True, label=label)
    return dx


def linear_forward(x, w, bias, relu=True, want_stats=True, w_transposed=False, row_w=None, out=None, finalize=None,
                   label=None, split=False, foreign=False):
    """x (R,K) view, w (N,K) [or (K,N) if w_transposed] -> y (R,N), stats f64 (2,N) or None.
    ``finalize=(count, eps)``: the BatchNorm mean / inverse std are formed by the kernel's last workgroup
    (mvx_linear_forward_bn); returns (y, mean_inv) then.  ``split``: bf16x3 arithmetic where the shape qualifies
    (MVX_FLAG_SPLIT); ``label``: timer name of this call (default linear_fwd / linear_dgrad by w_transposed)."""
    R, K = x.shape
    N = w.shape[1] if w_transposed else w.shape[0]
    if out is None:
        out = torch.empty((R, N), dtype=torch.float32, device=x.device)
    stats, fz = _acc_f64((STATS_REPLICAS, 2, N), x.device) if want_stats else (None, 0)
    if label == 'linear_dgrad':
        split = grad_split(split, x)
    xfl = 0
    if foreign:                                      # x comes from outside the library: foreign_split
        split, xfl = foreign_split(split, x)
    if split and int(split) == 4:
        guard_fp16_weight(w)
    if finalize is not None and want_stats and R > 0:
        counter = _fin_slot(x.device, fz)
        if counter is None:
            counter = torch.zeros((1,), dtype=torch.float64, device=x.device)
        mi = torch.empty((2, N), dtype=torch.float32, device=x.device)
        bind_amax(split, x)
        X.call('mvx_linear_forward_bn', _vptr(x), _ld(x), _vptr(w), _ld(w), int(w_transposed), bias, _vptr(out), _ld(out), stats,
               row_w, R, K, N, (FLAG_RELU if relu else 0) | fz | split_flags(split, True) | xfl, counter, float(finalize[0]),
               float(finalize[1]), mi)
        return out, mi
    ws = None
    if bias is None and not relu and not want_stats and K >= 256 and R * N <= (1 << 22):
        ws = workspace(X.lib.mvx_linear_splitk_workspace_bytes(R, N), x.device, 'splitk')
    with _Timed(label or ('linear_dgrad' if w_transposed else 'linear_fwd'), 2.0 * R * K * N if KERNEL_TIMERS is not None else 0):
        bind_amax(split, x)
        X.call('mvx_linear_forward', _vptr(x), _ld(x), _vptr(w), _ld(w), int(w_transposed), bias, _vptr(out), _ld(out), stats,
               row_w, R, K, N, (FLAG_RELU if relu else 0) | fz | split_flags(split, True) | xfl, ws,
               ws.numel() if ws is not None else 0)
    if finalize is not None and want_stats:      # empty input: no launch happened, finalise the (zero) sums separately
        return out, bn_finalize(stats, finalize[0], finalize[1])
    return out, stats


def linear_forward_bn_frames(x, w2, bias, desc, kind, row_w, eps, split=False, foreign=False):
    """Rows of a frame set -> (y = ReLU(x w2^T + b), mean_inv (F,2,N)) with per-frame BatchNorm statistics formed and finalised
    inside the launch (mvx_linear_forward_bn_frames); ``desc`` / ``kind``: the frames and their row layout (X.ROWS_*).  When the
    producer of x wrote it as planes of bf16 pieces too (``x._mvx_planes``) and the shape qualifies (precut_ok), the row GEMM on
    pre-cut operands runs instead: same products, same accumulation order -- bit-identical y.  ``foreign``: x was not produced
    by this library (the sampled image features): foreign_split."""
    Rr, K = x.shape
    N = w2.shape[0]
    y = torch.empty((Rr, N), dtype=torch.float32, device=x.device)
    stats, fz = _acc_f64((desc.n_frames, STATS_REPLICAS, 2, N), x.device)
    counter = _fin_slot(x.device, fz)              # arena slot when the statistics came from the (pre-zeroed) arena
    if counter is None:
        counter = torch.zeros((1,), dtype=torch.float64, device=x.device)
    mi = torch.empty((desc.n_frames, 2, N), dtype=torch.float32, device=x.device)
    xp = getattr(x, '_mvx_planes', None)
    if xp is not None and precut_ok(split, Rr, K, N):
        linear_forward_pre(xp, weight_planes(w2, split), bias, y, stats, row_w, FLAG_RELU | fz | split_flags(split, True),
                           counter, eps, mi, desc, kind)
        return y, mi
    xfl = 0
    if foreign:
        split, xfl = foreign_split(split, x)
    if split and int(split) == 4:
        guard_fp16_weight(w2)                          # fp16x3: |w| < 255.9 (device-side status bit, checked once per step)
    with _Timed('linear_fwd', 2.0 * Rr * K * N if KERNEL_TIMERS is not None else 0):
        bind_amax(split, x)                            # fp16x3: the range tag of a foreign input (the sampled image features)
        X.call('mvx_linear_forward_bn_frames', _vptr(x), _ld(x), _vptr(w2), _ld(w2), 0, bias, _vptr(y), _ld(y), stats, row_w, Rr,
               K, N, FLAG_RELU | fz | split_flags(split, True) | xfl, counter, float(eps), mi, desc.ref(), kind)
    return y, mi


def linear_wgrad(x, dz, accumulate_into=None, split=None, x_foreign=False):
    """dW (N,K) = dz^T x; accumulate_into: existing contiguous (N,K)-sized gradient buffer to ADD to.  ``split``: bf16x3
    arithmetic (MVX_FLAG_SPLIT, csrc/linear_split.hip linear_wgrad_split); None = as ``row_split('wgrad')`` says."""
    R, K = x.shape
    N = dz.shape[1]
    if accumulate_into is not None:
        assert accumulate_into.is_contiguous() and accumulate_into.numel() == N * K
        dw, flags = accumulate_into, FLAG_ACCUMULATE
    else:
        dw, flags = torch.empty((N, K), dtype=torch.float32, device=x.device), 0
    split = grad_split(row_split('wgrad') if split is None else split, dz)
    if x_foreign:                                    # a foreign input of unknown range: see foreign_split
        split = foreign_split(split, x)[0]
    flags |= split_flags(split, True)
    nbytes = X.lib.mvx_linear_wgrad_workspace_bytes(R, K, N)
    with _wgrad_scope(accumulate_into, x, dz) as scope:
        ws = workspace(nbytes, x.device, 'lwgrad_side' if isinstance(scope, _SideStream) else 'lwgrad')
        with _Timed('linear_wgrad', 2.0 * R * K * N if KERNEL_TIMERS is not None else 0):
            bind_amax(split, x, dz)
            X.call('mvx_linear_wgrad', _vptr(x), _ld(x), _vptr(dz), _ld(dz), dw, R, K, N, flags, ws, ws.numel())
    return None if accumulate_into is not None else dw


# ---------------------------------------------------------------------------------------------
# VFE glue (dense [V][T][C] rows, or compact rows described by a CompactRows)
# ---------------------------------------------------------------------------------------------
class CompactRows:
    """Row layout of one frame in compact form: n_real real rows followed by one padded row per
    voxel (see include/mvx_hip.h, 'Compact rows')."""

    desc = None                          # one frame (frames.FrameSet, the same layout for a frame set, carries its X.FramesDesc here)

    def __init__(self, row_map, rows_sel, n_real, V, T):
        self.row_map, self.rows_sel = row_map, rows_sel
        self.n_real, self.V, self.T = int(n_real), int(V), int(T)
        self.voff, self.vcnt, self.row_w = voxel_row_offsets(row_map, self.V, self.T, self.n_real)

    @property
    def rows(self):
        return self.n_real + self.V

    @property
    def count(self):                     # rows of the dense tensor this layout stands for
        return self.V * self.T


def voxel_row_offsets(row_map, V, T, n_real, desc=None):
    """Per-voxel row offsets / counts i32 (V,) and the BatchNorm row weights f32 (n_real + V,) of a compact layout; with the
    ``desc`` of a frame set also the row weights of its fusion layout f32 (n_real + F,)."""
    dev = row_map.device
    voff = torch.empty((V,), dtype=torch.int32, device=dev)
    vcnt = torch.empty((V,), dtype=torch.int32, device=dev)
    row_w = torch.empty((n_real + V,), dtype=torch.float32, device=dev)
    fusion_row_w = torch.empty((n_real + desc.n_frames,), dtype=torch.float32, device=dev) if desc is not None else None
    X.call('mvx_voxel_row_offsets_frames', row_map, V, T, n_real, voff, vcnt, row_w, fusion_row_w, _desc_ref(desc))
    return (voff, vcnt, row_w) if desc is None else (voff, vcnt, row_w, fusion_row_w)


def _rows_args(cr):
    """``cr``: a CompactRows (one frame), a frames.FrameSet (a frame set: ``desc`` set), or None (dense rows)."""
    if cr is None:
        return None, None, 0, None
    return X.ptr(cr.voff), X.ptr(cr.vcnt), cr.n_real, _desc_ref(cr.desc)


def vfe_bn_max_concat(y, mi, V, T, cr=None):
    C = mi.shape[-1]
    out = torch.empty((y.shape[0], 2 * C), dtype=torch.float32, device=y.device)
    am = torch.empty((V, C), dtype=torch.int32, device=y.device)
    vo, vc, nr, d = _rows_args(cr)
    with _timed_bytes('vfe_bn_max_concat', y.shape[0] * C * 4 * 3 + V * C * 4):      # read y, write [x | max] + argmax
        X.call('mvx_vfe_bn_max_concat_frames', y, mi, out, am, V, T, C, vo, vc, nr, d)
    return out, am


def vfe_max_concat_backward(g, am, V, T, cr=None):
    C = am.shape[1]
    dyh = torch.empty((g.shape[0], C), dtype=torch.float32, device=g.device)
    vo, vc, nr, _ = _rows_args(cr)
    with _timed_bytes('vfe_max_concat_backward', g.shape[0] * C * 4 * 3 + V * C * 4):  # read [gx | gmax] + argmax, write dyhat
        X.call('mvx_vfe_max_concat_backward', g, am, dyh, V, T, C, vo, vc, nr)
    return dyh


def bn_segment_max(y, mi, V, T, cr=None):
    C = mi.shape[-1]
    out = torch.empty((V, C), dtype=torch.float32, device=y.device)
    am = torch.empty((V, C), dtype=torch.int32, device=y.device)
    vo, vc, nr, d = _rows_args(cr)
    with _timed_bytes('vfe_bn_segment_max', y.shape[0] * C * 4 + V * C * 8):          # read y, write max + argmax
        X.call('mvx_bn_segment_max_frames', y, mi, out, am, V, T, C, vo, vc, nr, d)
    return out, am


def segment_max_backward(dfeat, am, V, T, cr=None):
    C = am.shape[1]
    rows = cr.rows if cr is not None else V * T
    dyh = torch.empty((rows, C), dtype=torch.float32, device=dfeat.device)
    vo, vc, nr, _ = _rows_args(cr)
    X.call('mvx_segment_max_backward', dfeat, am, dyh, V, T, C, vo, vc, nr)
    return dyh


def vfe_compact_input(vox2d, imfeat_c, cr, pitch=None):
    """[7 geometric channels | image features] rows of the layout ``cr`` (see _rows_args); ``pitch``: floats per output row
    (default 7 + F; more: zero columns behind)."""
    F = imfeat_c.shape[1]
    pitch = 7 + F if pitch is None else pitch
    out = torch.empty((cr.rows, pitch), dtype=torch.float32, device=vox2d.device)
    X.call('mvx_vfe_compact_input_pitch_frames', vox2d, vox2d.shape[1], cr.rows_sel, imfeat_c, F, cr.n_real, cr.V, out, pitch,
           _desc_ref(cr.desc))
    return out


def vfe_compact_input_backward(g, F, cr):
    """Gradient of the image features f32 (real rows + one shared padded row per frame, F)."""
    nf = cr.desc.n_frames if cr.desc is not None else 1
    d = torch.empty((cr.n_real + nf, F), dtype=torch.float32, device=g.device)
    scratch = torch.empty((nf * F,), dtype=torch.float64, device=g.device)
    X.call('mvx_vfe_compact_input_backward_frames', g, F, cr.n_real, cr.V, d, scratch, _desc_ref(cr.desc))
    return d


# ---------------------------------------------------------------------------------------------
# point <-> image fusion
# ---------------------------------------------------------------------------------------------
def row_compact_map(vox2d, desc=None):
    """vox2d (R, vc) -> row_map i32 (R,), rows_sel i32 (R,), n_real i32 (1,) (all on the device); with the ``desc`` of a frame
    set (its voxel offsets) also the real-row offsets of its frames i32 (F+1,)."""
    R, vc = vox2d.shape
    dev = vox2d.device
    row_map = torch.empty((R,), dtype=torch.int32, device=dev)
    rows_sel = torch.empty((R,), dtype=torch.int32, device=dev)
    n_real = torch.empty((1,), dtype=torch.int32, device=dev)
    real_off = torch.empty((desc.n_frames + 1,), dtype=torch.int32, device=dev) if desc is not None else None
    nbytes = X.lib.mvx_row_compact_workspace_bytes(R)
    ws = workspace(nbytes, dev, 'compact')
    X.call('mvx_row_compact_map_frames', vox2d, vc, R, row_map, rows_sel, n_real, ws, ws.numel(), _desc_ref(desc), real_off)
    return (row_map, rows_sel, n_real) if desc is None else (row_map, rows_sel, n_real, real_off)


def feature_sample(vox2d, feats_cl, imsize_hw, eps, out, row_map=None, rows_sel=None, n_real=None):
    """vox2d (R, vc) modified in place; feats_cl: list of channels-last (H, W, C) maps.  With ``rows_sel`` and
    ``n_real`` (from row_compact_map, which already zeroed the padding rows) only the real rows are visited."""
    R, vc = vox2d.shape
    L = len(feats_cl)
    C = feats_cl[0].shape[2]
    for f in feats_cl:
        assert f.is_contiguous() and f.dtype == torch.float32 and f.shape[2] == C
    if rows_sel is not None and n_real is not None:
        return feature_sample_rows(vox2d, rows_sel, int(n_real), feats_cl, imsize_hw, eps, out)
    ptrs = (ctypes.c_void_p * L)(*[f.data_ptr() for f in feats_cl])
    hw = (ctypes.c_int32 * (2 * L))(*[int(v) for f in feats_cl for v in f.shape[:2]])
    status = torch.zeros((1,), dtype=torch.int32, device=vox2d.device)
    # algorithmic bytes: 4 taps x L levels x C floats gathered + L*C floats written per sampled row, + the voxel rows
    nrows = out.shape[0]
    with _timed_bytes('feature_sample', nrows * L * C * 4 * 5 + R * vc * 4):
        X.call('mvx_feature_sample', vox2d, vc, R, row_map, ptrs, hw, L, C, float(imsize_hw[0]), float(imsize_hw[1]), float(eps),
               out, status)
    return status


def feature_sample_rows(vox2d, rows_sel, n_real, feats_cl, imsize_hw, eps, out, desc=None, amax=None, planes=None):
    """The ``n_real`` real rows ``rows_sel`` of vox2d (modified in place) sampled from channels-last (H, W, C) maps into the rows
    of ``out`` (None: not written).  A frame set (``desc``): feats_cl holds the L levels of frame 0, then of frame 1, ...; every
    row reads its own frame's maps.  ``amax`` f32 (1,), ZERO on entry: receives max |sample|.  ``planes`` int16 (3, rows, L*C):
    the samples also as planes of bf16 pieces.  Returns the status word."""
    vc = vox2d.shape[1]
    L = len(feats_cl) // (desc.n_frames if desc is not None else 1)
    C = feats_cl[0].shape[2]
    ptrs = (ctypes.c_void_p * len(feats_cl))(*[f.data_ptr() for f in feats_cl])
    hw = (ctypes.c_int32 * (2 * L))(*[int(v) for f in feats_cl[:L] for v in f.shape[:2]])
    status = torch.zeros((1,), dtype=torch.int32, device=vox2d.device)
    # algorithmic bytes: 4 taps x L levels x C floats gathered + L*C floats written per sampled row, + the voxel rows
    with _timed_bytes('feature_sample', n_real * L * C * 4 * 5 + n_real * vc * 4 + (n_real * L * C * 6 if planes is not None else 0)):
        if planes is not None:
            X.call('mvx_feature_sample_rows_planes_frames', vox2d, vc, rows_sel, n_real, ptrs, hw, L, C, float(imsize_hw[0]),
                   float(imsize_hw[1]), float(eps), out, status, _desc_ref(desc), amax, planes, planes.shape[1])
        else:
            X.call('mvx_feature_sample_rows_frames', vox2d, vc, rows_sel, n_real, ptrs, hw, L, C, float(imsize_hw[0]),
                   float(imsize_hw[1]), float(eps), out, status, _desc_ref(desc), amax)
    return status


def expand_rows(compact, row_map, pad_row):
    R = row_map.shape[0]
    C = compact.shape[1]
    out = torch.empty((R, C), dtype=torch.float32, device=compact.device)
    X.call('mvx_expand_rows', compact, row_map, int(pad_row), out, R, C)
    return out


def expand_rows_backward(g, row_map, pad_row, n_compact):
    R, C = g.shape
    dc = torch.empty((n_compact, C), dtype=torch.float32, device=g.device)
    scratch = torch.empty((C,), dtype=torch.float64, device=g.device)
    X.call('mvx_expand_rows_backward', g, row_map, int(pad_row), dc, scratch, R, C)
    return dc


# ---------------------------------------------------------------------------------------------
# crops and projection
# ---------------------------------------------------------------------------------------------
def _host_f64(a, n):
    import ctypes
    import numpy as np
    if a is None:
        return None, None
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    assert arr.size == n
    return arr, arr.ctypes.data_as(ctypes.c_void_p)


def crop_points(pcd, n_in=None, range6=None, bounds_f32=False, cam_from_velo=None, p2=None, imsize_wh=(0.0, 0.0),
                math_f32=False, want_index=False):
    """pcd f32 (F, cap, ncol) on the GPU -> (out (F, cap, ncol), n_out i32 (F,), src_index or None)."""
    F, cap, ncol = pcd.shape
    dev = pcd.device
    out = torch.empty_like(pcd)
    n_out = torch.empty((F,), dtype=torch.int32, device=dev)
    src = torch.empty((F, cap), dtype=torch.int32, device=dev) if want_index else None
    ws = workspace(X.lib.mvx_crop_workspace_bytes(F, cap), dev, 'crop')
    k1, r_ptr = _host_f64(range6, 6)
    k2, m_ptr = _host_f64(cam_from_velo, 16)
    k3, p_ptr = _host_f64(p2, 16)
    X.call('mvx_crop_points', pcd, n_in, F, cap, ncol, r_ptr, int(bounds_f32), m_ptr, p_ptr, float(imsize_wh[0]),
           float(imsize_wh[1]), int(math_f32), out, n_out, src, ws, ws.numel())
    return out, n_out, src


def crop_project(pcd, n_in, range6, cam_from_velo64, p2_64, imsize_wh, cam_from_velo32, p2_32, cap_out):
    """Raw clouds f32 (F, cap, 4) -> (points6 (F, cap_out, 6) = [x y z r row col], n_out i32 (F,)): crop + cropToSight
    (numpy-path f64 masks) and the f32 projection of train.py:31-34 in one compaction pass.  n_out[f] counts the points that
    passed and may exceed cap_out: only the first cap_out of them are stored."""
    F, cap, ncol = pcd.shape
    dev = pcd.device
    out = torch.empty((F, cap_out, ncol + 2), dtype=torch.float32, device=dev)
    n_out = torch.empty((F,), dtype=torch.int32, device=dev)
    ws = workspace(X.lib.mvx_crop_project_workspace_bytes(F, cap), dev, 'crop')
    k1, r_ptr = _host_f64(range6, 6)
    k2, m_ptr = _host_f64(cam_from_velo64, 16)
    k3, p_ptr = _host_f64(p2_64, 16)
    k4, m32_ptr = _host_f64(cam_from_velo32, 16)
    k5, p32_ptr = _host_f64(p2_32, 16)
    with _timed_bytes('crop_project', F * cap * ncol * 4 * 2 + F * cap_out * (ncol + 2) * 4):
        X.call('mvx_crop_project_points', pcd, n_in, F, cap, ncol, r_ptr, m_ptr, p_ptr, float(imsize_wh[0]), float(imsize_wh[1]),
               m32_ptr, p32_ptr, out, int(cap_out), n_out, ws, ws.numel())
    return out, n_out


def lidar2img(pcd2d, cam_from_velo, p2, math_f32=True, out=None, col_offset=0, swap_rc=False, want_z=False):
    """pcd2d f32 (n, ncol) -> out (n, 2) = (u, v) [or written into columns col_offset.. of `out`]."""
    n, ncol = pcd2d.shape
    if out is None:
        out = torch.empty((n, 2), dtype=torch.float32, device=pcd2d.device)
    z = torch.empty((n,), dtype=torch.float32, device=pcd2d.device) if want_z else None
    k2, m_ptr = _host_f64(cam_from_velo, 16)
    k3, p_ptr = _host_f64(p2, 16)
    X.call('mvx_lidar2img', pcd2d, ncol, n, m_ptr, p_ptr, int(math_f32), _vptr(out), _ld(out), col_offset, int(swap_rc), z)
    return out, z


# ---------------------------------------------------------------------------------------------
# input-sparse convolution as voxel GEMMs + index-grid gathers
# ---------------------------------------------------------------------------------------------
def index_grid(coords, dhw, desc=None):
    """Voxel index grid of one frame; with the ``desc`` of a frame set (coords of its frames back to back) of every frame."""
    D, H, W = dhw
    nf = desc.n_frames if desc is not None else 1
    buf = torch.empty((X.lib.mvx_index_grid_bytes_frames(D, H, W, nf) // 4,), dtype=torch.int32, device=coords.device)
    status = torch.zeros((1,), dtype=torch.int32, device=coords.device)
    X.call('mvx_index_grid_frames', coords, coords.shape[0], D, H, W, buf, status, _desc_ref(desc))
    return buf, status


def sparse_conv_output(P, idx_grid, dhw, bias, cout, sd, pd, relu=True, want_stats=True):
    din, H, W = dhw
    dout = conv_out_depth(din, sd, pd)
    out = torch.empty((dout, H, W, cout), dtype=torch.float32, device=P.device)
    stats, fz = _acc_f64((STATS_REPLICAS, 2, cout), P.device) if want_stats else (None, 0)
    with _timed_bytes('sparse_conv_output', out.numel() * 4 + din * H * W * 4):     # dense output written + index grid read
        X.call('mvx_sparse_conv_output', P, idx_grid, bias, out, stats, din, dout, H, W, cout, sd, pd,
               (FLAG_RELU if relu else 0) | fz)
    return out, stats


def sparse_conv_output_tiles(P, idx_grid, dhw, bias, cout, sd, pd, tflag, F=1, out=None):
    """sparse_conv_output of F frames, built only on the tiles ``tflag`` of the output that hold a site next to a voxel; the
    voxel-free tiles are not written (MVX_FLAG_NO_BG_FILL).  ``out``: written into (default: a new tensor).  Statistics per frame."""
    din, H, W = dhw
    dout = conv_out_depth(din, sd, pd)
    if out is None:
        out = torch.empty((F * dout, H, W, cout), dtype=torch.float32, device=P.device)
    stats, fz = _acc_f64((F, STATS_REPLICAS, 2, cout), P.device)
    with _timed_bytes('sparse_conv_output', out.numel() * 4 + F * din * H * W * 4):     # dense output written + index grid read
        X.call('mvx_sparse_conv_output_tiles_frames', P, idx_grid, bias, out, stats, din, dout, H, W, cout, sd, pd,
               FLAG_RELU | FLAG_NO_BG_FILL | fz, F, tflag)
    return out, stats


def sparse_conv_gather_dz(dz, coords, din, sd, pd, desc=None):
    FD, H, W, cout = dz.shape
    dout = FD // (desc.n_frames if desc is not None else 1)
    V = coords.shape[0]
    G = torch.empty((V, 27 * cout), dtype=torch.float32, device=dz.device)
    X.call('mvx_sparse_conv_gather_dz_frames', dz, coords, V, G, din, dout, H, W, cout, sd, pd, _desc_ref(desc))
    return tag_amax(G, amax_of(dz))                     # G's rows are rows of dz


def sink_of(param):
    """The parameter's existing gradient buffer if direct accumulation is enabled, else None.  Used for
    WEIGHT gradients, whose kernels run on the side stream when ASYNC_WGRAD is on."""
    if GRAD_SINK and param is not None and param.grad is not None and param.grad.is_contiguous():
        return param.grad
    return None


class _BiasStage:
    """Per-lane staging copy of the flat gradient bucket for BIAS gradients.  With ASYNC_WGRAD every write to a
    .grad buffer must go through the one side stream (frames are in flight on several streams), but bias
    gradients are finished on the frame's own stream: they are accumulated here (single writer: the lane) and
    added to the bucket ONCE per frame on the side stream.  Two buffers alternate, so that clearing one for
    frame f+2 only waits for the flush of frame f."""

    def __init__(self, flat):
        self.flat = flat
        self.bufs = [torch.zeros_like(flat), torch.zeros_like(flat)]
        self.events = [None, None]
        self.touched = [{}, {}]            # per buffer: offset -> length of the slices handed out since its last clear
        self.turn = 0
        self.base = flat.data_ptr()

    def _slices(self, t, turn):
        return [t[o:o + n] for o, n in sorted(self.touched[turn].items())]

    def begin(self):
        self.turn ^= 1
        ev = self.events[self.turn]
        if ev is not None:
            torch.cuda.current_stream(self.flat.device).wait_event(ev)
        # only the bias slices are ever written: clear and flush those (one multi-tensor kernel each), not the whole
        # bucket (two full-bucket passes per frame to move a few KB)
        if self.touched[self.turn]:
            torch._foreach_zero_(self._slices(self.bufs[self.turn], self.turn))
            self.touched[self.turn] = {}

    def view_for(self, grad):
        off = (grad.data_ptr() - self.base) // 4
        n = grad.numel()
        if off < 0 or off + n > self.flat.numel():
            return None
        self.touched[self.turn][off] = n
        return self.bufs[self.turn][off:off + n]

    def flush(self):
        buf = self.bufs[self.turn]
        with _SideStream(buf) as sc:
            if self.touched[self.turn]:
                torch._foreach_add_(self._slices(self.flat, self.turn), self._slices(buf, self.turn))
            ev = torch.cuda.Event()
            ev.record(sc.side)
        self.events[self.turn] = ev


_BIAS_STAGES = {}        # (device, raw lane stream) -> _BiasStage
_BIAS_STAGE_ON = False


def bias_stage_begin(device, flat_grad):
    """Start a frame on the current stream with bias gradients staged (see _BiasStage)."""
    global _BIAS_STAGE_ON
    key = _arena_key(device)
    st = _BIAS_STAGES.get(key)
    if st is None or st.flat is not flat_grad:
        st = _BiasStage(flat_grad)
        _BIAS_STAGES[key] = st
    st.begin()
    _BIAS_STAGE_ON = True


def bias_stage_flush(device):
    st = _BIAS_STAGES.get(_arena_key(device))
    if st is not None:
        st.flush()


def bias_stage_end():
    global _BIAS_STAGE_ON
    _BIAS_STAGE_ON = False


def bias_sink_of(param):
    """Bias gradients are finished on the stream of the backward pass.  Without ASYNC_WGRAD they go straight
    into .grad; with it, into the lane's staging copy when the pipeline opened one (bias_stage_begin), else they
    are produced as a temporary and added by ``accumulate_grad`` on the side stream."""
    if not ASYNC_WGRAD:
        return sink_of(param)
    if _BIAS_STAGE_ON and GRAD_SINK and param is not None and param.grad is not None:
        st = _BIAS_STAGES.get(_arena_key(param.device))
        if st is not None:
            return st.view_for(param.grad)
    return None


def accumulate_grad(param, g):
    """Add ``g`` into ``param.grad`` without autograd when sinks are on (side stream if ASYNC_WGRAD);
    returns what the autograd node should return for this parameter (None, or g itself)."""
    if g is None:
        return None
    tgt = sink_of(param)
    if tgt is None:
        return g
    if ASYNC_WGRAD:
        with _SideStream(g):
            tgt.add_(g.view_as(tgt))
    else:
        tgt.add_(g.view_as(tgt))
    return None


# ---------------------------------------------------------------------------------------------
# target assignment and loss (csrc/anchors.hip, csrc/loss.hip)
# ---------------------------------------------------------------------------------------------
def bbox_pairwise(b1, b2, want_iou):
    """b1 (N,4,2), b2 (M,4,2) f32 BEV corners on the GPU -> (N,M) IoU or intersection area."""
    n, m = b1.shape[0], b2.shape[0]
    out = torch.empty((n, m), dtype=torch.float32, device=b1.device)
    X.call('mvx_bbox_pairwise', b1, n, b2, m, int(want_iou), out)
    return out


def _anchor_lists(F, cap, dev):
    """The list buffers of F frames: pos_idx i64 (F,3,cap), neg_idx i64 (F,3,cap), gi i64 (F,cap)."""
    return (torch.empty((F, 3, cap), dtype=torch.int64, device=dev), torch.empty((F, 3, cap), dtype=torch.int64, device=dev),
            torch.empty((F, cap), dtype=torch.int64, device=dev))


def _gt_offsets(gt_off):
    """The host list (F+1) as the C entries take it."""
    return (ctypes.c_int32 * len(gt_off))(*[int(v) for v in gt_off])


def classify_anchors(gts, anchor_bevs, nls, nws, neg_thr, pos_thr, radius, cap=None):
    """One frame of classify_anchors_frames: (pos_idx i64 (3,cap), neg_idx i64 (3,cap), gi i64 (cap,), counts i32 (2,),
    status i32 (1,))."""
    pos, neg, gi, counts, status = classify_anchors_frames(gts, [0, gts.shape[0]], anchor_bevs, nls, nws, neg_thr, pos_thr, radius, cap)
    return pos[0], neg[0], gi[0], counts[0], status


def classify_anchors_frames(gts, gt_off, anchor_bevs, nls, nws, neg_thr, pos_thr, radius, cap=None):
    """The frames of a step in one walk launch: gts (G_total,4,2) of all frames back to back, ``gt_off`` host list (F+1).
    Returns (pos_idx i64 (F,3,cap), neg_idx i64 (F,3,cap), gi i64 (F,cap), counts i32 (F,2), status i32 (1,))."""
    F = len(gt_off) - 1
    L, W, A = anchor_bevs.shape[:3]
    dev = anchor_bevs.device
    wn = 2 * radius + 1
    gmax = max(gt_off[f + 1] - gt_off[f] for f in range(F))
    cap = max(1, gmax * A * wn * wn) if cap is None else int(cap)
    pos, neg, gi = _anchor_lists(F, cap, dev)
    counts = torch.empty((F, 2), dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = workspace(X.lib.mvx_classify_anchors_workspace_bytes(int(gt_off[-1]), A, radius), dev, 'anchors')
    X.call('mvx_classify_anchors_frames', gts, _gt_offsets(gt_off), F, anchor_bevs, L, W, A, nls, nws, float(neg_thr),
           float(pos_thr), int(radius), pos, neg, gi, cap, counts, status, ws, ws.numel())
    return pos, neg, gi, counts, status


def assign_anchors_frames(gts, gt_off, anchor_bevs, neg_thr, pos_thr, force_thr, radius, cap=None):
    """Max-IoU assignment (csrc/assign.hip) of the frames of a step: gts (G_total,4,2) of all frames back to back, ``gt_off`` host
    list (F+1).  Returns (pos_idx i64 (F,3,cap), neg_idx i64 (F,3,cap), gi i64 (F,cap), host = i32 (2F + 1 + G_total): counts
    (F,2), status, then the bits of gt_best f32 (G_total) -- ONE device tensor, so that the caller reads them together)."""
    F = len(gt_off) - 1
    G = int(gt_off[-1])
    L, W, A = anchor_bevs.shape[:3]
    dev = anchor_bevs.device
    wn = 2 * radius + 1
    gmax = max(gt_off[f + 1] - gt_off[f] for f in range(F))
    cap = max(1, min(L * W * A, gmax * A * wn * wn)) if cap is None else int(cap)
    pos, neg, gi = _anchor_lists(F, cap, dev)
    host = torch.zeros((2 * F + 1 + G,), dtype=torch.int32, device=dev)
    counts, status, best = host[:2 * F], host[2 * F:2 * F + 1], host[2 * F + 1:]
    ws = workspace(X.lib.mvx_assign_anchors_frames_workspace_bytes(G, F, L, W, A), dev, 'anchors')
    X.call('mvx_assign_anchors_frames', gts, _gt_offsets(gt_off), F, anchor_bevs, L, W, A, float(neg_thr), float(pos_thr),
           float(force_thr), int(radius), pos, neg, gi, cap, counts, best if G else None, status, ws, ws.numel())
    return pos, neg, gi, host


def box_point_counts_frames(points6, n_points, boxes, gt_off):
    """Points inside every box (csrc/ignore.hip), all frames in one launch and one memset: points6 f32 (F, cap_points, ld),
    n_points i32 (F,), boxes f32 (G_total, 7) xyzlwhr of all frames back to back, gt_off i32 (F+1,), all on the device.
    Returns counts i32 (G_total,).  No host read."""
    F, cap_points, ld = points6.shape
    G = boxes.shape[0]
    assert points6.dtype == boxes.dtype == torch.float32 and n_points.dtype == gt_off.dtype == torch.int32
    assert tuple(n_points.shape) == (F,) and tuple(gt_off.shape) == (F + 1,) and (G == 0 or tuple(boxes.shape) == (G, 7))
    counts = torch.empty((G,), dtype=torch.int32, device=points6.device)
    X.call('mvx_box_point_counts_frames', points6, F, cap_points, ld, n_points, boxes if G else None, gt_off, G,
           counts if G else None)
    return counts


def ignore_anchors_frames(pos, neg, gi, counts, anchors, anchor_bevs, gt_off=None, gt_points=None, min_points=0, rects=None,
                          rect_off=None, img_from_lidar=None, ign_quads=None, ign_off=None, ioa_thr=0.5, cap_out=None, out=None):
    """The ignore pass (csrc/ignore.hip) on the lists of ``assign_anchors_frames``: pos / neg i64 (F,3,cap), gi i64
    (F,cap), counts i32 (2F,) or (F,2); anchors f32 (l,w,A,7) and anchor_bevs f32 (l,w,A,4,2); the sources are optional device
    tensors: gt_points i32 (G_total,) with gt_off i32 (F+1,); rects f32 (R_total,4) with rect_off i32 (F+1,) and img_from_lidar
    f64 (F,3,4); ign_quads f32 (B_total,4,2) with ign_off i32 (F+1,).  ``out``: an i32 device tensor of 6F + 1 words that receives
    counts' (2F), stats (4F) and the status word (zero on entry) -- a slice of the caller's host-read tensor; made here when None.
    Returns (pos' i64 (F,3,cap_out), neg' i64 (F,3,cap_out), gi' i64 (F,cap_out), out).  No host read."""
    F, cap = gi.shape
    L, W, A = anchor_bevs.shape[:3]
    dev = gi.device
    cap_out = L * W * A if cap_out is None else int(cap_out)
    assert pos.dtype == neg.dtype == gi.dtype == torch.int64 and counts.dtype == torch.int32 and counts.numel() == 2 * F
    assert tuple(pos.shape) == tuple(neg.shape) == (F, 3, cap) and anchors.numel() == L * W * A * 7
    assert anchors.dtype == anchor_bevs.dtype == torch.float32
    for t, dt, n in ((gt_off, torch.int32, F + 1), (rect_off, torch.int32, F + 1), (ign_off, torch.int32, F + 1),
                     (img_from_lidar, torch.float64, F * 12)):
        assert t is None or (t.dtype == dt and t.numel() == n)
    assert gt_points is None or gt_points.dtype == torch.int32
    assert (rects is None or rects.dtype == torch.float32) and (ign_quads is None or ign_quads.dtype == torch.float32)
    pos_o = torch.empty((F, 3, cap_out), dtype=torch.int64, device=dev)
    neg_o = torch.empty((F, 3, cap_out), dtype=torch.int64, device=dev)
    gi_o = torch.empty((F, cap_out), dtype=torch.int64, device=dev)
    if out is None:
        out = torch.zeros((6 * F + 1,), dtype=torch.int32, device=dev)
    assert out.dtype == torch.int32 and out.numel() == 6 * F + 1 and out.is_contiguous()
    nbytes = X.lib.mvx_ignore_anchors_frames_workspace_bytes(F, L, W, A)
    ws = workspace(nbytes, dev, 'ignore')
    X.call('mvx_ignore_anchors_frames', pos, neg, gi, cap, counts, F, gt_off, gt_points, int(min_points), anchors, anchor_bevs, L,
           W, A, rects, rect_off, img_from_lidar, ign_quads, ign_off, float(ioa_thr), pos_o, neg_o, gi_o, cap_out, out[:2 * F],
           out[2 * F:6 * F], out[6 * F:], ws, ws.numel())
    return pos_o, neg_o, gi_o, out


def voxel_loss(score, reg, pos_idx, neg_idx, gi, n_pos, n_neg, gts, anchors, A, a, b, eps, want_grads=True,
               dscore_out=None, dreg_out=None):
    """score (L,W,A) / reg (L,W,7A) f32 views with arbitrary strides; pos_idx / neg_idx i64 (3,cap) or None.
    Returns (losses f32 (2,), dscore, dreg) -- the gradients share the inputs' memory layout, or are written into the
    given views ``dscore_out`` / ``dreg_out`` (dreg_out ZERO on entry)."""
    L, W = score.shape[0], score.shape[1]
    dev = score.device
    losses = torch.empty((2,), dtype=torch.float32, device=dev)
    scratch = torch.empty((4,), dtype=torch.float64, device=dev)
    dscore = dscore_out
    if want_grads and dscore is None:
        dscore = torch.empty_strided(score.shape, score.stride(), dtype=torch.float32, device=dev)
    dreg = None
    if want_grads and reg is not None:
        dreg = dreg_out
        if dreg is None:
            dreg = torch.empty_strided(reg.shape, reg.stride(), dtype=torch.float32, device=dev)
            dreg.zero_()
    ss = score.stride()
    rs = reg.stride() if reg is not None else (0, 0, 0)
    ds = dscore.stride() if dscore is not None else (0, 0, 0)
    dr = dreg.stride() if dreg is not None else (0, 0, 0)
    X.call('mvx_voxel_loss', _vptr(score), ss[0], ss[1], ss[2], _vptr(reg), rs[0], rs[1], rs[2], pos_idx,
           pos_idx.shape[1] if pos_idx is not None else 0, neg_idx, neg_idx.shape[1] if neg_idx is not None else 0, gi, None,
           int(n_pos), int(n_neg), gts, gts.shape[1] if gts is not None else 7, anchors, L, W, int(A), float(a), float(b),
           float(eps), _vptr(dscore), ds[0], ds[1], ds[2], _vptr(dreg), dr[0], dr[1], dr[2], losses, scratch)
    return losses, dscore, dreg


def focal_loss_frames(heads, F, l, w, A, pos_idx, neg_idx, gi, counts, gts, gt_off, anchors, alpha, gamma, cls_weight, reg_weight,
                      want_grads=True):
    """Focal loss of all frames of a step in three launches and one memset (csrc/loss_frames.hip).  ``heads`` f32 (F*l*w, 8A)
    contiguous = [A cls logits | 7A regression]; pos_idx / neg_idx i64 (F,3,cap), gi i64 (F,cap), counts i32 (F,2), gts f32
    (n, >= 7) of all frames back to back, gt_off i32 (F+1,) and anchors f32 [l][w][A][7], all on the device.
    Returns (losses f32 (F,2) = (cls, reg) per frame, d_heads in the layout of ``heads`` or None without ``want_grads``)."""
    dev = heads.device
    assert heads.dtype == torch.float32 and tuple(heads.shape) == (F * l * w, 8 * A)
    assert tuple(pos_idx.shape) == tuple(neg_idx.shape) == (F, 3, gi.shape[1]) and tuple(gi.shape) == (F, gi.shape[1])
    assert pos_idx.dtype == neg_idx.dtype == gi.dtype == torch.int64 and counts.dtype == gt_off.dtype == torch.int32
    assert tuple(counts.shape) == (F, 2) and tuple(gt_off.shape) == (F + 1,) and gts.dtype == anchors.dtype == torch.float32
    assert gts.dim() == 2 and gts.shape[0] >= 1 and anchors.numel() == l * w * A * 7
    losses = torch.empty((F, 2), dtype=torch.float32, device=dev)
    d_heads = torch.empty_like(heads) if want_grads else None
    nbytes = X.lib.mvx_focal_loss_frames_workspace_bytes(int(F), int(l), int(w), int(A))
    ws = workspace(nbytes, dev, 'focal_loss')
    X.call('mvx_focal_loss_frames', heads, int(F), int(l), int(w), int(A), pos_idx, neg_idx, gi, gi.shape[1], counts, gts,
           gts.shape[1], gt_off, anchors, float(alpha), float(gamma), float(cls_weight), float(reg_weight), d_heads, losses, ws,
           ws.numel())
    return losses, d_heads


def focal_loss_dir_frames(heads, dir_logits, F, l, w, A, pos_idx, neg_idx, gi, counts, gts, gt_off, anchors, alpha, gamma, cls_weight,
                          reg_weight, dir_weight, dir_offset, want_grads=True, d_heads=None, d_dir=None):
    """Focal loss with the direction classifier and the sine angle term (csrc/loss_frames.hip), the three
    launches and one memset of ``focal_loss_frames``.  ``heads`` f32 (F*l*w, ld) with ld >= 8A a multiple of 4, unit column
    stride: the first 8A columns are [A cls logits | 7A regression]; ``dir_logits`` f32 (F*l*w, A) with any row stride and unit
    column stride -- columns of ``heads`` (``heads[:, 8A:9A]``) or a tensor of its own.  Lists, boxes and anchors as
    ``focal_loss_frames``.  Returns (losses f32 (F,3) = (cls, reg, dir) per frame, d_heads in the layout of ``heads``, d_dir a
    view like ``dir_logits``) -- the gradients None without ``want_grads``.  When ``dir_logits`` is a column range of ``heads``,
    d_dir is the same range of d_heads and every other column beyond 8A is zero; otherwise d_dir is a tensor shaped like
    ``dir_logits``'s storage rows whose A columns are written.  ``d_heads`` / ``d_dir`` (tests): buffers to write instead."""
    dev = heads.device
    rows = F * l * w
    assert heads.dtype == dir_logits.dtype == torch.float32 and heads.dim() == 2 and heads.shape[0] == rows
    assert heads.stride(1) == 1 and heads.shape[1] >= 8 * A and (rows == 1 or heads.stride(0) % 4 == 0)
    assert tuple(dir_logits.shape) == (rows, A) and dir_logits.stride(1) == 1
    assert tuple(pos_idx.shape) == tuple(neg_idx.shape) == (F, 3, gi.shape[1]) and tuple(gi.shape) == (F, gi.shape[1])
    assert pos_idx.dtype == neg_idx.dtype == gi.dtype == torch.int64 and counts.dtype == gt_off.dtype == torch.int32
    assert tuple(counts.shape) == (F, 2) and tuple(gt_off.shape) == (F + 1,) and gts.dtype == anchors.dtype == torch.float32
    assert gts.dim() == 2 and gts.shape[0] >= 1 and anchors.numel() == l * w * A * 7
    ld, dir_ld = heads.stride(0), dir_logits.stride(0)
    losses = torch.empty((F, 3), dtype=torch.float32, device=dev)
    ldd = ld
    if want_grads:
        inside = (dir_ld == ld and 0 <= dir_logits.data_ptr() - heads.data_ptr() <= 4 * (heads.shape[1] - A)
                  and dir_logits.untyped_storage().data_ptr() == heads.untyped_storage().data_ptr())
        if d_heads is None:
            d_heads = torch.empty((rows, heads.shape[1]), dtype=torch.float32, device=dev)
        if d_dir is None:
            if inside:
                c0 = (dir_logits.data_ptr() - heads.data_ptr()) // 4
                d_dir = d_heads[:, c0:c0 + A]
            else:
                d_dir = torch.empty((rows, A), dtype=torch.float32, device=dev)
        assert d_heads.stride(1) == 1 and d_dir.stride(1) == 1 and tuple(d_dir.shape) == (rows, A)
        ldd = d_heads.stride(0)
    else:
        d_heads = d_dir = None
    nbytes = X.lib.mvx_focal_loss_dir_frames_workspace_bytes(int(F), int(l), int(w), int(A), int(ldd))
    ws = workspace(nbytes, dev, 'focal_loss')
    X.call('mvx_focal_loss_dir_frames', _vptr(heads), int(ld), _vptr(dir_logits), int(dir_ld), int(F), int(l), int(w), int(A),
           pos_idx, neg_idx, gi, gi.shape[1], counts, gts, gts.shape[1], gt_off, anchors, float(alpha), float(gamma),
           float(cls_weight), float(reg_weight), float(dir_weight), float(dir_offset), _vptr(d_heads) if want_grads else None,
           int(ldd), _vptr(d_dir) if want_grads else None, int(d_dir.stride(0)) if want_grads else 0, losses, ws, ws.numel())
    return losses, d_heads, d_dir


def _column_range(cols, heads, A):
    """Is ``cols`` (rows, A) a column range of the rows of ``heads``?  -> its first column, or None."""
    off = cols.data_ptr() - heads.data_ptr()
    if (cols.stride(0) == heads.stride(0) and 0 <= off <= 4 * (heads.shape[1] - A)
            and cols.untyped_storage().data_ptr() == heads.untyped_storage().data_ptr()):
        return off // 4
    return None


def focal_loss_iou_frames(heads, dir_logits, iou_logits, F, l, w, A, pos_idx, neg_idx, gi, counts, gts, gt_off, anchors, alpha, gamma,
                          cls_weight, reg_weight, dir_weight, dir_offset, iou_weight, want_grads=True, want_q=False, d_heads=None,
                          d_dir=None, d_iou=None):
    """``focal_loss_dir_frames`` plus the IoU-aware confidence head (csrc/loss_frames.hip): the memset and four
    launches.  ``iou_logits`` f32 (F*l*w, A) with any row stride and unit column stride, like ``dir_logits``: columns of
    ``heads`` (``heads[:, 9A:10A]``) or a tensor of its own.  Returns (losses f32 (F,4) = (cls, reg, dir, iou) per frame,
    d_heads, d_dir, d_iou, q) -- the gradients None without ``want_grads``, d_dir / d_iou column ranges of d_heads when the
    logits are column ranges of ``heads`` and tensors of their own otherwise; q f32 (F, cap) with ``want_q``: the IoU target of
    every pos_idx entry, -1 for skipped entries and unused slots (None otherwise).  ``d_heads`` / ``d_dir`` / ``d_iou``
    (tests): buffers to write instead."""
    dev = heads.device
    rows = F * l * w
    assert heads.dtype == dir_logits.dtype == iou_logits.dtype == torch.float32 and heads.dim() == 2 and heads.shape[0] == rows
    assert heads.stride(1) == 1 and heads.shape[1] >= 8 * A and (rows == 1 or heads.stride(0) % 4 == 0)
    assert tuple(dir_logits.shape) == (rows, A) and dir_logits.stride(1) == 1
    assert tuple(iou_logits.shape) == (rows, A) and iou_logits.stride(1) == 1
    assert tuple(pos_idx.shape) == tuple(neg_idx.shape) == (F, 3, gi.shape[1]) and tuple(gi.shape) == (F, gi.shape[1])
    assert pos_idx.dtype == neg_idx.dtype == gi.dtype == torch.int64 and counts.dtype == gt_off.dtype == torch.int32
    assert tuple(counts.shape) == (F, 2) and tuple(gt_off.shape) == (F + 1,) and gts.dtype == anchors.dtype == torch.float32
    assert gts.dim() == 2 and gts.shape[0] >= 1 and anchors.numel() == l * w * A * 7
    ld, cap = heads.stride(0), gi.shape[1]
    losses = torch.empty((F, 4), dtype=torch.float32, device=dev)
    q = torch.empty((F, cap), dtype=torch.float32, device=dev) if want_q else None
    ldd = ld
    if want_grads:
        if d_heads is None:
            d_heads = torch.empty((rows, heads.shape[1]), dtype=torch.float32, device=dev)

        def grad_of(logits, given):
            if given is not None:
                return given
            c0 = _column_range(logits, heads, A)
            return d_heads[:, c0:c0 + A] if c0 is not None else torch.empty((rows, A), dtype=torch.float32, device=dev)
        d_dir, d_iou = grad_of(dir_logits, d_dir), grad_of(iou_logits, d_iou)
        assert d_heads.stride(1) == 1 and d_dir.stride(1) == 1 and tuple(d_dir.shape) == (rows, A)
        assert d_iou.stride(1) == 1 and tuple(d_iou.shape) == (rows, A)
        ldd = d_heads.stride(0)
    else:
        d_heads = d_dir = d_iou = None
    nbytes = X.lib.mvx_focal_loss_iou_frames_workspace_bytes(int(F), int(l), int(w), int(A), int(ldd), int(cap))
    ws = workspace(nbytes, dev, 'focal_loss')
    X.call('mvx_focal_loss_iou_frames', _vptr(heads), int(ld), _vptr(dir_logits), int(dir_logits.stride(0)), _vptr(iou_logits),
           int(iou_logits.stride(0)), int(F), int(l), int(w), int(A), pos_idx, neg_idx, gi, cap, counts, gts, gts.shape[1], gt_off,
           anchors, float(alpha), float(gamma), float(cls_weight), float(reg_weight), float(dir_weight), float(dir_offset),
           float(iou_weight), _vptr(d_heads) if want_grads else None, int(ldd), _vptr(d_dir) if want_grads else None,
           int(d_dir.stride(0)) if want_grads else 0, _vptr(d_iou) if want_grads else None,
           int(d_iou.stride(0)) if want_grads else 0, q, losses, ws, ws.numel())
    return losses, d_heads, d_dir, d_iou, q


def box_iou_loss_frames(heads, F, l, w, A, pos_idx, gi, counts, gts, gt_off, anchors, weight=1.0, want_grads=True, want_q=False,
                        d_heads=None, loss_add=None):
    """The rotated 3D IoU regression loss ``1 - IoU3D`` of all frames of a step and its analytic gradient in ONE launch, without a
    workspace or a host read (csrc/box_iou_loss.hip).  ``heads`` f32 (F*l*w, >= 8A) with a row stride that is a
    multiple of 4 and unit column stride, the rows ``focal_loss_dir_frames`` reads; lists, boxes and anchors as there (neg_idx
    is not needed).  Per pos_idx entry that is not skipped: q = the 3D IoU of the box the anchor's regression row decodes
    ('loss' decode) with its ground truth, 0 with a zero gradient when they do not overlap or a component is not finite.
    Returns (out f32 (F,2) = (weight / max(1, n_pos) * sum (1 - q), mean q over the entries taken or 0) per frame, d_heads, q):

      * ``want_grads``: the gradient is ADDED into the seven regression columns of the listed anchors of ``d_heads`` (f32, rows of
        any stride >= 8A) -- the tensor the focal call has just written -- and nothing else of it is touched; without a
        ``d_heads`` a zeroed one shaped like ``heads`` is made.  ``want_grads=False``: forward only, d_heads is returned as given.
      * ``loss_add``: f32 view (F,) or (F,1) of any stride, e.g. ``losses[:, 1:2]`` of the focal losses: the frame's term is added
        to it on the device.
      * ``want_q``: q f32 (F, cap), -1 for skipped entries and unused slots (None otherwise).
    ``weight = 0`` leaves ``d_heads`` and ``loss_add`` untouched."""
    dev = heads.device
    rows = F * l * w
    assert heads.dtype == torch.float32 and heads.dim() == 2 and heads.shape[0] == rows
    assert heads.stride(1) == 1 and heads.shape[1] >= 8 * A and (rows == 1 or heads.stride(0) % 4 == 0)
    assert tuple(pos_idx.shape) == (F, 3, gi.shape[1]) and tuple(gi.shape) == (F, gi.shape[1])
    assert pos_idx.dtype == gi.dtype == torch.int64 and counts.dtype == gt_off.dtype == torch.int32
    assert pos_idx.is_contiguous() and gi.is_contiguous() and counts.is_contiguous() and gts.is_contiguous()
    assert tuple(counts.shape) == (F, 2) and tuple(gt_off.shape) == (F + 1,) and gts.dtype == anchors.dtype == torch.float32
    assert gts.dim() == 2 and gts.shape[0] >= 1 and anchors.numel() == l * w * A * 7
    cap = gi.shape[1]
    out = torch.empty((F, 2), dtype=torch.float32, device=dev)
    q = torch.empty((F, cap), dtype=torch.float32, device=dev) if want_q else None
    if want_grads:
        if d_heads is None:
            d_heads = torch.zeros((rows, heads.shape[1]), dtype=torch.float32, device=dev)
        assert d_heads.dtype == torch.float32 and d_heads.dim() == 2 and d_heads.shape[0] == rows and d_heads.shape[1] >= 8 * A
        assert d_heads.stride(1) == 1 and d_heads.device == dev
    add_ld = 0
    if loss_add is not None:
        assert loss_add.dtype == torch.float32 and loss_add.device == dev and loss_add.shape[0] == F and loss_add.numel() == F
        add_ld = loss_add.stride(0) if F > 1 else 1
    X.call('mvx_box_iou_loss_frames', _vptr(heads), int(heads.stride(0)), int(F), int(l), int(w), int(A), pos_idx, gi, cap, counts,
           gts, gts.shape[1], gt_off, anchors, float(weight), _vptr(d_heads) if want_grads else None,
           int(d_heads.stride(0)) if want_grads else 0, _vptr(loss_add), int(add_ld), out, q)
    return out, d_heads, q


# ---------------------------------------------------------------------------------------------
# detection output (csrc/detect.hip)
# ---------------------------------------------------------------------------------------------
DECODE_MODES = {'loss': 0, 'reference': 1}


def detect_frames(cls, reg, anchors, F, l, w, A, score_thr, iou_thr, pre_max, post_max, decode='loss', debug=False, dir_logits=None,
                  dir_offset=math.pi / 4, iou_logits=None, iou_alpha=0.5):
    """Selection, decoding and rotated BEV NMS of F frames in four launches.  ``cls`` / ``reg``: f32 views (F, l, w, A) and
    (F, l, w, 7A) with arbitrary element strides (the frame-set heads or NCHW maps, read in place); anchors f32 [l][w][A][7]
    contiguous on the device.  Returns (boxes (F,post_max,7), scores (F,post_max), anchor_idx i32 (F,post_max), meta i32 (3,F) =
    (kept count, candidates above score_thr, status)) on the device, plus (candidate anchor indices i32 (F,pre_max), decoded
    boxes (F,pre_max,7), corners (F,pre_max,4,2)) with ``debug``.  ``dir_logits``: f32 view (F, l, w, A) of the direction head:
    the decoded yaw is folded into the half turn its sign names, around ``dir_offset``, and wrapped into [-pi, pi)
    (mvx_detect_frames_dir); None is the plain decode (mvx_detect_frames).  ``iou_logits``: f32 view (F, l, w, A) of the IoU head:
    candidates are admitted, ordered and scored by cls^(1-a) iou^a with a = ``iou_alpha`` in [0, 1] (mvx_detect_frames_iou,
    DESIGN.md 3.35); None leaves the score sigmoid(cls)."""
    if decode not in DECODE_MODES:
        raise X.MvxHipError("decode must be 'loss' or 'reference', not %r" % (decode,))
    dev = cls.device
    assert cls.shape == (F, l, w, A) and reg.shape == (F, l, w, 7 * A)
    anchors = anchors.detach().float().contiguous()
    assert anchors.is_cuda and anchors.numel() == l * w * A * 7
    boxes = torch.empty((F, post_max, 7), dtype=torch.float32, device=dev)
    scores = torch.empty((F, post_max), dtype=torch.float32, device=dev)
    idx = torch.empty((F, post_max), dtype=torch.int32, device=dev)
    meta = torch.empty((3, F), dtype=torch.int32, device=dev)          # counts, n_candidates, status
    dbg = (None, None, None)
    if debug:
        dbg = (torch.empty((F, pre_max), dtype=torch.int32, device=dev), torch.empty((F, pre_max, 7), dtype=torch.float32, device=dev),
               torch.empty((F, pre_max, 4, 2), dtype=torch.float32, device=dev))
    nbytes = X.lib.mvx_detect_workspace_bytes(F, l * w * A, pre_max)
    ws = workspace(nbytes, dev, 'detect')
    cs, rs = cls.stride(), reg.stride()
    if iou_logits is not None:
        assert iou_logits.shape == (F, l, w, A) and iou_logits.dtype == torch.float32 and iou_logits.device == dev
        assert dir_logits is None or (dir_logits.shape == (F, l, w, A) and dir_logits.dtype == torch.float32 and dir_logits.device == dev)
        ds, us = dir_logits.stride() if dir_logits is not None else (0, 0, 0, 0), iou_logits.stride()
        X.call('mvx_detect_frames_iou', _vptr(cls), cs[0], cs[1], cs[2], cs[3], _vptr(reg), rs[0], rs[1], rs[2], rs[3],
               _vptr(dir_logits) if dir_logits is not None else None, ds[0], ds[1], ds[2], ds[3], float(dir_offset),
               _vptr(iou_logits), us[0], us[1], us[2], us[3], float(iou_alpha), anchors, int(F), int(l), int(w), int(A),
               float(score_thr), float(iou_thr), int(pre_max), int(post_max), DECODE_MODES[decode], boxes, scores, idx, meta[0],
               meta[1], meta[2], dbg[0], dbg[1], dbg[2], ws, ws.numel())
        out = (boxes, scores, idx, meta)
        return out + dbg if debug else out
    if dir_logits is not None:
        assert dir_logits.shape == (F, l, w, A) and dir_logits.dtype == torch.float32 and dir_logits.device == dev
        ds = dir_logits.stride()
        X.call('mvx_detect_frames_dir', _vptr(cls), cs[0], cs[1], cs[2], cs[3], _vptr(reg), rs[0], rs[1], rs[2], rs[3],
               _vptr(dir_logits), ds[0], ds[1], ds[2], ds[3], float(dir_offset), anchors, int(F), int(l), int(w), int(A),
               float(score_thr), float(iou_thr), int(pre_max), int(post_max), DECODE_MODES[decode], boxes, scores, idx, meta[0],
               meta[1], meta[2], dbg[0], dbg[1], dbg[2], ws, ws.numel())
        out = (boxes, scores, idx, meta)
        return out + dbg if debug else out
    X.call('mvx_detect_frames', _vptr(cls), cs[0], cs[1], cs[2], cs[3], _vptr(reg), rs[0], rs[1], rs[2], rs[3], anchors, int(F),
           int(l), int(w), int(A), float(score_thr), float(iou_thr), int(pre_max), int(post_max), DECODE_MODES[decode], boxes,
           scores, idx, meta[0], meta[1], meta[2], dbg[0], dbg[1], dbg[2], ws, ws.numel())
    out = (boxes, scores, idx, meta)
    return out + dbg if debug else out


# ---------------------------------------------------------------------------------------------
# test-time augmentation: fusion of the views' detections (csrc/tta.hip)
# ---------------------------------------------------------------------------------------------
TTA_MAX_VIEWS, TTA_MAX_BOXES, TTA_NONFINITE = 8, 1024, 2      # MVX_TTA_*


def _arena_bytes(nbytes, dev, tag):
    """A 256-byte aligned byte buffer: carved from the step's arena while one is open, else the grow-only workspace of ``tag``."""
    if _ARENA_ON:
        a = _ARENAS.get(_arena_key(dev))
        v = a.take((int(nbytes) + 7) // 8) if a is not None else None
        if v is not None and v.data_ptr() % 256 == 0:
            return v.view(torch.uint8)
    return workspace(nbytes, dev, tag)


def tta_fuse_frames(boxes, scores, counts, views, F, iou_thr, fuse_iou, min_views, out_max, full_turn):
    """The detections of V views of F source frames -> one list per source frame, three launches (mvx_tta_fuse_frames).
    boxes f32 (F*V, post_max, 7), scores f32 (F*V, post_max), counts i32 (F*V,), frame f*V + v being view v of source frame f;
    views f32 (V, 4) rows (phi, s, flip, 0) on the device.  Returns (boxes (F,out_max,7), scores (F,out_max), n_views i32
    (F,out_max), src i32 (F,out_max) = view * post_max + rank of the cluster's head, meta i32 (2,F) = (counts, status))."""
    dev = boxes.device
    V, post_max = views.shape[0], boxes.shape[1]
    if not 1 <= V <= TTA_MAX_VIEWS or V * post_max > TTA_MAX_BOXES:
        raise X.MvxHipError('the fusion takes 1..%d views and at most %d boxes per source frame, not %d x %d'
                            % (TTA_MAX_VIEWS, TTA_MAX_BOXES, V, post_max))
    assert boxes.shape == (F * V, post_max, 7) and scores.shape == (F * V, post_max) and counts.shape == (F * V,)
    assert views.shape == (V, 4) and boxes.dtype == scores.dtype == views.dtype == torch.float32 and counts.dtype == torch.int32
    out_boxes = torch.empty((F, out_max, 7), dtype=torch.float32, device=dev)
    out_scores = torch.empty((F, out_max), dtype=torch.float32, device=dev)
    n_views = torch.empty((F, out_max), dtype=torch.int32, device=dev)
    src = torch.empty((F, out_max), dtype=torch.int32, device=dev)
    meta = torch.empty((2, F), dtype=torch.int32, device=dev)           # counts, status
    nbytes = X.lib.mvx_tta_workspace_bytes(int(F), int(V), int(post_max))
    ws = _arena_bytes(nbytes, dev, 'tta')
    X.call('mvx_tta_fuse_frames', boxes, scores, counts, views, int(F), int(V), int(post_max), float(iou_thr), float(fuse_iou),
           int(min_views), int(out_max), int(bool(full_turn)), out_boxes, out_scores, n_views, src, meta[0], meta[1], ws, int(nbytes))
    return out_boxes, out_scores, n_views, src, meta


# ---------------------------------------------------------------------------------------------
# KITTI object evaluation (csrc/kitti_eval.hip); ``inp`` is a kitti_eval.EvalInput, ``t`` its device copies
# ---------------------------------------------------------------------------------------------
def _host_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def kitti_eval_overlaps(inp, t):
    """(overlaps f64 (3, n_pairs) = 2D | BEV | 3D, dc_overlaps f64 (n_dc_pairs,)) of every frame."""
    dev = t['off'].device
    ov = torch.empty((3, inp.n_pairs), dtype=torch.float64, device=dev)
    dco = torch.empty((inp.n_dc_pairs,), dtype=torch.float64, device=dev)
    X.call('mvx_kitti_eval_overlaps', inp.F, _host_ptr(inp.off), t['off'], t['pair_off'], t['det_rows'], t['det_quads'],
           t['gt_rows'], t['gt_quads'], t['dc_rows'], ov, dco)
    return ov, dco


def kitti_eval_tp_scores(inp, t, ov):
    """Threshold pass: (TP scores f64 (C, n_slots), -inf in unused slots; valid GTs i32 (C, F))."""
    dev = ov.device
    C = len(inp.keys)
    tp = torch.empty((C, inp.n_slots), dtype=torch.float64, device=dev)
    n_valid = torch.empty((C, inp.F), dtype=torch.int32, device=dev)
    X.call('mvx_kitti_eval_tp_scores', inp.F, _host_ptr(inp.off), t['off'], t['pair_off'], C, _host_ptr(inp.curves),
           _host_ptr(inp.min_overlaps), inp.ignored_gt.shape[0], t['ignored_gt'], t['ignored_det'], t['scores'], ov, tp, n_valid)
    return tp, n_valid


def kitti_eval_thresholds(inp, tp_sorted, n_valid):
    """get_thresholds of every curve from its descending TP scores: (thresholds f64 (C, 41), count i32 (C,), n_gt i32 (C,))."""
    dev = n_valid.device
    C = len(inp.keys)
    thr = torch.empty((C, 41), dtype=torch.float64, device=dev)
    n_thr = torch.empty((C,), dtype=torch.int32, device=dev)
    n_gt = torch.empty((C,), dtype=torch.int32, device=dev)
    X.call('mvx_kitti_eval_thresholds', inp.F, C, inp.n_slots, tp_sorted.contiguous(), n_valid, thr, n_thr, n_gt)
    return thr, n_thr, n_gt


def kitti_eval_counts(inp, t, ov, dco, thr, n_thr):
    """Counting pass summed over the frames: (tp / fp / fn i32 (C, 41, 3), AOS similarity f64 (C, 41))."""
    dev = ov.device
    C = len(inp.keys)
    totals = torch.empty((C, 41, 3), dtype=torch.int32, device=dev)
    sim = torch.empty((C, 41), dtype=torch.float64, device=dev)
    ws = workspace(X.lib.mvx_kitti_eval_workspace_bytes(inp.F, C), dev, 'kitti_eval')
    X.call('mvx_kitti_eval_counts', inp.F, _host_ptr(inp.off), t['off'], t['pair_off'], C, _host_ptr(inp.curves),
           _host_ptr(inp.min_overlaps), inp.ignored_gt.shape[0], t['ignored_gt'], t['ignored_det'], t['scores'], t['det_alpha'],
           t['gt_alpha'], ov, dco, thr, n_thr, totals, sim, ws, ws.numel())
    return totals, sim


# ---------------------------------------------------------------------------------------------
# GT-paste augmentation (csrc/augment.hip); ``db`` is a modules.augment.LoadGT.GTDatabase on the device
# ---------------------------------------------------------------------------------------------
GT_PASTE_MAX_BOXES, GT_PASTE_MAX_CAND, GT_PASTE_MAX_SLOTS = 32, 32, 32      # MVX_GT_PASTE_MAX_*
GT_PASTE_POINTS_OVERFLOW, GT_PASTE_BAD_COUNT, GT_PASTE_SLOTS_SHORT, GT_PASTE_BAD_INDEX = 1, 2, 4, 8


def gt_paste_ground(points6, n_points, range6, grid_shape=(704, 800)):
    """zmax f32 (F, gh, gw): the largest z of the scene points of every x/y cell, (float)(range6[2] - 1) where there is none
    (Augment.py check).  points6 f32 (F, cap, 6), n_points i32 (F,)."""
    F, cap = points6.shape[0], points6.shape[1]
    gh, gw = int(grid_shape[0]), int(grid_shape[1])
    dev = points6.device
    nbytes = X.lib.mvx_gt_paste_workspace_bytes(F, gh, gw)
    zmax = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
    X.call('mvx_gt_paste_ground_frames', points6, n_points, F, cap, float(range6[0]), float(range6[1]), float(range6[2]),
           float(range6[3]), float(range6[4]), gh, gw, zmax, nbytes)
    return zmax[:F * gh * gw].view(F, gh, gw)


def gt_paste_place(zmax, range6, box2d, box3d, bev, n_scene, lim, cand, thr, db, status, cell=0.1, z_margin=0.1, iou_thr=0.05,
                   debug=False):
    """The placement of all frames in one launch.  zmax (F, gh, gw); the scene tables box2d (F, cap, 4), box3d (F, cap, 7),
    bev (F, cap, 4, 2) grow in place; n_scene i32 (F,); cand i32 (F, S, C), thr f32 (F, S); status i32 (F,) is OR-ed into.
    Returns (picked i32 (F, S), n_out i32 (F,)) plus (first failing test i32 (F, S, C), decision values f32 (F, S, C, 3))
    with ``debug``."""
    F, gh, gw = zmax.shape
    cap = box2d.shape[1]
    S, C = cand.shape[1], cand.shape[2]
    dev = zmax.device
    assert box2d.shape == (F, cap, 4) and box3d.shape == (F, cap, 7) and bev.shape == (F, cap, 4, 2)
    assert cand.shape[0] == F and thr.shape == (F, S) and cand.dtype == torch.int32 and thr.dtype == torch.float32
    picked = torch.empty((F, S), dtype=torch.int32, device=dev)
    n_out = torch.empty((F,), dtype=torch.int32, device=dev)
    dbg = (None, None)
    if debug:
        dbg = (torch.empty((F, S, C), dtype=torch.int32, device=dev), torch.empty((F, S, C, 3), dtype=torch.float32, device=dev))
    X.call('mvx_gt_paste_place_frames', zmax, gh, gw, float(range6[0]), float(range6[1]), float(cell), float(z_margin),
           float(iou_thr), box2d, box3d, bev, n_scene, F, cap, int(lim), cand, thr, S, C, db.box2d, db.box3d, db.bev, db.n,
           picked, n_out, status, dbg[0], dbg[1])
    out = (picked, n_out)
    return out + dbg if debug else out


def gt_paste_points(points6, n_points, picked, db, status):
    """Appends the picked objects' rows behind the scene points of every frame (in place); returns the new counts i32 (F,)."""
    F, cap = points6.shape[0], points6.shape[1]
    n_new = torch.empty((F,), dtype=torch.int32, device=points6.device)
    X.call('mvx_gt_paste_points_frames', points6, n_points, n_new, F, cap, picked, picked.shape[1], db.points, db.pt_off, db.n,
           status)
    return n_new


def gt_paste_image(img, picked, db):
    """img u8 (F, H, W, 3) in place: every picked object's patch under its mask, later slots over earlier ones."""
    F, H, W = img.shape[0], img.shape[1], img.shape[2]
    assert img.dtype == torch.uint8 and img.shape[3] == 3
    X.call('mvx_gt_paste_image_frames', img, F, H, W, picked, picked.shape[1], db.patch, db.mask, db.px_off, db.maskbbox, db.n,
           int(db.max_patch_px))
    return img


# ---------------------------------------------------------------------------------------------
# Geometric augmentation (csrc/geom_augment.hip): per-object noise, global rotation / scaling / flip, range filter
# ---------------------------------------------------------------------------------------------
GEOM_MAX_TRIALS, GEOM_BAD_COUNT = 32, 2      # MVX_GEOM_*


class GeomPlaced:
    """Device outputs of geom_place: trial i32 (F, B), move f32 (F, B, 4), box3d f32 (F, B, 7), bev f32 (F, B, 4, 2),
    kept_idx i32 (F, B), n_kept i32 (F,)."""
    __slots__ = ('trial', 'move', 'box3d', 'bev', 'kept_idx', 'n_kept')


def _range6_host(range6):
    import numpy as np
    return np.ascontiguousarray([float(v) for v in range6], dtype=np.float64)


def geom_place(box3d, n_box, noise, glob, range6, status, iou_thr=0.05):
    """The per-object placement, the global step on the boxes and the box filter of all frames in one launch.  box3d f32
    (F, B, 7) (read only), n_box i32 (F,), noise f32 (F, B, T, 4), glob f32 (F, 4); status i32 (F,) is OR-ed into."""
    F, B = box3d.shape[0], box3d.shape[1]
    T = noise.shape[2]
    dev = box3d.device
    assert box3d.shape == (F, B, 7) and noise.shape == (F, B, T, 4) and glob.shape == (F, 4) and n_box.shape == (F,)
    assert box3d.dtype == noise.dtype == glob.dtype == torch.float32 and n_box.dtype == torch.int32
    out = GeomPlaced()
    out.trial = torch.empty((F, B), dtype=torch.int32, device=dev)
    out.move = torch.empty((F, B, 4), dtype=torch.float32, device=dev)
    out.box3d = torch.zeros((F, B, 7), dtype=torch.float32, device=dev)
    out.bev = torch.zeros((F, B, 4, 2), dtype=torch.float32, device=dev)
    out.kept_idx = torch.empty((F, B), dtype=torch.int32, device=dev)
    out.n_kept = torch.empty((F,), dtype=torch.int32, device=dev)
    r = _range6_host(range6)
    X.call('mvx_geom_place_frames', box3d, n_box, F, B, noise, T, glob, float(iou_thr), _host_ptr(r), out.trial, out.move,
           out.box3d, out.bev, out.kept_idx, out.n_kept, status)
    return out


def geom_points(points6, n_points, box3d, n_box, placed, glob, range6):
    """Every point of every frame through the per-object move (membership in the ORIGINAL boxes ``box3d``), the global step
    and the range filter, compacted in order into a new buffer.  Returns (points6 f32 (F, cap, 6), n_points i32 (F,))."""
    F, cap = points6.shape[0], points6.shape[1]
    B = box3d.shape[1]
    dev = points6.device
    assert points6.shape == (F, cap, 6) and points6.dtype == torch.float32 and n_points.dtype == torch.int32
    out = torch.empty_like(points6)
    n_out = torch.empty((F,), dtype=torch.int32, device=dev)
    ws = workspace(X.lib.mvx_geom_workspace_bytes(F, cap), dev, 'geom')
    r = _range6_host(range6)
    with _timed_bytes('geom_points', F * cap * 6 * 4 * 3):
        X.call('mvx_geom_points_frames', points6, n_points, F, cap, box3d, n_box, B, placed.trial, placed.move, glob,
               _host_ptr(r), out, n_out, ws, ws.numel())
    return out, n_out


# ---------------------------------------------------------------------------------------------
# Builder of the GT-paste database (csrc/gtdb.hip); ``t`` holds the device tables of a call (modules.augment.BuildGT.pack):
# lab_box2d / lab_box3d / lab_cs / lab_frame / lab_group, ann_box / ann_off, edges / edge_poly / edge_off, images / im_hw,
# points / pts_off, and the host numbers n_labels, n_frames, max_frame_points
# ---------------------------------------------------------------------------------------------
GTDB_IOU_THR = 0.65
GTDB_CHUNK = 1024           # MVX_GTDB_CHUNK


def gtdb_match(t, iou_thr=GTDB_IOU_THR):
    """Per label: (best i32 (n,), iou f32 (n,), flag i32 (n,), roi i32 (n, 4), px_off i64 (n + 1,)); an object has flag 3."""
    n, dev = t.n_labels, t.lab_box2d.device
    assert t.lab_box2d.shape == (n, 4) and t.lab_box2d.dtype == torch.float32 and t.ann_box.dtype == torch.float32
    assert t.lab_group.dtype == torch.int32 and t.lab_frame.dtype == torch.int32 and t.ann_off.dtype == torch.int32
    assert t.im_hw.shape == (t.n_frames, 2) and t.im_hw.dtype == torch.int32
    best = torch.empty((n,), dtype=torch.int32, device=dev)
    iou = torch.empty((n,), dtype=torch.float32, device=dev)
    flag = torch.empty((n,), dtype=torch.int32, device=dev)
    roi = torch.empty((n, 4), dtype=torch.int32, device=dev)
    px_off = torch.empty((n + 1,), dtype=torch.int64, device=dev)
    X.call('mvx_gtdb_match', t.lab_box2d, t.lab_group, t.lab_frame, n, t.ann_box, t.ann_off, t.ann_off.numel() - 1, t.im_hw,
           t.n_frames, float(iou_thr), best, iou, flag, roi, px_off)
    return best, iou, flag, roi, px_off


def gtdb_crop_count(t, flag):
    """(pt_off i64 (n + 1,), workspace): how many points of its frame every object's box holds, scanned; the workspace keeps
    the chunk offsets for gtdb_crop_write."""
    n, dev = t.n_labels, t.points.device
    assert t.points.dtype == torch.float32 and t.points.shape[1] == 4 and t.pts_off.dtype == torch.int64
    assert t.lab_box3d.shape == (n, 7) and t.lab_cs.shape == (n, 2)
    nbytes = X.lib.mvx_gtdb_workspace_bytes(n, int(t.max_frame_points))
    ws = torch.empty((max(int(nbytes), 256),), dtype=torch.uint8, device=dev)
    pt_off = torch.empty((n + 1,), dtype=torch.int64, device=dev)
    X.call('mvx_gtdb_crop_count', t.points, t.pts_off, t.n_frames, int(t.max_frame_points), t.lab_box3d, t.lab_cs, t.lab_frame,
           flag, n, pt_off, ws, ws.numel())
    return pt_off, ws


def gtdb_crop_write(t, flag, pt_off, ws, n_rows):
    """points f32 (max(n_rows, 1), 4): every object's inside points at pt_off, in file order."""
    out = torch.zeros((max(int(n_rows), 1), 4), dtype=torch.float32, device=t.points.device)
    X.call('mvx_gtdb_crop_write', t.points, t.pts_off, t.n_frames, int(t.max_frame_points), t.lab_box3d, t.lab_cs, t.lab_frame,
           flag, t.n_labels, pt_off, ws, ws.numel(), out, out.shape[0])
    return out


def gtdb_raster(t, best, flag, roi, px_off, n_px, max_roi_rows):
    """(mask u8 (max(n_px, 1),), patch u8 (max(n_px, 1), 3)) of every object at px_off."""
    dev = t.images.device
    F, H, W = t.images.shape[0], t.images.shape[1], t.images.shape[2]
    assert t.images.dtype == torch.uint8 and t.images.shape[3] == 3 and F == t.n_frames
    assert t.edges.dtype == torch.float64 and t.edge_poly.dtype == torch.int32 and t.edge_off.dtype == torch.int32
    mask = torch.zeros((max(int(n_px), 1),), dtype=torch.uint8, device=dev)
    patch = torch.zeros((max(int(n_px), 1), 3), dtype=torch.uint8, device=dev)
    X.call('mvx_gtdb_raster', t.images, F, H, W, t.lab_frame, flag, best, roi, px_off, t.n_labels, t.edges, t.edge_poly,
           t.edge_off, t.edge_off.numel() - 1, max(1, min(int(max_roi_rows), H)), mask, patch, mask.numel())
    return mask, patch


# ---------------------------------------------------------------------------------------------
# Frozen ResNet50-FPN image extractor (csrc/extractor.hip; modules/imhead/Extractor.py chains these with the row GEMMs and the
# conv2d kernels above).  Forward only, channels-last frame sets (F, h, w, C).
# ---------------------------------------------------------------------------------------------
def prepared_size(h, w, min_size=800, max_size=1333, divisor=32):
    """(oh, ow, ph, pw) of torchvision's GeneralizedRCNNTransform in eval mode: the resized size floor(dim * s) with
    s = min(min_size / min(h, w), max_size / max(h, w)) held in float32 (torchvision forms it from float32 tensors and hands
    interpolate its ``.item()``), and that size padded up to multiples of ``divisor``."""
    import numpy as np
    s = float(min(np.float32(min_size) / np.float32(min(h, w)), np.float32(max_size) / np.float32(max(h, w))))
    oh, ow = int(np.floor(float(h) * s)), int(np.floor(float(w) * s))
    up = lambda v: -(-v // divisor) * divisor
    return oh, ow, up(oh), up(ow)


def image_prepare(img, min_size=800, max_size=1333):
    """u8 (F, H, W, 3) or f32 (F, 3, H, W) images -> (normalised, resized, zero-padded f32 (F, ph, pw, 4) with channel 3 zero,
    (oh, ow)) in one launch (mvx_image_prepare_frames)."""
    u8 = img.dtype == torch.uint8
    if u8:
        assert img.dim() == 4 and img.shape[3] == 3
        F, H, W = img.shape[0], img.shape[1], img.shape[2]
    else:
        assert img.dtype == torch.float32 and img.dim() == 4 and img.shape[1] == 3
        F, H, W = img.shape[0], img.shape[2], img.shape[3]
    oh, ow, ph, pw = prepared_size(H, W, min_size, max_size)
    out = torch.empty((F, ph, pw, 4), dtype=torch.float32, device=img.device)
    with _timed_bytes('image_prepare', out.numel() * 4 + img.numel() * img.element_size()):
        X.call('mvx_image_prepare_frames', img, int(u8), out, F, H, W, oh, ow, ph, pw)
    return out, (oh, ow)


def stem_conv7(x4, wpk, bias):
    """ReLU(conv 7x7 / 2 / 3 (3 -> 64) + bias) of the prepared image (F, ph, pw, 4) -> (F, ch, cw, 64); wpk f32 (7, 7, 3, 64)."""
    F, ph, pw = x4.shape[0], x4.shape[1], x4.shape[2]
    assert x4.shape[3] == 4 and wpk.numel() == 49 * 3 * 64 and bias.numel() == 64
    out = torch.empty((F, (ph - 1) // 2 + 1, (pw - 1) // 2 + 1, 64), dtype=torch.float32, device=x4.device)
    with _Timed('stem_conv7', 2.0 * out.numel() * 147 if KERNEL_TIMERS is not None else 0):
        X.call('mvx_stem_conv7_frames', x4, wpk, bias, out, F, ph, pw)
    return out


def maxpool3s2(x):
    """Max pool 3x3 / 2 / 1 of (F, h, w, C)."""
    F, h, w, C = x.shape
    out = torch.empty((F, (h - 1) // 2 + 1, (w - 1) // 2 + 1, C), dtype=torch.float32, device=x.device)
    X.call('mvx_maxpool3s2_frames', x, out, F, h, w, C)
    return out


def add_relu(a, b):
    """ReLU(a + b) of two tensors of the same shape (the bottleneck's skip)."""
    assert a.shape == b.shape
    out = torch.empty_like(a)
    X.call('mvx_add_relu_frames', a, b, out, a.numel())
    return out


def gather_stride2(x):
    """(F, h, w, C) -> its even (y, x) sites (F, ceil(h / 2), ceil(w / 2), C): the rows a 1x1 stride-2 convolution reads."""
    F, h, w, C = x.shape
    out = torch.empty((F, (h - 1) // 2 + 1, (w - 1) // 2 + 1, C), dtype=torch.float32, device=x.device)
    X.call('mvx_gather_stride2_frames', x, out, F, h, w, C)
    return out


def topdown_merge(lateral, top):
    """lateral (F, 2h, 2w, C) + nearest_upsample(top (F, h, w, C)); any other size relation is an error."""
    F, lh, lw, C = lateral.shape
    if top.shape != (F, lh // 2, lw // 2, C) or lh % 2 or lw % 2:
        raise X.MvxHipError('topdown_merge: the lateral map %s is not exactly twice the top map %s' % (tuple(lateral.shape), tuple(top.shape)))
    out = torch.empty_like(lateral)
    X.call('mvx_topdown_merge_frames', lateral, top, out, F, lh, lw, top.shape[1], top.shape[2], C)
    return out


def conv2d_forward_plain(x, wpk, bias, F, h, w, cin, cout, flags, relu, split=False):
    """[ReLU](conv(x) + b) of the conv2d kernels WITHOUT BatchNorm statistics (stats == NULL): the 3x3 layers of a frozen network
    whose BatchNorm is folded into weight and bias."""
    y = torch.empty((F, h, w, cout), dtype=torch.float32, device=x.device)
    fl = (FLAG_RELU if relu else 0) | flags
    with _Timed('extractor_conv', _conv2d_flops(F, h, w, cin, cout, flags)):
        if split:
            X.call('mvx_conv2d_forward_split_frames', x, wpk, bias, y, None, h, w, cin, cout, fl | split_flags(split), F)
        else:
            X.call('mvx_conv2d_forward_frames', x, wpk, bias, y, None, h, w, cin, cout, fl, None, 0.0, None,
                   _work_counter(x.device), F)
    return y


# ---------------------------------------------------------------------------------------------
# Fused AdamW over the flat gradient bucket (csrc/optim.hip; modules/optim.py)
# ---------------------------------------------------------------------------------------------
OPTIM_CHUNK = 4096          # MVX_OPTIM_CHUNK


def optim_adamw_step(table, grad_flat, m_flat, v_flat, count, state, lr, beta1, beta2, eps, weight_decay, max_norm, guard):
    """One guarded, clipped AdamW step on the current stream: norm, prepare and update launches, no host read.  table i64
    (n_chunks, 3) on the device, grad_flat / m_flat / v_flat f32 (n,), count f32 (1,) or None, state f64 (8,)."""
    n = grad_flat.numel()
    dev = grad_flat.device
    assert table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == 3
    assert grad_flat.dtype == m_flat.dtype == v_flat.dtype == torch.float32 and m_flat.numel() == v_flat.numel() == n
    assert state.dtype == torch.float64 and state.numel() == 8 and (count is None or count.dtype == torch.float32)
    ws = workspace(X.lib.mvx_optim_workspace_bytes(n), dev, 'optim')
    with _timed_bytes('optim_adamw', 7 * 4 * n):
        X.call('mvx_optim_adamw_step', table, table.shape[0], grad_flat, m_flat, v_flat, n, count, state, float(lr), float(beta1),
               float(beta2), float(eps), float(weight_decay), float(max_norm), 1 if guard else 0, ws, ws.numel())


# ---------------------------------------------------------------------------------------------
# Frame rendering (csrc/render.hip; modules/render.py).  The draw list of both views: boxes f32 (F, Bcap, 7), n_boxes i32 (F,),
# colors (F, Bcap) = prio << 24 | R << 16 | G << 8 | B, the u32 words carried in an int32 tensor
# ---------------------------------------------------------------------------------------------
RENDER_MAX_SIDE, RENDER_BAD_BOX = 4096, 1      # MVX_RENDER_*
RENDER_COLOR_BY = {'height': 0, 'intensity': 1}


def _render_common(points6, n_points, boxes, n_boxes, colors, lut, H, W):
    F, cap, ld = points6.shape
    dev = points6.device
    assert points6.dtype == torch.float32 and ld >= 6 and n_points.dtype == torch.int32 and n_points.shape == (F,)
    assert lut.dtype == torch.uint8 and lut.shape == (256, 3)
    Bcap = 0 if boxes is None else boxes.shape[1]
    if Bcap:
        assert boxes.shape == (F, Bcap, 7) and boxes.dtype == torch.float32
        assert n_boxes.shape == (F,) and n_boxes.dtype == torch.int32 and colors.shape == (F, Bcap) and colors.dtype == torch.int32
    else:
        boxes = n_boxes = colors = None
    out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    status = torch.empty((F,), dtype=torch.int32, device=dev)
    ws = workspace(X.lib.mvx_render_workspace_bytes(F, H, W), dev, 'render')
    return F, cap, ld, Bcap, boxes, n_boxes, colors, out, status, ws


def render_bev_frames(points6, n_points, boxes, n_boxes, colors, x0, y0, res, z0, z1, H, W, lut, color_by='height', cmax=8,
                      background=0, thickness=1):
    """The bird's-eye view of F frames in three launches: (image u8 (F, H, W, 3) RGB, status i32 (F,)) on the device.
    points6 f32 (F, cap, >= 6), n_points i32 (F,); lut u8 (256, 3); ``background`` = R << 16 | G << 8 | B."""
    if color_by not in RENDER_COLOR_BY:
        raise X.MvxHipError("color_by must be 'height' or 'intensity', not %r" % (color_by,))
    F, cap, ld, Bcap, boxes, n_boxes, colors, out, status, ws = _render_common(points6, n_points, boxes, n_boxes, colors, lut, H, W)
    with _timed_bytes('render_bev', F * (cap * ld * 4 + H * W * 15)):
        X.call('mvx_render_bev_frames', points6, ld, n_points, F, cap, boxes, n_boxes, colors, Bcap, float(x0), float(y0),
               float(res), float(z0), float(z1), int(H), int(W), lut, RENDER_COLOR_BY[color_by], int(cmax),
               int(background) & 0xFFFFFF, int(thickness), out, status, ws, ws.numel())
    return out, status


def render_camera_frames(points6, n_points, boxes, n_boxes, colors, image_from_lidar, H, W, lut_depth, z_near=0.5, depth_max=70.4,
                         point_radius=1, images=None, images_bgr=True, thickness=1):
    """The camera view of F frames in three launches: (image u8 (F, H, W, 3) RGB, status i32 (F,)) on the device.
    image_from_lidar f64 (F, 4, 4) on the device; ``images`` u8 (F, H, W, 3) or None (black)."""
    F, cap, ld, Bcap, boxes, n_boxes, colors, out, status, ws = _render_common(points6, n_points, boxes, n_boxes, colors, lut_depth,
                                                                               H, W)
    assert image_from_lidar.dtype == torch.float64 and image_from_lidar.shape == (F, 4, 4)
    assert images is None or (images.dtype == torch.uint8 and images.shape == (F, H, W, 3))
    with _timed_bytes('render_camera', F * (cap * ld * 4 + H * W * (11 + (3 if images is not None else 0)))):
        X.call('mvx_render_camera_frames', points6, ld, n_points, F, cap, boxes, n_boxes, colors, Bcap, image_from_lidar,
               float(z_near), float(depth_max), int(H), int(W), lut_depth, int(point_radius), images, 1 if images_bgr else 0,
               int(thickness), out, status, ws, ws.numel())
    return out, status
