"""CPU-only checks: the C-ABI library loads and exports every symbol that include/mvx_hip.h
declares (no compute calls without a GPU), the ctypes table mirrors the header, the host-side
configuration / sharding logic, and the product path never imports the oracle."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import abi_header

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = abi_header.HEADER


def test_library_exports_every_declared_symbol():
    from modules import Extension as X
    lib = ctypes.CDLL(X.LIB_PATH)
    names = sorted(abi_header.declarations())
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), 'libmvx_hip.so lacks %s declared in include/mvx_hip.h' % n
    assert set(names) == set(X.PROTOTYPES), set(names) ^ set(X.PROTOTYPES)
    assert lib.mvx_abi_version() == X.ABI_VERSION


def test_argument_counts_match_header():
    """Every entry of the prototype table against the header: the same names, and per name the result type and the whole list
    of argument types (a pointer is c_void_p, ``int`` is int32_t)."""
    from modules import Extension as X
    decl = abi_header.declarations()
    assert set(decl) == set(X.PROTOTYPES), set(decl) ^ set(X.PROTOTYPES)
    for name, (res, args) in X.PROTOTYPES.items():
        assert len(decl[name][1]) == len(args), (name, len(decl[name][1]), len(args))
        assert decl[name][0] is res, (name, decl[name][0], res)
        assert abi_header.parameter_types(name) == list(args), name


def test_every_call_site_names_an_entry_point_that_ends_in_the_stream():
    """Extension.call appends the stream itself: every entry point _hip.py reaches through it takes ``void *stream`` last."""
    src = open(os.path.join(REPO, 'mvxnet-makise_amd', 'modules', '_hip.py')).read()
    names = re.findall(r"X\.call\('(mvx_\w+)'", src)
    assert names and len(re.findall(r'X\.call\(', src)) == len(names)                      # no call with a computed name
    from modules import Extension as X
    decl = abi_header.declarations()
    for name in sorted(set(names)):
        assert decl[name][1][-1] == ('stream', ctypes.c_void_p), name
        assert decl[name][0] is ctypes.c_int32, name                                         # a status for Extension.check
        fn, pointers = X._LAUNCHES[name]                                                     # the helper's own table agrees
        assert list(pointers) == [i for i, (_, t) in enumerate(decl[name][1][:-1]) if t is ctypes.c_void_p], name
        assert fn.argtypes == X.PROTOTYPES[name][1] and fn.restype is ctypes.c_int32, name


def test_no_cpu_fallback_and_loud_failure():
    from modules import Extension as X
    with pytest.raises(X.MvxHipError):
        X.ptr(torch.zeros(4))                      # CPU tensor -> refused, never silently computed
    if not torch.cuda.is_available():
        with pytest.raises(X.MvxHipError):
            X.device()
    # size queries are pure host code and must work without a GPU
    assert X.lib.mvx_voxelize_workspace_bytes(2, 20000) > 0
    assert X.lib.mvx_conv3d_packed_weight_bytes(64, 128) == 27 * 64 * 128 * 4
    assert X.lib.mvx_conv3d_wgrad_workspace_bytes(352, 400, 128, 64) > 0
    # argument validation happens before any launch
    assert X.lib.mvx_voxelize(None, None, None, None, 1, 10, 4, 0., 0., 0., 1., 1., 1., 35, 9, 10,
                              None, None, None, None, None, None, 0, None) == -1


# (h, w, cin, cout, n_frames) -> bytes of mvx_conv3d_wgrad_workspace_bytes(h, w, cin, cout),
# mvx_conv3d_wgrad_bg_workspace_bytes_frames(dout = 3, h, w, cin, cout, n_frames) and
# mvx_conv2d_wgrad_workspace_bytes_frames(h, w, cin, cout, n_frames).  The values are those of the library BEFORE the
# convolution files shared their host scaffold (csrc/conv_geom.h), recorded once by calling that build; ragged h x w (no
# multiples of the 8 x 16 tile), every channel count of the network, and the shapes each query rejects (0).
CONV_WORKSPACE_BYTES = {
    (11, 37, 64, 64, 1): (2654208, 56623336, 56623216),
    (11, 37, 64, 64, 4): (2654208, 56623984, 56623504),
    (9, 17, 128, 64, 1): (3538944, 56623264, 113246288),
    (50, 44, 128, 256, 4): (74317824, 0, 113247568),
    (25, 22, 256, 256, 1): (56623104, 0, 113246352),
    (19, 35, 256, 64, 4): (15925248, 56624416, 113246800),
    (352, 400, 128, 64, 4): (75202560, 56781520, 113316624),
    (352, 400, 64, 64, 1): (69894144, 56662720, 56640720),
    (176, 200, 128, 256, 4): (254803968, 0, 113264528),
    (9, 17, 32, 64, 1): (884736, 0, 0),
    (9, 17, 33, 64, 1): (912384, 0, 0),
    (9, 17, 64, 32, 1): (0, 0, 0),
    (9, 17, 64, 128, 1): (3538944, 0, 113246288),
    (0, 17, 64, 64, 1): (0, 0, 0),
    (9, 17, 64, 64, 0): (1769472, 0, 0),
}


def test_conv_wgrad_workspace_sizes_are_those_of_the_separate_copies():
    from modules import Extension as X
    for (h, w, cin, cout, nf), want in CONV_WORKSPACE_BYTES.items():
        got = (X.lib.mvx_conv3d_wgrad_workspace_bytes(h, w, cin, cout),
               X.lib.mvx_conv3d_wgrad_bg_workspace_bytes_frames(3, h, w, cin, cout, nf),
               X.lib.mvx_conv2d_wgrad_workspace_bytes_frames(h, w, cin, cout, nf))
        assert got == want, ((h, w, cin, cout, nf), got, want)
    assert X.lib.mvx_conv3d_wgrad_bg_workspace_bytes(3, 11, 37, 64, 64) == CONV_WORKSPACE_BYTES[(11, 37, 64, 64, 1)][1]
    assert X.lib.mvx_conv3d_wgrad_bg_workspace_bytes_frames(0, 11, 37, 64, 64, 1) == 0


# every convolution entry point that launches a gather or a weight gradient: f32 and split, 3-D and 2-D
CONV_ENTRY_POINTS = (
    'mvx_conv3d_forward', 'mvx_conv3d_forward_bg', 'mvx_conv3d_forward_bg_frames', 'mvx_conv3d_dgrad', 'mvx_conv3d_dgrad_tiles',
    'mvx_conv3d_dgrad_tiles_frames', 'mvx_conv3d_wgrad', 'mvx_conv3d_wgrad_bg', 'mvx_conv3d_wgrad_bg_frames',
    'mvx_conv2d_forward_frames', 'mvx_conv2d_dgrad_frames', 'mvx_conv2d_wgrad_frames',
    'mvx_conv3d_forward_split', 'mvx_conv3d_forward_bg_split', 'mvx_conv3d_forward_bg_split_frames', 'mvx_conv3d_dgrad_split',
    'mvx_conv3d_dgrad_tiles_split', 'mvx_conv3d_dgrad_tiles_split_frames', 'mvx_conv2d_forward_split_frames',
    'mvx_conv2d_dgrad_split_frames')
# one bad argument each -> the parameter it needs (a function without it is not called with that case), the code.  The
# codes are those the library returned BEFORE the shared geometry check (recorded once from that build, for every pair of
# entry point and case below): MVX_ESIZE (-2) for a channel granule, MVX_EINVAL (-1) for everything else.
CONV_BAD_ARGUMENTS = (
    ('cin', 33, -2), ('stride_d', 3, -1), ('pad_d', 2, -1), ('h', 0, -1), ('n_frames', 0, -1), ('n_frames', 17, -1),
    ('dout', 5, -1))


def test_conv_entry_points_reject_bad_geometry_before_any_launch():
    """Dummy non-null pointers and ONE bad argument: the call must come back with the argument error -- a launch on these
    pointers would fault, and without a GPU it would return a HIP error instead.  `dout = 5` is wrong for the forward
    convolutions only (din = 4, stride 1, padding 1 -> 4); the gradients take any dout."""
    from modules import Extension as X
    dummy = (ctypes.c_double * 64)()
    good = dict(din=4, dout=4, h=9, w=17, cin=64, cout=64, stride_d=1, pad_d=1, flags=0, n_frames=1, border_active=0,
                count=1.0, eps=1e-5, workspace_bytes=1 << 40, stream=None)
    calls = 0
    for name in CONV_ENTRY_POINTS:
        names = abi_header.parameter_names(name)
        assert len(names) == len(X.PROTOTYPES[name][1])
        for param, value, code in CONV_BAD_ARGUMENTS:
            if param not in names or (param == 'dout' and 'forward' not in name):
                continue
            args = [value if n == param else good[n] if n in good else ctypes.addressof(dummy) for n in names]
            assert getattr(X.lib, name)(*args) == code, (name, param, value)
            calls += 1
    assert calls == 96
    # the frame-set form of the closed-form input-gradient term has no channel granule: frame count only
    for nf in (0, 17):
        assert X.lib.mvx_conv3d_input_grad_sums_frames(ctypes.addressof(dummy), ctypes.addressof(dummy), 4, 4, 64, 64, 1, 1,
                                                       ctypes.addressof(dummy), nf, None) == -1


# (rows, k, n) -> bytes of mvx_linear_splitk_workspace_bytes(rows, n), mvx_linear_wgrad_workspace_bytes(rows, k, n),
# mvx_linear_wgrad_pre_workspace_bytes(rows, k, n) and mvx_split_planes_bytes(rows, k, flags) for the flags MVX_FLAG_SPLIT3,
# MVX_FLAG_SPLIT_F16 and MVX_FLAG_SPLIT alone (no piece format: 0).  The values are those of the library BEFORE the row GEMMs
# shared their host helpers (csrc/rowgemm_common.h), recorded once by calling that build.
ROWGEMM_WORKSPACE_BYTES = {
    (0, 23, 16): (0, 256, 0, 0, 0, 0),
    (0, 128, 128): (0, 256, 0, 0, 0, 0),
    (0, 768, 768): (0, 256, 0, 0, 0, 0),
    (0, 768, 128): (0, 256, 0, 0, 0, 0),
    (37, 23, 16): (37888, 1472, 4416, 5106, 3404, 0),
    (37, 128, 128): (303104, 65536, 196608, 28416, 18944, 0),
    (37, 768, 768): (1818624, 2359296, 7077888, 170496, 113664, 0),
    (37, 768, 128): (303104, 393216, 1179648, 170496, 113664, 0),
    (4099, 23, 16): (4197376, 48576, 189888, 565662, 377108, 0),
    (4099, 128, 128): (33579008, 2162688, 8454144, 3148032, 2098688, 0),
    (4099, 768, 768): (201474048, 77856768, 61341696, 18888192, 12592128, 0),
    (4099, 768, 128): (33579008, 12976128, 25559040, 18888192, 12592128, 0),
    (80000, 23, 16): (81920000, 736000, 368000, 11040000, 7360000, 0),
    (80000, 128, 128): (655360000, 32768000, 16384000, 61440000, 40960000, 0),
    (80000, 768, 768): (3932160000, 99090432, 66060288, 368640000, 245760000, 0),
    (80000, 768, 128): (655360000, 36569088, 33423360, 368640000, 245760000, 0),
}


def test_rowgemm_workspace_sizes_are_those_of_the_separate_copies():
    from modules import Extension as X
    for (rows, k, n), want in ROWGEMM_WORKSPACE_BYTES.items():
        got = (X.lib.mvx_linear_splitk_workspace_bytes(rows, n), X.lib.mvx_linear_wgrad_workspace_bytes(rows, k, n),
               X.lib.mvx_linear_wgrad_pre_workspace_bytes(rows, k, n), X.lib.mvx_split_planes_bytes(rows, k, 128),
               X.lib.mvx_split_planes_bytes(rows, k, 512), X.lib.mvx_split_planes_bytes(rows, k, 64))
        assert got == want, ((rows, k, n), got, want)


# every mvx_linear_* entry point and mvx_split_rows -> the pointers it cannot do without
ROWGEMM_ENTRY_POINTS = {
    'mvx_linear_forward': ('x', 'w', 'y'),
    'mvx_linear_forward_bn': ('x', 'w', 'y', 'stats', 'done_counter', 'mean_inv'),
    'mvx_linear_forward_bn_frames': ('x', 'w', 'y', 'stats', 'done_counter', 'mean_inv', 'frames_host'),
    'mvx_linear_wgrad': ('x', 'dz', 'dw', 'workspace'),
    'mvx_split_rows': ('x', 'planes'),
    'mvx_linear_forward_pre_frames': ('a_planes', 'b_planes', 'y'),
    'mvx_linear_wgrad_pre': ('x_planes', 'dz_planes', 'dw', 'workspace'),
    'mvx_linear_wgrad_pre_rows': ('x_planes', 'dz_planes', 'dw', 'workspace'),
}
# one bad argument each (after a null for every pointer above): k = 0, a leading dimension below the row length, a k that is
# no multiple of the DMA step (the entry points on pre-cut planes only: the others take it), an empty row range
ROWGEMM_BAD_ARGUMENTS = (('k', 0), ('ldx', 8), ('ldy', 8), ('lddz', 8), ('k', 40), ('row_hi', 0))


def test_rowgemm_entry_points_reject_a_bad_argument_before_any_launch():
    """As for the convolutions: 64-byte-aligned dummy pointers, a valid one-frame descriptor, MVX_FLAG_PREZEROED (no memset
    either) and ONE bad argument.  Every code is MVX_EINVAL (-1), which is what the library returned for each of these
    pairs BEFORE the row GEMMs shared their argument checks and stats preamble (recorded once from that build).  Not covered:
    whether a check comes before or after the clearing of the sums -- with MVX_FLAG_PREZEROED nothing is cleared, and without it
    a rejected call and a failed memset on these host pointers could not be told apart by a code that differs per machine."""
    from modules import Extension as X
    buf = ctypes.create_string_buffer(4096 + 64)
    dummy = (ctypes.addressof(buf) + 63) & ~63
    fr = X.FramesDesc()
    fr.n_frames, fr.t = 1, 1
    fr.real_off[1] = fr.vox_off[1] = 256
    good = dict(ldx=64, ldw=64, w_transposed=0, ldy=64, lddz=64, rows=256, k=64, n=64, flags=2 | 128, splitk_workspace_bytes=0,
                count=1.0, eps=1e-5, scale=1.0, out_scale=1.0, workspace_bytes=1 << 40, plane_rows=256, row_lo=0, row_hi=256,
                frames_host=ctypes.addressof(fr), row_kind=5, stream=None)
    calls = 0
    for name, pointers in ROWGEMM_ENTRY_POINTS.items():
        names = abi_header.parameter_names(name)
        assert len(names) == len(X.PROTOTYPES[name][1])
        for param, value in tuple((p, None) for p in pointers) + ROWGEMM_BAD_ARGUMENTS:
            if param not in names or ((param, value) == ('k', 40) and 'pre' not in name):
                continue
            args = [value if q == param else good[q] if q in good else dummy for q in names]
            assert getattr(X.lib, name)(*args) == -1, (name, param, value)
            calls += 1
    assert calls == 55
    assert sorted(n for n in X.PROTOTYPES if n.startswith('mvx_linear_') and X.PROTOTYPES[n][0] is ctypes.c_int32) == \
        sorted(n for n in ROWGEMM_ENTRY_POINTS if n != 'mvx_split_rows')


def test_product_path_never_imports_the_oracle():
    pkg = os.path.join(REPO, 'mvxnet-makise_amd')
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h')):
                src = open(os.path.join(root, f)).read()
                assert 'mvx_oracle' not in src and 'liboracle' not in src and 'oracle/' not in src, f


def test_only_hip_py_names_the_c_entry_points():
    """Every kernel call of the package has ONE Python wrapper, in modules/_hip.py (Extension.py loads the library): no other
    file of the package names an ``X.lib.mvx_*`` function."""
    import re as _re
    pkg = os.path.join(REPO, 'mvxnet-makise_amd')
    raw = []
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py') and f not in ('_hip.py', 'Extension.py'):
                src = open(os.path.join(root, f)).read()
                raw += ['%s: %s' % (os.path.relpath(os.path.join(root, f), pkg), m) for m in _re.findall(r'lib\.mvx_\w+', src)]
    assert not raw, raw


def test_config_surface():
    import modules.config as cfg
    assert cfg.voxelshape == [352, 400, 10] and cfg.samplenum == 35
    assert cfg.voxelsize == [0.2, 0.2, 0.4]            # exactly the reference's doubles (Config.py:7)
    assert cfg.eps == 1e-6 and cfg.dtype == torch.float32
    with pytest.raises(AttributeError):
        cfg.no_such_key


def test_arithmetic_selection_logic():
    """Host side of `convmath` (modules/_hip.py): config value -> split code -> flag bits of a call; which row GEMMs take the
    split arithmetic; the fall-backs of fp16x3 for operands without a range tag.  No GPU involved."""
    import re as _re
    import modules.config as cfg
    from modules import _hip
    header = open(HEADER).read()
    for name, val in (('MVX_FLAG_SPLIT', _hip.FLAG_SPLIT), ('MVX_FLAG_SPLIT3', _hip.FLAG_SPLIT3), ('MVX_FLAG_SPLIT_F16', _hip.FLAG_SPLIT_F16),
                      ('MVX_FLAG_AMAX_COARSE', _hip.FLAG_AMAX_COARSE), ('MVX_FLAG_NO_BG_FILL', _hip.FLAG_NO_BG_FILL)):
        assert int(_re.search(r'#define %s (\d+)' % name, header).group(1)) == val, name
    assert cfg.config['convmath'] == os.environ.get('MVX_CONVMATH', 'bf16x6')   # the shipped default: operand-exact (config.yml:2 half: False)
    old = cfg.config['convmath']
    try:
        codes = {}
        for math, code in (('f32', 0), ('bf16x3', 2), ('bf16x6', 3), ('fp16x3', 4)):
            cfg.config['convmath'] = math
            assert _hip.split_pieces() == code
            codes[math] = {t: _hip.row_split(t) for t in ('fusion_768x768', 'vfe', 'conv1', 'rpn', 'dgrad', 'wgrad')}
        assert set(codes['f32'].values()) == {0}
        assert codes['bf16x3'] == {'fusion_768x768': 0, 'vfe': 0, 'conv1': 0, 'rpn': 2, 'dgrad': 2, 'wgrad': 2}    # forward rows stay exact f32
        assert set(codes['bf16x6'].values()) == {3} and set(codes['fp16x3'].values()) == {4}
        cfg.config['convmath'] = 'fp8'
        with pytest.raises(Exception):
            _hip.split_pieces()
    finally:
        cfg.config['convmath'] = old
    assert _hip.split_flags(0) == 0 and _hip.split_flags(2) == 0 and _hip.split_flags(2, True) == _hip.FLAG_SPLIT
    assert _hip.split_flags(3) == _hip.FLAG_SPLIT3 and _hip.split_flags(3, True) == _hip.FLAG_SPLIT | _hip.FLAG_SPLIT3
    assert _hip.split_flags(4) == _hip.FLAG_SPLIT_F16 and _hip.split_flags(4, True) == _hip.FLAG_SPLIT | _hip.FLAG_SPLIT_F16
    t = torch.zeros(4)
    assert _hip.amax_of(t) is None
    assert _hip.grad_split(4, t) == 3 and _hip.grad_split(3, t) == 3 and _hip.grad_split(0, t) == 0      # untagged gradient: bf16x6
    assert _hip.foreign_split(4, t) == (3, 0) and _hip.foreign_split(2, t) == (2, 0)                       # untagged foreign input: bf16x6
    _hip.tag_amax(t, torch.ones(1))
    assert _hip.grad_split(4, t) == 4 and _hip.foreign_split(4, t) == (4, _hip.FLAG_AMAX_COARSE)
    assert _hip.amax_of(t.view(2, 2)) is None                  # a view does not carry the tag (callers re-tag)


def test_weight_copies_follow_the_parameter():
    """The cached derived copies of a weight (zero-padded columns for rows written with a 4-float pitch, the row-major
    transpose for the input-gradient GEMMs) are remade when the parameter changes -- optimizer step, load_state_dict -- and die
    with it (they live in the parameter's __dict__)."""
    import torch
    from modules import _hip
    w = torch.nn.Parameter(torch.arange(16 * 23, dtype=torch.float32).reshape(16, 23))
    p1 = _hip.padded_weight(w, 24)
    assert p1.shape == (16, 24) and torch.equal(p1[:, :23], w.detach()) and float(p1[:, 23].abs().max()) == 0.0
    assert _hip.padded_weight(w, 24) is p1                       # cached
    assert _hip.padded_weight(w, 23) is w                        # nothing to pad
    t1 = _hip.transposed_weight(w)
    assert torch.equal(t1, w.detach().t())
    with torch.no_grad():
        w.add_(1.0)                                              # an in-place update bumps the version counter
    p2, t2 = _hip.padded_weight(w, 24), _hip.transposed_weight(w)
    assert p2 is not p1 and torch.equal(p2[:, :23], w.detach()) and torch.equal(t2, w.detach().t())


def test_2d_blocks_never_fall_to_torch_silently():
    """a stand-alone CRB2d / DeCRB2d on a CPU tensor raises (this package has no CPU path); the torch /
    MIOpen form only runs where the caller chose it (RPN.forward_torch, `crb2d_hip: false`) or with a RuntimeWarning."""
    import modules.config as cfg
    from modules.Extension import MvxHipError
    from modules.layers import CRB2d, DeCRB2d
    from modules.layers import Blocks
    x = torch.randn(1, 64, 8, 8)
    for m in (CRB2d(64, 64, 3, 1, 1), DeCRB2d(64, 64, 3, 1, 1)):
        with pytest.raises(MvxHipError):
            m(x)
        old = cfg.config.get('crb2d_hip', True)
        cfg.config['crb2d_hip'] = False                       # the explicit opt-out: torch modules, no complaint
        try:
            assert m(x).shape == (1, 64, 8, 8)
        finally:
            cfg.config['crb2d_hip'] = old
        Blocks._IN_FORWARD_TORCH[0] = True                    # the comparison path of the tests
        try:
            assert m(x).shape == (1, 64, 8, 8)
        finally:
            Blocks._IN_FORWARD_TORCH[0] = False


def test_state_dict_keys_and_param_counts():
    from MVXNet import MVXNet
    m = MVXNet()
    sd = m.state_dict()
    assert sum(p.numel() for k, p in sd.items() if k.startswith('backbone.')) == 6670608
    assert sum(p.numel() for k, p in sd.items() if k.startswith('head.fusion.')) == 707872
    assert 'head.fusion.conv1.conv.weight' in sd and sd['head.fusion.conv1.conv.weight'].shape == (128, 768, 1, 1)


def test_shard_frames_partition():
    from modules.parallel import shard_frames
    for world in (1, 2, 4, 8):
        got = sorted(sum((shard_frames(16, r, world) for r in range(world)), []))
        assert got == list(range(16))


def test_synthetic_frames_are_deterministic():
    from modules.data import Synthetic as S
    a, b = S.synth_uniform(5, 2000), S.synth_uniform(5, 2000)
    assert np.array_equal(a, b) and a.dtype == np.float32
    lo, hi = np.array(S.VELORANGE[:3]), np.array(S.VELORANGE[3:])
    assert np.all(a[:, :3] >= lo) and np.all(a[:, :3] < hi)
    assert sorted(S.synth_perm(3, 100).tolist()) == list(range(100))


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return str(sk.getsockname()[1])


@pytest.mark.parametrize('mode,world', [('toy', 2), ('chunks', 2), ('model', 2), ('model', 8)])
def test_data_parallel_gradient_exchange_gloo(mode, world):
    """CPU processes over gloo.  toy: the flat bucket all-reduce gives the mean over all frames.  model (world 2 and the
    north_star's world 8): the real GradBucket over MVXNet's 1,169,440 hot-path parameters in its two-part layout
    [early | late | count] with DIFFERENT per-frame gradients on every rank, exchanged by the two-part branch, equals the
    single-process sum over all frames, and the replicas stay identical after AdamW."""
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=_free_port(), OMP_NUM_THREADS='1')
    worker = os.path.join(REPO, 'tests', '_dp_worker.py')
    procs = [subprocess.Popen([sys.executable, worker, mode], env=dict(env, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert 'DP_OK' in o, o
