"""The row BatchNorm (csrc/bn.hip) entry by entry against float64, through the C ABI (mvx_row_stats, mvx_bn_finalize,
mvx_bn_apply_frames, mvx_bn_relu_backward_frames and its planes / parts forms) so that the test chooses flags, scratch and
aliasing itself.  Layouts, operands, the launch geometry and the reference over the dense expansion: tests/bn_rows_cases.py.

Every destination and scratch buffer starts as NaN with NaN behind it; operands carry NaN rows behind the last one.  Afterwards
exactly the result elements differ from NaN.  The statistics handed to the backward are the float64 statistics of y rounded to
f32, the same numbers for kernel and reference, so the errors below are the kernels' own.

Reduction shapes of bn_bwd_reduce / bn_bwd_apply (C/4 = c4 threads per row):
    shuffle   64 % c4 == 0: wave shuffles, four waves through LDS          C = 4, 16, 32, 64, 128, 256
    serial    otherwise: one thread per channel quad walks rpi partials     C = 12, 48, 768
    columns   C > 1024: several column blocks, each serial                  C = 1028
Each case asserts the geometry it names (bn_rows_cases.check_shape, spanning_blocks).

Bounds: 2e-5 of the largest float64 magnitude for mean, inverse deviation, apply and dz, 1e-4 for dbias -- the project's
bounds for these kernels (test_batchnorm_relu_forward_backward, tests/test_conv3d_gpu.py).  Every case prints its error (-s).

Bit-identity claims (PREZEROED, a second call, aliasing, parts) hold because the f64 cross-block sums only reach the result
rounded to f32; with at most 32 blocks every accumulator replica has a single writer and they are deterministic outright.

Largest error per reduction shape, measured on an MI355X in one run of this whole file (dz against its frame's largest float64
magnitude, dbias; the case that gave the dz figure; test_print_measured prints them again):
    shuffle   dz 1.455e-07   dbias 1.052e-06   fusion_empty, C = 128
    serial    dz 8.174e-08   dbias 4.685e-07   single, C = 48, 700 rows
    columns   dz 6.551e-08   dbias 2.003e-07   single, C = 1028, 41 rows
Apply: at most 9.4e-08; mean at most 1.8e-08 and inverse deviation at most 5.8e-11 (mvx_row_stats sums in f64).  Before
mvx_row_stats did, its f32 partials gave the constant channel of test_row_stats_and_finalize an inverse deviation of 920 .. 974
instead of 1000 at eight of the eleven shapes.  The bounds are the project's and were not tightened to these figures."""
import ctypes

import numpy as np
import pytest
import torch

import bn_rows_cases as B

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
GUARD = 64                              # NaN elements behind every destination and scratch buffer
TAIL = 3                                # NaN rows behind every operand

MEASURED = {}                          # this run's largest (dz, dbias, case) per reduction shape: test_print_measured


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _nan(n, dtype=torch.float32):
    return torch.full((n,), NAN, dtype=dtype, device=DEV)


def _rows_buf(a):
    """A device copy of the (rows, C) array with TAIL NaN rows behind it -> (buffer, view)."""
    a = np.asarray(a, np.float32)
    buf = torch.full((a.shape[0] + TAIL,) + a.shape[1:], NAN, device=DEV)
    buf[:a.shape[0]] = torch.from_numpy(a)
    return buf, buf[:a.shape[0]]


def _host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _desc(lay):
    from modules import Extension as X
    if lay.kind == 'single':
        return None, X.ROWS_SINGLE
    kind = {'grid': X.ROWS_GRID, 'real': X.ROWS_REAL, 'voxels': X.ROWS_VOXELS, 'vfe': X.ROWS_VFE, 'fusion': X.ROWS_FUSION}[lay.kind]
    return X.FramesDesc.make(lay.vox_off, lay.real_off, lay.t), kind


def _row_w(lay):
    if lay.kind not in ('vfe', 'fusion'):
        return None
    buf = _nan(lay.rows + 4)
    buf[:lay.rows] = torch.from_numpy(lay.weight.astype(np.float32))
    return buf[:lay.rows]


class Call:
    """The device operands of one (layout, C) and calls of the backward entries on them."""

    def __init__(self, lay, C, seed=0, peak_last=False):
        self.lay, self.C = lay, C
        self.y_h, self.g_h, self.mi_h = B.operands(lay, C, seed=seed, peak_last=peak_last)
        _, self.y = _rows_buf(self.y_h)
        _, self.g = _rows_buf(self.g_h)
        self.mi = torch.from_numpy(self.mi_h).to(DEV).contiguous()
        self.row_w = _row_w(lay)
        self.desc, self.kind = _desc(lay)
        self.count = float(lay.rows) if lay.kind == 'single' else 1.0
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = B.bn_relu_backward(self.lay, self.g_h, self.y_h, self.mi_h)
        return self._ref

    def scratch(self, zero=False):
        from modules import Extension as X
        nbytes = X.lib.mvx_bn_backward_scratch_bytes_frames(self.C, self.lay.F)
        assert nbytes % 8 == 0
        s = _nan(nbytes // 8 + GUARD, torch.float64)
        if zero:
            s[:nbytes // 8] = 0
        return s, nbytes // 8

    def backward(self, flags=0, dbias_fill=NAN, alias=False, scratch=None, planes=False, amax=True, dbias=True):
        """One call of mvx_bn_relu_backward_frames (planes: ..._planes_frames).  -> dz (rows, C) f32 (planes: int16 (3, rows, C)),
        dbias (C,), amax (float or None), the scratch; guards are checked here."""
        from modules import Extension as X
        lay, C = self.lay, self.C
        n = lay.rows * C
        if alias:
            dzbuf = _nan(n + GUARD)
            dzbuf[:n] = self.g.reshape(-1)
            src = dzbuf
        else:
            dzbuf = _nan((3 * n + 1) // 2 + GUARD) if planes else _nan(n + GUARD)
            src = self.g
        dbbuf = _nan(C + GUARD)
        dbbuf[:C] = dbias_fill
        ambuf = _nan(1 + GUARD)
        sc, sn = self.scratch() if scratch is None else scratch
        fn = X.lib.mvx_bn_relu_backward_planes_frames if planes else X.lib.mvx_bn_relu_backward_frames
        rc = fn(_p(src), _p(self.y), _p(self.mi), self.count, _p(dzbuf), _p(dbbuf) if dbias else None, _p(sc), _p(self.row_w), lay.rows,
                C, flags, self.desc.ref() if self.desc is not None else None, self.kind, _p(ambuf) if amax else None, X.stream())
        torch.cuda.synchronize()
        assert rc == 0, 'returned %d' % rc
        assert torch.isnan(sc[sn:]).all() and torch.isnan(dbbuf[C:]).all() and torch.isnan(ambuf[1:]).all()
        if planes:
            pl = dzbuf.view(torch.int16)
            assert torch.isnan(dzbuf[(3 * n + 1) // 2:]).all()
            dz = pl[:3 * n].view(3, lay.rows, C)
        else:
            assert torch.isnan(dzbuf[n:]).all()
            dz = dzbuf[:n].view(lay.rows, C)
        if lay.rows:
            assert not torch.isnan(sc[:sn]).any(), 'part of the scratch was never written'
        return dz, dbbuf[:C], (float(ambuf[0]) if amax else None), sc

    def check(self, tag, dz, db, shape=None):
        """dz of every frame and dbias against float64; rows that stand for no dense row are exactly 0."""
        ref_dz, ref_db = self.ref()
        dzh = _host(dz)
        none = self.lay.weight == 0
        assert (dzh[none] == 0).all(), tag + ': a row that stands for no dense row is not exactly zero'
        assert np.isfinite(dzh).all(), tag + ': dz is not finite'
        live = ~none
        errs = []
        for f in range(self.lay.F):                   # every frame against its OWN largest magnitude
            r = self.lay.frame_rows(f)
            r = r[live[r]]
            if len(r):
                errs.append(float(np.abs(dzh[r] - ref_dz[r]).max() / np.abs(ref_dz[r]).max()))
        e_dz = max(errs)
        e_db = B.rel(_host(db), ref_db) if db is not None else 0.0
        print('%s: dz vs float64 %.3e (per frame %s), dbias %.3e' % (tag, e_dz, ' '.join('%.2e' % e for e in errs), e_db))
        assert e_dz < B.BOUND, tag
        assert e_db < B.BOUND_DBIAS, tag
        if shape is not None:
            old = MEASURED.get(shape, (0.0, 0.0, ''))
            MEASURED[shape] = (max(old[0], e_dz), max(old[1], e_db), tag if e_dz > old[0] else old[2])
        return e_dz, e_db


def _planes_to_f32(pl):
    hi, mid, lo = (pl[q].view(torch.bfloat16).float() for q in range(3))
    return (hi + mid) + lo


_CALLS = {}


def _call(kind, C):
    if (kind, C) not in _CALLS:
        _CALLS[(kind, C)] = Call(B.layout(kind), C)
    return _CALLS[(kind, C)]


# ---- statistics ------------------------------------------------------------------------------------------------------------
def _stats(y, rows, C, frames=None):
    from modules import _hip
    from modules import Extension as X
    F = frames or 1
    per = _hip.STATS_REPLICAS * 2 * C * F
    st = _nan(per + GUARD, torch.float64)
    if frames is None:
        rc = X.lib.mvx_row_stats(_p(y), _p(st), rows, C, X.stream())
    else:
        rc = X.lib.mvx_row_stats_frames(_p(y), _p(st), rows, C, F, X.stream())
    torch.cuda.synchronize()
    return rc, st, per


def _finalize(st, count, C, F=1):
    from modules import Extension as X
    mi = _nan(F * 2 * C + GUARD)
    rc = X.lib.mvx_bn_finalize_frames(_p(st), float(count), B.EPS, _p(mi), C, F, X.stream())
    torch.cuda.synchronize()
    assert rc == 0 and torch.isnan(mi[F * 2 * C:]).all()
    return mi[:F * 2 * C].view(F, 2, C)


@pytest.mark.parametrize('s', B.C_TABLE, ids=B.shape_id)
def test_row_stats_and_finalize(s):
    """mvx_row_stats + mvx_bn_finalize over all rows as one frame: mean and inverse deviation against float64.  Channel 0 holds one
    value in every row (E[y^2] - mean^2 cancels completely): its inverse deviation is 1 / sqrt(eps) to the bound.  C = 1028:
    mvx_row_stats_frames refuses it with the argument error, mvx_row_stats computes it."""
    rows, C = s.per * s.F, s.C
    rng = np.random.default_rng(11 * C + rows)
    y = (rng.standard_normal((rows, C)) * 1.5 + 0.7).astype(np.float32)
    y[:, 0] = np.float32(3.7)                                  # not a dyadic number: the sums are not exact in f32
    if C >= 8:
        y[:, 5] = 0.0                                          # what a dead ReLU channel looks like
    _, yd = _rows_buf(y)
    rc, st, per = _stats(yd, rows, C)
    assert rc == 0 and torch.isnan(st[per:]).all() and not torch.isnan(st[:per]).any()
    mi = _host(_finalize(st, rows, C))[0]
    ref = B.bn_forward(B.single(rows), y)[0]
    assert abs(ref[1, 0] - 1.0 / np.sqrt(B.EPS)) < 1e-9
    e_m, e_i = B.rel(mi[0], ref[0]), B.rel(mi[1], ref[1])
    e_c = abs(mi[1, 0] - ref[1, 0]) / ref[1, 0]
    print('%s: mean %.3e, inverse deviation %.3e (constant channel: %.6g, off by %.3e)' % (B.shape_id(s), e_m, e_i, mi[1, 0], e_c))
    assert e_m < B.BOUND and e_i < B.BOUND and e_c < B.BOUND
    if C > 1024:
        rc, st2, _ = _stats(yd, rows, C, frames=1)
        assert rc < 0 and torch.isnan(st2).all(), 'mvx_row_stats_frames must refuse C > 1024 without writing'


# ---- apply -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', B.KIND_C)
@pytest.mark.parametrize('kind', B.KINDS)
def test_apply_uses_the_statistics_of_the_rows_frame(kind, C):
    from modules import Extension as X
    c = _call(kind, C)
    lay, n = c.lay, c.lay.rows * C
    out = _nan(n + GUARD)
    d = c.desc.ref() if c.desc is not None else None
    assert X.lib.mvx_bn_apply_frames(_p(c.y), _p(c.mi), _p(out), lay.rows, C, d, c.kind, X.stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out[n:]).all()
    ref = B.apply(lay, c.y_h, c.mi_h)
    err = B.rel(_host(out[:n]).reshape(lay.rows, C), ref)
    print('apply %s C %d: vs float64 %.3e' % (kind, C, err))
    assert err < B.BOUND
    inpl = _nan(n + GUARD)
    inpl[:n] = c.y.reshape(-1)
    assert X.lib.mvx_bn_apply_frames(_p(inpl), _p(c.mi), _p(inpl), lay.rows, C, d, c.kind, X.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(inpl[:n], out[:n]) and torch.isnan(inpl[n:]).all()


# ---- backward: the C table on SINGLE and GRID ----------------------------------------------------------------------------------
@pytest.mark.parametrize('s', B.C_TABLE, ids=B.shape_id)
def test_backward_c_table(s):
    """dz and dbias (into a NaN dbias: overwritten) of every reduction shape; the amax slot is max |dz| of the returned tensor."""
    g = B.check_shape(s)
    lay = B.table_layout(s)
    if s.F > 1:
        assert B.spanning_blocks(lay, s.C) >= 1
    c = Call(lay, s.C)
    dz, db, amax, _ = c.backward()
    c.check('%s %s (%s, %d blocks)' % (lay.kind, B.shape_id(s), g.shape, g.blocks), dz, db, shape=g.shape)
    assert amax == float(dz.abs().max())


# ---- backward: every layout kind -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', B.KIND_C)
@pytest.mark.parametrize('kind', B.KINDS)
def test_backward_every_kind(kind, C):
    """F = 3 (SINGLE: 1) with a block that spans two segments; dz per frame, dbias over the frames, rows that stand for no dense
    row exactly 0; the amax slot; PREZEROED with a scratch zeroed here, a second call on a used scratch and dz aliasing dyhat
    repeat the first call bit for bit; ACCUMULATE adds to 0.5."""
    from modules import _hip
    c = _call(kind, C)
    lay = c.lay
    g = B.geometry(lay.rows, C)
    if kind != 'single':
        assert lay.F == 3 and B.spanning_blocks(lay, C) >= 1
    if kind in ('vfe', 'fusion'):
        assert c.row_w is not None and lay.weight.max() > 1
    if kind == 'vfe':
        assert (lay.weight == 0).sum() >= 5
    dz, db, amax, sc = c.backward()
    c.check('%s C %d' % (kind, C), dz, db, shape=g.shape)
    assert amax == float(dz.abs().max())
    # a second call on the scratch the first one left behind
    dz2, db2, amax2, _ = c.backward(scratch=(sc, sc.numel() - GUARD))
    assert torch.equal(dz2, dz) and torch.equal(db2, db) and amax2 == amax
    dz3, db3, _, _ = c.backward(flags=_hip.FLAG_PREZEROED, scratch=c.scratch(zero=True))
    assert torch.equal(dz3, dz) and torch.equal(db3, db)
    dz4, db4, amax4, _ = c.backward(alias=True)
    assert torch.equal(dz4, dz) and torch.equal(db4, db) and amax4 == amax
    dz5, db5, _, _ = c.backward(flags=_hip.FLAG_ACCUMULATE, dbias_fill=0.5)
    assert torch.equal(dz5, dz)
    c.check('%s C %d accumulate' % (kind, C), dz5, db5 - 0.5)
    # no dbias asked for: dz all the same
    dz6, db6, _, _ = c.backward(dbias=False, amax=False)
    assert torch.equal(dz6, dz) and torch.isnan(db6).all()


@pytest.mark.parametrize('s', [B.C_TABLE[2], B.C_TABLE[4], B.C_TABLE[8]], ids=B.shape_id)
def test_amax_of_a_maximum_in_the_last_partial_trip(s):
    """The largest |dz| sits in the last row, which the last block reaches in a trip that the end of the matrix cuts short."""
    lay = B.table_layout(s)
    assert B.last_trip_is_partial(lay.rows, s.C)
    c = Call(lay, s.C, seed=5, peak_last=True)
    dz, db, amax, _ = c.backward()
    c.check('peak in the last row %s' % B.shape_id(s), dz, db)
    assert int(dz.abs().max(1).values.argmax()) == lay.rows - 1
    assert amax == float(dz.abs().max())


@pytest.mark.parametrize('accumulate', [False, True])
def test_backward_without_rows(accumulate):
    """rows == 0: dz untouched, dbias zero (or unchanged under ACCUMULATE), the amax slot zero."""
    from modules import _hip
    from modules import Extension as X
    C = 16
    y, g, dz = _nan(C), _nan(C), _nan(C)
    mi = torch.ones((2 * C,), device=DEV)
    before = torch.arange(C, dtype=torch.float32, device=DEV) - 3.5
    db = _nan(C + GUARD)
    db[:C] = before if accumulate else NAN
    am = _nan(1 + GUARD)
    nb = X.lib.mvx_bn_backward_scratch_bytes_frames(C, 1) // 8
    sc = _nan(nb + GUARD, torch.float64)
    rc = X.lib.mvx_bn_relu_backward_frames(_p(g), _p(y), _p(mi), 1.0, _p(dz), _p(db), _p(sc), None, 0, C,
                                           _hip.FLAG_ACCUMULATE if accumulate else 0, None, X.ROWS_SINGLE, _p(am), X.stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.isnan(dz).all() and torch.isnan(db[C:]).all() and torch.isnan(sc[nb:]).all() and torch.isnan(am[1:]).all()
    assert torch.equal(db[:C], before if accumulate else torch.zeros_like(before))
    assert float(am[0]) == 0.0


# ---- planes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,C', [('grid', 16), ('fusion', 128), ('vfe', 16), ('real', 128)])
def test_planes_sum_to_dz_and_meet_float64(kind, C):
    """mvx_bn_relu_backward_planes_frames: hi + mid + lo, three bf16 pieces, against float64 directly, and equal to the f32 entry
    bit for bit (the pieces carry the whole f32)."""
    c = _call(kind, C)
    pl, db, amax, _ = c.backward(planes=True)
    dz = _planes_to_f32(pl)
    c.check('planes %s C %d' % (kind, C), dz, db)
    dz32, db32, amax32, _ = c.backward()
    assert torch.equal(dz, dz32) and torch.equal(db, db32) and amax == amax32


@pytest.mark.parametrize('s', [B.C_TABLE[2], B.C_TABLE[8]], ids=B.shape_id)
def test_planes_in_parts(s):
    """mvx_bn_relu_backward_planes_part_frames with nparts in {1, 2, 7, blocks + 3}: the ranges tile [0, rows) in order (with more
    parts than blocks some are empty and launch nothing), the planes are those of the one-pass form bit for bit, rows outside the
    ranges written so far are untouched, dbias is complete after the last part."""
    from modules import Extension as X
    g = B.check_shape(s)
    lay = B.table_layout(s)
    c = Call(lay, s.C, seed=6)
    whole, db_whole, _, _ = c.backward(planes=True)
    c.check('one pass %s' % B.shape_id(s), _planes_to_f32(whole), db_whole)
    n = lay.rows * s.C
    for nparts in (1, 2, 7, g.blocks + 3):
        buf = torch.full((3 * n + 2 * GUARD,), -1, dtype=torch.int16, device=DEV)
        dbbuf = _nan(s.C + GUARD)
        sc, sn = c.scratch()
        rng = (ctypes.c_int64 * 2)()
        at, empty = 0, 0
        for part in range(nparts):
            rc = X.lib.mvx_bn_relu_backward_planes_part_frames(_p(c.g), _p(c.y), _p(c.mi), c.count, _p(buf), _p(dbbuf), _p(sc), None,
                                                               lay.rows, s.C, 0, c.desc.ref() if c.desc is not None else None,
                                                               c.kind, part, nparts, rng, X.stream())
            torch.cuda.synchronize()
            assert rc == 0
            lo, hi = int(rng[0]), int(rng[1])
            assert lo == at and hi >= lo and hi <= lay.rows, (nparts, part, lo, hi)
            assert lo % g.rpb == 0 and (hi % g.rpb == 0 or hi == lay.rows)
            empty += hi == lo
            at = hi
            got = buf[:3 * n].view(3, lay.rows, s.C)
            assert torch.equal(got[:, :hi], whole[:, :hi]), (nparts, part)
            assert (got[:, hi:] == -1).all(), 'part %d of %d wrote rows behind its range' % (part, nparts)
        assert at == lay.rows
        assert (empty > 0) == (nparts > g.blocks)
        assert (buf[3 * n:] == -1).all() and torch.isnan(dbbuf[s.C:]).all() and torch.isnan(sc[sn:]).all()
        assert torch.equal(dbbuf[:s.C], db_whole)
        print('parts %s nparts %d: %d empty, planes and dbias equal to one pass' % (B.shape_id(s), nparts, empty))


# ---- a frame without voxels in the fusion layout ---------------------------------------------------------------------------------
@pytest.mark.parametrize('C', B.KIND_C)
def test_fusion_frame_without_voxels(C):
    """MVX_ROWS_FUSION stores the shared padded row of every frame, also of one without voxels: population 0, weight 0.  With
    finite statistics supplied for that frame, positive y and zero dyhat on that row, its dz is exactly 0, dz of the live frames
    and dbias meet the float64 bound, and nothing is NaN (bn_bwd_reduce: a frame with population 0 gets a = b = 0)."""
    c = _call('fusion_empty', C)
    lay = c.lay
    row = lay.real_off[-1] + 1
    assert lay.pop[1] == 0 and lay.weight[row] == 0 and lay.frame[row] == 1
    assert (c.y_h[row] > 0).all() and (c.g_h[row] == 0).all() and np.isfinite(c.mi_h[1]).all()
    dz, db, amax, sc = c.backward()
    assert not torch.isnan(dz).any() and not torch.isnan(db).any(), 'NaN from a frame without population'
    assert (dz[row] == 0).all()
    c.check('fusion, middle frame without voxels, C %d' % C, dz, db)
    pl, db2, _, _ = c.backward(planes=True)
    assert torch.equal(_planes_to_f32(pl), dz) and torch.equal(db2, db)


def test_print_measured():
    """Last in the file: the largest errors per reduction shape of this run (-s)."""
    for shape, (e_dz, e_db, tag) in sorted(MEASURED.items()):
        print('%-8s dz %.3e  dbias %.3e  (%s)' % (shape, e_dz, e_db, tag))
