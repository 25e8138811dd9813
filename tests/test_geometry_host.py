"""CPU only: the two references of tests/geometry_ref.py are tied to each other on the inputs of tests/geometry_cases.py (the GPU
tests compare the kernels with the second, bit for bit), the inputs are what they claim, every edge row is decided as listed by
both layers, and the argument checks of csrc/geometry.hip return before any launch."""
import ctypes

import numpy as np
import pytest

import geometry_cases as K
import geometry_ref as R

CALIBS = ('kitti', 'generic')
ARITH = ((1, np.float32), (0, np.float64))


@pytest.fixture(scope='module')
def ld():
    """The plain statement needs the 80-bit longdouble."""
    if not np.finfo(np.longdouble).eps < 1e-18:
        pytest.skip('numpy.longdouble is no wider than float64 here (eps %g): the plain statement has no headroom'
                    % np.finfo(np.longdouble).eps)


def live_rows(c):
    return np.concatenate([c.pcd[f, :K.live(c, f), :3] for f in range(c.F)])


# ---- (b) against (a) -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cal', CALIBS)
@pytest.mark.parametrize('name', K.CLOUD_NAMES)
def test_kernel_order_restatement_lies_within_the_derived_bound_of_the_plain_statement(name, cal, ld):
    c, cb = K.cloud(name), K.calib(cal)
    xyz = live_rows(c)
    for math_f32, T in ARITH:
        m, p2, lims = R.as_type(cb.m, T), R.as_type(cb.p2, T), R.limits(cb.imsize_wh, math_f32)
        ex = R.exact(xyz, m, p2, lims)
        bz, bu, bv = R.bounds(ex, T)
        z, u, v = R.project(xyz, cb.m, cb.p2, T)
        ez, eu, ev = (np.abs(a.astype(R.LD) - b) for a, b in ((z, ex.z), (u, ex.u), (v, ex.v)))
        assert (ez <= bz).all()
        fin = np.isfinite(bu)
        assert (eu[fin] <= bu[fin]).all() and (ev[fin] <= bv[fin]).all()
        sure_in, sure_out = R.sure(ex, bz, bu, bv, lims)
        kept = R.sight_keep(xyz, cb.m, cb.p2, cb.imsize_wh, math_f32)
        assert kept[sure_in].all() and not kept[sure_out].any()
        undecided = ~(sure_in | sure_out)
        assert undecided.mean() <= 0.01, 'a condition on the inputs: at most 1 % of a case may lie inside the band'
        deep = np.asarray(ex.z > 0.5) & fin
        print('%-8s %-7s %s: bound of u at depth > 0.5 m up to %.3g px, measured |du| %.3g |dv| %.3g px, |dz| %.3g m '
              '(bound %.3g); largest error / bound %.3g; undecided %d of %d (%.2f %%)'
              % (name, cal, T.__name__, float(bu[deep].max()), float(eu[deep].max()), float(ev[deep].max()), float(ez.max()),
                 float(bz.max()), float(max((eu[fin] / bu[fin]).max(), (ev[fin] / bv[fin]).max(), (ez / bz).max())),
                 undecided.sum(), len(xyz), 100 * undecided.mean()))
    # the range test rounds nothing: equal on every point, whichever way the bounds are rounded
    for bounds_f32 in (0, 1):
        ex = R.exact(xyz, range6=R.bounds6(K.RANGE, bounds_f32))
        assert np.array_equal(ex.range_mask, R.range_keep(xyz, K.RANGE, bounds_f32))


def test_the_oracle_of_the_existing_tests_agrees_with_the_restatement(ld):
    """mvx_oracle's crop / crop_to_sight masks (matrix products, another order) on a cloud: the same decisions as (b) outside the
    band; and (b)'s range mask is the oracle's."""
    import mvx_oracle as O
    c, cb = K.cloud('c1000one'), K.calib('kitti')
    xyz = c.pcd[0]
    for bounds_f32 in (0, 1):
        assert np.array_equal(O.crop_mask(xyz, list(K.RANGE), bool(bounds_f32)), R.range_keep(xyz[:, :3], K.RANGE, bounds_f32))
    for math_f32, T in ARITH:
        lims = R.limits(cb.imsize_wh, math_f32)
        ex = R.exact(xyz[:, :3], R.as_type(cb.m, T), R.as_type(cb.p2, T), lims)
        sure_in, sure_out = R.sure(ex, *R.bounds(ex, T), lims)
        got = O.crop_to_sight_mask(xyz, O.KITTI_CALIB, cb.imsize_wh, T)
        assert got[sure_in].all() and not got[sure_out].any()


# ---- the inputs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cal', CALIBS)
@pytest.mark.parametrize('name', K.CLOUD_NAMES)
def test_every_filter_rejects_a_real_share(name, cal):
    c, cb = K.cloud(name), K.calib(cal)
    xyz = live_rows(c)
    assert c.pcd.shape == (c.F, c.cap, c.ncol) and c.pcd.dtype == np.float32
    r = R.range_keep(xyz, K.RANGE, 0)
    for math_f32, _ in ARITH:
        s = R.sight_keep(xyz, cb.m, cb.p2, cb.imsize_wh, math_f32)
        for label, kept in (('range', r), ('sight', s), ('both', r & s)):
            assert 0.05 <= kept.mean() <= 0.95, (label, kept.mean())
        assert (r & ~s).any() and (s & ~r).any(), 'each filter alone rejects points the other keeps'
    print('%-8s %-7s keeps %.0f %% (range) %.0f %% (sight) %.0f %% (both) of %d' % (name, cal, 100 * r.mean(), 100 * s.mean(),
                                                                                   100 * (r & s).mean(), len(xyz)))


@pytest.mark.parametrize('name', [n for n in K.CLOUD_NAMES if K.cloud(n).n_in is not None])
def test_rows_beyond_n_in_would_pass(name, ld):
    c = K.cloud(name)
    assert (c.n_in > c.cap).any() if name == 'c257' else (c.n_in == 0).any(), 'one entry above cap, or an empty frame'
    seen = 0
    for f in range(c.F):
        tail = c.pcd[f, K.live(c, f):, :3]
        seen += len(tail)
        for cal in CALIBS:
            cb = K.calib(cal)
            for math_f32, T in ARITH:
                assert R.keep(tail, K.RANGE, math_f32, cb.m, cb.p2, cb.imsize_wh, math_f32).all()
                lims = R.limits(cb.imsize_wh, math_f32)
                ex = R.exact(tail, R.as_type(cb.m, T), R.as_type(cb.p2, T), lims, K.RANGE)
                assert R.sure(ex, *R.bounds(ex, T), lims)[0].all() and ex.range_mask.all()
    assert seen > 100


def test_columns_past_xyz_name_their_place():
    for name in K.CLOUD_NAMES:
        c = K.cloud(name)
        extra = c.pcd[..., 3:]
        assert len(np.unique(extra)) == extra.size
        rows = c.pcd.reshape(-1, c.ncol)
        assert len(np.unique(rows, axis=0)) == len(rows), 'no two rows alike: a row copied from the wrong source is seen'
    assert sorted({K.cloud(n).cap for n in K.CLOUD_NAMES}) == [1, 255, 256, 257, 300, 1000]
    assert {K.cloud(n).ncol for n in K.CLOUD_NAMES} == {3, 4, 6} and {K.cloud(n).F for n in K.CLOUD_NAMES} == {1, 3}


def test_calibrations_differ_where_a_swap_must_show():
    k, g, d = K.calib('kitti'), K.calib('generic'), K.calib('dyadic')
    rot = g.m[:3, :3]
    assert np.allclose(rot @ rot.T, np.eye(3), atol=1e-14) and (np.abs(rot) > 0.03).all(), 'a rotation aligned with no axis'
    assert g.p2[0, 0] != g.p2[1, 1] and g.p2[0, 0] != k.p2[0, 0] and g.imsize_wh != k.imsize_wh
    # the dyadic one: every entry 0 or a power of two in magnitude
    for a in (d.m, d.p2):
        nz = np.abs(a[a != 0])
        assert np.array_equal(np.log2(nz), np.round(np.log2(nz)))
    # the real pairing: the f32-formed product differs from the f64 product rounded to f32, and so do the columns it gives
    k32 = K.f32_formed(k)
    assert (R.as_type(k.m, np.float32) != k32.m).any() and np.array_equal(k32.m, R.as_type(k32.m, np.float32))
    rel = np.abs(k.m - k32.m)[:3].max() / np.abs(k.m[:3]).max()
    assert 0 < rel < 1e-6
    xyz = K.cloud('c1000one').pcd[0, :, :3]
    a, _ = R.lidar2img(xyz, k.m, k.p2, 1, 1)
    b, _ = R.lidar2img(xyz, k32.m, k32.p2, 1, 1)
    differ = (a != b).any(1)
    kept = R.keep(xyz, K.RANGE, 0, k.m, k.p2, k.imsize_wh, 0)
    assert (differ & kept).sum() >= 5, 'a swap of the two matrix sets changes appended columns of kept rows'
    print('f32-formed product: relative difference %.2g; %d of %d kept rows get other columns' % (rel, (differ & kept).sum(), kept.sum()))


# ---- the edge rows -----------------------------------------------------------------------------------------------------------------
def test_the_f32_and_f64_limits_lie_as_the_edge_rows_assume():
    f = np.float32
    for w in (2, 16, 370):
        assert float(f(w) - f(1e-3)) < w - 1e-3
    for w in (64, 128, 1224):
        assert float(f(w) - f(1e-3)) > w - 1e-3
    assert R.limits((16, 370), 1) == (float(K.LIM_W32), float(K.LIM_H32))
    assert float(f(70.2)) < 70.2 and float(f(-39.9)) < -39.9 and float(f(70.4)) > 70.4
    assert K.STEP == 2.0 ** -149
    # formed in f64 and then rounded to f32, the limit is the f32-formed one for every integer size ...
    assert all(f(w - 1e-3) == f(w) - f(1e-3) for w in range(2, 2049))
    # ... but one step above it for the sizes of 'dyadic_frac', which round to 16 and 370 and leave every edge row where it is
    for w, lim32 in zip(K.FRAC_WH, (K.LIM_W32, K.LIM_H32)):
        assert f(w) == f(round(w)) and f(w) - f(1e-3) == lim32 and f(w - 1e-3) == np.nextafter(lim32, f(np.inf))
        assert float(lim32) < w - 1e-3 < float(np.nextafter(lim32, f(np.inf)))             # python floats: compared in f64
    assert R.limits(K.FRAC_WH, 1) == R.limits((16, 370), 1) and R.limits(K.FRAC_WH, 0) != R.limits((16, 370), 0)


def margin_ok(got, want, limit):
    step = float(np.spacing(np.float32(abs(limit)) if limit else np.float32(0)))
    if want is None:
        return True
    if want == 'ulp':
        return float(got) == step
    if want == 'sub':
        return 0 < float(got) < step
    return float(got) == want


@pytest.mark.parametrize('cal', ['dyadic', 'dyadic_frac'])
def test_every_edge_row_is_decided_as_listed_by_both_layers(cal, ld):
    c, cb = K.edges(), K.calib(cal)
    xyz = c.pcd[0, :, :3]
    assert np.array_equal(xyz[np.isfinite(xyz)].astype(np.float64), np.array([v for e in K.EDGES for v in e.xyz if np.isfinite(v)]))
    differ = {'s': 0, 'r': 0}
    for k, (math_f32, T) in enumerate(ARITH):              # k: 0 = the f32 column of the table, 1 = the f64 one
        lims = R.limits(cb.imsize_wh, math_f32)
        ex = R.exact(xyz, R.as_type(cb.m, T), R.as_type(cb.p2, T), lims, R.bounds6(K.EDGE_RANGE, math_f32))
        z, u, v = R.project(xyz, cb.m, cb.p2, T)
        fin = np.isfinite(xyz).all(1) & np.array(['s' in e.filt for e in K.EDGES])
        # the dyadic calibration at depth 0, one step and 1 (the rows of the sight filter): (b) equals (a) exactly
        for a, b in ((z, ex.z), (u, ex.u), (v, ex.v)):
            assert np.array_equal(a[fin].astype(R.LD), b[fin])
        sight_b = R.sight_keep(xyz, cb.m, cb.p2, cb.imsize_wh, math_f32)
        range_b = R.range_keep(xyz, K.EDGE_RANGE, math_f32)
        limit_of = (0.0, 0.0, 0.0, lims[0], lims[1])
        for i, e in enumerate(K.EDGES):
            want = (e.keep_f32, e.keep_f64)[k]
            if 's' in e.filt:
                assert sight_b[i] == want and ex.sight_mask[i] == want, (e.name, T.__name__)
            if 'r' in e.filt:
                assert range_b[i] == want and ex.range_mask[i] == want, (e.name, T.__name__)
            if e.margin is not None:
                if e.quantity is None:
                    assert margin_ok(ex.range_margin[i], e.margin[k], np.abs(xyz[i]).max()), (e.name, T.__name__)
                else:
                    assert margin_ok(ex.sight_margin[i, e.quantity], e.margin[k], limit_of[e.quantity]), (e.name, T.__name__)
    for e in K.EDGES:
        if e.keep_f32 != e.keep_f64:
            differ[e.filt] += 1
    assert differ == {'s': 2, 'r': 2}, 'u and v at the f32 limit; x at f32(hi) and y at f32(lo)'
    # non-finite rows: dropped by each filter alone, in each arithmetic, under the random calibrations as well
    bad = ~np.isfinite(xyz).all(1)
    assert bad.sum() == 6
    for other in (cal,) + CALIBS:
        cc = K.calib(other)
        for flag in (0, 1):
            assert not R.sight_keep(xyz, cc.m, cc.p2, cc.imsize_wh, flag)[bad].any()
            assert not R.range_keep(xyz, K.EDGE_RANGE, flag)[bad].any()


# ---- argument checks: rejected before any launch -----------------------------------------------------------------------------------
CANARY = -777.25


def test_geometry_entry_points_reject_bad_arguments_before_any_launch():
    """HOST buffers on the canary stand for pcd, out, n_out and the workspace, ONE bad argument per call; the complete valid
    combination is never passed.  A rejected call returns -1 and the buffers still hold the canary; a launch on these pointers
    would fault, and without a GPU it would return a HIP error instead."""
    from modules import Extension as X
    lib = X.lib
    F, cap, ncol = 2, 300, 4
    out = np.full((F * cap * (ncol + 2),), CANARY, np.float32)
    n_out = np.full((F,), -7, np.int32)
    pcd = np.zeros((F * cap * ncol,), np.float32)
    need = lib.mvx_crop_workspace_bytes(F, cap)
    assert need == lib.mvx_crop_project_workspace_bytes(F, cap) == F * 2 * 4
    ws = np.zeros((need,), np.uint8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    k = K.calib('kitti')
    m, p2, rng = (np.ascontiguousarray(a, np.float64) for a in (k.m, k.p2, K.RANGE))

    def crop(ncol=ncol, rng=p(rng), m=p(m), p2=p(p2), nbytes=need, F=F, cap=cap, out=p(out), n_out=p(n_out), pcd=p(pcd)):
        return lib.mvx_crop_points(pcd, None, F, cap, ncol, rng, 0, m, p2, 1224.0, 370.0, 0, out, n_out, None, p(ws), nbytes, None)

    def crop_project(ncol=ncol, rng=p(rng), m=p(m), p2=p(p2), pm=p(m), pp=p(p2), nbytes=need, cap_out=cap, F=F, cap=cap):
        return lib.mvx_crop_project_points(p(pcd), None, F, cap, ncol, rng, m, p2, 1224.0, 370.0, pm, pp, p(out), cap_out, p(n_out),
                                           p(ws), nbytes, None)

    def l2i(ncol=ncol, n=10, m=p(m), p2=p(p2), ld=2, off=0):
        return lib.mvx_lidar2img(p(pcd), ncol, n, m, p2, 1, p(out), ld, off, 0, None, None)

    bad_crop = [dict(ncol=2), dict(rng=None, m=None, p2=None), dict(p2=None), dict(nbytes=need - 1), dict(F=0), dict(cap=0),
                dict(out=None), dict(n_out=None), dict(pcd=None)]
    bad_project = [dict(ncol=2), dict(rng=None), dict(m=None), dict(p2=None), dict(pm=None), dict(pp=None), dict(nbytes=need - 1),
                   dict(cap_out=0), dict(cap_out=-1), dict(F=0), dict(cap=0)]
    bad_l2i = [dict(ncol=2), dict(ld=1), dict(ld=6, off=5), dict(off=-1), dict(ld=2, off=1), dict(m=None), dict(p2=None), dict(n=-1)]
    for fn, bad in ((crop, bad_crop), (crop_project, bad_project), (l2i, bad_l2i)):
        for b in bad:
            assert fn(**b) == -1, (fn.__name__, b)
    assert l2i(n=0) == 0 and l2i(n=0, ld=7, off=5) == 0, 'no points: nothing to do, and nothing launched'
    assert (out == np.float32(CANARY)).all() and (n_out == -7).all()


def test_crop_workspace_bytes():
    from modules import Extension as X
    q, qp = X.lib.mvx_crop_workspace_bytes, X.lib.mvx_crop_project_workspace_bytes
    for F, cap in ((0, 300), (-1, 300), (3, 0), (3, -5)):
        assert q(F, cap) == 0 and qp(F, cap) == 0
    for F, cap in ((1, 1), (1, 256), (1, 257), (3, 1000), (16, 120000)):
        assert q(F, cap) == qp(F, cap) == F * -(-cap // 256) * 4


def test_header_states_the_count_contract():
    import os
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = ' '.join(open(os.path.join(here, 'include', 'mvx_hip.h')).read().split())
    sec = text[text.index('Range crop, camera-frustum crop'):text.index('int mvx_lidar2img(')]
    sec = sec.replace(' * ', ' ')
    assert 'n_in[f] is clamped to cap_points' in sec
    assert 'rows of out at and after n_out[f] are not written' in sec
    assert 'may exceed cap_out' in sec and 'only the first cap_out' in sec
    from modules import _hip
    assert 'may exceed cap_out' in ' '.join(_hip.crop_project.__doc__.split())
