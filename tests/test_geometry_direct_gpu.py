"""mvx_crop_points, mvx_crop_project_points and mvx_lidar2img through the C ABI on buffers the test fills itself, against the
restatement of the kernels' arithmetic in their own order (tests/geometry_ref.py (b), tied to a longdouble statement by
tests/test_geometry_host.py): the kept set, the kept rows, src_index and every projected value are compared BIT FOR BIT, the
library being built without contraction and dividing with correct rounding.

Every output is allocated with GUARD rows past what the kernel is told and filled with a canary (floats CANARY, integers -7); each
check asserts that whatever lies past the rows a call may write still holds it.  `out` always has at least n_frames * cap_points
rows, whatever cap_out is."""
import numpy as np
import pytest
import torch

import geometry_cases as K
import geometry_ref as R

pytestmark = pytest.mark.gpu

GUARD = 8
CANARY = np.float32(-777.25)
ICANARY = -7
CALIBS = ('kitti', 'generic')
FILTERS = ('range', 'sight', 'both')


def dev():
    return torch.device('cuda')


def up(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev())          # a copy: the cases are read-only


def host(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1))


def hptr(a):
    import ctypes
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Crop:
    """One mvx_crop_points call; the full buffers (guard rows included) come back as numpy arrays."""

    def __init__(self, pcd, n_in, filt, cb, rng=K.RANGE, bounds_f32=0, math_f32=0, want_src=True, **bad):
        from modules import Extension as X
        F, cap, ncol = pcd.shape
        self.F, self.cap, self.ncol = F, cap, ncol
        self.args = dict(range6=rng if filt in ('range', 'both') else None, bounds_f32=bounds_f32, math_f32=math_f32,
                         m=cb.m if filt in ('sight', 'both') else None, p2=cb.p2 if filt in ('sight', 'both') else None,
                         imsize_wh=cb.imsize_wh)
        a = dict(self.args, ncol=ncol, ws_short=0)
        a.update(bad)
        r6, m, p2 = (None if a[k] is None else host(a[k]) for k in ('range6', 'm', 'p2'))
        out = torch.full((F * cap + GUARD, ncol), float(CANARY), dtype=torch.float32, device=dev())
        src = torch.full((F * cap + GUARD,), ICANARY, dtype=torch.int32, device=dev()) if want_src else None
        n_out = torch.full((F + GUARD,), ICANARY, dtype=torch.int32, device=dev())
        nbytes = X.lib.mvx_crop_workspace_bytes(F, cap)
        ws = torch.empty((nbytes + 16,), dtype=torch.uint8, device=dev())
        d_pcd, d_n = up(pcd), up(n_in)                                          # named: they live until the synchronize
        self.rc = X.lib.mvx_crop_points(X.ptr(d_pcd), X.ptr(d_n), F, cap, a['ncol'], hptr(r6), int(bounds_f32), hptr(m),
                                        hptr(p2), float(cb.imsize_wh[0]), float(cb.imsize_wh[1]), int(math_f32), X.ptr(out),
                                        X.ptr(n_out), X.ptr(src), X.ptr(ws), nbytes - a['ws_short'], X.stream())
        torch.cuda.synchronize()
        self.out, self.n_out = out.cpu().numpy(), n_out.cpu().numpy()
        self.src = None if src is None else src.cpu().numpy()

    def untouched(self):
        return bool((self.out == CANARY).all() and (self.n_out == ICANARY).all() and (self.src is None or (self.src == ICANARY).all()))


def expected_rows(pcd, n_in, f, **args):
    """(kept rows, their source indices) of frame f by the restatement."""
    cap = pcd.shape[1]
    n = cap if n_in is None else min(int(n_in[f]), cap)
    mask = R.keep(pcd[f, :n, :3], **args)
    return pcd[f, :n][mask], np.flatnonzero(mask).astype(np.int32)


def check_crop(run, pcd, n_in):
    F, cap = run.F, run.cap
    assert run.rc == 0
    assert (run.n_out[F:] == ICANARY).all()
    for f in range(F):
        rows, idx = expected_rows(pcd, n_in, f, **run.args)
        n = len(idx)
        assert run.n_out[f] == n, 'frame %d' % f
        lo = f * cap
        assert run.out[lo:lo + n].tobytes() == rows.tobytes(), 'frame %d: kept rows, bitwise and in source order' % f
        assert (run.out[lo + n:lo + cap] == CANARY).all(), 'frame %d: rows past n_out' % f
        if run.src is not None:
            assert np.array_equal(run.src[lo:lo + n], idx) and (run.src[lo + n:lo + cap] == ICANARY).all(), 'frame %d: src_index' % f
    assert (run.out[F * cap:] == CANARY).all() and (run.src is None or (run.src[F * cap:] == ICANARY).all()), 'guard rows'


# ---- mvx_crop_points -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cal', CALIBS)
@pytest.mark.parametrize('name', K.CLOUD_NAMES)
def test_crop_points_equals_the_restatement(name, cal):
    """Every filter combination, both arithmetics, both roundings of the bounds; src_index present and NULL give the same rows."""
    c, cb = K.cloud(name), K.calib(cal)
    for filt in FILTERS:
        for math_f32 in ((0, 1) if filt != 'range' else (0,)):
            for bounds_f32 in ((0, 1) if filt != 'sight' else (0,)):
                run = Crop(c.pcd, c.n_in, filt, cb, bounds_f32=bounds_f32, math_f32=math_f32)
                check_crop(run, c.pcd, c.n_in)
    bare = Crop(c.pcd, c.n_in, 'both', cb, want_src=False)
    check_crop(bare, c.pcd, c.n_in)
    same = Crop(c.pcd, c.n_in, 'both', cb)
    assert bare.out.tobytes() == same.out.tobytes() and np.array_equal(bare.n_out, same.n_out)


@pytest.mark.parametrize('name', [n for n in K.CLOUD_NAMES if K.cloud(n).F == 3])
def test_a_frame_of_three_equals_that_frame_alone(name):
    c, cb = K.cloud(name), K.calib('kitti')
    for filt, math_f32 in (('both', 0), ('sight', 1)):
        three = Crop(c.pcd, c.n_in, filt, cb, math_f32=math_f32)
        for f in range(3):
            one = Crop(c.pcd[f:f + 1], None if c.n_in is None else c.n_in[f:f + 1], filt, cb, math_f32=math_f32)
            assert one.rc == 0 and one.n_out[0] == three.n_out[f]
            lo = f * c.cap
            assert one.out[:c.cap].tobytes() == three.out[lo:lo + c.cap].tobytes()
            assert np.array_equal(one.src[:c.cap], three.src[lo:lo + c.cap])
    if c.n_in is not None and (c.n_in == 0).any():
        assert three.n_out[1] == 0


@pytest.mark.parametrize('name', ['c257', 'c1000', 'c256'])
def test_cropping_the_output_again_keeps_everything(name):
    c, cb = K.cloud(name), K.calib('generic')
    for math_f32 in (0, 1):
        first = Crop(c.pcd, c.n_in, 'both', cb, math_f32=math_f32, bounds_f32=math_f32)
        again = Crop(first.out[:c.F * c.cap].reshape(c.F, c.cap, c.ncol), first.n_out[:c.F], 'both', cb, math_f32=math_f32,
                     bounds_f32=math_f32)
        assert again.rc == 0 and np.array_equal(again.n_out, first.n_out) and first.n_out[:c.F].sum() > 0
        for f in range(c.F):
            n, lo = first.n_out[f], f * c.cap
            assert again.out[lo:lo + n].tobytes() == first.out[lo:lo + n].tobytes()
            assert np.array_equal(again.src[lo:lo + n], np.arange(n)) and (again.out[lo + n:lo + c.cap] == CANARY).all()


@pytest.mark.parametrize('cal', ('dyadic', 'dyadic_frac') + CALIBS)
def test_edge_rows(cal):
    """The rows of geometry_cases.EDGES, placed ON the limits of every test (the host test asserts how both references decide each
    under the dyadic calibration, and that the two arithmetics and the two roundings of the bounds disagree where they should);
    non-finite rows are dropped by every filter.  'dyadic_frac': image sizes that are no f32 values, the only ones that show in which
    type the f32 limit was formed."""
    cb = K.calib(cal)
    for ncol in (3, 4):
        c = K.edges(ncol)
        for filt in FILTERS:
            for math_f32 in (0, 1):
                for bounds_f32 in (0, 1):
                    run = Crop(c.pcd, None, filt, cb, rng=K.EDGE_RANGE, bounds_f32=bounds_f32, math_f32=math_f32)
                    check_crop(run, c.pcd, None)
                    kept = run.src[:run.n_out[0]]
                    assert np.isfinite(c.pcd[0, kept, :3]).all()
                    if cal.startswith('dyadic') and filt != 'both':
                        k = 1 - (math_f32 if filt == 'sight' else bounds_f32)
                        want = [i for i, e in enumerate(K.EDGES) if filt[0] in e.filt and (e.keep_f32, e.keep_f64)[k]]
                        assert [i for i in kept if filt[0] in K.EDGES[i].filt] == want


# ---- mvx_crop_project_points ---------------------------------------------------------------------------------------------------------
class CropProject:
    def __init__(self, pcd, n_in, mask_cb, proj_cb, cap_out, rng=K.RANGE, **bad):
        from modules import Extension as X
        F, cap, ncol = pcd.shape
        self.F, self.cap, self.ncol, self.cap_out = F, cap, ncol, cap_out
        a = dict(ncol=ncol, range6=rng, m=mask_cb.m, p2=mask_cb.p2, pm=proj_cb.m, pp=proj_cb.p2, cap_out_arg=cap_out, ws_short=0)
        a.update(bad)
        r6, m, p2, pm, pp = (None if a[k] is None else host(a[k]) for k in ('range6', 'm', 'p2', 'pm', 'pp'))
        self.rows = F * max(cap, cap_out) + GUARD
        out = torch.full((self.rows, ncol + 2), float(CANARY), dtype=torch.float32, device=dev())
        n_out = torch.full((F + GUARD,), ICANARY, dtype=torch.int32, device=dev())
        nbytes = X.lib.mvx_crop_project_workspace_bytes(F, cap)
        ws = torch.empty((nbytes + 16,), dtype=torch.uint8, device=dev())
        self.d_out, self.d_n_out = out, n_out
        d_pcd, d_n = up(pcd), up(n_in)
        self.rc = X.lib.mvx_crop_project_points(X.ptr(d_pcd), X.ptr(d_n), F, cap, a['ncol'], hptr(r6), hptr(m), hptr(p2),
                                                float(mask_cb.imsize_wh[0]), float(mask_cb.imsize_wh[1]), hptr(pm), hptr(pp),
                                                X.ptr(out), a['cap_out_arg'], X.ptr(n_out), X.ptr(ws), nbytes - a['ws_short'],
                                                X.stream())
        torch.cuda.synchronize()
        self.out, self.n_out = out.cpu().numpy(), n_out.cpu().numpy()

    def untouched(self):
        return bool((self.out == CANARY).all() and (self.n_out == ICANARY).all())


def check_crop_project(run, pcd, n_in, mask_cb, proj_cb, rng=K.RANGE):
    """Kept set: the f64 masks of the MASK matrices.  Columns ncol, ncol + 1: the f32 (v, u) of the PROJECTION matrices.  Frame
    stride cap_out; only the first cap_out kept rows are stored, n_out holds the full count."""
    F, ncol, co = run.F, run.ncol, run.cap_out
    assert run.rc == 0 and (run.n_out[F:] == ICANARY).all()
    full = []
    for f in range(F):
        rows, _ = expected_rows(pcd, n_in, f, range6=rng, bounds_f32=0, m=mask_cb.m, p2=mask_cb.p2, imsize_wh=mask_cb.imsize_wh,
                                math_f32=0)
        vu, _ = R.lidar2img(rows[:, :3], proj_cb.m, proj_cb.p2, 1, 1)
        exp = np.concatenate([rows, vu], 1)
        full.append(len(exp))
        assert run.n_out[f] == len(exp), 'frame %d: the FULL count' % f
        shown = min(len(exp), co)
        lo = f * co
        got = run.out[lo:lo + shown]
        assert got[:, :ncol].tobytes() == exp[:shown, :ncol].tobytes(), 'frame %d: kept rows' % f
        assert got[:, ncol].tobytes() == exp[:shown, ncol].tobytes(), 'frame %d: column ncol = row = v' % f
        assert got[:, ncol + 1].tobytes() == exp[:shown, ncol + 1].tobytes(), 'frame %d: column ncol + 1 = col = u' % f
        assert (run.out[lo + shown:lo + co] == CANARY).all(), 'frame %d: rows past its count' % f
    assert (run.out[F * co:] == CANARY).all(), 'everything after the last frame'
    return full


def l2i(xyz_rows, cb, math_f32, swap, ld=2, off=0, want_z=False, n=None, **bad):
    """mvx_lidar2img on rows f32 (n, ncol) -> (rc, out (n + GUARD, ld) with the canary, cam_z (n + GUARD) or None)."""
    from modules import Extension as X
    rows = np.ascontiguousarray(xyz_rows, np.float32)
    n = rows.shape[0] if n is None else n
    a = dict(ncol=rows.shape[1], m=cb.m, p2=cb.p2)
    a.update(bad)
    d_in = up(rows if rows.shape[0] else np.zeros((1, rows.shape[1]), np.float32))
    out = torch.full((rows.shape[0] + GUARD, ld), float(CANARY), dtype=torch.float32, device=dev())
    z = torch.full((rows.shape[0] + GUARD,), float(CANARY), dtype=torch.float32, device=dev()) if want_z else None
    m, p2 = (None if a[k] is None else host(a[k]) for k in ('m', 'p2'))
    rc = X.lib.mvx_lidar2img(X.ptr(d_in), a['ncol'], n, hptr(m), hptr(p2), int(math_f32), X.ptr(out), ld, off, int(swap), X.ptr(z),
                             X.stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), None if z is None else z.cpu().numpy()


PAIRS = (('kitti', 'generic'), ('generic', 'kitti'), ('kitti', 'kitti_f32'))


def pair(mask, proj):
    return K.calib(mask), K.f32_formed(K.calib('kitti')) if proj == 'kitti_f32' else K.calib(proj)


@pytest.mark.parametrize('mask,proj', PAIRS, ids=['%s_%s' % p for p in PAIRS])
@pytest.mark.parametrize('name', K.CLOUD_NAMES)
def test_crop_project_masks_with_one_matrix_set_and_projects_with_the_other(name, mask, proj):
    """Two DIFFERENT calibrations for the masks and for the appended columns, both ways round, and the pairing FrameBatch.prepared()
    builds (f64 product against f32-formed product); cap_out above cap.  The appended columns are also what mvx_lidar2img writes
    for the kept rows with math_f32 = 1 and swap_to_row_col = 1."""
    c = K.cloud(name)
    mask_cb, proj_cb = pair(mask, proj)
    run = CropProject(c.pcd, c.n_in, mask_cb, proj_cb, c.cap + 5)
    full = check_crop_project(run, c.pcd, c.n_in, mask_cb, proj_cb)
    for f, n in enumerate(full):
        lo = f * run.cap_out
        rc, vu, _ = l2i(run.out[lo:lo + n, :c.ncol], proj_cb, 1, 1)
        assert rc == 0 and vu[:n].tobytes() == run.out[lo:lo + n, c.ncol:].tobytes()


@pytest.mark.parametrize('name', ['c1000', 'c257', 'c1000one'])
def test_crop_project_cap_out_equal_to_and_below_the_kept_count(name):
    c = K.cloud(name)
    mask_cb, proj_cb = pair('kitti', 'kitti_f32')
    full = check_crop_project(CropProject(c.pcd, c.n_in, mask_cb, proj_cb, c.cap), c.pcd, c.n_in, mask_cb, proj_cb)
    most = max(full)
    assert most < c.cap
    fit = CropProject(c.pcd, c.n_in, mask_cb, proj_cb, most)                     # the fullest frame fits exactly
    assert check_crop_project(fit, c.pcd, c.n_in, mask_cb, proj_cb) == full
    for below in (most - 1, max(1, min(n for n in full if n) // 2), 1):
        run = CropProject(c.pcd, c.n_in, mask_cb, proj_cb, below)
        assert check_crop_project(run, c.pcd, c.n_in, mask_cb, proj_cb) == full
        assert (run.n_out[:c.F] > below).any(), 'a frame overflows, and n_out says so'
        for f in range(1, c.F):                                                 # the next frame starts at cap_out, not at cap
            if full[f]:
                assert run.out[f * below].tobytes() == fit.out[f * most].tobytes()


def test_an_overflowing_crop_project_feeds_the_voxelizer():
    """(out, n_out) with n_out above cap_out go to the voxelizer as they are: it clamps the count and groups exactly the stored
    rows."""
    import mvx_oracle as O
    from modules import _hip
    c = K.cloud('c1000')
    ncol = 4
    pcd = np.ascontiguousarray(c.pcd[..., :ncol])
    mask_cb, proj_cb = pair('kitti', 'kitti_f32')
    full = check_crop_project(CropProject(pcd, c.n_in, mask_cb, proj_cb, c.cap), pcd, c.n_in, mask_cb, proj_cb)
    cap_out = max(full) // 2
    run = CropProject(pcd, c.n_in, mask_cb, proj_cb, cap_out)
    check_crop_project(run, pcd, c.n_in, mask_cb, proj_cb)
    assert run.n_out[0] > cap_out and 0 < run.n_out[2] < cap_out and run.n_out[1] == 0
    points6 = run.d_out[:c.F * cap_out].reshape(c.F, cap_out, ncol + 2)
    res = _hip.voxelize(points6, None, run.d_n_out[:c.F].contiguous(), K.RANGE[:3], O.voxelsize(), 35, 9)
    torch.cuda.synchronize()
    assert int(res.status) == 0
    n_vox, counts = res.n_voxels.cpu().numpy(), res.counts.cpu().numpy()
    for f in range(c.F):
        n = min(int(run.n_out[f]), cap_out)
        assert counts[f, :n_vox[f]].sum() <= cap_out
        if n == 0:
            assert n_vox[f] == 0
            continue
        rows = run.out[f * cap_out:f * cap_out + n]
        _, idx, cnt = O.group(rows, np.arange(n, dtype=np.int32), list(K.RANGE), O.voxelsize(), 35)
        assert n_vox[f] == len(cnt) and counts[f, :n_vox[f]].sum() == cnt.sum() == n
        assert np.array_equal(res.coords[f, :n_vox[f], 1:].cpu().numpy(), idx.astype(np.int64))


# ---- mvx_lidar2img -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ld,off', [(2, 0), (7, 5), (6, 4)])
@pytest.mark.parametrize('n', [0, 1, 257])
def test_lidar2img_writes_two_columns_and_nothing_else(n, ld, off):
    c = K.cloud('c300')
    for cal in CALIBS:
        cb = K.calib(cal)
        rows = c.pcd[0, :n]
        for math_f32 in (0, 1):
            for swap in (0, 1):
                for want_z in (False, True):
                    rc, out, z = l2i(rows, cb, math_f32, swap, ld, off, want_z)
                    exp, exp_z = R.lidar2img(rows[:, :3], cb.m, cb.p2, math_f32, swap)
                    assert rc == 0
                    assert out[:n, off:off + 2].tobytes() == exp.tobytes()
                    rest = np.delete(out, [off, off + 1], axis=1)
                    assert (rest == CANARY).all() and (out[n:] == CANARY).all(), 'every other column, and the guard rows'
                    if want_z:
                        assert z[:n].tobytes() == exp_z.tobytes() and (z[n:] == CANARY).all()
    if n == 257:
        assert (exp[:, 0] != exp[:, 1]).any(), 'the swap moves values'


def test_lidar2img_on_the_edge_rows():
    """Depth 0 and non-finite coordinates: no filter here, the quotients are written as they come (inf, nan), bit for bit."""
    c = K.edges()
    for cal in ('dyadic', 'kitti'):
        cb = K.calib(cal)
        for math_f32 in (0, 1):
            rc, out, z = l2i(c.pcd[0], cb, math_f32, 0, want_z=True)
            exp, exp_z = R.lidar2img(c.pcd[0, :, :3], cb.m, cb.p2, math_f32, 0)
            n = len(exp)
            assert rc == 0 and out[:n].tobytes() == exp.tobytes() and z[:n].tobytes() == exp_z.tobytes()


# ---- argument checks -------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_launch_nothing():
    """Each call returns a non-zero code and leaves out, src_index and n_out on the canary."""
    c, cb = K.cloud('c300'), K.calib('kitti')
    pcd = np.ascontiguousarray(np.concatenate([c.pcd, c.pcd[..., :1]], 2))                    # four columns
    for bad in (dict(ncol=2), dict(range6=None, m=None, p2=None), dict(range6=None, p2=None), dict(p2=None), dict(ws_short=1)):
        run = Crop(pcd, c.n_in, 'both', cb, **bad)
        assert run.rc != 0 and run.untouched(), bad
    for bad in (dict(ncol=2), dict(cap_out_arg=0), dict(pm=None), dict(pp=None), dict(range6=None), dict(m=None), dict(p2=None),
                dict(ws_short=1)):
        run = CropProject(pcd, c.n_in, cb, cb, c.cap, **bad)
        assert run.rc != 0 and run.untouched(), bad
    for bad in (dict(ld=1, off=0), dict(ld=6, off=5), dict(ld=4, off=-1), dict(ld=2, off=0, ncol=2), dict(ld=2, off=0, m=None)):
        rc, out, z = l2i(pcd[0], cb, 1, 0, want_z=True, **bad)
        assert rc != 0 and (out == CANARY).all() and (z == CANARY).all(), bad
    good = Crop(pcd, c.n_in, 'both', cb)
    assert good.rc == 0 and not good.untouched()


def test_workspace_sizes():
    from modules import Extension as X
    q, qp = X.lib.mvx_crop_workspace_bytes, X.lib.mvx_crop_project_workspace_bytes
    for F, cap in ((0, 300), (-1, 300), (3, 0), (3, -5), (0, 0)):
        assert q(F, cap) == 0 and qp(F, cap) == 0
    for F, cap in ((1, 1), (1, 256), (1, 257), (3, 1000), (16, 120000)):
        assert q(F, cap) == qp(F, cap) == F * -(-cap // 256) * 4
