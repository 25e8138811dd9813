"""mvx_voxelize_frames through the C ABI, both batch layouts, against the per-frame CPU oracle (tests/voxelize_cases.py: the
inputs and `expected`, the one statement of the layouts).  The kernels move points and integers: every comparison is array_equal.

Every output is allocated with GUARD rows past the capacity the kernel is told and poisoned (voxels NaN; coords, counts, n_voxels,
vox_off -7); `check` asserts for every call that the rows of real voxels equal the oracle, that every row past them (per frame past
n_voxels[f], concat past the total) and every guard row is untouched, and the status word."""
import numpy as np
import pytest
import torch

import mvx_oracle as O
import voxelize_cases as K

pytestmark = pytest.mark.gpu

GUARD = 8
POISON = -7


class Run:
    """One call.  The full buffers (guard rows included) come back as numpy arrays."""

    def __init__(self, fs, T, C, concat, perm=True, ncol=6, cap_voxels=None, n_points=None, ext_idx=None, status0=0, size=K.SIZE,
                 pcd=None, perm_array=None):
        from modules import Extension as X
        dev = torch.device('cuda')
        F, cap = len(fs.n_points), fs.cap
        src = fs.pcd if pcd is None else pcd
        if ncol == 4:
            src = src[..., :4]
        elif ncol == 7:
            src = np.concatenate([src, np.random.default_rng(9).random(src.shape[:2] + (1,)).astype(np.float32)], 2)
        assert src.shape == (F, cap, ncol)
        self.F, self.T, self.C, self.concat = F, T, C, concat
        self.cap_voxels = cv = int(cap_voxels if cap_voxels is not None else (F * cap if concat else cap))
        rows = (cv if concat else F * cv) + GUARD
        up = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)      # a copy: the cases are read-only
        d_pcd, d_n = up(src), up(fs.n_points if n_points is None else np.asarray(n_points, np.int32))
        d_perm = up(fs.perm if perm_array is None else perm_array) if perm else None
        d_ext = up(ext_idx)
        voxels = torch.full((rows, T, C), float('nan'), dtype=torch.float32, device=dev)
        coords = torch.full((rows, 4), POISON, dtype=torch.int64, device=dev)
        counts = torch.full((rows,), POISON, dtype=torch.int32, device=dev)
        n_vox = torch.full((F + GUARD,), POISON, dtype=torch.int32, device=dev)
        vox_off = torch.full((F + 1 + GUARD,), POISON, dtype=torch.int32, device=dev)
        status = torch.tensor([status0, POISON], dtype=torch.int32, device=dev)
        nbytes = X.lib.mvx_voxelize_workspace_bytes(F, cap)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        self.rc = X.lib.mvx_voxelize_frames(X.ptr(d_pcd), X.ptr(d_perm), X.ptr(d_n), X.ptr(d_ext), F, cap, ncol,
                                            float(K.LO[0]), float(K.LO[1]), float(K.LO[2]), float(size[0]), float(size[1]),
                                            float(size[2]), T, C, cv, int(concat), X.ptr(voxels), X.ptr(coords), X.ptr(counts),
                                            X.ptr(n_vox), X.ptr(vox_off), X.ptr(status), X.ptr(ws), nbytes, X.stream())
        torch.cuda.synchronize()
        self.voxels, self.coords, self.counts = voxels.cpu().numpy(), coords.cpu().numpy(), counts.cpu().numpy()
        self.n_voxels, self.vox_off, self.status = n_vox.cpu().numpy(), vox_off.cpu().numpy(), status.cpu().numpy()

    def untouched(self, lo, hi):
        return bool(np.isnan(self.voxels[lo:hi]).all() and (self.coords[lo:hi] == POISON).all() and (self.counts[lo:hi] == POISON).all())

    def rows_equal(self, lo, v, c, n, what):
        assert np.array_equal(self.coords[lo:lo + len(n)], c), what + ': coords'
        assert np.array_equal(self.counts[lo:lo + len(n)], n), what + ': counts'
        assert np.array_equal(self.voxels[lo:lo + len(n)], v), what + ': payload'

    def frame_rows(self, f):
        """(first row, rows written) of frame f as the run itself reports them."""
        nv = int(self.n_voxels[f])
        if self.concat:
            lo = int(self.vox_off[f])
            return lo, max(0, min(nv, self.cap_voxels - lo))
        return f * self.cap_voxels, min(nv, self.cap_voxels)


def check(run, exp, status=0):
    """`exp`: K.expected(...) in the layout of the run.  With a capacity below the voxel count only the first cap_voxels rows (of
    the frame, or of the concatenation) are written and compared; n_voxels and vox_off report the true counts all the same."""
    F, cv = run.F, run.cap_voxels
    assert run.rc == 0
    assert run.status[0] == status and run.status[1] == POISON
    assert np.array_equal(run.n_voxels[:F], exp.n_voxels) and (run.n_voxels[F:] == POISON).all()
    assert np.array_equal(run.vox_off[:F + 1], exp.vox_off) and (run.vox_off[F + 1:] == POISON).all()
    assert np.array_equal(run.vox_off[:F + 1], np.concatenate([[0], np.cumsum(run.n_voxels[:F])]))
    if run.concat:
        shown = min(int(exp.vox_off[-1]), cv)
        run.rows_equal(0, exp.voxels[:shown], exp.coords[:shown], exp.counts[:shown], 'concat')
        assert np.array_equal(run.coords[:shown, 0], np.repeat(np.arange(F), exp.n_voxels)[:shown]), 'coords[:,0] = frame index'
        assert run.untouched(shown, cv + GUARD), 'rows past the total, guard rows'
    else:
        for f in range(F):
            shown = min(int(exp.n_voxels[f]), cv)
            run.rows_equal(f * cv, exp.voxels[f][:shown], exp.coords[f][:shown], exp.counts[f][:shown], 'frame %d' % f)
            assert (run.coords[f * cv:f * cv + shown, 0] == 0).all()
            assert run.untouched(f * cv + shown, (f + 1) * cv), 'frame %d: rows past n_voxels' % f
        assert run.untouched(F * cv, F * cv + GUARD), 'guard rows'


# ---- one frame: every route of the gather, both channel counts, with and without a permutation --------------------------------
@pytest.mark.parametrize('use_perm', [True, False], ids=['perm', 'noperm'])
@pytest.mark.parametrize('C', [9, 7])
@pytest.mark.parametrize('T', K.T_VALUES)
def test_single_frame_member_counts_at_the_thresholds(T, C, use_perm):
    fs = K.case('single')
    for concat in (0, 1):
        check(Run(fs, T, C, concat, perm=use_perm), K.expected('single', T, C, concat, use_perm=use_perm))


@pytest.mark.parametrize('C', [9, 7])
@pytest.mark.parametrize('ncol', [4, 6, 7])
def test_point_rows_of_four_six_and_seven_columns(ncol, C):
    """ncol = 4: row / col are written as zeros; ncol = 7: the seventh column is ignored."""
    fs = K.case('single')
    exp = K.expected('single', 35, C, 1, ncol=min(ncol, 6))
    if ncol == 4 and C == 9:
        assert not exp.voxels[..., 7:].any() and K.expected('single', 35, 9, 1).voxels[..., 7:].any()
    check(Run(fs, 35, C, 1, ncol=ncol), exp)


def test_mvx_voxelize_is_the_per_frame_layout():
    """The older entry point (no vox_off, no concat) through modules._hip.voxelize."""
    from modules import _hip
    fs = K.case('ragged4')
    dev = torch.device('cuda')
    res = _hip.voxelize(torch.tensor(fs.pcd, device=dev), torch.tensor(fs.perm, device=dev), torch.tensor(fs.n_points, device=dev),
                        K.RNG[:3], K.SIZE, 35, 9)
    exp = K.expected('ragged4', 35, 9, 0)
    assert int(res.status) == 0 and np.array_equal(res.n_voxels.cpu().numpy(), exp.n_voxels)
    for f, nv in enumerate(exp.n_voxels):
        assert np.array_equal(res.voxels[f, :nv].cpu().numpy(), exp.voxels[f])
        assert np.array_equal(res.coords[f, :nv].cpu().numpy(), exp.coords[f])
        assert np.array_equal(res.counts[f, :nv].cpu().numpy(), exp.counts[f])


# ---- frame sets: ragged, empty ends, frames that end on a scan block ------------------------------------------------------------
@pytest.mark.parametrize('name', ['ragged4', 'ends_empty', 'aligned1024', 'aligned1023'])
def test_both_layouts_agree_voxel_for_voxel(name):
    fs = K.case(name)
    per, cat = Run(fs, 35, 9, 0), Run(fs, 35, 9, 1)
    check(per, K.expected(name, 35, 9, 0))
    check(cat, K.expected(name, 35, 9, 1))
    # and with each other, without the oracle in between
    assert np.array_equal(per.n_voxels, cat.n_voxels) and np.array_equal(per.vox_off, cat.vox_off)
    for f in range(per.F):
        a, n = per.frame_rows(f)
        b, m = cat.frame_rows(f)
        assert n == m == per.n_voxels[f]
        assert np.array_equal(per.voxels[a:a + n], cat.voxels[b:b + n]) and np.array_equal(per.counts[a:a + n], cat.counts[b:b + n])
        assert np.array_equal(per.coords[a:a + n, 1:], cat.coords[b:b + n, 1:])
        assert (per.coords[a:a + n, 0] == 0).all() and (cat.coords[b:b + n, 0] == f).all()
    if name == 'ends_empty':
        assert per.n_voxels[:3].tolist()[0::2] == [0, 0] and cat.vox_off[1] == 0 and cat.vox_off[2] == cat.vox_off[3]


def test_seven_channels_with_more_than_one_frame():
    check(Run(K.case('ragged4'), 35, 7, 1), K.expected('ragged4', 35, 7, 1))


@pytest.mark.parametrize('concat', [1, 0], ids=['concat', 'per_frame'])
def test_63_frames_over_68_scan_blocks(concat):
    """The frame limit, and a scan whose later blocks look back over more than 64 predecessors; every frame against the oracle."""
    check(Run(K.case('many63'), 35, 9, concat), K.expected('many63', 35, 9, concat))


def test_point_counts_above_the_capacity_are_clamped():
    for name in ('aligned1024', 'ragged4'):
        fs = K.case(name)
        n = fs.n_points.copy()
        n[0] = fs.cap + 500                    # frame 0 is full in both cases
        assert fs.n_points[0] == fs.cap
        for concat in (0, 1):
            check(Run(fs, 35, 9, concat, n_points=n), K.expected(name, 35, 9, concat))


# ---- the status word ------------------------------------------------------------------------------------------------------------
def test_capacity_overflow_per_frame():
    """cap_voxels three below the fullest frame: bit 1; n_voxels true; that frame's first cap_voxels voxels exact, the other frames
    complete, nothing past the cap (check's per-frame tail and guard assertions).  The preset bit 2 of status survives."""
    exp = K.expected('ragged4', 35, 9, 0)
    full = int(exp.n_voxels.max())
    cv = full - 3
    assert np.sort(exp.n_voxels)[-2] < cv, 'one frame overflows'
    run = Run(K.case('ragged4'), 35, 9, 0, cap_voxels=cv, status0=4)
    check(run, exp, status=4 | 2)
    assert run.n_voxels[int(exp.n_voxels.argmax())] == full > cv


def test_capacity_overflow_concat():
    exp = K.expected('ragged4', 35, 9, 1)
    total = int(exp.vox_off[-1])
    run = Run(K.case('ragged4'), 35, 9, 1, cap_voxels=total - 5, status0=4)
    check(run, exp, status=4 | 2)
    assert run.vox_off[4] == total
    # a capacity that exactly fits: no bit
    check(Run(K.case('ragged4'), 35, 9, 1, cap_voxels=total, status0=4), exp, status=4)
    check(Run(K.case('ragged4'), 35, 9, 0, cap_voxels=int(exp.n_voxels.max())), K.expected('ragged4', 35, 9, 0), status=0)


@pytest.mark.parametrize('concat', [0, 1])
def test_index_outside_the_key_range(concat):
    """One point at x = 3e5 (index 1.5 M, past the 21-bit key) in frame 2 of four: bit 0; frames 0, 1 and 3 exact.  Frame 2: the key
    is aliased, so its voxel count is within 1 of the oracle's without that point; the aliased voxel's payload is left open."""
    fs = K.case('ragged4')
    pcd, perm, n = fs.pcd.copy(), fs.perm.copy(), fs.n_points.copy()
    pcd[2, 37] = (3e5, 0.0, 0.0, 0.5, 1.0, 2.0)
    n[2] = 38
    perm[2, :38] = np.random.default_rng(5).permutation(38)
    assert O.voxel_index(pcd[2, 37:38, :3], K.RNG, K.SIZE)[0, 0] + (1 << 20) >= (1 << 21)
    run = Run(fs, 35, 9, concat, pcd=pcd, perm_array=perm, n_points=n, status0=4)
    exp = K.expected('ragged4', 35, 9, 0)
    assert run.rc == 0 and run.status[0] == (4 | 1)
    assert np.array_equal(run.n_voxels[[0, 1, 3]], exp.n_voxels[[0, 1, 3]]) and abs(int(run.n_voxels[2]) - int(exp.n_voxels[2])) <= 1
    assert np.array_equal(run.vox_off[:5], np.concatenate([[0], np.cumsum(run.n_voxels[:4])]))
    for f in (0, 1, 3):
        lo, nv = run.frame_rows(f)
        assert nv == exp.n_voxels[f]
        coords = exp.coords[f].copy()
        coords[:, 0] = f if concat else 0
        run.rows_equal(lo, exp.voxels[f], coords, exp.counts[f], 'frame %d' % f)
    if concat:
        assert run.untouched(int(run.vox_off[4]), run.cap_voxels + GUARD)
    else:
        for f in range(4):
            lo, nv = run.frame_rows(f)
            assert run.untouched(lo + nv, (f + 1) * run.cap_voxels)
        assert run.untouched(4 * run.cap_voxels, 4 * run.cap_voxels + GUARD)


# ---- precomputed indices ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('concat', [0, 1])
def test_ext_idx_is_read_in_stream_order(concat):
    fs = K.case('ragged4')
    # (a) the oracle's own indices give what the computed path gives
    check(Run(fs, 35, 9, concat, ext_idx=K.oracle_indices(fs)), K.expected('ragged4', 35, 9, concat))
    # (b) indices of another voxel size while the call keeps the usual one: the grouping follows the ARRAY
    coarse = (0.4, 0.4, 0.8)
    exp = K.expected('ragged4', 35, 9, concat, size=coarse)
    assert exp.vox_off[-1] < K.expected('ragged4', 35, 9, concat).vox_off[-1]
    check(Run(fs, 35, 9, concat, ext_idx=K.oracle_indices(fs, np.array(coarse))), exp)


# ---- determinism ------------------------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_equal():
    """The bucket is filled in arrival order, which differs from call to call; the outputs must not."""
    for name, concat in (('single', 0), ('ragged4', 1)):
        a, b = Run(K.case(name), 35, 9, concat), Run(K.case(name), 35, 9, concat)
        for x, y in ((a.voxels, b.voxels), (a.coords, b.coords), (a.counts, b.counts), (a.n_voxels, b.n_voxels), (a.vox_off, b.vox_off)):
            assert x.tobytes() == y.tobytes()
