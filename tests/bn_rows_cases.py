"""Case tables, row layouts, operands and the float64 reference of the row BatchNorm tests (tests/test_bn_rows_gpu.py; the
reference and the tables are checked without a GPU by tests/test_bn_rows_host.py).  numpy only; imports nothing of the package.

The kernels (csrc/bn.hip) see a row-major [rows][C] f32 matrix whose rows belong to the frames of a frame set, segment by
segment (include/mvx_hip.h "Frame sets", MVX_ROWS_*); a stored row may stand for several identical rows of the dense tensor
(``weight``: the row weights of the VFE and fusion layouts).  The reference is BatchNorm with batch statistics (biased
variance, no affine) behind a ReLU, forward and backward, per frame, computed on that DENSE EXPANSION: every stored row repeated
``weight`` times, the incoming gradient of a repeated row shared equally between its copies, the gradient wrt the stored row the
sum over its copies.  For the VFE layout the same quantities come from tests/rows_ref.py (bn_forward, bn_relu_backward).

Launch geometry of bn_relu_backward_impl, restated in ``geometry`` and used ONLY to assert that a case reaches the situation it
names (reduction shape, block count, blocks that span two segments, a partial last trip)."""
import collections

import numpy as np

import rows_ref as R

EPS = 1e-6
REP = 32                               # replicas of the cross-block accumulators (MVX_STATS_REPLICAS, REP of csrc/bn.hip)
TRIP = 4                               # BWD_TRIP: rows per thread and trip of the two backward passes

# ---- bounds: the project's for these kernels (test_batchnorm_relu_forward_backward, tests/test_conv3d_gpu.py) ---------------
BOUND = 2e-5                           # mean, inverse deviation, apply, dz: max error over max |float64 reference|
BOUND_DBIAS = 1e-4


# ---- launch geometry -----------------------------------------------------------------------------------------------------
Geometry = collections.namedtuple('Geometry', 'c4 rpi grid rpb blocks shape')


def geometry(rows, C):
    """rpi = max(1, 256 / (C/4)); grid = min(1024, ceil(rows / (8 rpi))); rpb = ceil(rows / grid) rounded up to 4 rpi;
    blocks = ceil(rows / rpb).  shape: 'columns' (C > 1024: several column blocks, each reduced serially), 'shuffle'
    (64 % (C/4) == 0) or 'serial'."""
    c4 = C // 4
    rpi = max(1, 256 // c4)
    grid = min(1024, max(1, -(-rows // (2 * TRIP * rpi))))
    rpb = -(-rows // grid)
    rpb = -(-rpb // (TRIP * rpi)) * (TRIP * rpi)
    blocks = -(-rows // rpb) if rows else 0
    shape = 'columns' if c4 > 256 else 'shuffle' if 64 % c4 == 0 else 'serial'
    return Geometry(c4, rpi, grid, rpb, blocks, shape)


def spanning_blocks(lay, C):
    """Blocks of the backward passes whose row run holds rows of more than one segment."""
    g = geometry(lay.rows, C)
    n = 0
    for b in range(g.blocks):
        lo, hi = b * g.rpb, min(lay.rows, (b + 1) * g.rpb)
        n += sum(1 for s_lo, s_hi, _ in lay.segs if s_lo < hi and s_hi > lo and s_hi > s_lo) > 1
    return n


def last_trip_is_partial(rows, C):
    """The last block's last trip of TRIP x rpi rows is cut short by the end of the matrix."""
    g = geometry(rows, C)
    return (rows - (g.blocks - 1) * g.rpb) % (TRIP * g.rpi) != 0


# The C table of the issue: (C, rows per frame, frames, reduction shape, blocks, what it reaches)
Shape = collections.namedtuple('Shape', 'C per F shape blocks what')
C_TABLE = [
    Shape(4, 70001, 1, 'shuffle', 35, 'C/4 = 1: full-wave shuffle; the replica index wraps past 32'),
    Shape(12, 2000, 1, 'serial', 3, 'serial LDS walk, rpi = 85, thread 255 idle'),
    Shape(16, 1237, 3, 'shuffle', 8, 'blocks of 512 rows cross both frame bounds'),
    Shape(32, 2917, 3, 'shuffle', 35, 'shuffle; 35 blocks'),
    Shape(48, 700, 1, 'serial', 5, 'serial walk, rpi = 21'),
    Shape(64, 5, 1, 'shuffle', 1, 'fewer rows than one trip, one block'),
    Shape(128, 431, 3, 'shuffle', 21, 'shuffle across the two wave halves'),
    Shape(256, 9001, 1, 'shuffle', 282, 'C/4 = 64: the shuffle loop is empty, four waves fold through LDS'),
    Shape(768, 67, 3, 'serial', 26, 'rpi = 1, 8-row blocks crossing segments'),
    Shape(768, 2731, 3, 'serial', 683, 'grid capped at 1024'),
    Shape(1028, 41, 1, 'columns', 6, 'two column blocks (C > 1024)'),
]


def shape_id(s):
    return 'C%d_%dx%d' % (s.C, s.F, s.per)


def check_shape(s):
    """The geometry of a C_TABLE row is what the row says (asserted by the host test and again by every GPU test)."""
    rows = s.per * s.F
    g = geometry(rows, s.C)
    assert g.shape == s.shape, (s, g)
    assert g.blocks == s.blocks, (s, g)
    if s.C == 4:
        assert g.c4 == 1 and g.blocks > REP
    if s.C == 12:
        assert g.rpi == 85 and 255 // g.c4 >= g.rpi              # thread 255: row slot 85 of 0..84
    if s.C == 16:
        assert g.rpb == 512 and (s.per % 512) and (2 * s.per % 512)
    if s.C == 32:
        assert g.blocks > REP
    if s.C == 48:
        assert g.rpi == 21
    if s.C == 64:
        assert rows < TRIP * g.rpi and g.blocks == 1
    if s.C == 128:
        assert g.c4 == 32
    if s.C == 256:
        assert g.c4 == 64
    if s.C == 768:
        assert g.rpi == 1
        if s.per == 67:
            assert g.rpb == 8 and s.per % 8
        else:
            assert -(-rows // (2 * TRIP * g.rpi)) > 1024 and g.grid == 1024
    if s.C == 1028:
        assert g.c4 > 256 and -(-g.c4 // 256) == 2
    return g


# ---- row layouts ---------------------------------------------------------------------------------------------------------
class Rows:
    """A row layout of a frame set.  segs: (lo, hi, frame) in row order; weight (rows,): dense rows each stored row stands for;
    pop (F,): BatchNorm population of each frame = the sum of its weights; vox_off / real_off / t: what the mvx_frames_t
    descriptor takes (None for 'single': no descriptor)."""

    def __init__(self, kind, segs, weight, vox_off=None, real_off=None, t=1, vfe=None):
        self.kind, self.segs = kind, [(int(a), int(b), int(f)) for a, b, f in segs]
        self.weight = np.asarray(weight, np.int64)
        self.rows = int(self.weight.shape[0])
        self.F = 1 + max(f for _, _, f in self.segs)
        self.vox_off, self.real_off, self.t, self.vfe = vox_off, real_off, int(t), vfe
        self.frame = np.full((self.rows,), -1, np.int64)
        at = 0
        for lo, hi, f in self.segs:
            assert lo == at and hi >= lo
            self.frame[lo:hi] = f
            at = hi
        assert at == self.rows
        self.pop = np.asarray([int(self.weight[self.frame == f].sum()) for f in range(self.F)], np.int64)
        if kind != 'single' and kind != 'grid':
            want = [(vox_off[f + 1] - vox_off[f]) * self.t for f in range(self.F)]
            assert list(self.pop) == want, (kind, list(self.pop), want)      # what mvx_build_frame_map will take as population

    def frame_rows(self, f):
        return np.nonzero(self.frame == f)[0]

    def expansion(self, f):
        """Stored row of every dense row of frame f, and the share 1 / weight of each copy."""
        r = self.frame_rows(f)
        w = self.weight[r]
        return np.repeat(r, w), np.repeat(1.0 / np.maximum(w, 1), w)


def _offsets(counts):
    return [int(v) for v in np.concatenate([[0], np.cumsum(counts)])]


def single(rows):
    return Rows('single', [(0, rows, 0)], np.ones((rows,)))


def grid(F, per):
    z = [0] * (F + 1)
    return Rows('grid', [(f * per, (f + 1) * per, f) for f in range(F)], np.ones((F * per,)), z, z, 1)


def real(counts):
    off = _offsets(counts)
    return Rows('real', [(off[f], off[f + 1], f) for f in range(len(counts))], np.ones((off[-1],)), off, off, 1)


def voxels(counts):
    off = _offsets(counts)
    return Rows('voxels', [(off[f], off[f + 1], f) for f in range(len(counts))], np.ones((off[-1],)), off, off, 1)


def fusion(real_counts, vox_counts, t):
    """[real rows of all frames][one shared padded row per frame]; the shared row of frame f stands for every padded row of f:
    voxels x t - real rows (0 for a frame without voxels, whose shared row is still stored)."""
    F = len(real_counts)
    ro, vo = _offsets(real_counts), _offsets(vox_counts)
    w = np.ones((ro[-1] + F,), np.int64)
    for f in range(F):
        w[ro[-1] + f] = vox_counts[f] * t - real_counts[f]
    assert w.min() >= 0
    segs = [(ro[f], ro[f + 1], f) for f in range(F)] + [(ro[-1] + f, ro[-1] + f + 1, f) for f in range(F)]
    return Rows('fusion', segs, w, vo, ro, t)


def vfe(L):
    """A compact rows_ref.Layout: [real rows of all frames][one padded row per voxel]."""
    w = np.ones((L.rows,), np.int64)
    w[L.n_real:] = L.T - L.vcnt
    segs = [(L.real_off[f], L.real_off[f + 1], f) for f in range(L.F)]
    segs += [(L.n_real + L.vox_off[f], L.n_real + L.vox_off[f + 1], f) for f in range(L.F)]
    return Rows('vfe', segs, w, list(L.vox_off), list(L.real_off), L.T, vfe=L)


def _vfe_set_a():
    """Built like frame set A of the rows-glue tests (tests/test_rows_glue_gpu.py): 590 voxels of 35 rows in three frames, the middle one empty."""
    rng = np.random.default_rng(3)
    V, T = 590, 35
    kind = rng.random(V)
    c = rng.integers(2, 12, V)
    c[kind < 0.10] = 0
    c[(kind >= 0.10) & (kind < 0.25)] = 1
    c[(kind >= 0.25) & (kind < 0.32)] = T - 1
    c[(kind >= 0.32) & (kind < 0.40)] = T
    c[1:6], c[6:11], c[11:16] = 0, 1, T
    c[0] = c[-1] = T
    return R.Layout(T, V, c, [0, 250, 250, 590])


_LAYOUTS = {}


def layout(name):
    """The F = 3 layouts every kind is tested on (and their forms with an empty middle frame)."""
    if name not in _LAYOUTS:
        _LAYOUTS[name] = {
            'single': lambda: single(1293),
            'grid': lambda: grid(3, 431),
            'real': lambda: real([700, 431, 1237]),
            'real_empty': lambda: real([700, 0, 1237]),
            'voxels': lambda: voxels([431, 1237, 300]),
            'voxels_empty': lambda: voxels([431, 0, 1237]),
            'vfe': lambda: vfe(_vfe_set_a()),
            # the shared rows stand for 2000, 3050 and 77 dense rows
            'fusion': lambda: fusion([1500, 800, 623], [100, 110, 20], 35),
            'fusion_empty': lambda: fusion([1500, 0, 623], [100, 0, 20], 35),
        }[name]()
    return _LAYOUTS[name]


KINDS = ('single', 'grid', 'real', 'real_empty', 'voxels', 'voxels_empty', 'vfe', 'fusion', 'fusion_empty')
KIND_C = (16, 128)


def table_layout(s):
    return single(s.per) if s.F == 1 else grid(s.F, s.per)


# ---- float64 reference over the dense expansion --------------------------------------------------------------------------------
def bn_forward(lay, y, eps=EPS):
    """Per frame: mean and 1 / sqrt(var + eps), biased variance, over the dense expansion.  A frame without population: NaN."""
    if lay.vfe is not None:
        return R.bn_forward(y, lay.vfe, eps)
    y = np.asarray(y, np.float64)
    mi = np.full((lay.F, 2, y.shape[1]), np.nan)
    for f in range(lay.F):
        idx, _ = lay.expansion(f)
        if len(idx):
            d = y[idx]
            mean = d.mean(0)
            mi[f] = mean, 1.0 / np.sqrt(((d - mean) ** 2).mean(0) + eps)
    return mi


def bn_relu_backward(lay, dyhat, y, mi):
    """Gradient of yhat = BN(y), y = relu(z), wrt z with the statistics ``mi`` (F, 2, C), on the dense expansion and folded back on
    the stored rows; dbias = the sum of dz over all dense rows of all frames.  A stored row that stands for no dense row has no
    dz (NaN).  -> (dz (rows, C), dbias (C,))"""
    if lay.vfe is not None:
        return R.bn_relu_backward(dyhat, y, mi, lay.vfe)
    dyhat, y, mi = np.asarray(dyhat, np.float64), np.asarray(y, np.float64), np.asarray(mi, np.float64)
    dz = np.full(y.shape, np.nan)
    dbias = np.zeros((y.shape[1],))
    for f in range(lay.F):
        idx, share = lay.expansion(f)
        if not len(idx):
            continue
        yd, gd = y[idx], dyhat[idx] * share[:, None]
        yh = (yd - mi[f, 0]) * mi[f, 1]
        N = len(idx)
        dzd = mi[f, 1] * (gd - gd.sum(0) / N - yh * (gd * yh).sum(0) / N) * (yd > 0)
        r = lay.frame_rows(f)
        w = lay.weight[r]
        keep = w > 0
        dz[r[keep]] = np.add.reduceat(dzd, (np.cumsum(w[keep]) - w[keep]), axis=0)
        dbias += dzd.sum(0)
    return dz, dbias


def apply(lay, y, mi):
    """(y - mean) * inv of every row with its own frame's statistics."""
    y, mi = np.asarray(y, np.float64), np.asarray(mi, np.float64)
    return (y - mi[lay.frame, 0]) * mi[lay.frame, 1]


# ---- operands --------------------------------------------------------------------------------------------------------------
FRAME_SCALE = (1.0, 2.5, 0.4)
FRAME_OFFSET = (0.3, -0.8, 1.5)


def operands(lay, C, seed=0, peak_last=False):
    """y (rows, C) f32 = relu(randn * scale_f + offset_f): every frame its own distribution, about a third to two thirds exact
    zeros; dyhat f32; the gradient of a row that stands for no dense row is zero and its y positive (its dz must come out as
    exactly 0).  mi f32 (F, 2, C): the float64 statistics of y rounded to f32 -- kernel and reference read the same numbers; a frame
    without population gets finite statistics of its own that nothing may use.  peak_last: the last row carries by far the
    largest gradient on positive y, so max |dz| lies there."""
    rng = np.random.default_rng(1000 * seed + 7 * C + lay.rows)
    fr = np.maximum(lay.frame, 0)
    sc, of = np.asarray(FRAME_SCALE)[fr % 3][:, None], np.asarray(FRAME_OFFSET)[fr % 3][:, None]
    y = np.maximum(rng.standard_normal((lay.rows, C)) * sc + of, 0.0).astype(np.float32)
    g = (rng.standard_normal((lay.rows, C)) * 0.1).astype(np.float32)
    none = lay.weight == 0
    g[none] = 0.0
    y[none] = np.abs(y[none]) + 0.5
    if peak_last and lay.rows:
        y[-1] = np.abs(y[-1]) + 0.25
        g[-1] = np.where(g[-1] >= 0, 50.0, -50.0) + g[-1]
    mi = bn_forward(lay, y)
    for f in range(lay.F):
        if lay.pop[f] == 0:
            mi[f, 0], mi[f, 1] = 0.125 * (f + 1), 3.0
    return y, g, mi.astype(np.float32)


def rel(a, b):
    """max |a - b| over max |b|, float64; NaN in both at the same place counts as equal."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), 'NaN pattern differs'
    m = ~np.isnan(b)
    if not m.any():
        return 0.0
    return float(np.abs(a[m] - b[m]).max() / max(np.abs(b[m]).max(), 1e-300))
