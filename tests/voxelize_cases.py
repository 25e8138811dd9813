"""Inputs of the voxelizer tests (tests/test_voxelize_host.py, tests/test_voxelize_batch_gpu.py): numpy only, seeded.

The reference of every comparison is the CPU oracle, ``mvx_oracle.group`` (nine channels) / ``group7`` (seven), called frame by
frame; ``expected`` states ONCE how the per-frame results make up the two batch layouts of ``mvx_voxelize_frames``.  Range and
voxel size are the product's (``O.VELORANGE``, ``O.voxelsize()``): cells of 0.2 x 0.2 x 0.4 from (0, -40, -3)."""
import collections
import functools

import numpy as np

import mvx_oracle as O

RNG = O.VELORANGE
LO = np.array(RNG[:3], np.float64)
HI = np.array(RNG[3:], np.float64)
SIZE = np.array(O.voxelsize(), np.float64)
CAP = 1100

# member counts around the thresholds of the gather: 16 (lanes of a narrow group), T, 64 (bucket entries), more (ordered walk)
COUNTS = (1, 2, 4, 5, 6, 15, 16, 17, 34, 35, 36, 63, 64, 65, 200)
T_VALUES = (5, 16, 35, 64)

FrameSet = collections.namedtuple('FrameSet', 'name pcd perm n_points cap')      # pcd f32 (F, cap, 6), perm i32 (F, cap), n i32 (F,)
Expected = collections.namedtuple('Expected', 'voxels coords counts n_voxels vox_off')


def crowd_cell(k):
    return np.array([3 + 2 * k, 5 + k % 7, k % 10], np.float64)


def crowd(seed, counts=COUNTS):
    """The k-th entry n of ``counts``: n points inside the one cell ``crowd_cell(k)``, a tenth of a cell away from its faces, so
    that the cell has exactly n members; columns 3:6 (r, row, col) random."""
    g = np.random.default_rng(seed)
    rows = []
    for k, n in enumerate(counts):
        xyz = LO + (crowd_cell(k) + 0.1 + 0.8 * g.random((n, 3))) * SIZE
        rows.append(np.concatenate([xyz, g.random((n, 1)), g.uniform(0, 369, (n, 1)), g.uniform(0, 1223, (n, 1))], 1))
    return np.concatenate(rows).astype(np.float32)


# xyz of edges() and the index the contract gives each: f64 (x - lo) / size on the f32 value, truncated toward zero
EDGE_POINTS = (
    ((0.0, -40.0, -3.0), (0, 0, 0)),              # exactly on the range minimum
    ((-0.05, -39.95, -2.9), (0, 0, 0)),           # x 0.05 below it: -0.25 truncates to 0, the cell of the point above
    ((0.2, -39.8, -2.6), (1, 1, 1)),              # the corner lo + size: the three f32 values are at or just inside cell 1
    ((0.6, -39.9, -2.9), (3, 0, 0)),              # f32(0.6) = 0.60000002 lies in cell 3 (the f64 quotient 0.6 / 0.2 is 2.99..)
    ((np.nextafter(np.float32(0.6), np.float32(0)), -39.9, -2.9), (2, 0, 0)),     # one f32 step below: cell 2
    ((1.4, -39.9, -2.9), (6, 0, 0)),              # f32(1.4) = 1.39999998 stays in cell 6
    ((np.nextafter(np.float32(1.4), np.float32(2)), -39.9, -2.9), (7, 0, 0)),     # one f32 step above: cell 7
    ((0.1, -39.9, -2.2), (0, 0, 1)),              # f32(-2.2) + 3 = 0.79999995: below the face at 0.8
    ((0.1, -39.9, np.nextafter(np.float32(-2.2), np.float32(0))), (0, 0, 2)),     # one f32 step up: on or past it
    ((-100.0, -39.9, -2.9), (-500, 0, 0)),        # negative indices inside the 21-bit key range: decoded through KEY_BIAS,
    ((0.1, -39.9, -30.0), (0, 0, -67)),           # not flagged; -67.5 truncates toward zero
    ((0.1, -39.9, -2.9), (0, 0, 0)),              # a third member of cell (0, 0, 0)
)


def edges():
    xyz = np.array([p for p, _ in EDGE_POINTS], np.float32)
    pay = np.stack([np.linspace(0.1, 0.9, len(xyz)), np.linspace(3, 360, len(xyz)), np.linspace(7, 1200, len(xyz))], 1)
    return np.concatenate([xyz, pay.astype(np.float32)], 1)


def edge_indices():
    return np.array([i for _, i in EDGE_POINTS], np.int32)


def uniform(seed, n):
    """Half of the points uniform over the whole range (1.4 M cells: singletons), half over a block of 8 x 6 x 2 cells at cell
    (100, 200, 2), away from the crowd cells: together mostly 1 to 4 members per voxel."""
    g = np.random.default_rng(seed)
    far = LO + g.random((n // 2, 3)) * (HI - LO) * 0.999
    near = LO + (np.array([100., 200., 2.]) + g.random((n - n // 2, 3)) * np.array([8., 6., 2.])) * SIZE
    xyz = np.concatenate([far, near])
    return np.concatenate([xyz, g.random((n, 1)), g.uniform(0, 369, (n, 1)), g.uniform(0, 1223, (n, 1))], 1).astype(np.float32)


def full_mix(seed, n):
    """crowd + edges + uniform, n points in all (n >= 575)."""
    c, e = crowd(seed), edges()
    return np.concatenate([c, e, uniform(seed + 1000, n - len(c) - len(e))])


def sampled_mix(seed, n):
    """n rows drawn without replacement from crowd + edges + uniform(600): every frame another mix of member counts."""
    pool = np.concatenate([crowd(seed), edges(), uniform(seed + 1000, 600)])
    return pool[np.random.default_rng(seed + 2000).permutation(len(pool))[:n]]


def frame_set(name, frames, cap):
    """Rows past a frame's live count are never read: NaN points; their perm entries name the frame's last (NaN) row."""
    F = len(frames)
    pcd = np.full((F, cap, 6), np.nan, np.float32)
    perm = np.full((F, cap), cap - 1, np.int32)
    n = np.array([len(f) for f in frames], np.int32)
    for k, f in enumerate(frames):
        assert len(f) <= cap
        pcd[k, :len(f)] = f
        perm[k, :len(f)] = np.random.default_rng(77 + 13 * k + len(f)).permutation(len(f))
    for a in (pcd, perm, n):
        a.setflags(write=False)
    return FrameSet(name, pcd, perm, n, cap)


MANY63_N = tuple((37 * f) % 1101 for f in range(63))


@functools.lru_cache(maxsize=None)
def case(name):
    if name == 'single':
        return frame_set(name, [np.concatenate([crowd(1), edges(), uniform(2, 400)])], CAP)
    if name == 'ragged4':
        return frame_set(name, [full_mix(3, 1100), np.zeros((0, 6), np.float32), uniform(4, 37), crowd(5)], CAP)
    if name == 'ends_empty':
        z = np.zeros((0, 6), np.float32)
        return frame_set(name, [z, full_mix(6, 700), z], CAP)
    if name in ('aligned1024', 'aligned1023'):
        cap = int(name[-4:])
        return frame_set(name, [full_mix(10 + k, cap) for k in range(3)], cap)
    if name == 'many63':
        return frame_set(name, [sampled_mix(100 + f, n) for f, n in enumerate(MANY63_N)], CAP)
    raise KeyError(name)


def stream(fs, f):
    """The live points of frame f in stream order."""
    n = int(fs.n_points[f])
    return fs.pcd[f][fs.perm[f, :n]]


def oracle_indices(fs, size=SIZE):
    """i32 (F, cap, 3): the oracle's voxel index of every stream position (the ``ext_idx`` input); -7 past the live count."""
    ext = np.full(fs.perm.shape + (3,), -7, np.int32)
    for f in range(len(fs.n_points)):
        ext[f, :fs.n_points[f]] = O.voxel_index(stream(fs, f)[:, :3], RNG, size)
    return ext


@functools.lru_cache(maxsize=None)
def oracle_frames(name, T, C, ncol=6, use_perm=True, size=None):
    """Per frame (voxels f32 (V, T, C), indices i64 (V, 3), counts i32 (V,)) of the oracle.  ncol = 4: the kernel reads x y z r
    only and writes zeros for row / col.  use_perm = False: the stream is the storage order."""
    fs = case(name)
    out = []
    for f in range(len(fs.n_points)):
        n = int(fs.n_points[f])
        pts = fs.pcd[f, :n].copy()
        if ncol == 4:
            pts[:, 4:] = 0
        perm = fs.perm[f, :n] if use_perm else np.arange(n, dtype=np.int32)
        fn = O.group if C == 9 else O.group7
        v, i, c = fn(pts, perm, RNG, list(size) if size else list(SIZE), T)
        out.append((v.astype(np.float32), i.astype(np.int64).reshape(-1, 3), c.astype(np.int32)))
    return out


def layout(frames, concat):
    """How per-frame results become the outputs of mvx_voxelize_frames.  n_voxels[f] = voxels of frame f, vox_off = its
    cumulative sum from 0.  concat = 0: a list over the frames, coords = (0, ix, iy, iz).  concat != 0: the frames' voxels back
    to back in frame order, coords = (frame, ix, iy, iz)."""
    nv = np.array([len(c) for _, _, c in frames], np.int32)
    off = np.concatenate([[0], np.cumsum(nv)]).astype(np.int32)
    coords = [np.concatenate([np.full((len(i), 1), f if concat else 0, np.int64), i], 1) for f, (_, i, _) in enumerate(frames)]
    if not concat:
        return Expected([v for v, _, _ in frames], coords, [c for _, _, c in frames], nv, off)
    return Expected(np.concatenate([v for v, _, _ in frames]), np.concatenate(coords), np.concatenate([c for _, _, c in frames]),
                    nv, off)


def expected(name, T, C, concat, ncol=6, use_perm=True, size=None):
    return layout(oracle_frames(name, T, C, ncol, use_perm, size), concat)
