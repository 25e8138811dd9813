"""Inputs of tests/test_sparse_first_host.py and tests/test_sparse_first_gpu.py: voxel sets placed where the kernels of the sparse
first CML layer can go wrong, and dyadic / random values for them.  Pure numpy: the host test checks the properties claimed here
on exactly the arrays the GPU test uploads."""
import functools

import numpy as np

import sparse_ref as R

# (din, H, W, sd, pd) of the FIRST layer
GEOMS = {
    'model': (10, 37, 53, 2, 1),        # the model's conv1 depth geometry; partial last tile row and column; W % 4 != 0: scalar dilation
    'vec4': (5, 40, 48, 1, 0),          # W % 4 == 0: the four-sites-per-thread dilation
    'ragged4': (3, 24, 36, 1, 1),       # W % 4 == 0 and W % 16 != 0
    'onetile': (5, 8, 16, 2, 1),        # exactly one tile
    # 9 x 7 tiles.  With fewer than 7 tile rows or 5 tile columns every tile has a unit on the image border in its 3 x 3
    # neighbourhood, units on the border are always computed, and mvx_tile_read_flags marks every tile of every plane that has a
    # reader: only an image this large can hold a tile that is NOT read (the unit rows (0,1) and (8) touch the border, tile
    # row 3 sees only the units (2,3) and (4,5); the lone voxel below makes the tile columns 0..3 read: tile (3, 4) is not).
    # Its voxel at (60, 70) flags the halo of tile (7, 4) alone: the unit (6,7) of column 4 is computed because of its SECOND
    # tile row only.  Tile bookkeeping tests only.
    'wide': (10, 72, 112, 2, 1),
}
# layers 2 and 3 of the chain grid_activity builds behind the first layer: (sd, pd) of conv2 and conv3
CHAIN = ((1, 0), (2, 1))
# frames -> the empty ones.  4: frame 1 empty; 16 = MVX_MAX_FRAMES: the first, one in the middle and the last
EMPTY = {1: (), 4: (1,), 16: (0, 9, 15)}
TARGET_VOXELS = 210


def geom(name, F):
    return R.Geom(*GEOMS[name], F)


def block_origin(name):
    """(z0, y0, x0) of the full 3 x 3 x 3 voxel block of the first non-empty frame: its centre site (the local output plane that
    reads z0 .. z0 + 2 through kd = 0 .. 2) sums 27 terms.  Astride a tile corner where the image has one."""
    din, H, W, sd, pd = GEOMS[name]
    z0 = 1 if sd == 2 else (0 if pd == 1 else 1)          # d * sd - pd == z0 for a valid d
    return (z0, 6, 14) if H > 8 and W > 16 else (z0, 2, 5)


@functools.lru_cache(None)
def voxels(name, F):
    """-> (coords i64 [V][4], vox_off [F + 1]).  Unique sites.  Every non-empty frame holds: the corners (0,0,0) and
    (D-1,H-1,W-1); a voxel in its last plane and one in plane 0 at the same (y, x) = (3, 9), so that a gather or a dilation that
    crosses into the neighbouring frame meets a voxel; both sides of every tile edge (y in {7, 8} x x in {15, 16}), the last row
    and the last column; a LONE voxel in the corner (16, 32) of tile (2, 2) in plane D // 2, which the tiles (1,1), (1,2) and (2,1)
    see through their halo only (the last-row and last-column voxels lie in plane 0), and a voxel at (20, 17) of that plane,
    whose dilation reaches column 16: tile (2, 0) sees it in its halo and not inside, so halo and tile flags differ; on 'wide'
    a voxel at (60, 70) of that plane (see GEOMS); random fillers in the first tile row (y < 8), so that planes without a placed
    voxel are empty from y = 9 on.  The first non-empty frame also holds the full 3 x 3 x 3 block (rows 6..8, columns 14..16)."""
    din, H, W, sd, pd = GEOMS[name]
    rng = np.random.default_rng(sorted(GEOMS).index(name) * 100 + F)
    live = [f for f in range(F) if f not in EMPTY[F]]
    coords, vox_off = [], [0]
    for f in range(F):
        sites = []

        def put(z, y, x):
            if 0 <= z < din and 0 <= y < H and 0 <= x < W and (z, y, x) not in sites:
                sites.append((z, y, x))
        if f in live:
            put(0, 0, 0), put(din - 1, H - 1, W - 1)
            put(din - 1, 3, 9), put(0, 3, 9)
            if H > 8 and W > 16:
                for y in (7, 8):
                    for x in (15, 16):
                        put(1, y, x)
                put(0, H - 1, W - 2), put(0, 5, W - 1)
                put(din // 2, 16, 32), put(din // 2, 20, 17)
                if H >= 72:
                    put(din // 2, 60, 70)
            if f == live[0]:
                z0, y0, x0 = block_origin(name)
                for dz in range(3):
                    for dy in range(3):
                        for dx in range(3):
                            put(z0 + dz, y0 + dy, x0 + dx)
            want = max(len(sites) + 4, TARGET_VOXELS // len(live))
            while len(sites) < want:
                put(int(rng.integers(din)), int(rng.integers(min(H, 8))), int(rng.integers(W)))
        rng.shuffle(sites)                                  # voxel ids carry no spatial order
        coords += [(f, y, x, z) for z, y, x in sites]
        vox_off.append(len(coords))
    if len(coords) % 16 == 0:                               # V * 27 * C / 4 threads of the gather: no multiple of 256 for C = 16, 64
        f = live[-1]
        taken = {c[1:] for c in coords[vox_off[f]:vox_off[f + 1]]}
        extra = next((f, y, x, 2) for y in range(min(H, 8)) for x in range(W) if (y, x, 2) not in taken)
        coords.insert(vox_off[f + 1], extra)
        vox_off = [o + (i > f) for i, o in enumerate(vox_off)]
    return np.asarray(coords, np.int64).reshape(-1, 4), vox_off


def with_out_of_range(name, F):
    """The voxel set followed by three voxels with iy = -1, ix = W and iz = D (in the last frame)."""
    din, H, W, _, _ = GEOMS[name]
    coords, vox_off = voxels(name, F)
    bad = np.asarray([(0, -1, 2, 1), (0, 2, W, 1), (0, 2, 3, din)], np.int64)
    return np.concatenate([coords, bad]), vox_off[:-1] + [vox_off[-1] + 3]


def dyadic(rng, shape):
    """Multiples of 1/4 with magnitude <= 2."""
    return rng.integers(-8, 9, shape) / 4.0


@functools.lru_cache(None)
def values(name, F, C, kind):
    """-> (P [V][27 * C], bias [C], dz [F * dout][H][W][C]) in float64 holding f32 values.  'dyadic': multiples of 1/4, |.| <= 2,
    biases of both signs (and a zero); 'random': standard normal."""
    g = geom(name, F)
    V = len(voxels(name, F)[0])
    rng = np.random.default_rng(7 * C + F + (1000 if kind == 'random' else 0))
    shapes = ((V, 27 * C), (C,), (F * g.dout, g.H, g.W, C))
    if kind == 'dyadic':
        P, bias, dz = (dyadic(rng, s) for s in shapes)
        bias[:3] = (-1.75, 0.0, 1.25)
    else:
        P, bias, dz = (rng.standard_normal(s).astype(np.float32).astype(np.float64) for s in shapes)
    return P, bias, dz


@functools.lru_cache(None)
def reference_grid(name, F):
    din, H, W, _, _ = GEOMS[name]
    coords, vox_off = voxels(name, F)
    return R.index_grid(coords, vox_off, din, H, W)


@functools.lru_cache(None)
def reference_chain(name, F):
    """The three layers of grid_activity in the reference: [(din, sd, pd, mark_border, (mask, halo, tile))]; the first from the
    index grid, the next two from the previous mask with the image border marked."""
    g = geom(name, F)
    grid, _, _ = reference_grid(name, F)
    layers, src, din = [], grid >= 0, g.din
    for li, (sd, pd) in enumerate(((g.sd, g.pd),) + CHAIN):
        res = R.dilate(src, din, sd, pd, F, li > 0)
        layers.append((din, sd, pd, li > 0, res))
        src, din = res[0] != 0, R.out_depth(din, sd, pd)
    return layers
