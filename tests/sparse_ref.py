"""Plain numpy reference of the sparse first CML layer and its tile bookkeeping, written from the header comments of
include/mvx_hip.h ("Input-sparse first convolution", "mvx_activity_dilate ... mvx_tile_read_flags_frames"): float64 and integers,
loops over voxels, taps and tiles.  Where the kernels GATHER (one thread per output site or tile looks at its sources), these
functions SCATTER (every voxel, active site or computed tile marks what reads it), so the two share the conventions below and
nothing else.  tests/test_sparse_first_host.py holds every function against torch in float64.

Conventions (those of the library):
  coords[v] = (unused, iy in [0, H), ix in [0, W), iz in [0, D)); the frame of voxel v follows from vox_off;
  frames are stacked along depth: the global plane of (frame f, local plane z) is f * D + z;
  output site (d, y, x) of a frame reads source (d * sd - pd + kd, y + a - 1, x + b - 1) of the SAME frame through the P row
  v * 27 + kd * 9 + a * 3 + b of the voxel v there; sources outside the frame's grid do not exist (zero padding);
  tiles are 8 rows x 16 columns, tile index ty * ceil(W / 16) + tx; the last tile row / column may be partial."""
import collections

import numpy as np

TH, TW = 8, 16


class Geom(collections.namedtuple('Geom', 'din H W sd pd F')):
    """Depth geometry of one layer (planes PER FRAME) on an H x W image, F frames."""
    __slots__ = ()

    @property
    def dout(self):
        return out_depth(self.din, self.sd, self.pd)

    @property
    def tiles(self):
        return tiles_of(self.H, self.W)


def out_depth(din, sd, pd):
    return (din + 2 * pd - 3) // sd + 1


def tiles_of(H, W):
    return -(-H // TH), -(-W // TW)


def frame_of(v, vox_off):
    """The frame whose voxel range [vox_off[f], vox_off[f + 1]) holds v."""
    for f in range(len(vox_off) - 1):
        if vox_off[f] <= v < vox_off[f + 1]:
            return f
    raise ValueError('voxel %d lies in no frame' % v)


def readers(z, din, dout, sd, pd):
    """[(local output plane, kd)] that read local source plane z: d * sd - pd + kd == z."""
    res = []
    for kd in range(3):
        t = z + pd - kd
        if t >= 0 and t % sd == 0 and t // sd < dout:
            res.append((t // sd, kd))
    return res


def sources(d, din, sd, pd):
    """[(local source plane, kd)] that local output plane d reads."""
    return [(d * sd - pd + kd, kd) for kd in range(3) if 0 <= d * sd - pd + kd < din]


# ---- mvx_index_grid_frames -------------------------------------------------------------------------------------------------------
def index_grid(coords, vox_off, D, H, W):
    """-> (site grid i32 [F * D][H][W], -1 = empty; occupancy counts i32 [F * D][tiles_y][tiles_x]; status: bit 0 (value 1) set
    when a coordinate was out of range -- that voxel is dropped)."""
    F = len(vox_off) - 1
    ty, tx = tiles_of(H, W)
    grid = np.full((F * D, H, W), -1, np.int32)
    occ = np.zeros((F * D, ty, tx), np.int32)
    status = 0
    for v in range(len(coords)):
        _, iy, ix, iz = (int(c) for c in coords[v])
        if not (0 <= iy < H and 0 <= ix < W and 0 <= iz < D):
            status |= 1
            continue
        p = frame_of(v, vox_off) * D + iz
        grid[p, iy, ix] = v
        occ[p, iy // TH, ix // TW] += 1
    return grid, occ, status


# ---- mvx_activity_dilate_frames ----------------------------------------------------------------------------------------------------
def dilate(src_active, din, sd, pd, F, mark_border):
    """src_active bool [F * din][H][W] -> (mask u8 [F * dout][H][W]: the 3 x 3 x 3 receptive field of the site holds an active
    source, or (mark_border) its in-plane window leaves the image; halo_flags i32 [F * dout][tiles_y][tiles_x]: the
    (8 + 2) x (16 + 2) window of the tile, clipped to the image, holds a masked site of that plane; tile_flags: the tile does)."""
    src_active = np.asarray(src_active)
    _, H, W = src_active.shape
    dout = out_depth(din, sd, pd)
    mask = np.zeros((F * dout, H, W), np.uint8)
    if mark_border:
        mask[:, 0, :] = mask[:, H - 1, :] = 1
        mask[:, :, 0] = mask[:, :, W - 1] = 1
    for p, y, x in np.argwhere(src_active):
        f, z = divmod(int(p), din)
        for d, _ in readers(z, din, dout, sd, pd):
            for a in range(3):
                for b in range(3):
                    yo, xo = y - (a - 1), x - (b - 1)
                    if 0 <= yo < H and 0 <= xo < W:
                        mask[f * dout + d, yo, xo] = 1
    ty, tx = tiles_of(H, W)
    halo = np.zeros((F * dout, ty, tx), np.int32)
    tile = np.zeros((F * dout, ty, tx), np.int32)
    for p in range(F * dout):
        for i in range(ty):
            for j in range(tx):
                y0, x0 = i * TH, j * TW
                tile[p, i, j] = int(mask[p, y0:y0 + TH, x0:x0 + TW].any())
                halo[p, i, j] = int(mask[p, max(y0 - 1, 0):y0 + TH + 1, max(x0 - 1, 0):x0 + TW + 1].any())
    return mask, halo, tile


# ---- mvx_tile_dilate_flags_frames ------------------------------------------------------------------------------------------------
def tile_dilate(in_flags, self_flags, din, dout, sd, pd, F):
    """out[d][t] = self[d][t] | any tile of the 3 x 3 neighbourhood of t flagged in an input plane that d reads through a depth tap.
    in_flags [F * din][tiles_y][tiles_x], self_flags (or None) and the result [F * dout][tiles_y][tiles_x]."""
    in_flags = np.asarray(in_flags)
    _, ty, tx = in_flags.shape
    out = np.zeros((F * dout, ty, tx), np.int32)
    if self_flags is not None:
        out[np.asarray(self_flags) != 0] = 1
    for p, i, j in np.argwhere(in_flags != 0):
        f, z = divmod(int(p), din)
        for d, _ in readers(z, din, dout, sd, pd):
            out[f * dout + d, max(i - 1, 0):i + 2, max(j - 1, 0):j + 2] = 1
    return out


# ---- mvx_tile_read_flags_frames --------------------------------------------------------------------------------------------------
def computed_tiles(halo_flags, din, dout, sd, pd, F):
    """bool [F * dout][tiles_y][tiles_x]: the output tiles the background-aware gather computes.  Units pair the tile rows 2k and
    2k + 1 (the last unit of an odd tile-row count is its single row); a unit touching the image border is always computed,
    another one when either of its tiles has a flagged source halo in a valid depth tap."""
    halo_flags = np.asarray(halo_flags)
    _, ty, tx = halo_flags.shape
    comp = np.zeros((F * dout, ty, tx), bool)
    for f in range(F):
        for d in range(dout):
            for k in range((ty + 1) // 2):
                rows = [r for r in (2 * k, 2 * k + 1) if r < ty]
                for j in range(tx):
                    on = j == 0 or j == tx - 1 or rows[0] == 0 or rows[-1] == ty - 1
                    for z, _ in sources(d, din, sd, pd):
                        on = on or any(halo_flags[f * din + z, r, j] != 0 for r in rows)
                    for r in rows:
                        comp[f * dout + d, r, j] = on
    return comp


def tile_read(halo_flags, din, dout, sd, pd, F):
    """read i32 [F * din][tiles_y][tiles_x]: a computed output tile (computed_tiles) marks its 3 x 3 tile neighbourhood in every
    valid source plane of its output plane."""
    comp = computed_tiles(halo_flags, din, dout, sd, pd, F)
    _, ty, tx = comp.shape
    read = np.zeros((F * din, ty, tx), np.int32)
    for p, i, j in np.argwhere(comp):
        f, d = divmod(int(p), dout)
        for z, _ in sources(d, din, sd, pd):
            read[f * din + z, max(i - 1, 0):i + 2, max(j - 1, 0):j + 2] = 1
    return read


# ---- mvx_sparse_conv_output*_frames ------------------------------------------------------------------------------------------------
def sparse_output(P, grid, bias, geometry, relu):
    """out f64 [F * dout][H][W][C] = [ReLU](bias + sum of the P rows of the <= 27 source voxels of each site), and the per-frame
    BatchNorm sums f64 [F][2][C] (sum, sum of squares over all dout * H * W sites of the frame).  P [V][27 * C], grid as index_grid."""
    g = geometry
    bias = np.asarray(bias, np.float64)
    C = bias.shape[0]
    P = np.asarray(P, np.float64).reshape(-1, 27, C)
    out = np.empty((g.F * g.dout, g.H, g.W, C), np.float64)
    out[:] = bias
    for p, y, x in np.argwhere(grid >= 0):
        v = int(grid[p, y, x])
        f, z = divmod(int(p), g.din)
        for d, kd in readers(z, g.din, g.dout, g.sd, g.pd):
            for a in range(3):
                for b in range(3):
                    yo, xo = y - (a - 1), x - (b - 1)
                    if 0 <= yo < g.H and 0 <= xo < g.W:
                        out[f * g.dout + d, yo, xo] += P[v, kd * 9 + a * 3 + b]
    if relu:
        out = np.maximum(out, 0.0)
    per_frame = out.reshape(g.F, -1, C)
    return out, np.stack([per_frame.sum(1), (per_frame * per_frame).sum(1)], axis=1)


def sparse_output_magnitude(P, grid, bias, geometry):
    """|bias| + sum |terms| per output element: what a rounding-error bound of the f32 sum scales with."""
    return sparse_output(np.abs(P), grid, np.abs(bias), geometry, False)[0]


def tile_sites(flags, H, W):
    """bool [planes][H][W]: the sites of the tiles whose flag [planes][tiles_y][tiles_x] is non-zero."""
    flags = np.asarray(flags) != 0
    return np.repeat(np.repeat(flags, TH, axis=1), TW, axis=2)[:, :H, :W]


# ---- mvx_sparse_conv_gather_dz_frames ----------------------------------------------------------------------------------------------
def gather_dz(dz, coords, vox_off, geometry):
    """G f64 [V][27 * C]: G[v][tap * C + c] = dz at the output site that read voxel v through tap (kd, a, b), zero if none."""
    g = geometry
    dz = np.asarray(dz, np.float64)
    C = dz.shape[-1]
    G = np.zeros((len(coords), 27, C), np.float64)
    for v in range(len(coords)):
        _, iy, ix, iz = (int(c) for c in coords[v])
        f = frame_of(v, vox_off)
        for d, kd in readers(iz, g.din, g.dout, g.sd, g.pd):
            for a in range(3):
                for b in range(3):
                    yo, xo = iy - (a - 1), ix - (b - 1)
                    if 0 <= yo < g.H and 0 <= xo < g.W:
                        G[v, kd * 9 + a * 3 + b] = dz[f * g.dout + d, yo, xo]
    return G.reshape(len(coords), 27 * C)
