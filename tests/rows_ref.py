"""Host reference of the voxel-row glue kernels (csrc/vfe.hip and the row half of csrc/fusion.hip) for
tests/test_rows_glue_gpu.py: numpy, float64, explicit loops over voxels and rows.  It restates the layouts from
include/mvx_hip.h ("Compact rows", "Frame sets") and the header comments of the two kernel files and imports nothing of the
package.

Layouts.  A voxel holds T sampled rows.
  dense    matrix row v * T + t, all T rows stored.
  compact  voxel v stores its vcnt[v] real rows at matrix rows voff[v] .. voff[v] + vcnt[v] - 1 and ONE padded row at matrix
           row n_real + v that stands for the T - vcnt[v] identical padded rows (n_real = all real rows).  The padded row is
           ALWAYS stored; it takes part in the maximum only when it stands for at least one row (vcnt[v] < T).  A voxel may
           have no real row at all (vcnt = 0, voff = 0): only its padded row is read.
  frame set  the voxels of frame f are vox_off[f] .. vox_off[f+1]-1, its real rows real_off[f] .. real_off[f+1]-1; all real rows
           of all frames come first, then one padded row per voxel.  Per-frame quantities carry a leading frame axis.
Local row index t of a voxel: 0 .. vcnt-1 are its real rows in stored order, t = vcnt is the padded row."""
import numpy as np


class Layout:
    """T rows per voxel; vcnt None = dense, else the real rows per voxel (compact); vox_off None = one frame."""

    def __init__(self, T, V, vcnt=None, vox_off=None):
        self.T, self.V = int(T), int(V)
        self.compact = vcnt is not None
        self.vox_off = [0, self.V] if vox_off is None else [int(v) for v in vox_off]
        self.F = len(self.vox_off) - 1
        assert self.vox_off[0] == 0 and self.vox_off[-1] == self.V
        if self.compact:
            self.vcnt = np.asarray(vcnt, np.int64)
            assert self.vcnt.shape == (self.V,) and self.vcnt.min() >= 0 and self.vcnt.max() <= self.T
            first = np.cumsum(self.vcnt) - self.vcnt
            self.voff = np.where(self.vcnt > 0, first, 0)
            self.n_real = int(self.vcnt.sum())
            self.rows = self.n_real + self.V
            self.real_off = [int(self.vcnt[:v].sum()) for v in self.vox_off]
        else:
            self.vcnt = self.voff = None
            self.n_real = 0
            self.rows = self.V * self.T
            self.real_off = None

    def frame_of(self, v):
        for f in range(self.F):
            if self.vox_off[f] <= v < self.vox_off[f + 1]:
                return f
        raise IndexError(v)

    def stored(self, v):
        """Matrix rows stored for voxel v, in local order (the padded row last)."""
        if not self.compact:
            return [v * self.T + t for t in range(self.T)]
        return [int(self.voff[v]) + t for t in range(int(self.vcnt[v]))] + [self.n_real + v]

    def in_max(self, v):
        """The stored rows that take part in the maximum: the padded row only when it stands for a row."""
        rows = self.stored(v)
        return rows if not self.compact or self.vcnt[v] < self.T else rows[:-1]

    def weight(self, v):
        """Dense rows each stored row of voxel v stands for."""
        if not self.compact:
            return [1] * self.T
        return [1] * int(self.vcnt[v]) + [self.T - int(self.vcnt[v])]


def _mi(mean_inv, L, v):
    mi = np.asarray(mean_inv, np.float64)
    return mi[L.frame_of(v)] if mi.ndim == 3 else mi


def normalise(y, mean_inv, L):
    """(y - mean) * inv of every stored row with its own frame's statistics; rows no voxel stores stay NaN."""
    y = np.asarray(y, np.float64)
    out = np.full(y.shape, np.nan)
    for v in range(L.V):
        mi = _mi(mean_inv, L, v)
        for r in L.stored(v):
            out[r] = (y[r] - mi[0]) * mi[1]
    return out


def bn_max(y, mean_inv, L):
    """Per voxel and channel: maximum of the normalised rows that take part and the local index of the FIRST maximal row in
    stored order (csrc/vfe.hip: "first maximum wins").  -> (yhat (rows, C), feat (V, C), argmax (V, C))."""
    yh = normalise(y, mean_inv, L)
    C = yh.shape[1]
    feat = np.empty((L.V, C))
    am = np.empty((L.V, C), np.int64)
    for v in range(L.V):
        rows = L.in_max(v)
        best = np.full((C,), -np.inf)
        bi = np.zeros((C,), np.int64)
        for t, r in enumerate(rows):
            better = yh[r] > best                      # strictly greater: an equal later row does not replace an earlier one
            best = np.where(better, yh[r], best)
            bi = np.where(better, t, bi)
        feat[v], am[v] = best, bi
    return yh, feat, am


def bn_max_concat(y, mean_inv, L):
    """One VFE layer's glue: out = [yhat | the voxel's maximum broadcast to every stored row], argmax."""
    yh, feat, am = bn_max(y, mean_inv, L)
    out = np.full((yh.shape[0], 2 * yh.shape[1]), np.nan)
    for v in range(L.V):
        for r in L.stored(v):
            out[r] = np.concatenate([yh[r], feat[v]])
    return out, am


def max_concat_backward(g, am, L):
    """Adjoint of bn_max_concat wrt yhat.  g (rows, 2C) is the gradient of the STORED rows: the padded row's entry is ONE
    stored value that the caller has already summed over the rows it stands for, so it enters every sum once.  The gradient
    of the maximum, summed over the voxel's stored rows, goes to the argmax row; every stored row also keeps g[:, :C]."""
    g = np.asarray(g, np.float64)
    C = g.shape[1] // 2
    d = np.full((g.shape[0], C), np.nan)
    for v in range(L.V):
        rows = L.stored(v)
        s = np.zeros((C,))
        for r in rows:
            s += g[r, C:]
        for t, r in enumerate(rows):
            d[r] = g[r, :C] + np.where(am[v] == t, s, 0.0)
    return d


def segment_max_backward(dfeat, am, L):
    """Adjoint of the head's maximum: the selected row gets dfeat, every other stored row exactly 0."""
    dfeat = np.asarray(dfeat, np.float64)
    C = dfeat.shape[1]
    d = np.full((L.rows, C), np.nan)
    for v in range(L.V):
        for t, r in enumerate(L.stored(v)):
            d[r] = np.where(am[v] == t, dfeat[v], 0.0)
    return d


# ---- bookkeeping ---------------------------------------------------------------------------------------------------------
def compact_map(vox):
    """Dense voxel rows (R, vc): a row whose x == y == z == 0 is padding.  -> (row_map (R,): rank of a real row among the real
    rows, -1 for padding; rows_sel (n_real,): the inverse list; n_real; the rows with channels 3.. of padding rows zeroed)."""
    vox = np.array(vox, np.float32)
    R = vox.shape[0]
    row_map = np.full((R,), -1, np.int64)
    rows_sel = []
    for r in range(R):
        if vox[r, 0] == 0 and vox[r, 1] == 0 and vox[r, 2] == 0:
            vox[r, 3:] = 0
        else:
            row_map[r] = len(rows_sel)
            rows_sel.append(r)
    return row_map, np.asarray(rows_sel, np.int64), len(rows_sel), vox


def real_offsets(row_map, vox_off, T):
    """real_off[f] = real rows before frame f's first dense row, real_off[F] = all real rows."""
    row_map = np.asarray(row_map)
    return np.asarray([int((row_map[:v * T] >= 0).sum()) for v in vox_off], np.int64)


def row_offsets(row_map, V, T):
    """-> voff (first compact row of the voxel, 0 without a real row), vcnt, row_w (n_real + V,): 1 for a real row,
    T - vcnt[v] for the padded row of voxel v."""
    row_map = np.asarray(row_map).reshape(V, T)
    n_real = int((row_map >= 0).sum())
    voff, vcnt = np.zeros((V,), np.int64), np.zeros((V,), np.int64)
    row_w = np.ones((n_real + V,))
    for v in range(V):
        real = [int(j) for j in row_map[v] if j >= 0]
        vcnt[v] = len(real)
        voff[v] = real[0] if real else 0
        row_w[n_real + v] = T - len(real)
    return voff, vcnt, row_w


def fusion_row_weights(vox_off, real_off, T):
    """Row weights of the fusion layout [real rows][one shared padded row per frame]: the shared row of frame f stands for
    every padded row of f = (voxels of f) * T - (real rows of f)."""
    F = len(vox_off) - 1
    w = np.ones((real_off[F] + F,))
    for f in range(F):
        w[real_off[F] + f] = (vox_off[f + 1] - vox_off[f]) * T - (real_off[f + 1] - real_off[f])
    return w


# ---- VFE-1 input -----------------------------------------------------------------------------------------------------------
def compact_input(vox, rows_sel, imfeat, L, pitch=None):
    """Real row j = [vox[rows_sel[j]][0:7] | imfeat[j]]; the padded row of voxel v = [0 x 7 | imfeat[n_real + frame(v)]] (its own
    frame's shared row); columns from 7 + F up to the pitch are zero."""
    imfeat = np.asarray(imfeat, np.float64)
    Fc = imfeat.shape[1]
    pitch = 7 + Fc if pitch is None else pitch
    out = np.zeros((L.rows, pitch))
    for j in range(L.n_real):
        out[j, :7] = vox[rows_sel[j], :7]
        out[j, 7:7 + Fc] = imfeat[j]
    for v in range(L.V):
        out[L.n_real + v, 7:7 + Fc] = imfeat[L.n_real + L.frame_of(v)]
    return out


def compact_input_backward(g, Fc, L):
    """Gradient wrt imfeat (n_real + F, Fc): real rows copy columns 7..7+Fc, frame f's shared row sums them over the padded
    rows of f's voxels."""
    g = np.asarray(g, np.float64)
    d = np.zeros((L.n_real + L.F, Fc))
    for j in range(L.n_real):
        d[j] = g[j, 7:7 + Fc]
    for v in range(L.V):
        d[L.n_real + L.frame_of(v)] += g[L.n_real + v, 7:7 + Fc]
    return d


def expand_rows(compact, row_map, pad_row):
    compact = np.asarray(compact, np.float64)
    return np.stack([compact[j if j >= 0 else pad_row] for j in row_map])


def expand_rows_backward(g, row_map, pad_row, n_compact):
    """Real rows copy, the shared row sums the padded rows; compact rows nothing maps to stay NaN (not written)."""
    g = np.asarray(g, np.float64)
    d = np.full((n_compact, g.shape[1]), np.nan)
    d[pad_row] = 0.0
    for r, j in enumerate(row_map):
        if j >= 0:
            d[j] = g[r]
        else:
            d[pad_row] += g[r]
    return d


# ---- weighted BatchNorm over compact rows -------------------------------------------------------------------------------------
def dense_expansion(L, f):
    """(stored row, copies) of frame f in the dense tensor it stands for: a padded row is repeated T - vcnt times."""
    pairs = []
    for v in range(L.vox_off[f], L.vox_off[f + 1]):
        pairs += [(r, w) for r, w in zip(L.stored(v), L.weight(v)) if w > 0]
    return pairs


def bn_forward(y, L, eps):
    """Per frame: mean and 1 / sqrt(var + eps) (biased variance) over the dense expansion; NaN for a frame without voxels (no
    population).  -> (F, 2, C)"""
    y = np.asarray(y, np.float64)
    mi = np.full((L.F, 2, y.shape[1]), np.nan)
    for f in range(L.F):
        pairs = dense_expansion(L, f)
        if not pairs:
            continue
        dense = np.stack([y[r] for r, w in pairs for _ in range(w)])
        mean = dense.mean(0)
        var = ((dense - mean) ** 2).mean(0)
        mi[f] = mean, 1.0 / np.sqrt(var + eps)
    return mi


def bn_relu_backward(dyhat, y, mi, L):
    """Gradient of yhat = BN(y), y = relu(z), wrt z on the dense expansion, folded back onto the stored rows.  dyhat of a padded row
    is the already summed gradient of its copies (each copy gets an equal share: the result does not depend on the split);
    its dz is the sum over the copies.  A stored row that stands for no dense row has no dz (NaN).  -> (dz, dbias)"""
    dyhat, y = np.asarray(dyhat, np.float64), np.asarray(y, np.float64)
    dz = np.full(y.shape, np.nan)
    dbias = np.zeros((y.shape[1],))
    for f in range(L.F):
        pairs = dense_expansion(L, f)
        if not pairs:
            continue
        idx = [r for r, w in pairs for _ in range(w)]
        share = np.asarray([1.0 / w for r, w in pairs for _ in range(w)])[:, None]
        yd, gd = y[idx], dyhat[idx] * share
        yh = (yd - mi[f, 0]) * mi[f, 1]
        N = len(idx)
        dzd = mi[f, 1] * (gd - gd.sum(0) / N - yh * (gd * yh).sum(0) / N) * (yd > 0)
        k = 0
        for r, w in pairs:
            dz[r] = dzd[k:k + w].sum(0)
            k += w
        dbias += dzd.sum(0)
    return dz, dbias


# ---- image-feature sampling --------------------------------------------------------------------------------------------------
def sample_rows(vox, rows_sel, frame_of_row, maps, imsize_hw, eps):
    """csrc/fusion.hip's header, per real row j (dense row rows_sel[j]) and level: in float32, operation for operation,
        q = proj / (imsize / feat_hw) - eps ;  i = trunc(q) ;  f = q - i        (proj = the row's last two columns: row, column)
    then in float64, on the map zero-padded by one row and one column,
        out = F[i,j]*fr*fc + F[i+1,j]*(1-fr)*fc + F[i,j+1]*fr*(1-fc) + F[i+1,j+1]*(1-fr)*(1-fc)
    (fr, fc: the row and column fractions; 1 - f formed in float32).  A sample with i < 0 or i + 1 > H (or the same in the
    column) is flagged: zeros, status bit 0.  maps[f][level]: (H, W, C) of frame f.
    -> (out (n, L*C) float64, mag (n, L*C) = sum over the taps of |F_tap * weight_tap|, flagged (n, L) bool)"""
    f32 = np.float32
    nl, C = len(maps[0]), maps[0][0].shape[2]
    n = len(rows_sel)
    out, mag = np.zeros((n, nl * C)), np.zeros((n, nl * C))
    flagged = np.zeros((n, nl), bool)
    for j in range(n):
        v = np.asarray(vox[rows_sel[j]], f32)
        for lv in range(nl):
            M = np.asarray(maps[frame_of_row[j]][lv], np.float64)
            H, W = M.shape[:2]
            qr = f32(f32(v[-2] / f32(f32(imsize_hw[0]) / f32(H))) - f32(eps))
            qc = f32(f32(v[-1] / f32(f32(imsize_hw[1]) / f32(W))) - f32(eps))
            ir, ic = int(np.trunc(qr)), int(np.trunc(qc))
            fr, fc = f32(qr - f32(ir)), f32(qc - f32(ic))
            if ir < 0 or ic < 0 or ir + 1 > H or ic + 1 > W:
                flagged[j, lv] = True
                continue
            P = np.zeros((H + 1, W + 1, C))
            P[:H, :W] = M
            fr_, fc_ = f32(f32(1) - fr), f32(f32(1) - fc)
            taps = ((P[ir, ic], fr, fc), (P[ir + 1, ic], fr_, fc), (P[ir, ic + 1], fr, fc_), (P[ir + 1, ic + 1], fr_, fc_))
            for val, a, b in taps:
                term = val * float(a) * float(b)
                out[j, lv * C:(lv + 1) * C] += term
                mag[j, lv * C:(lv + 1) * C] += np.abs(term)
    return out, mag, flagged
