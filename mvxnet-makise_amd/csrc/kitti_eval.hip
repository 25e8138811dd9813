// KITTI object AP evaluation (2D bbox, BEV, 3D, AOS; R11 and R40) of all frames of a split, in the semantics of the widely
// used kitti-object-eval-python tool (DESIGN.md section 3.17 states them).  Every stage covers all frames in one launch:
//   1. eval_overlaps  (one thread per (frame, GT, detection) pair, then per (frame, don't-care, detection) pair): the 2D IoU,
//                     the BEV IoU from bev_iou.h's f32 rotated intersection (bounding-circle rejection first) and the 3D IoU,
//                     f64; detection vs don't-care as intersection / detection area;
//   2. eval_tp_scores (one wave per (frame, curve)): the threshold pass (compute_fp = false): GTs in order, the detections
//                     spread over the lanes, a wave-wide arg-best by (score desc, index asc), the assigned set one u64 per
//                     lane; writes the TP scores into fixed per-(curve, frame) slots and the frame's valid GT count;
//   (the caller sorts every curve's slots in descending order)
//   3. eval_thresholds (one wave per curve): get_thresholds -- at most 41 scores picked by a ballot per pick;
//   4. eval_counts    (one wave per (frame, curve, threshold)): compute_fp = true; tp / fp / fn and the AOS similarity per
//                     frame into the workspace; eval_reduce (one wave per (curve, threshold)) sums the frames in a fixed
//                     order.
// No atomics: every output is bitwise reproducible.
#include <math.h>

#include "bev_iou.h"

namespace {

constexpr int OV_THREADS = 64;
constexpr int CNT_WAVES = 4;            // eval_counts: waves (thresholds) per workgroup
constexpr int NT = MVX_KITTI_THRESHOLDS;

struct Curves {
    int metric[MVX_KITTI_MAX_CURVES];   // 0 = 2D bbox, 1 = BEV, 2 = 3D
    int set[MVX_KITTI_MAX_CURVES];      // row of the cleaning flags (class * 3 + difficulty)
    double min_ov[MVX_KITTI_MAX_CURVES];
};

// Sizes derived on the host from the offsets
struct Sizes {
    long long n_det, n_gt, n_dc, n_pairs, n_dc_pairs, n_slots;
};

// row f64 [8] = x1 y1 x2 y2 l w h y (camera frame, y pointing down: the box spans [y - h, y])
constexpr int ROW = 8;

// axis-aligned overlap of det a with box b: intersection / union (dc = false) or / area of a (dc = true); 0 without overlap
__device__ __forceinline__ double image_overlap(const double *a, const double *b, bool dc) {
    const double iw = fmax(fmin(a[2], b[2]) - fmax(a[0], b[0]), 0.0);
    const double ih = fmax(fmin(a[3], b[3]) - fmax(a[1], b[1]), 0.0);
    const double inter = iw * ih;
    if (inter <= 0.0) return 0.0;
    const double area_a = (a[2] - a[0]) * (a[3] - a[1]);
    if (dc) return inter / area_a;
    const double area_b = (b[2] - b[0]) * (b[3] - b[1]);
    return inter / (area_a + area_b - inter);
}

// largest f with off[f] <= p (off ascending, off[0] = 0 <= p < off[F])
__device__ __forceinline__ int frame_of(const long long *off, int F, long long p) {
    int lo = 0, hi = F;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// 1. overlaps[m][pair_off[f] + g * nd + d] (m = 2D, BEV, 3D) and dc_overlaps[dc_pair_off[f] + k * nd + d]
__global__ __launch_bounds__(OV_THREADS) void eval_overlaps(int F, const int *__restrict__ off, const long long *__restrict__ pair_off,
                                                          Sizes sz, const double *__restrict__ det_rows,
                                                          const float *__restrict__ det_quads, const double *__restrict__ gt_rows,
                                                          const float *__restrict__ gt_quads, const double *__restrict__ dc_rows,
                                                          double *__restrict__ overlaps, double *__restrict__ dc_overlaps) {
    __shared__ P2 s_poly[POLY_SLOTS * OV_THREADS];
    const long long p = (long long)blockIdx.x * OV_THREADS + threadIdx.x;
    if (p >= sz.n_pairs + sz.n_dc_pairs) return;
    const int *det_off = off, *gt_off = off + (F + 1), *dc_off = off + 2 * (F + 1);
    if (p >= sz.n_pairs) {                      // detection vs don't-care
        const long long q = p - sz.n_pairs;
        const long long *dco = pair_off + (F + 1);
        const int f = frame_of(dco, F, q);
        const int nd = det_off[f + 1] - det_off[f];
        const long long loc = q - dco[f];
        const int k = (int)(loc / nd), d = (int)(loc - (long long)k * nd);
        if (k >= dc_off[f + 1] - dc_off[f]) return;
        dc_overlaps[q] = image_overlap(det_rows + (size_t)(det_off[f] + d) * ROW, dc_rows + (size_t)(dc_off[f] + k) * 4, true);
        return;
    }
    const int f = frame_of(pair_off, F, p);
    const int nd = det_off[f + 1] - det_off[f];
    const long long loc = p - pair_off[f];
    const int g = (int)(loc / nd), d = (int)(loc - (long long)g * nd);
    if (g >= gt_off[f + 1] - gt_off[f]) return;
    const int di = det_off[f] + d, gi = gt_off[f] + g;
    const double *a = det_rows + (size_t)di * ROW, *b = gt_rows + (size_t)gi * ROW;
    const float *qa = det_quads + (size_t)di * 8, *qb = gt_quads + (size_t)gi * 8;
    overlaps[p] = image_overlap(a, b, false);

    // BEV intersection: f32 with bboxIntersection's arithmetic, 0 where the bounding circles cannot touch
    P2 c1, c2;
    float r1, r2;
    quad_circle((const P2 *)qa, c1, r1);
    quad_circle((const P2 *)qb, c2, r2);
    float inter = 0.f;
    if (!circles_apart(c1, r1, c2, r2)) {
        const Polys w = polys_of(s_poly, OV_THREADS, threadIdx.x);
        load_oriented(w.q1, qa);                // the areas are not used: the denominators below are the f64 l * w
        load_oriented(w.q2, qb);
        inter = quad_intersection(w.q1, w.q2, w.p, w.q);
    }
    const double I = (double)inter;
    const double la = a[4], wa = a[5], ha = a[6], lb = b[4], wb = b[5], hb = b[6];
    overlaps[sz.n_pairs + p] = I / (la * wa + lb * wb - I);
    const double ih = fmin(a[7], b[7]) - fmax(a[7] - ha, b[7] - hb);
    double iou3 = 0.0;
    if (ih > 0.0) {
        const double inc = I * ih;
        iou3 = inc / (la * ha * wa + lb * hb * wb - inc);
    }
    overlaps[2 * sz.n_pairs + p] = iou3;
}

// (key desc, index asc) arg-best over the wave; index < 0 = no candidate.  Every lane returns the same pair.
__device__ __forceinline__ void wave_argbest(double &key, int &idx) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const double ok = __shfl_xor(key, m, 64);
        const int oi = __shfl_xor(idx, m, 64);
        if (oi >= 0 && (idx < 0 || ok > key || (ok == key && oi < idx))) { key = ok; idx = oi; }
    }
}

__device__ __forceinline__ int wave_min_idx(int idx) {      // smallest non-negative index, -1 if none
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const int oi = __shfl_xor(idx, m, 64);
        if (oi >= 0 && (idx < 0 || oi < idx)) idx = oi;
    }
    return idx;
}

// Per-(frame, curve) view of the inputs
struct FrameView {
    int nd, ng, nc, metric;
    double mo;
    const signed char *ig, *idt;
    const double *sc, *ov;
    __device__ FrameView(int F, int f, int c, const int *off, const long long *pair_off, const Sizes &sz, const Curves &cv,
                         const signed char *ign_gt, const signed char *ign_det, const double *scores, const double *overlaps) {
        const int d0 = off[f], g0 = off[F + 1 + f];
        nd = off[f + 1] - d0;
        ng = off[F + 2 + f] - g0;
        nc = off[2 * (F + 1) + f + 1] - off[2 * (F + 1) + f];
        metric = cv.metric[c];
        mo = cv.min_ov[c];
        ig = ign_gt + (size_t)cv.set[c] * sz.n_gt + g0;
        idt = ign_det + (size_t)cv.set[c] * sz.n_det + d0;
        sc = scores + d0;
        ov = overlaps + (size_t)metric * sz.n_pairs + pair_off[f];
    }
};

// 2. threshold pass: TP scores into tp_scores[c][slot_off[f] .. + min(nd, ng)) (the rest -inf), n_valid_gt[c][f]
__global__ __launch_bounds__(64) void eval_tp_scores(int F, const int *__restrict__ off, const long long *__restrict__ pair_off, Sizes sz,
                                                     Curves cv, const signed char *__restrict__ ign_gt,
                                                     const signed char *__restrict__ ign_det, const double *__restrict__ scores,
                                                     const double *__restrict__ overlaps, double *__restrict__ tp_scores,
                                                     int *__restrict__ n_valid_gt) {
    const int f = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
    const FrameView v(F, f, c, off, pair_off, sz, cv, ign_gt, ign_det, scores, overlaps);
    double *slots = tp_scores + (size_t)c * sz.n_slots + pair_off[2 * (F + 1) + f];
    const int cap = min(v.nd, v.ng);
    unsigned long long assigned = 0ull;        // bit k: detection lane + 64 k
    int tp = 0, n_valid = 0;
    for (int g = 0; g < v.ng; ++g) {
        const int igg = v.ig[g];
        if (igg == -1) continue;
        n_valid += igg == 0;
        double best = -1e7;
        int bi = -1;
        for (int k = 0; lane + 64 * k < v.nd; ++k) {
            const int j = lane + 64 * k;
            if (v.idt[j] == -1 || ((assigned >> k) & 1ull)) continue;
            const double o = v.ov[(size_t)g * v.nd + j], s = v.sc[j];
            if (o > v.mo && s > best) { best = s; bi = j; }
        }
        wave_argbest(best, bi);
        if (bi < 0) continue;                   // an fn when igg == 0 (not counted in this pass)
        if (lane == (bi & 63)) assigned |= 1ull << (bi >> 6);
        if (igg == 1 || v.idt[bi] == 1) continue;
        if (lane == 0 && tp < cap) slots[tp] = v.sc[bi];
        ++tp;
    }
    for (int k = tp + lane; k < cap; k += 64) slots[k] = -INFINITY;
    if (lane == 0) n_valid_gt[(size_t)c * F + f] = n_valid;
}

// 3. one wave per curve over its descending TP scores (-inf padded): n_gt, the picked thresholds (0-padded to 41)
__global__ __launch_bounds__(64) void eval_thresholds(int F, long long n_slots, const double *__restrict__ sorted,
                                                      const int *__restrict__ n_valid_gt, double *__restrict__ thresholds,
                                                      int *__restrict__ n_thresholds, int *__restrict__ n_gt_out) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const double *s = sorted + (size_t)c * n_slots;
    int ng = 0, ntp = 0;
    for (int f = lane; f < F; f += 64) ng += n_valid_gt[(size_t)c * F + f];
    for (long long i = lane; i < n_slots; i += 64) ntp += s[i] > -INFINITY;
    ng = wave_sum_i32(ng);
    ntp = wave_sum_i32(ntp);
    const double step = 1.0 / (NT - 1.0);
    double cur = 0.0;
    int np = 0;
    long long start = 0;
    while (start < ntp && np < NT) {
        const long long i = start + lane;
        bool pick = false;
        if (i < ntp) {
            const bool last = i == ntp - 1;
            const double l = (double)(i + 1) / (double)ng;
            const double r = last ? l : (double)(i + 2) / (double)ng;
            pick = !((r - cur) < (cur - l) && !last);
        }
        const unsigned long long b = __ballot(pick);
        if (b == 0ull) { start += 64; continue; }
        const long long ip = start + __builtin_ctzll(b);
        if (lane == 0) thresholds[(size_t)c * NT + np] = s[ip];
        ++np;
        cur += step;
        start = ip + 1;
    }
    for (int k = np + lane; k < NT; k += 64) thresholds[(size_t)c * NT + k] = 0.0;
    if (lane == 0) { n_thresholds[c] = np; n_gt_out[c] = ng; }
}

// Workspace: per-frame statistics [n_curves][NT][F] as i32 tp | i32 fp | i32 fn | f64 similarity
struct StatLayout {
    size_t n, tp, fp, fn, sim, total;
    __host__ __device__ StatLayout(int F, int C) {
        n = (size_t)C * NT * F;
        tp = 0;
        fp = tp + ((n * 4 + 255) & ~(size_t)255);
        fn = fp + ((n * 4 + 255) & ~(size_t)255);
        sim = fn + ((n * 4 + 255) & ~(size_t)255);
        total = sim + n * 8 + 256;
    }
};

// 4. compute_fp = true for (frame f, curve c, threshold t = blockIdx.z * CNT_WAVES + wave)
__global__ __launch_bounds__(64 * CNT_WAVES) void eval_counts(int F, const int *__restrict__ off, const long long *__restrict__ pair_off,
                                                              Sizes sz, Curves cv, const signed char *__restrict__ ign_gt,
                                                              const signed char *__restrict__ ign_det, const double *__restrict__ scores,
                                                              const double *__restrict__ det_alpha, const double *__restrict__ gt_alpha,
                                                              const double *__restrict__ overlaps, const double *__restrict__ dc_overlaps,
                                                              const double *__restrict__ thresholds, const int *__restrict__ n_thresholds,
                                                              StatLayout lay, unsigned char *__restrict__ ws) {
    const int f = blockIdx.x, c = blockIdx.y, lane = threadIdx.x & 63;
    const int t = blockIdx.z * CNT_WAVES + (threadIdx.x >> 6);
    if (t >= NT) return;
    const size_t o = ((size_t)c * NT + t) * F + f;
    int *s_tp = (int *)(ws + lay.tp), *s_fp = (int *)(ws + lay.fp), *s_fn = (int *)(ws + lay.fn);
    double *s_sim = (double *)(ws + lay.sim);
    if (t >= n_thresholds[c]) {
        if (lane == 0) { s_tp[o] = 0; s_fp[o] = 0; s_fn[o] = 0; s_sim[o] = 0.0; }
        return;
    }
    const FrameView v(F, f, c, off, pair_off, sz, cv, ign_gt, ign_det, scores, overlaps);
    const double thr = thresholds[(size_t)c * NT + t];
    const int d0 = off[f], g0 = off[F + 1 + f];
    unsigned long long assigned = 0ull;
    int tp = 0, fn = 0;
    double sim = 0.0;
    for (int g = 0; g < v.ng; ++g) {
        const int igg = v.ig[g];
        if (igg == -1) continue;
        // the sequential rules reduce to: the largest overlap among eligible detections with ignored_det == 0 (first
        // of equals), else the first eligible one with ignored_det == 1
        double b0 = 0.0;
        int i0 = -1, i1 = -1;
        for (int k = 0; lane + 64 * k < v.nd; ++k) {
            const int j = lane + 64 * k;
            const int id = v.idt[j];
            if (id == -1 || ((assigned >> k) & 1ull) || v.sc[j] < thr) continue;
            const double ov = v.ov[(size_t)g * v.nd + j];
            if (!(ov > v.mo)) continue;
            if (id == 0) {
                if (i0 < 0 || ov > b0) { b0 = ov; i0 = j; }
            } else if (i1 < 0) {
                i1 = j;
            }
        }
        wave_argbest(b0, i0);
        const int det = i0 >= 0 ? i0 : wave_min_idx(i1);
        if (det < 0) {
            fn += igg == 0;
            continue;
        }
        if (lane == (det & 63)) assigned |= 1ull << (det >> 6);
        if (igg == 1 || v.idt[det] == 1) continue;
        ++tp;
        if (v.metric == 0) sim += (1.0 + cos(gt_alpha[g0 + g] - det_alpha[d0 + det])) / 2.0;
    }
    // false positives: unassigned, not ignored, not below the threshold; on 2D those inside a don't-care box are dropped
    const double *dco = dc_overlaps + pair_off[(F + 1) + f];
    int nfp = 0, nstuff = 0;
    for (int k = 0; lane + 64 * k < v.nd; ++k) {
        const int j = lane + 64 * k;
        if (((assigned >> k) & 1ull) || v.idt[j] != 0 || v.sc[j] < thr) continue;
        ++nfp;
        if (v.metric == 0) {
            bool hit = false;
            for (int q = 0; q < v.nc && !hit; ++q) hit = dco[(size_t)q * v.nd + j] > v.mo;
            nstuff += hit;
        }
    }
    const int fp = wave_sum_i32(nfp) - wave_sum_i32(nstuff);
    if (v.metric == 0) {
        if (tp + fp == 0) sim = -1.0;
    } else {
        sim = 0.0;
    }
    if (lane == 0) { s_tp[o] = tp; s_fp[o] = fp; s_fn[o] = fn; s_sim[o] = sim; }
}

// 4b. one wave per (curve, threshold): frame sums in a fixed order -> totals [c][t][3] (tp, fp, fn), similarity [c][t]
__global__ __launch_bounds__(64) void eval_reduce(int F, StatLayout lay, const unsigned char *__restrict__ ws, int *__restrict__ totals,
                                                  double *__restrict__ similarity) {
    const int ct = blockIdx.x, lane = threadIdx.x;
    const int *s_tp = (const int *)(ws + lay.tp), *s_fp = (const int *)(ws + lay.fp), *s_fn = (const int *)(ws + lay.fn);
    const double *s_sim = (const double *)(ws + lay.sim);
    int tp = 0, fp = 0, fn = 0;
    double sim = 0.0;
    for (int f = lane; f < F; f += 64) {
        const size_t o = (size_t)ct * F + f;
        tp += s_tp[o];
        fp += s_fp[o];
        fn += s_fn[o];
        sim += s_sim[o];
    }
    sim = wave_sum_f64(sim);
    tp = wave_sum_i32(tp);
    fp = wave_sum_i32(fp);
    fn = wave_sum_i32(fn);
    if (lane == 0) {
        totals[(size_t)ct * 3] = tp;
        totals[(size_t)ct * 3 + 1] = fp;
        totals[(size_t)ct * 3 + 2] = fn;
        similarity[ct] = sim;
    }
}

// ---- host-side checks ------------------------------------------------------------------------------------------------------
// Offsets (det, gt, dc) start at 0, never decrease, and respect the per-frame limits; fills the sizes.
int check_frames(int F, const int32_t *off_host, Sizes &sz) {
    if (F < 1 || !off_host) return MVX_EINVAL;
    const int32_t *det = off_host, *gt = off_host + (F + 1), *dc = off_host + 2 * (F + 1);
    if (det[0] != 0 || gt[0] != 0 || dc[0] != 0) return MVX_EINVAL;
    long long pairs = 0, dc_pairs = 0, slots = 0;
    for (int f = 0; f < F; ++f) {
        const long long nd = (long long)det[f + 1] - det[f], ng = (long long)gt[f + 1] - gt[f], nc = (long long)dc[f + 1] - dc[f];
        if (nd < 0 || ng < 0 || nc < 0 || nd > MVX_DETECT_MAX_PRE || ng + nc > MVX_KITTI_MAX_GT) return MVX_EINVAL;
        pairs += nd * ng;
        dc_pairs += nd * nc;
        slots += nd < ng ? nd : ng;
    }
    if ((pairs + dc_pairs) / OV_THREADS >= (1ll << 31)) return MVX_EINVAL;
    sz = Sizes{det[F], gt[F], dc[F], pairs, dc_pairs, slots};
    return MVX_OK;
}

int check_curves(int n_curves, const int32_t *curve_host, const double *min_overlap_host, int n_sets, Curves &cv) {
    if (n_curves < 1 || n_curves > MVX_KITTI_MAX_CURVES || n_sets < 1 || !curve_host || !min_overlap_host) return MVX_EINVAL;
    for (int c = 0; c < n_curves; ++c) {
        const int m = curve_host[2 * c], s = curve_host[2 * c + 1];
        const double mo = min_overlap_host[c];
        if (m < 0 || m > 2 || s < 0 || s >= n_sets || !(mo >= 0.0 && mo < 1.0)) return MVX_EINVAL;
        cv.metric[c] = m;
        cv.set[c] = s;
        cv.min_ov[c] = mo;
    }
    return MVX_OK;
}

}  // namespace

extern "C" size_t mvx_kitti_eval_workspace_bytes(int32_t n_frames, int32_t n_curves) {
    return StatLayout(n_frames > 0 ? n_frames : 0, n_curves > 0 ? n_curves : 0).total;
}

extern "C" int mvx_kitti_eval_overlaps(int32_t n_frames, const int32_t *off_host, const int32_t *off, const int64_t *pair_off,
                                       const double *det_rows, const float *det_quads, const double *gt_rows, const float *gt_quads,
                                       const double *dc_rows, double *overlaps, double *dc_overlaps, void *stream) {
    Sizes sz;
    const int st = check_frames(n_frames, off_host, sz);
    if (st != MVX_OK) return st;
    MVX_CHECK_ARG(off && pair_off);
    MVX_CHECK_ARG(sz.n_pairs == 0 || (det_rows && det_quads && gt_rows && gt_quads && overlaps));
    MVX_CHECK_ARG(sz.n_dc_pairs == 0 || (det_rows && dc_rows && dc_overlaps));
    const long long tot = sz.n_pairs + sz.n_dc_pairs;
    if (tot == 0) return MVX_OK;
    hipLaunchKernelGGL(eval_overlaps, dim3(mvx_cdiv(tot, OV_THREADS)), dim3(OV_THREADS), 0, (hipStream_t)stream, (int)n_frames, off,
                       (const long long *)pair_off, sz, det_rows, det_quads, gt_rows, gt_quads, dc_rows, overlaps, dc_overlaps);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_kitti_eval_tp_scores(int32_t n_frames, const int32_t *off_host, const int32_t *off, const int64_t *pair_off,
                                        int32_t n_curves, const int32_t *curve_host, const double *min_overlap_host, int32_t n_sets,
                                        const int8_t *ignored_gt, const int8_t *ignored_det, const double *scores,
                                        const double *overlaps, double *tp_scores, int32_t *n_valid_gt, void *stream) {
    Sizes sz;
    Curves cv;
    int st = check_frames(n_frames, off_host, sz);
    if (st == MVX_OK) st = check_curves(n_curves, curve_host, min_overlap_host, n_sets, cv);
    if (st != MVX_OK) return st;
    MVX_CHECK_ARG(off && pair_off && n_valid_gt);
    MVX_CHECK_ARG(sz.n_gt == 0 || ignored_gt);
    MVX_CHECK_ARG(sz.n_det == 0 || (ignored_det && scores));
    MVX_CHECK_ARG(sz.n_pairs == 0 || overlaps);
    MVX_CHECK_ARG(sz.n_slots == 0 || tp_scores);
    hipLaunchKernelGGL(eval_tp_scores, dim3(n_frames, n_curves), dim3(64), 0, (hipStream_t)stream, (int)n_frames, off,
                       (const long long *)pair_off, sz, cv, (const signed char *)ignored_gt, (const signed char *)ignored_det, scores,
                       overlaps, tp_scores, n_valid_gt);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_kitti_eval_thresholds(int32_t n_frames, int32_t n_curves, int64_t n_slots, const double *sorted_scores,
                                         const int32_t *n_valid_gt, double *thresholds, int32_t *n_thresholds, int32_t *n_gt,
                                         void *stream) {
    MVX_CHECK_ARG(n_frames >= 1 && n_curves >= 1 && n_curves <= MVX_KITTI_MAX_CURVES && n_slots >= 0);
    MVX_CHECK_ARG((n_slots == 0 || sorted_scores) && n_valid_gt && thresholds && n_thresholds && n_gt);
    hipLaunchKernelGGL(eval_thresholds, dim3(n_curves), dim3(64), 0, (hipStream_t)stream, (int)n_frames, (long long)n_slots,
                       sorted_scores, n_valid_gt, thresholds, n_thresholds, n_gt);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_kitti_eval_counts(int32_t n_frames, const int32_t *off_host, const int32_t *off, const int64_t *pair_off,
                                     int32_t n_curves, const int32_t *curve_host, const double *min_overlap_host, int32_t n_sets,
                                     const int8_t *ignored_gt, const int8_t *ignored_det, const double *scores,
                                     const double *det_alpha, const double *gt_alpha, const double *overlaps,
                                     const double *dc_overlaps, const double *thresholds, const int32_t *n_thresholds,
                                     int32_t *totals, double *similarity, void *workspace, size_t workspace_bytes, void *stream) {
    Sizes sz;
    Curves cv;
    int st = check_frames(n_frames, off_host, sz);
    if (st == MVX_OK) st = check_curves(n_curves, curve_host, min_overlap_host, n_sets, cv);
    if (st != MVX_OK) return st;
    MVX_CHECK_ARG(off && pair_off && thresholds && n_thresholds && totals && similarity && workspace);
    MVX_CHECK_ARG(sz.n_gt == 0 || (ignored_gt && gt_alpha));
    MVX_CHECK_ARG(sz.n_det == 0 || (ignored_det && scores && det_alpha));
    MVX_CHECK_ARG(sz.n_pairs == 0 || overlaps);
    MVX_CHECK_ARG(sz.n_dc_pairs == 0 || dc_overlaps);
    const StatLayout lay(n_frames, n_curves);
    MVX_CHECK_ARG(workspace_bytes >= lay.total && ((uintptr_t)workspace & 255) == 0);
    hipStream_t s = (hipStream_t)stream;
    unsigned char *ws = (unsigned char *)workspace;
    hipLaunchKernelGGL(eval_counts, dim3(n_frames, n_curves, (NT + CNT_WAVES - 1) / CNT_WAVES), dim3(64 * CNT_WAVES), 0, s,
                       (int)n_frames, off, (const long long *)pair_off, sz, cv, (const signed char *)ignored_gt,
                       (const signed char *)ignored_det, scores, det_alpha, gt_alpha, overlaps, dc_overlaps, thresholds,
                       n_thresholds, lay, ws);
    MVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(eval_reduce, dim3(n_curves * NT), dim3(64), 0, s, (int)n_frames, lay, (const unsigned char *)ws, totals,
                       similarity);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}
