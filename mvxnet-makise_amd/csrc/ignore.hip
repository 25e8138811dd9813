// Ignore regions for anchor targets: anchors over DontCare rectangles, over look-alike boxes and over labelled
// boxes that hold almost no points leave the classification loss.  Both losses read neg_idx as "the NOT-negative anchors" and
// give an anchor listed there and not in pos_idx no classification loss, so one pass behind mvx_assign_anchors_frames rewrites
// the lists and no loss kernel changes.
//
// The rule, per frame (restated in numpy in tests/ignore_ref.py):
//     sparse     a box g with gt_points[g] < min_points (gt_points given)
//     demotion   a pos_idx entry whose gi names a sparse box leaves the positive list and stays not negative; no rematch
//     rectangle  an anchor that is not yet not negative becomes so when its centre (x, y, z + h/2, 1), multiplied by the frame's
//                3 x 4 matrix M in f64 as  ((M[r][0] x + M[r][1] y) + M[r][2] zc) + M[r][3]  (no fused multiply-add), has depth
//                (row 2) > 0 and the pixel (row 0 / depth, row 1 / depth) lies in a rectangle of the frame, edges inclusive
//     box        an anchor that is still not not negative becomes so when  inter(b, a) >= ioa_thr * area(a)  in f32 for an ignore
//                quad b: inter = mvx_bbox_pairwise(b, a, 0), or 0 where the bounding circles are apart; area(a) = |shoelace| (f32)
//
// mvx_ignore_anchors_frames -- four launches and one memset for any number of frames:
//     memset  map u32 [F][N] and the four counters of every frame behind it
//     1  ignore_lists   scatters the incoming lists into the map: bit 0 = not negative, bit 1 = positive (kept), gi + 1 from bit 8
//     2  ignore_dense   a thread per anchor: the two tests (rectangles, matrix and ignore quads of the frame in LDS, the circle
//                       test in front of the clipping), bits 2 / 3 = newly ignored by a rectangle / by a box only, block counts
//     3  scan of the block counts (mvxi_scan_block_counts, 2F rows)
//     4  ignore_write   order-preserving compaction of the map into the lists (compact.h), counts clipped to cap_out
// Only integer atomics (OR into the map, adds of counters): the result does not depend on the order of arrival.
//
// mvx_box_point_counts_frames -- one launch and one memset: a workgroup takes 1024 rows of one frame's cloud, holds the frame's
// boxes in LDS 64 at a time (box3d.h, f64), counts per box in LDS integers and adds the sums to counts with integer atomics.
#include "anchor_lists.h"
#include "bev_iou.h"
#include "box3d.h"

namespace {

constexpr int CHUNK_B = 64;             // boxes of a frame held in LDS at a time (point counts)
constexpr int ROWS_PER_BLOCK = 1024;    // rows of a frame's cloud per workgroup
constexpr int CHUNK_R = 64;             // rectangles in LDS at a time
constexpr int CHUNK_Q = 32;             // ignore quads in LDS at a time
constexpr int GI_SHIFT = 8;
constexpr long long GI_MAX = (1ll << (32 - GI_SHIFT)) - 2;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void box_point_counts(const float *__restrict__ points, int cap_points, int ld,
                                                        const int *__restrict__ n_points, const float *__restrict__ boxes,
                                                        const int *__restrict__ gt_off, int G, int *__restrict__ counts) {
    __shared__ Box s_box[CHUNK_B];
    __shared__ int s_cnt[CHUNK_B];
    const int f = blockIdx.y, tid = threadIdx.x;
    const int n = clampi(n_points[f], 0, cap_points);
    const int r0 = blockIdx.x * ROWS_PER_BLOCK;
    if (r0 >= n) return;                                            // block-uniform: rows at or beyond n_points are never read
    const int g_lo = clampi(gt_off[f], 0, G), g_hi = clampi(gt_off[f + 1], g_lo, G);
    const float *pf = points + (size_t)f * cap_points * ld;
    double px[ROWS_PER_BLOCK / 256], py[ROWS_PER_BLOCK / 256], pz[ROWS_PER_BLOCK / 256];
    bool live[ROWS_PER_BLOCK / 256];
#pragma unroll
    for (int k = 0; k < ROWS_PER_BLOCK / 256; ++k) {
        const int r = r0 + k * 256 + tid;
        live[k] = r < n;
        const float *p = pf + (size_t)(live[k] ? r : r0) * ld;
        px[k] = (double)p[0]; py[k] = (double)p[1]; pz[k] = (double)p[2];
    }
    for (int g0 = g_lo; g0 < g_hi; g0 += CHUNK_B) {
        const int nb = min(CHUNK_B, g_hi - g0);
        if (tid < nb) {
            const float *b3 = boxes + (size_t)(g0 + tid) * 7;
            s_box[tid] = load_box(b3, cos((double)b3[6]), sin((double)b3[6]));
            s_cnt[tid] = 0;
        }
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
            const Box bx = s_box[b];
            int mine = 0;
#pragma unroll
            for (int k = 0; k < ROWS_PER_BLOCK / 256; ++k) mine += __popcll(__ballot(live[k] && inside(bx, px[k], py[k], pz[k])));
            if ((tid & 63) == 0 && mine) atomicAdd(&s_cnt[b], mine);
        }
        __syncthreads();
        if (tid < nb && s_cnt[tid]) atomicAdd(counts + g0 + tid, s_cnt[tid]);
        __syncthreads();
    }
}

// ---- the list rewrite ------------------------------------------------------------------------------------------------------
struct IgnoreArgs {
    const long long *pos_idx, *neg_idx, *gi;     // [F][3][cap], [F][3][cap], [F][cap]
    const int *counts;                           // [F][2]
    long long cap;
    const int *gt_off, *gt_points;               // [F+1], [G_total] or null
    int min_points;
    const float *anchors, *quads;                // [N][7], [N][4][2]
    int L, W, A;
    long long N;
    const float *rects;                          // [R_total][4] or null
    const int *rect_off;                         // [F+1]
    const double *mats;                          // [F][3][4]
    const float *ign;                            // [B_total][4][2] or null
    const int *ign_off;                          // [F+1]
    float ioa_thr;
    unsigned *map;                               // [F][N], then int wstats [F][4]
    int *wstats;
    int *bcount;
    int nblocks;
};

__device__ __forceinline__ long long flat_of(const long long *t, long long cap, long long e, int L, int W, int A) {
    const long long x = t[e], y = t[cap + e], z = t[2 * cap + e];
    if (x < 0 || x >= L || y < 0 || y >= W || z < 0 || z >= A) return -1;
    return (x * W + y) * A + z;
}

__global__ __launch_bounds__(256) void ignore_lists(IgnoreArgs a) {
    const int f = blockIdx.y, tid = threadIdx.x;
    const long long e = (long long)blockIdx.x * 256 + tid;
    const long long cap = a.cap;
    const long long n_pos = min(max((long long)a.counts[2 * f], 0ll), cap), n_neg = min(max((long long)a.counts[2 * f + 1], 0ll), cap);
    unsigned *map = a.map + (size_t)f * a.N;
    int g_lo = 0, g_hi = 0;
    if (a.gt_points) { g_lo = max(a.gt_off[f], 0); g_hi = max(a.gt_off[f + 1], g_lo); }
    bool demoted = false;
    if (e < n_pos) {
        const long long at = flat_of(a.pos_idx + (size_t)f * 3 * cap, cap, e, a.L, a.W, a.A);
        const long long g = a.gi[(size_t)f * cap + e];
        if (at >= 0 && g >= 0 && g <= GI_MAX) {
            const bool sparse = a.gt_points && g < g_hi - g_lo && a.gt_points[g_lo + g] < a.min_points;
            demoted = sparse;
            atomicOr(map + at, sparse ? 1u : (3u | ((unsigned)(g + 1) << GI_SHIFT)));
        }
    }
    if (e < n_neg) {
        const long long at = flat_of(a.neg_idx + (size_t)f * 3 * cap, cap, e, a.L, a.W, a.A);
        if (at >= 0) atomicOr(map + at, 1u);
    }
    const int nd = __popcll(__ballot(demoted));
    if ((tid & 63) == 0 && nd) atomicAdd(a.wstats + 4 * f, nd);
    if (blockIdx.x == 0 && a.gt_points) {                           // the sparse boxes of the frame
        int mine = 0;
        for (int g = g_lo + tid; g < g_hi; g += 256) mine += a.gt_points[g] < a.min_points ? 1 : 0;
        mine = wave_sum_i32(mine);
        if ((tid & 63) == 0 && mine) atomicAdd(a.wstats + 4 * f + 3, mine);
    }
}

__global__ __launch_bounds__(256) void ignore_dense(IgnoreArgs a) {
    __shared__ P2 s_poly[POLY_SLOTS * 256];
    __shared__ float s_rect[CHUNK_R][4];
    __shared__ float s_quad[CHUNK_Q][8], s_circ[CHUNK_Q][3];
    __shared__ double s_m[12];
    __shared__ int s[2][4];
    const int f = blockIdx.y, tid = threadIdx.x;
    const long long at = (long long)blockIdx.x * 256 + tid;
    const bool in = at < a.N;
    unsigned *slot = a.map + (size_t)f * a.N + (in ? at : 0);
    unsigned m = in ? *slot : 1u;                                   // a thread past the end takes no test
    const unsigned m_in = m;
    // ---- rectangles
    int r_lo = 0, r_hi = 0;
    if (a.rects) { r_lo = max(a.rect_off[f], 0); r_hi = max(a.rect_off[f + 1], r_lo); }
    if (r_hi > r_lo) {                                              // block-uniform
        if (tid < 12) s_m[tid] = a.mats[(size_t)f * 12 + tid];
        __syncthreads();
        bool front = false;
        double px = 0.0, py = 0.0;
        if (!(m & 1u)) {
            const float *an = a.anchors + (size_t)at * 7;
            const double x = (double)an[0], y = (double)an[1], zc = (double)an[2] + (double)an[5] / 2.0;
            const double u = ((s_m[0] * x + s_m[1] * y) + s_m[2] * zc) + s_m[3];
            const double v = ((s_m[4] * x + s_m[5] * y) + s_m[6] * zc) + s_m[7];
            const double d = ((s_m[8] * x + s_m[9] * y) + s_m[10] * zc) + s_m[11];
            front = d > 0.0;
            if (front) { px = u / d; py = v / d; }
        }
        for (int c0 = r_lo; c0 < r_hi; c0 += CHUNK_R) {
            const int nr = min(CHUNK_R, r_hi - c0);
            __syncthreads();
            if (tid < nr * 4) s_rect[tid >> 2][tid & 3] = a.rects[(size_t)c0 * 4 + tid];
            __syncthreads();
            if (front && !(m & 1u)) {
                for (int r = 0; r < nr; ++r)
                    if (px >= (double)s_rect[r][0] && px <= (double)s_rect[r][2] && py >= (double)s_rect[r][1] && py <= (double)s_rect[r][3]) {
                        m |= 5u;
                        break;
                    }
            }
        }
    }
    // ---- ignore boxes
    int q_lo = 0, q_hi = 0;
    if (a.ign) { q_lo = max(a.ign_off[f], 0); q_hi = max(a.ign_off[f + 1], q_lo); }
    if (q_hi > q_lo) {                                              // block-uniform
        const Polys wk = polys_of(s_poly, 256, tid);
        P2 ac = {0.f, 0.f};
        float ar = 0.f, a_area = 0.f;
        const bool test = !(m & 1u);
        if (test) {
            a_area = load_oriented(wk.q2, a.quads + (size_t)at * 8);
            quad_circle((const P2 *)(a.quads + (size_t)at * 8), ac, ar);
        }
        for (int c0 = q_lo; c0 < q_hi; c0 += CHUNK_Q) {
            const int nq = min(CHUNK_Q, q_hi - c0);
            __syncthreads();
            if (tid < nq * 8) s_quad[tid >> 3][tid & 7] = a.ign[(size_t)c0 * 8 + tid];
            __syncthreads();
            if (tid < nq) circle_of(s_quad[tid], s_circ[tid]);
            __syncthreads();
            if (test && !(m & 1u)) {
                for (int b = 0; b < nq; ++b) {
                    const P2 bc = {s_circ[b][0], s_circ[b][1]};
                    if (circles_apart(bc, s_circ[b][2], ac, ar)) continue;
                    load_oriented(wk.q1, s_quad[b]);
                    const float inter = quad_intersection(wk.q1, wk.q2, wk.p, wk.q);
                    if (inter >= a.ioa_thr * a_area) {
                        m |= 9u;
                        break;
                    }
                }
            }
        }
    }
    if (in && m != m_in) *slot = m;
    __syncthreads();
    list_block_counts(in ? (int)(m & 3u) : 0, f, a.nblocks, s, a.bcount);
    const int by_rect = __popcll(__ballot(in && (m & 4u))), by_box = __popcll(__ballot(in && (m & 8u)));
    if ((tid & 63) == 0) {
        if (by_rect) atomicAdd(a.wstats + 4 * f + 1, by_rect);
        if (by_box) atomicAdd(a.wstats + 4 * f + 2, by_box);
    }
}

__global__ __launch_bounds__(256) void ignore_write(const unsigned *__restrict__ map, const int *__restrict__ wstats, long long N, int W,
                                                    int A, int nblocks, const int *__restrict__ boff, const int *__restrict__ totals,
                                                    long long *__restrict__ pos_out, long long *__restrict__ neg_out,
                                                    long long *__restrict__ gi_out, long long cap, int *__restrict__ counts,
                                                    int *__restrict__ stats, int *__restrict__ status) {
    __shared__ int s[2][4];
    const int f = blockIdx.y;
    const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned m = at < N ? map[(size_t)f * N + at] : 0u;
    list_write((int)(m & 3u), (long long)(m >> GI_SHIFT) - 1, f, at, W, A, nblocks, s, boff, totals, pos_out, neg_out, gi_out, cap,
               counts, status);
    if (blockIdx.x == 0 && threadIdx.x < 4) stats[4 * f + threadIdx.x] = wstats[4 * f + threadIdx.x];
}

}  // namespace

extern "C" int mvx_box_point_counts_frames(const float *points6, int32_t n_frames, int32_t cap_points, int32_t ld,
                                           const int32_t *n_points, const float *boxes, const int32_t *gt_off, int32_t n_boxes_total,
                                           int32_t *counts, void *stream) {
    MVX_CHECK_ARG(n_frames >= 1 && n_frames <= MVX_MAX_FRAMES && cap_points >= 1 && ld >= 3 && n_boxes_total >= 0);
    if (n_boxes_total == 0) return MVX_OK;
    MVX_CHECK_ARG(points6 && n_points && boxes && gt_off && counts);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)n_boxes_total, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(box_point_counts, dim3(mvx_cdiv(cap_points, ROWS_PER_BLOCK), n_frames), dim3(256), 0, st, points6, cap_points, ld,
                       n_points, boxes, gt_off, n_boxes_total, counts);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" size_t mvx_ignore_anchors_frames_workspace_bytes(int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc) {
    if (n_frames <= 0 || l <= 0 || w <= 0 || anchors_per_loc <= 0) return 256;
    const size_t N = (size_t)l * w * anchors_per_loc, nb = (N + 255) / 256;
    return up256((size_t)n_frames * N * 4 + (size_t)n_frames * 16) + up256(2 * (size_t)n_frames * nb * 4) + up256(2 * (size_t)n_frames * 4);
}

extern "C" int mvx_ignore_anchors_frames(const int64_t *pos_idx, const int64_t *neg_idx, const int64_t *gi, int64_t cap,
                                         const int32_t *counts, int32_t n_frames, const int32_t *gt_off, const int32_t *gt_points,
                                         int32_t min_points, const float *anchors, const float *anchor_quads, int32_t l, int32_t w,
                                         int32_t anchors_per_loc, const float *rects, const int32_t *rect_off,
                                         const double *img_from_lidar, const float *ign_quads, const int32_t *ign_off, float ioa_thr,
                                         int64_t *pos_out, int64_t *neg_out, int64_t *gi_out, int64_t cap_out, int32_t *counts_out,
                                         int32_t *stats, int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
    MVX_CHECK_ARG(n_frames >= 1 && n_frames <= MVX_MAX_FRAMES && anchors_per_loc >= 1 && anchors_per_loc <= 4 && l > 0 && w > 0);
    MVX_CHECK_ARG(cap >= 1 && cap_out >= 1 && ioa_thr > 0.f && ioa_thr <= 1.f && min_points >= 0);
    MVX_CHECK_ARG((long long)l * w * anchors_per_loc < (1ll << 31));
    MVX_CHECK_ARG(pos_idx && neg_idx && gi && counts && anchors && anchor_quads);
    MVX_CHECK_ARG(pos_out && neg_out && gi_out && counts_out && stats && status && workspace);
    MVX_CHECK_ARG(!gt_points || gt_off);
    MVX_CHECK_ARG(!rects || (rect_off && img_from_lidar));
    MVX_CHECK_ARG(!ign_quads || ign_off);
    MVX_CHECK_ARG(workspace_bytes >= mvx_ignore_anchors_frames_workspace_bytes(n_frames, l, w, anchors_per_loc));
    const long long N = (long long)l * w * anchors_per_loc;
    const int nb = (int)mvx_cdiv(N, 256);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const size_t map_bytes = (size_t)n_frames * N * 4 + (size_t)n_frames * 16;
    IgnoreArgs a;
    a.pos_idx = (const long long *)pos_idx; a.neg_idx = (const long long *)neg_idx; a.gi = (const long long *)gi;
    a.counts = counts; a.cap = cap;
    a.gt_off = gt_off; a.gt_points = gt_points; a.min_points = min_points;
    a.anchors = anchors; a.quads = anchor_quads; a.L = l; a.W = w; a.A = anchors_per_loc; a.N = N;
    a.rects = rects; a.rect_off = rect_off; a.mats = img_from_lidar;
    a.ign = ign_quads; a.ign_off = ign_off; a.ioa_thr = ioa_thr;
    a.map = (unsigned *)ws;
    a.wstats = (int *)(ws + (size_t)n_frames * N * 4);
    ws += up256(map_bytes);
    a.bcount = (int *)ws;
    ws += up256(2 * (size_t)n_frames * nb * 4);
    int *totals = (int *)ws;
    a.nblocks = nb;
    hipError_t e = hipMemsetAsync(a.map, 0, map_bytes, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(ignore_lists, dim3(mvx_cdiv(cap, 256), n_frames), dim3(256), 0, st, a);
    MVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(ignore_dense, dim3(nb, n_frames), dim3(256), 0, st, a);
    MVX_LAUNCH_CHECK();
    const int rc = mvxi_scan_block_counts(a.bcount, nb, 2 * n_frames, totals, st);
    if (rc != MVX_OK) return rc;
    hipLaunchKernelGGL(ignore_write, dim3(nb, n_frames), dim3(256), 0, st, (const unsigned *)a.map, (const int *)a.wstats, N, w,
                       anchors_per_loc, nb, (const int *)a.bcount, (const int *)totals, (long long *)pos_out, (long long *)neg_out,
                       (long long *)gi_out, (long long)cap_out, counts_out, stats, status);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}
