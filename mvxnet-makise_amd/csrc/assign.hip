// Max-IoU anchor assignment on the GPU: thresholds plus "the best anchor of every ground truth".
//
// The reference's classifyAnchors (anchors.hip) has no forced match, lists an anchor once per box that reaches the threshold
// and needs the centre cells from the host.  The rule here, per frame, with iou(g, a) = 0 when the bounding circles are apart
// (circles_apart) and quad_iou(ground truth, anchor) otherwise -- bit-equal to mvx_bbox_pairwise(gts, anchors, 1)[g][a]:
//     m(a) = max_g iou(g, a), o(a) the lowest g attaining it;  b(g) = max_a iou(g, a), c(g) the lowest a attaining it
//     positive by threshold: m(a) >= pos_thr, matched to o(a)
//     positive by force:     a = c(g) of a g with b(g) >= force_thr; several g on one anchor: the largest iou(g, a), ties the
//                            lowest g; a forced match overrides o(a)
//     not negative:          m(a) >= neg_thr, plus every positive
// Every anchor at most once per list, lists in ascending flat index (x * W + y) * A + z, gi local to the frame.
//
// Five launches and one memset for any number of frames and boxes:
//     memset  key map u64 [F][N] = 0
//     1  assign_window   a workgroup per (ground truth, orientation): the IoUs of a (2R+1)^2 window of cells around the box's
//                        centre cell (found here, from the quad and the anchor table); every IoU >= neg_thr goes into the
//                        anchor's key with atomicMax; the pair's best (iou, lowest index) by a fixed-order tree in LDS
//     2  assign_boxes    a thread per ground truth: b(g), c(g) from its A pairs, gt_best, the exactness test of the window,
//                        and the forced key
//     3  assign_count    per block of 256 anchors: how many are positive / not negative
//     4  scan of the block counts (mvxi_scan_block_counts, 2F rows)
//     5  assign_write    order-preserving compaction of the map into the lists (compact.h), counts clipped to cap
// The key of an anchor is  forced << 63 | iou bits << 32 | ~g : the largest key is the match the rule asks for (a forced
// match beats a threshold match, a larger IoU a smaller, a lower g a higher), so the 64-bit integer atomicMax gives the same
// map whatever the order of arrival -- no float atomics, two runs are bitwise equal.
//
// Why the window is exact.  The anchor table is taken as the regular grid create_anchors makes (centre of cell (x, y) =
// centre of cell (0, 0) + (x * dx, y * dy), every orientation of a cell about the same centre and of one size over the grid;
// the far corner of the table is tested against that and a table that is no such grid gets status 1).  The centre cell
// (nl, nw) is the nearest one, unclamped, so an anchor of the grid outside the window in x is at least (R + 0.5) |dx| away in
// x -- (k - 0.5) |dx| when the nearest cell the window leaves out is k cells from nl, which is more than R + 1 for a centre
// beyond the grid's edge (cells_outside) -- and likewise in y.  Per (box, orientation), with a 0.1 % margin for the f32 roundings:
//   - if that distance exceeds the circles_apart bound 1.01 (r_gt + r_anchor) + 1e-3 on every axis the window does not span
//     wholly, every anchor outside has iou = 0 by the rule: exact;
//   - otherwise the intersection with an anchor outside lies inside the overlap of the two bounding rectangles, at most
//     (hx_gt + hx_a - distance) wide and 2 min(hy_gt, hy_a) high, and the union is at least the larger box, which bounds the
//     true IoU by `ub`; the f32 IoU is within 3e-4 of the truth (targets_cases.IOU_BOUND).  If ub + 1e-3 is below both neg_thr
//     and b(g), no anchor outside can enter a list, be c(g) or change b(g): exact.  If not: status bit 1, replay with a
//     larger radius.
#include "anchor_lists.h"
#include "bev_iou.h"

namespace {

constexpr unsigned long long FORCED = 1ull << 63;
constexpr float NOISE = 1e-3f;              // > IOU_BOUND = 3e-4, the largest |f32 IoU - truth|

__device__ __forceinline__ unsigned long long make_key(float iou, int g_local) {
    return ((unsigned long long)__float_as_uint(iou) << 32) | (unsigned long long)(~(unsigned)g_local);
}
__device__ __forceinline__ float key_iou(unsigned long long k) { return __uint_as_float((unsigned)(k >> 32) & 0x7fffffffu); }
__device__ __forceinline__ int key_g(unsigned long long k) { return (int)(~(unsigned)k); }

__device__ __forceinline__ int frame_of(const FrameOffsets &o, int F, int g) {
    int f = 0;
    for (int k = 1; k < F; ++k) f += (g >= o.off[k]);
    return f;
}

// centre and half extents of a quad's bounding rectangle about its circle centre
__device__ __forceinline__ void half_extents(const float *quad8, P2 c, float &hx, float &hy) {
    hx = 0.f; hy = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        hx = fmaxf(hx, fabsf(quad8[2 * k] - c.x));
        hy = fmaxf(hy, fabsf(quad8[2 * k + 1] - c.y));
    }
}

__device__ __forceinline__ float quad_area(const float *q) {      // |shoelace| in f32, for the bound only
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int n = (k + 1) & 3;
        acc += q[2 * k] * q[2 * n + 1] - q[2 * k + 1] * q[2 * n];
    }
    return 0.5f * fabsf(acc);
}

// Cells between the centre cell n and the nearest cell of the grid [0, len) that the window [n - R, n + R] leaves out along one
// axis (at least R + 1; more when the centre lies beyond the grid's edge), or 0 when the window spans the axis.
__device__ __forceinline__ long long cells_outside(long long n, int R, int len) {
    const long long lo = n - R - 1, hi = n + R + 1;                // the first cells left out below and above the window
    long long d = 0;
    if (lo >= 0) d = n - (lo < len - 1 ? lo : len - 1);
    if (hi <= len - 1) {
        const long long e = (hi > 0 ? hi : 0) - n;
        d = d == 0 || e < d ? e : d;
    }
    return d;
}

// pair_best: per pair [iou f32, lowest flat anchor index i32, ub f32, 1 if anchors of the grid lie outside the window]
__global__ __launch_bounds__(256) void assign_window(const float *__restrict__ gts, const float *__restrict__ anchors, int L, int W,
                                                     int A, FrameOffsets goff, int F, float neg_thr, int R,
                                                     unsigned long long *__restrict__ keymap, float *__restrict__ pair_iou,
                                                     int *__restrict__ pair_idx, float *__restrict__ pair_ub,
                                                     int *__restrict__ pair_outside, int *__restrict__ status) {
    __shared__ P2 s_poly[POLY_SLOTS * 256];
    __shared__ float s_best[256];
    __shared__ int s_bidx[256];
    const int pair = blockIdx.x, g = pair / A, z = pair % A;
    const int f = frame_of(goff, F, g);
    const long long N = (long long)L * W * A;
    const Polys wk = polys_of(s_poly, 256, threadIdx.x);
    const LP gt = wk.q1, q = wk.q2;
    const float *gq = gts + (size_t)g * 8;
    load_quad(gt, gq);
    P2 gc;
    float gr;
    quad_circle(gt, gc, gr);
    const float gt_area = fabsf(shoelace(gt, 4));
    orient_ccw(gt);
    // the grid: centre of cell (0, 0), the pitches, the centre cell of this box
    P2 c00, c10 = {0.f, 0.f}, c01 = {0.f, 0.f};
    float r00;
    quad_circle((const P2 *)anchors, c00, r00);
    if (L > 1) { float r; quad_circle((const P2 *)(anchors + (size_t)W * A * 8), c10, r); }
    if (W > 1) { float r; quad_circle((const P2 *)(anchors + (size_t)A * 8), c01, r); }
    const float dx = L > 1 ? c10.x - c00.x : 0.f, dy = W > 1 ? c01.y - c00.y : 0.f;
    const float lim = 1048576.f;
    const long long nl = dx != 0.f ? (long long)fminf(fmaxf(floorf((gc.x - c00.x) / dx + 0.5f), -lim), lim) : 0;
    const long long nw = dy != 0.f ? (long long)fminf(fmaxf(floorf((gc.y - c00.y) / dy + 0.5f), -lim), lim) : 0;
    const int Wn = 2 * R + 1;
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    for (int c = threadIdx.x; c < Wn * Wn; c += blockDim.x) {       // ascending c = ascending flat index: the first best stays
        const long long x = nl + c / Wn - R, y = nw + c % Wn - R;
        if (x < 0 || x >= L || y < 0 || y >= W) continue;
        const long long a = (x * W + y) * A + z;
        const float *aq = anchors + (size_t)a * 8;
        load_quad(q, aq);
        P2 ac;
        float ar;
        quad_circle(q, ac, ar);
        float iou = 0.f;
        if (!circles_apart(gc, gr, ac, ar)) {
            const float a_area = fabsf(shoelace(q, 4));
            orient_ccw(q);
            const float inter = quad_intersection(gt, q, wk.p, wk.q);
            iou = inter / (gt_area + a_area - inter);
        }
        if (iou > best) { best = iou; bidx = (int)a; }
        if (iou >= neg_thr) atomicMax(keymap + (size_t)f * N + a, make_key(iou, g - goff.off[f]));
    }
    s_best[threadIdx.x] = best;
    s_bidx[threadIdx.x] = bidx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {                             // fixed order: the same tree every run
        if (threadIdx.x < s) {
            const float o = s_best[threadIdx.x + s];
            const int oi = s_bidx[threadIdx.x + s];
            if (o > s_best[threadIdx.x] || (o == s_best[threadIdx.x] && oi < s_bidx[threadIdx.x])) {
                s_best[threadIdx.x] = o;
                s_bidx[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    // what the window leaves out (header comment)
    const long long cx = cells_outside(nl, R, L), cy = cells_outside(nw, R, W);
    const bool xcover = cx == 0, ycover = cy == 0;
    const float *a0 = anchors + (size_t)z * 8;                      // the anchor of this orientation at cell (0, 0)
    P2 a0c;
    float a0r, hxa, hya, hxg, hyg;
    quad_circle((const P2 *)a0, a0c, a0r);
    half_extents(a0, a0c, hxa, hya);
    half_extents(gq, gc, hxg, hyg);
    const float distx = ((float)cx - 0.5f) * fabsf(dx) * 0.999f, disty = ((float)cy - 0.5f) * fabsf(dy) * 0.999f;
    const float reach = 1.01f * (gr + a0r) + 2e-3f;
    const bool x0 = xcover || distx > reach, y0 = ycover || disty > reach;
    const float big = fmaxf(fmaxf(gt_area, quad_area(a0)), 1e-12f);
    const float ubx = x0 ? 0.f : fmaxf(0.f, hxg + hxa + 1e-3f - distx) * 2.f * fminf(hyg, hya) / big;
    const float uby = y0 ? 0.f : fmaxf(0.f, hyg + hya + 1e-3f - disty) * 2.f * fminf(hxg, hxa) / big;
    float ub = (x0 && y0) ? -1.f : fmaxf(ubx, uby);
    if (!(ub == ub)) ub = 2.f;                                      // a NaN box: never exact
    pair_iou[pair] = s_best[0];
    pair_idx[pair] = s_bidx[0];
    pair_ub[pair] = ub;
    pair_outside[pair] = !(xcover && ycover);
    if (pair == 0) {                                                // is the table the regular grid the argument above needs?
        P2 cf;
        float rf;
        quad_circle((const P2 *)(anchors + ((size_t)(L - 1) * W + (W - 1)) * A * 8), cf, rf);
        const float ex = fabsf(cf.x - (c00.x + (L - 1) * dx)), ey = fabsf(cf.y - (c00.y + (W - 1) * dy));
        const bool ok = (L == 1 || (dx != 0.f && ex <= 0.25f * fabsf(dx))) && (W == 1 || (dy != 0.f && ey <= 0.25f * fabsf(dy)));
        if (!ok) atomicOr(status, 1);
    }
}

__global__ __launch_bounds__(256) void assign_boxes(int G, int A, long long N, FrameOffsets goff, int F, float neg_thr, float force_thr,
                                                    const float *__restrict__ pair_iou, const int *__restrict__ pair_idx,
                                                    const float *__restrict__ pair_ub, const int *__restrict__ pair_outside,
                                                    unsigned long long *__restrict__ keymap, float *__restrict__ gt_best,
                                                    int *__restrict__ status) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    float b = -INFINITY;
    int c = 0x7fffffff, outside = 0;
    for (int z = 0; z < A; ++z) {
        const float v = pair_iou[g * A + z];
        const int i = pair_idx[g * A + z];
        if (v > b || (v == b && i < c)) { b = v; c = i; }
        outside |= pair_outside[g * A + z];
    }
    if (b < 0.f && outside) b = 0.f;                               // an anchor outside the window is at least 0 (or status 1 below)
    bool exact = true;
    for (int z = 0; z < A; ++z) {
        const float ub = pair_ub[g * A + z];
        if (ub >= 0.f && !(ub + NOISE < fminf(neg_thr, b))) exact = false;
    }
    if (!exact) atomicOr(status, 1);
    gt_best[g] = b;
    if (force_thr <= 1.5f && b >= force_thr) {
        const int f = frame_of(goff, F, g);
        atomicMax(keymap + (size_t)f * N + c, FORCED | make_key(b, g - goff.off[f]));
    }
}

// flags of an anchor from its key: bit 0 = not negative, bit 1 = positive
__device__ __forceinline__ int key_flags(unsigned long long k, float pos_thr) {
    if (k == 0) return 0;
    return 1 | (((k & FORCED) || key_iou(k) >= pos_thr) ? 2 : 0);
}

__global__ __launch_bounds__(256) void assign_count(const unsigned long long *__restrict__ keymap, long long N, int nblocks, float pos_thr,
                                                    int *__restrict__ bcount) {
    __shared__ int s[2][4];
    const int f = blockIdx.y;
    const long long a = (long long)blockIdx.x * 256 + threadIdx.x;
    list_block_counts(a < N ? key_flags(keymap[(size_t)f * N + a], pos_thr) : 0, f, nblocks, s, bcount);
}

__global__ __launch_bounds__(256) void assign_write(const unsigned long long *__restrict__ keymap, long long N, int W, int A, int nblocks,
                                                    float pos_thr, const int *__restrict__ boff, const int *__restrict__ totals,
                                                    long long *__restrict__ pos_idx, long long *__restrict__ neg_idx,
                                                    long long *__restrict__ gi, long long cap, int *__restrict__ counts,
                                                    int *__restrict__ status) {
    __shared__ int s[2][4];
    const int f = blockIdx.y;
    const long long a = (long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long k = a < N ? keymap[(size_t)f * N + a] : 0ull;
    list_write(key_flags(k, pos_thr), key_g(k), f, a, W, A, nblocks, s, boff, totals, pos_idx, neg_idx, gi, cap, counts, status);
}

}  // namespace

extern "C" size_t mvx_assign_anchors_frames_workspace_bytes(int32_t n_gt_total, int32_t n_frames, int32_t l, int32_t w,
                                                            int32_t anchors_per_loc) {
    if (n_gt_total <= 0 || n_frames <= 0 || l <= 0 || w <= 0 || anchors_per_loc <= 0) return 256;
    const size_t N = (size_t)l * w * anchors_per_loc, pairs = (size_t)n_gt_total * anchors_per_loc;
    const size_t nb = (N + 255) / 256;
    return up256((size_t)n_frames * N * 8) + up256(pairs * 16) + up256(2 * (size_t)n_frames * nb * 4) + up256(2 * (size_t)n_frames * 4);
}

extern "C" int mvx_assign_anchors_frames(const float *gts, const int32_t *gt_off_host, int32_t n_frames, const float *anchors,
                                         int32_t l, int32_t w, int32_t anchors_per_loc, float neg_thr, float pos_thr,
                                         float force_thr, int32_t window_radius, int64_t *pos_idx, int64_t *neg_idx, int64_t *gi,
                                         int64_t cap, int32_t *counts, float *gt_best, int32_t *status, void *workspace,
                                         size_t workspace_bytes, void *stream) {
    MVX_CHECK_ARG(gt_off_host && n_frames >= 1 && n_frames <= MVX_MAX_FRAMES);
    MVX_CHECK_ARG(l > 0 && w > 0 && anchors_per_loc > 0 && window_radius >= 1 && window_radius <= 55);
    MVX_CHECK_ARG(neg_thr > 0.f && neg_thr <= pos_thr && force_thr > 0.f);
    MVX_CHECK_ARG(counts && status && cap >= 0);
    MVX_CHECK_ARG((long long)l * w * anchors_per_loc < (1ll << 31));
    FrameOffsets goff;
    MVX_CHECK_ARG(frame_offsets(gt_off_host, n_frames, goff));
    const int n_gt = goff.off[n_frames];
    hipStream_t st = (hipStream_t)stream;
    if (n_gt == 0) {
        hipError_t e = hipMemsetAsync(counts, 0, 2 * sizeof(int32_t) * n_frames, st);
        return e == hipSuccess ? MVX_OK : (int)e;
    }
    MVX_CHECK_ARG((long long)n_gt * anchors_per_loc < (1ll << 31));
    MVX_CHECK_ARG(gts && anchors && pos_idx && neg_idx && gi && gt_best && workspace);
    MVX_CHECK_ARG(workspace_bytes >= mvx_assign_anchors_frames_workspace_bytes(n_gt, n_frames, l, w, anchors_per_loc));
    const long long N = (long long)l * w * anchors_per_loc;
    const int pairs = n_gt * anchors_per_loc, nb = (int)mvx_cdiv(N, 256);
    char *ws = (char *)workspace;
    unsigned long long *keymap = (unsigned long long *)ws;
    ws += up256((size_t)n_frames * N * 8);
    float *pair_iou = (float *)ws;
    int *pair_idx = (int *)(pair_iou + pairs);
    float *pair_ub = (float *)(pair_idx + pairs);
    int *pair_outside = (int *)(pair_ub + pairs);
    ws += up256((size_t)pairs * 16);
    int *bcount = (int *)ws;
    ws += up256(2 * (size_t)n_frames * nb * 4);
    int *totals = (int *)ws;
    hipError_t e = hipMemsetAsync(keymap, 0, (size_t)n_frames * N * 8, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(assign_window, dim3(pairs), dim3(256), 0, st, gts, anchors, l, w, anchors_per_loc, goff, n_frames, neg_thr,
                       window_radius, keymap, pair_iou, pair_idx, pair_ub, pair_outside, status);
    MVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(assign_boxes, dim3(mvx_cdiv(n_gt, 256)), dim3(256), 0, st, n_gt, anchors_per_loc, N, goff, n_frames, neg_thr,
                       force_thr, (const float *)pair_iou, (const int *)pair_idx, (const float *)pair_ub, (const int *)pair_outside,
                       keymap, gt_best, status);
    MVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(assign_count, dim3(nb, n_frames), dim3(256), 0, st, (const unsigned long long *)keymap, N, nb, pos_thr, bcount);
    MVX_LAUNCH_CHECK();
    const int rc = mvxi_scan_block_counts(bcount, nb, 2 * n_frames, totals, st);
    if (rc != MVX_OK) return rc;
    hipLaunchKernelGGL(assign_write, dim3(nb, n_frames), dim3(256), 0, st, (const unsigned long long *)keymap, N, w, anchors_per_loc, nb,
                       pos_thr, (const int *)bcount, (const int *)totals, (long long *)pos_idx, (long long *)neg_idx, (long long *)gi,
                       (long long)cap, counts, status);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}
