// Focal loss of the RPN heads for all frames of a step: forward + backward in three launches and one memset, for any F.
//
// Reads the raw head output of rpn_frames.rpn_forward, rows [A cls logits | 7A regression] (A anchors per location), and the
// lists mvx_classify_anchors_frames writes.  Per frame f, by SET membership of the anchors (VoxelLoss subtracts an anchor
// that is listed twice two times; here it counts once):
//   positive = listed in pos_idx; ignored = listed in neg_idx (the NOT-negative anchors) and not positive; negative = the rest
//   cls_f = cls_weight / max(1, n_pos) * ( sum_pos alpha (1-p)^gamma (-log p) + sum_neg (1-alpha) p^gamma (-log(1-p)) )
//   reg_f = reg_weight * VoxelLoss's regression term (csrc/loss.hip: its targets, SmoothL1 with beta 1, once per pos_idx
//           entry, mean over n_pos * 7; 0 without a positive)
// Everything is evaluated from the logit x, so that nothing overflows or cancels:
//   -log(1-p) = softplus(x) = max(x,0) + log1p(exp(-|x|)),  -log p = softplus(-x),  p and 1-p from exp(-|x|),
//   p^gamma = exp(-gamma softplus(-x)),  (1-p)^gamma = exp(-gamma softplus(x)).
//
//   1. focal_flags   the lists of all frames -> one flag byte per anchor (bit 0 positive, bit 1 listed in neg_idx), OR-ed
//                    into the zeroed workspace: the result does not depend on the order
//   2. focal_dense   all rows of all frames: the whole 8A-wide gradient row (regression columns zero) and ONE f64 partial
//                    sum per workgroup, each reduced in a fixed order
//   3. focal_lists   one workgroup per frame: the regression term (float atomicAdd into the regression columns only:
//                    entries that name the same anchor collide there), then the frame's partials summed in index order
// No f64 atomic, no atomic across workgroups on a sum: the losses are bitwise reproducible, and so is the gradient whenever
// no anchor is listed twice in pos_idx.  counts and gt_off are read on the device: the host reads nothing.
//
// mvx_focal_loss_dir_frames is the same three launches with a direction classifier (SECOND, PointPillars): rows of any stride
// (heads / d_heads may carry further columns), and per pos_idx entry of anchor a, box g and direction logit x, in focal_lists:
//   angle column   SmoothL1(sin D), D = r6 - (g6 - an6), in place of SmoothL1(D): blind to half turns; gradient
//                  reg_scale * SmoothL1'(sin D) * cos D
//   direction bit  b = floor(mod(g6 - dir_offset, 2 pi) / pi) = floor((g6 - dir_offset) / pi) mod 2
//   dir_f = dir_weight / max(1, n_pos) * sum (b ? softplus(-x) : softplus(x)),  gradient dir_weight / max(1, n_pos) * (sigmoid(x) - b)
// The direction logits and their gradient come as pointer + row stride: columns of the head rows (the dense pass zeroes them
// with the rest of the row) or a tensor of their own (the dense pass zeroes its A columns).  losses is (F,3) = (cls, reg, dir).
//
// mvx_focal_loss_iou_frames adds the IoU-aware confidence head (CIA-SSD, AFDetV2) and one launch, focal_iou,
// between the dense and the list pass.  Per pos_idx entry of anchor a, box g and IoU logit x (entries the regression term skips
// are skipped, duplicates count every time), with the anchor's regression row r read as a constant:
//   b = the 'loss' decode of detect_select (diagonal of (an3, an4), expf on the sizes, b6 = r6 + an6, no direction fold)
//   I = BEV intersection of box_quad(b) and box_quad(g) (bev_iou.h), 0 when circles_apart; ih = min(b2+b5, g2+g5) - max(b2, g2)
//   q = clamp(I ih / (b3 b4 b5 + g3 g4 g5 - I ih), 0, 1), 0 when ih <= 0, when b is not finite or the quotient is not
//   iou_f = iou_weight / max(1, n_pos) * sum (softplus(x) - q x),  gradient iou_weight / max(1, n_pos) * (sigmoid(x) - q)
// Nothing flows into the regression columns.  The clipping keeps POLY_SLOTS P2 per thread in LDS (320 B), so the pass cannot
// live in the 1024-thread focal_lists (320 KB): 128 threads (40 KB), grid (nq, F), nq = min(ceil(cap / 128), 64), a strided loop
// over the entries and one f64 partial per workgroup, which focal_lists sums in index order into losses[f][3].  The IoU logits
// and their gradient come as pointer + row stride like the direction logits.  losses is (F,4) = (cls, reg, dir, iou).
#include "bev_iou.h"

namespace {

constexpr int DENSE_THREADS = 256;
constexpr int DENSE_MAX_BLOCKS = 128;      // workgroups (= partial sums) per frame at most
constexpr int LIST_BLOCKS = 8;             // workgroups per frame of the flag pass
constexpr int LIST_THREADS = 1024;
constexpr int IOU_THREADS = 128;           // focal_iou: 40 KB of polygon slots per workgroup
constexpr int IOU_MAX_BLOCKS = 64;         // its workgroups (= partial sums) per frame at most

inline int iou_blocks(long long cap) {
    const long long want = (cap + IOU_THREADS - 1) / IOU_THREADS;
    return (int)(want > IOU_MAX_BLOCKS ? IOU_MAX_BLOCKS : (want < 1 ? 1 : want));
}

struct Layout {
    long long n_anchors;      // per frame
    long long flag_bytes;     // all frames, one byte per anchor, rounded up to 256
    int nb;                   // workgroups of the dense pass per frame
    bool ok;
    // ld: floats per row of the gradient the dense pass writes (8A for the plain rows)
    Layout(int F, int l, int w, int A, int ld) {
        ok = F >= 1 && F <= MVX_MAX_FRAMES && l > 0 && w > 0 && A >= 1 && A <= 4 && ld >= 8 * A && ld % 4 == 0 &&
             (long long)F * l * w * ld < (1ll << 31);
        n_anchors = ok ? (long long)l * w * A : 0;
        flag_bytes = ((long long)F * n_anchors + 255) & ~255ll;
        const long long chunks = (long long)l * w * (ld / 4);   // float4 pieces of a frame's rows
        const long long want = ok ? (chunks + DENSE_THREADS * 4 - 1) / (DENSE_THREADS * 4) : 0;
        nb = (int)(want > DENSE_MAX_BLOCKS ? DENSE_MAX_BLOCKS : want);
    }
    long long partials() const { return flag_bytes; }
    long long total(int F) const { return ok ? flag_bytes + (long long)F * nb * (long long)sizeof(double) : 0; }
};

struct Lists {
    const long long *pos, *neg, *gi;      // (F,3,cap), (F,3,cap), (F,cap)
    long long cap;
    const int *counts;                    // (F,2)
};

__device__ __forceinline__ int list_count(const Lists &ls, int f, int which) {
    const int n = ls.counts[2 * f + which];
    return n < 0 ? 0 : ((long long)n > ls.cap ? (int)ls.cap : n);
}

// anchor (x, y, z) of entry k of a (3,cap) list -> index inside the frame, or -1 when it lies outside the grid
__device__ __forceinline__ long long list_anchor(const long long *idx, long long cap, int k, int L, int W, int A) {
    const long long x = idx[k], y = idx[cap + k], z = idx[2 * cap + k];
    if (x < 0 || x >= L || y < 0 || y >= W || z < 0 || z >= A) return -1;
    return (x * W + y) * A + z;
}

__global__ void focal_flags(Lists ls, int L, int W, int A, unsigned *__restrict__ flags) {
    const int f = blockIdx.y;
    const long long base = (long long)f * L * W * A;
    const int n_pos = list_count(ls, f, 0), n_neg = list_count(ls, f, 1);
    const long long *pos = ls.pos + (size_t)f * 3 * ls.cap, *neg = ls.neg + (size_t)f * 3 * ls.cap;
    const int step = gridDim.x * blockDim.x;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n_pos; k += step) {
        const long long a = list_anchor(pos, ls.cap, k, L, W, A);
        if (a >= 0) atomicOr(flags + ((base + a) >> 2), 1u << (8 * (unsigned)((base + a) & 3)));
    }
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n_neg; k += step) {
        const long long a = list_anchor(neg, ls.cap, k, L, W, A);
        if (a >= 0) atomicOr(flags + ((base + a) >> 2), 2u << (8 * (unsigned)((base + a) & 3)));
    }
}

// sum over the workgroup in a fixed order (lanes by xor shuffles, then the waves in index order); valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double *s_part) {
    v = wave_sum_f64(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) s_part[wid] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < (int)(blockDim.x >> 6); ++k) t += s_part[k];
    return t;
}

// One thread per float4 of a gradient row (ldd floats); the first float4 of a row holds its A <= 4 logits.  zero / ldz: a
// direction gradient outside the head rows, whose A columns per row are zeroed here for the list pass to add into; zero2 /
// ldz2: the same for an IoU gradient outside the head rows (focal_iou adds into it).
__global__ void __launch_bounds__(DENSE_THREADS)
focal_dense(const float *__restrict__ heads, int ld, int rows, int A, const unsigned char *__restrict__ flags, Lists ls, float alpha,
            float gamma, float cls_weight, float *__restrict__ d_heads, int ldd, float *__restrict__ zero, int ldz,
            float *__restrict__ zero2, int ldz2, double *__restrict__ partials) {
    const int f = blockIdx.y;
    const int cpr = ldd >> 2, cpr_in = ld >> 2;              // float4 pieces per row
    const long long chunks = (long long)rows * cpr;
    const float4 *src = (const float4 *)(heads + (size_t)f * rows * ld);
    float4 *dst = d_heads ? (float4 *)(d_heads + (size_t)f * rows * ldd) : nullptr;
    const unsigned char *fl = flags + (size_t)f * rows * A;
    const int n_pos = list_count(ls, f, 0);
    const float scale = cls_weight / (float)(n_pos > 1 ? n_pos : 1);
    double part = 0.0;
    for (long long i = (long long)blockIdx.x * DENSE_THREADS + threadIdx.x; i < chunks; i += (long long)gridDim.x * DENSE_THREADS) {
        const long long row = i / cpr;
        float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i - row * cpr == 0) {
            const float4 in = src[row * cpr_in];
            const float xs[4] = {in.x, in.y, in.z, in.w};
            float g[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                if (a >= A) break;
                const unsigned flag = fl[row * A + a];
                if (flag == 2u) continue;                    // ignored: no loss, no gradient
                const float x = xs[a];
                const float e = expf(-fabsf(x));
                const float l1p = log1pf(e);
                const float sp_x = fmaxf(x, 0.f) + l1p;      // softplus(x)  = -log(1 - p)
                const float sp_mx = fmaxf(-x, 0.f) + l1p;    // softplus(-x) = -log p
                const float inv = 1.f / (1.f + e);
                const float p = x >= 0.f ? inv : e * inv, q = x >= 0.f ? e * inv : inv;
                if (flag & 1u) {
                    const float m = alpha * expf(-gamma * sp_x);               // alpha (1-p)^gamma
                    part += (double)(m * sp_mx);
                    g[a] = -scale * m * (q + gamma * p * sp_mx);
                } else {
                    const float m = (1.f - alpha) * expf(-gamma * sp_mx);      // (1-alpha) p^gamma
                    part += (double)(m * sp_x);
                    g[a] = scale * m * (p + gamma * q * sp_x);
                }
            }
            out = make_float4(g[0], g[1], g[2], g[3]);
        }
        if (dst) dst[i] = out;
    }
    if (zero)
        for (long long i = (long long)blockIdx.x * DENSE_THREADS + threadIdx.x; i < (long long)rows * A; i += (long long)gridDim.x * DENSE_THREADS)
            zero[((size_t)f * rows + i / A) * ldz + i % A] = 0.f;
    if (zero2)
        for (long long i = (long long)blockIdx.x * DENSE_THREADS + threadIdx.x; i < (long long)rows * A; i += (long long)gridDim.x * DENSE_THREADS)
            zero2[((size_t)f * rows + i / A) * ldz2 + i % A] = 0.f;
    __shared__ double s_part[DENSE_THREADS / 64];
    const double t = block_sum_f64(part, s_part);
    if (threadIdx.x == 0) partials[(size_t)f * gridDim.x + blockIdx.x] = t;
}

// The direction classifier of mvx_focal_loss_dir_frames: logits x and their gradient d as pointer + row stride.
struct Dir {
    const float *x;
    float *d;
    int ldx, ldd;
    float weight, offset;
};

constexpr float PI_F = 3.14159265358979323846f;

// The IoU head of mvx_focal_loss_iou_frames: logits x and their gradient d as pointer + row stride, the optional target output
// q_out (F,cap), and the f64 partials (F,nq) of focal_iou that focal_lists sums.
struct Iou {
    const float *x;
    float *d;
    int ldx, ldd;
    float weight;
    float *q_out;
    double *partials;
    int nq;
};

// grid (nq, F): a strided loop over the frame's pos_idx entries, one thread per entry at a time
__global__ void __launch_bounds__(IOU_THREADS)
focal_iou(const float *__restrict__ heads, int ld, Lists ls, const float *__restrict__ gts, int gt_ld, const int *__restrict__ gt_off,
          const float *__restrict__ anchors, int L, int W, int A, Iou iou) {
    __shared__ P2 s_poly[POLY_SLOTS * IOU_THREADS];
    __shared__ double s_part[IOU_THREADS / 64];
    const int f = blockIdx.y;
    const int n_pos = list_count(ls, f, 0);
    const long long *pos = ls.pos + (size_t)f * 3 * ls.cap, *gi = ls.gi + (size_t)f * ls.cap;
    const int g_lo = gt_off[f], n_gt = gt_off[f + 1] - g_lo;
    const size_t cell0 = (size_t)f * L * W;
    const float scale = iou.weight / (float)(n_pos > 1 ? n_pos : 1);
    const Polys w = polys_of(s_poly, IOU_THREADS, threadIdx.x);
    const long long end = iou.q_out ? ls.cap : (long long)n_pos;       // q_out is written for every slot of the list
    double s_iou = 0.0;
    for (long long k = (long long)blockIdx.x * IOU_THREADS + threadIdx.x; k < end; k += (long long)gridDim.x * IOU_THREADS) {
        float q = -1.f;
        const long long a = k < n_pos ? list_anchor(pos, ls.cap, (int)k, L, W, A) : -1;
        const long long gk = k < n_pos ? gi[k] : -1;
        if (a >= 0 && gk >= 0 && gk < n_gt) {
            const int z = (int)(a % A);
            const float *g = gts + (size_t)(g_lo + gk) * gt_ld;
            const float *an = anchors + (size_t)a * 7;
            const size_t cell = cell0 + (size_t)(a / A);
            const float *r = heads + cell * ld + A + z * 7;
            const float d = sqrtf(an[3] * an[3] + an[4] * an[4]);
            float b[7], gb[7];
            b[0] = r[0] * d + an[0];
            b[1] = r[1] * d + an[1];
            b[2] = r[2] * an[5] + an[2];
            b[3] = expf(r[3]) * an[3];
            b[4] = expf(r[4]) * an[4];
            b[5] = expf(r[5]) * an[5];
            b[6] = r[6] + an[6];
            bool ok = true;
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                gb[c] = g[c];
                ok = ok && isfinite(b[c]) && isfinite(gb[c]);
            }
            q = 0.f;
            const float ih = fminf(b[2] + b[5], gb[2] + gb[5]) - fmaxf(b[2], gb[2]);      // z is the bottom face (box3d.h)
            if (ok && ih > 0.f) {
                P2 q1[4], q2[4], c1, c2;
                float r1, r2;
                box_quad(b, q1);
                box_quad(gb, q2);
                quad_circle(q1, c1, r1);
                quad_circle(q2, c2, r2);
                if (!circles_apart(c1, r1, c2, r2)) {
                    load_oriented(w.q1, (const float *)q1);      // the areas are not used: the volumes below are l w h
                    load_oriented(w.q2, (const float *)q2);
                    const float inter = quad_intersection(w.q1, w.q2, w.p, w.q);
                    const float vol = inter * ih;
                    const float v = vol / (b[3] * b[4] * b[5] + gb[3] * gb[4] * gb[5] - vol);
                    q = isfinite(v) ? fminf(fmaxf(v, 0.f), 1.f) : 0.f;
                }
            }
            const float x = iou.x[cell * iou.ldx + z];
            const float e = expf(-fabsf(x));
            const float l1p = log1pf(e);
            s_iou += (double)(fmaxf(x, 0.f) + l1p) - (double)q * (double)x;      // softplus(x) - q x
            const float inv = 1.f / (1.f + e);
            if (iou.d) atomicAdd(iou.d + cell * iou.ldd + z, scale * ((x >= 0.f ? inv : e * inv) - q));
        }
        if (iou.q_out) iou.q_out[(size_t)f * ls.cap + k] = q;
    }
    const double t = block_sum_f64(s_iou, s_part);
    if (threadIdx.x == 0) iou.partials[(size_t)f * gridDim.x + blockIdx.x] = t;
}

template <bool DIR, bool IOU>
__global__ void __launch_bounds__(LIST_THREADS)
focal_lists(const float *__restrict__ heads, int ld, Lists ls, const float *__restrict__ gts, int gt_ld,
            const int *__restrict__ gt_off, const float *__restrict__ anchors, int L, int W, int A, float cls_weight,
            float reg_weight, float *__restrict__ d_heads, int ldd, const double *__restrict__ partials, int nb, Dir dir,
            Iou iou, float *__restrict__ losses) {
    const int f = blockIdx.x;
    const int n_pos = list_count(ls, f, 0);
    const long long *pos = ls.pos + (size_t)f * 3 * ls.cap, *gi = ls.gi + (size_t)f * ls.cap;
    const int g_lo = gt_off[f], n_gt = gt_off[f + 1] - g_lo;
    const size_t cell0 = (size_t)f * L * W;
    const float reg_scale = n_pos > 0 ? reg_weight / (float)(n_pos * 7) : 0.f;
    const float dir_scale = DIR ? dir.weight / (float)(n_pos > 1 ? n_pos : 1) : 0.f;
    double s_reg = 0.0, s_dir = 0.0;
    for (int k = threadIdx.x; k < n_pos; k += blockDim.x) {
        const long long a = list_anchor(pos, ls.cap, k, L, W, A);
        const long long gk = gi[k];
        if (a < 0 || gk < 0 || gk >= n_gt) continue;
        const int z = (int)(a % A);
        const float *g = gts + (size_t)(g_lo + gk) * gt_ld;
        const float *an = anchors + (size_t)a * 7;
        const float d = sqrtf(an[3] * an[3] + an[4] * an[4]);
        float t[7];
        t[0] = (g[0] - an[0]) / d;
        t[1] = (g[1] - an[1]) / d;
        t[2] = (g[2] - an[2]) / an[5];
        t[3] = logf(g[3] / an[3]);
        t[4] = logf(g[4] / an[4]);
        t[5] = logf(g[5] / an[5]);
        t[6] = g[6] - an[6];
        const size_t cell = cell0 + (size_t)(a / A);
        const size_t col0 = cell * ld + A + z * 7, dcol0 = cell * ldd + A + z * 7;
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            float diff = heads[col0 + c] - t[c];
            float chain = 1.f;
            if (DIR && c == 6) {                         // the angle through its sine: d/dD SmoothL1(sin D) = SmoothL1'(sin D) cos D
                const float delta = diff;
                sincosf(delta, &diff, &chain);
            }
            const float ad = fabsf(diff);
            s_reg += (double)(ad < 1.f ? 0.5f * diff * diff : ad - 0.5f);
            const float slope = ad < 1.f ? diff : (diff > 0.f ? 1.f : -1.f);
            if (d_heads) atomicAdd(d_heads + dcol0 + c, DIR && c == 6 ? reg_scale * slope * chain : reg_scale * slope);
        }
        if (DIR) {
            const int bit = (int)floorf((g[6] - dir.offset) / PI_F) & 1;
            const float x = dir.x[cell * dir.ldx + z];
            const float e = expf(-fabsf(x));
            const float l1p = log1pf(e);
            s_dir += (double)((bit ? fmaxf(-x, 0.f) : fmaxf(x, 0.f)) + l1p);      // softplus(-x) : softplus(x)
            const float inv = 1.f / (1.f + e);
            if (dir.d) atomicAdd(dir.d + cell * dir.ldd + z, dir_scale * ((x >= 0.f ? inv : e * inv) - (float)bit));
        }
    }
    __shared__ double s_part[LIST_THREADS / 64];
    __shared__ double s_part_dir[DIR ? LIST_THREADS / 64 : 1];
    __shared__ double s_cls[DENSE_MAX_BLOCKS];
    for (int k = threadIdx.x; k < nb; k += blockDim.x) s_cls[k] = partials[(size_t)f * nb + k];
    const double tr = block_sum_f64(s_reg, s_part);      // its barrier also publishes s_cls
    const double td = DIR ? block_sum_f64(s_dir, s_part_dir) : 0.0;
    if (threadIdx.x == 0) {
        double tc = 0.0;
        for (int k = 0; k < nb; ++k) tc += s_cls[k];
        float *out = losses + (IOU ? 4 : DIR ? 3 : 2) * f;
        out[0] = (float)((double)cls_weight * tc / (double)(n_pos > 1 ? n_pos : 1));
        out[1] = n_pos > 0 ? (float)((double)reg_weight * tr / (double)(n_pos * 7)) : 0.f;
        if (DIR) out[2] = (float)((double)dir.weight * td / (double)(n_pos > 1 ? n_pos : 1));
        if (IOU) {                                           // focal_iou's partials of this frame, in index order
            double ti = 0.0;
            for (int k = 0; k < iou.nq; ++k) ti += iou.partials[(size_t)f * iou.nq + k];
            out[3] = (float)((double)iou.weight * ti / (double)(n_pos > 1 ? n_pos : 1));
        }
    }
}

const Iou NO_IOU = {nullptr, nullptr, 0, 0, 0.f, nullptr, nullptr, 0};

// The launches of the three entry points.  dir.x == nullptr: the plain loss, losses (F,2); iou.x: focal_iou as a fourth
// launch, losses (F,4).
int focal_launch(const float *heads, int ld, int n_frames, int l, int w, int A, const Lists &ls, const float *gts, int gt_ld,
                 const int *gt_off, const float *anchors, float alpha, float gamma, float cls_weight, float reg_weight, float *d_heads,
                 int ldd, const Dir &dir, const Iou &iou, float *losses, const Layout &lay, void *workspace, hipStream_t st) {
    unsigned char *ws = (unsigned char *)workspace;
    double *partials = (double *)(ws + lay.partials());
    hipError_t e = hipMemsetAsync(ws, 0, (size_t)lay.flag_bytes, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(focal_flags, dim3(LIST_BLOCKS, n_frames), dim3(256), 0, st, ls, l, w, A, (unsigned *)ws);
    MVX_LAUNCH_CHECK();
    // a direction gradient that is not a column range of the d_heads rows is zeroed by the dense pass too
    const bool inside = dir.d && d_heads && dir.ldd == ldd && dir.d >= d_heads && dir.d + A <= d_heads + ldd;
    const bool inside_iou = iou.d && d_heads && iou.ldd == ldd && iou.d >= d_heads && iou.d + A <= d_heads + ldd;
    hipLaunchKernelGGL(focal_dense, dim3(lay.nb, n_frames), dim3(DENSE_THREADS), 0, st, heads, ld, l * w, A, ws, ls, alpha, gamma,
                       cls_weight, d_heads, ldd, dir.d && !inside ? dir.d : nullptr, dir.ldd, iou.d && !inside_iou ? iou.d : nullptr,
                       iou.ldd, partials);
    MVX_LAUNCH_CHECK();
    if (iou.x) {
        hipLaunchKernelGGL(focal_iou, dim3(iou.nq, n_frames), dim3(IOU_THREADS), 0, st, heads, ld, ls, gts, gt_ld, gt_off, anchors, l, w,
                           A, iou);
        MVX_LAUNCH_CHECK();
        hipLaunchKernelGGL((focal_lists<true, true>), dim3(n_frames), dim3(LIST_THREADS), 0, st, heads, ld, ls, gts, gt_ld, gt_off,
                           anchors, l, w, A, cls_weight, reg_weight, d_heads, ldd, partials, lay.nb, dir, iou, losses);
    } else if (dir.x)
        hipLaunchKernelGGL((focal_lists<true, false>), dim3(n_frames), dim3(LIST_THREADS), 0, st, heads, ld, ls, gts, gt_ld, gt_off,
                           anchors, l, w, A, cls_weight, reg_weight, d_heads, ldd, partials, lay.nb, dir, iou, losses);
    else
        hipLaunchKernelGGL((focal_lists<false, false>), dim3(n_frames), dim3(LIST_THREADS), 0, st, heads, ld, ls, gts, gt_ld, gt_off,
                           anchors, l, w, A, cls_weight, reg_weight, d_heads, ldd, partials, lay.nb, dir, iou, losses);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

}  // namespace

extern "C" int64_t mvx_focal_loss_frames_workspace_bytes(int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc) {
    return Layout(n_frames, l, w, anchors_per_loc, 8 * anchors_per_loc).total(n_frames);
}

extern "C" int mvx_focal_loss_frames(const float *heads, int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc,
                                     const int64_t *pos_idx, const int64_t *neg_idx, const int64_t *gi, int64_t cap,
                                     const int32_t *counts, const float *gts, int32_t gt_ld, const int32_t *gt_off,
                                     const float *anchors, float alpha, float gamma, float cls_weight, float reg_weight,
                                     float *d_heads, float *losses, void *workspace, int64_t workspace_bytes, void *stream) {
    const int ld = 8 * anchors_per_loc;
    const Layout lay(n_frames, l, w, anchors_per_loc, ld);
    MVX_CHECK_ARG(lay.ok);
    MVX_CHECK_ARG(heads && pos_idx && neg_idx && gi && counts && gts && gt_off && anchors && losses && workspace);
    MVX_CHECK_ARG(cap >= 1 && cap < (1ll << 31) && gt_ld >= 7);
    MVX_CHECK_ARG(alpha >= 0.f && alpha <= 1.f && gamma >= 0.f);
    MVX_CHECK_ARG(workspace_bytes >= lay.total(n_frames));
    // rows are read and written as float4; the flag words and the f64 partials sit in the workspace
    MVX_CHECK_ARG(((uintptr_t)heads & 15) == 0 && ((uintptr_t)d_heads & 15) == 0 && ((uintptr_t)workspace & 7) == 0);
    const Lists ls = {(const long long *)pos_idx, (const long long *)neg_idx, (const long long *)gi, (long long)cap, counts};
    const Dir none = {nullptr, nullptr, 0, 0, 0.f, 0.f};
    return focal_launch(heads, ld, n_frames, l, w, anchors_per_loc, ls, gts, gt_ld, gt_off, anchors, alpha, gamma, cls_weight,
                        reg_weight, d_heads, ld, none, NO_IOU, losses, lay, workspace, (hipStream_t)stream);
}

extern "C" int64_t mvx_focal_loss_dir_frames_workspace_bytes(int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc,
                                                             int32_t d_heads_ld) {
    return Layout(n_frames, l, w, anchors_per_loc, d_heads_ld).total(n_frames);
}

extern "C" int mvx_focal_loss_dir_frames(const float *heads, int32_t heads_ld, const float *dir, int32_t dir_ld, int32_t n_frames,
                                         int32_t l, int32_t w, int32_t anchors_per_loc, const int64_t *pos_idx,
                                         const int64_t *neg_idx, const int64_t *gi, int64_t cap, const int32_t *counts,
                                         const float *gts, int32_t gt_ld, const int32_t *gt_off, const float *anchors, float alpha,
                                         float gamma, float cls_weight, float reg_weight, float dir_weight, float dir_offset,
                                         float *d_heads, int32_t d_heads_ld, float *d_dir, int32_t d_dir_ld, float *losses,
                                         void *workspace, int64_t workspace_bytes, void *stream) {
    const Layout lay(n_frames, l, w, anchors_per_loc, d_heads_ld);
    MVX_CHECK_ARG(lay.ok);
    MVX_CHECK_ARG(heads && dir && pos_idx && neg_idx && gi && counts && gts && gt_off && anchors && losses && workspace);
    MVX_CHECK_ARG(heads_ld >= 8 * anchors_per_loc && heads_ld % 4 == 0 && (long long)n_frames * l * w * heads_ld < (1ll << 31));
    MVX_CHECK_ARG(dir_ld >= anchors_per_loc && (long long)n_frames * l * w * dir_ld < (1ll << 31));
    MVX_CHECK_ARG((d_heads == nullptr) == (d_dir == nullptr));
    MVX_CHECK_ARG(!d_dir || (d_dir_ld >= anchors_per_loc && (long long)n_frames * l * w * d_dir_ld < (1ll << 31)));
    MVX_CHECK_ARG(cap >= 1 && cap < (1ll << 31) && gt_ld >= 7);
    MVX_CHECK_ARG(alpha >= 0.f && alpha <= 1.f && gamma >= 0.f && dir_weight >= 0.f && dir_offset == dir_offset);
    MVX_CHECK_ARG(workspace_bytes >= lay.total(n_frames));
    MVX_CHECK_ARG(((uintptr_t)heads & 15) == 0 && ((uintptr_t)d_heads & 15) == 0 && ((uintptr_t)workspace & 7) == 0);
    MVX_CHECK_ARG(((uintptr_t)dir & 3) == 0 && ((uintptr_t)d_dir & 3) == 0);
    const Lists ls = {(const long long *)pos_idx, (const long long *)neg_idx, (const long long *)gi, (long long)cap, counts};
    const Dir d = {dir, d_dir, dir_ld, d_dir_ld, dir_weight, dir_offset};
    return focal_launch(heads, heads_ld, n_frames, l, w, anchors_per_loc, ls, gts, gt_ld, gt_off, anchors, alpha, gamma, cls_weight,
                        reg_weight, d_heads, d_heads_ld, d, NO_IOU, losses, lay, workspace, (hipStream_t)stream);
}

extern "C" int64_t mvx_focal_loss_iou_frames_workspace_bytes(int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc,
                                                             int32_t d_heads_ld, int64_t cap) {
    const Layout lay(n_frames, l, w, anchors_per_loc, d_heads_ld);
    return lay.ok && cap >= 1 ? lay.total(n_frames) + (long long)n_frames * iou_blocks(cap) * (long long)sizeof(double) : 0;
}

extern "C" int mvx_focal_loss_iou_frames(const float *heads, int32_t heads_ld, const float *dir, int32_t dir_ld, const float *iou,
                                         int32_t iou_ld, int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc,
                                         const int64_t *pos_idx, const int64_t *neg_idx, const int64_t *gi, int64_t cap,
                                         const int32_t *counts, const float *gts, int32_t gt_ld, const int32_t *gt_off,
                                         const float *anchors, float alpha, float gamma, float cls_weight, float reg_weight,
                                         float dir_weight, float dir_offset, float iou_weight, float *d_heads, int32_t d_heads_ld,
                                         float *d_dir, int32_t d_dir_ld, float *d_iou, int32_t d_iou_ld, float *q_out, float *losses,
                                         void *workspace, int64_t workspace_bytes, void *stream) {
    const Layout lay(n_frames, l, w, anchors_per_loc, d_heads_ld);
    MVX_CHECK_ARG(lay.ok);
    MVX_CHECK_ARG(heads && dir && iou && pos_idx && neg_idx && gi && counts && gts && gt_off && anchors && losses && workspace);
    MVX_CHECK_ARG(heads_ld >= 8 * anchors_per_loc && heads_ld % 4 == 0 && (long long)n_frames * l * w * heads_ld < (1ll << 31));
    MVX_CHECK_ARG(dir_ld >= anchors_per_loc && (long long)n_frames * l * w * dir_ld < (1ll << 31));
    MVX_CHECK_ARG(iou_ld >= anchors_per_loc && (long long)n_frames * l * w * iou_ld < (1ll << 31));
    MVX_CHECK_ARG((d_heads == nullptr) == (d_dir == nullptr) && (d_heads == nullptr) == (d_iou == nullptr));
    MVX_CHECK_ARG(!d_dir || (d_dir_ld >= anchors_per_loc && (long long)n_frames * l * w * d_dir_ld < (1ll << 31)));
    MVX_CHECK_ARG(!d_iou || (d_iou_ld >= anchors_per_loc && (long long)n_frames * l * w * d_iou_ld < (1ll << 31)));
    MVX_CHECK_ARG(cap >= 1 && cap < (1ll << 31) && gt_ld >= 7 && (!q_out || (long long)n_frames * cap < (1ll << 31)));
    MVX_CHECK_ARG(alpha >= 0.f && alpha <= 1.f && gamma >= 0.f && dir_weight >= 0.f && dir_offset == dir_offset && iou_weight >= 0.f);
    const int nq = iou_blocks(cap);
    MVX_CHECK_ARG(workspace_bytes >= lay.total(n_frames) + (long long)n_frames * nq * (long long)sizeof(double));
    MVX_CHECK_ARG(((uintptr_t)heads & 15) == 0 && ((uintptr_t)d_heads & 15) == 0 && ((uintptr_t)workspace & 7) == 0);
    MVX_CHECK_ARG(((uintptr_t)dir & 3) == 0 && ((uintptr_t)d_dir & 3) == 0 && ((uintptr_t)iou & 3) == 0 && ((uintptr_t)d_iou & 3) == 0 &&
                  ((uintptr_t)q_out & 3) == 0);
    const Lists ls = {(const long long *)pos_idx, (const long long *)neg_idx, (const long long *)gi, (long long)cap, counts};
    const Dir d = {dir, d_dir, dir_ld, d_dir_ld, dir_weight, dir_offset};
    const Iou u = {iou, d_iou, iou_ld, d_iou_ld, iou_weight, q_out, (double *)((unsigned char *)workspace + lay.total(n_frames)), nq};
    return focal_launch(heads, heads_ld, n_frames, l, w, anchors_per_loc, ls, gts, gt_ld, gt_off, anchors, alpha, gamma, cls_weight,
                        reg_weight, d_heads, d_heads_ld, d, u, losses, lay, workspace, (hipStream_t)stream);
}
