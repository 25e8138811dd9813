// Rotated 3D IoU regression loss, 1 - IoU3D, with its analytic gradient, for all frames of a step in ONE launch (Zhou et al.,
// "IoU Loss for 2D/3D Object Detection", 3DV 2019; SE-SSD's ODIoU; mmdetection3d's RotatedIoU3DLoss).
//
// Reads the head rows and the lists in the layout of mvx_focal_loss_dir_frames (csrc/loss_frames.hip) and is meant to run right
// behind it on the same d_heads.  Per pos_idx entry of frame f (anchor a, box g, the anchor's regression row r), skipped exactly
// as focal_lists / focal_iou skip it (anchor outside the grid, gi outside the frame's boxes), duplicates counted every time:
//   b  = the 'loss' decode: d = sqrt(an3^2 + an4^2), b0,1 = r0,1 d + an0,1, b2 = r2 an5 + an2, b3..5 = expf(r3..5) an3..5,
//        b6 = r6 + an6 (no direction fold: a rectangle is blind to a half turn)
//   ih = min(b2 + b5, g2 + g5) - max(b2, g2)                                                   (z is the bottom face)
//   I  = BEV intersection area, yaw convention of box_quad / Calc.bbox3d2bev (CLOCKWISE: a corner (px, py) of a box lies at
//        (px c + py s, -px s + py c) + (x, y))
//   V = I ih, U = b3 b4 b5 + g3 g4 g5 - V, q = clamp(V / U, 0, 1); q = 0 with a zero gradient when ih <= 0, when b or g is not
//   finite, or when the rectangles do not overlap
//   term_f = weight / max(1, n_pos) * sum (1 - q)
//
// I and its derivative do not come from bev_iou.h: that is the origin-fan clip of the NMS with a 1e-6 tolerance, f32 in world
// coordinates -- fine for thresholding an IoU, not differentiable, and its error grows with the range.  Here:
//   1. the ground truth is expressed in the predicted box's own frame, the centre difference (g0 - b0, g1 - b1) taken FIRST
//      (no cancellation at 70 m), the relative rotation from the angle difference g6 - b6;
//   2. there the predicted box is [-l/2, l/2] x [-w/2, w/2]: Sutherland-Hodgman against its four sides, at most 8 vertices.
//      Every vertex carries the tag of the edge that LEAVES it: an in->out crossing gets the clipping side's tag, an out->in
//      crossing keeps the tag of the edge it cuts;
//   3. I = the shoelace area of the closed polygon (robust when the edges of the two boxes nearly coincide, which is where
//      training converges);
//   4. dI with respect to the predicted box = boundary integrals over the edges tagged with one of ITS sides: for side +-x with
//      piece length s and midpoint (., ym): translation along local x +-s, dl s/2, local rotation -+ym s; likewise for +-y;
//   5. the translation part is rotated back to world coordinates, the rotation part negated (clockwise yaw).
// Chain rule: dq = (dV (U + V) - V d(b3 b4 b5)) / U^2, dV = ih dI + I dih (dih = the indicators of the min / max), then
//   dr0 = d dbx, dr1 = d dby, dr2 = an5 dbz, dr3..5 = b3..5 dbl,w,h, dr6 = dbtheta,
// added with float atomicAdd into the anchor's seven regression columns of d_heads (entries that name the same anchor collide
// there, as in focal_lists); nothing else of d_heads is touched.
//
// One workgroup per frame and a strided loop: a frame has at most a few thousand positives, the launch is latency-bound (read
// from the code, not measured at the time of writing; DESIGN.md 3.36 has the measurement).  The polygon lives in LDS, slot-major
// (two buffers of 8 vertices per thread, 48 KB per workgroup): indexed by a run-time vertex count it would otherwise go to
// scratch (see the note at the top of bev_iou.h).  The frame's sums are f64, reduced in a fixed order: out is bitwise
// reproducible, and so is the gradient whenever no anchor is listed twice.  No workspace, no host read.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_VERTS = 8;

__device__ __forceinline__ int list_count(const int *counts, long long cap, int f, int which) {
    const int n = counts[2 * f + which];
    return n < 0 ? 0 : ((long long)n > cap ? (int)cap : n);
}

// anchor (x, y, z) of entry k of a (3,cap) list -> index inside the frame, or -1 when it lies outside the grid
__device__ __forceinline__ long long list_anchor(const long long *idx, long long cap, int k, int L, int W, int A) {
    const long long x = idx[k], y = idx[cap + k], z = idx[2 * cap + k];
    if (x < 0 || x >= L || y < 0 || y >= W || z < 0 || z >= A) return -1;
    return (x * W + y) * A + z;
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

// A thread's polygon in LDS: vertex k at [k * THREADS] of the three arrays (already offset by the thread index)
struct Poly {
    float *x, *y;
    int *t;
};

// One Sutherland-Hodgman pass.  SIDE 0: x <= h, 1: x >= -h, 2: y <= h, 3: y >= -h.  Returns the vertex count (<= MAX_VERTS: a
// convex polygon gains at most one vertex per pass; the bound is enforced for inputs that are not).
template <int SIDE>
__device__ __forceinline__ int clip_side(const Poly &in, int n, const Poly &out, float h) {
    int m = 0;
    for (int k = 0; k < n; ++k) {
        const int k1 = k + 1 < n ? k + 1 : 0;
        const float px = in.x[k * THREADS], py = in.y[k * THREADS], qx = in.x[k1 * THREADS], qy = in.y[k1 * THREADS];
        const int tp = in.t[k * THREADS];
        const float dp = SIDE == 0 ? h - px : SIDE == 1 ? px + h : SIDE == 2 ? h - py : py + h;
        const float dq = SIDE == 0 ? h - qx : SIDE == 1 ? qx + h : SIDE == 2 ? h - qy : qy + h;
        const bool pin = dp >= 0.f, qin = dq >= 0.f;
        if (pin && m < MAX_VERTS) {
            out.x[m * THREADS] = px;
            out.y[m * THREADS] = py;
            out.t[m * THREADS] = tp;
            ++m;
        }
        if (pin != qin && m < MAX_VERTS) {
            const float u = dp / (dp - dq);
            float cx = px + u * (qx - px), cy = py + u * (qy - py);
            if (SIDE == 0) cx = h;                       // the crossing lies ON the side
            if (SIDE == 1) cx = -h;
            if (SIDE == 2) cy = h;
            if (SIDE == 3) cy = -h;
            out.x[m * THREADS] = cx;
            out.y[m * THREADS] = cy;
            out.t[m * THREADS] = pin ? SIDE : tp;        // in->out: the edge that leaves runs along the side; out->in: the cut edge
            ++m;
        }
    }
    return m;
}

struct Args {
    const float *heads;
    int ld;
    const long long *pos, *gi;      // (F,3,cap), (F,cap)
    long long cap;
    const int *counts;              // (F,2)
    const float *gts;
    int gt_ld;
    const int *gt_off;
    const float *anchors;
    int L, W, A;
    float weight;
    float *d_heads;
    int ldd;
    float *loss_add;
    int loss_add_ld;
    float *out, *q_out;
};

__global__ void __launch_bounds__(THREADS) box_iou_loss(Args p) {
    __shared__ float s_x[2 * MAX_VERTS * THREADS], s_y[2 * MAX_VERTS * THREADS];
    __shared__ int s_t[2 * MAX_VERTS * THREADS];
    __shared__ double s_part[3][THREADS / 64];
    const int f = blockIdx.x;
    const int L = p.L, W = p.W, A = p.A;
    const int n_pos = list_count(p.counts, p.cap, f, 0);
    const long long *pos = p.pos + (size_t)f * 3 * p.cap, *gi = p.gi + (size_t)f * p.cap;
    const int g_lo = p.gt_off[f], n_gt = p.gt_off[f + 1] - g_lo;
    const size_t cell0 = (size_t)f * L * W;
    const float scale = p.weight / (float)(n_pos > 1 ? n_pos : 1);
    const Poly pa = {s_x + threadIdx.x, s_y + threadIdx.x, s_t + threadIdx.x};
    const Poly pb = {s_x + MAX_VERTS * THREADS + threadIdx.x, s_y + MAX_VERTS * THREADS + threadIdx.x,
                     s_t + MAX_VERTS * THREADS + threadIdx.x};
    const long long end = p.q_out ? p.cap : (long long)n_pos;          // q_out is written for every slot of the list
    double s_loss = 0.0, s_q = 0.0, s_n = 0.0;
    for (long long k = threadIdx.x; k < end; k += THREADS) {
        float q = -1.f;
        const long long a = k < n_pos ? list_anchor(pos, p.cap, (int)k, L, W, A) : -1;
        const long long gk = k < n_pos ? gi[k] : -1;
        if (a >= 0 && gk >= 0 && gk < n_gt) {
            const int z = (int)(a % A);
            const float *g = p.gts + (size_t)(g_lo + gk) * p.gt_ld;
            const float *an = p.anchors + (size_t)a * 7;
            const size_t cell = cell0 + (size_t)(a / A);
            const float *r = p.heads + cell * p.ld + A + z * 7;
            const float d = sqrtf(an[3] * an[3] + an[4] * an[4]);
            const float an5 = an[5];
            float b[7], gb[7];
            b[0] = r[0] * d + an[0];
            b[1] = r[1] * d + an[1];
            b[2] = r[2] * an5 + an[2];
            b[3] = expf(r[3]) * an[3];
            b[4] = expf(r[4]) * an[4];
            b[5] = expf(r[5]) * an5;
            b[6] = r[6] + an[6];
            bool ok = true;
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                gb[c] = g[c];
                ok = ok && isfinite(b[c]) && isfinite(gb[c]);
            }
            q = 0.f;
            const float top_b = b[2] + b[5], top_g = gb[2] + gb[5];
            const float ih = fminf(top_b, top_g) - fmaxf(b[2], gb[2]);
            if (ok && ih > 0.f) {
                // the ground truth in the predicted box's frame: centre difference first, then the rotation
                float sb, cb, sd, cd;
                sincosf(b[6], &sb, &cb);
                sincosf(gb[6] - b[6], &sd, &cd);
                const float dx = gb[0] - b[0], dy = gb[1] - b[1];
                const float tx = cb * dx - sb * dy, ty = sb * dx + cb * dy;
                const float ux[4] = {0.5f, -0.5f, -0.5f, 0.5f}, uy[4] = {0.5f, 0.5f, -0.5f, -0.5f};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float px = ux[c] * gb[3], py = uy[c] * gb[4];
                    pa.x[c * THREADS] = (px * cd + py * sd) + tx;
                    pa.y[c * THREADS] = (px * -sd + py * cd) + ty;
                    pa.t[c * THREADS] = 4;                       // an edge of the ground truth: no side of the predicted box
                }
                const float hl = 0.5f * b[3], hw = 0.5f * b[4];
                int n = clip_side<0>(pa, 4, pb, hl);
                n = clip_side<1>(pb, n, pa, hl);
                n = clip_side<2>(pa, n, pb, hw);
                n = clip_side<3>(pb, n, pa, hw);
                // shoelace area and the boundary integrals over the predicted box's sides, in one walk
                float area2 = 0.f, gtx = 0.f, gty = 0.f, gl = 0.f, gw = 0.f, gphi = 0.f;
                for (int c = 0; c < n; ++c) {
                    const int c1 = c + 1 < n ? c + 1 : 0;
                    const float x0 = pa.x[c * THREADS], y0 = pa.y[c * THREADS], x1 = pa.x[c1 * THREADS], y1 = pa.y[c1 * THREADS];
                    const int tag = pa.t[c * THREADS];
                    area2 += x0 * y1 - y0 * x1;
                    if (tag < 2) {                               // a piece of side +x (0) / -x (1)
                        const float s = fabsf(y1 - y0), ym = 0.5f * (y0 + y1);
                        gl += 0.5f * s;
                        gtx += tag == 0 ? s : -s;
                        gphi += tag == 0 ? -ym * s : ym * s;
                    } else if (tag < 4) {                        // a piece of side +y (2) / -y (3)
                        const float s = fabsf(x1 - x0), xm = 0.5f * (x0 + x1);
                        gw += 0.5f * s;
                        gty += tag == 2 ? s : -s;
                        gphi += tag == 2 ? xm * s : -xm * s;
                    }
                }
                const float inter = 0.5f * area2;
                if (n >= 3 && inter > 0.f) {
                    const float vb = b[3] * b[4] * b[5];
                    const float vol = inter * ih;
                    const float uni = vb + gb[3] * gb[4] * gb[5] - vol;
                    const float v = vol / uni;
                    if (isfinite(v) && uni > 0.f) {
                        q = fminf(fmaxf(v, 0.f), 1.f);
                        if (p.d_heads && scale != 0.f) {
                            // d(I) by the box: world translation (rotated back), sizes, yaw (clockwise: the local rotation negated)
                            const float dI[7] = {cb * gtx + sb * gty, -sb * gtx + cb * gty, 0.f, gl, gw, 0.f, -gphi};
                            const float lower = top_b < top_g ? 1.f : 0.f;                       // the min takes b's top face
                            const float dih[7] = {0.f, 0.f, lower - (b[2] > gb[2] ? 1.f : 0.f), 0.f, 0.f, lower, 0.f};
                            const float dvb[7] = {0.f, 0.f, 0.f, b[4] * b[5], b[3] * b[5], b[3] * b[4], 0.f};
                            const float chain[7] = {d, d, an5, b[3], b[4], b[5], 1.f};
                            const float inv_u2 = 1.f / (uni * uni);
                            float *dst = p.d_heads + cell * p.ldd + A + z * 7;
#pragma unroll
                            for (int c = 0; c < 7; ++c) {
                                const float dV = ih * dI[c] + inter * dih[c];
                                const float dq = (dV * (uni + vol) - vol * dvb[c]) * inv_u2;
                                const float gr = -scale * (dq * chain[c]);
                                if (isfinite(gr)) atomicAdd(dst + c, gr);
                            }
                        }
                    }
                }
            }
            s_loss += (double)(1.f - q);
            s_q += (double)q;
            s_n += 1.0;
        }
        if (p.q_out) p.q_out[(size_t)f * p.cap + k] = q;
    }
    const double tl = block_sum_f64(s_loss, s_part[0]);
    const double tq = block_sum_f64(s_q, s_part[1]);
    const double tn = block_sum_f64(s_n, s_part[2]);
    if (threadIdx.x == 0) {
        const float term = (float)((double)p.weight * tl / (double)(n_pos > 1 ? n_pos : 1));
        p.out[2 * f] = term;
        p.out[2 * f + 1] = tn > 0.0 ? (float)(tq / tn) : 0.f;
        if (p.loss_add && p.weight != 0.f) p.loss_add[(size_t)f * p.loss_add_ld] += term;
    }
}

}  // namespace

extern "C" int mvx_box_iou_loss_frames(const float *heads, int32_t heads_ld, int32_t n_frames, int32_t l, int32_t w,
                                       int32_t anchors_per_loc, const int64_t *pos_idx, const int64_t *gi, int64_t cap,
                                       const int32_t *counts, const float *gts, int32_t gt_ld, const int32_t *gt_off,
                                       const float *anchors, float weight, float *d_heads, int32_t d_heads_ld, float *loss_add,
                                       int32_t loss_add_ld, float *out, float *q_out, void *stream) {
    const int A = anchors_per_loc;
    MVX_CHECK_ARG(n_frames >= 1 && n_frames <= MVX_MAX_FRAMES && l > 0 && w > 0 && A >= 1 && A <= 4);
    MVX_CHECK_ARG(heads && pos_idx && gi && counts && gts && gt_off && anchors && out);
    MVX_CHECK_ARG(heads_ld >= 8 * A && heads_ld % 4 == 0 && (long long)n_frames * l * w * heads_ld < (1ll << 31));
    MVX_CHECK_ARG(!d_heads || (d_heads_ld >= 8 * A && (long long)n_frames * l * w * d_heads_ld < (1ll << 31)));
    MVX_CHECK_ARG(cap >= 1 && cap < (1ll << 31) && gt_ld >= 7 && (!q_out || (long long)n_frames * cap < (1ll << 31)));
    MVX_CHECK_ARG(weight >= 0.f);                            // a NaN fails the comparison
    MVX_CHECK_ARG(!loss_add || (loss_add_ld >= 1 && (long long)n_frames * loss_add_ld < (1ll << 31)));
    MVX_CHECK_ARG(((uintptr_t)heads & 15) == 0 && ((uintptr_t)pos_idx & 7) == 0 && ((uintptr_t)gi & 7) == 0);
    MVX_CHECK_ARG(((uintptr_t)counts & 3) == 0 && ((uintptr_t)gts & 3) == 0 && ((uintptr_t)gt_off & 3) == 0 &&
                  ((uintptr_t)anchors & 3) == 0 && ((uintptr_t)d_heads & 3) == 0 && ((uintptr_t)loss_add & 3) == 0 &&
                  ((uintptr_t)out & 3) == 0 && ((uintptr_t)q_out & 3) == 0);
    const Args p = {heads, heads_ld, (const long long *)pos_idx, (const long long *)gi, (long long)cap, counts, gts, gt_ld, gt_off,
                    anchors, l, w, A, weight, d_heads, d_heads_ld, loss_add, loss_add_ld, out, q_out};
    hipLaunchKernelGGL(box_iou_loss, dim3(n_frames), dim3(THREADS), 0, (hipStream_t)stream, p);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}
