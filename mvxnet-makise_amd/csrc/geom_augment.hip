// Geometric augmentation for the frames of a step (VoxelNet section 3.2 plus the flip of the common MVX-Net recipes): per-object
// noise with a collision test, then global rotation, scaling and y flip, then the range filter.  The host draws every random
// number; the kernels are deterministic functions of their inputs (no float atomics: two runs are bitwise identical).
//
//   1. geom_place   (one workgroup per frame, box tables in LDS): the boxes in index order; for box i the T trials in parallel
//                   -- the moved quad of every trial against every other box (j < i in its moved pose, j > i in its original
//                   one) by bev_iou.h's clipping, pairs whose bounding circles cannot touch counting as 0 -- the first trial
//                   whose largest IoU does not exceed iou_thr is taken (LDS integer atomicMin), none: the box keeps its pose.
//                   Then the global step on every box, the centre filter and the ordered compaction (one wave).
//   2. geom_count   (grid (block of 256 points, frame), one thread per point): membership in the ORIGINAL boxes (box3d.h,
//                   lowest index wins), the per-object move, the global step, the range test; kept points per block.
//   3. geom_write   (same grid): the same arithmetic again, the block's offset = the sum of the counts of the blocks before it,
//                   the rank inside the block (compact.h), rows stored in order with 16-byte accesses where the 24-byte rows allow.
// Coordinates are computed in f64 from the f32 inputs and rounded to f32 once; every decision on a stored value (range test,
// box filter) is taken on the rounded f32 value, so what is kept is inside the range as stored.
#include "bev_iou.h"
#include "box3d.h"
#include "compact.h"

namespace {

constexpr int PLACE_THREADS = 128;          // 40 polygon slots of 8 B per thread: 40 KB of LDS
constexpr int PT_THREADS = 256;
constexpr int MAXB = MVX_GT_PASTE_MAX_BOXES, MAXT = MVX_GEOM_MAX_TRIALS;
constexpr double PI = 3.14159265358979323846;

// q = p @ R(a) of Calc.getRotationMatrices: R(a) = [[c, -s], [s, c]] on row vectors
__device__ __forceinline__ void rot(double px, double py, double c, double s, double &qx, double &qy) {
    qx = px * c + py * s;
    qy = -px * s + py * c;
}

// Calc.bbox3d2bev: corners (+,+), (-,+), (-,-), (+,-) of (l, w) / 2, @ R(r) + centre; f64, rounded to f32 once
__device__ void quad_of(double x, double y, double l, double w, double r, float *q) {
    const double c = cos(r), s = sin(r);
    const double hx[4] = {0.5, -0.5, -0.5, 0.5}, hy[4] = {0.5, 0.5, -0.5, -0.5};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double qx, qy;
        rot(hx[k] * l, hy[k] * w, c, s, qx, qy);
        q[2 * k] = (float)(qx + x);
        q[2 * k + 1] = (float)(qy + y);
    }
}

struct Glob { double c, s, scale; bool flip; };

__device__ __forceinline__ Glob load_glob(const float *g) {
    Glob o;
    o.c = cos((double)g[0]); o.s = sin((double)g[0]); o.scale = (double)g[1]; o.flip = g[2] != 0.f;
    return o;
}

// the global step on a point: p_xy <- s (p_xy @ R(phi)), p_z <- s p_z, then the flip of y
__device__ __forceinline__ void global_step(const Glob &g, double &x, double &y, double &z) {
    double qx, qy;
    rot(x, y, g.c, g.s, qx, qy);
    x = g.scale * qx;
    y = g.scale * qy;
    z = g.scale * z;
    if (g.flip) y = -y;
}

struct Range6 { double lo[3], hi[3]; };

// 1. -------------------------------------------------------------------------------------------------------------------
struct PlaceArgs {
    const float *box3d;          // [F][B][7]
    const int *n_box;            // [F]
    const float *noise;          // [F][B][T][4]
    const float *glob;           // [F][4]
    int B, T;
    float iou_thr;
    Range6 r;
    int *trial;                  // [F][B]
    float *move;                 // [F][B][4]
    float *out_box3d, *out_bev;  // [F][B][7], [F][B][4][2]
    int *kept_idx, *n_kept, *status;
};

__global__ __launch_bounds__(PLACE_THREADS) void geom_place(PlaceArgs a) {
    __shared__ P2 s_poly[POLY_SLOTS * PLACE_THREADS];
    __shared__ float s_b3[MAXB][7], s_quad[MAXB][8], s_circ[MAXB][3], s_move[MAXB][4];
    __shared__ float c_quad[MAXT][8], c_circ[MAXT][3], s_iou[MAXT][MAXB];
    __shared__ int s_trial[MAXB], s_win;
    const int f = blockIdx.x, tid = threadIdx.x, B = a.B, T = a.T;
    const float *g_b3 = a.box3d + (size_t)f * B * 7, *g_noise = a.noise + (size_t)f * B * T * 4;
    int n = a.n_box[f];
    const bool bad = n < 0 || n > B;
    if (bad) n = 0;
    for (int i = tid; i < n; i += PLACE_THREADS) {
#pragma unroll
        for (int k = 0; k < 7; ++k) s_b3[i][k] = g_b3[i * 7 + k];
        quad_of((double)s_b3[i][0], (double)s_b3[i][1], (double)s_b3[i][3], (double)s_b3[i][4], (double)s_b3[i][6], s_quad[i]);
        circle_of(s_quad[i], s_circ[i]);
#pragma unroll
        for (int k = 0; k < 4; ++k) s_move[i][k] = 0.f;
        s_trial[i] = -1;
    }
    __syncthreads();
    const Polys w = polys_of(s_poly, PLACE_THREADS, tid);
    for (int i = 0; i < n; ++i) {
        // ---- the T trial poses of box i
        if (tid < T) {
            const float *nz = g_noise + ((size_t)i * T + tid) * 4;
            quad_of((double)s_b3[i][0] + (double)nz[0], (double)s_b3[i][1] + (double)nz[1], (double)s_b3[i][3], (double)s_b3[i][4],
                    (double)s_b3[i][6] + (double)nz[3], c_quad[tid]);
            circle_of(c_quad[tid], c_circ[tid]);
        }
        if (tid == 0) s_win = MAXT;
        __syncthreads();
        // ---- pairs (trial t, other box j): the moved boxes j < i are already in s_quad
        for (int p = tid; p < T * n; p += PLACE_THREADS) {
            const int t = p / n, j = p - t * n;
            float iou = 0.f;
            const P2 c1 = {c_circ[t][0], c_circ[t][1]}, c2 = {s_circ[j][0], s_circ[j][1]};
            if (j != i && !circles_apart(c1, c_circ[t][2], c2, s_circ[j][2])) iou = quad_iou(w, c_quad[t], s_quad[j]);
            s_iou[t][j] = iou;
        }
        __syncthreads();
        if (tid < T) {
            float m = 0.f;
            for (int j = 0; j < n; ++j) m = fmaxf(m, s_iou[tid][j]);
            if (!(m > a.iou_thr)) atomicMin(&s_win, tid);
        }
        __syncthreads();
        const int win = s_win;
        if (win < MAXT) {
            if (tid < 8) s_quad[i][tid] = c_quad[win][tid];
            if (tid >= 8 && tid < 11) s_circ[i][tid - 8] = c_circ[win][tid - 8];
            if (tid >= 16 && tid < 20) s_move[i][tid - 16] = g_noise[((size_t)i * T + win) * 4 + tid - 16];
            if (tid == 0) s_trial[i] = win;
        }
        __syncthreads();
    }
    // ---- the chosen trials and moves of all B slots
    for (int i = tid; i < B; i += PLACE_THREADS) {
        a.trial[(size_t)f * B + i] = i < n ? s_trial[i] : -1;
#pragma unroll
        for (int k = 0; k < 4; ++k) a.move[((size_t)f * B + i) * 4 + k] = i < n ? s_move[i][k] : 0.f;
    }
    // ---- global step, centre filter, ordered compaction: wave 0, one box per lane (B <= 32)
    if (tid < MVX_WAVE) {
        const Glob g = load_glob(a.glob + (size_t)f * 4);
        float o[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        bool keep = false;
        if (tid < n) {
            double x = (double)s_b3[tid][0] + (double)s_move[tid][0], y = (double)s_b3[tid][1] + (double)s_move[tid][1];
            double z = (double)s_b3[tid][2] + (double)s_move[tid][2];
            global_step(g, x, y, z);
            double r = (double)s_b3[tid][6] + (double)s_move[tid][3] + (double)a.glob[(size_t)f * 4];
            if (g.flip) r = -r;
            r -= 2.0 * PI * floor((r + PI) / (2.0 * PI));          // into [-pi, pi)
            o[0] = (float)x; o[1] = (float)y; o[2] = (float)z;
#pragma unroll
            for (int k = 3; k < 6; ++k) o[k] = (float)(g.scale * (double)s_b3[tid][k]);
            o[6] = (float)r;
            keep = (double)o[0] >= a.r.lo[0] && (double)o[0] < a.r.hi[0] && (double)o[1] >= a.r.lo[1] && (double)o[1] < a.r.hi[1];
        }
        int total;
        const int at = block_kept_rank<1>(keep, nullptr, total);
        if (keep) {
            float *d3 = a.out_box3d + ((size_t)f * B + at) * 7, *dq = a.out_bev + ((size_t)f * B + at) * 8;
            float q[8];
            quad_of((double)o[0], (double)o[1], (double)o[3], (double)o[4], (double)o[6], q);
#pragma unroll
            for (int k = 0; k < 7; ++k) d3[k] = o[k];
#pragma unroll
            for (int k = 0; k < 8; ++k) dq[k] = q[k];
            a.kept_idx[(size_t)f * B + at] = tid;
        }
        if (tid >= total && tid < B) a.kept_idx[(size_t)f * B + tid] = -1;
        if (tid == 0) {
            a.n_kept[f] = total;
            if (bad) atomicOr(a.status + f, MVX_GEOM_BAD_COUNT);
        }
    }
}

// 2 / 3. ---------------------------------------------------------------------------------------------------------------
struct PointArgs {
    const float *in;             // [F][cap][6]
    const int *n_in;             // [F]
    int cap;
    const float *box3d;          // [F][B][7]  the ORIGINAL boxes
    const int *n_box, *trial;    // [F], [F][B]
    const float *move;           // [F][B][4]
    const float *glob;           // [F][4]
    int B;
    Range6 r;
    int n_blocks;
    int *block_cnt;              // [F][n_blocks]
    float *out;                  // [F][cap][6]
    int *n_out;                  // [F]
};

struct Move { double c, s, dx, dy, dz; int on; };

struct Tables {
    Box box[MAXB];
    Move mv[MAXB];
    Glob g;
    int n;
};

__device__ void load_tables(const PointArgs &a, int f, Tables &t) {
    const int tid = threadIdx.x;
    int n = a.n_box[f];
    if (n < 0 || n > a.B) n = 0;
    if (tid < n) {
        const float *b3 = a.box3d + ((size_t)f * a.B + tid) * 7, *m = a.move + ((size_t)f * a.B + tid) * 4;
        t.box[tid] = load_box(b3, cos((double)b3[6]), sin((double)b3[6]));
        Move v;
        v.on = a.trial[(size_t)f * a.B + tid] >= 0;
        v.dx = (double)m[0]; v.dy = (double)m[1]; v.dz = (double)m[2];
        v.c = cos((double)m[3]); v.s = sin((double)m[3]);
        t.mv[tid] = v;
    }
    if (tid == PT_THREADS - 1) { t.g = load_glob(a.glob + (size_t)f * 4); t.n = n; }
    __syncthreads();
}

// rows of 24 B: a row whose index in the whole (16-byte aligned) buffer is even starts on 16 bytes, an odd one ends on them
struct Row { float v[6]; };

__device__ __forceinline__ Row load_row(const float *base, size_t row) {
    const float *p = base + row * 6;
    Row r;
    if (row & 1) {
        const float2 a = *(const float2 *)p;
        const float4 b = *(const float4 *)(p + 2);
        r.v[0] = a.x; r.v[1] = a.y; r.v[2] = b.x; r.v[3] = b.y; r.v[4] = b.z; r.v[5] = b.w;
    } else {
        const float4 a = *(const float4 *)p;
        const float2 b = *(const float2 *)(p + 4);
        r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w; r.v[4] = b.x; r.v[5] = b.y;
    }
    return r;
}

__device__ __forceinline__ void store_row(float *base, size_t row, const Row &r) {
    float *p = base + row * 6;
    if (row & 1) {
        *(float2 *)p = make_float2(r.v[0], r.v[1]);
        *(float4 *)(p + 2) = make_float4(r.v[2], r.v[3], r.v[4], r.v[5]);
    } else {
        *(float4 *)p = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
        *(float2 *)(p + 4) = make_float2(r.v[4], r.v[5]);
    }
}

// per-object move, global step, rounding, range test: the row's x y z are replaced, the answer is "kept"
__device__ bool transform(const Tables &t, const Range6 &rg, Row &r) {
    double x = (double)r.v[0], y = (double)r.v[1], z = (double)r.v[2];
    int owner = -1;
    for (int i = 0; i < t.n; ++i)
        if (inside(t.box[i], x, y, z)) { owner = i; break; }          // the lowest box index owns the point
    if (owner >= 0 && t.mv[owner].on) {
        const Box &b = t.box[owner];
        const Move &m = t.mv[owner];
        double qx, qy;
        rot(x - b.x, y - b.y, m.c, m.s, qx, qy);
        x = qx + b.x + m.dx;
        y = qy + b.y + m.dy;
        z = z + m.dz;
    }
    global_step(t.g, x, y, z);
    r.v[0] = (float)x; r.v[1] = (float)y; r.v[2] = (float)z;
    bool keep = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) keep = keep && (double)r.v[k] >= rg.lo[k] && (double)r.v[k] < rg.hi[k];      // a NaN is dropped
    return keep;
}

__global__ __launch_bounds__(PT_THREADS) void geom_count(PointArgs a) {
    __shared__ Tables t;
    __shared__ int s_cnt[PT_THREADS / MVX_WAVE];
    const int blk = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const int n = min(max(a.n_in[f], 0), a.cap);
    int total = 0;
    if (blk * PT_THREADS < n) {                                        // block-uniform
        load_tables(a, f, t);
        const int p = blk * PT_THREADS + tid;
        bool keep = false;
        if (p < n) {
            Row r = load_row(a.in, (size_t)f * a.cap + p);
            keep = transform(t, a.r, r);
        }
        total = block_kept_count<PT_THREADS / MVX_WAVE>(keep, s_cnt);
    }
    if (tid == 0) a.block_cnt[(size_t)f * a.n_blocks + blk] = total;
}

__global__ __launch_bounds__(PT_THREADS) void geom_write(PointArgs a) {
    __shared__ Tables t;
    __shared__ int s_cnt[PT_THREADS / MVX_WAVE], s_part[PT_THREADS / MVX_WAVE];
    const int blk = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = min(max(a.n_in[f], 0), a.cap);
    // the blocks before this one (block 0 sums them all: the frame's new count)
    const int *cnt = a.block_cnt + (size_t)f * a.n_blocks;
    const int upto = blk == 0 ? a.n_blocks : blk;
    int part = 0;
    for (int k = tid; k < upto; k += PT_THREADS) part += cnt[k];
    part = wave_sum_i32(part);
    if (lane == 0) s_part[wv] = part;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < PT_THREADS / MVX_WAVE; ++k) before += s_part[k];
    if (blk == 0) {
        if (tid == 0) a.n_out[f] = before;
        before = 0;
    }
    if (blk * PT_THREADS >= n) return;                                 // block-uniform
    load_tables(a, f, t);
    const int p = blk * PT_THREADS + tid;
    bool keep = false;
    Row r;
    if (p < n) {
        r = load_row(a.in, (size_t)f * a.cap + p);
        keep = transform(t, a.r, r);
    }
    int kept;
    const int dst = before + block_kept_rank<PT_THREADS / MVX_WAVE>(keep, s_cnt, kept);
    if (keep && dst < a.cap) store_row(a.out, (size_t)f * a.cap + dst, r);
}

inline bool range_ok(const double *r) {
    for (int k = 0; k < 3; ++k)
        if (!(r[k + 3] > r[k])) return false;
    return true;
}

}  // namespace

extern "C" size_t mvx_geom_workspace_bytes(int32_t n_frames, int32_t cap_points) {
    const size_t F = n_frames > 0 ? n_frames : 0, nb = cap_points > 0 ? mvx_cdiv(cap_points, PT_THREADS) : 0;
    return (F * nb * sizeof(int32_t) + 255) & ~(size_t)255;
}

extern "C" int mvx_geom_place_frames(const float *box3d, const int32_t *n_box, int32_t n_frames, int32_t cap_boxes, const float *noise,
                                     int32_t n_trials, const float *glob, float iou_thr, const double *range6_host, int32_t *trial,
                                     float *move, float *out_box3d, float *out_bev, int32_t *kept_idx, int32_t *n_kept,
                                     int32_t *status, void *stream) {
    MVX_CHECK_ARG(n_frames >= 1 && n_frames <= MVX_MAX_FRAMES);
    MVX_CHECK_ARG(cap_boxes >= 1 && cap_boxes <= MVX_GT_PASTE_MAX_BOXES && n_trials >= 1 && n_trials <= MVX_GEOM_MAX_TRIALS);
    MVX_CHECK_ARG(box3d && n_box && noise && glob && range6_host && trial && move && out_box3d && out_bev && kept_idx && n_kept && status);
    MVX_CHECK_ARG(out_box3d != box3d && iou_thr >= 1e-3f && iou_thr < 1.f && range_ok(range6_host));
    PlaceArgs a = {box3d, n_box, noise, glob, cap_boxes, n_trials, iou_thr, {}, trial, move, out_box3d, out_bev, kept_idx, n_kept, status};
    for (int k = 0; k < 3; ++k) { a.r.lo[k] = range6_host[k]; a.r.hi[k] = range6_host[k + 3]; }
    hipLaunchKernelGGL(geom_place, dim3(n_frames), dim3(PLACE_THREADS), 0, (hipStream_t)stream, a);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_geom_points_frames(const float *points6, const int32_t *n_points, int32_t n_frames, int32_t cap_points,
                                      const float *box3d, const int32_t *n_box, int32_t cap_boxes, const int32_t *trial,
                                      const float *move, const float *glob, const double *range6_host, float *out_points6,
                                      int32_t *n_points_out, void *workspace, size_t workspace_bytes, void *stream) {
    MVX_CHECK_ARG(n_frames >= 1 && n_frames <= MVX_MAX_FRAMES && cap_points >= 1 && cap_points < (1 << 26));
    MVX_CHECK_ARG(cap_boxes >= 1 && cap_boxes <= MVX_GT_PASTE_MAX_BOXES);
    MVX_CHECK_ARG(points6 && n_points && box3d && n_box && trial && move && glob && range6_host && out_points6 && n_points_out && workspace);
    MVX_CHECK_ARG(out_points6 != points6 && n_points_out != n_points && range_ok(range6_host));
    MVX_CHECK_ARG(((uintptr_t)points6 & 15) == 0 && ((uintptr_t)out_points6 & 15) == 0 && ((uintptr_t)workspace & 3) == 0);
    MVX_CHECK_ARG(workspace_bytes >= mvx_geom_workspace_bytes(n_frames, cap_points));
    const int nb = (int)mvx_cdiv(cap_points, PT_THREADS);
    PointArgs a = {points6, n_points, cap_points, box3d, n_box, trial, move, glob, cap_boxes, {}, nb, (int *)workspace, out_points6,
                   n_points_out};
    for (int k = 0; k < 3; ++k) { a.r.lo[k] = range6_host[k]; a.r.hi[k] = range6_host[k + 3]; }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(geom_count, dim3(nb, n_frames), dim3(PT_THREADS), 0, st, a);
    MVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(geom_write, dim3(nb, n_frames), dim3(PT_THREADS), 0, st, a);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}
