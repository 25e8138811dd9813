// Channel-quad helpers of the BatchNorm / glue kernels (bn.hip, vfe.hip, activity.hip, rpn.hip, sparseconv.hip, fusion.hip):
// the arithmetic on one float4 of four neighbouring channels, the fold of per-thread quad sums across a workgroup, and the
// thread -> (site, channel quad) mapping of an 8 x 16-site tile.  The library is built with -ffp-contract=off: every expression
// below rounds exactly as when it is written out at the call site.
#pragma once
#include "common.h"

__device__ __forceinline__ float4 ld4(const float *p) { return *(const float4 *)p; }
__device__ __forceinline__ void st4(float *p, const float4 v) { *(float4 *)p = v; }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// BatchNorm without affine: (y - mean) * inv
__device__ __forceinline__ float bn1(float y, float m, float iv) { return (y - m) * iv; }
__device__ __forceinline__ float4 bn4(const float4 y, const float4 m, const float4 iv) {
    return make_float4(bn1(y.x, m.x, iv.x), bn1(y.y, m.y, iv.y), bn1(y.z, m.z, iv.z), bn1(y.w, m.w, iv.w));
}
// s += v and a * b per component (Q = float4 or double4)
template <typename Q>
__device__ __forceinline__ void acc4(Q &s, const Q v) { s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
template <typename Q>
__device__ __forceinline__ Q mul4(const Q a, const Q b) { Q r; r.x = a.x * b.x; r.y = a.y * b.y; r.z = a.z * b.z; r.w = a.w * b.w; return r; }
// max(mx, max |v|): the operand range the fp16-piece kernels scale by (mvx_wave_amax_to)
__device__ __forceinline__ float amax4(float mx, const float4 v) {
    return fmaxf(fmaxf(mx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
}
// BatchNorm + ReLU backward: dz = (y > 0) ? inv * (g - rw * (a + yhat * b)) : 0 with a = sum g / N, b = sum g yhat / N; rw is the
// number of dense rows a compact row stands for (ROW_W = false: no such weight, the factor is not formed)
template <bool ROW_W>
__device__ __forceinline__ float dz1(float g, float y, float yh, float iv, float a, float b, float rw) {
    const float t = a + yh * b;
    return y > 0.f ? iv * (g - (ROW_W ? rw * t : t)) : 0.f;
}
template <bool ROW_W>
__device__ __forceinline__ float4 dz4(const float4 g, const float4 y, const float4 yh, const float4 iv, const float4 a, const float4 b,
                                      float rw = 1.f) {
    return make_float4(dz1<ROW_W>(g.x, y.x, yh.x, iv.x, a.x, b.x, rw), dz1<ROW_W>(g.y, y.y, yh.y, iv.y, a.y, b.y, rw),
                       dz1<ROW_W>(g.z, y.z, yh.z, iv.z, a.z, b.z, rw), dz1<ROW_W>(g.w, y.w, yh.w, iv.w, a.w, b.w, rw));
}

// ---- the block fold: K quad sums per thread -> one f64 per channel ---------------------------------------------------------
// A workgroup of 256 threads holds, for c4 channel quads, rpi = 256 / c4 partial sums per quad (at least 1; thread = rt * c4 + ct,
// threads with rt >= rpi bring zeros); `col` is the thread's quad in the matrix (ct, plus the column block where C > 1024).  The
// fold hands add(k, channel, sum) the f64 sum of every channel of the quads col < c4, in one of two orders:
//   serial  : the thread rt == 0 of a quad walks its rpi partials in ascending order
//   shuffle : (64 % c4 == 0 only, T = double) __shfl_xor from off = c4 upward inside each wave, then the four wave partials
//             as (w0 + w1) + (w2 + w3).  The serial walk is 64 dependent LDS reads per value at C = 16.
// The order decides the rounding, so every call site keeps the one it was written with.  red: LDS, T [K][256][4].  Ends with a
// barrier (red is free on return) unless REUSE is false: the caller's last use of red, nothing to protect.
template <int K, bool REUSE = true, typename Q, typename T, typename Add>
__device__ __forceinline__ void fold_quads(const Q (&s)[K], T (*red)[256][4], int c4, int rpi, int col, bool shuffle, Add add) {
    const int ct = threadIdx.x % c4, rt = threadIdx.x / c4;
    if (shuffle) {
        double v[K][4];
#pragma unroll
        for (int k = 0; k < K; ++k) { v[k][0] = s[k].x; v[k][1] = s[k].y; v[k][2] = s[k].z; v[k][3] = s[k].w; }
        for (int off = c4; off < 64; off <<= 1)
#pragma unroll
            for (int i = 0; i < 4 * K; ++i) v[i >> 2][i & 3] += __shfl_xor(v[i >> 2][i & 3], off, 64);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane < c4)
#pragma unroll
            for (int i = 0; i < 4 * K; ++i) red[i >> 2][wave * c4 + lane][i & 3] = v[i >> 2][i & 3];
        __syncthreads();
        if ((int)threadIdx.x < c4)
            for (int k = 0; k < K; ++k)
                for (int j = 0; j < 4; ++j)
                    add(k, col * 4 + j, (red[k][ct][j] + red[k][c4 + ct][j]) + (red[k][2 * c4 + ct][j] + red[k][3 * c4 + ct][j]));
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            red[k][threadIdx.x][0] = s[k].x; red[k][threadIdx.x][1] = s[k].y; red[k][threadIdx.x][2] = s[k].z; red[k][threadIdx.x][3] = s[k].w;
        }
        __syncthreads();
        if (rt == 0 && col < c4)
            for (int k = 0; k < K; ++k)
                for (int j = 0; j < 4; ++j) {
                    double t = 0.0;
                    for (int r = 0; r < rpi; ++r) t += (double)red[k][r * c4 + ct][j];
                    add(k, col * 4 + j, t);
                }
    }
    if (REUSE) __syncthreads();
}
// rows (sites) a workgroup of 256 threads takes per trip at C channels: the rpi of fold_quads, host side
static inline int quad_rows_per_trip(int C) { return (256 / (C / 4)) > 1 ? 256 / (C / 4) : 1; }

// ---- thread -> (site, channel quad) of an 8 x 16-site tile (the tile of the convolution kernels), 256 % (C / 4) == 0 -------
constexpr int QTH = 8, QTW = 16;
struct TileThreads {
    int ct, st, spb;        // channel quad; first site of this thread; sites the workgroup takes per trip
    int ty0, tx0;           // the tile's first row and column in the image
    __device__ __forceinline__ TileThreads(int C, int tile, int W) {
        const int c4 = C >> 2;
        ct = threadIdx.x % c4; st = threadIdx.x / c4; spb = 256 / c4;
        at(tile, W);
    }
    __device__ __forceinline__ void at(int tile, int W) {
        const int tiles_x = (W + QTW - 1) / QTW;
        ty0 = (tile / tiles_x) * QTH; tx0 = (tile % tiles_x) * QTW;
    }
    // f(site index in the tile, image row, image column) for every site of the thread, in or outside the image
    template <typename F>
    __device__ __forceinline__ void for_each_site(F f) const {
        for (int sidx = st; sidx < QTH * QTW; sidx += spb) f(sidx, ty0 + sidx / QTW, tx0 + sidx % QTW);
    }
};
