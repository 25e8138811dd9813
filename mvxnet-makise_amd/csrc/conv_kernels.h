// Device code that the exact-f32 convolution kernels and their split-arithmetic forms share, one place per decision: the tile
// plan of the background rewrite (tile_plan, plan_stage), the gather epilogue (gather_epilogue) and the step walk of the
// eight-wave weight gradient (W4Walk, w4_slots, w4_store_slabs).  LDS staging, the K loop and its MFMAs stay with each kernel.
// Unnamed namespace and __forceinline__ like conv_geom.h: every including file gets its own copy, inlined into its kernels.
#pragma once
#include "conv_geom.h"
#include "split_common.h"

namespace {

// ---- tile plan of one gather unit (block-uniform) -------------------------------------------------------
struct TilePlan {
    int kd[3], ds[3], nk;       // the nk executed depth taps and their source planes, ascending
    unsigned skipped;           // bit kd: the tap was not executed and contributes its bg_tap constant instead
    bool active;                // false: a background tile, every site is the plane's constant
    bool idle_border;           // border tile without any active source site: filled from the nine bg_cls position classes
};

// Output plane d (global) of a unit that covers NT 8 x 16 tiles (t0, and t1 if NT == 2: their activity flags are ORed --
// computing a background half is exact, just not needed); `on_border`: the unit touches the image border.
// in_hflag[plane][tile] != 0: the tile's halo in that source plane holds a non-background site (activity.hip); null: no
// background description, every valid tap is executed.
// border_active bit 0: tiles on the image border always count as active (zero padding is not the background);
// bit 1: bg_pre is followed by per-depth-tap constants bg_tap[plane][kd][cout] -- in an INTERIOR tile a depth tap whose
// source halo holds no active site contributes exactly that constant (every source site is the plane's background
// value and the window stays inside the image), so it is not executed.  A BORDER tile without any active source site is not
// convolved either: its sites are the plane's background inside and, on the outermost ring, the background minus the taps
// that fall into the zero padding -- nine per-(plane, channel) constants by position class (bg_cls, after bg_tap).
// The list is filled and read by select chains: a runtime-indexed array would go to scratch.
template <int NT>
__device__ __forceinline__ TilePlan tile_plan(const Geom &g, const int d, const bool on_border,
                                              const int *__restrict__ in_hflag, const int border_active, const int ntiles,
                                              const int t0, const int t1) {
    TilePlan p{{0, 0, 0}, {0, 0, 0}, 0, 0u, true, false};
    const bool skip_taps = in_hflag && (border_active & 2) && !on_border;
    int any_flag = 0;
#pragma unroll
    for (int kd = 0; kd < 3; ++kd) {
        const int ds = src_depth(g, d, kd);
        if (ds >= 0) {
            int fl = 1;
            if (in_hflag) {
                fl = in_hflag[(size_t)ds * ntiles + t0];
                if (NT == 2) fl |= in_hflag[(size_t)ds * ntiles + t1];
            }
            any_flag |= fl;
            if (skip_taps && !fl) { p.skipped |= 1u << kd; continue; }
            if (p.nk == 0) { p.kd[0] = kd; p.ds[0] = ds; }
            else if (p.nk == 1) { p.kd[1] = kd; p.ds[1] = ds; }
            else { p.kd[2] = kd; p.ds[2] = ds; }
            ++p.nk;
        }
    }
    p.idle_border = in_hflag && (border_active & 2) && on_border && !any_flag;
    if (p.idle_border) p.nk = 0;
    // Background tiles (see activity.hip): no non-background source site in the halo of any depth tap and the
    // window never leaves the image -> every output site of the tile is the per-plane constant.
    if (in_hflag) p.active = (((border_active & 1) && on_border) || any_flag) != 0;
    return p;
}

// stage st of the K loop = (executed depth tap) x (channel chunk): its tap, source plane and chunk
__device__ __forceinline__ void plan_stage(const TilePlan &p, const int nchunks, const int st, int &kd, int &ds, int &cc) {
    const int i = st / nchunks;
    cc = st - i * nchunks;
    // every member is read before the choice: a choice between member ADDRESSES kept the plan in scratch memory
    const int k0 = p.kd[0], k1 = p.kd[1], k2 = p.kd[2], s0 = p.ds[0], s1 = p.ds[1], s2 = p.ds[2];
    kd = i == 0 ? k0 : (i == 1 ? k1 : k2);
    ds = i == 0 ? s0 : (i == 1 ? s1 : s2);
}

// ---- gather epilogue: bias, skipped-tap and idle-border constants, ReLU, store, BatchNorm statistics -------
//   acc[m][0 / 1]: accumulator tiles of wave wv -- site tile m = patch rows 2 MT wv + 2 m, + 1 of the unit at (tx0, ty0) of
//                  plane d, output channels nb * BNW + lane and + 32;
//   MT  : site tiles per wave (1: 8 x 16-site unit, 2: 16 x 16);
//   NB2 : 32-channel tiles per wave that exist -- 2: BNW = 64; 1: the narrow 32-channel unit, acc[m][1] is not stored;
//   S   : type of a lane's partial sums and of the wave-reduction scratch s_red[4][2 BN] (the caller's LDS, free by now).
//         double: f64 from the first addition on -- var = E[y^2] - mean^2 cancels, and f32 partial sums cost mean^2 / var
//         times their 1e-7 in the variance (the reference's torch-CPU BatchNorm accumulates in double too); float: f32
//         partials per lane, f64 across the waves;
//   unit: index of the unit in its launch, spreads the f64 atomics over the MVX_REP replicas of stats.
// The order of the floating-point operations of an output element and of a partial sum is part of the contract: results
// are compared bit for bit across unit shapes and library versions.
template <int MT, int NB2, typename S>
__device__ __forceinline__ void gather_epilogue(f32x16 (&acc)[MT][2], const TilePlan &p, const Geom &g, const int d,
                                                const int nb, const int tx0, const int ty0, const unsigned unit,
                                                S (*s_red)[2 * BN], const float *__restrict__ bias,
                                                float *__restrict__ out, double *__restrict__ stats, const int relu,
                                                const unsigned char *__restrict__ out_mask,
                                                const float *__restrict__ bg_pre) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lh = lane >> 5;
    constexpr int BNW = 32 * NB2;                    // output channels of this unit
    const int n0 = nb * BNW + li, n1 = NB2 == 2 ? n0 + 32 : n0;      // narrow unit: the second channel tile does not exist
    const float bias0 = bias ? bias[n0] : 0.f, bias1 = bias ? bias[n1] : 0.f;
    float skip0 = 0.f, skip1 = 0.f;            // constants of the depth taps that were not executed
    if (p.skipped && p.active) {
        const float *bg_tap = bg_pre + (size_t)g.Dout * g.F * g.Cout + (size_t)d * 3 * g.Cout;
#pragma unroll
        for (int kd = 0; kd < 3; ++kd)
            if ((p.skipped >> kd) & 1u) { skip0 += bg_tap[kd * g.Cout + n0]; skip1 += bg_tap[kd * g.Cout + n1]; }
    }
    // background value of this plane: the same fp32 operations as a computed site, on the constant
    float bgv0 = (bg_pre ? bg_pre[(size_t)d * g.Cout + n0] : 0.f) + bias0, bgv1 = (bg_pre ? bg_pre[(size_t)d * g.Cout + n1] : 0.f) + bias1;
    if (relu) { bgv0 = fmaxf(bgv0, 0.f); bgv1 = fmaxf(bgv1, 0.f); }
    S s1a = 0, s2a = 0, s1b = 0, s2b = 0;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int py = ty0 + 2 * MT * wv + 2 * m;       // first of this site tile's two patch rows
        if (p.idle_border) {                            // the accumulators are still zero: they take the position-class constants
            const float *bg_cls = bg_pre + (size_t)4 * g.Dout * g.F * g.Cout + (size_t)d * 9 * g.Cout;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = mfma32_row(r) + 4 * lh;
                const int gy = py + (row >> 4), gx = tx0 + (row & 15);
                const int q = 3 * (gy == 0 ? 0 : (gy >= g.H - 1 ? 2 : 1)) + (gx == 0 ? 0 : (gx >= g.W - 1 ? 2 : 1));
                acc[m][0][r] = bg_cls[q * g.Cout + n0];
                acc[m][1][r] = bg_cls[q * g.Cout + n1];
            }
        }
        // the 16 site-mask bytes of this lane are fetched up front, unconditionally from clamped coordinates: a load between the
        // stores (vector-memory operations return in order) made every store pair wait for the previous one to complete
        unsigned site_on = p.active ? 0xffffu : 0u;     // bit r: site r is a computed (non-background) site
        if (out_mask && p.active) {
            unsigned char mk[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = mfma32_row(r) + 4 * lh;
                const int gy = min(py + (row >> 4), g.H - 1), gx = min(tx0 + (row & 15), g.W - 1);
                mk[r] = out_mask[((size_t)d * g.H + gy) * g.W + gx];
            }
            site_on = 0u;
#pragma unroll
            for (int r = 0; r < 16; ++r) site_on |= (mk[r] ? 1u : 0u) << r;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mfma32_row(r) + 4 * lh;
            const int gy = py + (row >> 4), gx = tx0 + (row & 15);
            float v0 = (acc[m][0][r] + skip0) + bias0, v1 = (acc[m][1][r] + skip1) + bias1;
            if (relu) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }
            // a background SITE holds the constant bit for bit, also inside a computed tile
            if (out_mask && !((site_on >> r) & 1u)) { v0 = bgv0; v1 = bgv1; }
            if (gy < g.H && gx < g.W) {                 // ragged right / bottom edge
                float *o = out + (((size_t)d * g.H + gy) * g.W + gx) * g.Cout;
                o[n0] = v0;
                if (NB2 == 2) o[n1] = v1;
                s1a += (S)v0; s2a += (S)v0 * (S)v0;
                s1b += (S)v1; s2b += (S)v1 * (S)v1;
            }
        }
    }
    if (stats) {
        s1a += __shfl_xor(s1a, 32, 64); s2a += __shfl_xor(s2a, 32, 64);
        s1b += __shfl_xor(s1b, 32, 64); s2b += __shfl_xor(s2b, 32, 64);
        __syncthreads();
        if (lh == 0) {
            s_red[wv][li] = s1a; s_red[wv][32 + li] = s1b;
            s_red[wv][BN + li] = s2a; s_red[wv][BN + 32 + li] = s2b;
        }
        __syncthreads();
        if (tid < 2 * BNW) {
            const int which = tid / BNW, c = tid % BNW, j = which * BN + c;
            const double t = (double)s_red[0][j] + (double)s_red[1][j] + (double)s_red[2][j] + (double)s_red[3][j];
            const unsigned rep = unit % MVX_REP;
            double *fstats = stats + (size_t)(d / g.Dout) * MVX_REP * 2 * g.Cout;       // the plane's frame
            atomicAdd(fstats + ((size_t)rep * 2 + which) * g.Cout + nb * BNW + c, t);
        }
    }
}

// ---- eight-wave weight gradient (conv3d_wgrad4, conv3d_wgrad4s): one workgroup per (strip, depth tap kd x 64-channel chunk
// cc of the input, 64-channel block of dz), (m, n) in 2 x 2 waves over a 64(c) x 64(n) block of dW, times two tap groups
struct Strips { int n[3]; };       // workgroups (strips) per depth tap in list mode
constexpr int W4_THREADS = 512;
constexpr int W4_C = 64;               // input channels per workgroup
constexpr int W4_NX = (HH * HW * 16 + W4_THREADS - 1) / W4_THREADS;    // float4 per thread and step, halo (64 channels)
constexpr int W4_NZ = TH * TW * 16 / W4_THREADS;                       // float4 per thread and step, dz

// tap OWNED (written) by slot i of a tap group (-1: none); the first w4_ncomp() slots are computed, the rest stay zero
__host__ __device__ constexpr int w4_own(bool t2, int grp, int i) {
    return t2 ? (grp == 0 ? (i < 3 ? i : i + 2) : (i < 2 ? i + 3 : (i < 4 ? i + 5 : -1)))      // {0,1,2,5,6} / {3,4,7,8}
              : (grp == 0 ? i : (i < 4 ? i + 5 : -1));                                         // {0,1,2,3,4} / {5,6,7,8}
}
__host__ __device__ constexpr int w4_ncomp(bool t2, int grp) { return t2 ? 2 : (grp == 0 ? 5 : 4); }

// Steps of a workgroup: (output plane d with a valid source plane for kd) x (tile).
// Dense (no step_list): the strip's contiguous range of `tiles_per_strip` tiles for every valid plane, the whole grid for
// every depth tap.  With a background description the steps whose source halo holds a non-background site were compacted
// into step_list[kd][] (everywhere else x - c is exactly zero) and are dealt round-robin to the strips: balanced and
// deterministic; each tap gets a share of the workgroups proportional to its number of valid planes (conv3: 1 / 2 / 1).
struct W4Walk {
    int tiles_x, ntiles, kd, cc, strip, nstrips;
    int dlo, per, nsteps;
    const int *list;

    // false: this workgroup has no strip of its depth tap
    __device__ __forceinline__ bool init(const Geom &g, const int tiles_per_strip, const int *__restrict__ step_list,
                                         const int *__restrict__ step_count, const Strips &ks) {
        tiles_x = (g.W + TW - 1) / TW;
        ntiles = tiles_x * ((g.H + TH - 1) / TH);
        const int nchunks = g.Cin / W4_C;
        kd = blockIdx.y / nchunks, cc = blockIdx.y % nchunks;
        strip = blockIdx.x, nstrips = step_list ? (kd == 0 ? ks.n[0] : (kd == 1 ? ks.n[1] : ks.n[2])) : (int)gridDim.x;
        if (strip >= nstrips) return false;
        int dhi = -1;                                    // valid output planes form a contiguous range
        dlo = 0;
        for (int d = 0; d < g.Dout; ++d) {
            const int ds = d * g.sd - g.pd + kd;
            if (ds >= 0 && ds < g.Din) { if (dhi < 0) dlo = d; dhi = d; }
        }
        const int nd = dhi >= dlo ? dhi - dlo + 1 : 0;
        per = tiles_per_strip;
        list = step_list ? step_list + (size_t)kd * g.Dout * g.F * ntiles : nullptr;
        const int nlist = step_list ? step_count[kd] : 0;
        nsteps = step_list ? (nlist > strip ? (nlist - strip + nstrips - 1) / nstrips : 0) : nd * per;
        return true;
    }
    // step i -> (plane, tile); dense steps past the last tile are dead (ragged last strip)
    __device__ __forceinline__ void step_of(const int i, int &d, int &t) const {
        if (list) { const int e = list[strip + i * nstrips]; d = e / ntiles; t = e - d * ntiles; }
        else { d = dlo + i / per; t = strip * per + i % per; }
    }
    // first live step at or after i (nsteps: none)
    __device__ __forceinline__ int next_live(int i) const {
        if (list) return i < nsteps ? i : nsteps;
        while (i < nsteps && strip * per + i % per >= ntiles) ++i;      // ragged last strip
        return i < nsteps ? i : nsteps;
    }
    // operands of step i, global memory -> registers: the 10 x 18-site halo of x (minus the plane's background c_in, if
    // given) and the 8 x 16-site tile of dz, zeros outside the image
    __device__ __forceinline__ void load_step(const int i, const Geom &g, const float *__restrict__ in,
                                              const float *__restrict__ dz, const float *__restrict__ c_in,
                                              f32x4 (&xr)[W4_NX], f32x4 (&zr)[W4_NZ]) const {
        const int tid = threadIdx.x;
        int d, t;
        step_of(i, d, t);
        const int ds = mvx_src_plane(d, g.Din, g.Dout, g.sd, g.pd, kd);      // listed / dense steps always have a valid source
        const int tx0 = (t % tiles_x) * TW, ty0 = (t / tiles_x) * TH;
#pragma unroll
        for (int u = 0; u < W4_NX; ++u) {
            const int c = tid + W4_THREADS * u;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (c < HH * HW * 16) {
                const int r = c >> 4, part = c & 15;
                const int gy = ty0 - 1 + r / HW, gx = tx0 - 1 + r % HW;
                if (gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) {
                    v = *(const f32x4 *)(in + (((size_t)ds * g.H + gy) * g.W + gx) * g.Cin + cc * W4_C + part * 4);
                    if (c_in) v -= *(const f32x4 *)(c_in + (size_t)ds * g.Cin + cc * W4_C + part * 4);
                }
            }
            xr[u] = v;
        }
#pragma unroll
        for (int u = 0; u < W4_NZ; ++u) {
            const int c = tid + W4_THREADS * u;
            const int r = c >> 4, part = c & 15;
            const int gy = ty0 + (r >> 4), gx = tx0 + (r & 15);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (gy < g.H && gx < g.W)
                v = *(const f32x4 *)(dz + (((size_t)d * g.H + gy) * g.W + gx) * g.Cout + part * 4);
            zr[u] = v;
        }
    }
};

// ``slots``: bit i = slot i of tap group grp is executed (block-uniform; all ones except for the structurally zero
// (tap, parity) blocks of a stride-2 kernel in space-to-depth form, Geom::s2d): the window taps that carry weight for the
// parity block of input-channel chunk cc (group 0 owns window taps (0,0), (0,1) = slots 0, 1; group 1 owns (1,0), (1,1))
template <bool T2>
__device__ __forceinline__ unsigned w4_slots(const Geom &g, const int cc, const int grp) {
    if (!(T2 && g.s2d > 0)) return 0x1fu;
    const unsigned m = s2d_tap_mask((cc * W4_C) / g.s2d);
    return grp == 0 ? (m & 3u) : ((m >> 2) & 3u);
}

// slab[strip][kd][tap][c (Cin)][n (64)] = acc * o_scale: every tap is written by the group that owns it (zeros where nothing
// was computed); o_scale undoes the operand scaling of fp16 pieces and is 1 otherwise
template <bool T2>
__device__ __forceinline__ void w4_store_slabs(const f32x16 (&acc)[5], float *__restrict__ slabs, const W4Walk &wk,
                                               const Geom &g, const float o_scale) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
    const int grp = wv >> 2, wm = (wv >> 1) & 1, wn = wv & 1;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int t9 = grp == 0 ? w4_own(T2, 0, i) : w4_own(T2, 1, i);
        if (t9 < 0) continue;
        float *o = slabs + ((((size_t)wk.strip * 3 + wk.kd) * 9 + t9) * g.Cin + wk.cc * W4_C + wm * 32) * BN + wn * 32;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mfma32_row(r) + 4 * lh;
            o[(size_t)row * BN + li] = acc[i][r] * o_scale;
        }
    }
}

}  // namespace
