// Dense 3x3x3 convolution, forward and input gradient, on the bf16 matrix cores with fp32-grade accuracy ("bf16x3" split).
//
// Every f32 operand x is split on the fly into two bf16 numbers, hi = bf16(x) and
// lo = bf16(x - hi) (together 16 mantissa bits), and a product is evaluated as
//     x*w  ~=  hi_x*hi_w + hi_x*lo_w + lo_x*hi_w            (3 v_mfma_f32_32x32x16_bf16, f32 accumulate)
// The dropped terms are O(2^-16 |x w|): per-product relative error ~2e-5, far inside the 1e-4 bar of
// the fp32 features (tests compare against the float64 oracle).  A bf16 MFMA retires 16x the MACs
// per cycle of the exact-f32 MFMA, so three of them are ~5x faster than one f32 MFMA step.
//
// Structure = conv3d.hip's gather kernel (8x16-site patch x 64 output channels per workgroup, wave w
// owns rows 2w,2w+1; halo staged once per (depth tap, 32-channel chunk)), with:
//   - LDS rows of pieces x 64 B + 16 B pad -> ds_read_b128 operand fetches
//     (8 consecutive k per lane, the native 32x32x16 A/B fragment) are bank-conflict free;
//   - the f32 -> bf16 pieces split of the activations happens while the halo is staged;
//   - with THREE pieces per operand and six MFMAs per product ("bf16x6", MVX_FLAG_SPLIT3) the arithmetic is fp32-grade:
//     hi + mid + lo is the f32 operand exactly and the dropped cross terms are below the rounding of an f32 product;
//   - weights are pre-split by the pack kernel and staged three taps (one kernel row) at a time, so a
//     barrier pair covers 3 taps x 12 MFMAs per wave instead of one tap.
// The weight gradient in these arithmetics is conv3d_wgrad4s (conv3d.hip), behind the f32 entry points with MVX_FLAG_SPLIT.
#include "common.h"
#include "conv_kernels.h"
#include "rowgemm_common.h"      // mvxi_rowgemm_k128_enable (mvx_tuning_set lives in this file)

namespace {

constexpr int TH2 = 16;                           // patch height of the 16 x 16-site gather units

// torch W[co][ci][kd][kh][kw] -> wsp[kd][tap][32-channel chunk][n][piece][32] (bf16), forward or dgrad view
__global__ void pack_weights_split(const float *__restrict__ w, unsigned short *__restrict__ wsp, int Co, int Ci, int dgrad, int np, int fmt) {
    const int K = dgrad ? Co : Ci, N = dgrad ? Ci : Co;
    const int nch = K / BK;
    const long long total = 27ll * K * N;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(e % BK);
        long long r = e / BK;
        const int n = (int)(r % N); r /= N;
        const int ch = (int)(r % nch); r /= nch;
        const int tap = (int)(r % 9);
        const int kd = (int)(r / 9);
        const int a = tap / 3, b = tap % 3;
        const int kk = ch * BK + k;
        const int co = dgrad ? kk : n, ci = dgrad ? n : kk;
        const int kh = dgrad ? 2 - a : a, kw = dgrad ? 2 - b : b;
        float x = w[((((long long)co * Ci + ci) * 3 + kd) * 3 + kh) * 3 + kw];
        const long long row = (((long long)kd * 9 + tap) * nch + ch) * N + n;
        for (int q = 0; q < np; ++q) {
            if (fmt == 0) {
                const __bf16 pb = (__bf16)x;
                wsp[(row * np + q) * BK + k] = __builtin_bit_cast(unsigned short, pb);
                x -= (float)pb;
            } else {
                if (q == 0) x *= SPLIT_F16_WSCALE;
                const _Float16 pb = (_Float16)x;
                wsp[(row * np + q) * BK + k] = __builtin_bit_cast(unsigned short, pb);
                x -= (float)pb;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// The gather (forward / dgrad).  Template: NP pieces, BKT input channels per stage (32 or 16), MT site tiles per wave:
//   MT = 1: 8 x 16-site patch per workgroup, wave w owns patch rows 2w, 2w+1 (32 sites) x 64 channels;
//   MT = 2: 16 x 16-site patch, a wave owns 64 sites x 64 channels (four accumulator tiles): half the weight bytes and
//           weight-operand reads per MFMA and twice the matrix work between two barriers.  The activity flags stay per
//           8 x 16 tile (what activity.hip produces): a workgroup covers the tiles (tx, 2 ty) and (tx, 2 ty + 1) and ORs
//           their flags -- computing a background half is exact, just not needed.
// LDS rows hold the NP pieces of a site's (or an output channel's) BKT channels back to back + 16 B pad (an odd number
// of 16-byte slots: the ds_read_b128 fragment reads of 16 consecutive rows cover all banks); the halo row pitch is a
// multiple of 256 B so that the two patch rows a fragment read touches start on the same slot (lane groups
// {0-3,12-15,20-27} / {4-11,16-19,28-31} then hit 16 distinct slots).  Shapes used (launch_gather_split):
//   bf16x3: <2,32,1> 57 KB and <2,32,2> 79 KB;   bf16x6: <3,32,1> 79 KB and <3,16,2> 59 KB -- two workgroups per CU each.
// WIN: the launch has a tap window or structural zeros (MVX_FLAG_TAPS2): rows and columns of the 3 x 3 kernel are skipped by
// block-uniform masks; without it the three kernel rows are unrolled at compile time (8 % faster on the dense launches).
// ------------------------------------------------------------------------------------------
template <int NP, int BKT, int MT, bool WIN, int FMT>
__global__ __launch_bounds__(256, 2) void conv3d_gather_splitT(const float *__restrict__ in,
                                                               const unsigned short *__restrict__ wsp,
                                                               const float *__restrict__ bias,
                                                               float *__restrict__ out, double *__restrict__ stats,
                                                               Geom g, int relu, const int *__restrict__ in_hflag,
                                                               const unsigned char *__restrict__ out_mask,
                                                               const float *__restrict__ bg_pre, int border_active,
                                                               const int *__restrict__ only_tiles,
                                                               unsigned long long *__restrict__ exec_stages,
                                                               const float *__restrict__ in_amax) {
    // fp16 pieces (FMT = 1, split_common.h): `in` is scaled by a_scale (from its bound amax, else 1), the weights were packed
    // times SPLIT_F16_WSCALE; the accumulators are scaled back before the epilogue
    float a_scale = 1.f;
    if constexpr (FMT == 1) a_scale = split_scale_of(in_amax);
    constexpr int THT = TH * MT, HHT = THT + 2;
    constexpr int ROWBT = NP * BKT * 2 + 16;                 // bytes per LDS row
    constexpr int HROW = (HW * ROWBT + 255) / 256 * 256;     // halo row pitch
    constexpr int PPR = NP * BKT / 8;                        // 16-byte pieces per staged weight row
    constexpr int PT = BN * PPR;                             // ... per tap tile
    constexpr int NWU = (3 * PT + 255) / 256;                // ... per thread and kernel row (3 taps)
    constexpr int PARTS = BKT / 4;                           // float4 per site and stage
    constexpr int NH = (HHT * HW * PARTS + 255) / 256;
    constexpr int KS = BKT / 16;                             // MFMA k-steps per stage
    __shared__ __attribute__((aligned(256))) unsigned char s_halo[HHT * HROW];
    __shared__ __attribute__((aligned(16))) unsigned char s_w[3][BN * ROWBT];
    __shared__ float s_red[4][2 * BN];
    const int tiles_x = (g.W + TW - 1) / TW, tiles_y8 = (g.H + TH - 1) / TH;
    const int ntiles8 = tiles_x * tiles_y8;
    const int tx = blockIdx.x % tiles_x, tyb = blockIdx.x / tiles_x;
    const int tx0 = tx * TW, ty0 = tyb * THT;
    const int t_top = (MT * tyb) * tiles_x + tx;
    const bool has_bot = MT == 2 && 2 * tyb + 1 < tiles_y8;
    const int t_bot = has_bot ? t_top + tiles_x : t_top;
    const int d = blockIdx.y, nb = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int nchunks = g.Cin / BKT;
    // restricted launch: only the units with a flagged output tile are produced
    if (only_tiles && !(only_tiles[(size_t)d * ntiles8 + t_top] | only_tiles[(size_t)d * ntiles8 + t_bot])) return;
    // executed depth taps, skipped ones and the unit's state from the ORed flags of its MT tiles (conv_kernels.h)
    const bool on_border = tx0 == 0 || ty0 == 0 || tx0 + TW >= g.W || ty0 + THT >= g.H;
    const TilePlan plan = tile_plan<MT>(g, d, on_border, in_hflag, border_active, ntiles8, t_top, t_bot);

    f32x16 acc[MT][2];                                   // [site tile m: patch rows 2 MT wv + 2 m, + 1][channel tile: n0, n0 + 32]
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
    int a_base[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) a_base[m] = (2 * MT * wv + 2 * m + (li >> 4)) * HROW + (li & 15) * ROWBT + lh * 16;
    const int b_base = li * ROWBT + lh * 16;

    // one kernel row (three tap tiles) of pre-split weights per barrier pair.  NATIVE vector types: an array of HIP's uint4
    // struct stays an alloca, and the backend "promoted" it to LDS (one workgroup per CU)
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 wreg[NWU];
    auto load_w3 = [&](int kd, int a, int cc) __attribute__((always_inline)) {
        // global rows are [n][piece][32 channels] per 32-channel chunk; a BKT = 16 stage takes one half of every piece
        const int c32 = (cc * BKT) / BK, half = BKT == 16 ? (cc & 1) : 0;
#pragma unroll
        for (int u = 0; u < NWU; ++u) {
            int c = tid + 256 * u;
            if (3 * PT % 256 && c >= 3 * PT) c = 3 * PT - 1;                 // clamped; not stored
            const int t = c / PT, rem = c - t * PT;
            const int n = rem / PPR, piece = rem - n * PPR;
            const int q = piece / (BKT / 8), sub = piece - q * (BKT / 8);     // bf16 piece of the split, 16-byte part inside it
            const unsigned char *row = (const unsigned char *)wsp +
                (((((size_t)kd * 9 + a * 3 + t) * (g.Cin / BK) + c32) * g.Cout + (size_t)nb * BN + n) * NP + q) * (BK * 2);
            wreg[u] = *(const u32x4 *)(row + half * 32 + sub * 16);
        }
    };
    auto store_w3 = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < NWU; ++u) {
            const int c = tid + 256 * u;
            if (3 * PT % 256 == 0 || c < 3 * PT) {
                const int t = c / PT, rem = c - t * PT;
                const int n = rem / PPR, piece = rem - n * PPR;
                *(u32x4 *)(s_w[t] + n * ROWBT + piece * 16) = wreg[u];
            }
        }
    };

    // Stages = (valid depth tap) x (BKT-channel chunk), software-pipelined like conv3d_gather_pf (conv3d.hip): the halo of
    // stage s + 1 is fetched into registers while stage s computes (split into its pieces when it is written to LDS), the
    // weight rows go to LDS one kernel row at a time with the next row in flight, and the row needed next is always issued
    // BEFORE the long-latency halo fetch (vector-memory returns are in order).
    const int nstages = plan.active ? plan.nk * nchunks : 0;
    // executed work in units of the 8 x 16-tile, 32-channel stage (what the roofline prices)
    if (exec_stages && nstages > 0 && threadIdx.x == 0)
        atomicAdd(exec_stages, (unsigned long long)(plan.nk * (g.Cin / BK)) * (has_bot ? 2 : 1));
    int h_off[NH], h_lds[NH];     // per-thread halo slots: global float offset inside a (plane, chunk) image or -1; LDS byte offset or -1
#pragma unroll
    for (int u = 0; u < NH; ++u) {
        const int c = tid + 256 * u;
        h_off[u] = -1;
        h_lds[u] = -1;
        if (c < HHT * HW * PARTS) {
            const int r = c / PARTS, part = c - r * PARTS;
            const int hy = r / HW, hx = r - hy * HW;
            const int gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
            h_lds[u] = hy * HROW + hx * ROWBT + part * 8;
            if (gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) h_off[u] = (gy * g.W + gx) * g.Cin + part * 4;
        }
    }
    f32x4 hreg[NH];
    auto load_halo = [&](int st) __attribute__((always_inline)) {
        int kd, ds, cc;
        plan_stage(plan, nchunks, st, kd, ds, cc);
        const float *img = in + (size_t)ds * g.H * g.W * g.Cin + cc * BKT;
#pragma unroll
        for (int u = 0; u < NH; ++u)
            hreg[u] = h_off[u] >= 0 ? *(const f32x4 *)(img + h_off[u]) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    auto store_halo = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < NH; ++u)
            if (h_lds[u] >= 0) {
                uint2 pc[NP];
                if constexpr (FMT == 1) hreg[u] *= a_scale;
                split_n<NP, FMT>(hreg[u][0], hreg[u][1], hreg[u][2], hreg[u][3], pc);
#pragma unroll
                for (int q = 0; q < NP; ++q) *(uint2 *)(s_halo + h_lds[u] + q * BKT * 2) = pc[q];
            }
    };
    auto load_wrow = [&](int st, int a) __attribute__((always_inline)) {
        int kd, ds, cc;
        plan_stage(plan, nchunks, st, kd, ds, cc);
        load_w3(kd, a, cc);
    };
    auto compute_row = [&](int a, unsigned colmask) __attribute__((always_inline)) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            if (!((colmask >> b) & 1u)) continue;             // block-uniform: taps outside the window / structural zeros
#pragma unroll
            for (int s2 = 0; s2 < KS; ++s2) {
                bf16x8 b0[NP], b1[NP];
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    b0[q] = __builtin_bit_cast(bf16x8, *(const uint4 *)(s_w[b] + b_base + q * BKT * 2 + s2 * 32));
                    b1[q] = __builtin_bit_cast(bf16x8, *(const uint4 *)(s_w[b] + b_base + 32 * ROWBT + q * BKT * 2 + s2 * 32));
                }
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const int a_off = a_base[m] + a * HROW + b * ROWBT + s2 * 32;
                    bf16x8 av[NP];
#pragma unroll
                    for (int q = 0; q < NP; ++q) av[q] = __builtin_bit_cast(bf16x8, *(const uint4 *)(s_halo + a_off + q * BKT * 2));
                    split_mac2<NP, FMT>(acc[m][0], acc[m][1], av, b0, b1);
                }
            }
        }
    };
    if constexpr (!WIN) {
        if (nstages > 0) {
            load_wrow(0, 0);
            load_halo(0);
        }
        for (int st = 0; st < nstages; ++st) {
            const int nxt = st + 1 < nstages ? st + 1 : st;      // unconditional prefetches: the last stage re-fetches and drops
            __syncthreads();                                      // the previous stage's LDS reads are done
            store_halo();
            store_w3();                                           // kernel row 0
            __syncthreads();
            load_wrow(st, 1);                                     // next weight row first ...
            load_halo(nxt);                                       // ... then the long-latency halo of the next stage
            compute_row(0, 7u);
            __syncthreads();
            store_w3();                                           // kernel row 1
            __syncthreads();
            load_wrow(st, 2);
            compute_row(1, 7u);
            __syncthreads();
            store_w3();                                           // kernel row 2
            __syncthreads();
            load_wrow(nxt, 0);
            compute_row(2, 7u);
        }
    } else {
        // taps executed in a stage, bit (a * 3 + b): all nine, or the window [tap_lo, tap_hi)^2, minus the structural zeros of a
        // stride-2 kernel in space-to-depth form (forward: by the parity block of the stage's input channels; dgrad: of this
        // unit's output channels).  Block-uniform, and never empty (tap (1,1) of the window always carries weight).
        auto taps_of = [&](int st) __attribute__((always_inline)) -> unsigned {
            unsigned m4 = 0xfu;
            if (g.s2d > 0) m4 = s2d_tap_mask(g.mode == 0 ? ((st % nchunks) * BKT) / g.s2d : (nb * BN) / g.s2d);
            unsigned m9 = 0u;
    #pragma unroll
            for (int a = 0; a < 3; ++a)
    #pragma unroll
                for (int b = 0; b < 3; ++b) {
                    const int ta = g.mode == 0 ? a : 2 - a, tb = g.mode == 0 ? b : 2 - b;       // window tap of kernel row / column
                    const bool in = a >= g.tap_lo && a < g.tap_hi && b >= g.tap_lo && b < g.tap_hi;
                    const bool on = g.s2d > 0 ? ((m4 >> ((ta & 1) * 2 + (tb & 1))) & 1u) && ta < 2 && tb < 2 : true;
                    if (in && on) m9 |= 1u << (a * 3 + b);
                }
            return m9;
        };
        auto first_row = [&](unsigned m9) __attribute__((always_inline)) { return (m9 & 7u) ? 0 : ((m9 & 0x38u) ? 1 : 2); };
        auto next_row = [&](unsigned m9, int a) __attribute__((always_inline)) {      // next executed kernel row after a, or -1
            for (int r = a + 1; r < 3; ++r)
                if ((m9 >> (3 * r)) & 7u) return r;
            return -1;
        };
        int st = 0;
        unsigned m9 = nstages > 0 ? taps_of(0) : 0x1ffu;
        int a = first_row(m9);
        if (nstages > 0) {
            load_wrow(0, a);
            load_halo(0);
        }
        while (st < nstages) {
            const bool first = a == first_row(m9);
            int a2 = next_row(m9, a), st2 = st;
            unsigned m9n = m9;
            if (a2 < 0) {
                st2 = st + 1;
                m9n = st2 < nstages ? taps_of(st2) : m9;
                a2 = first_row(m9n);
            }
            const int stp = st2 < nstages ? st2 : st;            // unconditional prefetches: the last one re-fetches and drops
            __syncthreads();                                      // the previous row's LDS reads are done
            if (first) store_halo();
            store_w3();
            __syncthreads();
            load_wrow(stp, a2);                                   // next weight row first ...
            if (first) load_halo(st + 1 < nstages ? st + 1 : st); // ... then the long-latency halo of the next stage
            compute_row(a, (m9 >> (3 * a)) & 7u);
            st = st2; a = a2; m9 = m9n;
        }
    }

    if constexpr (FMT == 1) {
        const float o_scale = split_inverse(split_scale_of(in_amax)) * (1.f / SPLIT_F16_WSCALE);
#pragma unroll
        for (int m = 0; m < MT; ++m) { acc[m][0] *= o_scale; acc[m][1] *= o_scale; }
    }
    // ---- epilogue (conv_kernels.h): f32 sums per lane, f64 across the waves
    gather_epilogue<MT, 2, float>(acc, plan, g, d, nb, tx0, ty0, blockIdx.x + blockIdx.y * gridDim.x, s_red, bias, out, stats, relu,
                                  out_mask, bg_pre);
}

// 16 x 16-site units when the launch has enough of them to fill two workgroup slots on every CU with a margin, else 8 x 16.
// The threshold is a tuning value (mvx_tuning_set(MVX_TUNE_SPLIT16_MIN_UNITS, v): 0 forces the 16 x 16 kernel, a huge
// value the 8 x 16 one; the tests run both shapes on small inputs that way).
static long long g_split16_min_units = 768;

extern "C" int mvx_tuning_set(int32_t key, int64_t value) {
    if (key == MVX_TUNE_SPLIT16_MIN_UNITS) { g_split16_min_units = value; return MVX_OK; }
    if (key == MVX_TUNE_GATHER_NARROW_MAX_UNITS) { mvxi_gather_narrow_max_units(value); return MVX_OK; }
    if (key == MVX_TUNE_ROWGEMM_K128) { mvxi_rowgemm_k128_enable(value); return MVX_OK; }
    return MVX_EINVAL;
}

static inline int pieces_of(int flags) { return (flags & MVX_FLAG_SPLIT_F16) ? 2 : (flags & MVX_FLAG_SPLIT3) ? 3 : 2; }
static inline int fmt_of(int flags) { return (flags & MVX_FLAG_SPLIT_F16) ? 1 : 0; }

// (no BatchNorm finalize and no persistent launch here: those fields of GatherArgs stay off)
static void launch_gather_split(hipStream_t st, int flags, const Geom &g, const unsigned short *wsp, const GatherArgs &a) {
    const int planes = g.Dout * g.F, nblocks = g.Cout / BN;
    const int tiles_x = (int)mvx_cdiv(g.W, TW);
    const long long units16 = (long long)tiles_x * mvx_cdiv(g.H, TH2) * planes * nblocks;
    const bool big = units16 >= g_split16_min_units;
    const dim3 grid(tiles_x * mvx_cdiv(g.H, big ? TH2 : TH), planes, nblocks);
    const bool win = g.tap_lo != 0 || g.tap_hi != 3 || g.s2d > 0;
    const SplitAmax am = mvxi_take_split_amax();         // bound by mvx_split_operand_amax for this launch (fp16 pieces), else NULLs
#define MVX_GO(NP_, BK_, MT_, F_)                                                                                                        \
    do {                                                                                                                             \
        if (win)                                                                                                                     \
            hipLaunchKernelGGL((conv3d_gather_splitT<NP_, BK_, MT_, true, F_>), grid, dim3(256), 0, st, a.in, wsp, a.bias, a.out,        \
                               a.stats, g, a.relu, a.in_hflag, a.out_mask, a.bg_pre, a.border_active, a.only_tiles,                  \
                               a.exec_stages, am.a);                                                                                 \
        else                                                                                                                         \
            hipLaunchKernelGGL((conv3d_gather_splitT<NP_, BK_, MT_, false, F_>), grid, dim3(256), 0, st, a.in, wsp, a.bias, a.out,       \
                               a.stats, g, a.relu, a.in_hflag, a.out_mask, a.bg_pre, a.border_active, a.only_tiles,                  \
                               a.exec_stages, am.a);                                                                                 \
    } while (0)
    if (fmt_of(flags)) { if (big) MVX_GO(2, 32, 2, 1); else MVX_GO(2, 32, 1, 1); }
    else if (pieces_of(flags) == 3) { if (big) MVX_GO(3, 16, 2, 0); else MVX_GO(3, 32, 1, 0); }
    else              { if (big) MVX_GO(2, 32, 2, 0); else MVX_GO(2, 32, 1, 0); }
#undef MVX_GO
}

}  // namespace

extern "C" size_t mvx_conv3d_packed_weight_bytes_split(int32_t cout, int32_t cin, int32_t flags) {
    if (cout <= 0 || cin <= 0) return 0;
    return (size_t)27 * cout * cin * pieces_of(flags) * sizeof(unsigned short);
}

extern "C" int mvx_conv3d_pack_weights_split(const float *w, void *wsplit, int32_t cout, int32_t cin, int32_t for_dgrad,
                                             int32_t flags, void *stream) {
    MVX_CHECK_ARG(w && wsplit && cout > 0 && cin > 0);
    MVX_CHECK_ARG((for_dgrad ? cout : cin) % BK == 0);
    const long long total = 27ll * cout * cin;
    hipLaunchKernelGGL(pack_weights_split, dim3(mvx_cdiv(total, 256) > 2048 ? 2048 : mvx_cdiv(total, 256)), dim3(256), 0,
                       (hipStream_t)stream, w, (unsigned short *)wsplit, cout, cin, for_dgrad, pieces_of(flags), fmt_of(flags));
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_conv3d_forward_split(const float *in, const void *wsplit, const float *bias, float *out, double *stats,
                                        int32_t din, int32_t dout, int32_t h, int32_t w, int32_t cin, int32_t cout,
                                        int32_t stride_d, int32_t pad_d, int32_t flags, void *stream) {
    MVX_CHECK_ARG(in && wsplit && out);
    int rc = conv_check_forward(din, dout, h, w, cin, cout, stride_d, pad_d);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = conv_zero_stats(stats, nullptr, cout, 1, flags, st);
    if (e != hipSuccess) return (int)e;
    Geom g{din, dout, h, w, cin, cout, stride_d, pad_d, 0};
    GatherArgs a;
    a.in = in; a.bias = bias; a.out = out; a.stats = stats; a.relu = flags & MVX_FLAG_RELU;
    launch_gather_split(st, flags, g, (const unsigned short *)wsplit, a);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_conv3d_forward_bg_split_frames(const float *in, const void *wsplit, const float *bias, float *out,
                                                  double *stats, int32_t din, int32_t dout, int32_t h, int32_t w, int32_t cin,
                                                  int32_t cout, int32_t stride_d, int32_t pad_d, int32_t flags,
                                                  const int32_t *in_halo_flags, const uint8_t *out_mask, const float *bg_pre,
                                                  int32_t border_active, uint64_t *exec_stages, int32_t n_frames, void *stream) {
    MVX_CHECK_ARG(in && wsplit && out && in_halo_flags && out_mask && bg_pre);
    int rc = conv_check_frames(n_frames);
    if (rc) return rc;
    if ((rc = conv_check_forward(din, dout, h, w, cin, cout, stride_d, pad_d))) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = conv_zero_stats(stats, nullptr, cout, n_frames, flags, st);
    if (e != hipSuccess) return (int)e;
    Geom g{din, dout, h, w, cin, cout, stride_d, pad_d, 0, n_frames};
    GatherArgs a;
    a.in = in; a.bias = bias; a.out = out; a.stats = stats; a.relu = flags & MVX_FLAG_RELU;
    a.in_hflag = in_halo_flags; a.out_mask = out_mask; a.bg_pre = bg_pre;
    a.border_active = (border_active ? 1 : 0) | ((flags & MVX_FLAG_BG_TAPS) ? 2 : 0);
    a.exec_stages = (unsigned long long *)exec_stages;
    launch_gather_split(st, flags, g, (const unsigned short *)wsplit, a);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_conv3d_forward_bg_split(const float *in, const void *wsplit, const float *bias, float *out, double *stats,
                                           int32_t din, int32_t dout, int32_t h, int32_t w, int32_t cin, int32_t cout,
                                           int32_t stride_d, int32_t pad_d, int32_t flags, const int32_t *in_halo_flags,
                                           const uint8_t *out_mask, const float *bg_pre, int32_t border_active,
                                           void *stream) {
    return mvx_conv3d_forward_bg_split_frames(in, wsplit, bias, out, stats, din, dout, h, w, cin, cout, stride_d, pad_d, flags,
                                              in_halo_flags, out_mask, bg_pre, border_active, nullptr, 1, stream);
}

static int launch_dgrad_split(const float *dz, const void *wsplit_dgrad, float *dx, int32_t din, int32_t dout, int32_t h,
                              int32_t w, int32_t cin, int32_t cout, int32_t stride_d, int32_t pad_d, int32_t flags,
                              const int32_t *only_tiles, uint64_t *exec_stages, int32_t n_frames, void *stream) {
    MVX_CHECK_ARG(dz && wsplit_dgrad && dx);
    int rc = conv_check_frames(n_frames);
    if (rc) return rc;
    if ((rc = conv_check_geom(din, dout, h, w, cout, cin, stride_d, pad_d))) return rc;
    Geom g{dout, din, h, w, cout, cin, stride_d, pad_d, 1, n_frames};
    conv_set_taps2(g, flags, CONV_INPUT_GRAD, BN);
    GatherArgs a;
    a.in = dz; a.out = dx; a.only_tiles = only_tiles; a.exec_stages = (unsigned long long *)exec_stages;
    launch_gather_split((hipStream_t)stream, flags, g, (const unsigned short *)wsplit_dgrad, a);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_conv3d_dgrad_tiles_split_frames(const float *dz, const void *wsplit_dgrad, float *dx, int32_t din,
                                                   int32_t dout, int32_t h, int32_t w, int32_t cin, int32_t cout,
                                                   int32_t stride_d, int32_t pad_d, int32_t flags,
                                                   const int32_t *dx_tile_flags, uint64_t *exec_stages, int32_t n_frames,
                                                   void *stream) {
    MVX_CHECK_ARG(dx_tile_flags);
    return launch_dgrad_split(dz, wsplit_dgrad, dx, din, dout, h, w, cin, cout, stride_d, pad_d, flags, dx_tile_flags,
                              exec_stages, n_frames, stream);
}

extern "C" int mvx_conv3d_dgrad_tiles_split(const float *dz, const void *wsplit_dgrad, float *dx, int32_t din, int32_t dout,
                                            int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t stride_d,
                                            int32_t pad_d, int32_t flags, const int32_t *dx_tile_flags, void *stream) {
    MVX_CHECK_ARG(dx_tile_flags);
    return launch_dgrad_split(dz, wsplit_dgrad, dx, din, dout, h, w, cin, cout, stride_d, pad_d, flags, dx_tile_flags, nullptr, 1,
                              stream);
}

extern "C" int mvx_conv3d_dgrad_split(const float *dz, const void *wsplit_dgrad, float *dx, int32_t din, int32_t dout,
                                      int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t stride_d, int32_t pad_d,
                                      int32_t flags, void *stream) {
    return launch_dgrad_split(dz, wsplit_dgrad, dx, din, dout, h, w, cin, cout, stride_d, pad_d, flags, nullptr, nullptr, 1, stream);
}

// ------------------------------------------------------------------------------------------
// 2-D convolutions of the RPN on frame sets, bf16x3 (modules/voxelnet/Pipe.py:45-75): the same kernels with one plane
// per frame (din = dout = 1, pad_d = 1: only the middle depth tap exists).  Weights: the 2-D kernel placed in the middle
// depth slice of a 3-D one and packed with mvx_conv3d_pack_weights_split.  The stride-2 layers run on the space-to-depth
// image with their rearranged 3x3 kernel (MVX_FLAG_TAPS2: only its 2x2 window is executed, conv_set_taps2).
// ------------------------------------------------------------------------------------------
extern "C" int mvx_conv2d_forward_split_frames(const float *in, const void *wsplit, const float *bias, float *out, double *stats,
                                               int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t flags,
                                               int32_t n_frames, void *stream) {
    MVX_CHECK_ARG(in && wsplit && out);
    int rc = conv_check_frames(n_frames);
    if (rc) return rc;
    if ((rc = conv_check_geom(1, 1, h, w, cin, cout, 1, 1))) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = conv_zero_stats(stats, nullptr, cout, n_frames, flags, st);
    if (e != hipSuccess) return (int)e;
    Geom g{1, 1, h, w, cin, cout, 1, 1, 0, n_frames};
    conv_set_taps2(g, flags, CONV_FORWARD, BK);
    GatherArgs a;
    a.in = in; a.bias = bias; a.out = out; a.stats = stats; a.relu = flags & MVX_FLAG_RELU;
    launch_gather_split(st, flags, g, (const unsigned short *)wsplit, a);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_conv2d_dgrad_split_frames(const float *dz, const void *wsplit_dgrad, float *dx, int32_t h, int32_t w,
                                             int32_t cin, int32_t cout, int32_t flags, int32_t n_frames, void *stream) {
    return launch_dgrad_split(dz, wsplit_dgrad, dx, 1, 1, h, w, cin, cout, 1, 1, flags, nullptr, nullptr, n_frames, stream);
}
