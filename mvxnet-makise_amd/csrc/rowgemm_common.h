// What the row GEMMs (linear.hip, linear_split.hip, rowgemm_k128.hip, rowgemm_pre.hip) share: the tile epilogue of the two
// 128-row forward kernels, the XCD-aware tile order, the slab store of the two strip weight gradients, the host-side
// dispatch over the split arithmetics, the head of the entry points that keep BatchNorm sums, and the prototypes by which
// linear.hip hands a call to the other files (NOT part of the C ABI).  DESIGN.md section 3.25 says what stayed separate.
#pragma once
#include <type_traits>
#include "common.h"
#include "split_common.h"

// ---- XCD-aware tile order ------------------------------------------------------------------------------------------------
// Workgroup -> tile mapping that follows the chip: workgroups are dealt round-robin over the 8 XCDs (blocks h and h + 8 share
// one, MI355X_MICROARCH.md), and every XCD has its own L2.  With the plain (column block fastest) order the 6 column blocks
// of a 768-wide layer that share a 128-row block of x land on 6 different XCDs and each L2 fetches those rows for itself:
// 6 x 246 MB of HBM / Infinity-Cache reads for the 80 k x 768 x 768 layer, which made the GEMM memory-bound at 0.3-0.4 of the
// matrix pipe.  Here the launch is one-dimensional: XCD x = h % 8 runs the row blocks {8 j + x} and walks a row block's nbx
// column blocks in consecutive slots, so the blocks that share rows run on the SAME L2 at the same time.  (Speed only: nothing
// depends on the placement.)  Blocks beyond the last of the nby row blocks are off and exit.  The weight gradients use it with
// row block = row strip and column block = output block of the strip.
struct XcdTile { unsigned rb, cb; bool on; };
__device__ __forceinline__ XcdTile xcd_tile(unsigned h, unsigned nbx, unsigned nby) {
    const unsigned xcd = h & 7u, s = h >> 3;
    XcdTile t;
    t.rb = (s / nbx) * 8u + xcd;
    t.cb = s % nbx;
    t.on = t.rb < nby;
    return t;
}
static inline unsigned xcd_grid(unsigned nbx, unsigned nby) { return 8u * ((nby + 7u) / 8u) * nbx; }

// ---- tile epilogue of linear_fwd and linear_fwd_split ------------------------------------------------------------------
// The workgroup holds a 128-row x (32 NT)-column tile at (r0, n0): wave wv owns rows 32 wv .. 32 wv + 31 as NT accumulator
// tiles of 32 x 32.  y = [ReLU](acc + bias) is stored, and with `stats` the per-frame BatchNorm sums of the stored values go
// to replica `rep`; with `done_counter` the last of the launch's `total_blocks` workgroups finalises them.  `s_red` is the
// caller's LDS scratch.
//
// Every load the epilogue needs (bias, row weights) is issued FIRST and unconditionally from clamped addresses, the
// accumulators become the outputs in place, and only then come the stores: vector-memory operations return in order
// (one vmcnt), so a load issued between stores -- or under a condition the waitcnt pass cannot see through -- made
// every store wait for all earlier ones (`s_waitcnt vmcnt(0)` in front of each of the 16 * NT stores).
template <int NT>
__device__ __forceinline__ void rowgemm_tile_epilogue(f32x16 (&acc)[NT], const float *__restrict__ bias, float *__restrict__ y,
                                                      int ldy, double *__restrict__ stats, const float *__restrict__ row_w,
                                                      long long R, int N, int relu, long long r0, int n0, unsigned rep,
                                                      unsigned total_blocks, unsigned *__restrict__ done_counter, double fin_eps,
                                                      float *__restrict__ fin_mean_inv, const FrameMap &fm,
                                                      double (&s_red)[4][2 * 32 * NT]) {
    constexpr int BM = 128, BNL = 32 * NT;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lh = lane >> 5;
    float bsv[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = n0 + t * 32 + li;
        bsv[t] = bias ? bias[c < N ? c : N - 1] : 0.f;
    }
    float rwv[16];
    if (stats && row_w) {                      // one uniform branch around the whole batch of loads
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long gr = r0 + wv * 32 + mfma32_row(r) + 4 * lh;
            rwv[r] = row_w[gr < R ? gr : R - 1];
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) rwv[r] = 1.f;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = acc[t][r] + bsv[t];
            if (relu) v = fmaxf(v, 0.f);
            acc[t][r] = v;
        }
    // store, then the BatchNorm sums.  A 128-row block almost always lies inside one frame; a block that straddles a
    // frame boundary repeats the (register-only) reduction once per frame with the other frames' rows masked out.
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = n0 + t * 32 + li;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long gr = r0 + wv * 32 + mfma32_row(r) + 4 * lh;
            if (gr < R && c < N) y[gr * ldy + c] = acc[t][r];
        }
    }
    if (stats) {
        // frames met by this block, in segment order (a block can cross from the real rows into the padded rows, whose
        // frame order starts again at 0): walk the segments, one reduction per segment
        const int s_lo = fm_seg_at(fm, r0), s_hi = fm_seg_at(fm, r0 + BM - 1 < R ? r0 + BM - 1 : R - 1);
        for (int sg = s_lo; sg <= s_hi; ++sg) {
            const long long lo = fm_seg_lo(fm, sg), hi = fm_seg_hi(fm, sg, R);
            double s1[NT], s2[NT];          // f64 from the first addition on (var = E[y^2] - mean^2 cancels)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int c = n0 + t * 32 + li;
                s1[t] = 0.0; s2[t] = 0.0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long long gr = r0 + wv * 32 + mfma32_row(r) + 4 * lh;
                    if (gr < R && c < N && gr >= lo && gr < hi) {
                        // opaque per segment, and INSIDE the branch.  Opaque keeps the f64 conversions from being hoisted out
                        // of the segment loop: the 64 of v with their squares cost 256 VGPRs (the second wave), the 16 of the
                        // row weights 32 (the third wave of the NT = 4 f32 kernel).  Inside, because an asm cannot be
                        // speculated: the sums stay under exec masks.  Turned into selects (which the compiler did as soon as
                        // this code became a function) every term needs temporaries: 198 - 229 VGPRs instead of 157.
                        float v = acc[t][r], rwf = rwv[r];
                        asm volatile("" : "+v"(v), "+v"(rwf));
                        const double rw = (double)rwf;
                        s1[t] += rw * (double)v;
                        s2[t] += rw * (double)v * (double)v;
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const double a = s1[t] + __shfl_xor(s1[t], 32, 64), b = s2[t] + __shfl_xor(s2[t], 32, 64);
                if (lh == 0) { s_red[wv][t * 32 + li] = a; s_red[wv][BNL + t * 32 + li] = b; }
            }
            __syncthreads();
            double *slot = fm_stats_slot(stats, fm_seg_frame(fm, sg), rep, N);
            for (int e = tid; e < 2 * BNL; e += 256) {
                const int which = e / BNL, c = e % BNL;
                if (n0 + c < N) {
                    const double t = s_red[0][e] + s_red[1][e] + s_red[2][e] + s_red[3][e];
                    atomicAdd(slot + (size_t)which * N + n0 + c, t);
                }
            }
        }
        if (done_counter) {
            __shared__ int s_last;
            bn_finalize_by_last_block(done_counter, total_blocks, stats, N, fm, fin_eps, fin_mean_inv, &s_last);
        }
    }
}

// ---- slab store of linear_wgrad and linear_wgrad_split -----------------------------------------------------------------
// A wave's 64 x 64 block of a strip's slab o [N][K] at (n_base, k_base): acc[a][b] is its 32 x 32 tile (a, b).
__device__ __forceinline__ void store_slab_2x2(float *__restrict__ o, const f32x16 (&acc)[2][2], int n_base, int k_base, int N,
                                               int K, int li, int lh) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n_base + a * 32 + mfma32_row(r) + 4 * lh;
                const int k = k_base + b * 32 + li;
                if (n < N && k < K) o[(size_t)n * K + k] = acc[a][b][r];
            }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// Arithmetic code of a flags word (mvx_split_code, common.h) -> the <NP, FMT> of a split kernel (split_common.h): 4 = fp16x3
// (two fp16 pieces), 3 = bf16x6 (three bf16 pieces), anything else bf16x3 (two bf16 pieces).  `go` is a generic lambda that
// receives NP and FMT as std::integral_constant and launches its kernel.  X3 = false: the caller has no bf16x3 kernel (and has
// rejected the code): none is instantiated.
template <bool X3 = true, typename Go>
static inline void mvx_dispatch_pieces(int code, Go &&go) {
    using std::integral_constant;
    if (code == 4) go(integral_constant<int, 2>{}, integral_constant<int, 1>{});
    else if (code == 3) go(integral_constant<int, 3>{}, integral_constant<int, 0>{});
    else if constexpr (X3) go(integral_constant<int, 2>{}, integral_constant<int, 0>{});
}
// 16-bit planes per operand for a flags word; operands stored as planes (rowgemm_pre.hip) exist for the fp32-grade codes only:
// three bf16 pieces (MVX_FLAG_SPLIT3) or two fp16 pieces (MVX_FLAG_SPLIT_F16); 0: the flags name neither
static inline int mvx_split_planes(int flags) {
    const int code = mvx_split_code(flags);
    return code == 4 ? 2 : code == 3 ? 3 : 0;
}

static inline int mvx_clear_unless_prezeroed(void *p, size_t bytes, int flags, hipStream_t st) {
    if (flags & MVX_FLAG_PREZEROED) return MVX_OK;
    const hipError_t e = hipMemsetAsync(p, 0, bytes, st);
    return e == hipSuccess ? MVX_OK : (int)e;
}
// Head of a forward entry point, after its own argument checks: the frame map of the row layout, and the BatchNorm sums
// f64 [F][MVX_REP][2][n] cleared unless the caller did.  Nonzero: return it.  Zero and rows == 0: return MVX_OK, nothing to launch.
static inline int mvx_stats_preamble(FrameMap &fm, const mvx_frames_t *frames, int row_kind, long long rows, double count,
                                     double *stats, int n, int flags, hipStream_t st) {
    MVX_CHECK_ARG(mvx_build_frame_map(fm, frames, row_kind, rows, count));
    return stats ? mvx_clear_unless_prezeroed(stats, sizeof(double) * MVX_REP * 2 * n * fm.F, flags, st) : MVX_OK;
}

// ---- calls between the files (the caller has checked the arguments and built the frame map) -----------------------------
// linear_split.hip: the split arithmetics of mvx_linear_forward* / mvx_linear_wgrad for 16-byte aligned wide layers
int mvxi_linear_forward_split(const float *x, int ldx, const float *w, int ldw, const float *bias, float *y,
                              int ldy, double *stats, const float *row_w, long long rows, int k, int n, int relu,
                              unsigned *fin_counter, double fin_eps, float *fin_mean_inv, const FrameMap &fm, int pieces,
                              hipStream_t st, const SplitAmax &am = SplitAmax{nullptr, nullptr, 0});
int mvxi_linear_wgrad_split(const float *x, int ldx, const float *dz, int lddz, float *slabs, long long rows, int k, int n,
                            long long rows_per_strip, long long strips, int pieces, hipStream_t st,
                            const SplitAmax &am = SplitAmax{nullptr, nullptr, 0});
// rowgemm_k128.hip, K = 128: weights resident in LDS, rows streamed through registers; same contract and numbers
bool mvxi_rowgemm_k128_ok(int ldx, int ldw, int ldy, int k, int n);
void mvxi_rowgemm_k128_enable(long long v);
int mvxi_linear_forward_k128(const float *x, int ldx, const float *w, int ldw, const float *bias, float *y, int ldy, double *stats,
                             const float *row_w, long long rows, int n, int relu, unsigned *fin_counter, double fin_eps,
                             float *fin_mean_inv, const FrameMap &fm, int pieces, hipStream_t st, const SplitAmax &am);
