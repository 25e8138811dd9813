// What the exact-f32 convolution (conv3d.hip) and its split-arithmetic form (conv3d_split.hip) agree on: the workgroup tile,
// the launch geometry `Geom` with its plane and tap-window rules, and the host scaffold of their entry points (argument
// checks, statistics zeroing, the MVX_FLAG_TAPS2 window, the operands of a gather launch `GatherArgs`, the layout of a
// weight-gradient workspace).  The device code the kernels share -- tile plan, gather epilogue, weight-gradient step walk --
// is in conv_kernels.h, which includes this file.  Per-kernel constants (LDS pitches, TH2, ...) and the strip-count
// heuristics stay with their kernels.
//
// Everything sits in an unnamed namespace, like the kernels that take a Geom by value: each of the two files gets its own copy.
#pragma once
#include "common.h"

namespace {

constexpr int TH = 8, TW = 16;          // output patch of a workgroup
constexpr int HH = TH + 2, HW = TW + 2; // halo
constexpr int BK = 32;                  // channels per K chunk
constexpr int BN = 64;                  // output channels per workgroup

struct Geom {
    int Din, Dout, H, W, Cin, Cout;     // gather view: in has Cin channels, out has Cout; Din / Dout = planes PER FRAME
    int sd, pd;                         // depth stride / padding of the FORWARD conv
    int mode;                           // 0 forward gather, 1 dgrad gather
    int F = 1;                          // frames stacked along the depth axis: global plane = frame * planes + local plane
    int tap_lo = 0, tap_hi = 3;         // in-plane taps (rows AND columns) [tap_lo, tap_hi) carry weight; the others are skipped
                                        // (stride-2 convolutions evaluated on the space-to-depth image use a 2x2 window)
    int s2d = 0;                        // > 0: channels per parity block of that image, see conv_set_taps2
};

// valid window taps of parity block p = pr * 2 + pc as a 4-bit mask, bit (ta * 2 + tb) (see conv_set_taps2)
__device__ __forceinline__ unsigned s2d_tap_mask(int p) {
    const int pr = p >> 1, pc = p & 1;
    unsigned m = 8u;                                   // (1,1) always
    if (pr) m |= 2u;                                   // (0,1)
    if (pc) m |= 4u;                                   // (1,0)
    if (pr && pc) m |= 1u;                             // (0,0)
    return m;
}

// source depth plane (global) of GLOBAL output plane d for depth tap kd; -1 if the tap falls outside the frame's volume
// (planes of different frames never connect)
__device__ __forceinline__ int src_depth(const Geom &g, int d, int kd) {
    if (g.mode == 0) return mvx_src_plane(d, g.Din, g.Dout, g.sd, g.pd, kd);
    // dgrad gather: the result (dx) has g.Dout planes per frame, the source (dz) g.Din
    return mvx_dst_plane(d, g.Dout, g.Din, g.sd, g.pd, kd);
}

// ---- host side of the entry points -----------------------------------------------------------------
// Sizes, depth stride / padding and channel granules of a gather view (its input channels in K chunks, its output channels
// in workgroup blocks).  2-D layers: (1, 1, h, w, cin, cout, 1, 1).  A rejected call drops the operand ranges bound for it
// (common.h MVX_CHECK_ARG).
static inline int conv_check_geom(int32_t din, int32_t dout, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t sd,
                                  int32_t pd) {
    MVX_CHECK_ARG(din > 0 && dout > 0 && h > 0 && w > 0 && cin > 0 && cout > 0);
    MVX_CHECK_ARG(sd >= 1 && sd <= 2 && pd >= 0 && pd <= 1);
    if (cin % BK || cout % BN) {
        mvxi_drop_split_amax();
        return MVX_ESIZE;
    }
    return MVX_OK;
}

// ... of a forward convolution, whose output depth follows from the input's
static inline int conv_check_forward(int32_t din, int32_t dout, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t sd,
                                     int32_t pd) {
    const int rc = conv_check_geom(din, dout, h, w, cin, cout, sd, pd);
    if (rc) return rc;
    MVX_CHECK_ARG(dout == (din + 2 * pd - 3) / sd + 1);
    return MVX_OK;
}

static inline int conv_check_frames(int32_t n_frames) {
    MVX_CHECK_ARG(n_frames >= 1 && n_frames <= MVX_MAX_FRAMES);
    return MVX_OK;
}

// 8 x 16-site tiles of a plane
static inline int conv_ntiles(int32_t h, int32_t w) { return (int)(mvx_cdiv(w, TW) * mvx_cdiv(h, TH)); }

// BatchNorm sums f64 [n_frames][MVX_REP][2][cout] and the arrival counter of the finalising launches (either may be null):
// zeroed on the stream unless the caller did it (MVX_FLAG_PREZEROED)
static inline hipError_t conv_zero_stats(double *stats, uint32_t *done_counter, int32_t cout, int32_t n_frames, int32_t flags,
                                         hipStream_t st) {
    if (flags & MVX_FLAG_PREZEROED) return hipSuccess;
    if (stats) {
        const hipError_t e = hipMemsetAsync(stats, 0, sizeof(double) * MVX_REP * 2 * cout * n_frames, st);
        if (e != hipSuccess) return e;
    }
    return done_counter ? hipMemsetAsync(done_counter, 0, sizeof(uint32_t), st) : hipSuccess;
}

// MVX_FLAG_TAPS2 (include/mvx_hip.h): a stride-2 3x3 convolution evaluated on the space-to-depth image of its input.  Only
// the 2x2 window of taps {0,1}^2 of the rearranged kernel carries weight; the input gradient reads the flipped window {1,2}^2.
// The image's channels are four parity blocks [pr][pc] of s2d channels each, and window tap (ta, tb) carries weight for
// parity (pr, pc) only if (ta == 1 || pr == 1) && (tb == 1 || pc == 1) -- 9 of the 16 (tap, parity) blocks; the others are
// structural zeros and are not executed (s2d_tap_mask), when a parity block is whole units of the calling kernel: `granule`
// = its K chunk (forward: the parity of a stage's input channels), its output-channel block (input gradient: the parity
// of the unit's OUTPUT channels) or its input-channel block (weight gradient).
enum ConvDir { CONV_FORWARD, CONV_INPUT_GRAD, CONV_WEIGHT_GRAD };
static inline void conv_set_taps2(Geom &g, int32_t flags, ConvDir dir, int granule) {
    if (!(flags & MVX_FLAG_TAPS2)) return;
    g.tap_lo = dir == CONV_INPUT_GRAD ? 1 : 0;
    g.tap_hi = g.tap_lo + 2;
    const int c = dir == CONV_INPUT_GRAD ? g.Cout : g.Cin;      // channels of the space-to-depth image
    if (c % 4 == 0 && (c / 4) % granule == 0) g.s2d = c / 4;
}

// Operands of a gather launch (launch_gather in conv3d.hip, launch_gather_split in conv3d_split.hip), by name: an entry point
// fills what it has and the rest stays off.  The packed weights, whose type differs between the two, are passed beside it.
struct GatherArgs {
    const float *in = nullptr, *bias = nullptr;
    float *out = nullptr;
    double *stats = nullptr;                    // BatchNorm sums of the output, see conv_zero_stats
    int relu = 0;
    // background rewrite (conv_kernels.h): halo activity [source plane][tile], computed output sites [plane][y][x], constants
    const int *in_hflag = nullptr;
    const unsigned char *out_mask = nullptr;
    const float *bg_pre = nullptr;
    int border_active = 0;                      // bit 0: border tiles always active, bit 1: bg_pre has bg_tap and bg_cls
    const int *only_tiles = nullptr;            // [output plane][tile] restricted launch: only flagged tiles are produced
    unsigned long long *exec_stages = nullptr;  // counter of executed K stages
    // f32 gather only: BatchNorm finalize by the last workgroup (counter, sites per channel, eps, result) and the zeroed unit
    // counter that allows the persistent launch
    unsigned *done_counter = nullptr;
    double fin_count = 0.0, fin_eps = 0.0;
    float *fin_mean_inv = nullptr;
    unsigned *work_counter = nullptr;
};

// Workspace of a weight gradient on compacted step lists: [slabs f32, slab_bytes][step list i32 3 x planes x ntiles]
// [step counts i32 4][ones i32 planes x ntiles], planes = output planes of all frames.  `ones` (with_ones) are the all-set
// activity flags of a launch that has none of its own.  workspace == NULL: only `bytes`, for the size queries.
struct WgradWorkspace {
    float *slabs;
    int *list, *count, *ones;
    size_t bytes;
};
static inline WgradWorkspace conv_carve_wgrad(void *workspace, size_t slab_bytes, int planes, int ntiles, bool with_ones) {
    const size_t steps = (size_t)planes * ntiles;
    WgradWorkspace c{nullptr, nullptr, nullptr, nullptr, slab_bytes + sizeof(int) * (3 * steps + 4 + (with_ones ? steps : 0))};
    if (workspace) {
        c.slabs = (float *)workspace;
        c.list = (int *)((char *)workspace + slab_bytes);
        c.count = c.list + 3 * steps;
        c.ones = with_ones ? c.count + 4 : nullptr;
    }
    return c;
}

}  // namespace
