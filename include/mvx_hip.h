/* libmvx_hip -- C ABI of the MI355X-native MVXNet hot path (gfx950).
 *
 * This library stands where the reference's pybind11 extension stood
 * (modules/Extension.py:1-3 -> cpp/voxelutil.cpp:362-368, entry `_group`) and additionally
 * carries the GPU kernels that the reference obtained implicitly from ATen/cuDNN for the
 * modules on the hot path.
 *
 * Conventions (every entry point):
 *   - plain C types only; every data pointer is a DEVICE pointer unless its name ends in
 *     `_host`; `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - returns 0 on success, a negative MVX_E* code for an argument error, or a positive
 *     hipError_t from the launch;
 *   - stream-ordered, no hidden synchronisation, no persistent allocation: scratch memory
 *     comes from the caller (`*_workspace_bytes` queries), so calls can be graph-captured;
 *   - re-entrant and stream-ordered: no entry point keeps state between calls.  Process-wide exceptions, none of them in a
 *     data path: the launch-shape tuning values of mvx_tuning_set (read at launch time; the tests set them to force a
 *     kernel shape) and the diagnostic counter behind mvx_launch_count.  One per-THREAD exception: the operand ranges bound
 *     by mvx_split_operand_amax apply to the calling thread's next split-arithmetic launch and are cleared by it.
 */
#ifndef MVX_HIP_H
#define MVX_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per-channel BatchNorm accumulators are kept in MVX_STATS_REPLICAS replicas (workgroup b adds to
 * replica b mod R) so that the f64 atomics of concurrently finishing workgroups do not pile up on
 * one address; every `stats` buffer below is f64 [MVX_STATS_REPLICAS][2][channels] and
 * mvx_bn_finalize sums the replicas. */
#define MVX_STATS_REPLICAS 32

/* Bits of the `flags` arguments.  (Entry points that used to take `relu` take `flags`; bit 0 keeps
 * the old meaning.) */
#define MVX_FLAG_RELU 1        /* apply ReLU in the epilogue */
#define MVX_FLAG_PREZEROED 2   /* the stats / scratch accumulators passed in are already zero: skip the memset
                                  (lets a caller clear all accumulators of a frame with ONE fill) */
#define MVX_FLAG_ACCUMULATE 4  /* add the gradient to the destination instead of overwriting it */
#define MVX_FLAG_CONV2D 8      /* mvx_conv3d_wgrad: dw is a 2-D kernel gradient [cout][cin][3][3] (din = dout = 1, pad_d = 1) */
#define MVX_FLAG_TAPS2 16      /* mvx_conv2d_*: only the 2x2 tap window {0,1}^2 carries weight (stride-2 conv on the space-to-depth image) */
#define MVX_FLAG_BG_TAPS 32    /* mvx_conv3d_forward_bg_frames: bg_pre is the buffer of mvx_conv3d_background_taps_frames ([planes][cout] totals |
                                  [planes][3][cout] per-depth-tap constants | [planes][9][cout] image-border position classes): in interior
                                  tiles a depth tap whose source halo holds no active site is not executed (its constant is added in the
                                  epilogue), and a border tile without any active source is filled from the class constants (exact rewrites) */
#define MVX_FLAG_SPLIT 64      /* mvx_linear_forward*, mvx_linear_wgrad, mvx_conv3d_wgrad, mvx_conv3d_wgrad_bg*, mvx_conv2d_wgrad_frames (conv3d_wgrad4s, the
                                  convolutions' only split-arithmetic weight gradient: cin a multiple of 64): bf16x3 split arithmetic (three bf16 MFMAs per product, f32 accumulate, ~2e-5 per
                                  product: the row-GEMM side of `convmath: bf16x3`) for layers with n > 64, k % 4 == 0, 16-byte aligned
                                  operands and a row-major weight (w_transposed = 0); other calls run the exact-f32 kernel */

#define MVX_FLAG_SPLIT3 128    /* with MVX_FLAG_SPLIT, and on the *_split convolution entry points (forward, input gradient, weight packing): THREE bf16 pieces per f32 operand and six bf16 MFMAs per product
                                  ("bf16x6": hi + mid + lo is the operand exactly, dropped cross terms < 2^-25: fp32-grade accuracy) instead of two / three */

#define MVX_FLAG_PRE_XCD_STRIPS 4096  /* mvx_linear_wgrad_pre: every block of a row strip on the same XCD (shared L2) instead of consecutive block ids */
#define MVX_FLAG_SPLIT_F16 512  /* with MVX_FLAG_SPLIT, and on the *_split convolution entry points: TWO fp16 pieces per f32 operand (22 mantissa bits) and three
                                  fp16 MFMAs per product ("fp16x3": fp32-grade accuracy at the matrix work of bf16x3) -- for operands inside fp16's
                                  range: values above 65,504 overflow and below ~1e-4 lose relative precision, so callers scale by powers of two */

#define MVX_FLAG_AMAX_COARSE 1024 /* mvx_linear_forward*: the x operand bound by mvx_split_operand_amax is a FORWARD input from outside the library
                                  (sampled image features): its scale exponent is rounded down to a multiple of 8 binades, so that a frame set and
                                  one of its frames -- whose maxima differ -- scale, and therefore round, alike */

#define MVX_FLAG_NO_BG_FILL 2048  /* mvx_sparse_conv_output_frames: tiles (8 x 16 sites) whose 3 x 3 tile neighbourhood holds no voxel in any source
                                  plane are NOT written -- every site of them is ReLU(bias), which the tile-restricted consumers
                                  (mvx_bn_apply_tiles_frames, mvx_bn_relu_backward_tiles_frames) never read; the BatchNorm sums count them
                                  in closed form either way */

#define MVX_OK 0
#define MVX_EINVAL (-1)   /* bad argument (null pointer, size, unsupported combination) */
#define MVX_ESIZE (-2)    /* a size exceeds what the kernel supports */

/* ------------------------------------------------------------------------------------------
 * Frame sets.  The reference is batch-1 (config.yml:18, modules/voxelnet/VoxelNet.py:19): a batch of B frames is B
 * independent forwards with PER-FRAME BatchNorm statistics and summed parameter gradients.  The
 * `*_frames` entry points run all frames of a step through ONE launch per layer: row matrices hold the frames back to
 * back, grids stack them along the depth axis ([n_frames * planes][h][w][c]), and every per-frame quantity (statistics,
 * mean / inverse std, background constants, counters) gets a leading frame dimension.  Parameter gradients are summed
 * over the frames by construction.  The descriptor lives on the HOST and is copied by value into the launches.
 *
 *   real_off[f] .. real_off[f+1]   compact REAL rows of frame f (points that survived the T cap), all frames back to back
 *   vox_off[f]  .. vox_off[f+1]    voxels of frame f
 *   t                              samples per voxel: frame f stands for (vox_off[f+1]-vox_off[f]) * t dense rows
 * Row layouts (`row_kind`):
 *   MVX_ROWS_SINGLE  one frame, no descriptor (what the entry points without `_frames` use)
 *   MVX_ROWS_FUSION  [real rows of all frames][one shared padded row per frame]        (fusion MLP, imhead/Pipe.py:84-104)
 *   MVX_ROWS_VFE     [real rows of all frames][one padded row per voxel, all frames]   (VFE stack, voxelnet/Pipe.py:5-29)
 *   MVX_ROWS_VOXELS  [one row per voxel, all frames]
 *   MVX_ROWS_GRID    [n_frames][rows / n_frames] equal shares (channels-last grids)
 *   MVX_ROWS_REAL    [real rows of all frames] (the sampler's output before the shared padded rows are appended)
 */
#define MVX_MAX_FRAMES 16
#define MVX_ROWS_SINGLE 0
#define MVX_ROWS_FUSION 1
#define MVX_ROWS_VFE 2
#define MVX_ROWS_VOXELS 3
#define MVX_ROWS_GRID 4
#define MVX_ROWS_REAL 5        /* [real rows of all frames] only */
typedef struct {
    int32_t n_frames;
    int32_t t;
    int32_t real_off[MVX_MAX_FRAMES + 1];
    int32_t vox_off[MVX_MAX_FRAMES + 1];
} mvx_frames_t;

/* ABI version; bumped whenever a signature changes. */
int mvx_abi_version(void);
/* tuning values of the library (process-wide, not stream-ordered; meant for benchmarks and tests).  Keys:
 *   MVX_TUNE_SPLIT16_MIN_UNITS  the bf16x3 gather uses 16 x 16-site workgroup units when a launch has at least this many of them
 *                               (default 768), else 8 x 16-site units; 0 = always 16 x 16, a huge value = never
 *   MVX_TUNE_GATHER_NARROW_MAX_UNITS  the f32 gather (conv3d / conv2d forward and dgrad) runs a launch with fewer 64-channel
 *                               workgroup units than this as twice as many 32-channel units; 0 = never, negative (default) = fewer than
 *                               1.5 units per CU, i.e. while the doubled units are all resident at once
 *   MVX_TUNE_ROWGEMM_K128       1 (default): split-arithmetic row layers with k = 128 and n a multiple of 128 run the
 *                               weights-resident streaming kernel (csrc/rowgemm_k128.hip; same numbers); 0: linear_fwd_split */
#define MVX_TUNE_SPLIT16_MIN_UNITS 1
#define MVX_TUNE_GATHER_NARROW_MAX_UNITS 2
#define MVX_TUNE_ROWGEMM_K128 3
int mvx_tuning_set(int32_t key, int64_t value);

/* fp16x3 arithmetic (MVX_FLAG_SPLIT_F16): operand ranges.  An fp16 piece pair covers an f32 operand to 2^-22 while the low piece
 * is a normal fp16 number, i.e. for magnitudes in [2^-3, 65504]; activations behind a BatchNorm and weights (scaled by a fixed
 * 2^8 inside the library) sit there, gradients (1e-3 ... 1e-8) and foreign feature maps need not.  For those the caller binds
 * the device address of ONE float = max |value| of the tensor, and the kernel multiplies the operand by the power of two that
 * brings that maximum into [2^14, 2^15) and the f32 accumulator by its inverse -- powers of two change no rounding, so the
 * result is the same function of the inputs.  amax_a / amax_b belong to the first / second f32 operand of the calling
 * thread's NEXT launch that takes MVX_FLAG_SPLIT_F16 (convolution forward / input gradient and row GEMM: a = in / dz / x;
 * weight gradients: a = in / x, b = dz); NULL = that operand is not scaled.  The launch consumes the binding.  The floats are
 * read on the device in stream order: they may be written by an earlier kernel of the same stream.  Sources:
 * mvx_bn_relu_backward_frames and mvx_bn_relu_backward_tiles_frames
 * (dz_amax), mvx_tensor_amax for any other tensor.  Bound ranges are ignored by the other arithmetics. */
int mvx_split_operand_amax(const float *amax_a, const float *amax_b);
/* amax[0] = max(amax[0], max |x[i]|), i < n; amax is zeroed first unless MVX_FLAG_PREZEROED.  x 16-byte aligned. */
int mvx_tensor_amax(const float *x, int64_t n, float *amax, int32_t flags, void *stream);
/* Range guard of the fp16-piece arithmetic: weights are cut times 2^8, so |w| must stay below 65504 / 256 = 255.9.
 * status[0] |= MVX_STATUS_F16_WEIGHT_RANGE when an element of w (f32 [n]) does not (or is not finite); status is a device
 * word the caller checks with its other data-dependent status words (once per step: no host read inside the step). */
#define MVX_STATUS_F16_WEIGHT_RANGE 8
int mvx_split_f16_weight_check(const float *w, int64_t n, int32_t *status, void *stream);
/* Diagnostics: number of kernel launches the library has issued since it was loaded (fills excluded). */
uint64_t mvx_launch_count(void);

/* ------------------------------------------------------------------------------------------
 * Voxelizer.  Replaces cpp/voxelutil.cpp:325-360 (`_group`) together with the Python around
 * it: modules/data/Preprocessing.py:75-116 (`group`, out_channels = 9) and :57-73 (`group_`,
 * out_channels = 7).
 *
 * Frames are batched with a fixed stride: frame f owns points  pcd[f*cap_points ...] and
 * outputs [f*cap_voxels ...]; the live point count of each frame is read from DEVICE memory
 * (n_points[f]) so a preceding GPU crop can feed it without a host round trip.
 *
 *   pcd        f32 [F][cap_points][ncol]   ncol >= 4: x y z r (row col)
 *   perm       i32 [F][cap_points] or NULL shuffle permutation (Preprocessing.py:86 is an
 *                                          input here: stream position s reads point perm[s])
 *   n_points   i32 [F]
 *   ext_idx    i32 [F][cap_points][3] or NULL: precomputed voxel indices in STREAM order, the
 *                                          `idx` argument of the reference `_group`
 *                                          (voxelutil.cpp:325); NULL = computed here
 *   lo[3], size[3]                         range minimum and voxel size, f64 (Config.py:7)
 *   T                                      samplesPerVoxel (<= 64)
 *   out_channels                           9: x y z dx dy dz r row col, centroid = sequential
 *                                             f64 sum / count (Preprocessing.py:112-115)
 *                                          7: x y z dx dy dz r, centroid = f32 sum / count in
 *                                             f64 (Preprocessing.py:71-72)
 *   voxels     f32 [F][cap_voxels][T][out_channels]   (the reference's f64 rounded once to
 *                                          f32, which is what train.py:125 feeds the model)
 *   coords     i64 [F][cap_voxels][4]      (0, ix, iy, iz)  == train.py:119 layout
 *   counts     i32 [F][cap_voxels]         kept points per voxel (<= T)
 *   n_voxels   i32 [F]
 *   status     i32 [1]                     OR-ed flags: bit0 = an index fell outside the
 *                                          21-bit key range, bit1 = cap_voxels exceeded
 * cap_voxels >= cap_points always suffices.
 *
 * mvx_voxelize_frames: the same with the batch layout as an option.  concat = 0: as above.  concat != 0: the voxels of
 *   all frames are written BACK TO BACK in frame order -- voxels [cap_voxels][T][C], coords [cap_voxels][4] with
 *   coords[:,0] = frame index (the batch column of train.py:119), counts [cap_voxels]; cap_voxels is then the TOTAL
 *   capacity (n_frames * cap_points always suffices).  vox_off (optional) i32 [n_frames + 1] on the device = voxel
 *   offsets of the frames (vox_off[n_frames] = total).
 * Both entry points take 1 <= n_frames <= 63 (the gathers hold the n_frames + 1 voxel offsets one per lane of a wave);
 * anything else is MVX_EINVAL.
 * Four launches (insert, one look-back scan over all frames, gather of the voxels with at most 16 members, gather of the
 * rest) and two memsets per call.
 */
size_t mvx_voxelize_workspace_bytes(int32_t n_frames, int32_t cap_points);

int mvx_voxelize(const float *pcd, const int32_t *perm, const int32_t *n_points,
                 const int32_t *ext_idx, int32_t n_frames, int32_t cap_points, int32_t ncol,
                 double lo_x, double lo_y, double lo_z,
                 double size_x, double size_y, double size_z,
                 int32_t T, int32_t out_channels, int32_t cap_voxels,
                 float *voxels, int64_t *coords, int32_t *counts, int32_t *n_voxels,
                 int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
int mvx_voxelize_frames(const float *pcd, const int32_t *perm, const int32_t *n_points,
                        const int32_t *ext_idx, int32_t n_frames, int32_t cap_points, int32_t ncol,
                        double lo_x, double lo_y, double lo_z,
                        double size_x, double size_y, double size_z,
                        int32_t T, int32_t out_channels, int32_t cap_voxels, int32_t concat,
                        float *voxels, int64_t *coords, int32_t *counts, int32_t *n_voxels, int32_t *vox_off,
                        int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Sparse voxel rows <-> dense grid.  Replaces VoxelNet.reindex (modules/voxelnet/VoxelNet.py:16-22,
 * `res[b,:,iz,ix,iy] = x[v,:]`) and its autograd gather.  The grid is channels-last:
 *   grid f32 [d=iz][h=ix][w=iy][channels]   (logical NCDHW (1,C,D,H,W) with C innermost)
 *   feat f32 [n_voxels][channels], coords i64 [n_voxels][4] = (b, ix, iy, iz)
 * zero_grid != 0 clears the whole grid first (the reference allocates zeros every call).
 * status (optional) bit0 = a coordinate fell outside the grid (row skipped).
 * occupancy (optional) i32 [d][ceil(h/tile_h)][ceil(w/tile_w)]: number of voxels per tile, for the
 * input-sparse first convolution (tile shape from mvx_conv3d_tile_shape).
 * site_bits (optional) u32 [d][h][ceil(w/32)]: one bit per site that holds a voxel.
 */
int mvx_scatter_voxels(const float *feat, const int64_t *coords, float *grid, int32_t n_voxels,
                       int32_t channels, int32_t d, int32_t h, int32_t w, int32_t zero_grid,
                       int32_t *status, int32_t *occupancy, int32_t tile_h, int32_t tile_w,
                       uint32_t *site_bits, void *stream);
int mvx_gather_voxels(const float *grid, const int64_t *coords, float *feat, int32_t n_voxels,
                      int32_t channels, int32_t d, int32_t h, int32_t w, void *stream);

/* CML output -> bird's-eye-view map: the reshape of VoxelNet.py:36, (1,C,D,H,W) -> (1,C*D,H,W).
 *   cl  f32 [d][h][w][channels] (channels-last),  bev f32 [channels*d][h][w], bev channel = c*d_total + d
 *   reverse = 0: cl -> bev (forward);  reverse = 1: bev -> cl (its gradient).  `cl` is written then. */
int mvx_cl_to_bev(const float *cl, float *bev, int32_t d, int32_t h, int32_t w, int32_t channels,
                  int32_t reverse, void *stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm with batch statistics, fused with the preceding ReLU.  Replaces the
 * nn.BatchNorm2d/3d(affine=False, track_running_stats=False) calls of
 * modules/layers/Blocks.py:10,16,25,29 (forward) and their autograd (backward).
 * All matrices are row-major [rows][channels] f32 (channels-last), channels % 4 == 0.
 *
 *   mvx_row_stats       stats (replicated, see MVX_STATS_REPLICAS) = per-channel (sum, sum of squares)
 *   mvx_bn_finalize     mean_inv f32 [2][C] = (mean, 1/sqrt(biased var + eps)), count = #rows
 *   mvx_bn_apply        out = (y - mean) * inv          (out may alias y)
 *   mvx_bn_relu_backward
 *        given dyhat = dL/d(BN output) and y = ReLU output (BN input):
 *        dz = (y > 0) ? inv * (dyhat - mean(dyhat) - yhat * mean(dyhat * yhat)) : 0
 *        dbias (optional) f32 [C] = column sums of dz;  scratch: mvx_bn_backward_scratch_bytes(C)
 *        bytes (replicated f64 accumulators);  dz may alias dyhat.
 *        row_w (optional) f32 [rows]: row r stands for row_w[r] identical rows of the dense tensor
 *        and dyhat[r] is already the SUM of their gradients; `count` is the dense row count.
 */
int mvx_row_stats(const float *y, double *stats, int64_t rows, int32_t channels, void *stream);
int mvx_bn_finalize(const double *stats, double count, double eps, float *mean_inv, int32_t channels,
                    void *stream);
int mvx_bn_apply(const float *y, const float *mean_inv, float *out, int64_t rows, int32_t channels,
                 void *stream);
size_t mvx_bn_backward_scratch_bytes(int32_t channels);
int mvx_bn_relu_backward(const float *dyhat, const float *y, const float *mean_inv, double count,
                         float *dz, float *dbias, double *scratch, const float *row_w, int64_t rows,
                         int32_t channels, int32_t flags, void *stream);

/* ------------------------------------------------------------------------------------------
 * Dense 3x3x3 convolution on the matrix cores (fp32 MFMA), one frame, channels-last
 * activations [D][H][W][C].  Replaces the nn.Conv3d forward/backward that CML obtains from
 * ATen/cuDNN (modules/voxelnet/Pipe.py:36-43, modules/layers/Blocks.py:24,28): kernel 3,
 * stride (stride_d,1,1), padding (pad_d,1,1); cin % 32 == 0, cout % 64 == 0.
 *
 *   mvx_conv3d_pack_weights  torch layout W[cout][cin][3][3][3] -> kernel layout
 *                            (for_dgrad bit 0 = 0: forward operand, 1: transposed/flipped operand; bit 1 set: the source
 *                            is a 2-D kernel W[cout][cin][3][3] = the middle depth slice -- with din = dout = 1 and
 *                            pad_d = 1 the same kernels then evaluate nn.Conv2d 3x3, stride 1, padding 1: the RPN
 *                            blocks of modules/voxelnet/Pipe.py:45-75, next scope row)
 *   mvx_conv3d_forward       out = [ReLU](conv(in) + bias); stats (optional, replicated f64 [R][2][cout]) =
 *                            per-channel (sum, sum of squares) of `out` for the BatchNorm that
 *                            follows (Blocks.py:28-29)
 *   work_counter (optional, forward / dgrad and their _bg / _tiles forms): u32 [1] holding ZERO; the launch then uses
 *                            the persistent form of the kernel -- two workgroups per CU pull (tile, plane, channel block)
 *                            units from this counter until none is left: no tail round of idle CUs, constant-fill tiles do
 *                            not unbalance the workgroups.  NULL: one workgroup per unit.
 *   mvx_conv3d_dgrad         dx [din][h][w][cin] from dz [dout][h][w][cout]
 *   mvx_conv3d_wgrad         dw in torch layout [cout][cin][3][3][3] ([cout][cin][3][3] with MVX_FLAG_CONV2D);
 *                            cout % 64 == 0 when cin % 64 == 0, else cout == 64
 */
size_t mvx_conv3d_packed_weight_bytes(int32_t cout, int32_t cin);
int mvx_conv3d_pack_weights(const float *w, float *wpk, int32_t cout, int32_t cin, int32_t for_dgrad,
                            void *stream);
void mvx_conv3d_tile_shape(int32_t *tile_h, int32_t *tile_w);
int mvx_conv3d_forward(const float *in, const float *wpk, const float *bias, float *out, double *stats,
                       int32_t din, int32_t dout, int32_t h, int32_t w, int32_t cin, int32_t cout,
                       int32_t stride_d, int32_t pad_d, int32_t flags, uint32_t *work_counter, void *stream);
int mvx_conv3d_dgrad(const float *dz, const float *wpk_dgrad, float *dx, int32_t din, int32_t dout,
                     int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t stride_d, int32_t pad_d,
                     uint32_t *work_counter, void *stream);
size_t mvx_conv3d_wgrad_workspace_bytes(int32_t h, int32_t w, int32_t cin, int32_t cout);
int mvx_conv3d_wgrad(const float *in, const float *dz, float *dw, int32_t din, int32_t dout, int32_t h,
                     int32_t w, int32_t cin, int32_t cout, int32_t stride_d, int32_t pad_d, int32_t flags,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Background rewrite of the CML stack (csrc/activity.hip).  The grid VoxelNet.reindex fills
 * (modules/voxelnet/VoxelNet.py:16-22) is zero outside the voxel sites and every CML block is
 * Conv3d -> ReLU -> BatchNorm without affine (modules/voxelnet/Pipe.py:31-43, modules/layers/Blocks.py:20-29),
 * so a site without a voxel in its receptive field holds one per-(plane, channel) constant after each
 * layer.  These entry points describe that background and let forward and wgrad skip it -- exact
 * rewrites of the dense arithmetic, no approximation:
 *
 *   mvx_activity_dilate   dst_mask u8 [dout][h][w] = 1 where the 3x3x3 receptive field holds an active source
 *                         site (src: i32 index grid [din][h][w], -1 = empty, or u8 mask), or, with mark_border,
 *                         where the in-plane window leaves the image (zero padding is not the background);
 *                         dst_halo_flags (optional) i32 [dout][tiles]: the (8+2)x(16+2) halo of the tile holds
 *                         an active site of that plane (tiles as mvx_conv3d_tile_shape)
 *   mvx_conv3d_background bg_pre f32 [dout][cout] = conv of the constant input c_in f32 [din][cin] at an interior
 *                         site (valid depth taps of each plane only); w in torch layout
 *   mvx_bn_background     y_bg = [ReLU](bg_pre + bias), c_out = (y_bg - mean) * inv: the normalised background
 *                         of the layer output, bit-equal to what mvx_bn_apply writes at background sites
 *   mvx_conv3d_forward_bg mvx_conv3d_forward on a source with background: tiles whose halo flags are clear
 *                         (and, with border_active, that do not touch the image border) are filled with the
 *                         constant; background SITES (out_mask == 0) inside computed tiles get it too.
 *                         exec_stages (optional) u64 [1] += executed (depth tap, 32-channel) stages of 4.7 MFLOP
 *   mvx_plane_tap_sums    tap_sums f32 [planes][9][channels]: for each in-plane tap (a,b) the sum of dz over the sites
 *                         whose tap source (y+a-1, x+b-1) lies inside the image (f64 accumulation).  With tile_flags
 *                         + inactive_sums f32 [planes][channels] (both or neither): dz is only defined on the flagged
 *                         tiles (which must include every border tile); the rest of each plane contributes inactive_sums
 *   mvx_tile_dilate_flags out[d][t] = self[d][t] | any 3x3 tile neighbour flagged in an input plane tied to d by a depth
 *                         tap: the tiles of a layer's output gradient that a restricted backward of its consumer reads
 *   mvx_conv3d_wgrad_bg   dw = sum (in - c_in) (x) dz over the tiles with a set halo flag + c_in (x) tap_sums, equal to
 *                         mvx_conv3d_wgrad
 *   mvx_conv3d_input_grad_sums  plane_grad_sums f32 [din][cin] = per input plane, the sum over all its sites of the
 *                         input gradient (what mvx_conv3d_dgrad would write), from tap_sums in closed form
 *   mvx_conv3d_dgrad_tiles      mvx_conv3d_dgrad for the output tiles with dx_tile_flags i32 [din][tiles] set.  An unflagged
 *                         tile is left untouched, except that the 16 x 16-site units of the split forms (_split, which
 *                         pair the tile rows 2k and 2k + 1) also write the unflagged vertical partner of a flagged tile:
 *                         its content is then unspecified (it may be computed from parts of dz the caller left undefined)
 *   mvx_bn_relu_backward_tiles  mvx_bn_relu_backward of a layer whose output is the background (y_bg, c_bg per plane)
 *                         outside the flagged tiles and whose incoming gradient dyhat is only valid ON them:
 *                         the batch sums take the rest from plane_grad_sums; dz is written on the flagged tiles only;
 *                         dz_inactive_sums (optional) f32 [planes][channels] = sum of dz over the other tiles (closed form)
 */
int mvx_activity_dilate(const void *src, int32_t src_is_index, int32_t din, int32_t dout, int32_t h, int32_t w,
                        int32_t stride_d, int32_t pad_d, int32_t mark_border, uint8_t *dst_mask,
                        int32_t *dst_halo_flags, int32_t *dst_tile_flags, void *stream);
/* BatchNorm apply of a layer output with a background: (y - mean) * inv on the tiles whose flag is set (tiles as
 * mvx_conv3d_tile_shape, flags i32 [n_frames * planes][tiles]), the normalised background constant c_bg f32
 * [n_frames * planes][channels] (mvx_bn_background) everywhere else, without reading y there.  Bit-identical to mvx_bn_apply. */
int mvx_bn_apply_tiles_frames(const float *y, const float *mean_inv, const float *c_bg, const int32_t *tile_flags, float *out,
                              int32_t planes, int32_t h, int32_t w, int32_t channels, int32_t n_frames, void *stream);
/* ... that leaves the background tiles no consumer reads unwritten.  read_flags [n_frames * planes][tiles]: mvx_tile_read_flags_frames
 * of the CONSUMING layer (in_halo_flags = this tensor's halo flags, din / dout / stride_d / pad_d = the consumer's depth geometry):
 * non-zero = the consumer's background-aware forward or weight gradient may read the tile (a superset: the 3 x 3 tile neighbourhoods
 * of the output tiles it computes, in every valid source plane). */
int mvx_bn_apply_tiles_read_frames(const float *y, const float *mean_inv, const float *c_bg, const int32_t *tile_flags,
                                   const int32_t *read_flags, float *out, int32_t planes, int32_t h, int32_t w, int32_t channels,
                                   int32_t n_frames, void *stream);
int mvx_tile_read_flags_frames(const int32_t *in_halo_flags, int32_t din, int32_t dout, int32_t h, int32_t w, int32_t stride_d,
                               int32_t pad_d, int32_t *read_flags, int32_t n_frames, void *stream);
/* ... written as the reference's middle output instead: bev [frame][c * planes + d][h][w] (modules/voxelnet/Pipe.py:40-41, the
 * (C, D, H, W) result viewed as (C * D, H, W)); equal to mvx_bn_apply_tiles_frames followed by mvx_cl_to_bev_frames bit for bit,
 * without the channels-last tensor in between.  channels <= 64. */
int mvx_bn_apply_tiles_bev_frames(const float *y, const float *mean_inv, const float *c_bg, const int32_t *tile_flags, float *bev,
                                  int32_t planes, int32_t h, int32_t w, int32_t channels, int32_t n_frames, void *stream);
int mvx_conv3d_background_taps_frames(const float *w, const float *c_in, int32_t din, int32_t dout, int32_t cin, int32_t cout,
                                      int32_t stride_d, int32_t pad_d, float *bg, int32_t n_frames, void *stream);
int mvx_conv3d_background(const float *w, const float *c_in, int32_t din, int32_t dout, int32_t cin, int32_t cout,
                          int32_t stride_d, int32_t pad_d, float *bg_pre, void *stream);
int mvx_bn_background(const float *bg_pre, const float *bias, const float *mean_inv, int32_t planes, int32_t channels,
                      int32_t flags, float *y_bg, float *c_out, void *stream);
int mvx_conv3d_forward_bg(const float *in, const float *wpk, const float *bias, float *out, double *stats,
                          int32_t din, int32_t dout, int32_t h, int32_t w, int32_t cin, int32_t cout,
                          int32_t stride_d, int32_t pad_d, int32_t flags, const int32_t *in_halo_flags,
                          const uint8_t *out_mask, const float *bg_pre, int32_t border_active,
                          uint64_t *exec_stages, uint32_t *done_counter, double count, double eps, float *mean_inv,
                          uint32_t *work_counter, void *stream);
size_t mvx_conv3d_wgrad_bg_workspace_bytes(int32_t dout, int32_t h, int32_t w, int32_t cin, int32_t cout);
int mvx_conv3d_wgrad_bg(const float *in, const float *dz, float *dw, int32_t din, int32_t dout, int32_t h,
                        int32_t w, int32_t cin, int32_t cout, int32_t stride_d, int32_t pad_d, int32_t flags,
                        const int32_t *in_halo_flags, const float *c_in, const float *tap_sums, void *workspace,
                        size_t workspace_bytes, void *stream);
size_t mvx_plane_tap_sums_workspace_bytes(int32_t planes, int32_t channels);
int mvx_plane_tap_sums(const float *dz, int32_t planes, int32_t h, int32_t w, int32_t channels,
                       const int32_t *tile_flags, const float *inactive_sums, float *tap_sums, void *workspace,
                       size_t workspace_bytes, void *stream);
int mvx_tile_dilate_flags(const int32_t *in_tile_flags, const int32_t *self_tile_flags, int32_t din, int32_t dout,
                          int32_t h, int32_t w, int32_t stride_d, int32_t pad_d, int32_t *out_tile_flags, void *stream);
int mvx_conv3d_input_grad_sums(const float *w, const float *tap_sums, int32_t din, int32_t dout, int32_t cin,
                               int32_t cout, int32_t stride_d, int32_t pad_d, float *plane_grad_sums, void *stream);
int mvx_conv3d_dgrad_tiles(const float *dz, const float *wpk_dgrad, float *dx, int32_t din, int32_t dout, int32_t h,
                           int32_t w, int32_t cin, int32_t cout, int32_t stride_d, int32_t pad_d,
                           const int32_t *dx_tile_flags, uint64_t *exec_stages, uint32_t *work_counter, void *stream);
/* bf16x3 forms of the background-aware forward and input gradient (csrc/conv3d_split.hip; weights from
 * mvx_conv3d_pack_weights_split).  The weight gradient in these arithmetics is mvx_conv3d_wgrad_bg* with MVX_FLAG_SPLIT. */
int mvx_conv3d_forward_bg_split(const float *in, const void *wsplit, const float *bias, float *out, double *stats,
                                int32_t din, int32_t dout, int32_t h, int32_t w, int32_t cin, int32_t cout,
                                int32_t stride_d, int32_t pad_d, int32_t flags, const int32_t *in_halo_flags,
                                const uint8_t *out_mask, const float *bg_pre, int32_t border_active, void *stream);
int mvx_conv3d_dgrad_tiles_split(const float *dz, const void *wsplit_dgrad, float *dx, int32_t din, int32_t dout,
                                 int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t stride_d, int32_t pad_d,
                                 int32_t flags, const int32_t *dx_tile_flags, void *stream);
/* ... and their frame-set forms (planes of n_frames frames stacked along depth, per-frame statistics [F][R][2][cout];
 * exec_stages (optional) u64 [1] += executed (depth tap, 32-channel chunk) stages, as in the f32 kernels) */
int mvx_conv3d_forward_bg_split_frames(const float *in, const void *wsplit, const float *bias, float *out, double *stats,
                                       int32_t din, int32_t dout, int32_t h, int32_t w, int32_t cin, int32_t cout,
                                       int32_t stride_d, int32_t pad_d, int32_t flags, const int32_t *in_halo_flags,
                                       const uint8_t *out_mask, const float *bg_pre, int32_t border_active,
                                       uint64_t *exec_stages, int32_t n_frames, void *stream);
int mvx_conv3d_dgrad_tiles_split_frames(const float *dz, const void *wsplit_dgrad, float *dx, int32_t din, int32_t dout,
                                        int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t stride_d, int32_t pad_d,
                                        int32_t flags, const int32_t *dx_tile_flags, uint64_t *exec_stages, int32_t n_frames,
                                        void *stream);
/* bf16x3 forms of the RPN's 2-D forward and input gradient on frame sets (modules/voxelnet/Pipe.py:45-75; one plane per
 * frame).  wsplit: the 2-D kernel placed in the middle depth slice of a [cout][cin][3][3][3] tensor, packed by
 * mvx_conv3d_pack_weights_split.  The weight gradient is mvx_conv2d_wgrad_frames with MVX_FLAG_SPLIT. */
int mvx_conv2d_forward_split_frames(const float *in, const void *wsplit, const float *bias, float *out, double *stats,
                                    int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t flags, int32_t n_frames,
                                    void *stream);
int mvx_conv2d_dgrad_split_frames(const float *dz, const void *wsplit_dgrad, float *dx, int32_t h, int32_t w, int32_t cin,
                                  int32_t cout, int32_t flags, int32_t n_frames, void *stream);
size_t mvx_bn_relu_backward_tiles_workspace_bytes(int32_t planes, int32_t h, int32_t w, int32_t channels);
int mvx_bn_relu_backward_tiles(const float *dyhat, const float *y, const float *mean_inv, const float *c_bg,
                               const float *y_bg, const float *plane_grad_sums, const int32_t *tile_flags,
                               int32_t planes, int32_t h, int32_t w, int32_t channels, float *dz, float *dbias,
                               float *dz_inactive_sums, int32_t flags, void *workspace, size_t workspace_bytes,
                               void *stream);

/* ------------------------------------------------------------------------------------------
 * Row-wise fully connected layer on the matrix cores (fp32 MFMA).  Replaces the nn.Linear /
 * 1x1 nn.Conv2d GEMMs of FCN and CRB2d (modules/layers/Blocks.py:9,14,35,39) and their autograd.
 *   x f32 [rows][ldx] (k columns used), w f32 [n][ldw] (or [k][ldw] when w_transposed),
 *   y f32 [rows][ldy] (n columns written) = [ReLU](x w^T + bias)
 *   stats (optional, replicated f64 [R][2][n]): per-column (sum, sum of squares) of y weighted by row_w
 *   row_w (optional) f32 [rows]: multiplicity of each row in the reference's dense tensor
 *   splitk_workspace (optional, mvx_linear_splitk_workspace_bytes): lets a skinny product without
 *   epilogue (no bias/ReLU/stats, ldy == n, few output blocks, long k) be split along k into slabs
 *   that are summed in a fixed order -- fills the chip when rows x n alone cannot.
 * mvx_linear_wgrad: dw f32 [n][k] = dz^T x  (dz f32 [rows][lddz]).
 * mvx_linear_forward_bn (and the done_counter / count / eps / mean_inv arguments of mvx_conv3d_forward_bg): the
 *   workgroup that finishes last turns the statistics into mean_inv f32 [2][n] (= mvx_bn_finalize) inside the same
 *   launch; done_counter u32 [1] must be zero (cleared here unless MVX_FLAG_PREZEROED).
 */
size_t mvx_linear_splitk_workspace_bytes(int64_t rows, int32_t n);
int mvx_linear_forward_bn(const float *x, int32_t ldx, const float *w, int32_t ldw, int32_t w_transposed,
                          const float *bias, float *y, int32_t ldy, double *stats, const float *row_w, int64_t rows,
                          int32_t k, int32_t n, int32_t flags, uint32_t *done_counter, double count, double eps,
                          float *mean_inv, void *stream);
int mvx_linear_forward(const float *x, int32_t ldx, const float *w, int32_t ldw, int32_t w_transposed,
                       const float *bias, float *y, int32_t ldy, double *stats, const float *row_w,
                       int64_t rows, int32_t k, int32_t n, int32_t flags, void *splitk_workspace,
                       size_t splitk_workspace_bytes, void *stream);
size_t mvx_linear_wgrad_workspace_bytes(int64_t rows, int32_t k, int32_t n);

/* ------------------------------------------------------------------------------------------
 * Row GEMMs on PRE-CUT operands (csrc/rowgemm_pre.hip): the same nn.Linear / 1x1 Conv2d products
 * (modules/layers/Blocks.py:9,14,35,39; the fusion MLP of modules/imhead/Pipe.py:84-104) in the split arithmetics
 * MVX_FLAG_SPLIT3 (three bf16 pieces = the f32 operand exactly, six MFMAs per product) / MVX_FLAG_SPLIT_F16 (two fp16 pieces),
 * with every operand stored as PLANES of 16-bit pieces -- u16 [pieces][rows][k], plane stride rows * k -- by the kernel that
 * produced it, so that the GEMM moves its tiles global -> LDS by DMA and issues nothing but matrix instructions and LDS reads.
 *   mvx_split_planes_bytes     size of the planes of a [rows][k] f32 matrix
 *   mvx_split_rows             f32 [rows][ldx] -> planes (weights, once per optimizer step; any tensor whose producer does not
 *                              write planes itself); `scale` multiplies the values first (fp16 pieces only; a power of two)
 *   mvx_linear_forward_pre_frames  y f32 [rows][ldy] = [ReLU](out_scale * a b^T + bias) from a = planes of x [rows][k] and
 *                              b = planes of the weight [n][k] (input gradient: of the transposed weight), per-frame
 *                              BatchNorm sums / finalisation exactly as mvx_linear_forward_bn_frames; k % 32 == 0
 *   mvx_linear_wgrad_pre       dw f32 [n][k] (+= with MVX_FLAG_ACCUMULATE) = out_scale * dz^T x from the planes of dz [rows][n]
 *                              and x [rows][k]; n % 128 == 0, k % 128 == 0; workspace: mvx_linear_wgrad_pre_workspace_bytes
 */
size_t mvx_split_planes_bytes(int64_t rows, int32_t k, int32_t flags);
int mvx_split_rows(const float *x, int32_t ldx, int64_t rows, int32_t k, void *planes, int32_t flags, float scale, void *stream);
int mvx_linear_forward_pre_frames(const void *a_planes, const void *b_planes, const float *bias, float *y, int32_t ldy,
                                  double *stats, const float *row_w, int64_t rows, int32_t k, int32_t n, int32_t flags,
                                  float out_scale, uint32_t *done_counter, double eps, float *mean_inv,
                                  const mvx_frames_t *frames_host, int32_t row_kind, void *stream);
size_t mvx_linear_wgrad_pre_workspace_bytes(int64_t rows, int32_t k, int32_t n);
int mvx_linear_wgrad_pre(const void *x_planes, const void *dz_planes, float *dw, int64_t rows, int32_t k, int32_t n,
                         int32_t flags, float out_scale, void *workspace, size_t workspace_bytes, void *stream);
/* ... over the rows [row_lo, row_hi) of planes holding plane_rows rows each (workspace of the whole range suffices): the weight
 * gradient of a row range whose dz planes are already written (mvx_bn_relu_backward_planes_part_frames). */
int mvx_linear_wgrad_pre_rows(const void *x_planes, const void *dz_planes, float *dw, int64_t plane_rows, int64_t row_lo,
                              int64_t row_hi, int32_t k, int32_t n, int32_t flags, float out_scale, void *workspace,
                              size_t workspace_bytes, void *stream);
int mvx_linear_wgrad(const float *x, int32_t ldx, const float *dz, int32_t lddz, float *dw, int64_t rows,
                     int32_t k, int32_t n, int32_t flags, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * VFE glue on [n_voxels][t][channels] rows.  Replaces modules/voxelnet/Pipe.py:14-18
 * (BN -> max over t -> repeat -> concat) and modules/voxelnet/VoxelNet.py:30 (max over t),
 * with their autograd.  The max covers all t rows, padded ones included (no mask).
 *   mvx_vfe_bn_max_concat        out [V][t][2C] = [BN(y), max_t BN(y)], argmax i32 [V][C]
 *   mvx_vfe_max_concat_backward  dyhat [V][t][C] from grad_out [V][t][2C]
 *   mvx_bn_segment_max           out [V][C] = max_t BN(y), argmax i32 [V][C]
 *   mvx_segment_max_backward     dyhat [V][t][C] from dfeat [V][C]
 */
int mvx_vfe_bn_max_concat(const float *y, const float *mean_inv, float *out, int32_t *argmax,
                          int32_t n_voxels, int32_t t, int32_t channels, const int32_t *voff,
                          const int32_t *vcnt, int32_t n_real, void *stream);
int mvx_vfe_max_concat_backward(const float *grad_out, const int32_t *argmax, float *dyhat,
                                int32_t n_voxels, int32_t t, int32_t channels, const int32_t *voff,
                                const int32_t *vcnt, int32_t n_real, void *stream);
int mvx_bn_segment_max(const float *y, const float *mean_inv, float *out, int32_t *argmax,
                       int32_t n_voxels, int32_t t, int32_t channels, const int32_t *voff,
                       const int32_t *vcnt, int32_t n_real, void *stream);
int mvx_segment_max_backward(const float *dfeat, const int32_t *argmax, float *dyhat, int32_t n_voxels,
                             int32_t t, int32_t channels, const int32_t *voff, const int32_t *vcnt,
                             int32_t n_real, void *stream);

/* Compact rows: inside MVXNet all padded rows of a voxel are identical, so the t rows
 * of voxel v are stored as its vcnt[v] real rows (matrix rows voff[v] ...) plus ONE padded row
 * (matrix row n_real + v) that stands for the t - vcnt[v] identical padded rows: weight
 * row_w = t - vcnt[v] in the BatchNorm sums, gradient = sum over the rows it stands for.  The four
 * entry points above take voff/vcnt/n_real (NULL/NULL/0 = the dense [V][t][C] layout).
 *   mvx_voxel_row_offsets          row_map (mvx_row_compact_map) -> voff, vcnt i32 [V], row_w f32 [n_real+V]
 *   mvx_vfe_compact_input          VFE-1 input rows [n_real+V][7+F]: real row j = [voxels[rows_sel[j]][0:7],
 *                                  imfeat[j]], padded rows = [0 x 7, imfeat[n_real]]  (MVXNet.py:26)
 *   mvx_vfe_compact_input_backward dimfeat [n_real+1][F] from grad_out [n_real+V][7+F]; scratch f64 [F]
 */
int mvx_voxel_row_offsets(const int32_t *row_map, int32_t n_voxels, int32_t t, int32_t n_real,
                          int32_t *voff, int32_t *vcnt, float *row_w, void *stream);
int mvx_vfe_compact_input(const float *voxels, int32_t vox_channels, const int32_t *rows_sel,
                          const float *imfeat, int32_t feat_channels, int32_t n_real, int32_t n_voxels,
                          float *out, void *stream);
int mvx_vfe_compact_input_backward(const float *grad_out, int32_t feat_channels, int32_t n_real,
                                   int32_t n_voxels, float *dimfeat, double *scratch, void *stream);

/* ------------------------------------------------------------------------------------------
 * Point <-> image fusion sampling.  Replaces featureMaping (modules/imhead/Pipe.py:23-82).
 *   voxels   f32 [rows][vox_channels]  dense (V*T) voxel rows: xyz in columns 0..2, projected
 *            (row, col) in the LAST two columns; rows with x == y == z == 0 are padding and get
 *            all their columns zeroed IN PLACE (Pipe.py:54-59)
 *   feats_host[l]  device pointer of FPN level l, channels-last f32 [h_l][w_l][channels];
 *            feat_hw_host = {h_0, w_0, h_1, w_1, ...} (both arrays live on the HOST)
 *   out      f32 [rows or n_real(+1)][n_levels*channels]: level l in columns [l*C, (l+1)*C)
 *   row_map  NULL: dense output, padded rows written as zeros (Pipe.py:80);
 *            else i32 [rows] from mvx_row_compact_map: only real rows are sampled, into their
 *            compact row; the caller keeps one shared zero row for all padded rows
 *   status   bit0 = a sample index left the (zero-padded) map: the reference's assert, Pipe.py:71
 * mvx_row_compact_map: row_map[r] = rank of real row r among real rows, -1 for padded rows;
 *            rows_sel (optional) i32 [rows]: inverse list; n_real i32 [1] on the device.  Padding rows
 *            (x == y == z == 0) get their channels 3.. zeroed IN PLACE here (Pipe.py:54-59), so that
 * mvx_feature_sample_rows, the compact sampler, only visits the n_real real rows (dense row rows_sel[j]
 *            -> out row j); same arithmetic and status as mvx_feature_sample.
 * mvx_expand_rows / _backward: compact [n][C] <-> dense [rows][C]; every padded row reads the
 *            shared row `pad_row`, whose gradient is the sum over the padded rows (C <= 256;
 *            scratch f64 [C]).
 */
size_t mvx_row_compact_workspace_bytes(int64_t rows);
int mvx_row_compact_map(float *voxels, int32_t vox_channels, int64_t rows, int32_t *row_map,
                        int32_t *rows_sel, int32_t *n_real, void *workspace, size_t workspace_bytes,
                        void *stream);
int mvx_feature_sample(float *voxels, int32_t vox_channels, int64_t rows, const int32_t *row_map,
                       const float *const *feats_host, const int32_t *feat_hw_host, int32_t n_levels,
                       int32_t channels, float imsize_h, float imsize_w, float eps, float *out,
                       int32_t *status, void *stream);
int mvx_feature_sample_rows(const float *voxels, int32_t vox_channels, const int32_t *rows_sel, int32_t n_real,
                            const float *const *feats_host, const int32_t *feat_hw_host, int32_t n_levels,
                            int32_t channels, float imsize_h, float imsize_w, float eps, float *out,
                            int32_t *status, void *stream);
int mvx_expand_rows(const float *compact, const int32_t *row_map, int32_t pad_row, float *out,
                    int64_t rows, int32_t channels, void *stream);
int mvx_expand_rows_backward(const float *grad_out, const int32_t *row_map, int32_t pad_row,
                             float *dcompact, double *scratch, int64_t rows, int32_t channels,
                             void *stream);

/* ------------------------------------------------------------------------------------------
 * Range crop, camera-frustum crop, lidar -> image projection.  Replaces
 * modules/data/Preprocessing.py:12-24 (crop / cropTensor), :26-55 (cropToSight) and
 * modules/utils/Calib.py:47-69 (lidar2Img).
 *
 * mvx_crop_points: order-preserving compaction of the points that pass the enabled filters.
 *   pcd f32 [F][cap_points][ncol], n_in i32 [F] (device, NULL = all cap_points live)
 *   range6_host  (lo xyz, hi xyz) f64 on the HOST or NULL: keep lo <= xyz < hi; bounds_f32 rounds
 *                the bounds to f32 first (cropTensor semantics)
 *   cam_from_velo_host = R0_rect @ Tr_velo_to_cam and p2_host = P2, row-major 4x4 f64 on the HOST,
 *                or NULL: keep cam.z > 0 and 0 <= (u, v) < (imsize_w, imsize_h) - 1e-3;
 *                math_f32 selects the torch-path (f32) arithmetic instead of the numpy-path (f64)
 *   out f32 [F][cap_points][ncol], n_out i32 [F]; src_index (optional) i32 [F][cap_points]
 *   n_in[f] is clamped to cap_points.  n_out[f] = the number of points of frame f that passed; rows of out
 *   at and after n_out[f] are not written, nor are those of src_index.
 * mvx_lidar2img: out[i][col_offset + 0..1] = (u, v), or (v, u) = (row, col) when swap_to_row_col
 *   (train.py:33); cam_z (optional) f32 [n] = depth in the camera frame.
 */
size_t mvx_crop_workspace_bytes(int32_t n_frames, int32_t cap_points);
int mvx_crop_points(const float *pcd, const int32_t *n_in, int32_t n_frames, int32_t cap_points,
                    int32_t ncol, const double *range6_host, int32_t bounds_f32,
                    const double *cam_from_velo_host, const double *p2_host, double imsize_w,
                    double imsize_h, int32_t math_f32, float *out, int32_t *n_out, int32_t *src_index,
                    void *workspace, size_t workspace_bytes, void *stream);
/* mvx_crop_project_points: the per-frame input preparation of the training loop in one compaction pass --
 *   crop + cropToSight with the numpy-path (f64) masks of cropdata.py:30-65, then for every kept point the f32
 *   projection of train.py:31-34 (lidar2Img on the torch path, swapped to (row, col)) appended as two columns:
 *   out f32 [F][cap_out][ncol + 2] = [x y z r ... row col], n_out i32 [F].  cam_from_velo / p2: the f64 matrices of the
 *   masks; proj_*: the matrices of the f32 projection (R0_rect @ Tr_velo_to_cam formed in f32, as torch does).
 *   The input stride is cap_points, the output stride cap_out.  n_out[f] is the number of points that passed, which
 *   may exceed cap_out: only the first cap_out of them, in source order, are stored, and the caller sees the overflow
 *   in the count (every consumer of (out, n_out) takes min(n_out[f], cap_out)). */
size_t mvx_crop_project_workspace_bytes(int32_t n_frames, int32_t cap_points);
int mvx_crop_project_points(const float *pcd, const int32_t *n_in, int32_t n_frames, int32_t cap_points, int32_t ncol,
                            const double *range6_host, const double *cam_from_velo_host, const double *p2_host,
                            double imsize_w, double imsize_h, const double *proj_cam_from_velo_host,
                            const double *proj_p2_host, float *out, int32_t cap_out, int32_t *n_out, void *workspace,
                            size_t workspace_bytes, void *stream);
int mvx_lidar2img(const float *pcd, int32_t ncol, int64_t n_points, const double *cam_from_velo_host,
                  const double *p2_host, int32_t math_f32, float *out, int32_t ld_out, int32_t col_offset,
                  int32_t swap_to_row_col, float *cam_z, void *stream);

/* ------------------------------------------------------------------------------------------
 * Input-sparse first convolution as voxel GEMMs + index-grid gathers (exact up to fp32 summation
 * order).  Replaces VoxelNet.reindex + cml.conv1 (VoxelNet.py:16-22, Pipe.py:36) and their autograd
 * without ever building the 721 MB dense input grid:
 *   mvx_index_grid            grid i32 [d][h][w] = voxel id at occupied sites, -1 elsewhere, followed in the
 *                             same buffer by a coarse per-tile occupancy count (buffer size:
 *                             mvx_index_grid_bytes)
 *   forward:  P = X W_all^T   via mvx_linear_forward (X f32 [V][cin], W_all f32 [27*cout][cin],
 *                             row (kd*9+a*3+b)*cout + co = W[co][:][kd][a][b])
 *             mvx_sparse_conv_output:  out [dout][h][w][cout] = [ReLU](bias + sum of the P rows of the
 *                             <= 27 source voxels of each site), stats as in mvx_conv3d_forward
 *   backward: mvx_sparse_conv_gather_dz:  G f32 [V][27*cout], G[v][tap*cout + c] = dz at the output site
 *                             that read voxel v through tap (zero if none)
 *             dX = G W_all (mvx_linear_forward, w_transposed), dW_all = G^T X (mvx_linear_wgrad)
 */
size_t mvx_index_grid_bytes(int32_t d, int32_t h, int32_t w);
int mvx_index_grid(const int64_t *coords, int32_t n_voxels, int32_t d, int32_t h, int32_t w,
                   int32_t *grid, int32_t *status, void *stream);
int mvx_sparse_conv_output(const float *p, const int32_t *index_grid, const float *bias, float *out,
                           double *stats, int32_t din, int32_t dout, int32_t h, int32_t w, int32_t cout,
                           int32_t stride_d, int32_t pad_d, int32_t flags, void *stream);
int mvx_sparse_conv_gather_dz(const float *dz, const int64_t *coords, int32_t n_voxels, float *g_rows,
                              int32_t din, int32_t dout, int32_t h, int32_t w, int32_t cout,
                              int32_t stride_d, int32_t pad_d, void *stream);

/* ------------------------------------------------------------------------------------------
 * "bf16x3" variants of the dense convolution's forward and input gradient: every f32 operand is split into hi + lo bf16 and a
 * product is hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with f32 accumulation (per-product
 * relative error ~2e-5, i.e. fp32-grade for the 1e-4 feature bar; ~5x the rate of the exact-f32
 * MFMA).  Same arguments and layouts as the f32 entry points; weights are packed (and pre-split) by
 * mvx_conv3d_pack_weights_split into mvx_conv3d_packed_weight_bytes_split(cout, cin, flags) bytes.
 *
 * "bf16x6" (MVX_FLAG_SPLIT3 in `flags` of the pack AND of every call that uses the pack): THREE pieces per operand
 * (hi + mid + lo = the f32 value exactly) and the six products hh + hm + mh + hl + lh + mm; the dropped cross terms are
 * below 2^-25 of a product, i.e. under its f32 rounding: fp32-GRADE accuracy (tests hold it to the bounds of the
 * exact-f32 kernels) at 6/16 of the exact-f32 MFMA's matrix cycles.  Every `flags` below takes MVX_FLAG_SPLIT3.
 *
 * The weight gradient in these arithmetics has no entry point of its own: mvx_conv3d_wgrad with MVX_FLAG_SPLIT (cin a
 * multiple of 64).
 */
size_t mvx_conv3d_packed_weight_bytes_split(int32_t cout, int32_t cin, int32_t flags);
int mvx_conv3d_pack_weights_split(const float *w, void *wsplit, int32_t cout, int32_t cin, int32_t for_dgrad,
                                  int32_t flags, void *stream);
int mvx_conv3d_forward_split(const float *in, const void *wsplit, const float *bias, float *out, double *stats,
                             int32_t din, int32_t dout, int32_t h, int32_t w, int32_t cin, int32_t cout,
                             int32_t stride_d, int32_t pad_d, int32_t flags, void *stream);
int mvx_conv3d_dgrad_split(const float *dz, const void *wsplit_dgrad, float *dx, int32_t din, int32_t dout,
                           int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t stride_d, int32_t pad_d,
                           int32_t flags, void *stream);

/* ------------------------------------------------------------------------------------------
 * Frame-set forms (see mvx_frames_t above): the same operations as the entry points of the same name without `_frames`,
 * for all frames of a step in ONE launch.  Conventions:
 *   - `frames_host` is a HOST pointer (copied by value into the launch); NULL = one frame;
 *   - `n_frames` forms: grids hold the frames stacked along depth -- [n_frames * planes][h][w][c]; din / dout / planes
 *     are PER FRAME; per-plane arrays (background constants, halo / tile flags, tap sums, plane gradient sums) are
 *     indexed by the global plane frame * planes + local plane;
 *   - per-frame results get a leading frame dimension: stats f64 [F][R][2][C], mean_inv f32 [F][2][C];
 *   - bias / weight gradients are summed over the frames (the reference accumulates them over the frames of a step).
 * Row forms take `row_kind` (MVX_ROWS_*).  BatchNorm populations per frame follow from the descriptor
 * (voxels of the frame x t), or, for MVX_ROWS_GRID, rows / n_frames.
 */
int mvx_linear_forward_bn_frames(const float *x, int32_t ldx, const float *w, int32_t ldw, int32_t w_transposed,
                                 const float *bias, float *y, int32_t ldy, double *stats, const float *row_w, int64_t rows,
                                 int32_t k, int32_t n, int32_t flags, uint32_t *done_counter, double eps, float *mean_inv,
                                 const mvx_frames_t *frames_host, int32_t row_kind, void *stream);
int mvx_bn_finalize_frames(const double *stats, double count, double eps, float *mean_inv, int32_t channels,
                           int32_t n_frames, void *stream);
int mvx_bn_apply_frames(const float *y, const float *mean_inv, float *out, int64_t rows, int32_t channels,
                        const mvx_frames_t *frames_host, int32_t row_kind, void *stream);
size_t mvx_bn_backward_scratch_bytes_frames(int32_t channels, int32_t n_frames);
/* A frame without voxels has no population.  Of the row layouts only MVX_ROWS_FUSION still stores a row for it (its shared
 * padded row, weight 0).  Forward: the in-launch finalisations give such a frame mean 0 and inverse deviation 1/sqrt(eps).
 * Backward: with finite mean_inv for that frame and zero dyhat on that row, its dz is exactly 0 and it adds nothing to dbias. */
int mvx_bn_relu_backward_frames(const float *dyhat, const float *y, const float *mean_inv, double count, float *dz,
                                float *dbias, double *scratch, const float *row_w, int64_t rows, int32_t channels,
                                int32_t flags, const mvx_frames_t *frames_host, int32_t row_kind,
                                float *dz_amax /* NULL or 1 float: max |dz| written (mvx_split_operand_amax) */, void *stream);
/* ... with dz written as three planes of bf16 pieces, u16 [3][rows][channels] (hi + mid + lo = dz exactly: the operand format
 * of mvx_linear_wgrad_pre), instead of f32 -- for a layer whose dz only feeds its own weight gradient (modules/imhead/Pipe.py:94:
 * the first fusion layer's input carries no gradient). */
int mvx_bn_relu_backward_planes_frames(const float *dyhat, const float *y, const float *mean_inv, double count, void *dz_planes,
                                       float *dbias, double *scratch, const float *row_w, int64_t rows, int32_t channels,
                                       int32_t flags, const mvx_frames_t *frames_host, int32_t row_kind, float *dz_amax,
                                       void *stream);
/* ... enqueued in nparts calls (part = 0 .. nparts - 1 in this order, same arguments and stream): part 0 runs the reduction pass
 * over all rows and the apply pass of the first row range, part p > 0 the apply pass of its range; part_rows[0..1] (host) receives
 * the rows [lo, hi) whose planes this call writes (the ranges tile [0, rows)).  The step's last weight gradient then runs range by
 * range (mvx_linear_wgrad_pre_rows, side stream) beside the apply pass of the next range instead of after the whole pass.  The bias
 * gradient is complete after the last part. */
int mvx_bn_relu_backward_planes_part_frames(const float *dyhat, const float *y, const float *mean_inv, double count,
                                            void *dz_planes, float *dbias, double *scratch, const float *row_w, int64_t rows,
                                            int32_t channels, int32_t flags, const mvx_frames_t *frames_host, int32_t row_kind,
                                            int32_t part, int32_t nparts, int64_t *part_rows, void *stream);
int mvx_vfe_bn_max_concat_frames(const float *y, const float *mean_inv, float *out, int32_t *argmax, int32_t n_voxels,
                                 int32_t t, int32_t channels, const int32_t *voff, const int32_t *vcnt, int32_t n_real,
                                 const mvx_frames_t *frames_host, void *stream);
int mvx_bn_segment_max_frames(const float *y, const float *mean_inv, float *out, int32_t *argmax, int32_t n_voxels,
                              int32_t t, int32_t channels, const int32_t *voff, const int32_t *vcnt, int32_t n_real,
                              const mvx_frames_t *frames_host, void *stream);
/* fusion_row_w (optional) f32 [n_real + n_frames]: row weights of the MVX_ROWS_FUSION layout (1 for real rows, the number
 * of padded rows of frame f for its shared padded row) */
int mvx_voxel_row_offsets_frames(const int32_t *row_map, int32_t n_voxels, int32_t t, int32_t n_real, int32_t *voff,
                                 int32_t *vcnt, float *row_w, float *fusion_row_w, const mvx_frames_t *frames_host,
                                 void *stream);
/* imfeat / dimfeat: MVX_ROWS_FUSION layout [n_real + n_frames][F]; scratch f64 [n_frames][F] */
int mvx_vfe_compact_input_frames(const float *voxels, int32_t vox_channels, const int32_t *rows_sel, const float *imfeat,
                                 int32_t feat_channels, int32_t n_real, int32_t n_voxels, float *out,
                                 const mvx_frames_t *frames_host, void *stream);
/* ... with a row pitch ld >= 7 + feat_channels (out [n_real + n_voxels][ld], the extra columns zero): a pitch that is a multiple of
 * 4 floats lets mvx_linear_forward* / mvx_linear_wgrad read the rows with 16-byte loads (k = ld, the weight padded with zero columns) */
int mvx_vfe_compact_input_pitch_frames(const float *voxels, int32_t vox_channels, const int32_t *rows_sel, const float *imfeat,
                                       int32_t feat_channels, int32_t n_real, int32_t n_voxels, float *out, int32_t ld,
                                       const mvx_frames_t *frames_host, void *stream);
int mvx_vfe_compact_input_backward_frames(const float *grad_out, int32_t feat_channels, int32_t n_real, int32_t n_voxels,
                                          float *dimfeat, double *scratch, const mvx_frames_t *frames_host, void *stream);
/* voxels of all frames back to back ([vox_off[F]][t][vox_channels]); real_off i32 [n_frames + 1] on the DEVICE receives the
 * real-row offsets of the frames (only vox_off and t of the descriptor are read) */
int mvx_row_compact_map_frames(float *voxels, int32_t vox_channels, int64_t rows, int32_t *row_map, int32_t *rows_sel,
                               int32_t *n_real, void *workspace, size_t workspace_bytes, const mvx_frames_t *frames_host,
                               int32_t *real_off, void *stream);
/* feats_host[f * n_levels + l] = level l of frame f (every frame has the same level shapes) */
int mvx_feature_sample_rows_frames(const float *voxels, int32_t vox_channels, const int32_t *rows_sel, int32_t n_real,
                                   const float *const *feats_host, const int32_t *feat_hw_host, int32_t n_levels,
                                   int32_t channels, float imsize_h, float imsize_w, float eps, float *out, int32_t *status,
                                   const mvx_frames_t *frames_host,
                                   float *out_amax /* NULL, or 1 float RAISED to max |out| (zero it first): mvx_split_operand_amax */, void *stream);
/* ... which also writes the rows as planes of bf16 pieces, u16 [3][plane_rows][n_levels * channels] (rows [0, n_real): hi + mid +
 * lo = the f32 value exactly; the caller clears the other rows): what mvx_split_rows would make of `out`, without reading it back.
 * out may be NULL: planes only (both readers of the rows -- mvx_linear_forward_pre_frames, mvx_linear_wgrad_pre -- take planes) */
int mvx_feature_sample_rows_planes_frames(const float *voxels, int32_t vox_channels, const int32_t *rows_sel, int32_t n_real,
                                          const float *const *feats_host, const int32_t *feat_hw_host, int32_t n_levels,
                                          int32_t channels, float imsize_h, float imsize_w, float eps, float *out, int32_t *status,
                                          const mvx_frames_t *frames_host, float *out_amax, void *planes, int64_t plane_rows,
                                          void *stream);
/* coords of all frames back to back; the frame of voxel v follows from vox_off (coords[:,0] is not read) */
size_t mvx_index_grid_bytes_frames(int32_t d, int32_t h, int32_t w, int32_t n_frames);
int mvx_index_grid_frames(const int64_t *coords, int32_t n_voxels, int32_t d, int32_t h, int32_t w, int32_t *grid,
                          int32_t *status, const mvx_frames_t *frames_host, void *stream);
int mvx_sparse_conv_output_frames(const float *p, const int32_t *index_grid, const float *bias, float *out, double *stats,
                                  int32_t din, int32_t dout, int32_t h, int32_t w, int32_t cout, int32_t stride_d,
                                  int32_t pad_d, int32_t flags, int32_t n_frames, void *stream);
/* ... told which 8 x 16 tiles of the OUTPUT hold a site with a voxel under its taps (the tile flags mvx_activity_dilate_frames forms
 * from the index grid, [n_frames * dout][tiles]): only those are built, the rest is ReLU(bias) (written, or implied under
 * MVX_FLAG_NO_BG_FILL); the BatchNorm sums count the rest in closed form as before. */
int mvx_sparse_conv_output_tiles_frames(const float *p, const int32_t *index_grid, const float *bias, float *out, double *stats,
                                        int32_t din, int32_t dout, int32_t h, int32_t w, int32_t cout, int32_t stride_d,
                                        int32_t pad_d, int32_t flags, int32_t n_frames, const int32_t *tile_flags, void *stream);
int mvx_sparse_conv_gather_dz_frames(const float *dz, const int64_t *coords, int32_t n_voxels, float *g_rows, int32_t din,
                                     int32_t dout, int32_t h, int32_t w, int32_t cout, int32_t stride_d, int32_t pad_d,
                                     const mvx_frames_t *frames_host, void *stream);
int mvx_activity_dilate_frames(const void *src, int32_t src_is_index, int32_t din, int32_t dout, int32_t h, int32_t w,
                               int32_t stride_d, int32_t pad_d, int32_t mark_border, uint8_t *dst_mask,
                               int32_t *dst_halo_flags, int32_t *dst_tile_flags, int32_t n_frames, void *stream);
int mvx_tile_dilate_flags_frames(const int32_t *in_tile_flags, const int32_t *self_tile_flags, int32_t din, int32_t dout,
                                 int32_t h, int32_t w, int32_t stride_d, int32_t pad_d, int32_t *out_tile_flags,
                                 int32_t n_frames, void *stream);
int mvx_conv3d_background_frames(const float *w, const float *c_in, int32_t din, int32_t dout, int32_t cin, int32_t cout,
                                 int32_t stride_d, int32_t pad_d, float *bg_pre, int32_t n_frames, void *stream);
int mvx_bn_background_frames(const float *bg_pre, const float *bias, const float *mean_inv, int32_t planes, int32_t channels,
                             int32_t flags, float *y_bg, float *c_out, int32_t n_frames, void *stream);
int mvx_conv3d_forward_bg_frames(const float *in, const float *wpk, const float *bias, float *out, double *stats,
                                 int32_t din, int32_t dout, int32_t h, int32_t w, int32_t cin, int32_t cout,
                                 int32_t stride_d, int32_t pad_d, int32_t flags, const int32_t *in_halo_flags,
                                 const uint8_t *out_mask, const float *bg_pre, int32_t border_active, uint64_t *exec_stages,
                                 uint32_t *done_counter, double count, double eps, float *mean_inv, uint32_t *work_counter,
                                 int32_t n_frames, void *stream);
int mvx_conv3d_dgrad_tiles_frames(const float *dz, const float *wpk_dgrad, float *dx, int32_t din, int32_t dout, int32_t h,
                                  int32_t w, int32_t cin, int32_t cout, int32_t stride_d, int32_t pad_d,
                                  const int32_t *dx_tile_flags, uint64_t *exec_stages, uint32_t *work_counter,
                                  int32_t n_frames, void *stream);
int mvx_conv3d_input_grad_sums_frames(const float *w, const float *tap_sums, int32_t din, int32_t dout, int32_t cin,
                                      int32_t cout, int32_t stride_d, int32_t pad_d, float *plane_grad_sums,
                                      int32_t n_frames, void *stream);
size_t mvx_conv3d_wgrad_bg_workspace_bytes_frames(int32_t dout, int32_t h, int32_t w, int32_t cin, int32_t cout,
                                                  int32_t n_frames);
int mvx_conv3d_wgrad_bg_frames(const float *in, const float *dz, float *dw, int32_t din, int32_t dout, int32_t h, int32_t w,
                               int32_t cin, int32_t cout, int32_t stride_d, int32_t pad_d, int32_t flags,
                               const int32_t *in_halo_flags, const float *c_in, const float *tap_sums, void *workspace,
                               size_t workspace_bytes, int32_t n_frames, void *stream);
size_t mvx_bn_relu_backward_tiles_workspace_bytes_frames(int32_t planes, int32_t h, int32_t w, int32_t channels,
                                                         int32_t n_frames);
int mvx_bn_relu_backward_tiles_frames(const float *dyhat, const float *y, const float *mean_inv, const float *c_bg,
                                      const float *y_bg, const float *plane_grad_sums, const int32_t *tile_flags,
                                      int32_t planes, int32_t h, int32_t w, int32_t channels, float *dz, float *dbias,
                                      float *dz_inactive_sums, float *dz_amax /* NULL or 1 float: max |dz| written */,
                                      int32_t flags, void *workspace, size_t workspace_bytes, int32_t n_frames, void *stream);
/* cl f32 [n_frames * d][h][w][c]  <->  bev f32 [n_frames][c * d][h][w] */
int mvx_cl_to_bev_frames(const float *cl, float *bev, int32_t d, int32_t h, int32_t w, int32_t channels, int32_t reverse,
                         int32_t n_frames, void *stream);
/* one (C*D, H, W) map -> `copies` channels-last frames [copies][d][h][w][channels], one pass: a gradient of the middle output that
 * is shared by all frames of a step, in the layout and multiplicity the frame-set backward reads */
int mvx_bev_to_cl_broadcast(const float *bev, float *cl, int32_t d, int32_t h, int32_t w, int32_t channels, int32_t copies,
                            void *stream);

/* ------------------------------------------------------------------------------------------
 * Region proposal network on frame sets.  Replaces what RPN.forward and its autograd obtain from
 * ATen / MIOpen (modules/voxelnet/Pipe.py:45-75; CRB2d / DeCRB2d of modules/layers/Blocks.py:31-51): maps are
 * channels-last [n_frames][h][w][c] f32, BatchNorm statistics per frame.
 *
 *   mvx_conv2d_forward_frames  out = [ReLU](conv3x3(in) + bias), stride 1, padding 1; stats / in-kernel finalisation as
 *                              mvx_conv3d_forward_bg_frames (count = h * w per frame).  wpk from mvx_conv3d_pack_weights with
 *                              bit 1 of for_dgrad set (2-D source kernel).  MVX_FLAG_TAPS2: only taps {0,1}^2 carry weight:
 *                              a stride-2 3x3 convolution (padding 1) of an image X equals this 2x2-window convolution of
 *                              space_to_depth(X) with the weight rearranged as W2[co][(pr,pc,ci)][ta][tb] = W[co][ci][a][b],
 *                              a -> (ta, pr): 0 -> (0,1), 1 -> (1,0), 2 -> (1,1), likewise b -> (tb, pc).  Only 9 of the 16
 *                              (window tap, parity) blocks of W2 hold a kernel tap; the other 7 are zero BY THIS DEFINITION
 *                              and the three kernels do not execute them (forward / dgrad / wgrad run the true 9-tap FLOPs,
 *                              the weight gradient of those blocks is returned as zero).
 *   mvx_conv2d_dgrad_frames    dx from dz (flipped window {1,2}^2 under MVX_FLAG_TAPS2)
 *   mvx_conv2d_wgrad_frames    dw f32 [cout][cin][3][3] summed over all frames; cin % 64 == 0, cout % 64 == 0
 *   mvx_space_to_depth_frames  in [F*planes][h][w][c] -> out [F][h/2][w/2][4][planes][c], channel block p = 2*(y&1) + (x&1)
 *                              (reverse != 0: the inverse, `in` is the space-to-depth tensor and `out` the full one)
 *   mvx_d2s_bn_apply_frames    t [F][h][w][s*s][c] (row-GEMM output of a ConvTranspose2d with kernel = stride = s, column
 *                              order (i, j, co)) -> out[f][y*s+i][x*s+j][col_offset + co] = (t - mean_f) * inv_f with rows of
 *                              ld_out floats (mean_inv NULL: copy); reverse != 0: t is WRITTEN from the out slice
 *   mvx_bn_apply_strided_frames  y [rows][c] dense -> out rows of ld_out floats at col_offset (frames = equal row shares);
 *                              reverse != 0: y is WRITTEN from the out slice
 *   mvx_row_stats_frames       stats f64 [F][R][2][c] of y [F][rows / F][c]
 */
int mvx_conv2d_forward_frames(const float *in, const float *wpk, const float *bias, float *out, double *stats, int32_t h,
                              int32_t w, int32_t cin, int32_t cout, int32_t flags, uint32_t *done_counter, double eps,
                              float *mean_inv, uint32_t *work_counter, int32_t n_frames, void *stream);
int mvx_conv2d_dgrad_frames(const float *dz, const float *wpk_dgrad, float *dx, int32_t h, int32_t w, int32_t cin,
                            int32_t cout, int32_t flags, uint32_t *work_counter, int32_t n_frames, void *stream);
size_t mvx_conv2d_wgrad_workspace_bytes_frames(int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t n_frames);
int mvx_conv2d_wgrad_frames(const float *in, const float *dz, float *dw, int32_t h, int32_t w, int32_t cin, int32_t cout,
                            int32_t flags, void *workspace, size_t workspace_bytes, int32_t n_frames, void *stream);
int mvx_space_to_depth_frames(const float *in, float *out, int32_t n_frames, int32_t planes, int32_t h, int32_t w,
                              int32_t channels, int32_t reverse, void *stream);
int mvx_d2s_bn_apply_frames(float *t, const float *mean_inv, float *out, int32_t n_frames, int32_t h, int32_t w, int32_t s,
                            int32_t channels, int32_t ld_out, int32_t col_offset, int32_t reverse, void *stream);
int mvx_bn_apply_strided_frames(float *y, const float *mean_inv, float *out, int64_t rows, int32_t channels, int32_t ld_out,
                                int32_t col_offset, int32_t n_frames, int32_t reverse, void *stream);
int mvx_row_stats_frames(const float *y, double *stats, int64_t rows, int32_t channels, int32_t n_frames, void *stream);

/* ------------------------------------------------------------------------------------------
 * Target assignment and loss.
 *
 * mvx_bbox_pairwise: cpp.bboxOverlap / cpp.bboxIntersection (cpp/voxelutil.cpp:96-136; callers
 *   modules/augment/Augment.py:54).  boxes f32 [n][4][2] BEV corner points -> out f32 [n1][n2]: IoU (want_iou != 0)
 *   or intersection area, with the reference's origin-fan clipping arithmetic in f32.  The reference fills r2[j]
 *   (box index) instead of r2[k] (corner index) at :107-109 -- out of bounds beyond 5 boxes; computed here is what its
 *   callers expect, box i against box j.
 *
 * mvx_classify_anchors: cpp._classifyAnchors (cpp/voxelutil.cpp:138-316; modules/Calc.py:88-96; train.py:46).
 *   gts f32 [n_gt][4][2], anchors f32 [l][w][anchors_per_loc][4][2] (BEV corners), nls / nws i64 [n_gt] = centre cell of
 *   every ground truth (Calc.py:91-94).  Output, in the reference's visiting order (ground truth, orientation, rows
 *   up then down, columns right then left):
 *     pos_idx i64 [3][cap] (x, y, z of the positives: IoU >= pos_thr), gi i64 [cap] their ground-truth ids,
 *     neg_idx i64 [3][cap] (the NOT-negative anchors: IoU >= neg_thr, positives included), counts i32 [2] on the device.
 *   window_radius R (1..55): the walk is replayed inside a (2R+1)^2 window of cells around the centre; R must cover
 *   every cell with IoU >= 0.1 (half the sum of the two box diagonals / cell size).  status i32 [1] (OR-ed): 1 = the walk
 *   reached the window edge (raise R), 2 = cap exceeded, 4 = a centre cell outside the grid (ground truth skipped;
 *   the reference indexes out of bounds there).
 *   One documented difference: when the reference's crossing test fails on a near-degenerate edge (|s2 - s1| <= 1e-6,
 *   :44) its static scratch keeps a point from an EARLIER call; this library takes the edge's start point instead.  On
 *   the degenerate pairs of tests/targets_cases.py that fill stays within 5e-8 (IoU) / 9e-6 m^2 (intersection) of the
 *   geometric truth, where a leftover point is off by up to 0.28 m^2.
 *   A second one: the reference puts the SIGNED shoelace areas of the two boxes into the union (:105,110,112), so a
 *   clockwise quad turns the union negative (IoU -1 for a box against itself); this library (mvx_bbox_pairwise, the anchor
 *   walk, NMS and the augmentations alike) takes the magnitudes.  Counter-clockwise quads, which is what Calc.bbox3d2bev
 *   produces, give the reference's result bit for bit.  Against the geometric truth the IoU is good to 7.4e-5 within the
 *   KITTI range (the error of the f32 origin fan grows with the distance from the origin; below 1e-5 within 40 m).
 * mvx_classify_anchors_frames: the same for the frames of a step in ONE walk launch (train.py:46 once per frame): gts / nls /
 *   nws hold the ground truths of all frames back to back, gt_off_host i32 [n_frames + 1] (HOST memory, read during the
 *   call) their offsets; frame f's lists go to pos_idx[f][3][cap], neg_idx[f][3][cap], gi[f][cap] (ground-truth ids local
 *   to the frame) and counts[f][2]; status is OR-ed over the frames.  workspace: the _workspace_bytes of the TOTAL count.
 *
 * mvx_voxel_loss: VoxelLoss forward + backward (modules/voxelnet/Loss.py:15-45; train.py:140,161).
 *   score f32 (l, w, anchors_per_loc) and reg f32 (l, w, 7*anchors_per_loc) through explicit element strides (the RPN's
 *   (1,2,L,W) / (1,14,L,W) maps are read in place); pos_idx / neg_idx / gi as above with leading dimensions pos_ld /
 *   neg_ld; gts f32 [n][gt_ld >= 7] xyzlwhr, anchors f32 [l][w][anchors_per_loc][7].
 *   losses f32 [2] = (clsLoss, regLoss); dscore / dreg (optional) = d(clsLoss)/dscore and d(regLoss)/dreg written through
 *   their own strides -- dreg must be ZERO on entry (only positive anchors receive a gradient; repeated anchors add up).
 *   n_pos = 0: regLoss = 0 (the reference returns None); n_pos = n_neg = 0 is the `pi is None` branch (Loss.py:17-19).
 *   counts_dev (optional) i32 [2]: read n_pos / n_neg from the device instead (forward only: dscore must be NULL).
 *   scratch f64 [4].
 */
int mvx_bbox_pairwise(const float *boxes1, int32_t n1, const float *boxes2, int32_t n2, int32_t want_iou, float *out,
                      void *stream);
size_t mvx_classify_anchors_workspace_bytes(int32_t n_gt, int32_t anchors_per_loc, int32_t window_radius);
int mvx_classify_anchors(const float *gts, int32_t n_gt, const float *anchors, int32_t l, int32_t w,
                         int32_t anchors_per_loc, const int64_t *nls, const int64_t *nws, float neg_thr, float pos_thr,
                         int32_t window_radius, int64_t *pos_idx, int64_t *neg_idx, int64_t *gi, int64_t cap,
                         int32_t *counts, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
int mvx_classify_anchors_frames(const float *gts, const int32_t *gt_off_host, int32_t n_frames, const float *anchors, int32_t l,
                                int32_t w, int32_t anchors_per_loc, const int64_t *nls, const int64_t *nws, float neg_thr,
                                float pos_thr, int32_t window_radius, int64_t *pos_idx, int64_t *neg_idx, int64_t *gi,
                                int64_t cap, int32_t *counts, int32_t *status, void *workspace, size_t workspace_bytes,
                                void *stream);
/* Max-IoU anchor assignment (csrc/assign.hip).  The reference has none: its rule is mvx_classify_anchors.
 * Per frame, iou(g, a) = mvx_bbox_pairwise(gts, anchors, 1)[g][a], or 0 where the two bounding circles are apart:
 *   positive: max_g iou(g, a) >= pos_thr, matched to the lowest g attaining it; or a = the best anchor (lowest flat index
 *     (x * w + y) * anchors_per_loc + z) of a ground truth whose best IoU is >= force_thr -- several ground truths on one
 *     anchor: the largest IoU, ties the lowest g; a forced match overrides the threshold match.  force_thr > 1.5: no forcing.
 *   not negative: max_g iou(g, a) >= neg_thr, plus every positive.
 * mvx_assign_anchors_frames: gts f32 [G_total][4][2] of all frames back to back, gt_off_host i32 [n_frames + 1] (HOST memory),
 *   anchors f32 [l][w][anchors_per_loc][4][2], a regular grid.  No centre cells: they are found on the device, and a centre
 *   outside the grid only clips the window.  0 < neg_thr <= pos_thr, force_thr > 0, window_radius 1..55.  Output per frame f, every
 *   anchor at most once per list, in ascending flat index: pos_idx i64 [f][3][cap], gi i64 [f][cap] (local to the frame),
 *   neg_idx i64 [f][3][cap] (the NOT-negative anchors), counts i32 [f][2]; gt_best f32 [G_total] = the best IoU of every
 *   ground truth.  status i32 [1], zero on entry, OR-ed: 1 = for some box the window could not be shown to give the result of
 *   all anchors against all boxes (raise window_radius and replay; the lists are then not to be used), 2 = a list is longer
 *   than cap (counts clipped, nothing written past cap).  Five launches and one memset for any n_frames and G_total; bitwise
 *   reproducible.  G_total = 0: counts are zeroed, nothing else is touched.
 */
size_t mvx_assign_anchors_frames_workspace_bytes(int32_t n_gt_total, int32_t n_frames, int32_t l, int32_t w,
                                                 int32_t anchors_per_loc);
int mvx_assign_anchors_frames(const float *gts, const int32_t *gt_off_host, int32_t n_frames, const float *anchors, int32_t l,
                              int32_t w, int32_t anchors_per_loc, float neg_thr, float pos_thr, float force_thr,
                              int32_t window_radius, int64_t *pos_idx, int64_t *neg_idx, int64_t *gi, int64_t cap,
                              int32_t *counts, float *gt_best, int32_t *status, void *workspace, size_t workspace_bytes,
                              void *stream);
/* Ignore regions for anchor targets (csrc/ignore.hip).  The reference has none.  Both losses give an anchor that
 * neg_idx (the NOT-negative anchors) lists and pos_idx does not no classification loss; these two calls put more anchors there.
 *
 * mvx_box_point_counts_frames: counts i32 [n_boxes_total] = the points inside every box, all frames in one launch and one memset.
 *   points6 f32 [n_frames][cap_points][ld >= 3] (x y z first), n_points i32 [n_frames] on the device (taken as
 *   min(max(n, 0), cap_points); rows at or beyond it are never read), boxes f32 [n_boxes_total][7] xyzlwhr (z = bottom face) of
 *   all frames back to back, gt_off i32 [n_frames + 1] on the DEVICE.  The decision is the f64 one of the GT-database crop and
 *   the per-object augmentation (csrc/box3d.h, edges inclusive; cos / sin of the yaw in f64).  Integer sums: bitwise
 *   reproducible.  No host read.  n_boxes_total = 0: nothing is touched.
 *
 * mvx_ignore_anchors_frames: rewrites the lists of mvx_assign_anchors_frames (pos_idx / neg_idx i64 [n_frames][3][cap], gi i64
 *   [n_frames][cap], counts i32 [n_frames][2], all on the device, every anchor at most once per list; entries beyond a frame's
 *   count are never read, an entry outside the grid is skipped).  Per frame f, anchors_per_loc 1..4:
 *     sparse:    a box g of the frame with gt_points[gt_off[f] + g] < min_points (gt_points i32 [G_total] and gt_off i32
 *                [n_frames + 1] on the device; gt_points NULL: no box is sparse).
 *     demotion:  a pos_idx entry whose gi names a sparse box leaves the positive list and stays not negative; no rematch.
 *     rectangle: an anchor not yet not negative becomes not negative when its centre (x, y, z + h/2) of anchors f32
 *                [l][w][A][7], through M = img_from_lidar f64 [n_frames][3][4] as
 *                    row_r = ((M[r][0] * x + M[r][1] * y) + M[r][2] * (z + h / 2)) + M[r][3]      (f64, no fused multiply-add)
 *                has row_2 > 0 and (row_0 / row_2, row_1 / row_2) inside one of rects f32 [R_total][4] = (x1, y1, x2, y2) pixels
 *                of the frame (rect_off i32 [n_frames + 1] on the device), edges inclusive.  rects NULL: none.
 *     box:       an anchor still not not negative becomes not negative when, for a quad b of ign_quads f32 [B_total][4][2] of the
 *                frame (ign_off i32 [n_frames + 1] on the device), inter(b, a) >= ioa_thr * area(a) in f32: inter =
 *                mvx_bbox_pairwise(b, a, 0) on anchor_quads f32 [l][w][A][4][2], or 0 where the two bounding circles are apart;
 *                area(a) = the magnitude of the f32 shoelace area.  Intersection over the ANCHOR's area.  ign_quads NULL: none.
 *   Out: pos_out / neg_out i64 [n_frames][3][cap_out], gi_out i64 [n_frames][cap_out] (local to the unchanged box array),
 *   counts_out i32 [n_frames][2]: the kept positives and the union of the not-negative anchors, every anchor at most once, in
 *   ascending flat index; stats i32 [n_frames][4] = (demoted positives, anchors newly ignored by a rectangle, newly ignored by a
 *   box only, sparse boxes); status i32 [1], OR-ed: 2 = a list is longer than cap_out (counts clipped, nothing written past it).
 *   With no source at all the output lists equal the input lists.  Four launches and one memset for any n_frames; integer
 *   atomics only: bitwise reproducible.  MVX_EINVAL before any launch: a NULL required pointer (gt_off with gt_points, rect_off
 *   and img_from_lidar with rects, ign_off with ign_quads), n_frames outside 1..MVX_MAX_FRAMES, anchors_per_loc outside 1..4,
 *   cap or cap_out < 1, ioa_thr outside (0, 1], min_points < 0, a workspace smaller than
 *   mvx_ignore_anchors_frames_workspace_bytes(n_frames, l, w, anchors_per_loc).
 */
int mvx_box_point_counts_frames(const float *points6, int32_t n_frames, int32_t cap_points, int32_t ld, const int32_t *n_points,
                                const float *boxes, const int32_t *gt_off, int32_t n_boxes_total, int32_t *counts, void *stream);
size_t mvx_ignore_anchors_frames_workspace_bytes(int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc);
int mvx_ignore_anchors_frames(const int64_t *pos_idx, const int64_t *neg_idx, const int64_t *gi, int64_t cap,
                              const int32_t *counts, int32_t n_frames, const int32_t *gt_off, const int32_t *gt_points,
                              int32_t min_points, const float *anchors, const float *anchor_quads, int32_t l, int32_t w,
                              int32_t anchors_per_loc, const float *rects, const int32_t *rect_off,
                              const double *img_from_lidar, const float *ign_quads, const int32_t *ign_off, float ioa_thr,
                              int64_t *pos_out, int64_t *neg_out, int64_t *gi_out, int64_t cap_out, int32_t *counts_out,
                              int32_t *stats, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
int mvx_voxel_loss(const float *score, int64_t score_sl, int64_t score_sw, int64_t score_sa, const float *reg,
                   int64_t reg_sl, int64_t reg_sw, int64_t reg_sc, const int64_t *pos_idx, int64_t pos_ld,
                   const int64_t *neg_idx, int64_t neg_ld, const int64_t *gi, const int32_t *counts_dev, int32_t n_pos,
                   int32_t n_neg, const float *gts, int32_t gt_ld, const float *anchors, int32_t l, int32_t w,
                   int32_t anchors_per_loc, float a, float b, float eps, float *dscore, int64_t dscore_sl,
                   int64_t dscore_sw, int64_t dscore_sa, float *dreg, int64_t dreg_sl, int64_t dreg_sw, int64_t dreg_sc,
                   float *losses, double *scratch, void *stream);

/* ------------------------------------------------------------------------------------------
 * Focal loss of the RPN heads for the frames of a step (csrc/loss_frames.hip).  The reference has none: its
 * VoxelLoss is a plain log loss.  Forward + backward of all frames in three launches and one memset, for any n_frames.
 *
 * mvx_focal_loss_frames: per frame f < n_frames (1..MVX_MAX_FRAMES), A = anchors_per_loc (1..4):
 *   heads f32 [n_frames*l*w][8A] contiguous, 16-byte aligned, a row = [A cls logits | 7A regression]: the raw output of the
 *     heads (rpn_frames.rpn_forward, 16 wide), logits and not probabilities;
 *   pos_idx / neg_idx i64 [n_frames][3][cap], gi i64 [n_frames][cap], counts i32 [n_frames][2] = (n_pos, n_notneg) on the
 *     device: what mvx_classify_anchors_frames writes.  Entries beyond a frame's count are never read; a count is taken as
 *     min(max(count, 0), cap); an entry outside the grid (or a gi outside the frame's boxes) is skipped;
 *   gts f32 [n][gt_ld >= 7] xyzlwhr, the boxes of all frames back to back, gt_off i32 [n_frames + 1] on the DEVICE the first
 *     row of every frame (gi is local to the frame); anchors f32 [l][w][A][7].
 *   By set membership: an anchor is positive when pos_idx lists it at least once, ignored when neg_idx (the NOT-negative
 *   anchors) lists it and it is not positive, negative otherwise.  With x a logit, p = sigmoid(x), N_f = max(1, n_pos):
 *     cls_f = cls_weight / N_f * ( sum_positive alpha (1-p)^gamma (-log p) + sum_negative (1-alpha) p^gamma (-log(1-p)) )
 *     reg_f = reg_weight * mvx_voxel_loss's regLoss (its targets, SmoothL1 with beta 1, once per pos_idx entry, mean over
 *             n_pos*7; 0 when n_pos = 0)
 *   all from the logit (softplus forms, accurate expf / log1pf), per-frame sums in f64.
 *   losses f32 [n_frames][2] = (cls_f, reg_f).  d_heads (optional; 16-byte aligned, layout of heads) = d(cls_f + reg_f)/d(row),
 *   with respect to the LOGITS, zero on ignored anchors; written in full, so it need not be zero on entry.
 *   workspace: mvx_focal_loss_frames_workspace_bytes(n_frames, l, w, anchors_per_loc) bytes, 8-byte aligned (0 for a shape the
 *   call rejects; pure host code).  MVX_EINVAL before any launch: a NULL required pointer, n_frames or anchors_per_loc outside
 *   their ranges, cap < 1, gt_ld < 7, alpha outside [0, 1], gamma < 0, a workspace that is too small.
 *   No host read, no f64 atomic: losses are bitwise reproducible, and d_heads too whenever pos_idx lists no anchor twice (the
 *   regression columns are float atomicAdd-ed per entry).
 */
int64_t mvx_focal_loss_frames_workspace_bytes(int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc);
int mvx_focal_loss_frames(const float *heads, int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc,
                          const int64_t *pos_idx, const int64_t *neg_idx, const int64_t *gi, int64_t cap,
                          const int32_t *counts, const float *gts, int32_t gt_ld, const int32_t *gt_off,
                          const float *anchors, float alpha, float gamma, float cls_weight, float reg_weight,
                          float *d_heads, float *losses, void *workspace, int64_t workspace_bytes, void *stream);

/* mvx_focal_loss_dir_frames: mvx_focal_loss_frames with a direction classifier (SECOND / PointPillars), the
 * same three launches and memset.  Rows carry explicit strides: heads f32 rows of heads_ld >= 8A floats (a multiple of 4, base
 * 16-byte aligned) whose first 8A columns are mvx_focal_loss_frames's; d_heads (optional) rows of d_heads_ld floats, written
 * in full: every column beyond 8A is zero unless the direction gradient lives there.  The direction logits and their gradient
 * come as pointer + row stride, dir[row*dir_ld + a] for anchor a < A of BEV cell row: columns of the head rows (dir = heads +
 * 8A, dir_ld = heads_ld) or a tensor of their own; d_dir likewise (given exactly when d_heads is; outside the d_heads rows its
 * A columns per row are zeroed first, further columns are left alone).  Per pos_idx entry (anchor a, box g, direction logit x;
 * entries the regression term skips are skipped, duplicates count every time):
 *   angle column:  SmoothL1(sin D) with D = r6 - (g6 - an6) in place of SmoothL1(D), same mean and reg_weight; gradient
 *                  reg_weight / (n_pos*7) * SmoothL1'(sin D) * cos D;
 *   direction bit: b = floor(mod(g6 - dir_offset, 2 pi) / pi) in {0, 1};
 *   dir_f = dir_weight / max(1, n_pos) * sum (b ? softplus(-x) : softplus(x)), gradient dir_weight / max(1, n_pos) * (sigmoid(x) - b).
 * The classification term and regression columns 0..5 are mvx_focal_loss_frames's (the cls loss and gradient bit for bit).
 * losses f32 [n_frames][3] = (cls_f, reg_f, dir_f).  workspace: mvx_focal_loss_dir_frames_workspace_bytes(n_frames, l, w,
 * anchors_per_loc, d_heads_ld) bytes (pass heads_ld without d_heads).  Reproducibility as mvx_focal_loss_frames.
 */
int64_t mvx_focal_loss_dir_frames_workspace_bytes(int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc,
                                                  int32_t d_heads_ld);
int mvx_focal_loss_dir_frames(const float *heads, int32_t heads_ld, const float *dir, int32_t dir_ld, int32_t n_frames, int32_t l,
                              int32_t w, int32_t anchors_per_loc, const int64_t *pos_idx, const int64_t *neg_idx,
                              const int64_t *gi, int64_t cap, const int32_t *counts, const float *gts, int32_t gt_ld,
                              const int32_t *gt_off, const float *anchors, float alpha, float gamma, float cls_weight,
                              float reg_weight, float dir_weight, float dir_offset, float *d_heads, int32_t d_heads_ld,
                              float *d_dir, int32_t d_dir_ld, float *losses, void *workspace, int64_t workspace_bytes,
                              void *stream);

/* mvx_focal_loss_iou_frames: mvx_focal_loss_dir_frames with an IoU-aware confidence head (CIA-SSD, AFDetV2, CenterPoint's second
 * stage): one more launch (the memset plus four, for any F).  The IoU logits and their gradient come as pointer +
 * row stride exactly like the direction logits: iou[row*iou_ld + a], columns of the head rows (iou = heads + 9A, iou_ld =
 * heads_ld) or a tensor of their own; d_iou likewise (given exactly when d_heads is; outside the d_heads rows its A columns per
 * row are zeroed first).  Per pos_idx entry (anchor a, box g, IoU logit x, the anchor's regression row r read as a constant;
 * entries the regression term skips are skipped, duplicates count every time):
 *   b = the 'loss' decode of mvx_detect_frames: b0,1 = r0,1 * sqrt(an3^2 + an4^2) + an0,1, b2 = r2 an5 + an2, b3..5 = exp(r3..5)
 *       an3..5, b6 = r6 + an6 (no direction fold: a rectangle is blind to it);
 *   I = BEV intersection of the quads of b and g in the f32 arithmetic of the NMS, exactly 0 when their bounding circles
 *       cannot touch; ih = min(b2 + b5, g2 + g5) - max(b2, g2) (z is the bottom face);
 *   q = clamp(I ih / (b3 b4 b5 + g3 g4 g5 - I ih), 0, 1): the 3D IoU; 0 when ih <= 0, when a component of b (or g) is not
 *       finite, or when the quotient is not finite;
 *   iou_f = iou_weight / max(1, n_pos) * sum (softplus(x) - q x), gradient iou_weight / max(1, n_pos) * (sigmoid(x) - q).
 * Nothing flows into the regression columns from this term.  The cls, reg and dir terms and their gradient columns are
 * mvx_focal_loss_dir_frames's bit for bit.  iou_weight >= 0.  losses f32 [n_frames][4] = (cls_f, reg_f, dir_f, iou_f).
 * q_out (optional) f32 [n_frames][cap]: q of every pos_idx entry, -1 for skipped entries and for the slots beyond the count.
 * workspace: mvx_focal_loss_iou_frames_workspace_bytes(n_frames, l, w, anchors_per_loc, d_heads_ld, cap) bytes: the direction
 * entry's plus n_frames * min(ceil(cap / 128), 64) doubles.  The four losses are bitwise reproducible, the gradient whenever
 * no anchor is listed twice in pos_idx.
 */
int64_t mvx_focal_loss_iou_frames_workspace_bytes(int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc,
                                                  int32_t d_heads_ld, int64_t cap);
int mvx_focal_loss_iou_frames(const float *heads, int32_t heads_ld, const float *dir, int32_t dir_ld, const float *iou,
                              int32_t iou_ld, int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc,
                              const int64_t *pos_idx, const int64_t *neg_idx, const int64_t *gi, int64_t cap,
                              const int32_t *counts, const float *gts, int32_t gt_ld, const int32_t *gt_off,
                              const float *anchors, float alpha, float gamma, float cls_weight, float reg_weight,
                              float dir_weight, float dir_offset, float iou_weight, float *d_heads, int32_t d_heads_ld,
                              float *d_dir, int32_t d_dir_ld, float *d_iou, int32_t d_iou_ld, float *q_out, float *losses,
                              void *workspace, int64_t workspace_bytes, void *stream);

/* mvx_box_iou_loss_frames: the rotated 3D IoU regression loss 1 - IoU3D (Zhou et al., 3DV 2019; SE-SSD's ODIoU, mmdetection3d's
 * RotatedIoU3DLoss; csrc/box_iou_loss.hip) with its analytic gradient, for the frames of a step in ONE launch:
 * no workspace, no host read.  heads (rows of heads_ld >= 8A floats, a multiple of 4, base 16-byte aligned), the lists, boxes
 * and anchors are mvx_focal_loss_dir_frames's; neg_idx is not needed.  Per pos_idx entry of frame f (anchor a, box g, the
 * anchor's regression row r; an entry outside the grid or with gi outside the frame's boxes is skipped, duplicates count every
 * time):
 *   b  = the 'loss' decode of mvx_detect_frames (see mvx_focal_loss_iou_frames), g = the ground-truth row, z the bottom face;
 *   ih = min(b2 + b5, g2 + g5) - max(b2, g2);
 *   I  = BEV intersection area of the two rectangles (clockwise yaw: a corner (px, py) of the box lies at
 *        (px c + py s, -px s + py c) + (x, y)), by an exact convex clip in the predicted box's own frame;
 *   V = I ih, U = b3 b4 b5 + g3 g4 g5 - V, q = clamp(V / U, 0, 1); q = 0 with a zero gradient when ih <= 0, when a component of
 *   b or g is not finite, or when the rectangles do not overlap.
 *   out f32 [n_frames][2] = (weight / max(1, n_pos) * sum (1 - q), mean q over the entries taken or 0), sums in f64 in a fixed
 *   order: bitwise reproducible.
 *   d_heads (optional) rows of d_heads_ld floats (>= 8A, base 4-byte aligned): d(term)/d(r) is ADDED (float atomicAdd) into
 *   the anchor's seven regression columns, nothing else is touched; bitwise reproducible when no anchor is listed twice.
 *   loss_add (optional): the frame's term is added to loss_add[f * loss_add_ld] (column 1 of the focal losses).
 *   q_out (optional) f32 [n_frames][cap]: q per pos_idx slot, -1 for skipped entries and for the slots beyond the count.
 * MVX_EINVAL before any launch: a NULL required pointer, n_frames, anchors_per_loc or cap outside their ranges, gt_ld < 7, a
 * row stride below 8A (heads_ld also not a multiple of 4) or rows beyond 2^31 floats, weight < 0 or NaN, loss_add_ld < 1 with
 * loss_add, a misaligned pointer.
 */
int mvx_box_iou_loss_frames(const float *heads, int32_t heads_ld, int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc,
                            const int64_t *pos_idx, const int64_t *gi, int64_t cap, const int32_t *counts, const float *gts,
                            int32_t gt_ld, const int32_t *gt_off, const float *anchors, float weight, float *d_heads,
                            int32_t d_heads_ld, float *loss_add, int32_t loss_add_ld, float *out, float *q_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Detection output (csrc/detect.hip): score selection, top-K, box decoding and rotated BEV NMS for the frames of a step.
 * The reference has none of it (its Calc.decodeRegression is never called).
 *
 * mvx_detect_frames: per frame f < n_frames (1..MVX_MAX_FRAMES), on the raw head output read in place through element
 *   strides (frame, x, y, channel):
 *     cls  f32 logits of anchor a at cls[f*cls_sf + x*cls_sl + y*cls_sw + a*cls_sa];
 *     reg  f32 regression k of anchor a at reg[f*reg_sf + x*reg_sl + y*reg_sw + (a*7 + k)*reg_sc] (voxelnet/Loss.py:42);
 *   the frame-set heads (F*l*w, 16) = [cls (2) | reg (14)] of rpn_frames.rpn_forward are cls = heads, reg = heads + 2,
 *   strides (l*w*16, w*16, 16, 1); NCHW maps (F,2,l,w) / (F,14,l,w) are (C*l*w, w, 1, l*w).
 *   anchors f32 [l][w][anchors_per_loc][7] xyzlwhr (Preprocessing.createAnchors); anchor index n = (x*w + y)*A + a.
 *   1. candidates: anchors with sigmoid(logit) >= score_thr (computed in the kernel), the first pre_max of them in the
 *      order logit descending, then anchor index ascending (a total order: the result is deterministic);
 *   2. decode (decode = MVX_DETECT_DECODE_LOSS): the exact inverse of VoxelLoss's targets (voxelnet/Loss.py:35-40),
 *        d = sqrt(l_a^2 + w_a^2); x = r0*d + x_a, y = r1*d + y_a, z = r2*h_a + z_a, (l, w, h) = exp(r3..5) * (l_a, w_a, h_a),
 *        yaw = r6 + yaw_a;
 *      MVX_DETECT_DECODE_REFERENCE: Calc.decodeRegression as the reference wrote it, d = sqrt(x_a^2 + y_a^2) (anchor columns
 *      0:2; a trained model does not match it).  BEV corners as Calc.bbox3d2bev.  A candidate with a non-finite decoded
 *      component is dropped (status bit MVX_DETECT_NONFINITE);
 *   3. greedy NMS in candidate order: j is suppressed by a kept i < j when IoU(i, j) > iou_thr (strict), IoU with
 *      bboxOverlap's arithmetic (mvx_bbox_pairwise, boxes i against j); pairs whose bounding circles cannot touch count
 *      as IoU 0 (the clipping there gives rounding noise of ~1e-6 only).  At most post_max boxes are kept.
 *   Outputs (device): boxes f32 [n_frames][post_max][7] xyzlwhr, scores f32 [n_frames][post_max] = sigmoid(logit),
 *   anchor_idx i32 [n_frames][post_max] (n), counts i32 [n_frames] kept boxes (the rest padded with 0 / index -1),
 *   n_candidates i32 [n_frames] = anchors that passed score_thr, before the pre_max truncation, status i32 [n_frames]:
 *   MVX_DETECT_TRUNCATED (informational) | MVX_DETECT_NONFINITE.  Optional debug outputs (all three or none):
 *   dbg_idx i32 [n_frames][pre_max] the sorted candidates' anchor indices (-1 beyond min(n_candidates, pre_max)),
 *   dbg_boxes f32 [n_frames][pre_max][7] their decoded boxes, dbg_corners f32 [n_frames][pre_max][4][2] their corners.
 *   Limits (MVX_EINVAL before any launch): 1 <= pre_max <= MVX_DETECT_MAX_PRE, 1 <= post_max <= pre_max,
 *   1e-3 <= iou_thr < 1, 0 <= score_thr < 1, non-NULL inputs / outputs, a 256-byte aligned workspace of
 *   mvx_detect_workspace_bytes(n_frames, l*w*anchors_per_loc, pre_max) bytes.  Four launches for all frames, no float
 *   atomics (bitwise reproducible), no host synchronisation.
 */
#define MVX_DETECT_MAX_PRE 4096
#define MVX_DETECT_DECODE_LOSS 0
#define MVX_DETECT_DECODE_REFERENCE 1
#define MVX_DETECT_TRUNCATED 1
#define MVX_DETECT_NONFINITE 2
size_t mvx_detect_workspace_bytes(int32_t n_frames, int32_t n_anchors, int32_t pre_max);
int mvx_detect_frames(const float *cls, int64_t cls_sf, int64_t cls_sl, int64_t cls_sw, int64_t cls_sa, const float *reg,
                      int64_t reg_sf, int64_t reg_sl, int64_t reg_sw, int64_t reg_sc, const float *anchors, int32_t n_frames,
                      int32_t l, int32_t w, int32_t anchors_per_loc, float score_thr, float iou_thr, int32_t pre_max,
                      int32_t post_max, int32_t decode, float *boxes, float *scores, int32_t *anchor_idx, int32_t *counts,
                      int32_t *n_candidates, int32_t *status, int32_t *dbg_idx, float *dbg_boxes, float *dbg_corners,
                      void *workspace, size_t workspace_bytes, void *stream);
/* mvx_detect_frames_dir: mvx_detect_frames plus a fourth head, the direction logit of anchor a at dir[f*dir_sf + x*dir_sl +
 * y*dir_sw + a*dir_sa] (what mvx_focal_loss_dir_frames trains), and dir_offset.  After yaw = r6 + yaw_a the decode computes
 *   base = (yaw - dir_offset) - floor((yaw - dir_offset) / pi) * pi,  yaw' = base + dir_offset + pi * [logit > 0],
 * wraps yaw' into [-pi, pi) and uses it for the corners, the NMS and the output: for a perfect regression and a correct bit
 * yaw' = g6 (mod 2 pi), also when the regression is half a turn off.  A non-finite yaw is left as it is and sets
 * MVX_DETECT_NONFINITE.  dir = NULL is mvx_detect_frames bit for bit (which calls this).
 */
int mvx_detect_frames_dir(const float *cls, int64_t cls_sf, int64_t cls_sl, int64_t cls_sw, int64_t cls_sa, const float *reg,
                          int64_t reg_sf, int64_t reg_sl, int64_t reg_sw, int64_t reg_sc, const float *dir, int64_t dir_sf,
                          int64_t dir_sl, int64_t dir_sw, int64_t dir_sa, float dir_offset, const float *anchors,
                          int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc, float score_thr, float iou_thr,
                          int32_t pre_max, int32_t post_max, int32_t decode, float *boxes, float *scores, int32_t *anchor_idx,
                          int32_t *counts, int32_t *n_candidates, int32_t *status, int32_t *dbg_idx, float *dbg_boxes,
                          float *dbg_corners, void *workspace, size_t workspace_bytes, void *stream);
/* mvx_detect_frames_iou: mvx_detect_frames_dir plus a fifth head, the IoU logit u of anchor a at iou[f*iou_sf + x*iou_sl +
 * y*iou_sw + a*iou_sa] (what mvx_focal_loss_iou_frames trains), and iou_alpha = a in [0, 1] (anything else, a NaN included, is
 * MVX_EINVAL before any launch).  The score becomes cls^(1-a) iou^a, formed from the logits as its logarithm
 *   s = -((1 - a) softplus(-c) + a softplus(-u)):
 * an anchor is a candidate when expf(s) >= score_thr (a NaN fails), candidates are ordered by s (ties: lowest anchor index
 * first) and the score written out is expf(s).  Boxes, direction fold, NMS and outputs are mvx_detect_frames_dir's.  iou = NULL
 * or iou_alpha = 0 is mvx_detect_frames_dir bit for bit (which calls this); the head is not read then.
 */
int mvx_detect_frames_iou(const float *cls, int64_t cls_sf, int64_t cls_sl, int64_t cls_sw, int64_t cls_sa, const float *reg,
                          int64_t reg_sf, int64_t reg_sl, int64_t reg_sw, int64_t reg_sc, const float *dir, int64_t dir_sf,
                          int64_t dir_sl, int64_t dir_sw, int64_t dir_sa, float dir_offset, const float *iou, int64_t iou_sf,
                          int64_t iou_sl, int64_t iou_sw, int64_t iou_sa, float iou_alpha, const float *anchors,
                          int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc, float score_thr, float iou_thr,
                          int32_t pre_max, int32_t post_max, int32_t decode, float *boxes, float *scores, int32_t *anchor_idx,
                          int32_t *counts, int32_t *n_candidates, int32_t *status, int32_t *dbg_idx, float *dbg_boxes,
                          float *dbg_corners, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Test-time augmentation, the fusion of the views' detections (csrc/tta.hip).  The reference has none of it.
 *
 * A view is a row (phi, s, flip, 0) as Geometry.draw_geometry writes `glob`, applied to the cloud by mvx_geom_points_frames'
 * global step; the detection step then runs over n_frames * n_views frames, view-major inside a source frame: frame
 * f * n_views + v is view v of source frame f.
 *
 * mvx_tta_fuse_frames: inputs (device) are that step's padded output,
 *     boxes f32 [n_frames * n_views][post_max][7] xyzlwhr, scores f32 [n_frames * n_views][post_max], counts i32
 *     [n_frames * n_views] (clamped to 0..post_max), each view's list in its own order, and views f32 [n_views][4].
 *   1. tta_merge: every box back into the source frame, the inverse of Geometry.transform_boxes, in f64 from the f32 inputs
 *      and rounded to f32 once: with the flip y <- -y and r <- -r; (x, y) <- ((x, y) @ R(-phi)) / s, z <- z / s,
 *      (l, w, h) <- (l, w, h) / s, r <- r - phi wrapped into [-pi, pi).  A row that is exactly (0, 1, 0) copies its boxes
 *      bitwise.  The N = n_views * post_max entries are ordered by score descending, then view, then rank ascending (a total
 *      order).  BEV corners and bounding circle as mvx_detect_frames forms them.  An entry with a non-finite box or score is
 *      dropped and sets MVX_TTA_NONFINITE.
 *   2. tta_mask: for every pair j > i in merged order ONE IoU (bboxOverlap's arithmetic; pairs whose bounding circles cannot
 *      touch count as IoU 0) gives two bits: sup = IoU > iou_thr, vote = IoU > fuse_iou.  Pairs of the same view are pairs
 *      like any other.
 *   3. tta_fuse: entry i is a HEAD iff no earlier head has its sup bit on i; every other entry belongs to the first head that
 *      suppresses it.  A member votes for its head iff its vote bit with that head is set and no earlier entry of its view
 *      has voted for that head; the head votes first, for its own view.  With weights w = score and the sums over the voters
 *      in merged order, in f64: x y z l w h = sum(w q) / sum(w); d_j = r_j - r_head wrapped into [-pi/2, pi/2), with
 *      full_turn != 0 into [-pi, pi); r = r_head + sum(w d) / sum(w) wrapped into [-pi, pi); rounded to f32 once.  A cluster
 *      whose only voter is its head (or whose weights do not sum to a positive number) copies the head's box bitwise.  Fused
 *      score = (sum of the voters' scores) / n_views in f64, rounded once: with n_views = 1 the head's score bitwise.
 *      Clusters with fewer than min_views voters are dropped; the rest are ordered by fused score descending, then head
 *      position ascending, and the first out_max are written.
 *   The heads are exactly the boxes a greedy NMS over the union of the views keeps, in their original poses.  Averaging moves
 *   them, so IoU <= iou_thr holds for the heads and not strictly for the fused poses.  For car-shaped boxes a fuse_iou above
 *   roughly 0.26 excludes voters a quarter turn off their head, so the half-turn wrap never sits near its seam.  The callers'
 *   defaults fuse_iou = 0.5 and min_views = 1 are design choices, not measured optima.
 *   Outputs (device), per source frame: out_boxes f32 [n_frames][out_max][7], out_scores f32 [n_frames][out_max],
 *   out_n_views i32 [n_frames][out_max] the voters of the cluster, out_src i32 [n_frames][out_max] = view * post_max + rank of
 *   the cluster's head, out_counts i32 [n_frames] (the rest padded with 0 / src -1), status i32 [n_frames]
 *   (MVX_TTA_NONFINITE).
 *   Limits (MVX_EINVAL before any launch): 1 <= n_frames <= MVX_MAX_FRAMES, 1 <= n_views <= MVX_TTA_MAX_VIEWS,
 *   n_views * post_max <= MVX_TTA_MAX_BOXES, 1e-3 <= iou_thr <= fuse_iou < 1, 1 <= min_views <= n_views,
 *   1 <= out_max <= n_views * post_max, non-NULL inputs / outputs, a 256-byte aligned workspace of
 *   mvx_tta_workspace_bytes(n_frames, n_views, post_max) bytes (0 for sizes outside the limits).  Three launches whatever
 *   n_frames and n_views are, no float atomics, every sum in a fixed order (bitwise reproducible), no host synchronisation.
 */
#define MVX_TTA_MAX_VIEWS 8
#define MVX_TTA_MAX_BOXES 1024
#define MVX_TTA_NONFINITE 2
size_t mvx_tta_workspace_bytes(int32_t n_frames, int32_t n_views, int32_t post_max);
int mvx_tta_fuse_frames(const float *boxes, const float *scores, const int32_t *counts, const float *views, int32_t n_frames,
                        int32_t n_views, int32_t post_max, float iou_thr, float fuse_iou, int32_t min_views, int32_t out_max,
                        int32_t full_turn, float *out_boxes, float *out_scores, int32_t *out_n_views, int32_t *out_src,
                        int32_t *out_counts, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * KITTI object evaluation (csrc/kitti_eval.hip): AP for 2D bbox, BEV and 3D, plus AOS, in the semantics of the widely used
 * kitti-object-eval-python tool as DESIGN.md section 3.17 states them.  The reference has no evaluation.
 *
 * All frames of an evaluation in one flat layout (F = n_frames >= 1, no MVX_MAX_FRAMES limit):
 *   off_host (host) / off (device) i32 [3][F+1]: offsets of the detection, GT and don't-care rows of every frame (each
 *     starting at 0); per frame at most MVX_DETECT_MAX_PRE detections and MVX_KITTI_MAX_GT GT plus don't-care rows;
 *   pair_off i64 [3][F+1] (device): prefix sums over the frames of nd*ng, nd*nc and min(nd, ng) (TP score slots);
 *   det_rows / gt_rows f64 [n][8] = x1 y1 x2 y2 l w h y (2-D box; camera-frame size and bottom y), dc_rows f64 [n][4];
 *   det_quads / gt_quads f32 [n][4][2]: BEV corner quads in the (x, z) plane; scores / det_alpha / gt_alpha f64 [n];
 *   curves: curve_host (host) i32 [n_curves][2] = (metric 0 = 2D / 1 = BEV / 2 = 3D, flag set), min_overlap_host (host)
 *     f64 [n_curves] in [0, 1), 1 <= n_curves <= MVX_KITTI_MAX_CURVES;
 *   ignored_gt / ignored_det i8 [n_sets][n_gt] / [n_sets][n_det]: the cleaning flags (-1 / 0 / 1) of every flag set.
 * mvx_kitti_eval_overlaps: overlaps f64 [3][n_pairs], frame f's pair (GT g, detection d) at pair_off[0][f] + g*nd + d;
 *   2D IoU, BEV IoU = I / (l_d w_d + l_g w_g - I) with I the f32 rotated intersection of the quads (bev_iou.h, 0 when the
 *   bounding circles cannot touch), 3D IoU over the vertical extents [y - h, y]; dc_overlaps f64 at pair_off[1][f] + k*nd + d:
 *   2-D intersection over the detection's area.
 * mvx_kitti_eval_tp_scores: the threshold pass (compute_fp = false) of every (frame, curve): tp_scores f64
 *   [n_curves][pair_off[2][F]] holds the TP scores of frame f from pair_off[2][f] on, -inf in the unused slots;
 *   n_valid_gt i32 [n_curves][F].  The caller sorts every curve's row in descending order for:
 * mvx_kitti_eval_thresholds: get_thresholds of every curve: thresholds f64 [n_curves][MVX_KITTI_THRESHOLDS] (0-padded),
 *   n_thresholds i32 [n_curves], n_gt i32 [n_curves] = valid GTs summed over the frames.
 * mvx_kitti_eval_counts: compute_fp = true for every (frame, curve, threshold), per-frame results in a 256-byte aligned
 *   workspace of mvx_kitti_eval_workspace_bytes(n_frames, n_curves) bytes, summed over the frames in a fixed order:
 *   totals i32 [n_curves][MVX_KITTI_THRESHOLDS][3] = (tp, fp, fn), similarity f64 [n_curves][MVX_KITTI_THRESHOLDS] (AOS,
 *   2D curves only; 0 elsewhere); thresholds beyond n_thresholds give zeros.
 * Argument errors, a frame over the limits included, return MVX_EINVAL before any launch.  No atomics (bitwise
 * reproducible), no host synchronisation.
 */
#define MVX_KITTI_MAX_GT 1024
#define MVX_KITTI_MAX_CURVES 72
#define MVX_KITTI_THRESHOLDS 41
size_t mvx_kitti_eval_workspace_bytes(int32_t n_frames, int32_t n_curves);
int mvx_kitti_eval_overlaps(int32_t n_frames, const int32_t *off_host, const int32_t *off, const int64_t *pair_off,
                            const double *det_rows, const float *det_quads, const double *gt_rows, const float *gt_quads,
                            const double *dc_rows, double *overlaps, double *dc_overlaps, void *stream);
int mvx_kitti_eval_tp_scores(int32_t n_frames, const int32_t *off_host, const int32_t *off, const int64_t *pair_off,
                             int32_t n_curves, const int32_t *curve_host, const double *min_overlap_host, int32_t n_sets,
                             const int8_t *ignored_gt, const int8_t *ignored_det, const double *scores, const double *overlaps,
                             double *tp_scores, int32_t *n_valid_gt, void *stream);
int mvx_kitti_eval_thresholds(int32_t n_frames, int32_t n_curves, int64_t n_slots, const double *sorted_scores,
                              const int32_t *n_valid_gt, double *thresholds, int32_t *n_thresholds, int32_t *n_gt, void *stream);
int mvx_kitti_eval_counts(int32_t n_frames, const int32_t *off_host, const int32_t *off, const int64_t *pair_off,
                          int32_t n_curves, const int32_t *curve_host, const double *min_overlap_host, int32_t n_sets,
                          const int8_t *ignored_gt, const int8_t *ignored_det, const double *scores, const double *det_alpha,
                          const double *gt_alpha, const double *overlaps, const double *dc_overlaps, const double *thresholds,
                          const int32_t *n_thresholds, int32_t *totals, double *similarity, void *workspace,
                          size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * GT-paste augmentation (csrc/augment.hip): the reference's modules/augment/Augment.py (check / locate / augment, called
 * by train.py:28) plus the concatenation of train.py:37-42, for the frames of a step (1..MVX_MAX_FRAMES) in four launches.
 * The host draws the random numbers (candidates and thresholds per slot, in the reference's order); the kernels decide.
 *
 * The object database is a set of device-resident flat tables over n_db objects (modules/augment/LoadGT.GTDatabase):
 *   db_box2d f32 [n_db][4] x1 y1 x2 y2, db_box3d f32 [n_db][7] xyzlwhr, db_bev f32 [n_db][4][2] (Calc.bbox3d2bev of db_box3d),
 *   db_points f32 [sum][6] = x y z r row col with pt_off i64 [n_db + 1] (row offsets),
 *   patch u8 [sum_px][3], mask u8 [sum_px] (zero / non-zero) with px_off i64 [n_db + 1] (pixel offsets) and maskbbox i32
 *   [n_db][4] = x1 y1 x2 y2 inclusive in image pixels: object k's patch is (y2-y1+1) rows of (x2-x1+1) pixels.
 *
 * mvx_gt_paste_ground_frames: zmax f32 [n_frames][grid_h][grid_w] (mvx_gt_paste_workspace_bytes bytes) = the largest z of
 *   the scene points points6 f32 [n_frames][cap_points][6] (the first n_points[f] rows) of every cell, cells without a point
 *   hold (float)(lo_z - 1).  Cell of a point: (int)(((double)x - lo_x) / ((hi_x - lo_x) / grid_h)), the same for y (Augment.py:16-17).
 *   Points outside [lo, hi) in x or y, or with a NaN z, are skipped (the reference indexes out of bounds); -0 counts as +0.
 *   A fill and ONE kernel; integer atomics on the f32 bit patterns (the maximum is exact and order-independent).
 * mvx_gt_paste_place_frames: one workgroup per frame.  The frame's scene boxes box2d f32 [n_frames][cap][4], box3d
 *   [n_frames][cap][7], bev [n_frames][cap][4][2] hold n_scene[f] rows on entry and n_out[f] rows on return (grown in place).
 *   A frame with n_scene[f] > lim gets nothing; otherwise S = lim - n_scene[f] slots run in sequence (S <= s_max).  Slot s
 *   tests its candidates cand i32 [n_frames][s_max][n_cand] (database indices, -1 = none) in order and takes the first that
 *   passes:  test 0 (ground): cell (int)((x - lo_x) / cell), (int)((y - lo_y) / cell) in f32 (a true division); rejected when
 *   the cell is outside the grid or zmax[cell] > z + z_margin;  with no scene box so far the candidate is accepted here;
 *   test 1 (2-D): rejected when max_i inter(box2d_i, candidate) / area(box2d_i) > thr[f][s] (f32, utils/Bbox.py);
 *   test 2 (BEV): rejected when max_i IoU(candidate bev, bev_i) > iou_thr, IoU as mvx_bbox_pairwise(candidate, box i);
 *   pairs whose bounding circles cannot touch count as IoU 0.  The winner's three boxes are appended, so later slots test
 *   against it.  picked i32 [n_frames][s_max] = its database index or -1.  Optional debug outputs (both or none):
 *   dbg_fail i32 [n_frames][s_max][n_cand] = the first failing test 0..2, 3 = passes all, -1 = no candidate / slot not run;
 *   dbg_val f32 [n_frames][s_max][n_cand][3] = (zmax of the cell, max 2-D ratio, max IoU).
 * mvx_gt_paste_points_frames: appends the rows of every picked object, in slot order, behind the n_points[f] scene rows of
 *   points6[f]; n_points_out[f] (a different array) = the new count.  An object that does not fit cap_points is dropped as
 *   a whole and reported.  points6 and db_points 16-byte aligned.
 * mvx_gt_paste_image_frames: img u8 [n_frames][h][w][3]: for every picked object in slot order img = mask ? patch : img over
 *   its maskbbox, clipped to the image; a later slot overwrites an earlier one.  max_patch_px: the largest patch of the
 *   database in pixels (sizes the grid).
 * status i32 [n_frames] (OR-ed into, zero it first): MVX_GT_PASTE_POINTS_OVERFLOW, MVX_GT_PASTE_BAD_COUNT (n_scene outside
 *   0..cap: frame untouched), MVX_GT_PASTE_SLOTS_SHORT (lim - n_scene > s_max: only s_max slots ran), MVX_GT_PASTE_BAD_INDEX
 *   (a candidate index >= n_db, treated as none).  Argument errors return MVX_EINVAL before any launch.  No float atomics
 *   (bitwise reproducible), no host synchronisation.
 */
#define MVX_GT_PASTE_MAX_BOXES 32
#define MVX_GT_PASTE_MAX_CAND 32
#define MVX_GT_PASTE_MAX_SLOTS 32
#define MVX_GT_PASTE_POINTS_OVERFLOW 1
#define MVX_GT_PASTE_BAD_COUNT 2
#define MVX_GT_PASTE_SLOTS_SHORT 4
#define MVX_GT_PASTE_BAD_INDEX 8
size_t mvx_gt_paste_workspace_bytes(int32_t n_frames, int32_t grid_h, int32_t grid_w);
int mvx_gt_paste_ground_frames(const float *points6, const int32_t *n_points, int32_t n_frames, int32_t cap_points, double lo_x,
                               double lo_y, double lo_z, double hi_x, double hi_y, int32_t grid_h, int32_t grid_w, float *zmax,
                               size_t zmax_bytes, void *stream);
int mvx_gt_paste_place_frames(const float *zmax, int32_t grid_h, int32_t grid_w, float lo_x, float lo_y, float cell, float z_margin,
                              float iou_thr, float *box2d, float *box3d, float *bev, const int32_t *n_scene, int32_t n_frames,
                              int32_t cap, int32_t lim, const int32_t *cand, const float *thr, int32_t s_max, int32_t n_cand,
                              const float *db_box2d, const float *db_box3d, const float *db_bev, int32_t n_db, int32_t *picked,
                              int32_t *n_out, int32_t *status, int32_t *dbg_fail, float *dbg_val, void *stream);
int mvx_gt_paste_points_frames(float *points6, const int32_t *n_points, int32_t *n_points_out, int32_t n_frames,
                               int32_t cap_points, const int32_t *picked, int32_t s_max, const float *db_points,
                               const int64_t *pt_off, int32_t n_db, int32_t *status, void *stream);
int mvx_gt_paste_image_frames(uint8_t *img, int32_t n_frames, int32_t h, int32_t w, const int32_t *picked, int32_t s_max,
                              const uint8_t *patch, const uint8_t *mask, const int64_t *px_off, const int32_t *maskbbox,
                              int32_t n_db, int64_t max_patch_px, void *stream);

/* ------------------------------------------------------------------------------------------
 * Geometric augmentation (csrc/geom_augment.hip) for the frames of a step (1..MVX_MAX_FRAMES): the per-object noise, global
 * scaling and global rotation of VoxelNet section 3.2 and the y flip of the common MVX-Net recipes, then the range filter.  The
 * host draws every random number: noise f32 [n_frames][cap_boxes][n_trials][4] = (dx, dy, dz, dtheta) per box slot and trial,
 * glob f32 [n_frames][4] = (phi, s, flip != 0, unused).  Rotations are Calc.getRotationMatrices' R(a) = [[cos a, -sin a],
 * [sin a, cos a]] on row vectors (qx = px cos a + py sin a, qy = -px sin a + py cos a); boxes are x y z l w h r with z the
 * bottom face and corners local @ R(r) + centre (Calc.bbox3d2bev).  Coordinates are computed in f64 from the f32 inputs and
 * rounded to f32 once; range decisions are taken on the rounded values.  range6_host: 6 doubles on the HOST, lo xyz, hi xyz.
 *
 * mvx_geom_place_frames: one workgroup per frame.  box3d f32 [n_frames][cap_boxes][7] holds n_box[f] boxes (read only).  The
 *   boxes are visited in index order; trial t of box i passes when the quad of (x + dx, y + dy, l, w, r + dtheta) has
 *   IoU <= iou_thr (mvx_bbox_pairwise's arithmetic, trial quad first) with every other box of the frame -- boxes j < i in their
 *   already moved pose, boxes j > i in their original one; pairs whose bounding circles cannot touch count as 0.  The lowest
 *   passing trial is taken: trial i32 [n_frames][cap_boxes] (-1: none, the box keeps its pose; also for unused slots), move
 *   f32 [n_frames][cap_boxes][4] = its noise row, or zeros.  Then the global step on every box: centre and bottom z as a
 *   point (xy <- s (xy @ R(phi)), z <- s z, y <- -y with flip), l w h <- s (l w h), r <- r + phi, negated with flip, wrapped
 *   into [-pi, pi).  A box is kept iff lo <= (x, y) < hi; the kept boxes, in order, go to out_box3d [n_frames][cap_boxes][7]
 *   (columns 0..1 are the centres) and out_bev [n_frames][cap_boxes][4][2] (recomputed from the new box), their original
 *   indices to kept_idx i32 [n_frames][cap_boxes] (-1 padded), their number to n_kept i32 [n_frames].
 *   status i32 [n_frames] (OR-ed into): MVX_GEOM_BAD_COUNT when n_box[f] is outside 0..cap_boxes (the frame then has no box).
 * mvx_geom_points_frames: one thread per point, two launches (count per block of 256 points; offsets from the counts, ballot
 *   scan, ordered write).  A point inside ORIGINAL box i (|u| <= l/2, |v| <= w/2, 0 <= pz - z <= h as in mvx_gtdb_crop_count;
 *   the lowest index wins) with trial[i] >= 0 moves as xy <- (xy - c) @ R(dtheta) + c + (dx, dy), z <- z + dz; then every point
 *   takes the global step; a point is kept iff lo <= p < hi on all three axes.  Kept rows keep their order and go to
 *   out_points6 (a different buffer, same shape) with columns 3..5 copied bitwise; n_points_out[f] = their number.  Rows behind
 *   n_points[f] are never read.  Both buffers 16-byte aligned; workspace: mvx_geom_workspace_bytes bytes.
 * Limits (MVX_EINVAL before any launch): cap_boxes <= MVX_GT_PASTE_MAX_BOXES, n_trials <= MVX_GEOM_MAX_TRIALS.  No float
 * atomics (bitwise reproducible), no host synchronisation.
 */
#define MVX_GEOM_MAX_TRIALS 32
#define MVX_GEOM_BAD_COUNT 2
size_t mvx_geom_workspace_bytes(int32_t n_frames, int32_t cap_points);
int mvx_geom_place_frames(const float *box3d, const int32_t *n_box, int32_t n_frames, int32_t cap_boxes, const float *noise,
                          int32_t n_trials, const float *glob, float iou_thr, const double *range6_host, int32_t *trial,
                          float *move, float *out_box3d, float *out_bev, int32_t *kept_idx, int32_t *n_kept, int32_t *status,
                          void *stream);
int mvx_geom_points_frames(const float *points6, const int32_t *n_points, int32_t n_frames, int32_t cap_points,
                           const float *box3d, const int32_t *n_box, int32_t cap_boxes, const int32_t *trial, const float *move,
                           const float *glob, const double *range6_host, float *out_points6, int32_t *n_points_out,
                           void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Builder of the GT-paste object database (csrc/gtdb.hip): the reference's create_gtdatabase.py for the frames of a call.
 * The host parses (label files, the KINS annotation file, images, clouds) and prepares the label rows; the kernels match,
 * rasterise and cut.  Tables, all on the device:
 *   labels, n_labels rows in any order (the host sorts by class, frame, row so that a class is a contiguous range):
 *     lab_box2d f32 [n][4] x1 y1 x2 y2, lab_box3d f32 [n][7] xyzlwhr (LiDAR), lab_cs f32 [n][2] = cos, sin of the yaw (the
 *     entries of Calc.getRotationMatrices), lab_frame i32 [n], lab_group i32 [n] = the (frame, class) group of the row;
 *   annotations sorted by group: ann_box f32 [n_ann][4] x1 y1 x2 y2, ann_off i32 [n_groups + 1]; their polygons as edges:
 *     edges f64 [n_edges][4] = x0 y0 x1 y1 (every polygon closed), edge_poly i32 [n_edges] = the polygon of the edge inside
 *     its instance (non-decreasing), edge_off i32 [n_ann + 1];
 *   frames: images u8 [n_frames][h][w][3] BGR, im_hw i32 [n_frames][2] = the rows and columns that are really there (<= h, w);
 *     points f32 [sum][4] x y z r with pts_off i64 [n_frames + 1], 16-byte aligned.
 *
 * mvx_gtdb_match: per label the IoU (torchvision box_iou arithmetic, f32) against the annotation boxes of its group:
 *   best i32 [n] = the first annotation (global index) reaching the maximum, -1 for an empty group; iou f32 [n]; roi i32 [n][4]
 *   = the annotation box truncated to int and clipped to the frame's image, x1 y1 x2 y2 inclusive; flag i32 [n]: bit 0 =
 *   iou >= iou_thr, bit 1 = the ROI is not empty; a label is an OBJECT when flag == 3.  px_off i64 [n + 1] = the exclusive
 *   scan of the objects' ROI pixel counts (0 for the other labels), by a second, single-workgroup kernel.
 * mvx_gtdb_crop_count: pt_off i64 [n + 1] = the exclusive scan of the number of points of the label's frame inside its box
 *   (objects only).  Inside, in f64 on the f32 values: dx = px - x, dy = py - y, u = dx * c - dy * s, v = dx * s + dy * c,
 *   |u| <= l / 2, |v| <= w / 2, 0 <= pz - z <= h.  Counts per chunk of MVX_GTDB_CHUNK points go to the workspace
 *   (mvx_gtdb_workspace_bytes) and become offsets there; mvx_gtdb_crop_write reads them.
 * mvx_gtdb_crop_write: out_points f32 [out_rows][4]: the inside points of object k at rows pt_off[k] .. pt_off[k + 1], in file
 *   order (count, scan, ordered write: no atomics; bitwise reproducible).  Same tables and workspace as the count call.
 * mvx_gtdb_raster: for every object, mask u8 [n_px] (0 / 1) and patch u8 [n_px][3] at px_off: a pixel of the ROI is set when
 *   its centre (x + 0.5, y + 0.5) is inside any polygon of annotation best[k] by the even-odd rule -- per edge, in f64:
 *   (y0 > py) != (y1 > py) and px < (x1 - x0) * (py - y0) / (y1 - y0) + x0 --; patch = mask ? image : 0.  max_roi_rows sizes
 *   the grid (the largest ROI height).  Every output byte has one writer.
 * Argument errors return MVX_EINVAL before any launch.
 */
#define MVX_GTDB_CHUNK 1024
size_t mvx_gtdb_workspace_bytes(int32_t n_labels, int32_t max_frame_points);
int mvx_gtdb_match(const float *lab_box2d, const int32_t *lab_group, const int32_t *lab_frame, int32_t n_labels,
                   const float *ann_box, const int32_t *ann_off, int32_t n_groups, const int32_t *im_hw, int32_t n_frames,
                   float iou_thr, int32_t *best, float *iou, int32_t *flag, int32_t *roi, int64_t *px_off, void *stream);
int mvx_gtdb_crop_count(const float *points, const int64_t *pts_off, int32_t n_frames, int32_t max_frame_points,
                        const float *lab_box3d, const float *lab_cs, const int32_t *lab_frame, const int32_t *flag,
                        int32_t n_labels, int64_t *pt_off, void *workspace, size_t workspace_bytes, void *stream);
int mvx_gtdb_crop_write(const float *points, const int64_t *pts_off, int32_t n_frames, int32_t max_frame_points,
                        const float *lab_box3d, const float *lab_cs, const int32_t *lab_frame, const int32_t *flag,
                        int32_t n_labels, const int64_t *pt_off, const void *workspace, size_t workspace_bytes,
                        float *out_points, int64_t out_rows, void *stream);
int mvx_gtdb_raster(const uint8_t *images, int32_t n_frames, int32_t h, int32_t w, const int32_t *lab_frame,
                    const int32_t *flag, const int32_t *best, const int32_t *roi, const int64_t *px_off, int32_t n_labels,
                    const double *edges, const int32_t *edge_poly, const int32_t *edge_off, int32_t n_ann,
                    int32_t max_roi_rows, uint8_t *mask, uint8_t *patch, int64_t n_px, void *stream);

/* ------------------------------------------------------------------------------------------
 * Frozen ResNet50-FPN image extractor (csrc/extractor.hip; the reference's torchvision trunk, modules/imhead/Pipe.py:8-21):
 * the glue between the row GEMMs (1x1 convolutions) and the mvx_conv2d_*_frames kernels (3x3).  Forward only; maps are
 * channels-last frame sets [F][h][w][c] f32; every output element has one writer.
 *   mvx_image_prepare_frames   torchvision's GeneralizedRCNNTransform (eval) in one launch.  img: u8 [F][h][w][3] (is_u8 != 0;
 *                              values / 255 in f32) or f32 [F][3][h][w]; the channel order is kept.  (x - mean) / std with the
 *                              ImageNet constants, bilinear resize to oh x ow (align_corners = False, coordinate scale h / oh and
 *                              w / ow in f32), zeros from there to ph x pw.  out f32 [F][ph][pw][4], channel 3 is zero.
 *   mvx_stem_conv7_frames      out [F][ch][cw][64] = ReLU(conv 7x7, stride 2, padding 3 of `in` [F][ph][pw][4] (channel 3 unread) +
 *                              bias), ch = (ph - 1) / 2 + 1; wpk f32 [7][7][3][64] = W[co][ci][ky][kx] with BatchNorm folded in
 *   mvx_maxpool3s2_frames      3x3, stride 2, padding 1: out [F][(h - 1) / 2 + 1][(w - 1) / 2 + 1][c]
 *   mvx_add_relu_frames        out = ReLU(a + b) over n floats (n % 4 == 0)
 *   mvx_gather_stride2_frames  out [F][(h - 1) / 2 + 1][(w - 1) / 2 + 1][c] = in at the even (y, x) sites
 *   mvx_topdown_merge_frames   out [F][lat_h][lat_w][c] = lateral + top [F][top_h][top_w][c] at (y / 2, x / 2); the lateral map
 *                              must be EXACTLY twice the top one (MVX_EINVAL otherwise)
 * channels % 4 == 0 and 16-byte aligned pointers throughout.
 */
int mvx_image_prepare_frames(const void *img, int32_t is_u8, float *out, int32_t n_frames, int32_t h, int32_t w, int32_t oh,
                             int32_t ow, int32_t ph, int32_t pw, void *stream);
int mvx_stem_conv7_frames(const float *in, const float *wpk, const float *bias, float *out, int32_t n_frames, int32_t ph,
                          int32_t pw, void *stream);
int mvx_maxpool3s2_frames(const float *in, float *out, int32_t n_frames, int32_t h, int32_t w, int32_t channels, void *stream);
int mvx_add_relu_frames(const float *a, const float *b, float *out, int64_t n, void *stream);
int mvx_gather_stride2_frames(const float *in, float *out, int32_t n_frames, int32_t h, int32_t w, int32_t channels, void *stream);
int mvx_topdown_merge_frames(const float *lateral, const float *top, float *out, int32_t n_frames, int32_t lat_h, int32_t lat_w,
                             int32_t top_h, int32_t top_w, int32_t channels, void *stream);

/* ------------------------------------------------------------------------------------------
 * Fused AdamW over a flat gradient buffer (csrc/optim.hip): global gradient norm, clipping, a guard against non-finite
 * gradients and the update, three launches, no host read, no float atomics (bitwise reproducible).
 *   grad_flat f32 [n] (read only), m_flat / v_flat f32 [n]: first and second moment in the same layout; n < 2^31.
 *   chunk_table i64 [n_chunks][3] on the device: {address of the chunk's first parameter element, its offset in the flat
 *     layout, its element count}, 1 <= count <= MVX_OPTIM_CHUNK, a chunk inside ONE parameter; the chunks cover [0, n) once.
 *     The table lives on the device, so only its size is checked here; an entry that leaves [0, n) or the count limit is
 *     skipped by the kernel.  The parameter addresses are the caller's responsibility.
 *   count_or_null: f32 device scalar, the number of samples summed into the gradient: the gradient is scaled by
 *     1 / max(count, 1) on the fly (NULL: by 1).
 *   state f64 [8], kept by the caller between steps, zeros at the start: [0] step t, [1] skipped steps, [2] the last norm,
 *     [3] the last clip coefficient, [4] 1.0 when the last step was skipped.
 * norm = sqrt(sum g^2, f64) * gscale; coef = min(1, max_norm / (norm + 1e-6)) for max_norm > 0, else 1
 * (torch.nn.utils.clip_grad_norm_).  With guard != 0 a step whose gradient holds an inf or a NaN, or whose norm is not finite,
 * changes no parameter and no moment, leaves t as it is and counts one skipped step.  Otherwise t += 1 and, per element in
 * f32, torch's single-tensor AdamW:  g' = g * (gscale * coef);  p *= 1 - lr * wd;  m += (g' - m) * (1 - beta1);
 * v = v * beta2 + (1 - beta2) * g' * g';  p -= lr / (1 - beta1^t) * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps)), the division
 * by sqrt(1 - beta2^t) as a multiplication by its reciprocal; the scalar factors are computed in f64 and rounded to f32 once.
 * workspace: mvx_optim_workspace_bytes bytes, 8-byte aligned.  Argument errors return MVX_EINVAL before any launch:
 * 0 <= beta < 1, lr, eps, weight_decay, max_norm >= 0 and finite.
 */
#define MVX_OPTIM_CHUNK 4096
size_t mvx_optim_workspace_bytes(int64_t n);
int mvx_optim_adamw_step(const int64_t *chunk_table, int32_t n_chunks, const float *grad_flat, float *m_flat, float *v_flat,
                         int64_t n, const float *count_or_null, double *state, double lr, double beta1, double beta2, double eps,
                         double weight_decay, double max_norm, int32_t guard, void *workspace, size_t workspace_bytes,
                         void *stream);

/* ------------------------------------------------------------------------------------------
 * Frame rendering (csrc/render.hip): a bird's-eye view and a camera view of the frames of a step (1..MVX_MAX_FRAMES) with a
 * list of coloured boxes, u8 RGB images [n_frames][h][w][3], h and w in 1..MVX_RENDER_MAX_SIDE.  Three launches per view for
 * all frames; the planes the kernels meet on are u32 words combined by integer atomicMax / atomicMin / atomicAdd (no float
 * atomics), every pixel is decided by integer arithmetic on f64 geometry: bitwise reproducible, independent of the order of
 * points and boxes.  The planes are cleared on `stream`; no host synchronisation.
 *   points6 f32 [n_frames][cap_points][ld] (ld >= 6: x y z r row col), n_points i32 [n_frames] on the device (clamped to
 *   0..cap_points).  The draw list: boxes f32 [n_frames][cap_boxes][7] x y z l w h r in the LiDAR frame, z the bottom face
 *   (Calc.bbox3d2corner), n_boxes i32 [n_frames] on the device (clamped to 0..cap_boxes), colors u32 [n_frames][cap_boxes] =
 *   prio << 24 | R << 16 | G << 8 | B; cap_boxes = 0: nothing is drawn and the three pointers may be null.  Where segments
 *   meet on a pixel the larger word wins; 0 draws nothing.  The kernels know colours, not classes.
 *   A box with a non-finite field, or with a segment end whose pixel row or column is not below 2^24 in magnitude, is dropped
 *   whole and sets MVX_RENDER_BAD_BOX in status i32 [n_frames] (written by the call).
 * Segment rule (both views), integer ends (r0, c0), (r1, c1): the major axis is rows iff |dr| >= |dc|; the end with the smaller
 *   (major, minor) pair comes first; n = max(|dr|, |dc|); pixel k = 0..n: major = m0 + k, minor = q0 + sgn(dq) *
 *   ((2 k |dq| + n) / (2 n)) in i64 (n = 0: one pixel).  Only the k whose major coordinate is inside the image are visited
 *   (the range is computed); pixels whose minor coordinate is outside are skipped.  Each pixel stamps a thickness x thickness
 *   square with offsets -(T / 2) .. T - 1 - (T / 2), clipped to the image; thickness 1..3.
 * mvx_render_bev_frames: cell i = floor(((double)x - x0) / res), j = floor(((double)y - y0) / res); image row h - 1 - i, column
 *   w - 1 - j; a point is drawn iff 0 <= i < h and 0 <= j < w and x, y, z are finite.  Per pixel the largest
 *   key = ((zq << 8) | iq) + 1, zq = clamp(floor((z - z0) / (z1 - z0) * 65535), 0, 65535), iq = clamp(floor(r * 255), 0, 255)
 *   (a NaN clamps to 0), and the number of points.  Shading, integer floor divisions: idx = zq >> 8 (MVX_RENDER_BY_HEIGHT) or
 *   iq (MVX_RENDER_BY_INTENSITY); out[ch] = lut[idx][ch] * (64 + 191 * min(count, cmax) / cmax) / 255; pixels without a point
 *   take `background` (R << 16 | G << 8 | B).  lut u8 [256][3] on the device.  Boxes: corners as Calc.bbox3d2bev with cos and
 *   sin of (double)yaw, each mapped to a pixel by the floor rule above; the four edges and a heading marker from the centre to
 *   the midpoint of the edge at u = +l/2.
 * mvx_render_camera_frames: background = image_or_null u8 [n_frames][h][w][3] (channels swapped when image_is_bgr != 0) or
 *   black.  A point's pixel is (floor(row), floor(col)) of columns 4 and 5; it stamps a (2 R + 1)^2 square, R = point_radius in
 *   0..2, clipped to the image, with dq = clamp(floor(x / depth_max * 65535), 0, 65535) under atomicMin; a pixel with a point
 *   takes lut_depth[dq >> 8].  Points with a non-finite x, row or col are skipped.  Boxes: the eight corners in the order of
 *   Calc.bbox3d2corner through image_from_lidar f64 [n_frames][4][4] on the device (rows 0..2: u' v' w', each
 *   ((m0 X + m1 Y) + m2 Z) + m3); the twelve edges and the two diagonals of the face at u = +l/2; a segment with both ends at
 *   w' < z_near is dropped, one with a single end there has that end moved to the plane (t = (z_near - wa) / (wb - wa),
 *   a + t (b - a), w' = z_near); then column = floor(u' / w'), row = floor(v' / w').  Order: background, points, boxes.
 * workspace: mvx_render_workspace_bytes(n_frames, h, w) bytes (0 for sizes outside the limits), 16-byte aligned; out and
 * image_or_null 4-byte aligned.  MVX_EINVAL before any launch: a null required pointer, n_frames, h or w outside the limits,
 * res <= 0, z1 <= z0, cmax < 1, thickness outside 1..3, point_radius outside 0..2, z_near or depth_max <= 0, ld < 6, a
 * workspace that is too small.
 */
#define MVX_RENDER_MAX_SIDE 4096
#define MVX_RENDER_BAD_BOX 1
#define MVX_RENDER_BY_HEIGHT 0
#define MVX_RENDER_BY_INTENSITY 1
size_t mvx_render_workspace_bytes(int32_t n_frames, int32_t h, int32_t w);
int mvx_render_bev_frames(const float *points6, int32_t ld, const int32_t *n_points, int32_t n_frames, int32_t cap_points,
                          const float *boxes, const int32_t *n_boxes, const uint32_t *colors, int32_t cap_boxes, double x0,
                          double y0, double res, double z0, double z1, int32_t h, int32_t w, const uint8_t *lut,
                          int32_t color_by, int32_t cmax, uint32_t background, int32_t thickness, uint8_t *out,
                          int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
int mvx_render_camera_frames(const float *points6, int32_t ld, const int32_t *n_points, int32_t n_frames, int32_t cap_points,
                             const float *boxes, const int32_t *n_boxes, const uint32_t *colors, int32_t cap_boxes,
                             const double *image_from_lidar, double z_near, double depth_max, int32_t h, int32_t w,
                             const uint8_t *lut_depth, int32_t point_radius, const uint8_t *image_or_null,
                             int32_t image_is_bgr, int32_t thickness, uint8_t *out, int32_t *status, void *workspace,
                             size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Running BatchNorm statistics (csrc/bn_running.hip; config.yml `bntrack`, nn.BatchNorm*d(track_running_stats=True)).
 * Every BatchNorm site of the frame-set path hands its consumer mean_inv f32 [n_frames][2][channels] = (mean,
 * 1 / sqrt(biased var + eps)) per frame; the apply kernels, mvx_bn_background_frames and the fused BEV writer read only that.
 * Tracking folds these tensors into the modules' buffers, eval mode fills them from the buffers -- each direction for ALL
 * sites of a step in one launch, one thread per (site, channel), plain vector stores.  The site table is a HOST array that
 * travels by value in the kernel arguments (like mvx_frames_t): no host synchronisation, nothing to keep alive.  One launch
 * takes up to MVX_BN_SITES_PER_LAUNCH sites with up to 8 distinct population vectors (the model has 30 sites and 7); a longer
 * table goes out in further launches.
 *   mean_inv                    f32 [n_frames][2][channels] on the device (update: read; mean_inv_sites: written)
 *   running_mean / running_var  f32 [channels], num_batches_tracked i64 [1]: the module's buffers, on the device
 *   momentum                    the module's bn.momentum, 0..1 (None, the cumulative average, is refused by the caller)
 *   row_kind, rows              the layout of the site's row matrix and its row count over all frames: the per-frame populations
 *                               are those of the site's finaliser -- MVX_ROWS_GRID: rows / n_frames; the row layouts (FUSION,
 *                               VFE, VOXELS, REAL): (voxels of the frame) x t of `frames_host`, the DENSE population the compact
 *                               rows stand for.  `rows` must match the layout like in every frame-set entry point.
 * mvx_bn_running_update_sites (training): the reference runs batch 1, one forward per frame, so the fold is n_frames sequential
 *   PyTorch updates in frame order; for every frame f with bit f of live_mask set and a population n_f > 0:
 *     rm = (1 - m) rm + m mean_f;   rv = (1 - m) rv + m var_f n_f / (n_f - 1),   var_f = max(0, 1 / inv_f^2 - eps)
 *   (n_f = 1 folds the mean and leaves rv alone), the whole chain in float64 registers, each buffer element stored once as
 *   f32; num_batches_tracked += the number of frames folded.  A frame without population (no voxels: the finalisers give it
 *   mean 0, inverse deviation 1 / sqrt(eps)) folds nothing and is not counted.  frames_host may be NULL when every site is
 *   MVX_ROWS_GRID; otherwise frames_host->n_frames == n_frames.
 * mvx_bn_running_mean_inv_sites (eval): mean_inv[f] = (running_mean, 1 / sqrt(running_var + eps)) for every f < n_frames, the
 *   inverse deviation computed in float64 and rounded once; momentum, rows, row_kind and num_batches_tracked are not read.
 * MVX_EINVAL before any launch (no buffer is touched): a null table or buffer pointer, channels <= 0, n_frames outside
 *   1..MVX_MAX_FRAMES, eps < 0, momentum outside 0..1, an inconsistent layout.
 */
#define MVX_BN_SITES_PER_LAUNCH 48
typedef struct {
    float *mean_inv;
    float *running_mean;
    float *running_var;
    int64_t *num_batches_tracked;
    int64_t rows;
    double momentum;
    int32_t channels;
    int32_t row_kind;
} mvx_bn_site_t;
int mvx_bn_running_update_sites(const mvx_bn_site_t *sites_host, int32_t n_sites, const mvx_frames_t *frames_host,
                                int32_t n_frames, uint32_t live_mask, double eps, void *stream);
int mvx_bn_running_mean_inv_sites(const mvx_bn_site_t *sites_host, int32_t n_sites, int32_t n_frames, double eps, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MVX_HIP_H */
