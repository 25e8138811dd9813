// Voxel Feature Encoding glue: BatchNorm + per-voxel max over the T sampled rows + concat.
//
// Replaces, for one VFE layer (modules/voxelnet/Pipe.py:12-18):
//     x = BN(relu(fc(x)));  s = max_t x;  out = cat([x, repeat(s, T)], -1)
// and for the head (modules/voxelnet/VoxelNet.py:28-33):  x = BN(relu(fc(x)));  feat = max_t x
// The max runs over ALL T rows, padded ones included (no mask).  BatchNorm is a
// per-channel increasing affine map, so max_t BN(y) = BN(max_t y): the kernels normalise while
// they reduce and never materialise the intermediate tensor separately.
// Rows are [V][T][C] row-major; one thread owns one (voxel, channel) column, so loads and
// stores are coalesced across channels.
//
// Compact rows.  Inside MVXNet every padded row of a voxel is identical, so the T rows
// of voxel v can be stored as its vcnt[v] real rows (rows voff[v] .. voff[v]+vcnt[v]-1 of the
// matrix) plus ONE padded row (row n_real + v) that stands for the T - vcnt[v] identical padded
// rows.  With voff/vcnt given, the kernels below walk that layout; the padded row takes part in
// the max only if T - vcnt[v] > 0, and its gradient is the SUM over the rows it stands for.
// argmax holds the local row (0..vcnt-1) or vcnt[v] for the padded row.
#include "common.h"
#include "quad.h"

namespace {

// One thread owns VEC neighbouring channels of one voxel and moves them as one load / store.  VEC = 4 is the form of the workload
// (channels a multiple of 4, 16-byte aligned tensors); VEC = 1 serves every other call.  Both keep VU rows of the voxel in flight
// per trip (one dependent 4-byte row at a time ran at 0.9-1.9 TB/s), and the arithmetic and its order per channel -- first maximum
// wins, gradient sums in stored-row order -- do not depend on VEC: the two instantiations give the same bits.
constexpr int VU = 4;
template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) Pack { T c[VEC]; };
template <int VEC, typename T>
__device__ __forceinline__ Pack<T, VEC> ldv(const T *p) { return *(const Pack<T, VEC> *)p; }
template <int VEC, typename T>
__device__ __forceinline__ void stv(T *p, const Pack<T, VEC> &v) { *(Pack<T, VEC> *)p = v; }

// rows of voxel v in compact or dense layout, resolved once per thread (voff / vcnt are the same for all lanes of a voxel)
struct VoxRows {
    size_t first, pad;      // first real row, the padded row (dense: first row, unused)
    int count, n, nw;       // real rows (dense: all T); rows that take part in the max; rows that are stored
    __device__ __forceinline__ VoxRows(const int *voff, const int *vcnt, int T, int n_real, int v) {
        count = vcnt ? vcnt[v] : T;
        first = vcnt ? (size_t)voff[v] : (size_t)v * T;
        pad = (size_t)n_real + v;
        n = count + (count < T ? 1 : 0);
        nw = vcnt ? count + 1 : T;                        // the padded row is always written
    }
    __device__ __forceinline__ size_t row(int t) const { return t < count ? first + t : pad; }
    // row t of a trip that loads VU rows whatever is left: the rows past the last of `rows` read that last one again
    __device__ __forceinline__ size_t row_of(int t, int rows) const { return row(t < rows ? t : rows - 1); }
};
#define VOX_ROWS_PARAMS const int *__restrict__ voff, const int *__restrict__ vcnt, int T, int n_real

// this thread's voxel and first channel, or false past the end
template <int VEC>
__device__ __forceinline__ bool vfe_thread(int V, int C, int &v, int &c) {
    const int cv = C / VEC;
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    v = (int)(e / cv); c = (int)(e % cv) * VEC;
    return e < (long long)V * cv;
}

// out = BN(y) and its max over the voxel's rows: CONCAT [row][2C] = (BN(y), max), else [voxel][C] = max alone
template <int VEC, bool CONCAT>
__global__ __launch_bounds__(256) void vfe_bn_max(const float *__restrict__ y, const float *__restrict__ mi,
                                                  float *__restrict__ out, int *__restrict__ argmax, int V, int C,
                                                  VOX_ROWS_PARAMS, FrameMap fm) {
    int v, c;
    if (!vfe_thread<VEC>(V, C, v, c)) return;
    mi += (size_t)fm_frame_of(fm, v) * 2 * C;             // per-frame BatchNorm (frames = voxel segments)
    const Pack<float, VEC> m = ldv<VEC>(mi + c), iv = ldv<VEC>(mi + C + c);
    const VoxRows w(voff, vcnt, T, n_real, v);
    auto bn = [&](const Pack<float, VEC> &q) {
        Pack<float, VEC> r;
#pragma unroll
        for (int i = 0; i < VEC; ++i) r.c[i] = bn1(q.c[i], m.c[i], iv.c[i]);
        return r;
    };
    Pack<float, VEC> best;
    Pack<int, VEC> bi;
#pragma unroll
    for (int i = 0; i < VEC; ++i) { best.c[i] = -INFINITY; bi.c[i] = 0; }
    for (int t0 = 0; t0 < w.n; t0 += VU) {
        Pack<float, VEC> q[VU];
#pragma unroll
        for (int u = 0; u < VU; ++u) q[u] = ldv<VEC>(y + w.row_of(t0 + u, w.n) * C + c);
#pragma unroll
        for (int u = 0; u < VU; ++u)
            if (t0 + u < w.n) {
                const Pack<float, VEC> val = bn(q[u]);
#pragma unroll
                for (int i = 0; i < VEC; ++i)
                    if (val.c[i] > best.c[i]) { best.c[i] = val.c[i]; bi.c[i] = t0 + u; }       // the first maximum wins
            }
    }
    if (CONCAT) {
        for (int t0 = 0; t0 < w.nw; t0 += VU) {
            Pack<float, VEC> q[VU];
#pragma unroll
            for (int u = 0; u < VU; ++u) q[u] = ldv<VEC>(y + w.row_of(t0 + u, w.nw) * C + c);
#pragma unroll
            for (int u = 0; u < VU; ++u)
                if (t0 + u < w.nw) {
                    float *o = out + w.row(t0 + u) * 2 * C;
                    stv<VEC>(o + c, bn(q[u]));
                    stv<VEC>(o + C + c, best);
                }
        }
    } else {
        stv<VEC>(out + (size_t)v * C + c, best);
    }
    stv<VEC>(argmax + (size_t)v * C + c, bi);
}

template <int VEC>
__global__ __launch_bounds__(256) void vfe_max_concat_bwd(const float *__restrict__ g, const int *__restrict__ argmax,
                                                          float *__restrict__ dyh, int V, int C, VOX_ROWS_PARAMS) {
    int v, c;
    if (!vfe_thread<VEC>(V, C, v, c)) return;
    const VoxRows w(voff, vcnt, T, n_real, v);
    Pack<float, VEC> s;
#pragma unroll
    for (int i = 0; i < VEC; ++i) s.c[i] = 0.f;
    for (int t0 = 0; t0 < w.nw; t0 += VU) {                // the gradient of the max: summed in row order (padded row: already summed)
        Pack<float, VEC> q[VU];
#pragma unroll
        for (int u = 0; u < VU; ++u) q[u] = ldv<VEC>(g + w.row_of(t0 + u, w.nw) * 2 * C + C + c);
#pragma unroll
        for (int u = 0; u < VU; ++u)
            if (t0 + u < w.nw)
#pragma unroll
                for (int i = 0; i < VEC; ++i) s.c[i] += q[u].c[i];
    }
    const Pack<int, VEC> am = ldv<VEC>(argmax + (size_t)v * C + c);
    for (int t0 = 0; t0 < w.nw; t0 += VU) {
        Pack<float, VEC> q[VU];
#pragma unroll
        for (int u = 0; u < VU; ++u) q[u] = ldv<VEC>(g + w.row_of(t0 + u, w.nw) * 2 * C + c);
#pragma unroll
        for (int u = 0; u < VU; ++u) {
            const int t = t0 + u;
            if (t >= w.nw) break;
#pragma unroll
            for (int i = 0; i < VEC; ++i) q[u].c[i] += t == am.c[i] ? s.c[i] : 0.f;
            stv<VEC>(dyh + w.row(t) * C + c, q[u]);
        }
    }
}

template <int VEC>
__global__ __launch_bounds__(256) void segmax_bwd(const float *__restrict__ dfeat, const int *__restrict__ argmax,
                                                  float *__restrict__ dyh, int V, int C, VOX_ROWS_PARAMS) {
    int v, c;
    if (!vfe_thread<VEC>(V, C, v, c)) return;
    const VoxRows w(voff, vcnt, T, n_real, v);
    const Pack<float, VEC> gv = ldv<VEC>(dfeat + (size_t)v * C + c);
    const Pack<int, VEC> am = ldv<VEC>(argmax + (size_t)v * C + c);
    for (int t = 0; t < w.nw; ++t) {
        Pack<float, VEC> o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) o.c[i] = t == am.c[i] ? gv.c[i] : 0.f;
        stv<VEC>(dyh + w.row(t) * C + c, o);
    }
}

// ---- compact row bookkeeping --------------------------------------------------------------------
// row_map [V*T] (dense row -> compact real row or -1)  ->  voff[v] = first compact row of voxel v,
// vcnt[v] = number of real rows, row_w[n_real + v] = T - vcnt[v] (weight of the padded row),
// row_w[real rows] = 1.
__global__ void voxel_row_offsets(const int *__restrict__ row_map, int V, int T, int n_real, int *__restrict__ voff,
                                  int *__restrict__ vcnt, float *__restrict__ row_w, float *__restrict__ fusion_row_w,
                                  FrameMap fm) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    // fusion layout (optional): real rows weigh 1, the shared padded row of frame f stands for all padded rows of f
    if (fusion_row_w) {
        for (int j = v; j < n_real; j += gridDim.x * blockDim.x) fusion_row_w[j] = 1.f;
        if (v < fm.F) {
            int nreal_f = 0;                          // real rows of frame f = extent of its real-row segment
            for (int sg = 0; sg < fm.nseg; ++sg)
                if (fm.seg_frame[sg] == v && fm.bound[sg + 1] <= n_real) nreal_f += fm.bound[sg + 1] - fm.bound[sg];
            fusion_row_w[n_real + v] = (float)(fm.count[v] - (double)nreal_f);
        }
    }
    if (v >= V) return;
    int first = -1, n = 0;
    for (int t = 0; t < T; ++t) {
        const int j = row_map[(size_t)v * T + t];
        if (j >= 0) { if (first < 0) first = j; row_w[j] = 1.f; ++n; }
    }
    voff[v] = first < 0 ? 0 : first;
    vcnt[v] = n;
    row_w[n_real + v] = (float)(T - n);
}

// VFE-1 input in compact form: real row j = [voxels[r][0:7], imfeat[j][0:F]], padded row of voxel v =
// [0 x 7, imfeat[n_real][0:F]] (imfeat's last row is the fusion output of the shared padded row).
// ld >= 7 + F: the row pitch of `out`; columns [7 + F, ld) are written as zeros (a pitch that is a multiple of 4 lets the row GEMM
// and its weight gradient read the rows with 16-byte loads: 23 floats per row made both fall to their scalar-load forms)
__global__ void vfe_compact_input(const float *__restrict__ vox, int vc, const int *__restrict__ rows_sel,
                                  const float *__restrict__ imfeat, int F, int n_real, int V, float *__restrict__ out,
                                  FrameMap fm, int ld) {
    const int W = 7 + F;
    const long long total = (long long)(n_real + V) * ld;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(e / ld), c = (int)(e % ld);
        float val;
        if (c >= W) val = 0.f;
        else if (j < n_real) val = c < 7 ? vox[(size_t)rows_sel[j] * vc + c] : imfeat[(size_t)j * F + c - 7];
        else val = c < 7 ? 0.f : imfeat[(size_t)(n_real + fm_frame_of(fm, j - n_real)) * F + c - 7];   // its frame's shared padded row
        out[e] = val;
    }
}

// gradient wrt imfeat: real rows copy columns 7.., the shared padded row sums them over the voxels
__global__ __launch_bounds__(256) void vfe_compact_input_bwd(const float *__restrict__ g, int F, int n_real, int V,
                                                             float *__restrict__ dimfeat, double *__restrict__ padsum,
                                                             FrameMap fm) {
    const int W = 7 + F;
    const long long total = (long long)n_real * F;
    // four independent elements in flight per thread (one load per trip left the 4-byte gather latency-bound)
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e0 = blockIdx.x * (long long)blockDim.x + threadIdx.x; e0 < total; e0 += 4 * stride) {
        float q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long e = e0 + u * stride;
            const long long j = (e < total ? e : e0) / F;
            q[u] = g[(size_t)j * W + 7 + (int)((e < total ? e : e0) - j * F)];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (e0 + u * stride < total) dimfeat[e0 + u * stride] = q[u];
    }
    // padded rows: the padded rows of frame f feed the shared padded row of f.  ONE pass over the voxels with an LDS table of
    // per-(frame, column) f64 cells that goes out with one f64 atomic per touched cell.  (The first form made one pass PER FRAME, each with two barriers and a serial fold: 121 us for
    // 16 frames of 37 MB.)
    constexpr int MAXF = 64;                                  // columns the table holds (the fusion branch has 16)
    __shared__ double acc[MVX_MAX_FRAMES * MAXF];
    if (F <= MAXF && 256 % F == 0) {
        for (int i = threadIdx.x; i < fm.F * F; i += blockDim.x) acc[i] = 0.0;
        __syncthreads();
        // a workgroup takes a CONTIGUOUS run of voxels (one or two frames), thread (rt, ct) every rpi-th voxel of it at column ct:
        // a running f64 sum that goes to the table when the frame changes and at the end (<= 2-3 LDS atomics per thread)
        const int rpi = 256 / F, ct = threadIdx.x % F, rt = threadIdx.x / F;
        const long long per = ((long long)V + gridDim.x - 1) / gridDim.x;
        const long long lo = blockIdx.x * per, hi = lo + per < V ? lo + per : V;
        double run = 0.0;
        int cur = -1;
        for (long long v = lo + rt; v < hi; v += rpi) {
            const int f = fm_frame_of(fm, v);
            if (f != cur) {
                if (cur >= 0) atomicAdd(&acc[cur * F + ct], run);
                cur = f; run = 0.0;
            }
            run += (double)g[(size_t)(n_real + v) * W + 7 + ct];
        }
        if (cur >= 0) atomicAdd(&acc[cur * F + ct], run);
        __syncthreads();
        for (int i = threadIdx.x; i < fm.F * F; i += blockDim.x)
            if (acc[i] != 0.0) atomicAdd(padsum + i, acc[i]);
        return;
    }
    __shared__ float red[256];
    const int rpi = 256 / F;
    const int ct = threadIdx.x % F, rt = threadIdx.x / F;
    for (int sg = 0; sg < fm.nseg; ++sg) {
        const long long lo = fm.F == 1 ? 0 : fm.bound[sg], hi = fm.F == 1 ? V : fm.bound[sg + 1];
        const int f = fm.F == 1 ? 0 : (int)fm.seg_frame[sg];
        float s = 0.f;
        if (rt < rpi)
            for (long long v = lo + blockIdx.x * (long long)rpi + rt; v < hi; v += (long long)gridDim.x * rpi)
                s += g[(size_t)(n_real + v) * W + 7 + ct];
        __syncthreads();
        red[threadIdx.x] = s;
        __syncthreads();
        if (rt == 0) {
            double t = 0.0;
            for (int k = 0; k < rpi; ++k) t += (double)red[k * F + ct];
            atomicAdd(padsum + (size_t)f * F + ct, t);
        }
    }
}

__global__ void vfe_compact_pad_finish(const double *__restrict__ padsum, float *__restrict__ dimfeat, int n_real, int F,
                                       int n_frames) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < F * n_frames) dimfeat[(size_t)n_real * F + e] = (float)padsum[e];
}

}  // namespace

#define VFE_ARGS_OK (n_voxels >= 0 && t > 0 && channels > 0)
#define VFE_GRID(vec) dim3(mvx_cdiv((long long)n_voxels * (channels / (vec)), 256)), dim3(256), 0, (hipStream_t)stream
#define VFE_ROWS voff, vcnt, t, n_real
static inline bool vfe_vec4(int channels, const void *a, const void *b, const void *c) {
    return channels % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}
#define VFE_ROWS_OK ((voff == nullptr) == (vcnt == nullptr))
#define VFE_FRAMES(fm) FrameMap fm; MVX_CHECK_ARG(mvx_build_frame_map(fm, frames_host, frames_host ? MVX_ROWS_VOXELS : MVX_ROWS_SINGLE, n_voxels, 1.0))

extern "C" int mvx_vfe_bn_max_concat_frames(const float *y, const float *mean_inv, float *out, int32_t *argmax,
                                            int32_t n_voxels, int32_t t, int32_t channels, const int32_t *voff,
                                            const int32_t *vcnt, int32_t n_real, const mvx_frames_t *frames_host,
                                            void *stream) {
    MVX_CHECK_ARG(y && mean_inv && out && argmax && VFE_ARGS_OK && VFE_ROWS_OK);
    if (n_voxels == 0) return MVX_OK;
    VFE_FRAMES(fm);
    if (vfe_vec4(channels, y, out, argmax) && ((uintptr_t)mean_inv & 15) == 0)
        hipLaunchKernelGGL((vfe_bn_max<4, true>), VFE_GRID(4), y, mean_inv, out, argmax, n_voxels, channels, VFE_ROWS, fm);
    else
        hipLaunchKernelGGL((vfe_bn_max<1, true>), VFE_GRID(1), y, mean_inv, out, argmax, n_voxels, channels, VFE_ROWS, fm);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_vfe_bn_max_concat(const float *y, const float *mean_inv, float *out, int32_t *argmax,
                                     int32_t n_voxels, int32_t t, int32_t channels, const int32_t *voff,
                                     const int32_t *vcnt, int32_t n_real, void *stream) {
    return mvx_vfe_bn_max_concat_frames(y, mean_inv, out, argmax, n_voxels, t, channels, voff, vcnt, n_real, nullptr, stream);
}

extern "C" int mvx_vfe_max_concat_backward(const float *grad_out, const int32_t *argmax, float *dyhat,
                                           int32_t n_voxels, int32_t t, int32_t channels, const int32_t *voff,
                                           const int32_t *vcnt, int32_t n_real, void *stream) {
    MVX_CHECK_ARG(grad_out && argmax && dyhat && VFE_ARGS_OK && VFE_ROWS_OK);
    if (n_voxels == 0) return MVX_OK;
    if (vfe_vec4(channels, grad_out, dyhat, argmax))
        hipLaunchKernelGGL(vfe_max_concat_bwd<4>, VFE_GRID(4), grad_out, argmax, dyhat, n_voxels, channels, VFE_ROWS);
    else
        hipLaunchKernelGGL(vfe_max_concat_bwd<1>, VFE_GRID(1), grad_out, argmax, dyhat, n_voxels, channels, VFE_ROWS);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_bn_segment_max_frames(const float *y, const float *mean_inv, float *out, int32_t *argmax,
                                         int32_t n_voxels, int32_t t, int32_t channels, const int32_t *voff,
                                         const int32_t *vcnt, int32_t n_real, const mvx_frames_t *frames_host,
                                         void *stream) {
    MVX_CHECK_ARG(y && mean_inv && out && argmax && VFE_ARGS_OK && VFE_ROWS_OK);
    if (n_voxels == 0) return MVX_OK;
    VFE_FRAMES(fm);
    if (vfe_vec4(channels, y, out, argmax) && ((uintptr_t)mean_inv & 15) == 0)
        hipLaunchKernelGGL((vfe_bn_max<4, false>), VFE_GRID(4), y, mean_inv, out, argmax, n_voxels, channels, VFE_ROWS, fm);
    else
        hipLaunchKernelGGL((vfe_bn_max<1, false>), VFE_GRID(1), y, mean_inv, out, argmax, n_voxels, channels, VFE_ROWS, fm);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_bn_segment_max(const float *y, const float *mean_inv, float *out, int32_t *argmax,
                                  int32_t n_voxels, int32_t t, int32_t channels, const int32_t *voff,
                                  const int32_t *vcnt, int32_t n_real, void *stream) {
    return mvx_bn_segment_max_frames(y, mean_inv, out, argmax, n_voxels, t, channels, voff, vcnt, n_real, nullptr, stream);
}

extern "C" int mvx_segment_max_backward(const float *dfeat, const int32_t *argmax, float *dyhat, int32_t n_voxels,
                                        int32_t t, int32_t channels, const int32_t *voff, const int32_t *vcnt,
                                        int32_t n_real, void *stream) {
    MVX_CHECK_ARG(dfeat && argmax && dyhat && VFE_ARGS_OK && VFE_ROWS_OK);
    if (n_voxels == 0) return MVX_OK;
    if (vfe_vec4(channels, dfeat, dyhat, argmax))
        hipLaunchKernelGGL(segmax_bwd<4>, VFE_GRID(4), dfeat, argmax, dyhat, n_voxels, channels, VFE_ROWS);
    else
        hipLaunchKernelGGL(segmax_bwd<1>, VFE_GRID(1), dfeat, argmax, dyhat, n_voxels, channels, VFE_ROWS);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_voxel_row_offsets_frames(const int32_t *row_map, int32_t n_voxels, int32_t t, int32_t n_real,
                                            int32_t *voff, int32_t *vcnt, float *row_w, float *fusion_row_w,
                                            const mvx_frames_t *frames_host, void *stream) {
    MVX_CHECK_ARG(row_map && voff && vcnt && row_w && n_voxels >= 0 && t > 0 && n_real >= 0);
    if (n_voxels == 0) return MVX_OK;
    FrameMap fm;
    // the FUSION layout's segment table carries the real-row extents the shared-row weights need
    MVX_CHECK_ARG(mvx_build_frame_map(fm, frames_host, frames_host ? MVX_ROWS_FUSION : MVX_ROWS_SINGLE,
                                      frames_host ? (long long)n_real + frames_host->n_frames : (long long)n_real + 1,
                                      (double)n_voxels * t));
    MVX_CHECK_ARG(!fusion_row_w || frames_host);
    hipLaunchKernelGGL(voxel_row_offsets, dim3(mvx_cdiv(n_voxels, 256)), dim3(256), 0, (hipStream_t)stream, row_map,
                       n_voxels, t, n_real, voff, vcnt, row_w, fusion_row_w, fm);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_voxel_row_offsets(const int32_t *row_map, int32_t n_voxels, int32_t t, int32_t n_real,
                                     int32_t *voff, int32_t *vcnt, float *row_w, void *stream) {
    return mvx_voxel_row_offsets_frames(row_map, n_voxels, t, n_real, voff, vcnt, row_w, nullptr, nullptr, stream);
}

// ... with a row pitch: out is [n_real + n_voxels][ld], ld >= 7 + feat_channels, the columns beyond 7 + feat_channels zero
extern "C" int mvx_vfe_compact_input_pitch_frames(const float *voxels, int32_t vox_channels, const int32_t *rows_sel,
                                                  const float *imfeat, int32_t feat_channels, int32_t n_real, int32_t n_voxels,
                                                  float *out, int32_t ld, const mvx_frames_t *frames_host, void *stream) {
    MVX_CHECK_ARG(voxels && rows_sel && imfeat && out && vox_channels >= 7 && feat_channels > 0);
    MVX_CHECK_ARG(n_real >= 0 && n_voxels >= 0 && ld >= 7 + feat_channels);
    const long long total = (long long)(n_real + n_voxels) * ld;
    if (total == 0) return MVX_OK;
    VFE_FRAMES(fm);
    hipLaunchKernelGGL(vfe_compact_input, dim3(mvx_cdiv(total, 256) > 2048 ? 2048 : mvx_cdiv(total, 256)), dim3(256), 0,
                       (hipStream_t)stream, voxels, vox_channels, rows_sel, imfeat, feat_channels, n_real, n_voxels, out, fm, ld);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_vfe_compact_input_frames(const float *voxels, int32_t vox_channels, const int32_t *rows_sel,
                                            const float *imfeat, int32_t feat_channels, int32_t n_real, int32_t n_voxels,
                                            float *out, const mvx_frames_t *frames_host, void *stream) {
    return mvx_vfe_compact_input_pitch_frames(voxels, vox_channels, rows_sel, imfeat, feat_channels, n_real, n_voxels, out,
                                              7 + feat_channels, frames_host, stream);
}

extern "C" int mvx_vfe_compact_input(const float *voxels, int32_t vox_channels, const int32_t *rows_sel,
                                     const float *imfeat, int32_t feat_channels, int32_t n_real, int32_t n_voxels,
                                     float *out, void *stream) {
    return mvx_vfe_compact_input_frames(voxels, vox_channels, rows_sel, imfeat, feat_channels, n_real, n_voxels, out, nullptr,
                                        stream);
}

extern "C" int mvx_vfe_compact_input_backward_frames(const float *grad_out, int32_t feat_channels, int32_t n_real,
                                                     int32_t n_voxels, float *dimfeat, double *scratch,
                                                     const mvx_frames_t *frames_host, void *stream) {
    MVX_CHECK_ARG(grad_out && dimfeat && scratch && feat_channels > 0 && feat_channels <= 256);
    MVX_CHECK_ARG(n_real >= 0 && n_voxels >= 0);
    VFE_FRAMES(fm);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(scratch, 0, sizeof(double) * feat_channels * fm.F, st);
    if (e != hipSuccess) return (int)e;
    const long long cells = (long long)n_real * feat_channels;
    const unsigned grid = (unsigned)(mvx_cdiv(cells, 1024) > 2048 ? 2048 : (mvx_cdiv(cells, 1024) < 256 ? 256 : mvx_cdiv(cells, 1024)));
    hipLaunchKernelGGL(vfe_compact_input_bwd, dim3(grid), dim3(256), 0, st, grad_out, feat_channels, n_real, n_voxels,
                       dimfeat, scratch, fm);
    MVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(vfe_compact_pad_finish, dim3(mvx_cdiv(feat_channels * fm.F, 64)), dim3(64), 0, st,
                       (const double *)scratch, dimfeat, n_real, feat_channels, fm.F);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_vfe_compact_input_backward(const float *grad_out, int32_t feat_channels, int32_t n_real,
                                              int32_t n_voxels, float *dimfeat, double *scratch, void *stream) {
    return mvx_vfe_compact_input_backward_frames(grad_out, feat_channels, n_real, n_voxels, dimfeat, scratch, nullptr, stream);
}
