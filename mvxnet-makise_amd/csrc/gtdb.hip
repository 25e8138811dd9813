// Builder of the GT-paste object database (reference create_gtdatabase.py) for the frames of a call: label boxes against
// instance annotations, instance polygons into masks and patches, points inside every oriented 3-D box.  All stages are
// batched over the labels of all frames (n_labels rows, any order; the host sorts them by class, frame, row).
//
//   1. gtdb_match  (one thread per label): torchvision box_iou in f32 against the annotation boxes of the label's group
//                  (frame x class), the maximum and the first index reaching it, the flag iou >= 0.65, the annotation box
//                  truncated to int and clipped to the frame's image (the ROI); then gtdb_scan, one workgroup: px_off = the
//                  exclusive scan of the objects' ROI pixel counts.
//   2. gtdb_count  (grid (chunk of 1024 points, label)): how many points of the label's frame lie inside its box, per
//                  chunk; then gtdb_offsets, one workgroup: the chunk counts become offsets inside the object, the
//                  objects' totals become pt_off.  Positions come from counts and scans alone -- no atomics.
//   3. gtdb_raster (grid (band of 8 ROI rows, label)): the instance's polygon edges staged in LDS, a pixel is set when its
//                  centre is inside any polygon by the even-odd rule; mask byte and patch = mask ? bgr : 0.  One thread owns
//                  a pixel: its mask byte and its three patch bytes have no other writer.
//   4. gtdb_write  (same grid as 2): the inside test again, the rank inside the chunk (compact.h), rows [x y z r] stored in
//                  file order with 16-byte loads and stores.
// The f64 decisions (crossing test, box faces) use a fixed operand order and the file is built with -ffp-contract=off, so a
// host restatement in the same order gives the same bits.
#include "box3d.h"
#include "compact.h"

namespace {

constexpr int THREADS = 256;
constexpr int CHUNK = MVX_GTDB_CHUNK;       // points per workgroup of stages 2 and 4
constexpr int BAND = 8;                     // ROI rows per workgroup of stage 3
constexpr int EDGES = 512;                  // polygon edges per LDS stage: 16 KB of f64 + 2 KB of polygon ids

// inclusive scan of a[0..n) in place by ONE workgroup of THREADS threads: trips of THREADS with a carry; s: 17 words
__device__ void scan_inplace(long long *a, int n, long long *s) {
    long long carry = 0;
    for (int base = 0; base < n; base += THREADS) {
        const int i = base + threadIdx.x;
        const long long v = i < n ? a[i] : 0;
        long long tot;
        const long long ex = block_excl_scan<long long>(v, s, &tot);
        if (i < n) a[i] = carry + ex + v;
        carry += tot;
    }
}

// 1. -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void gtdb_match(const float4 *__restrict__ lab_box2d, const int *__restrict__ lab_group,
                                                      const int *__restrict__ lab_frame, int n_labels,
                                                      const float4 *__restrict__ ann_box, const int *__restrict__ ann_off,
                                                      int n_groups, const int *__restrict__ im_hw, int n_frames, float thr,
                                                      int *__restrict__ best, float *__restrict__ iou, int *__restrict__ flag,
                                                      int4 *__restrict__ roi, long long *__restrict__ px_off) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_labels) return;
    const int g = lab_group[i], f = lab_frame[i];
    int b = -1, fl = 0;
    float bi = -INFINITY;
    int4 r = make_int4(0, 0, -1, -1);
    long long cnt = 0;
    if (g >= 0 && g < n_groups && f >= 0 && f < n_frames) {
        const float4 p = lab_box2d[i];
        const float area1 = (p.z - p.x) * (p.w - p.y);
        for (int a = ann_off[g]; a < ann_off[g + 1]; ++a) {
            const float4 q = ann_box[a];
            const float area2 = (q.z - q.x) * (q.w - q.y);
            const float w = fmaxf(fminf(p.z, q.z) - fmaxf(p.x, q.x), 0.f), h = fmaxf(fminf(p.w, q.w) - fmaxf(p.y, q.y), 0.f);
            const float inter = w * h;
            const float v = inter / (area1 + area2 - inter);
            if (v > bi) { bi = v; b = a; }            // the first index that reaches the maximum; a NaN never does
        }
        if (b >= 0) {
            const float4 q = ann_box[b];
            const float lim = 1.0e9f;
            const int x1 = (int)fminf(fmaxf(q.x, -lim), lim), y1 = (int)fminf(fmaxf(q.y, -lim), lim);
            const int x2 = (int)fminf(fmaxf(q.z, -lim), lim), y2 = (int)fminf(fmaxf(q.w, -lim), lim);
            r = make_int4(max(x1, 0), max(y1, 0), min(x2, im_hw[2 * f + 1] - 1), min(y2, im_hw[2 * f] - 1));
            fl = (bi >= thr ? 1 : 0) | ((r.z >= r.x && r.w >= r.y) ? 2 : 0);
            if (fl == 3) cnt = (long long)(r.z - r.x + 1) * (r.w - r.y + 1);
        }
    }
    best[i] = b;
    iou[i] = b >= 0 ? bi : 0.f;
    flag[i] = fl;
    roi[i] = r;
    px_off[i + 1] = cnt;
    if (i == 0) px_off[0] = 0;
}

__global__ __launch_bounds__(THREADS) void gtdb_scan(long long *off, int n) {
    __shared__ long long s[17];
    scan_inplace(off + 1, n, s);
}

// 2 / 4. ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Box label_box(const float *__restrict__ lab_box3d, const float *__restrict__ lab_cs, int i) {
    return load_box(lab_box3d + (size_t)i * 7, (double)lab_cs[(size_t)i * 2], (double)lab_cs[(size_t)i * 2 + 1]);      // the host's cos / sin
}
__device__ __forceinline__ bool inside(const Box &b, const float4 &p) { return inside(b, (double)p.x, (double)p.y, (double)p.z); }

__global__ __launch_bounds__(THREADS) void gtdb_count(const float4 *__restrict__ points, const long long *__restrict__ pts_off,
                                                      int n_frames, const float *__restrict__ lab_box3d,
                                                      const float *__restrict__ lab_cs, const int *__restrict__ lab_frame,
                                                      const int *__restrict__ flag, int n_chunks, int *__restrict__ chunk_cnt) {
    __shared__ int s_cnt[THREADS / MVX_WAVE];
    const int chunk = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
    const int f = lab_frame[i];
    int total = 0;
    if (flag[i] == 3 && f >= 0 && f < n_frames) {                 // block-uniform
        const long long lo = pts_off[f], n = pts_off[f + 1] - lo;
        if ((long long)chunk * CHUNK < n) {
            const Box b = label_box(lab_box3d, lab_cs, i);
            int mine = 0;
            for (int k = 0; k < CHUNK / THREADS; ++k) {
                const long long p = (long long)chunk * CHUNK + k * THREADS + tid;
                if (p < n) mine += inside(b, points[lo + p]);
            }
            mine = wave_sum_i32(mine);
            if ((tid & 63) == 0) s_cnt[tid >> 6] = mine;
            __syncthreads();
            for (int k = 0; k < THREADS / MVX_WAVE; ++k) total += s_cnt[k];
        }
    }
    if (tid == 0) chunk_cnt[(size_t)i * n_chunks + chunk] = total;
}

__global__ __launch_bounds__(THREADS) void gtdb_offsets(int *__restrict__ chunk_cnt, int n_chunks, long long *__restrict__ pt_off,
                                                        int n_labels) {
    __shared__ long long s[17];
    for (int i = threadIdx.x; i < n_labels; i += THREADS) {
        int *row = chunk_cnt + (size_t)i * n_chunks;
        int run = 0;
        for (int k = 0; k < n_chunks; ++k) { const int c = row[k]; row[k] = run; run += c; }
        pt_off[i + 1] = run;
    }
    if (threadIdx.x == 0) pt_off[0] = 0;
    __syncthreads();
    scan_inplace(pt_off + 1, n_labels, s);
}

__global__ __launch_bounds__(THREADS) void gtdb_write(const float4 *__restrict__ points, const long long *__restrict__ pts_off,
                                                      int n_frames, const float *__restrict__ lab_box3d,
                                                      const float *__restrict__ lab_cs, const int *__restrict__ lab_frame,
                                                      const int *__restrict__ flag, int n_chunks, const int *__restrict__ chunk_off,
                                                      const long long *__restrict__ pt_off, float4 *__restrict__ out,
                                                      long long out_rows) {
    __shared__ int s_cnt[2][THREADS / MVX_WAVE];
    const int chunk = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
    const int f = lab_frame[i];
    if (flag[i] != 3 || f < 0 || f >= n_frames) return;            // block-uniform
    const long long lo = pts_off[f], n = pts_off[f + 1] - lo;
    if ((long long)chunk * CHUNK >= n) return;
    const Box b = label_box(lab_box3d, lab_cs, i);
    const long long end = pt_off[i + 1];
    long long at = pt_off[i] + chunk_off[(size_t)i * n_chunks + chunk];
    for (int k = 0; k < CHUNK / THREADS; ++k) {                    // file order: sub-chunk, then thread
        const long long p = (long long)chunk * CHUNK + k * THREADS + tid;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        bool in = false;
        if (p < n) { v = points[lo + p]; in = inside(b, v); }
        int all;
        const long long dst = at + block_kept_rank<THREADS / MVX_WAVE>(in, s_cnt[k & 1], all);      // the rows alternate: one barrier per sub-chunk
        if (in && dst < end && dst < out_rows) out[dst] = v;
        at += all;
    }
}

// 3. -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void gtdb_raster(const unsigned char *__restrict__ images, int n_frames, int H, int W,
                                                       const int *__restrict__ lab_frame, const int *__restrict__ flag,
                                                       const int *__restrict__ best, const int4 *__restrict__ roi,
                                                       const long long *__restrict__ px_off, const double *__restrict__ edges,
                                                       const int *__restrict__ edge_poly, const int *__restrict__ edge_off,
                                                       int n_ann, unsigned char *__restrict__ mask,
                                                       unsigned char *__restrict__ patch, long long n_px) {
    __shared__ double s_e[EDGES][4];
    __shared__ int s_p[EDGES];
    const int band = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
    const int f = lab_frame[i], a = best[i];
    if (flag[i] != 3 || f < 0 || f >= n_frames || a < 0 || a >= n_ann) return;          // block-uniform
    const int4 r = roi[i];
    if (r.x < 0 || r.y < 0 || r.z >= W || r.w >= H) return;
    const int rw = r.z - r.x + 1, rh = r.w - r.y + 1;
    const long long base = px_off[i];
    if ((long long)rw * rh != px_off[i + 1] - base || base + (long long)rw * rh > n_px) return;
    const int row0 = band * BAND;
    if (row0 >= rh) return;
    const int rows = min(BAND, rh - row0), n_pix = rows * rw;
    const int e0 = edge_off[a], ne = edge_off[a + 1] - e0;
    int staged = -1;
    for (int p0 = 0; p0 < n_pix; p0 += THREADS) {
        const int p = p0 + tid;
        const bool live = p < n_pix;
        const int yy = row0 + (live ? p / rw : 0), xx = live ? p % rw : 0;
        const double px = (double)(r.x + xx) + 0.5, py = (double)(r.y + yy) + 0.5;
        int cur = -1;
        bool par = false, in = false;
        for (int c0 = 0; c0 < ne || c0 == 0; c0 += EDGES) {
            if (staged != c0) {                                    // one stage serves every pixel batch when the edges fit
                __syncthreads();
                for (int e = tid; e < min(EDGES, ne - c0); e += THREADS) {
                    const double *g = edges + (size_t)(e0 + c0 + e) * 4;
                    s_e[e][0] = g[0]; s_e[e][1] = g[1]; s_e[e][2] = g[2]; s_e[e][3] = g[3];
                    s_p[e] = edge_poly[e0 + c0 + e];
                }
                __syncthreads();
                staged = c0;
            }
            const int m = min(EDGES, ne - c0);
            for (int e = 0; e < m; ++e) {
                if (s_p[e] != cur) { in = in || par; par = false; cur = s_p[e]; }
                const double x0 = s_e[e][0], y0 = s_e[e][1], x1 = s_e[e][2], y1 = s_e[e][3];
                if ((y0 > py) != (y1 > py)) {
                    const double xi = (x1 - x0) * (py - y0) / (y1 - y0) + x0;
                    if (px < xi) par = !par;
                }
            }
        }
        in = in || par;
        if (live) {
            const long long o = base + (long long)yy * rw + xx;
            const unsigned char *src = images + (((size_t)f * H + (r.y + yy)) * W + (r.x + xx)) * 3;
            mask[o] = in ? 1 : 0;
            patch[o * 3] = in ? src[0] : 0;
            patch[o * 3 + 1] = in ? src[1] : 0;
            patch[o * 3 + 2] = in ? src[2] : 0;
        }
    }
}

inline int n_chunks_of(long long max_frame_points) {
    const long long n = (max_frame_points + CHUNK - 1) / CHUNK;
    return n > 0 ? (int)n : 1;
}

}  // namespace

extern "C" size_t mvx_gtdb_workspace_bytes(int32_t n_labels, int32_t max_frame_points) {
    const size_t n = n_labels > 0 ? n_labels : 0;
    return (n * n_chunks_of(max_frame_points > 0 ? max_frame_points : 0) * sizeof(int32_t) + 255) & ~(size_t)255;
}

extern "C" int mvx_gtdb_match(const float *lab_box2d, const int32_t *lab_group, const int32_t *lab_frame, int32_t n_labels,
                              const float *ann_box, const int32_t *ann_off, int32_t n_groups, const int32_t *im_hw,
                              int32_t n_frames, float iou_thr, int32_t *best, float *iou, int32_t *flag, int32_t *roi,
                              int64_t *px_off, void *stream) {
    MVX_CHECK_ARG(n_labels >= 1 && n_labels < (1 << 24) && n_groups >= 1 && n_frames >= 1);
    MVX_CHECK_ARG(lab_box2d && lab_group && lab_frame && ann_box && ann_off && im_hw && best && iou && flag && roi && px_off);
    MVX_CHECK_ARG(iou_thr > 0.f && iou_thr <= 1.f);
    MVX_CHECK_ARG(((uintptr_t)lab_box2d & 15) == 0 && ((uintptr_t)ann_box & 15) == 0 && ((uintptr_t)roi & 15) == 0);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gtdb_match, dim3(mvx_cdiv(n_labels, THREADS)), dim3(THREADS), 0, st, (const float4 *)lab_box2d, lab_group,
                       lab_frame, n_labels, (const float4 *)ann_box, ann_off, n_groups, im_hw, n_frames, iou_thr, best, iou, flag,
                       (int4 *)roi, (long long *)px_off);
    MVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(gtdb_scan, dim3(1), dim3(THREADS), 0, st, (long long *)px_off, n_labels);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_gtdb_crop_count(const float *points, const int64_t *pts_off, int32_t n_frames, int32_t max_frame_points,
                                   const float *lab_box3d, const float *lab_cs, const int32_t *lab_frame, const int32_t *flag,
                                   int32_t n_labels, int64_t *pt_off, void *workspace, size_t workspace_bytes, void *stream) {
    MVX_CHECK_ARG(n_labels >= 1 && n_labels <= 65535 && n_frames >= 1 && max_frame_points >= 0);
    MVX_CHECK_ARG(points && pts_off && lab_box3d && lab_cs && lab_frame && flag && pt_off && workspace);
    MVX_CHECK_ARG(((uintptr_t)points & 15) == 0 && ((uintptr_t)workspace & 3) == 0);
    MVX_CHECK_ARG(workspace_bytes >= mvx_gtdb_workspace_bytes(n_labels, max_frame_points));
    const int nc = n_chunks_of(max_frame_points);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gtdb_count, dim3(nc, n_labels), dim3(THREADS), 0, st, (const float4 *)points, (const long long *)pts_off,
                       n_frames, lab_box3d, lab_cs, lab_frame, flag, nc, (int *)workspace);
    MVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(gtdb_offsets, dim3(1), dim3(THREADS), 0, st, (int *)workspace, nc, (long long *)pt_off, n_labels);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_gtdb_crop_write(const float *points, const int64_t *pts_off, int32_t n_frames, int32_t max_frame_points,
                                   const float *lab_box3d, const float *lab_cs, const int32_t *lab_frame, const int32_t *flag,
                                   int32_t n_labels, const int64_t *pt_off, const void *workspace, size_t workspace_bytes,
                                   float *out_points, int64_t out_rows, void *stream) {
    MVX_CHECK_ARG(n_labels >= 1 && n_labels <= 65535 && n_frames >= 1 && max_frame_points >= 0 && out_rows >= 1);
    MVX_CHECK_ARG(points && pts_off && lab_box3d && lab_cs && lab_frame && flag && pt_off && workspace && out_points);
    MVX_CHECK_ARG(((uintptr_t)points & 15) == 0 && ((uintptr_t)out_points & 15) == 0 && ((uintptr_t)workspace & 3) == 0);
    MVX_CHECK_ARG(workspace_bytes >= mvx_gtdb_workspace_bytes(n_labels, max_frame_points));
    const int nc = n_chunks_of(max_frame_points);
    hipLaunchKernelGGL(gtdb_write, dim3(nc, n_labels), dim3(THREADS), 0, (hipStream_t)stream, (const float4 *)points,
                       (const long long *)pts_off, n_frames, lab_box3d, lab_cs, lab_frame, flag, nc, (const int *)workspace,
                       (const long long *)pt_off, (float4 *)out_points, (long long)out_rows);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_gtdb_raster(const uint8_t *images, int32_t n_frames, int32_t h, int32_t w, const int32_t *lab_frame,
                               const int32_t *flag, const int32_t *best, const int32_t *roi, const int64_t *px_off,
                               int32_t n_labels, const double *edges, const int32_t *edge_poly, const int32_t *edge_off,
                               int32_t n_ann, int32_t max_roi_rows, uint8_t *mask, uint8_t *patch, int64_t n_px, void *stream) {
    MVX_CHECK_ARG(n_labels >= 1 && n_labels <= 65535 && n_frames >= 1 && n_ann >= 1);
    MVX_CHECK_ARG(h >= 1 && w >= 1 && (long long)h * w < (1ll << 28) && max_roi_rows >= 1 && max_roi_rows <= h && n_px >= 1);
    MVX_CHECK_ARG(images && lab_frame && flag && best && roi && px_off && edges && edge_poly && edge_off && mask && patch);
    MVX_CHECK_ARG(((uintptr_t)roi & 15) == 0 && ((uintptr_t)edges & 7) == 0);
    hipLaunchKernelGGL(gtdb_raster, dim3(mvx_cdiv(max_roi_rows, BAND), n_labels), dim3(THREADS), 0, (hipStream_t)stream, images,
                       n_frames, h, w, lab_frame, flag, best, (const int4 *)roi, (const long long *)px_off, edges, edge_poly,
                       edge_off, n_ann, mask, patch, (long long)n_px);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}
