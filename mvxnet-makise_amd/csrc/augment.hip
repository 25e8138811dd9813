// GT-paste augmentation for the frames of a step (reference modules/augment/Augment.py:12-114, train.py:28-42): ground grid,
// placement, point paste and image paste, one launch each for all frames.
//
//   1. gt_ground  (all frames, one thread per point): zmax[f][gx][gy] = largest z of the scene points of a cell (Augment.py
//                 check).  The grid holds f32 values and is raised with INTEGER atomics on the float's own bit pattern: a
//                 non-negative float orders like its signed integer (atomicMax), a negative one inversely like its unsigned
//                 integer (atomicMin).  The maximum of f32 values is exact, so the result does not depend on the order.
//   2. gt_place   (one workgroup per frame): the slots of a frame in sequence (Augment.py augment / locate); within a slot
//                 the (candidate x scene box) pairs run across the threads: the 2-D intersection over the scene box's area
//                 and the rotated BEV IoU (bev_iou.h, polygons in LDS; pairs whose bounding circles cannot touch count as
//                 0), then per candidate the three tests, the first passing candidate by an LDS integer atomicMin, and the
//                 winner's boxes appended to the LDS tables before the next slot.
//   3. gt_points  (one workgroup per (slot, frame)): the picked objects' rows [x y z r row col] appended behind the scene
//                 points in slot order, 16-byte stores.
//   4. gt_image   (grid (pixel blocks, slot, frame)): img = mask ? patch : img over every picked object's mask box; where
//                 picked objects overlap the LATER slot wins, decided per pixel so that no two threads store to one byte.
// No float atomics and no host synchronisation: every output is bitwise reproducible.
#include <string.h>
#include "bev_iou.h"

namespace {

constexpr int PLACE_THREADS = 128;          // 40 polygon slots of 8 B per thread: 40 KB of LDS
constexpr int MAXB = MVX_GT_PASTE_MAX_BOXES, MAXC = MVX_GT_PASTE_MAX_CAND;

struct Range { double lo_x, lo_y, hi_x, hi_y, cell_x, cell_y; };

// 1. -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gt_ground(const float *__restrict__ points6, const int *__restrict__ n_points, int F,
                                                 int cap_points, Range r, int gh, int gw, float *__restrict__ zmax) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)F * cap_points) return;
    const int f = (int)(e / cap_points), p = (int)(e - (long long)f * cap_points);
    if (p >= min(n_points[f], cap_points)) return;
    const float *pt = points6 + (size_t)e * 6;
    const double x = (double)pt[0], y = (double)pt[1];
    float z = pt[2];
    if (!(x >= r.lo_x && x < r.hi_x && y >= r.lo_y && y < r.hi_y) || z != z) return;      // outside the grid (NaN included)
    const int gx = (int)((x - r.lo_x) / r.cell_x), gy = (int)((y - r.lo_y) / r.cell_y);
    if (gx < 0 || gx >= gh || gy < 0 || gy >= gw) return;
    if (z == 0.f) z = 0.f;                                                                   // -0 counts as +0
    float *cell = zmax + ((size_t)f * gh + gx) * gw + gy;
    if (z >= 0.f) atomicMax((int *)cell, __float_as_int(z));
    else atomicMin((unsigned *)cell, __float_as_uint(z));
}

// 2. -------------------------------------------------------------------------------------------------------------------
struct PlaceArgs {
    const float *zmax;
    int gh, gw;
    float lo_x, lo_y, cell, z_margin, iou_thr;
    float *box2d, *box3d, *bev;
    const int *n_scene;
    int cap, lim;
    const int *cand;
    const float *thr;
    int s_max, n_cand;
    const float *db_box2d, *db_box3d, *db_bev;
    int n_db;
    int *picked, *n_out, *status, *dbg_fail;
    float *dbg_val;
};

__global__ __launch_bounds__(PLACE_THREADS) void gt_place(PlaceArgs a) {
    __shared__ P2 s_poly[POLY_SLOTS * PLACE_THREADS];
    __shared__ float s_b2[MAXB][4], s_area[MAXB], s_b3[MAXB][7], s_quad[MAXB][8], s_circ[MAXB][3];
    __shared__ float c_b2[MAXC][4], c_quad[MAXC][8], c_circ[MAXC][3], c_zg[MAXC];
    __shared__ int c_idx[MAXC], c_state[MAXC];       // c_state: -1 absent, 0 fails the ground test, 1 passes it
    __shared__ float s_iof[MAXC][MAXB], s_iou[MAXC][MAXB];
    __shared__ int s_win, s_n, s_bad;
    const int f = blockIdx.x, tid = threadIdx.x;
    float *g_b2 = a.box2d + (size_t)f * a.cap * 4, *g_b3 = a.box3d + (size_t)f * a.cap * 7, *g_bev = a.bev + (size_t)f * a.cap * 8;
    const int n0 = a.n_scene[f];
    int bad = 0;
    if (n0 < 0 || n0 > a.cap) bad |= MVX_GT_PASTE_BAD_COUNT;
    // n_scene is read once, before the loop (Augment.py:72); a frame over the limit gets nothing (:67)
    int S = (bad || n0 > a.lim) ? 0 : a.lim - n0;
    if (S > a.s_max) { S = a.s_max; bad |= MVX_GT_PASTE_SLOTS_SHORT; }
    if (tid == 0) { s_n = bad ? 0 : n0; s_bad = 0; }
    if (!bad) {
        for (int i = tid; i < n0; i += PLACE_THREADS) {
#pragma unroll
            for (int k = 0; k < 4; ++k) s_b2[i][k] = g_b2[i * 4 + k];
            s_area[i] = (s_b2[i][2] - s_b2[i][0]) * (s_b2[i][3] - s_b2[i][1]);
#pragma unroll
            for (int k = 0; k < 8; ++k) s_quad[i][k] = g_bev[i * 8 + k];
            circle_of(s_quad[i], s_circ[i]);
        }
    }
    __syncthreads();
    const Polys w = polys_of(s_poly, PLACE_THREADS, tid);
    for (int s = 0; s < a.s_max; ++s) {
        const size_t so = (size_t)f * a.s_max + s;
        if (s >= S) {                               // block-uniform
            if (tid == 0) a.picked[so] = -1;
            if (a.dbg_fail)
                for (int c = tid; c < a.n_cand; c += PLACE_THREADS) {
                    a.dbg_fail[so * a.n_cand + c] = -1;
                    for (int k = 0; k < 3; ++k) a.dbg_val[(so * a.n_cand + c) * 3 + k] = 0.f;
                }
            continue;
        }
        const int n = s_n;
        // ---- candidates: ground test, boxes into LDS
        if (tid < a.n_cand) {
            const int c = tid, idx = a.cand[so * a.n_cand + c];
            int state = -1;
            float zg = 0.f;
            if (idx >= a.n_db) s_bad = 1;           // benign race: every writer stores 1
            if (idx >= 0 && idx < a.n_db) {
                const float *b3 = a.db_box3d + (size_t)idx * 7;
                // f32 subtraction and a true f32 division by the cell size, truncated (Augment.py:38-39)
                const float qx = (b3[0] - a.lo_x) / a.cell, qy = (b3[1] - a.lo_y) / a.cell;
                state = 0;
                if (qx > -1.f && qx < (float)a.gh && qy > -1.f && qy < (float)a.gw) {
                    zg = a.zmax[((size_t)f * a.gh + (int)qx) * a.gw + (int)qy];
                    state = !(zg > b3[2] + a.z_margin);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) c_b2[c][k] = a.db_box2d[(size_t)idx * 4 + k];
#pragma unroll
                for (int k = 0; k < 8; ++k) c_quad[c][k] = a.db_bev[(size_t)idx * 8 + k];
                circle_of(c_quad[c], c_circ[c]);
            }
            c_idx[c] = idx;
            c_state[c] = state;
            c_zg[c] = zg;
        }
        if (tid == 0) s_win = MAXC;
        __syncthreads();
        // ---- pairs (candidate c, scene box i): 2-D intersection over the scene box's area, BEV IoU (candidate against box)
        for (int p = tid; p < a.n_cand * n; p += PLACE_THREADS) {
            const int c = p / n, i = p - c * n;
            if (c_state[c] < 0) continue;
            const float lx = fmaxf(s_b2[i][0], c_b2[c][0]), ly = fmaxf(s_b2[i][1], c_b2[c][1]);
            const float rx = fminf(s_b2[i][2], c_b2[c][2]), ry = fminf(s_b2[i][3], c_b2[c][3]);
            const float iw = fmaxf(rx - lx, 0.f), ih = fmaxf(ry - ly, 0.f);
            s_iof[c][i] = (iw * ih) / s_area[i];
            float iou = 0.f;
            const P2 c1 = {c_circ[c][0], c_circ[c][1]}, c2 = {s_circ[i][0], s_circ[i][1]};
            if (!circles_apart(c1, c_circ[c][2], c2, s_circ[i][2])) iou = quad_iou(w, c_quad[c], s_quad[i]);
            s_iou[c][i] = iou;
        }
        __syncthreads();
        // ---- per candidate: the first failing test (0 ground, 1 2-D, 2 BEV, 3 none), in the reference's order
        if (tid < a.n_cand) {
            const int c = tid;
            float m_iof = 0.f, m_iou = 0.f;
            int fail = -1;
            if (c_state[c] >= 0) {
                if (n > 0) {
                    m_iof = -INFINITY; m_iou = -INFINITY;
                    for (int i = 0; i < n; ++i) { m_iof = fmaxf(m_iof, s_iof[c][i]); m_iou = fmaxf(m_iou, s_iou[c][i]); }
                }
                fail = c_state[c] == 0 ? 0 : (n > 0 && m_iof > a.thr[so]) ? 1 : (n > 0 && m_iou > a.iou_thr) ? 2 : 3;
                if (fail == 3) atomicMin(&s_win, c);
            }
            if (a.dbg_fail) {
                a.dbg_fail[so * a.n_cand + c] = fail;
                float *v = a.dbg_val + (so * a.n_cand + c) * 3;
                v[0] = c_zg[c]; v[1] = m_iof; v[2] = m_iou;
            }
        }
        __syncthreads();
        // ---- the winner joins the scene (Augment.py:78-80)
        const int win = s_win;
        if (win < MAXC) {
            const int idx = c_idx[win];
            if (tid < 4) s_b2[n][tid] = c_b2[win][tid];
            if (tid == 4) s_area[n] = (c_b2[win][2] - c_b2[win][0]) * (c_b2[win][3] - c_b2[win][1]);
            if (tid >= 8 && tid < 16) s_quad[n][tid - 8] = c_quad[win][tid - 8];
            if (tid >= 16 && tid < 19) s_circ[n][tid - 16] = c_circ[win][tid - 16];
            if (tid >= 24 && tid < 31) s_b3[n][tid - 24] = a.db_box3d[(size_t)idx * 7 + tid - 24];
            if (tid == 0) { a.picked[so] = idx; s_n = n + 1; }
        } else if (tid == 0) {
            a.picked[so] = -1;
        }
        __syncthreads();
    }
    // ---- the grown tables: rows n0 .. n of this frame
    const int n = s_n;
    if (!bad) {
        for (int e = tid; e < (n - n0) * 8; e += PLACE_THREADS) {
            const int i = n0 + e / 8, k = e % 8;
            g_bev[i * 8 + k] = s_quad[i][k];
            if (k < 4) g_b2[i * 4 + k] = s_b2[i][k];
            if (k < 7) g_b3[i * 7 + k] = s_b3[i][k];
        }
    }
    if (tid == 0) {
        a.n_out[f] = bad ? n0 : n;
        const int st = bad | (s_bad ? MVX_GT_PASTE_BAD_INDEX : 0);
        if (st) atomicOr(a.status + f, st);
    }
}

// 3. -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gt_points(float *__restrict__ points6, const int *__restrict__ n_in, int *__restrict__ n_out,
                                                 int cap_points, const int *__restrict__ picked, int s_max,
                                                 const float *__restrict__ db_points, const long long *__restrict__ pt_off, int n_db,
                                                 int *__restrict__ status) {
    const int s = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    // every workgroup replays the frame's (short) slot list: objects in slot order, one that does not fit is dropped whole
    int off = min(max(n_in[f], 0), cap_points), mine = -1, overflow = 0;
    long long my_src = 0, my_cnt = 0;
    for (int k = 0; k < s_max; ++k) {
        const int idx = picked[(size_t)f * s_max + k];
        if (idx < 0 || idx >= n_db) continue;
        const long long lo = pt_off[idx], cnt = pt_off[idx + 1] - lo;
        if (cnt < 0 || off + cnt > cap_points) { overflow = 1; continue; }
        if (k == s) { mine = off; my_src = lo; my_cnt = cnt; }
        off += (int)cnt;
    }
    if (s == 0 && tid == 0) {
        n_out[f] = off;
        if (overflow) atomicOr(status + f, MVX_GT_PASTE_POINTS_OVERFLOW);
    }
    if (mine < 0) return;
    // rows of 24 B: both sides are 8-byte aligned; the destination is brought to 16 bytes with one 8-byte store
    float *dst = points6 + ((size_t)f * cap_points + mine) * 6;
    const float *src = db_points + (size_t)my_src * 6;
    const long long nfl = my_cnt * 6;
    const int head = (((uintptr_t)dst & 15) != 0 && nfl >= 2) ? 2 : 0;
    if (head && tid == 0) *(float2 *)dst = *(const float2 *)src;
    const long long n4 = (nfl - head) / 4;
    for (long long i = tid; i < n4; i += blockDim.x) {
        const float2 u = *(const float2 *)(src + head + 4 * i), v = *(const float2 *)(src + head + 4 * i + 2);
        *(float4 *)(dst + head + 4 * i) = make_float4(u.x, u.y, v.x, v.y);
    }
    if (nfl - head - 4 * n4 >= 2 && tid == 0) *(float2 *)(dst + head + 4 * n4) = *(const float2 *)(src + head + 4 * n4);
}

// 4. -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gt_image(unsigned char *__restrict__ img, int H, int W, const int *__restrict__ picked, int s_max,
                                                const unsigned char *__restrict__ patch, const unsigned char *__restrict__ mask,
                                                const long long *__restrict__ px_off, const int *__restrict__ maskbbox, int n_db) {
    __shared__ int s_box[MVX_GT_PASTE_MAX_SLOTS][4];
    __shared__ long long s_off[MVX_GT_PASTE_MAX_SLOTS];
    const int s = blockIdx.y, f = blockIdx.z, tid = threadIdx.x;
    const int idx = picked[(size_t)f * s_max + s];
    if (idx < 0 || idx >= n_db) return;
    // the later slots of this frame: where one of them covers a pixel with its mask, the pixel is theirs
    if (tid < s_max) {
        const int j = picked[(size_t)f * s_max + tid];
        bool on = tid > s && j >= 0 && j < n_db;
        if (on) {
            const int *bb = maskbbox + (size_t)j * 4;
            const long long w2 = (long long)bb[2] - bb[0] + 1, h2 = (long long)bb[3] - bb[1] + 1;
            on = w2 > 0 && h2 > 0 && w2 * h2 == px_off[j + 1] - px_off[j];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) s_box[tid][k] = on ? maskbbox[(size_t)j * 4 + k] : (k < 2 ? 1 : 0);      // empty box when off
        s_off[tid] = on ? px_off[j] : 0;
    }
    __syncthreads();
    const int x1 = maskbbox[(size_t)idx * 4], y1 = maskbbox[(size_t)idx * 4 + 1], x2 = maskbbox[(size_t)idx * 4 + 2],
              y2 = maskbbox[(size_t)idx * 4 + 3];
    const long long pw = (long long)x2 - x1 + 1, ph = (long long)y2 - y1 + 1, base = px_off[idx];
    if (pw <= 0 || ph <= 0 || pw * ph != px_off[idx + 1] - base) return;         // an inconsistent entry pastes nothing
    for (long long e = (long long)blockIdx.x * blockDim.x + tid; e < pw * ph; e += (long long)gridDim.x * blockDim.x) {
        const int x = x1 + (int)(e % pw), y = y1 + (int)(e / pw);
        if (x < 0 || x >= W || y < 0 || y >= H || mask[base + e] == 0) continue;
        bool later = false;
        for (int k = s + 1; k < s_max; ++k) {
            if (x < s_box[k][0] || x > s_box[k][2] || y < s_box[k][1] || y > s_box[k][3]) continue;
            const long long w2 = (long long)s_box[k][2] - s_box[k][0] + 1;
            later = later || mask[s_off[k] + (long long)(y - s_box[k][1]) * w2 + (x - s_box[k][0])] != 0;
        }
        if (later) continue;
        unsigned char *o = img + (((size_t)f * H + y) * W + x) * 3;
        const unsigned char *pp = patch + (size_t)(base + e) * 3;
        o[0] = pp[0]; o[1] = pp[1]; o[2] = pp[2];
    }
}

}  // namespace

extern "C" size_t mvx_gt_paste_workspace_bytes(int32_t n_frames, int32_t grid_h, int32_t grid_w) {
    const size_t F = n_frames > 0 ? n_frames : 0, h = grid_h > 0 ? grid_h : 0, w = grid_w > 0 ? grid_w : 0;
    return (F * h * w * sizeof(float) + 255) & ~(size_t)255;
}

extern "C" int mvx_gt_paste_ground_frames(const float *points6, const int32_t *n_points, int32_t n_frames, int32_t cap_points,
                                          double lo_x, double lo_y, double lo_z, double hi_x, double hi_y, int32_t grid_h,
                                          int32_t grid_w, float *zmax, size_t zmax_bytes, void *stream) {
    MVX_CHECK_ARG(n_frames >= 1 && n_frames <= MVX_MAX_FRAMES);
    MVX_CHECK_ARG(points6 && n_points && zmax && cap_points >= 1);
    MVX_CHECK_ARG(grid_h >= 1 && grid_w >= 1 && (long long)grid_h * grid_w < (1ll << 27));
    MVX_CHECK_ARG(hi_x > lo_x && hi_y > lo_y && lo_z == lo_z);
    MVX_CHECK_ARG(zmax_bytes >= mvx_gt_paste_workspace_bytes(n_frames, grid_h, grid_w) && ((uintptr_t)zmax & 3) == 0);
    hipStream_t st = (hipStream_t)stream;
    // empty cells: one below the range (Augment.py:19); a fill, then the one kernel
    const float init = (float)(lo_z - 1.0);
    unsigned bits;
    memcpy(&bits, &init, 4);
    hipError_t e = hipMemsetD32Async((hipDeviceptr_t)zmax, (int)bits, (size_t)n_frames * grid_h * grid_w, st);
    if (e != hipSuccess) return (int)e;
    const Range r = {lo_x, lo_y, hi_x, hi_y, (hi_x - lo_x) / grid_h, (hi_y - lo_y) / grid_w};
    hipLaunchKernelGGL(gt_ground, dim3(mvx_cdiv((long long)n_frames * cap_points, 256)), dim3(256), 0, st, points6, n_points, n_frames,
                       cap_points, r, grid_h, grid_w, zmax);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_gt_paste_place_frames(const float *zmax, int32_t grid_h, int32_t grid_w, float lo_x, float lo_y, float cell,
                                         float z_margin, float iou_thr, float *box2d, float *box3d, float *bev,
                                         const int32_t *n_scene, int32_t n_frames, int32_t cap, int32_t lim, const int32_t *cand,
                                         const float *thr, int32_t s_max, int32_t n_cand, const float *db_box2d,
                                         const float *db_box3d, const float *db_bev, int32_t n_db, int32_t *picked,
                                         int32_t *n_out, int32_t *status, int32_t *dbg_fail, float *dbg_val, void *stream) {
    MVX_CHECK_ARG(n_frames >= 1 && n_frames <= MVX_MAX_FRAMES);
    MVX_CHECK_ARG(grid_h >= 1 && grid_w >= 1 && (long long)grid_h * grid_w < (1ll << 27) && cell > 0.f);
    MVX_CHECK_ARG(cap >= 1 && cap <= MVX_GT_PASTE_MAX_BOXES && lim >= 0 && lim <= cap);
    MVX_CHECK_ARG(s_max >= 1 && s_max <= MVX_GT_PASTE_MAX_SLOTS && n_cand >= 1 && n_cand <= MVX_GT_PASTE_MAX_CAND && n_db >= 1);
    MVX_CHECK_ARG(iou_thr >= 1e-3f && iou_thr < 1.f && z_margin == z_margin);
    MVX_CHECK_ARG(zmax && box2d && box3d && bev && n_scene && cand && thr && db_box2d && db_box3d && db_bev);
    MVX_CHECK_ARG(picked && n_out && status);
    MVX_CHECK_ARG((dbg_fail == nullptr) == (dbg_val == nullptr));
    PlaceArgs a = {zmax, grid_h, grid_w, lo_x, lo_y, cell, z_margin, iou_thr, box2d, box3d, bev, n_scene, cap, lim, cand, thr,
                   s_max, n_cand, db_box2d, db_box3d, db_bev, n_db, picked, n_out, status, dbg_fail, dbg_val};
    hipLaunchKernelGGL(gt_place, dim3(n_frames), dim3(PLACE_THREADS), 0, (hipStream_t)stream, a);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_gt_paste_points_frames(float *points6, const int32_t *n_points, int32_t *n_points_out, int32_t n_frames,
                                          int32_t cap_points, const int32_t *picked, int32_t s_max, const float *db_points,
                                          const int64_t *pt_off, int32_t n_db, int32_t *status, void *stream) {
    MVX_CHECK_ARG(n_frames >= 1 && n_frames <= MVX_MAX_FRAMES);
    MVX_CHECK_ARG(points6 && n_points && n_points_out && n_points_out != n_points && picked && db_points && pt_off && status);
    MVX_CHECK_ARG(cap_points >= 1 && s_max >= 1 && s_max <= MVX_GT_PASTE_MAX_SLOTS && n_db >= 1);
    MVX_CHECK_ARG(((uintptr_t)points6 & 15) == 0 && ((uintptr_t)db_points & 15) == 0);
    hipLaunchKernelGGL(gt_points, dim3(s_max, n_frames), dim3(256), 0, (hipStream_t)stream, points6, n_points, n_points_out, cap_points,
                       picked, s_max, db_points, (const long long *)pt_off, n_db, status);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_gt_paste_image_frames(uint8_t *img, int32_t n_frames, int32_t h, int32_t w, const int32_t *picked, int32_t s_max,
                                         const uint8_t *patch, const uint8_t *mask, const int64_t *px_off, const int32_t *maskbbox,
                                         int32_t n_db, int64_t max_patch_px, void *stream) {
    MVX_CHECK_ARG(n_frames >= 1 && n_frames <= MVX_MAX_FRAMES);
    MVX_CHECK_ARG(img && picked && patch && mask && px_off && maskbbox);
    MVX_CHECK_ARG(h >= 1 && w >= 1 && (long long)h * w < (1ll << 28) && s_max >= 1 && s_max <= MVX_GT_PASTE_MAX_SLOTS && n_db >= 1);
    MVX_CHECK_ARG(max_patch_px >= 1);
    const long long blocks = (max_patch_px + 255) / 256;
    hipLaunchKernelGGL(gt_image, dim3((unsigned)(blocks < 64 ? blocks : 64), s_max, n_frames), dim3(256), 0, (hipStream_t)stream, img, h,
                       w, picked, s_max, patch, mask, (const long long *)px_off, maskbbox, n_db);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}
