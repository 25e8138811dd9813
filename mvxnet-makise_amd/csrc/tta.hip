// Test-time augmentation, the fusion half: the detections of V views of a source frame (a view = a global rotation, scale and
// y flip of the cloud, geom_points' global step) brought back into the source frame and turned into one list, three launches
// for all frames.
//
// Input is the padded output of the detection step over F * V frames, view-major inside a source frame (frame f * V + v is
// view v of source frame f), and the views' rows (phi, s, flip, 0) as Geometry.draw_geometry writes them.
//   1. tta_merge  (one 1024-thread workgroup per source frame): every box through the inverse of Geometry.transform_boxes in
//                 f64, rounded to f32 once (an identity row copies bitwise); the N = V * post_max entries ordered by score
//                 descending, then view, then rank ascending (a bitonic sort of 64-bit keys in LDS, as detect_select's); BEV
//                 quad and bounding circle with detect_select's arithmetic (bev_iou.h); a non-finite box or score is dropped
//                 (MVX_TTA_NONFINITE);
//   2. tta_mask   (detect_mask's launch shape and arithmetic): from ONE IoU per pair j > i two bit matrices, `sup`
//                 (IoU > iou_thr) and `vote` (IoU > fuse_iou); circles_apart counts as IoU 0; pairs of the same view are pairs
//                 like any other;
//   3. tta_fuse   (one wave per source frame): the greedy scan in merged order -- entry i is a head iff no earlier head has
//                 its sup bit on i, a non-head belongs to the FIRST head that suppresses it; a member votes for its head iff
//                 its vote bit with the head is set and no earlier entry of its view has voted for that head (the head votes
//                 first, for its own view); the score-weighted f64 averages over the voters in merged order; clusters with
//                 fewer than min_views voters dropped; the rest ordered by fused score descending, then head position.
//
// The heads are exactly the boxes a greedy NMS over the union of the views would keep, in their original poses.  Averaging
// moves them: IoU <= iou_thr holds between the heads, not strictly between the fused poses.  Yaw differences are wrapped
// into the half turn [-pi/2, pi/2) (a model without direction head does not tell a box from its half-turn twin) or, with
// full_turn, into [-pi, pi); for car-shaped boxes (l / w about 2.4) a fuse_iou above roughly 0.26 excludes voters a quarter
// turn off the head, so the half-turn wrap never sits near its seam.
// No float atomics, no host synchronisation, every sum in a fixed order: two runs are bitwise identical.
#include "bev_iou.h"

namespace {

constexpr int MERGE_THREADS = MVX_TTA_MAX_BOXES;
constexpr int MASK_THREADS = 64;
constexpr int MASK_SPLIT = 8, MASK_COLS = MASK_THREADS / MASK_SPLIT;     // tta_mask: columns of a mask word per workgroup
constexpr int MAX_NW = MVX_TTA_MAX_BOXES / 64;
constexpr double PI_D = 3.14159265358979323846;

// Per-source-frame region of the workspace (N = V * post_max, NW = ceil(N / 64)); fbox / fscore / fnv: the fused clusters,
// indexed by their head's merged position.
struct Layout {
    long long N, NW;
    size_t sup, vote, box, quad, circ, score, prov, fbox, fscore, fnv, meta, frame_bytes;
    __host__ __device__ Layout(int n) {
        N = n;
        NW = (n + 63) / 64;
        sup = 0;
        vote = sup + (size_t)N * NW * 8;
        box = vote + (size_t)N * NW * 8;
        quad = box + (size_t)N * 7 * 4;
        circ = quad + (size_t)N * 8 * 4;
        score = circ + (size_t)N * 4 * 4;
        prov = score + (size_t)N * 4;
        fbox = prov + (size_t)N * 4;
        fscore = fbox + (size_t)N * 7 * 4;
        fnv = fscore + (size_t)N * 4;
        meta = fnv + (size_t)N * 4;
        frame_bytes = (meta + 16 + 255) & ~(size_t)255;
    }
    __host__ __device__ size_t total(int F) const { return frame_bytes * F; }
};

// r (f64) into [-period/2, period/2)
__device__ __forceinline__ double wrap_to(double r, double period) { return r - period * floor((r + 0.5 * period) / period); }

// ... into [-pi, pi), rounded to f32 once; the result is in [-pi, pi) as a real number too (detect_select's clamp)
__device__ __forceinline__ float wrap_pi_f32(double r) {
    const float PI_BELOW = 3.14159250f;
    const float t = (float)wrap_to(r, 2.0 * PI_D);
    return t > PI_BELOW ? -PI_BELOW : fmaxf(t, -PI_BELOW);
}

// A view's box `in` back in the source frame: the inverse of Geometry.transform_boxes for the row vw = (phi, s, flip, 0).
// Returns whether every component of the result is finite.
__device__ __forceinline__ bool to_source(const float *in, const float *vw, float *o) {
    if (vw[0] == 0.f && vw[1] == 1.f && vw[2] == 0.f) {
#pragma unroll
        for (int k = 0; k < 7; ++k) o[k] = in[k];
    } else {
        double x = (double)in[0], y = (double)in[1], r = (double)in[6];
        if (vw[2] != 0.f) { y = -y; r = -r; }
        const double phi = (double)vw[0], s = (double)vw[1];
        const double c = cos(phi), sn = sin(phi);
        o[0] = (float)((c * x - sn * y) / s);           // xy @ R(-phi), R of Calc.getRotationMatrices on row vectors
        o[1] = (float)((sn * x + c * y) / s);
        o[2] = (float)((double)in[2] / s);
#pragma unroll
        for (int k = 3; k < 6; ++k) o[k] = (float)((double)in[k] / s);
        o[6] = wrap_pi_f32(r - phi);
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 7; ++k) ok = ok && isfinite(o[k]);
    return ok;
}

// 1. one workgroup per source frame; thread e = view * post_max + rank
__global__ __launch_bounds__(MERGE_THREADS) void tta_merge(const float *__restrict__ boxes, const float *__restrict__ scores,
                                                           const int *__restrict__ counts, const float *__restrict__ views, int V,
                                                           int post_max, Layout lay, unsigned char *__restrict__ ws,
                                                           int *__restrict__ status) {
    __shared__ unsigned long long s_sort[MVX_TTA_MAX_BOXES];
    __shared__ int s_bad;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int N = (int)lay.N;
    unsigned char *fr = ws + (size_t)f * lay.frame_bytes;
    const float *fboxes = boxes + (size_t)f * N * 7, *fscores = scores + (size_t)f * N;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    unsigned long long key = 0ull;
    if (tid < N) {
        const int v = tid / post_max, rank = tid - v * post_max;
        const int cnt = min(max(counts[f * V + v], 0), post_max);
        if (rank < cnt) {
            float o[7];
            const float sc = fscores[tid];
            if (to_source(fboxes + (size_t)tid * 7, views + v * 4, o) && isfinite(sc))
                key = ((unsigned long long)order_key(sc) << 32) | (unsigned)~(unsigned)tid;
            else
                s_bad = 1;                      // benign race: every writer stores 1
        }
    }
    s_sort[tid] = key;
    const int n = __syncthreads_count(key != 0ull);
    // ---- bitonic sort, descending: score descending, then view * post_max + rank ascending (the ~index low word)
    int P = 1;
    while (P < N) P <<= 1;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int i = tid, ij = i ^ j;
            if (i < P && ij > i) {
                const unsigned long long a = s_sort[i], b = s_sort[ij];
                if (((i & k) == 0) ? (a < b) : (a > b)) { s_sort[i] = b; s_sort[ij] = a; }
            }
            __syncthreads();
        }
    }
    if (tid < n) {
        const int e = (int)~(unsigned)s_sort[tid];
        float b[7];
        to_source(fboxes + (size_t)e * 7, views + (e / post_max) * 4, b);
        P2 q[4];
        box_quad(b, q);
        P2 c;
        float rad;
        quad_circle(q, c, rad);
        float *c_box = (float *)(fr + lay.box), *c_quad = (float *)(fr + lay.quad), *c_circ = (float *)(fr + lay.circ);
#pragma unroll
        for (int k = 0; k < 7; ++k) c_box[(size_t)tid * 7 + k] = b[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) { c_quad[(size_t)tid * 8 + 2 * k] = q[k].x; c_quad[(size_t)tid * 8 + 2 * k + 1] = q[k].y; }
        c_circ[(size_t)tid * 4] = c.x;
        c_circ[(size_t)tid * 4 + 1] = c.y;
        c_circ[(size_t)tid * 4 + 2] = rad;
        c_circ[(size_t)tid * 4 + 3] = 0.f;
        ((float *)(fr + lay.score))[tid] = fscores[e];
        ((int *)(fr + lay.prov))[tid] = e;
    }
    if (tid == 0) {
        ((int *)(fr + lay.meta))[0] = n;
        status[f] = s_bad ? MVX_TTA_NONFINITE : 0;
    }
}

// 2. grid (column block * MASK_SPLIT + column part, row block, source frame), 64 threads: thread t owns row i = 64 * row block
// + t and the 8 columns of its part, byte `part` of the two mask words (detect_mask's shape)
__global__ __launch_bounds__(MASK_THREADS) void tta_mask(Layout lay, unsigned char *__restrict__ ws, float iou_thr, float fuse_iou) {
    __shared__ P2 s_poly[POLY_SLOTS * MASK_THREADS];
    __shared__ float s_quad[MASK_COLS * 8];
    __shared__ float s_circ[MASK_COLS * 4];
    const int cb = blockIdx.x / MASK_SPLIT, part = blockIdx.x % MASK_SPLIT, rb = blockIdx.y, f = blockIdx.z, t = threadIdx.x;
    unsigned char *fr = ws + (size_t)f * lay.frame_bytes;
    const int n = ((const int *)(fr + lay.meta))[0];
    if (rb * MASK_THREADS >= n || cb * MASK_THREADS >= n) return;                // words the scan never reads
    unsigned char *sup = fr + lay.sup, *vote = fr + lay.vote;
    const int i = rb * MASK_THREADS + t;
    const size_t byte = ((size_t)i * lay.NW + cb) * 8 + part;
    if (cb < rb) {                              // only bits j > i are used: the lower blocks are zero
        if (i < n) { sup[byte] = 0; vote[byte] = 0; }
        return;
    }
    const float *quad = (const float *)(fr + lay.quad), *circ = (const float *)(fr + lay.circ);
    const int j0 = cb * MASK_THREADS + part * MASK_COLS;
    if (t < MASK_COLS && j0 + t < n) {
#pragma unroll
        for (int k = 0; k < 8; ++k) s_quad[t * 8 + k] = quad[(size_t)(j0 + t) * 8 + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) s_circ[t * 4 + k] = circ[(size_t)(j0 + t) * 4 + k];
    }
    __syncthreads();
    if (i >= n) return;
    unsigned sbits = 0u, vbits = 0u;
    const Polys w = polys_of(s_poly, MASK_THREADS, t);
    const float a1 = load_oriented(w.q1, quad + (size_t)i * 8);         // row i once, outside the column loop
    const P2 c1 = {circ[(size_t)i * 4], circ[(size_t)i * 4 + 1]};
    const float r1 = circ[(size_t)i * 4 + 2];
    const int jn = min(MASK_COLS, n - j0);
    for (int jj = 0; jj < jn; ++jj) {
        const int j = j0 + jj;
        if (j <= i) continue;
        const P2 c2 = {s_circ[jj * 4], s_circ[jj * 4 + 1]};
        if (circles_apart(c1, r1, c2, s_circ[jj * 4 + 2])) continue;
        const float a2 = load_oriented(w.q2, s_quad + jj * 8);
        const float inter = quad_intersection(w.q1, w.q2, w.p, w.q);
        const float iou = inter / (a1 + a2 - inter);
        if (iou > iou_thr) sbits |= 1u << jj;
        if (iou > fuse_iou) vbits |= 1u << jj;
    }
    sup[byte] = (unsigned char)sbits;
    vote[byte] = (unsigned char)vbits;
}

// 3. one wave per source frame
__global__ __launch_bounds__(64) void tta_fuse(Layout lay, unsigned char *__restrict__ ws, int V, int post_max, int min_views,
                                               int out_max, int full_turn, float *__restrict__ boxes, float *__restrict__ scores,
                                               int *__restrict__ n_views, int *__restrict__ src, int *__restrict__ counts) {
    __shared__ unsigned long long s_rows[64][MAX_NW];
    __shared__ unsigned long long s_sort[MVX_TTA_MAX_BOXES];
    __shared__ int s_owner[MVX_TTA_MAX_BOXES];
    __shared__ int s_head[MVX_TTA_MAX_BOXES];
    __shared__ int s_kept;
    const int f = blockIdx.x, lane = threadIdx.x;
    unsigned char *fr = ws + (size_t)f * lay.frame_bytes;
    const int n = ((const int *)(fr + lay.meta))[0];
    const int nw = (n + 63) / 64;
    const unsigned long long *sup = (const unsigned long long *)(fr + lay.sup), *vote = (const unsigned long long *)(fr + lay.vote);
    const float *c_box = (const float *)(fr + lay.box), *c_score = (const float *)(fr + lay.score);
    const int *c_prov = (const int *)(fr + lay.prov);
    float *f_box = (float *)(fr + lay.fbox), *f_score = (float *)(fr + lay.fscore);
    int *f_nv = (int *)(fr + lay.fnv);
    if (lane == 0) s_kept = 0;
    // ---- heads and owners: lane L holds the suppressed bits of entries 64L .. 64L+63 (detect_scan's walk, without a cap)
    unsigned long long rem = 0ull;
    int cnt = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int rows = min(64, n - c0), cw = c0 >> 6;
        for (int e = lane; e < rows * nw; e += 64) {
            const int r = e / nw, wd = e - r * nw;
            s_rows[r][wd] = sup[(size_t)(c0 + r) * lay.NW + wd];
        }
        __syncthreads();
        unsigned long long word = __shfl(rem, cw, 64);          // this chunk's suppressed bits (wave-uniform from here on)
        for (int r = 0; r < rows; ++r) {
            if ((word >> r) & 1ull) continue;
            const int h = c0 + r;
            if (lane == 0) s_head[cnt] = h;
            ++cnt;
            if (lane < nw) {
                unsigned long long fresh = s_rows[r][lane] & ~rem;          // first suppressed by this head: its members
                rem |= fresh;
                while (fresh) {
                    s_owner[lane * 64 + __ffsll((long long)fresh) - 1] = h;
                    fresh &= fresh - 1ull;
                }
            }
            word |= s_rows[r][cw];
        }
        __syncthreads();
    }
    // ---- one cluster per lane at a time: the votes and the f64 sums, voters in merged order
    int P = 1;
    while (P < cnt) P <<= 1;
    const double period = full_turn ? 2.0 * PI_D : PI_D;
    for (int k = lane; k < P; k += 64) {
        unsigned long long key = 0ull;
        if (k < cnt) {
            const int h = s_head[k];
            const float *bh = c_box + (size_t)h * 7;
            const double wh = (double)c_score[h], rh = (double)bh[6];
            double sw = wh, sd = 0.0, sq[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) sq[c] = wh * (double)bh[c];
            unsigned seen = 1u << (c_prov[h] / post_max);
            int nv = 1;
            for (int wd = h >> 6; wd < nw; ++wd) {
                unsigned long long bits = vote[(size_t)h * lay.NW + wd];
                while (bits) {
                    const int j = wd * 64 + __ffsll((long long)bits) - 1;
                    bits &= bits - 1ull;
                    if (s_owner[j] != h) continue;
                    const unsigned vb = 1u << (c_prov[j] / post_max);
                    if (seen & vb) continue;
                    seen |= vb;
                    const float *bj = c_box + (size_t)j * 7;
                    const double wj = (double)c_score[j];
                    sw += wj;
#pragma unroll
                    for (int c = 0; c < 6; ++c) sq[c] += wj * (double)bj[c];
                    sd += wj * wrap_to((double)bj[6] - rh, period);
                    ++nv;
                }
            }
            float o[7];
            if (nv == 1 || !(sw > 0.0)) {       // the head alone (or weights that sum to nothing): its box as it is
#pragma unroll
                for (int c = 0; c < 7; ++c) o[c] = bh[c];
            } else {
#pragma unroll
                for (int c = 0; c < 6; ++c) o[c] = (float)(sq[c] / sw);
                o[6] = wrap_pi_f32(rh + sd / sw);
            }
            const float fs = (float)(sw / (double)V);
#pragma unroll
            for (int c = 0; c < 7; ++c) f_box[(size_t)h * 7 + c] = o[c];
            f_score[h] = fs;
            f_nv[h] = nv;
            if (nv >= min_views) {
                key = ((unsigned long long)order_key(fs) << 32) | (unsigned)~(unsigned)h;
                atomicAdd(&s_kept, 1);
            }
        }
        s_sort[k] = key;
    }
    __syncthreads();
    // ---- fused score descending, then head position ascending
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = lane; i < P; i += 64) {
                const int ij = i ^ j;
                if (ij > i) {
                    const unsigned long long a = s_sort[i], b = s_sort[ij];
                    if (((i & k) == 0) ? (a < b) : (a > b)) { s_sort[i] = b; s_sort[ij] = a; }
                }
            }
            __syncthreads();
        }
    }
    const int n_out = min(s_kept, out_max);
    for (int k = lane; k < out_max; k += 64) {
        const size_t o = (size_t)f * out_max + k;
        if (k < n_out) {
            const int h = (int)~(unsigned)s_sort[k];
#pragma unroll
            for (int c = 0; c < 7; ++c) boxes[o * 7 + c] = f_box[(size_t)h * 7 + c];
            scores[o] = f_score[h];
            n_views[o] = f_nv[h];
            src[o] = c_prov[h];
        } else {
#pragma unroll
            for (int c = 0; c < 7; ++c) boxes[o * 7 + c] = 0.f;
            scores[o] = 0.f;
            n_views[o] = 0;
            src[o] = -1;
        }
    }
    if (lane == 0) counts[f] = n_out;
}

}  // namespace

extern "C" size_t mvx_tta_workspace_bytes(int32_t n_frames, int32_t n_views, int32_t post_max) {
    const long long n = (long long)(n_views > 0 ? n_views : 0) * (post_max > 0 ? post_max : 0);
    if (n > MVX_TTA_MAX_BOXES) return 0;
    return Layout((int)n).total(n_frames > 0 ? n_frames : 0);
}

extern "C" int mvx_tta_fuse_frames(const float *boxes, const float *scores, const int32_t *counts, const float *views,
                                   int32_t n_frames, int32_t n_views, int32_t post_max, float iou_thr, float fuse_iou,
                                   int32_t min_views, int32_t out_max, int32_t full_turn, float *out_boxes, float *out_scores,
                                   int32_t *out_n_views, int32_t *out_src, int32_t *out_counts, int32_t *status, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    MVX_CHECK_ARG(n_frames >= 1 && n_frames <= MVX_MAX_FRAMES && n_views >= 1 && n_views <= MVX_TTA_MAX_VIEWS);
    MVX_CHECK_ARG(post_max >= 1 && (long long)n_views * post_max <= MVX_TTA_MAX_BOXES);
    MVX_CHECK_ARG(iou_thr >= 1e-3f && iou_thr <= fuse_iou && fuse_iou < 1.f);
    MVX_CHECK_ARG(min_views >= 1 && min_views <= n_views && out_max >= 1 && out_max <= n_views * post_max);
    MVX_CHECK_ARG(boxes && scores && counts && views && workspace);
    MVX_CHECK_ARG(out_boxes && out_scores && out_n_views && out_src && out_counts && status);
    const Layout lay(n_views * post_max);
    MVX_CHECK_ARG(workspace_bytes >= lay.total(n_frames));
    MVX_CHECK_ARG(((uintptr_t)workspace & 255) == 0);
    hipStream_t st = (hipStream_t)stream;
    unsigned char *ws = (unsigned char *)workspace;
    hipLaunchKernelGGL(tta_merge, dim3(n_frames), dim3(MERGE_THREADS), 0, st, boxes, scores, counts, views, n_views, post_max, lay, ws,
                       status);
    MVX_LAUNCH_CHECK();
    const unsigned nb = (unsigned)lay.NW;
    hipLaunchKernelGGL(tta_mask, dim3(nb * MASK_SPLIT, nb, n_frames), dim3(MASK_THREADS), 0, st, lay, ws, iou_thr, fuse_iou);
    MVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(tta_fuse, dim3(n_frames), dim3(64), 0, st, lay, ws, n_views, post_max, min_views, out_max, full_turn, out_boxes,
                       out_scores, out_n_views, out_src, out_counts);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}
