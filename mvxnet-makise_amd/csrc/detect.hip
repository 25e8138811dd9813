// Detection output for the frames of a step: score selection, top-K, box decoding and rotated BEV NMS in four launches.
//
// The reference stops at the RPN's score / regression maps (its Calc.decodeRegression is never called and it has no NMS).
// Per frame, on the raw head output of rpn_frames.rpn_forward (or NCHW maps), read in place through element strides:
//   1. detect_keys    (all frames, one thread per anchor): ordered 32-bit key of every logit whose sigmoid passes score_thr
//                     (0 = not a candidate) into a contiguous key array, so the per-frame passes below read 16-byte vectors;
//   2. detect_select  (one 1024-thread workgroup per frame): radix select of the pre_max-th largest key (4 byte digits, LDS
//                     histograms), an ordered compaction (ties at the threshold key taken lowest anchor index first), a
//                     bitonic sort of <= 4096 64-bit keys (key << 32 | ~index) in LDS, then decode + BEV corners + bounding
//                     circle of every candidate;
//   3. detect_mask    (one 64-thread workgroup per (frame, 64-row block, 8 columns)): the K x ceil(K/64) u64
//                     suppression mask, bit j of row i = IoU(i, j) > iou_thr for j > i, with bboxOverlap's arithmetic
//                     (bev_iou.h); pairs whose bounding circles cannot touch skip the clipping (their IoU is 0);
//   4. detect_scan    (one wave per frame): the greedy scan, the removed bitmap one u64 per lane, mask rows streamed through
//                     LDS 64 rows at a time; writes the kept boxes.
// No float atomics and no host synchronisation: every output is bitwise reproducible.
//
// mvx_detect_frames_dir adds a fourth head, one direction logit x per anchor (the classifier mvx_focal_loss_dir_frames trains):
// detect_select folds the decoded yaw t = r6 + an6 into the half turn the bit names,
//   base = (t - dir_offset) - floor((t - dir_offset) / pi) pi,  t' = base + dir_offset + pi [x > 0],  wrapped into [-pi, pi),
// before the corners are formed, so the circle, the NMS and the output all see t'.  A null head is mvx_detect_frames.
//
// mvx_detect_frames_iou adds a fifth head, the IoU logit u per anchor that mvx_focal_loss_iou_frames trains, and iou_alpha = a
// in [0, 1]: the score becomes cls^(1-a) iou^a (CIA-SSD, AFDetV2), formed from the logits as its logarithm
//   s = -((1 - a) softplus(-c) + a softplus(-u)),  softplus(-x) = max(-x, 0) + log1p(exp(-|x|)).
// detect_keys admits an anchor when expf(s) >= score_thr (a NaN fails) and keys it by order_key(s); detect_select writes expf(s)
// as the score.  Boxes, direction fold, NMS and outputs are unchanged.  A null head, or a = 0, is mvx_detect_frames_dir.
#include "bev_iou.h"

namespace {

struct Head { const float *p; long long sf, sl, sw, sc; };

constexpr int SEL_THREADS = 1024;
constexpr int MASK_THREADS = 64;
constexpr int MASK_SPLIT = 8, MASK_COLS = MASK_THREADS / MASK_SPLIT;     // detect_mask: columns of a mask word per workgroup

// Per-frame region of the workspace (K = pre_max, NW = ceil(K / 64)); the key arrays of all frames follow the F regions.
struct Layout {
    long long K, NW, npad;
    size_t mask, box, quad, circ, score, idx, ok, meta, frame_bytes, keys;
    __host__ __device__ Layout(int k, int n_anchors, int F) {
        K = k;
        NW = (k + 63) / 64;
        npad = ((long long)n_anchors + 3) & ~3ll;
        mask = 0;
        box = mask + (size_t)K * NW * 8;
        quad = box + (size_t)K * 7 * 4;
        circ = quad + (size_t)K * 8 * 4;
        score = circ + (size_t)K * 4 * 4;
        idx = score + (size_t)K * 4;
        ok = idx + (size_t)K * 4;
        meta = ok + (size_t)K * 4;
        frame_bytes = (meta + 16 + 255) & ~(size_t)255;
        keys = frame_bytes * F;
    }
    __host__ __device__ size_t total(int F) const { return keys + (size_t)F * npad * 4 + 256; }
};

__device__ __forceinline__ float sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ long long head_off(const Head &h, int f, int x, int y, int c) {
    return f * h.sf + x * h.sl + y * h.sw + c * h.sc;
}

__device__ __forceinline__ float softplus_neg(float x) { return fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x))); }      // -log sigmoid(x)

// log of the rectified score cls^(1-a) iou^a from the two logits
__device__ __forceinline__ float rectified_log(float c, float u, float a) {
    return -((1.f - a) * softplus_neg(c) + a * softplus_neg(u));
}

// 1. keys[f][n] for every anchor n = (x*w + y)*A + a; the tail up to npad is 0
__global__ __launch_bounds__(256) void detect_keys(Head cls, Head iou, float iou_alpha, int F, int L, int W, int A, float score_thr,
                                                   unsigned *__restrict__ keys, long long npad) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)F * npad) return;
    const int f = (int)(e / npad);
    const long long n = e - f * npad;
    unsigned k = 0;
    if (n < (long long)L * W * A) {
        const int a = (int)(n % A), cell = (int)(n / A);
        const float logit = cls.p[head_off(cls, f, cell / W, cell % W, a)];
        if (iou.p) {                                                 // the rectified score (kernel-uniform branch)
            const float s = rectified_log(logit, iou.p[head_off(iou, f, cell / W, cell % W, a)], iou_alpha);
            if (expf(s) >= score_thr) k = order_key(s);             // NaN fails the comparison
        } else if (sigmoid(logit) >= score_thr) k = order_key(logit);      // NaN fails the comparison
    }
    keys[e] = k;
}

// 2. one workgroup per frame
__global__ __launch_bounds__(SEL_THREADS) void detect_select(Head cls, Head reg, Head dir, float dir_offset, Head iou, float iou_alpha,
                                                             const float *__restrict__ anchors, int L, int W, int A,
                                                             int decode, Layout lay, unsigned char *__restrict__ ws,
                                                             int *__restrict__ n_candidates, int *__restrict__ status,
                                                             int *__restrict__ dbg_idx, float *__restrict__ dbg_boxes,
                                                             float *__restrict__ dbg_corners) {
    __shared__ unsigned long long s_sort[MVX_DETECT_MAX_PRE];
    __shared__ int s_hist[256];
    __shared__ int s_scan[17];
    __shared__ int s_pick[2];
    __shared__ int s_bad;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int K = (int)lay.K;
    const uint4 *keys4 = (const uint4 *)(ws + lay.keys) + (size_t)f * (lay.npad / 4);
    const int n4 = (int)(lay.npad / 4);
    unsigned char *fr = ws + (size_t)f * lay.frame_bytes;

    // ---- radix select of the K-th largest non-zero key: prefix / mask of the digits fixed so far, kk = rank inside them
    unsigned prefix = 0, mask = 0;
    int kk = K, C = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int b = tid; b < 256; b += SEL_THREADS) s_hist[b] = 0;
        __syncthreads();
        for (int i = tid; i < n4; i += SEL_THREADS) {
            const uint4 v = keys4[i];
            const unsigned kv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (kv[q] != 0u && (kv[q] & mask) == prefix) atomicAdd(&s_hist[(kv[q] >> shift) & 255u], 1);
        }
        __syncthreads();
        // bins from the top: exclusive prefix of hist[255 - t]
        const int h = tid < 256 ? s_hist[255 - tid] : 0;
        int tot;
        const int above = block_excl_scan_i32(h, s_scan, &tot);
        if (shift == 24) {
            C = tot;
            if (C <= K) break;                  // every candidate fits: no selection (block-uniform)
        }
        if (tid < 256 && above < kk && above + h >= kk) { s_pick[0] = 255 - tid; s_pick[1] = above; }
        __syncthreads();
        prefix |= (unsigned)s_pick[0] << shift;
        mask |= 255u << shift;
        kk -= s_pick[1];
        __syncthreads();
    }
    const bool all = C <= K;
    const unsigned T = prefix;                  // the K-th largest key; K - kk keys lie above it, kk ties are taken
    const int need = kk, n_sel = all ? C : K;

    // ---- ordered compaction into s_sort: position = (selected before it in index order); packed (above, tie) scan
    int base_g = 0, base_e = 0;
    for (int i0 = 0; i0 < n4; i0 += SEL_THREADS) {
        const int i = i0 + tid;
        unsigned kv[4] = {0u, 0u, 0u, 0u};
        if (i < n4) { const uint4 v = keys4[i]; kv[0] = v.x; kv[1] = v.y; kv[2] = v.z; kv[3] = v.w; }
        int g = 0, e = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            g += all ? (kv[q] != 0u) : (kv[q] > T);
            e += !all && kv[q] == T;
        }
        int tot;
        const int ex = block_excl_scan_i32(g | (e << 16), s_scan, &tot);      // <= 4096 per chunk: no carry
        int gb = base_g + (ex & 0xffff), eb = base_e + (ex >> 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned long long key = ((unsigned long long)kv[q] << 32) | (unsigned)~(unsigned)(4 * i + q);
            if (all ? kv[q] != 0u : kv[q] > T) {
                s_sort[gb + min(eb, need)] = key;
                ++gb;
            } else if (!all && kv[q] == T) {
                if (eb < need) s_sort[gb + eb] = key;
                ++eb;
            }
        }
        base_g += tot & 0xffff;
        base_e += tot >> 16;
    }
    // ---- bitonic sort, descending: logit descending, then anchor index ascending (the ~index low word)
    int P = 1;
    while (P < n_sel) P <<= 1;
    for (int i = n_sel + tid; i < P; i += SEL_THREADS) s_sort[i] = 0ull;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += SEL_THREADS) {
                const int ij = i ^ j;
                if (ij > i) {
                    const unsigned long long a = s_sort[i], b = s_sort[ij];
                    if (((i & k) == 0) ? (a < b) : (a > b)) { s_sort[i] = b; s_sort[ij] = a; }
                }
            }
            __syncthreads();
        }
    }

    // ---- decode, corners (Calc.bbox3d2bev), bounding circle
    float *c_box = (float *)(fr + lay.box), *c_quad = (float *)(fr + lay.quad), *c_circ = (float *)(fr + lay.circ);
    float *c_score = (float *)(fr + lay.score);
    int *c_idx = (int *)(fr + lay.idx), *c_ok = (int *)(fr + lay.ok);
    for (int i = tid; i < K; i += SEL_THREADS) {
        if (i >= n_sel) {
            if (dbg_idx) dbg_idx[(size_t)f * K + i] = -1;
            continue;
        }
        const int n = (int)~(unsigned)s_sort[i];
        const int a = n % A, cell = n / A, x = cell / W, y = cell % W;
        const float *an = anchors + (size_t)n * 7;
        float r[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) r[k] = reg.p[head_off(reg, f, x, y, a * 7 + k)];
        // 'loss': the inverse of VoxelLoss's targets (voxelnet/Loss.py:35-40), diagonal of (l, w);
        // 'reference': Calc.decodeRegression as written, diagonal of anchor columns 0:2
        const float d = decode == MVX_DETECT_DECODE_REFERENCE ? sqrtf(an[0] * an[0] + an[1] * an[1])
                                                              : sqrtf(an[3] * an[3] + an[4] * an[4]);
        float b[7];
        b[0] = r[0] * d + an[0];
        b[1] = r[1] * d + an[1];
        b[2] = r[2] * an[5] + an[2];
        b[3] = expf(r[3]) * an[3];
        b[4] = expf(r[4]) * an[4];
        b[5] = expf(r[5]) * an[5];
        b[6] = r[6] + an[6];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 7; ++k) ok = ok && isfinite(b[k]);
        if (dir.p && isfinite(b[6])) {              // the half turn the direction bit names; a non-finite yaw stays as it is
            const float PI = 3.14159265358979323846f, PI_BELOW = 3.14159250f;      // PI rounds above pi, PI_BELOW is the float under it
            const float v = b[6] - dir_offset;
            const float base = v - floorf(v / PI) * PI;
            float t = base + dir_offset + (dir.p[head_off(dir, f, x, y, a)] > 0.f ? PI : 0.f);
            t -= floorf((t + PI) / (2.f * PI)) * (2.f * PI);
            if (t > PI_BELOW) t -= 2.f * PI;
            b[6] = fmaxf(t, -PI_BELOW);             // [-pi, pi) as real numbers too
        }
        P2 q[4];
        box_quad(b, q);
        P2 c;
        float rad;
        quad_circle(q, c, rad);
#pragma unroll
        for (int k = 0; k < 7; ++k) c_box[(size_t)i * 7 + k] = b[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) { c_quad[(size_t)i * 8 + 2 * k] = q[k].x; c_quad[(size_t)i * 8 + 2 * k + 1] = q[k].y; }
        c_circ[(size_t)i * 4] = c.x;
        c_circ[(size_t)i * 4 + 1] = c.y;
        c_circ[(size_t)i * 4 + 2] = rad;
        c_circ[(size_t)i * 4 + 3] = 0.f;
        const float logit = cls.p[head_off(cls, f, x, y, a)];
        c_score[i] = iou.p ? expf(rectified_log(logit, iou.p[head_off(iou, f, x, y, a)], iou_alpha)) : sigmoid(logit);
        c_idx[i] = n;
        c_ok[i] = ok;
        if (!ok) s_bad = 1;                     // benign race: every writer stores 1
        if (dbg_idx) {
            dbg_idx[(size_t)f * K + i] = n;
#pragma unroll
            for (int k = 0; k < 7; ++k) dbg_boxes[((size_t)f * K + i) * 7 + k] = b[k];
#pragma unroll
            for (int k = 0; k < 8; ++k) dbg_corners[((size_t)f * K + i) * 8 + k] = c_quad[(size_t)i * 8 + k];
        }
    }
    __syncthreads();
    if (tid == 0) {
        ((int *)(fr + lay.meta))[0] = n_sel;
        n_candidates[f] = C;
        status[f] = (C > K ? MVX_DETECT_TRUNCATED : 0) | (s_bad ? MVX_DETECT_NONFINITE : 0);
    }
}

// 3. grid (column block * MASK_SPLIT + column part, row block, frame), 64 threads: thread t owns row i = 64 * row block + t
// and the 8 columns of its part, i.e. byte `part` of the mask word (little endian: bits 8 part .. 8 part + 7).  Splitting the
// 64 columns of a word over 8 workgroups gives the latency-bound clipping loop 8x the waves.
__global__ __launch_bounds__(MASK_THREADS) void detect_mask(Layout lay, unsigned char *__restrict__ ws, float iou_thr) {
    __shared__ P2 s_poly[POLY_SLOTS * MASK_THREADS];
    __shared__ float s_quad[MASK_COLS * 8];
    __shared__ float s_circ[MASK_COLS * 4];
    __shared__ int s_ok[MASK_COLS];
    const int cb = blockIdx.x / MASK_SPLIT, part = blockIdx.x % MASK_SPLIT, rb = blockIdx.y, f = blockIdx.z, t = threadIdx.x;
    unsigned char *fr = ws + (size_t)f * lay.frame_bytes;
    const int n_sel = ((const int *)(fr + lay.meta))[0];
    if (rb * MASK_THREADS >= n_sel || cb * MASK_THREADS >= n_sel) return;        // words the scan never reads
    unsigned char *mask = fr + lay.mask;
    const int i = rb * MASK_THREADS + t;
    const size_t byte = ((size_t)i * lay.NW + cb) * 8 + part;
    if (cb < rb) {                              // only bits j > i are used: the lower blocks are zero
        if (i < n_sel) mask[byte] = 0;
        return;
    }
    const float *quad = (const float *)(fr + lay.quad), *circ = (const float *)(fr + lay.circ);
    const int *okv = (const int *)(fr + lay.ok);
    const int j0 = cb * MASK_THREADS + part * MASK_COLS;
    if (t < MASK_COLS && j0 + t < n_sel) {
#pragma unroll
        for (int k = 0; k < 8; ++k) s_quad[t * 8 + k] = quad[(size_t)(j0 + t) * 8 + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) s_circ[t * 4 + k] = circ[(size_t)(j0 + t) * 4 + k];
        s_ok[t] = okv[j0 + t];
    }
    __syncthreads();
    if (i >= n_sel) return;
    unsigned bits = 0u;
    if (okv[i]) {
        const Polys w = polys_of(s_poly, MASK_THREADS, t);
        const float a1 = load_oriented(w.q1, quad + (size_t)i * 8);     // row i once, outside the column loop
        const P2 c1 = {circ[(size_t)i * 4], circ[(size_t)i * 4 + 1]};
        const float r1 = circ[(size_t)i * 4 + 2];
        const int jn = min(MASK_COLS, n_sel - j0);
        for (int jj = 0; jj < jn; ++jj) {
            const int j = j0 + jj;
            if (j <= i || !s_ok[jj]) continue;
            const P2 c2 = {s_circ[jj * 4], s_circ[jj * 4 + 1]};
            if (circles_apart(c1, r1, c2, s_circ[jj * 4 + 2])) continue;
            const float a2 = load_oriented(w.q2, s_quad + jj * 8);
            const float inter = quad_intersection(w.q1, w.q2, w.p, w.q);
            const float iou = inter / (a1 + a2 - inter);
            if (iou > iou_thr) bits |= 1u << jj;
        }
    }
    mask[byte] = (unsigned char)bits;
}

// 4. one wave per frame: greedy suppression in candidate order, at most post_max kept; writes the outputs
__global__ __launch_bounds__(64) void detect_scan(Layout lay, const unsigned char *__restrict__ ws, int post_max,
                                                  float *__restrict__ boxes, float *__restrict__ scores,
                                                  int *__restrict__ anchor_idx, int *__restrict__ counts) {
    __shared__ unsigned long long s_rows[64][64];
    __shared__ int s_keep[MVX_DETECT_MAX_PRE];
    const int f = blockIdx.x, lane = threadIdx.x;
    const unsigned char *fr = ws + (size_t)f * lay.frame_bytes;
    const int n_sel = ((const int *)(fr + lay.meta))[0];
    const int nw = (n_sel + 63) / 64;
    const unsigned long long *mask = (const unsigned long long *)(fr + lay.mask);
    const int *okv = (const int *)(fr + lay.ok);
    // lane L holds the removed bits of candidates 64L .. 64L+63; non-finite candidates start removed
    unsigned long long rem = 0ull;
    for (int b = 0; b < 64; ++b) {
        const int j = lane * 64 + b;
        if (j < n_sel && !okv[j]) rem |= 1ull << b;
    }
    int cnt = 0;
    for (int c0 = 0; c0 < n_sel && cnt < post_max; c0 += 64) {
        const int rows = min(64, n_sel - c0), cw = c0 >> 6;
        for (int e = lane; e < rows * nw; e += 64) {
            const int r = e / nw, wd = e - r * nw;
            s_rows[r][wd] = mask[(size_t)(c0 + r) * lay.NW + wd];
        }
        __syncthreads();
        unsigned long long word = __shfl(rem, cw, 64);          // this chunk's removed bits (wave-uniform from here on)
        for (int r = 0; r < rows; ++r) {
            if ((word >> r) & 1ull) continue;
            if (lane == 0) s_keep[cnt] = c0 + r;
            ++cnt;
            if (lane < nw) rem |= s_rows[r][lane];
            word |= s_rows[r][cw];
            if (cnt == post_max) break;
        }
        __syncthreads();
    }
    const float *c_box = (const float *)(fr + lay.box), *c_score = (const float *)(fr + lay.score);
    const int *c_idx = (const int *)(fr + lay.idx);
    for (int k = lane; k < post_max; k += 64) {
        const size_t o = (size_t)f * post_max + k;
        if (k < cnt) {
            const int s = s_keep[k];
#pragma unroll
            for (int c = 0; c < 7; ++c) boxes[o * 7 + c] = c_box[(size_t)s * 7 + c];
            scores[o] = c_score[s];
            anchor_idx[o] = c_idx[s];
        } else {
#pragma unroll
            for (int c = 0; c < 7; ++c) boxes[o * 7 + c] = 0.f;
            scores[o] = 0.f;
            anchor_idx[o] = -1;
        }
    }
    if (lane == 0) counts[f] = cnt;
}

}  // namespace

extern "C" size_t mvx_detect_workspace_bytes(int32_t n_frames, int32_t n_anchors, int32_t pre_max) {
    const int F = n_frames > 0 ? n_frames : 0;
    return Layout(pre_max > 0 ? pre_max : 0, n_anchors > 0 ? n_anchors : 0, F).total(F);
}

extern "C" int mvx_detect_frames_iou(const float *cls, int64_t cls_sf, int64_t cls_sl, int64_t cls_sw, int64_t cls_sa, const float *reg,
                                     int64_t reg_sf, int64_t reg_sl, int64_t reg_sw, int64_t reg_sc, const float *dir,
                                     int64_t dir_sf, int64_t dir_sl, int64_t dir_sw, int64_t dir_sa, float dir_offset,
                                     const float *iou, int64_t iou_sf, int64_t iou_sl, int64_t iou_sw, int64_t iou_sa,
                                     float iou_alpha, const float *anchors, int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc,
                                     float score_thr, float iou_thr, int32_t pre_max, int32_t post_max, int32_t decode, float *boxes,
                                     float *scores, int32_t *anchor_idx, int32_t *counts, int32_t *n_candidates, int32_t *status,
                                     int32_t *dbg_idx, float *dbg_boxes, float *dbg_corners, void *workspace, size_t workspace_bytes,
                                     void *stream) {
    MVX_CHECK_ARG(!dir || dir_offset == dir_offset);
    MVX_CHECK_ARG(iou_alpha >= 0.f && iou_alpha <= 1.f);      // a NaN fails both
    if (iou_alpha == 0.f) iou = nullptr;                      // cls^1 iou^0: the plain score and key, bit for bit; the head is not read
    MVX_CHECK_ARG(n_frames >= 1 && n_frames <= MVX_MAX_FRAMES);
    MVX_CHECK_ARG(pre_max >= 1 && pre_max <= MVX_DETECT_MAX_PRE && post_max >= 1 && post_max <= pre_max);
    MVX_CHECK_ARG(iou_thr >= 1e-3f && iou_thr < 1.f && score_thr >= 0.f && score_thr < 1.f);
    MVX_CHECK_ARG(decode == MVX_DETECT_DECODE_LOSS || decode == MVX_DETECT_DECODE_REFERENCE);
    MVX_CHECK_ARG(l > 0 && w > 0 && anchors_per_loc > 0 && (long long)l * w * anchors_per_loc < (1ll << 31) - 4);
    MVX_CHECK_ARG(cls && reg && anchors && workspace);
    MVX_CHECK_ARG(boxes && scores && anchor_idx && counts && n_candidates && status);
    MVX_CHECK_ARG((dbg_idx == nullptr) == (dbg_boxes == nullptr) && (dbg_idx == nullptr) == (dbg_corners == nullptr));
    const int n_anchors = l * w * anchors_per_loc;
    const Layout lay(pre_max, n_anchors, n_frames);
    MVX_CHECK_ARG(workspace_bytes >= lay.total(n_frames));
    MVX_CHECK_ARG(((uintptr_t)workspace & 255) == 0);
    hipStream_t st = (hipStream_t)stream;
    unsigned char *ws = (unsigned char *)workspace;
    const Head hc = {cls, cls_sf, cls_sl, cls_sw, cls_sa}, hr = {reg, reg_sf, reg_sl, reg_sw, reg_sc};
    const Head hd = {dir, dir_sf, dir_sl, dir_sw, dir_sa}, hu = {iou, iou_sf, iou_sl, iou_sw, iou_sa};
    const long long tot = (long long)n_frames * lay.npad;
    hipLaunchKernelGGL(detect_keys, dim3(mvx_cdiv(tot, 256)), dim3(256), 0, st, hc, hu, iou_alpha, n_frames, l, w, anchors_per_loc,
                       score_thr, (unsigned *)(ws + lay.keys), lay.npad);
    MVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(detect_select, dim3(n_frames), dim3(SEL_THREADS), 0, st, hc, hr, hd, dir_offset, hu, iou_alpha, anchors, l, w,
                       anchors_per_loc, decode, lay, ws, n_candidates, status, dbg_idx, dbg_boxes, dbg_corners);
    MVX_LAUNCH_CHECK();
    const unsigned nb = (unsigned)lay.NW;
    hipLaunchKernelGGL(detect_mask, dim3(nb * MASK_SPLIT, nb, n_frames), dim3(MASK_THREADS), 0, st, lay, ws, iou_thr);
    MVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(detect_scan, dim3(n_frames), dim3(64), 0, st, lay, ws, post_max, boxes, scores, anchor_idx, counts);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_detect_frames_dir(const float *cls, int64_t cls_sf, int64_t cls_sl, int64_t cls_sw, int64_t cls_sa, const float *reg,
                                     int64_t reg_sf, int64_t reg_sl, int64_t reg_sw, int64_t reg_sc, const float *dir,
                                     int64_t dir_sf, int64_t dir_sl, int64_t dir_sw, int64_t dir_sa, float dir_offset,
                                     const float *anchors, int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc,
                                     float score_thr, float iou_thr, int32_t pre_max, int32_t post_max, int32_t decode, float *boxes,
                                     float *scores, int32_t *anchor_idx, int32_t *counts, int32_t *n_candidates, int32_t *status,
                                     int32_t *dbg_idx, float *dbg_boxes, float *dbg_corners, void *workspace, size_t workspace_bytes,
                                     void *stream) {
    return mvx_detect_frames_iou(cls, cls_sf, cls_sl, cls_sw, cls_sa, reg, reg_sf, reg_sl, reg_sw, reg_sc, dir, dir_sf, dir_sl, dir_sw,
                                 dir_sa, dir_offset, nullptr, 0, 0, 0, 0, 0.f, anchors, n_frames, l, w, anchors_per_loc, score_thr,
                                 iou_thr, pre_max, post_max, decode, boxes, scores, anchor_idx, counts, n_candidates, status, dbg_idx,
                                 dbg_boxes, dbg_corners, workspace, workspace_bytes, stream);
}

extern "C" int mvx_detect_frames(const float *cls, int64_t cls_sf, int64_t cls_sl, int64_t cls_sw, int64_t cls_sa, const float *reg,
                                 int64_t reg_sf, int64_t reg_sl, int64_t reg_sw, int64_t reg_sc, const float *anchors,
                                 int32_t n_frames, int32_t l, int32_t w, int32_t anchors_per_loc, float score_thr, float iou_thr,
                                 int32_t pre_max, int32_t post_max, int32_t decode, float *boxes, float *scores,
                                 int32_t *anchor_idx, int32_t *counts, int32_t *n_candidates, int32_t *status, int32_t *dbg_idx,
                                 float *dbg_boxes, float *dbg_corners, void *workspace, size_t workspace_bytes, void *stream) {
    return mvx_detect_frames_dir(cls, cls_sf, cls_sl, cls_sw, cls_sa, reg, reg_sf, reg_sl, reg_sw, reg_sc, nullptr, 0, 0, 0, 0, 0.f,
                                 anchors, n_frames, l, w, anchors_per_loc, score_thr, iou_thr, pre_max, post_max, decode, boxes,
                                 scores, anchor_idx, counts, n_candidates, status, dbg_idx, dbg_boxes, dbg_corners, workspace,
                                 workspace_bytes, stream);
}
