// BEV rotated-box IoU device functions shared by target assignment, NMS, evaluation and the two augmentations.
//
// The arithmetic of the reference's cpp/voxelutil.cpp:18-116 (bboxOverlap), operation for operation in f32: origin-fan
// triangulation, half-plane cuts with the 1e-6 tolerance, shoelace areas halved in f64.  Every translation unit that
// includes this header is compiled with -ffp-contract=off, so all users produce bit-identical IoUs.
#pragma once
#include "common.h"

namespace {

struct P2 { float x, y; };

// The polygons of the clipping live in LDS, one slot column per thread (element i of thread t at base[i * stride + t]:
// consecutive lanes hit consecutive 8-byte words, no bank conflicts).  Thread-private arrays indexed by run-time counters
// (q[m++]) are placed in scratch memory by the compiler: 336 B per thread and ~2,000 dependent scratch accesses per IoU
// made one classifyAnchors call of 8 boxes take 0.5 ms.
struct LP {
    P2 *b;
    int stride;
    __device__ __forceinline__ P2 &operator[](int i) const { return b[i * stride]; }
};
constexpr int POLY_SLOTS = 40;          // per thread: p[10] | q[20] | quad 1 [5] | quad 2 [5]

constexpr float TOL = 1e-6f;

__device__ __forceinline__ int sgn(float d) { return (d > TOL) - (d < -TOL); }

__device__ __forceinline__ float cross3(P2 o, P2 a, P2 b) { return (a.x - o.x) * (b.y - o.y) - (b.x - o.x) * (a.y - o.y); }

__device__ __forceinline__ bool same_pt(P2 p, P2 q) { return sgn(p.x - q.x) == 0 && sgn(p.y - q.y) == 0; }

// shoelace area of ps[0..n) (ps[n] is set to ps[0]); f32 accumulation, the halving in f64 (voxelutil.cpp:31-38)
__device__ float shoelace(LP ps, int n) {
    float acc = 0.f;
    ps[n] = ps[0];
    for (int i = 0; i < n; ++i) {
        const P2 u = ps[i], v = ps[i + 1];
        acc += u.x * v.y - u.y * v.x;
    }
    return (float)((double)acc / 2.0);
}

// polygon p[0..n) cut by the half plane left of (a, b) (voxelutil.cpp:50-63); q: 20 slots of scratch
__device__ void cut(LP p, int &n, P2 a, P2 b, LP q) {
    int m = 0;
    p[n] = p[0];
    for (int i = 0; i < n; ++i) {
        const P2 pi = p[i], pj = p[i + 1];
        const float s1 = cross3(a, b, pi), s2 = cross3(a, b, pj);
        const int g1 = sgn(s1), g2 = sgn(s2);
        if (g1 > 0) q[m++] = pi;
        if (g1 != g2) {
            // The reference consumes a slot even when |s2 - s1| <= 1e-6 makes it skip the crossing (voxelutil.cpp:44),
            // leaving whatever an EARLIER call stored there; call history does not exist here, the slot takes p[i].
            P2 c = pi;
            if (sgn(s2 - s1) != 0) {
                c.x = (pi.x * s2 - pj.x * s1) / (s2 - s1);
                c.y = (pi.y * s2 - pj.y * s1) / (s2 - s1);
            }
            q[m++] = c;
        }
    }
    n = 0;
    for (int i = 0; i < m; ++i)
        if (i == 0 || !same_pt(q[i], q[i - 1])) p[n++] = q[i];
    while (n > 1 && same_pt(p[n - 1], p[0])) --n;
}

// signed intersection area of the origin triangles (o,a,b) and (o,c,d) (voxelutil.cpp:65-79); p: 10 slots, q: 20 slots
__device__ float tri_pair(P2 a, P2 b, P2 c, P2 d, LP p, LP q) {
    const P2 o = {0.f, 0.f};
    const int s1 = sgn(cross3(o, a, b)), s2 = sgn(cross3(o, c, d));
    if (s1 == 0 || s2 == 0) return 0.f;
    if (s1 == -1) { const P2 t = a; a = b; b = t; }
    if (s2 == -1) { const P2 t = c; c = d; d = t; }
    p[0] = o; p[1] = a; p[2] = b;
    int n = 3;
    cut(p, n, o, c, q);
    cut(p, n, c, d, q);
    cut(p, n, d, o, q);
    const float res = (float)fabs((double)shoelace(p, n));
    return (s1 * s2 == -1) ? -res : res;
}

__device__ void orient_ccw(LP q) {      // voxelutil.cpp:82-83
    if (shoelace(q, 4) < 0.f) {
        P2 t = q[0]; q[0] = q[3]; q[3] = t;
        t = q[1]; q[1] = q[2]; q[2] = t;
    }
    q[4] = q[0];
}

// q1, q2: 5 slots each, both already oriented (orient_ccw)
__device__ float quad_intersection(LP q1, LP q2, LP p, LP q) {
    float res = 0.f;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) res += tri_pair(q1[i], q1[i + 1], q2[j], q2[j + 1], p, q);
    return res;
}

__device__ __forceinline__ void load_quad(LP q, const float *src) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { P2 v; v.x = src[2 * k]; v.y = src[2 * k + 1]; q[k] = v; }
}

// quad `src` (8 floats) into q (5 slots), oriented for quad_intersection; returns its shoelace area, taken before the
// re-orientation as the reference does (voxelutil.cpp:99-103) -- but its magnitude: the reference keeps the sign, which turns
// the union of a clockwise quad negative (IoU -1 for a box against itself).  Counter-clockwise input, all the reference's own
// callers produce, is unaffected bit for bit.
__device__ __forceinline__ float load_oriented(LP q, const float *src) {
    load_quad(q, src);
    const float area = fabsf(shoelace(q, 4));
    orient_ccw(q);
    return area;
}

// the four polygon areas of this thread inside a [POLY_SLOTS][threads] LDS block
struct Polys { LP p, q, q1, q2; };
__device__ __forceinline__ Polys polys_of(P2 *block, int threads, int t) {
    Polys r;
    r.p = LP{block + t, threads};
    r.q = LP{block + 10 * threads + t, threads};
    r.q1 = LP{block + 30 * threads + t, threads};
    r.q2 = LP{block + 35 * threads + t, threads};
    return r;
}

// IoU of the quads qa, qb (8 floats each) as bboxOverlap computes it
__device__ __forceinline__ float quad_iou(const Polys &w, const float *qa, const float *qb) {
    const float a1 = load_oriented(w.q1, qa), a2 = load_oriented(w.q2, qb);
    const float inter = quad_intersection(w.q1, w.q2, w.p, w.q);
    return inter / (a1 + a2 - inter);
}

// Order-preserving map of a float to an unsigned key (larger float -> larger key); -0 counts as +0 so equal logits tie
// (the sort keys of detect_select, tta_merge and tta_fuse).
__device__ __forceinline__ unsigned order_key(float x) {
    const unsigned u = x == 0.f ? 0u : __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// BEV quad of a box b = xyzlwhr (Calc.bbox3d2bev), as detect_select and tta_merge form it
__device__ __forceinline__ void box_quad(const float *b, P2 *q) {
    // unit-square corners scaled by (l, w), times [[cos, -sin], [sin, cos]] from the right, shifted by (x, y)
    const float cs = cosf(b[6]), sn = sinf(b[6]);
    const float ux[4] = {0.5f, -0.5f, -0.5f, 0.5f}, uy[4] = {0.5f, 0.5f, -0.5f, -0.5f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float px = ux[k] * b[3], py = uy[k] * b[4];
        q[k].x = (px * cs + py * sn) + b[0];
        q[k].y = (px * -sn + py * cs) + b[1];
    }
}

// Bounding circle of a quad (q[0..4) as P2): centre = mean of the corners, radius = largest corner distance from it
template <class Quad>
__device__ __forceinline__ void quad_circle(const Quad &q, P2 &c, float &r) {
    c = {0.f, 0.f};
    r = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const P2 v = q[k]; c.x += 0.25f * v.x; c.y += 0.25f * v.y; }
#pragma unroll
    for (int k = 0; k < 4; ++k) { const P2 v = q[k]; r = fmaxf(r, sqrtf((v.x - c.x) * (v.x - c.x) + (v.y - c.y) * (v.y - c.y))); }
}

// ... as a table row [cx, cy, r] from the quad's 8 floats
__device__ __forceinline__ void circle_of(const float *quad8, float *circ3) {
    P2 c;
    float r;
    quad_circle((const P2 *)quad8, c, r);
    circ3[0] = c.x; circ3[1] = c.y; circ3[2] = r;
}

// Boxes whose centres are further apart than the two radii (+ 1 %) cannot touch: their true IoU is 0 and the origin-fan sum
// gives rounding noise of ~1e-6 there, so callers that compare the IoU with a threshold well above that skip the clipping.
__device__ __forceinline__ bool circles_apart(P2 c1, float r1, P2 c2, float r2) {
    const float dist = sqrtf((c2.x - c1.x) * (c2.x - c1.x) + (c2.y - c1.y) * (c2.y - c1.y));
    return dist > 1.01f * (r1 + r2) + 1e-3f;
}

}  // namespace
