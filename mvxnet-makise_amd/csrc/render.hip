// Frame rendering for the frames of a step: a bird's-eye view and a camera view of the resident point clouds with a list of
// coloured boxes drawn over them.  Every pixel is decided by integer arithmetic on values that f64 geometry produced, and
// the planes the kernels meet on are u32 words in global memory combined by integer atomicMax / atomicMin / atomicAdd: the
// images are bitwise reproducible and do not depend on the order of points, boxes or launches.
//
//   1. bev_splat / cam_points (grid (block of 256 points, frame), one thread per point): the point's pixel; BEV keeps the
//                   largest (height, intensity) key and a count per pixel, the camera view the smallest depth per pixel.
//   2. draw_boxes   (a wave per (frame, box slot), four waves per block): lane s computes segment s of the box -- BEV: the four
//                   edges and the heading marker; camera: the twelve edges and the diagonals of the front face, transformed
//                   and clipped against w >= z_near -- then the wave walks the segments, its lanes striding over the pixels
//                   of one segment (closed form per pixel, the range of k that is inside the image computed up front).
//   3. shade_pixels (four consecutive pixels of the whole frame set per thread): planes (and the camera image) -> u8 RGB.
// The kernels know colours, not classes: colors[f][b] = prio << 24 | R << 16 | G << 8 | B and the larger word wins a pixel.
#include "common.h"

namespace {

constexpr int PT_THREADS = 256, PX_THREADS = 256, BOX_WAVES = 4;
constexpr double COORD_LIMIT = 16777216.0;          // 2^24: pixel coordinates of a drawn segment stay below it

// floor(v) clamped into 0..hi; a NaN gives 0
__device__ __forceinline__ unsigned clampq(double v, unsigned hi) {
    if (!(v > 0.0)) return 0u;
    if (v >= (double)hi) return hi;
    return (unsigned)floor(v);
}

__device__ __forceinline__ bool finite3(double a, double b, double c) { return isfinite(a) && isfinite(b) && isfinite(c); }

__device__ __forceinline__ int clamp_count(int n, int cap) { return min(max(n, 0), cap); }

struct PointArgs {
    const float *pts;            // [F][cap][ld]
    const int *n_points;         // [F]
    int cap, ld, H, W;
    double x0, y0, res, z0, zspan;          // BEV
    double depth_max;                       // camera
    int radius;
    unsigned *plane_a, *plane_b;            // BEV: key, count; camera: depth
};

// 1. -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PT_THREADS) void bev_splat(PointArgs a) {
    const int f = blockIdx.y, p = blockIdx.x * PT_THREADS + threadIdx.x;
    if (p >= clamp_count(a.n_points[f], a.cap)) return;
    const float *q = a.pts + ((size_t)f * a.cap + p) * a.ld;
    const double x = (double)q[0], y = (double)q[1], z = (double)q[2], r = (double)q[3];
    if (!finite3(x, y, z)) return;
    const double di = floor((x - a.x0) / a.res), dj = floor((y - a.y0) / a.res);
    if (!(di >= 0.0 && di < (double)a.H && dj >= 0.0 && dj < (double)a.W)) return;
    const int row = a.H - 1 - (int)di, col = a.W - 1 - (int)dj;
    const unsigned zq = clampq((z - a.z0) / a.zspan * 65535.0, 65535u), iq = clampq(r * 255.0, 255u);
    const size_t at = ((size_t)f * a.H + row) * a.W + col;
    atomicMax(a.plane_a + at, ((zq << 8) | iq) + 1u);
    atomicAdd(a.plane_b + at, 1u);
}

__global__ __launch_bounds__(PT_THREADS) void cam_points(PointArgs a) {
    const int f = blockIdx.y, p = blockIdx.x * PT_THREADS + threadIdx.x;
    if (p >= clamp_count(a.n_points[f], a.cap)) return;
    const float *q = a.pts + ((size_t)f * a.cap + p) * a.ld;
    const double x = (double)q[0], dr = floor((double)q[4]), dc = floor((double)q[5]);
    if (!finite3(x, dr, dc)) return;
    const int R = a.radius;
    if (!(dr >= (double)-R && dr < (double)(a.H + R) && dc >= (double)-R && dc < (double)(a.W + R))) return;
    const int row = (int)dr, col = (int)dc;
    const unsigned dq = clampq(x / a.depth_max * 65535.0, 65535u);
    unsigned *plane = a.plane_a + (size_t)f * a.H * a.W;
    for (int rr = max(row - R, 0); rr <= min(row + R, a.H - 1); ++rr)
        for (int cc = max(col - R, 0); cc <= min(col + R, a.W - 1); ++cc) atomicMin(plane + (size_t)rr * a.W + cc, dq);
}

// 2. -------------------------------------------------------------------------------------------------------------------
// The pixels of the segment (r0, c0) - (r1, c1) on `plane`, lanes striding over k.  The end with the smaller (major, minor)
// pair comes first, so both directions give the same pixels; pixel k = (m0 + k, q0 + sgn(dq) ((2 k |dq| + n) / (2 n))).
__device__ void draw_segment(unsigned *plane, int H, int W, int r0, int c0, int r1, int c1, int T, unsigned color, int lane) {
    const int adr = abs(r1 - r0), adc = abs(c1 - c0);
    const bool rows_major = adr >= adc;
    long long m0 = rows_major ? r0 : c0, q0 = rows_major ? c0 : r0, m1 = rows_major ? r1 : c1, q1 = rows_major ? c1 : r1;
    if (m1 < m0 || (m1 == m0 && q1 < q0)) {
        long long t = m0; m0 = m1; m1 = t;
        t = q0; q0 = q1; q1 = t;
    }
    const long long n = m1 - m0, dq = q1 - q0, adq = dq < 0 ? -dq : dq, sgn = dq < 0 ? -1 : 1;
    const int M = rows_major ? H : W, Q = rows_major ? W : H;
    const long long klo = m0 < 0 ? -m0 : 0, khi = min(n, (long long)M - 1 - m0);
    const int lo = -(T / 2), hi = T - 1 - (T / 2);
    for (long long k = klo + lane; k <= khi; k += MVX_WAVE) {
        const long long major = m0 + k, minor = n == 0 ? q0 : q0 + sgn * ((2 * k * adq + n) / (2 * n));
        if (minor < 0 || minor >= Q) continue;
        const int pr = (int)(rows_major ? major : minor), pc = (int)(rows_major ? minor : major);
        for (int rr = max(pr + lo, 0); rr <= min(pr + hi, H - 1); ++rr)
            for (int cc = max(pc + lo, 0); cc <= min(pc + hi, W - 1); ++cc) atomicMax(plane + (size_t)rr * W + cc, color);
    }
}

struct BoxArgs {
    const float *boxes;          // [F][B][7] x y z l w h r, z the bottom face
    const int *n_boxes;          // [F]
    const unsigned *colors;      // [F][B]
    int B, H, W, T;
    double x0, y0, res;          // BEV
    const double *mat;           // camera: [F][4][4] image_from_lidar
    double z_near;
    unsigned *overlay;           // [F][H][W]
    int *status;                 // [F]
};

struct Box7 { double x, y, z, l, w, h, c, s; };

// corner k (0..3) of Calc.bbox3d2bev: (+,+), (-,+), (-,-), (+,-) of (l, w) / 2, @ R(r) + centre
__device__ __forceinline__ void bev_corner(const Box7 &b, int k, double &X, double &Y) {
    const double px = ((k == 0 || k == 3) ? 0.5 : -0.5) * b.l, py = (k < 2 ? 0.5 : -0.5) * b.w;
    X = (px * b.c + py * b.s) + b.x;
    Y = (-px * b.s + py * b.c) + b.y;
}

struct Seg { int r0, c0, r1, c1; bool draw, bad; };

__device__ __forceinline__ bool pixel_ok(double r, double c) { return fabs(r) < COORD_LIMIT && fabs(c) < COORD_LIMIT; }      // a NaN fails

// BEV segment s: 0..3 the edges corner s - corner s + 1, 4 the heading marker centre - midpoint of the edge at u = +l/2
__device__ Seg bev_segment(const BoxArgs &a, const Box7 &b, int s) {
    double X[2], Y[2];
    if (s < 4) {
        bev_corner(b, s, X[0], Y[0]);
        bev_corner(b, (s + 1) & 3, X[1], Y[1]);
    } else {
        const double px = 0.5 * b.l;
        X[0] = b.x; Y[0] = b.y;
        X[1] = px * b.c + b.x;
        Y[1] = -px * b.s + b.y;
    }
    double r[2], c[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        r[e] = (double)(a.H - 1) - floor((X[e] - a.x0) / a.res);
        c[e] = (double)(a.W - 1) - floor((Y[e] - a.y0) / a.res);
    }
    Seg o;
    o.bad = !(pixel_ok(r[0], c[0]) && pixel_ok(r[1], c[1]));
    o.draw = !o.bad;
    o.r0 = o.bad ? 0 : (int)r[0]; o.c0 = o.bad ? 0 : (int)c[0];
    o.r1 = o.bad ? 0 : (int)r[1]; o.c1 = o.bad ? 0 : (int)c[1];
    return o;
}

// camera segment s of the corners of Calc.bbox3d2corner (0..3 top face, 4..7 bottom face, BEV corner k & 3): top edges,
// bottom edges, verticals, then the diagonals 0-7 and 3-4 of the face at u = +l/2; a nibble per segment
__device__ Seg cam_segment(const BoxArgs &a, const Box7 &b, const double *m, int s) {
    const int ca = (int)((0x30321076543210ull >> (4 * s)) & 15), cb = (int)((0x47765447650321ull >> (4 * s)) & 15);
    double u[2], v[2], w[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int k = e ? cb : ca;
        double X, Y;
        bev_corner(b, k & 3, X, Y);
        const double Z = k < 4 ? b.z + b.h : b.z;
        u[e] = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3];
        v[e] = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7];
        w[e] = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11];
    }
    Seg o = {0, 0, 0, 0, false, false};
    const bool behind0 = w[0] < a.z_near, behind1 = w[1] < a.z_near;
    if (behind0 && behind1) return o;
    if (behind0 != behind1) {
        const int e = behind0 ? 0 : 1, g = 1 - e;           // end e moves to the plane along the segment
        const double t = (a.z_near - w[e]) / (w[g] - w[e]);
        u[e] = u[e] + t * (u[g] - u[e]);
        v[e] = v[e] + t * (v[g] - v[e]);
        w[e] = a.z_near;
    }
    const double r0 = floor(v[0] / w[0]), c0 = floor(u[0] / w[0]), r1 = floor(v[1] / w[1]), c1 = floor(u[1] / w[1]);
    o.bad = !(pixel_ok(r0, c0) && pixel_ok(r1, c1));
    o.draw = !o.bad;
    if (o.draw) { o.r0 = (int)r0; o.c0 = (int)c0; o.r1 = (int)r1; o.c1 = (int)c1; }
    return o;
}

template <bool CAMERA>
__global__ __launch_bounds__(BOX_WAVES * MVX_WAVE) void draw_boxes(BoxArgs a) {
    constexpr int NSEG = CAMERA ? 14 : 5;
    const int f = blockIdx.y, lane = threadIdx.x & 63, bi = blockIdx.x * BOX_WAVES + (threadIdx.x >> 6);
    if (bi >= clamp_count(a.n_boxes[f], a.B)) return;                  // wave-uniform
    const unsigned color = a.colors[(size_t)f * a.B + bi];
    if (color == 0u) return;                                           // 0 = nothing drawn
    const float *g = a.boxes + ((size_t)f * a.B + bi) * 7;
    Box7 b;
    b.x = (double)g[0]; b.y = (double)g[1]; b.z = (double)g[2]; b.l = (double)g[3]; b.w = (double)g[4]; b.h = (double)g[5];
    const double yaw = (double)g[6];
    bool bad = !(finite3(b.x, b.y, b.z) && finite3(b.l, b.w, b.h) && isfinite(yaw));
    Seg sg = {0, 0, 0, 0, false, false};
    if (!bad && lane < NSEG) {
        b.c = cos(yaw); b.s = sin(yaw);
        sg = CAMERA ? cam_segment(a, b, a.mat + (size_t)f * 16, lane) : bev_segment(a, b, lane);
        bad = sg.bad;
    }
    if (__ballot(bad) != 0ull) {                                       // one bad end drops the whole box
        if (lane == 0) atomicOr(a.status + f, MVX_RENDER_BAD_BOX);
        return;
    }
    unsigned *plane = a.overlay + (size_t)f * a.H * a.W;
#pragma unroll 1
    for (int s = 0; s < NSEG; ++s) {
        const int r0 = __shfl(sg.r0, s, 64), c0 = __shfl(sg.c0, s, 64), r1 = __shfl(sg.r1, s, 64), c1 = __shfl(sg.c1, s, 64);
        if (__shfl((int)sg.draw, s, 64)) draw_segment(plane, a.H, a.W, r0, c0, r1, c1, a.T, color, lane);
    }
}

// 3. -------------------------------------------------------------------------------------------------------------------
struct PixelArgs {
    const unsigned *plane_a, *plane_b, *overlay;      // BEV: key, count; camera: depth, -
    const unsigned char *lut;                         // [256][3]
    const unsigned char *image;                       // camera: [F][H][W][3] or NULL
    int by_intensity, bgr;
    unsigned cmax, background;
    size_t n_px;                                      // F * H * W
    unsigned char *out;                               // [F][H][W][3]
};

struct Rgb { unsigned r, g, b; };

__device__ __forceinline__ Rgb rgb_of_word(unsigned w) { return {(w >> 16) & 255u, (w >> 8) & 255u, w & 255u}; }

__device__ __forceinline__ Rgb bev_pixel(const PixelArgs &a, unsigned key, unsigned cnt, unsigned ov) {
    if (ov) return rgb_of_word(ov);
    if (!key) return rgb_of_word(a.background);
    const unsigned kq = key - 1u, idx = a.by_intensity ? (kq & 255u) : (kq >> 16);
    const unsigned shade = 64u + (unsigned)((191ull * min(cnt, a.cmax)) / a.cmax);
    const unsigned char *l = a.lut + 3 * idx;
    return {l[0] * shade / 255u, l[1] * shade / 255u, l[2] * shade / 255u};
}

__device__ __forceinline__ Rgb cam_pixel(const PixelArgs &a, unsigned depth, unsigned ov, Rgb under) {
    if (ov) return rgb_of_word(ov);
    if (depth == 0xFFFFFFFFu) return a.bgr ? Rgb{under.b, under.g, under.r} : under;
    const unsigned char *l = a.lut + 3 * (depth >> 8);
    return {l[0], l[1], l[2]};
}

// four pixels of the whole frame set per thread: 16-byte plane reads, 12 bytes of image in three aligned words
template <bool CAMERA>
__global__ __launch_bounds__(PX_THREADS) void shade_pixels(PixelArgs a) {
    const size_t p = ((size_t)blockIdx.x * PX_THREADS + threadIdx.x) * 4;
    if (p >= a.n_px) return;
    if (p + 4 <= a.n_px) {
        const uint4 va = *(const uint4 *)(a.plane_a + p), vo = *(const uint4 *)(a.overlay + p);
        uint4 vb = make_uint4(0u, 0u, 0u, 0u);
        if (!CAMERA) vb = *(const uint4 *)(a.plane_b + p);
        unsigned in[3] = {0u, 0u, 0u};
        if (CAMERA && a.image) {
            const uint3 t = *(const uint3 *)(a.image + 3 * p);
            in[0] = t.x; in[1] = t.y; in[2] = t.z;
        }
        const unsigned ka[4] = {va.x, va.y, va.z, va.w}, kb[4] = {vb.x, vb.y, vb.z, vb.w}, ko[4] = {vo.x, vo.y, vo.z, vo.w};
        unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            Rgb px;
            if (CAMERA) {
                Rgb under;
                under.r = (in[(3 * i) >> 2] >> (8 * ((3 * i) & 3))) & 255u;
                under.g = (in[(3 * i + 1) >> 2] >> (8 * ((3 * i + 1) & 3))) & 255u;
                under.b = (in[(3 * i + 2) >> 2] >> (8 * ((3 * i + 2) & 3))) & 255u;
                px = cam_pixel(a, ka[i], ko[i], under);
            } else {
                px = bev_pixel(a, ka[i], kb[i], ko[i]);
            }
            o[(3 * i) >> 2] |= px.r << (8 * ((3 * i) & 3));
            o[(3 * i + 1) >> 2] |= px.g << (8 * ((3 * i + 1) & 3));
            o[(3 * i + 2) >> 2] |= px.b << (8 * ((3 * i + 2) & 3));
        }
        *(uint3 *)(a.out + 3 * p) = make_uint3(o[0], o[1], o[2]);
        return;
    }
    for (size_t q = p; q < a.n_px; ++q) {                              // the last one to three pixels of the set
        Rgb px;
        if (CAMERA) {
            Rgb under = {0u, 0u, 0u};
            if (a.image) under = {a.image[3 * q], a.image[3 * q + 1], a.image[3 * q + 2]};
            px = cam_pixel(a, a.plane_a[q], a.overlay[q], under);
        } else {
            px = bev_pixel(a, a.plane_a[q], a.plane_b[q], a.overlay[q]);
        }
        a.out[3 * q] = (unsigned char)px.r; a.out[3 * q + 1] = (unsigned char)px.g; a.out[3 * q + 2] = (unsigned char)px.b;
    }
}

// one u32 plane of the frame set, in bytes, a multiple of 16
inline size_t plane_bytes(int F, int H, int W) { return ((size_t)F * H * W * sizeof(unsigned) + 15) & ~(size_t)15; }

inline bool common_ok(const void *points6, int ld, const void *n_points, int F, int cap_points, const void *boxes, const void *n_boxes,
                      const void *colors, int cap_boxes, int H, int W, const void *lut, int T, const void *out, const void *status,
                      const void *ws, size_t ws_bytes) {
    if (!(F >= 1 && F <= MVX_MAX_FRAMES && H >= 1 && H <= MVX_RENDER_MAX_SIDE && W >= 1 && W <= MVX_RENDER_MAX_SIDE)) return false;
    if (!(points6 && n_points && lut && out && status && ws && ld >= 6 && cap_points >= 1 && cap_points < (1 << 26))) return false;
    if (!(cap_boxes >= 0 && cap_boxes <= (1 << 16)) || (cap_boxes > 0 && !(boxes && n_boxes && colors))) return false;
    if (!(T >= 1 && T <= 3)) return false;
    if (((uintptr_t)out & 3) != 0 || ((uintptr_t)ws & 15) != 0) return false;
    return ws_bytes >= mvx_render_workspace_bytes(F, H, W);
}

}  // namespace

extern "C" size_t mvx_render_workspace_bytes(int32_t n_frames, int32_t h, int32_t w) {
    if (n_frames < 1 || n_frames > MVX_MAX_FRAMES || h < 1 || h > MVX_RENDER_MAX_SIDE || w < 1 || w > MVX_RENDER_MAX_SIDE) return 0;
    return (3 * plane_bytes(n_frames, h, w) + 255) & ~(size_t)255;
}

extern "C" int mvx_render_bev_frames(const float *points6, int32_t ld, const int32_t *n_points, int32_t n_frames, int32_t cap_points,
                                     const float *boxes, const int32_t *n_boxes, const uint32_t *colors, int32_t cap_boxes, double x0,
                                     double y0, double res, double z0, double z1, int32_t h, int32_t w, const uint8_t *lut,
                                     int32_t color_by, int32_t cmax, uint32_t background, int32_t thickness, uint8_t *out,
                                     int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
    MVX_CHECK_ARG(common_ok(points6, ld, n_points, n_frames, cap_points, boxes, n_boxes, colors, cap_boxes, h, w, lut, thickness, out,
                            status, workspace, workspace_bytes));
    MVX_CHECK_ARG(res > 0.0 && z1 > z0 && cmax >= 1 && (color_by == MVX_RENDER_BY_HEIGHT || color_by == MVX_RENDER_BY_INTENSITY));
    MVX_CHECK_ARG(std::isfinite(x0) && std::isfinite(y0) && std::isfinite(res) && std::isfinite(z1 - z0));
    hipStream_t st = (hipStream_t)stream;
    const size_t pb = plane_bytes(n_frames, h, w);
    unsigned *key = (unsigned *)workspace, *cnt = (unsigned *)((char *)workspace + pb), *ov = (unsigned *)((char *)workspace + 2 * pb);
    hipError_t e = hipMemsetAsync(workspace, 0, 3 * pb, st);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, (size_t)n_frames * sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    PointArgs pa = {points6, n_points, cap_points, ld, h, w, x0, y0, res, z0, z1 - z0, 1.0, 0, key, cnt};
    hipLaunchKernelGGL(bev_splat, dim3(mvx_cdiv(cap_points, PT_THREADS), n_frames), dim3(PT_THREADS), 0, st, pa);
    MVX_LAUNCH_CHECK();
    if (cap_boxes > 0) {
        BoxArgs ba = {boxes, n_boxes, colors, cap_boxes, h, w, thickness, x0, y0, res, nullptr, 0.0, ov, status};
        hipLaunchKernelGGL(draw_boxes<false>, dim3(mvx_cdiv(cap_boxes, BOX_WAVES), n_frames), dim3(BOX_WAVES * MVX_WAVE), 0, st, ba);
        MVX_LAUNCH_CHECK();
    }
    PixelArgs xa = {key, cnt, ov, lut, nullptr, color_by == MVX_RENDER_BY_INTENSITY, 0, (unsigned)cmax, background,
                    (size_t)n_frames * h * w, out};
    hipLaunchKernelGGL(shade_pixels<false>, dim3(mvx_cdiv(mvx_cdiv(xa.n_px, 4), PX_THREADS)), dim3(PX_THREADS), 0, st, xa);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_render_camera_frames(const float *points6, int32_t ld, const int32_t *n_points, int32_t n_frames,
                                        int32_t cap_points, const float *boxes, const int32_t *n_boxes, const uint32_t *colors,
                                        int32_t cap_boxes, const double *image_from_lidar, double z_near, double depth_max, int32_t h,
                                        int32_t w, const uint8_t *lut_depth, int32_t point_radius, const uint8_t *image_or_null,
                                        int32_t image_is_bgr, int32_t thickness, uint8_t *out, int32_t *status, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    MVX_CHECK_ARG(common_ok(points6, ld, n_points, n_frames, cap_points, boxes, n_boxes, colors, cap_boxes, h, w, lut_depth, thickness,
                            out, status, workspace, workspace_bytes));
    MVX_CHECK_ARG(image_from_lidar && point_radius >= 0 && point_radius <= 2 && ((uintptr_t)image_or_null & 3) == 0);
    MVX_CHECK_ARG(z_near > 0.0 && depth_max > 0.0 && std::isfinite(z_near) && std::isfinite(depth_max));
    hipStream_t st = (hipStream_t)stream;
    const size_t pb = plane_bytes(n_frames, h, w);
    unsigned *depth = (unsigned *)workspace, *ov = (unsigned *)((char *)workspace + pb);
    hipError_t e = hipMemsetAsync(depth, 0xFF, pb, st);
    if (e == hipSuccess) e = hipMemsetAsync(ov, 0, pb, st);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, (size_t)n_frames * sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    PointArgs pa = {points6, n_points, cap_points, ld, h, w, 0.0, 0.0, 1.0, 0.0, 1.0, depth_max, point_radius, depth, nullptr};
    hipLaunchKernelGGL(cam_points, dim3(mvx_cdiv(cap_points, PT_THREADS), n_frames), dim3(PT_THREADS), 0, st, pa);
    MVX_LAUNCH_CHECK();
    if (cap_boxes > 0) {
        BoxArgs ba = {boxes, n_boxes, colors, cap_boxes, h, w, thickness, 0.0, 0.0, 1.0, image_from_lidar, z_near, ov, status};
        hipLaunchKernelGGL(draw_boxes<true>, dim3(mvx_cdiv(cap_boxes, BOX_WAVES), n_frames), dim3(BOX_WAVES * MVX_WAVE), 0, st, ba);
        MVX_LAUNCH_CHECK();
    }
    PixelArgs xa = {depth, nullptr, ov, lut_depth, image_or_null, 0, image_is_bgr != 0, 1u, 0u, (size_t)n_frames * h * w, out};
    hipLaunchKernelGGL(shade_pixels<true>, dim3(mvx_cdiv(mvx_cdiv(xa.n_px, 4), PX_THREADS)), dim3(PX_THREADS), 0, st, xa);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}
