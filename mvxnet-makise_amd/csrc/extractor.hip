// Glue kernels of the frozen ResNet50-FPN image extractor (modules/imhead/Extractor.py; the reference runs torchvision's
// fasterrcnn_resnet50_fpn_v2 trunk, modules/imhead/Pipe.py:8-21).  The arithmetic of the network runs on the matrix-core kernels
// that exist: 1x1 convolutions are row GEMMs (linear.hip / linear_split.hip), 3x3 convolutions the gather kernels of conv3d.hip /
// conv3d_split.hip (stride 2 through the space-to-depth image, rpn.hip).  What a frozen CNN needs besides is here, forward only,
// on channels-last frame sets [F][h][w][c] f32, every output element written by exactly one thread (no atomics):
//
//   image_prepare     GeneralizedRCNNTransform in eval mode in one launch: u8 HWC / 255 or f32 CHW -> (x - mean) / std ->
//                     bilinear resize (align_corners = False, coordinate scale = in / out) -> zero padding to the padded size.
//                     Output [F][ph][pw][4]: three channels and a zero, so that every pixel is one 16-byte access.
//   stem_conv7        7x7 stride 2 padding 3, 3 -> 64, folded BatchNorm bias, ReLU (f32 FMAs: 147 products per output, 1.7 % of the
//                     network's work, too narrow for the matrix cores)
//   maxpool3s2        3x3 stride 2 padding 1
//   add_relu          the bottleneck's skip: out = ReLU(a + b)
//   gather_stride2    rows of the even (y, x) sites: the input of the 1x1 stride-2 downsample branches
//   topdown_merge     lateral + nearest_upsample(top), top exactly half the size
#include "common.h"

namespace {

__constant__ float c_mean[3] = {0.485f, 0.456f, 0.406f};      // torchvision's image_mean / image_std (ImageNet)
__constant__ float c_std[3] = {0.229f, 0.224f, 0.225f};

struct Px { float v[3]; };

template <bool U8>
__device__ __forceinline__ Px load_px(const void *img, int f, int y, int x, int H, int W) {
    Px p;
    if (U8) {
        const uint8_t *s = (const uint8_t *)img + (((size_t)f * H + y) * W + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) p.v[c] = ((float)s[c] / 255.0f - c_mean[c]) / c_std[c];
    } else {
        const float *s = (const float *)img + ((size_t)f * 3 * H + y) * W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) p.v[c] = (s[(size_t)c * H * W] - c_mean[c]) / c_std[c];
    }
    return p;
}

// source index of torch's upsample_bilinear2d (align_corners = False): scale * (dst + 0.5) - 0.5, clamped at 0
__device__ __forceinline__ void src_index(float scale, int dst, int n, int &i0, int &i1, float &l1) {
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    if (s < 0.f) s = 0.f;
    i0 = min((int)s, n - 1);
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
    l1 = s - (float)i0;
}

template <bool U8>
__global__ void image_prepare(const void *__restrict__ img, float *__restrict__ out, int F, int H, int W, int oh, int ow, int ph,
                              int pw, float sy, float sx) {
    const size_t total = (size_t)F * ph * pw;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(e % pw);
        const int y = (int)((e / pw) % ph);
        const int f = (int)(e / ((size_t)pw * ph));
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);          // the padding is zero AFTER the normalisation
        if (y < oh && x < ow) {
            int y0, y1, x0, x1;
            float ly, lx;
            src_index(sy, y, H, y0, y1, ly);
            src_index(sx, x, W, x0, x1, lx);
            const Px a = load_px<U8>(img, f, y0, x0, H, W), b = load_px<U8>(img, f, y0, x1, H, W);
            const Px c = load_px<U8>(img, f, y1, x0, H, W), d = load_px<U8>(img, f, y1, x1, H, W);
            const float hy = 1.f - ly, hx = 1.f - lx;
            float r[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) r[k] = hy * (hx * a.v[k] + lx * b.v[k]) + ly * (hx * c.v[k] + lx * d.v[k]);
            o = make_float4(r[0], r[1], r[2], 0.f);
        }
        ((float4 *)out)[e] = o;
    }
}

// ---- stem: 7x7 / stride 2 / padding 3, 3 -> 64 channels, + bias, ReLU ---------------------------------------------------
// A workgroup computes ST_TH x ST_TW output sites x 64 channels from an LDS copy of its input patch and of the whole kernel
// ([ky][kx][ci][co]: 37.6 KB).  A thread owns 4 channels (one 16-byte weight read per input channel and tap) and strips of 4
// sites along x: the 16 lanes of a channel group read consecutive weights, the 4 strips of a wave different pixels.
constexpr int ST_TH = 8, ST_TW = 32;
constexpr int ST_IH = 2 * ST_TH + 5, ST_IW = 2 * ST_TW + 5;
constexpr int ST_WN = 49 * 3 * 64;

__global__ __launch_bounds__(256) void stem_conv7(const float *__restrict__ in, const float *__restrict__ wpk,
                                                  const float *__restrict__ bias, float *__restrict__ out, int ph, int pw, int ch,
                                                  int cw) {
    __shared__ float4 s_in[ST_IH * ST_IW];
    __shared__ __attribute__((aligned(16))) float s_w[ST_WN];
    const int tid = threadIdx.x;
    const int f = blockIdx.z, oy0 = blockIdx.y * ST_TH, ox0 = blockIdx.x * ST_TW;
    for (int i = tid; i < ST_WN / 4; i += 256) ((float4 *)s_w)[i] = ((const float4 *)wpk)[i];
    for (int i = tid; i < ST_IH * ST_IW; i += 256) {
        const int r = i / ST_IW, c = i - r * ST_IW;
        const int iy = 2 * oy0 - 3 + r, ix = 2 * ox0 - 3 + c;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (iy >= 0 && iy < ph && ix >= 0 && ix < pw) v = ((const float4 *)in)[((size_t)f * ph + iy) * pw + ix];
        s_in[i] = v;
    }
    __syncthreads();
    const int cg = tid & 15, st = tid >> 4;
    const float4 b4 = *(const float4 *)(bias + cg * 4);
#pragma unroll 1
    for (int it = 0; it < ST_TH * ST_TW / 4 / 16; ++it) {
        const int strip = st + 16 * it;
        const int row = strip / (ST_TW / 4), xs = (strip - row * (ST_TW / 4)) * 4;
        float4 acc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = b4;
#pragma unroll 1
        for (int ky = 0; ky < 7; ++ky) {
            const float4 *rp = s_in + (2 * row + ky) * ST_IW + 2 * xs;
            float4 px[13];
#pragma unroll
            for (int j = 0; j < 13; ++j) px[j] = rp[j];
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const float *wp = s_w + (ky * 7 + kx) * 3 * 64 + cg * 4;
                const float4 w0 = *(const float4 *)wp, w1 = *(const float4 *)(wp + 64), w2 = *(const float4 *)(wp + 128);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float4 p = px[2 * s + kx];
                    acc[s].x = fmaf(p.z, w2.x, fmaf(p.y, w1.x, fmaf(p.x, w0.x, acc[s].x)));
                    acc[s].y = fmaf(p.z, w2.y, fmaf(p.y, w1.y, fmaf(p.x, w0.y, acc[s].y)));
                    acc[s].z = fmaf(p.z, w2.z, fmaf(p.y, w1.z, fmaf(p.x, w0.z, acc[s].z)));
                    acc[s].w = fmaf(p.z, w2.w, fmaf(p.y, w1.w, fmaf(p.x, w0.w, acc[s].w)));
                }
            }
        }
        const int oy = oy0 + row;
        if (oy >= ch) continue;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int ox = ox0 + xs + s;
            if (ox >= cw) continue;
            float4 v = acc[s];
            v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
            *(float4 *)(out + (((size_t)f * ch + oy) * cw + ox) * 64 + cg * 4) = v;
        }
    }
}

__global__ void maxpool3s2(const float *__restrict__ in, float *__restrict__ out, int F, int h, int w, int oh, int ow, int c4) {
    const size_t total = (size_t)F * oh * ow * c4;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        size_t r = e;
        const int c = (int)(r % c4); r /= c4;
        const int x = (int)(r % ow); r /= ow;
        const int y = (int)(r % oh);
        const int f = (int)(r / oh);
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int iy = 2 * y - 1 + dy;
            if (iy < 0 || iy >= h) continue;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int ix = 2 * x - 1 + dx;
                if (ix < 0 || ix >= w) continue;
                const float4 v = ((const float4 *)in)[(((size_t)f * h + iy) * w + ix) * c4 + c];
                m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
            }
        }
        ((float4 *)out)[e] = m;
    }
}

__global__ void add_relu(const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ out, size_t n4) {
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n4; e += (size_t)gridDim.x * blockDim.x) {
        const float4 u = ((const float4 *)a)[e], v = ((const float4 *)b)[e];
        ((float4 *)out)[e] = make_float4(fmaxf(u.x + v.x, 0.f), fmaxf(u.y + v.y, 0.f), fmaxf(u.z + v.z, 0.f), fmaxf(u.w + v.w, 0.f));
    }
}

// out [F][oh][ow][c] = in [F][h][w][c] at (2y, 2x)
__global__ void gather_stride2(const float *__restrict__ in, float *__restrict__ out, int F, int h, int w, int oh, int ow, int c4) {
    const size_t total = (size_t)F * oh * ow * c4;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        size_t r = e;
        const int c = (int)(r % c4); r /= c4;
        const int x = (int)(r % ow); r /= ow;
        const int y = (int)(r % oh);
        const int f = (int)(r / oh);
        ((float4 *)out)[e] = ((const float4 *)in)[(((size_t)f * h + 2 * y) * w + 2 * x) * c4 + c];
    }
}

// out [F][2h][2w][c] = lateral + top [F][h][w][c] at (y / 2, x / 2)
__global__ void topdown_merge(const float *__restrict__ lat, const float *__restrict__ top, float *__restrict__ out, int F, int h,
                              int w, int c4) {
    const int H = 2 * h, W = 2 * w;
    const size_t total = (size_t)F * H * W * c4;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        size_t r = e;
        const int c = (int)(r % c4); r /= c4;
        const int x = (int)(r % W); r /= W;
        const int y = (int)(r % H);
        const int f = (int)(r / H);
        const float4 u = ((const float4 *)lat)[e];
        const float4 v = ((const float4 *)top)[(((size_t)f * h + (y >> 1)) * w + (x >> 1)) * c4 + c];
        ((float4 *)out)[e] = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
    }
}

inline unsigned ew_grid(size_t n) { return (unsigned)(mvx_cdiv(n, 256) > 8192 ? 8192 : mvx_cdiv(n, 256)); }

}  // namespace

extern "C" int mvx_image_prepare_frames(const void *img, int32_t is_u8, float *out, int32_t n_frames, int32_t h, int32_t w,
                                        int32_t oh, int32_t ow, int32_t ph, int32_t pw, void *stream) {
    MVX_CHECK_ARG(img && out && n_frames >= 1 && h > 0 && w > 0 && oh > 0 && ow > 0 && ph >= oh && pw >= ow);
    const size_t total = (size_t)n_frames * ph * pw;
    const float sy = (float)h / (float)oh, sx = (float)w / (float)ow;      // recompute_scale_factor: the scale follows from the sizes
    if (is_u8)
        hipLaunchKernelGGL(image_prepare<true>, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, img, out, n_frames, h, w, oh,
                           ow, ph, pw, sy, sx);
    else
        hipLaunchKernelGGL(image_prepare<false>, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, img, out, n_frames, h, w, oh,
                           ow, ph, pw, sy, sx);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_stem_conv7_frames(const float *in, const float *wpk, const float *bias, float *out, int32_t n_frames, int32_t ph,
                                     int32_t pw, void *stream) {
    MVX_CHECK_ARG(in && wpk && bias && out && n_frames >= 1 && n_frames <= 65535 && ph > 0 && pw > 0);
    const int ch = (ph - 1) / 2 + 1, cw = (pw - 1) / 2 + 1;
    hipLaunchKernelGGL(stem_conv7, dim3(mvx_cdiv(cw, ST_TW), mvx_cdiv(ch, ST_TH), n_frames), dim3(256), 0, (hipStream_t)stream, in,
                       wpk, bias, out, ph, pw, ch, cw);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_maxpool3s2_frames(const float *in, float *out, int32_t n_frames, int32_t h, int32_t w, int32_t channels,
                                     void *stream) {
    MVX_CHECK_ARG(in && out && n_frames >= 1 && h > 0 && w > 0 && channels > 0 && channels % 4 == 0);
    const int oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1;
    hipLaunchKernelGGL(maxpool3s2, dim3(ew_grid((size_t)n_frames * oh * ow * (channels / 4))), dim3(256), 0, (hipStream_t)stream, in,
                       out, n_frames, h, w, oh, ow, channels / 4);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_add_relu_frames(const float *a, const float *b, float *out, int64_t n, void *stream) {
    MVX_CHECK_ARG(a && b && out && n >= 0 && n % 4 == 0);
    if (n == 0) return MVX_OK;
    hipLaunchKernelGGL(add_relu, dim3(ew_grid((size_t)n / 4)), dim3(256), 0, (hipStream_t)stream, a, b, out, (size_t)n / 4);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_gather_stride2_frames(const float *in, float *out, int32_t n_frames, int32_t h, int32_t w, int32_t channels,
                                         void *stream) {
    MVX_CHECK_ARG(in && out && n_frames >= 1 && h > 0 && w > 0 && channels > 0 && channels % 4 == 0);
    const int oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1;
    hipLaunchKernelGGL(gather_stride2, dim3(ew_grid((size_t)n_frames * oh * ow * (channels / 4))), dim3(256), 0, (hipStream_t)stream,
                       in, out, n_frames, h, w, oh, ow, channels / 4);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

extern "C" int mvx_topdown_merge_frames(const float *lateral, const float *top, float *out, int32_t n_frames, int32_t lat_h,
                                        int32_t lat_w, int32_t top_h, int32_t top_w, int32_t channels, void *stream) {
    MVX_CHECK_ARG(lateral && top && out && n_frames >= 1 && top_h > 0 && top_w > 0 && channels > 0 && channels % 4 == 0);
    MVX_CHECK_ARG(lat_h == 2 * top_h && lat_w == 2 * top_w);          // padded to 32: every level is exactly twice the next
    hipLaunchKernelGGL(topdown_merge, dim3(ew_grid((size_t)n_frames * lat_h * lat_w * (channels / 4))), dim3(256), 0,
                       (hipStream_t)stream, lateral, top, out, n_frames, top_h, top_w, channels / 4);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}
