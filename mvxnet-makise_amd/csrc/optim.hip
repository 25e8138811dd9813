// Fused AdamW over the flat gradient bucket (modules/parallel.py GradBucket): global gradient norm, clip coefficient, a guard
// against non-finite gradients and the update itself, in three launches with no host read and no float atomics (two runs
// from the same state are bitwise identical).
//
//   1. optim_norm_partial  (OPT_G workgroups of 256 threads, a constant grid): workgroup b owns the contiguous slice
//                          [b * per, (b + 1) * per) of the gradient, per = ceil(n / OPT_G) rounded up to 4 elements, and
//                          grid-strides inside it: scalar loads up to the first 16-byte boundary, 16-byte loads on the body,
//                          scalar loads on the tail.  Sum of g * g in f64 (the product of two f32 values is exact there), reduced
//                          over the wave (xor butterfly) and then over the four waves through LDS, both in a fixed order;
//                          partial[b] and nonfinite[b] (any inf or NaN in the slice).
//   2. optim_prepare       (one wave): the OPT_G partials in a fixed order -> norm, clip coefficient, skip decision; advances
//                          the state block and writes the control block that the update reads.
//   3. optim_adamw_update  (one workgroup per entry of the chunk table, <= 4096 elements of ONE parameter): returns at once when
//                          the control block says skip; otherwise torch's single-tensor AdamW in f32, 16-byte accesses when
//                          the chunk's parameter address and its addresses in the flat buffers are all 16-byte aligned, scalar
//                          accesses otherwise (the bucket packs parameters back to back: every parameter behind one whose
//                          element count is no multiple of 4 is misaligned in the flat buffers).
// The gradient is read only.
#include "common.h"
#include <math.h>

namespace {

constexpr int OPT_G = 1024;            // workgroups of the norm pass: a constant, so the summation order never depends on the data
constexpr int OPT_THREADS = 256;
constexpr int OPT_CHUNK = MVX_OPTIM_CHUNK;

// control block written by optim_prepare (f64 [8])
enum { CTL_SKIP = 0, CTL_GMUL = 1, CTL_DECAY = 2, CTL_STEP = 3, CTL_INV_BC2 = 4, CTL_EPS = 5 };
// state block kept by the caller (f64 [8])
enum { ST_T = 0, ST_SKIPPED = 1, ST_NORM = 2, ST_COEF = 3, ST_SKIP = 4 };

__device__ __forceinline__ int nonfinite_bits(float g) { return (__float_as_uint(g) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(OPT_THREADS) void optim_norm_partial(const float *__restrict__ g, long long n, long long per,
                                                                   double *__restrict__ partial, int *__restrict__ nonfinite) {
    __shared__ double s_sum[OPT_THREADS / 64];
    __shared__ int s_bad[OPT_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    long long lo = (long long)blockIdx.x * per, hi = lo + per;
    if (lo > n) lo = n;
    if (hi > n) hi = n;
    double acc = 0.0;
    int bad = 0;
    if (lo < hi) {
        // elements in front of the first 16-byte boundary of the slice
        long long head = (long long)(((16u - (unsigned)((uintptr_t)(g + lo) & 15u)) & 15u) >> 2);
        if (head > hi - lo) head = hi - lo;
        const long long body0 = lo + head, nvec = (hi - body0) >> 2, tail0 = body0 + (nvec << 2);
        if (tid < head) {
            const float x = g[lo + tid];
            acc += (double)x * (double)x;
            bad |= nonfinite_bits(x);
        }
        const float4 *gv = reinterpret_cast<const float4 *>(g + body0);
        for (long long i = tid; i < nvec; i += OPT_THREADS) {
            const float4 x = gv[i];
            acc += (double)x.x * (double)x.x;
            acc += (double)x.y * (double)x.y;
            acc += (double)x.z * (double)x.z;
            acc += (double)x.w * (double)x.w;
            bad |= nonfinite_bits(x.x) | nonfinite_bits(x.y) | nonfinite_bits(x.z) | nonfinite_bits(x.w);
        }
        if (tail0 + tid < hi) {
            const float x = g[tail0 + tid];
            acc += (double)x * (double)x;
            bad |= nonfinite_bits(x);
        }
    }
    acc = wave_sum_f64(acc);
    bad = __any(bad) ? 1 : 0;
    if (lane == 0) { s_sum[wid] = acc; s_bad[wid] = bad; }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        int b = 0;
#pragma unroll
        for (int w = 0; w < OPT_THREADS / 64; ++w) { s += s_sum[w]; b |= s_bad[w]; }
        partial[blockIdx.x] = s;
        nonfinite[blockIdx.x] = b;
    }
}

struct PrepArgs {
    const double *partial;
    const int *nonfinite;
    const float *count;          // device scalar: the number of frames that contributed to the summed gradient, or NULL
    double *state, *ctl;
    double lr, beta1, beta2, eps, weight_decay, max_norm;
    int guard;
};

__global__ __launch_bounds__(64) void optim_prepare(PrepArgs a) {
    const int lane = threadIdx.x;
    double s = 0.0;
    int bad = 0;
    for (int i = lane; i < OPT_G; i += 64) { s += a.partial[i]; bad |= a.nonfinite[i]; }
    s = wave_sum_f64(s);
    bad = __any(bad) ? 1 : 0;
    if (lane != 0) return;
    double gscale = 1.0;
    if (a.count) {
        const double c = (double)*a.count;
        gscale = 1.0 / (c > 1.0 ? c : 1.0);          // a NaN count divides by 1
    }
    const double norm = sqrt(s) * gscale;
    double coef = 1.0;
    if (a.max_norm > 0.0) {
        coef = a.max_norm / (norm + 1e-6);
        if (!(coef < 1.0)) coef = 1.0;
    }
    const bool finite = fabs(norm) <= 1.7976931348623157e308;
    const bool skip = a.guard && (bad || !finite);
    double t = a.state[ST_T];
    if (skip) a.state[ST_SKIPPED] += 1.0; else t += 1.0;
    a.state[ST_T] = t;
    a.state[ST_NORM] = norm;
    a.state[ST_COEF] = coef;
    a.state[ST_SKIP] = skip ? 1.0 : 0.0;
    const double tt = t > 1.0 ? t : 1.0;             // t = 0 only when the very first step is skipped: nothing reads the rest then
    a.ctl[CTL_SKIP] = skip ? 1.0 : 0.0;
    a.ctl[CTL_GMUL] = gscale * coef;
    a.ctl[CTL_DECAY] = 1.0 - a.lr * a.weight_decay;
    a.ctl[CTL_STEP] = a.lr / (1.0 - pow(a.beta1, tt));
    a.ctl[CTL_INV_BC2] = 1.0 / sqrt(1.0 - pow(a.beta2, tt));
    a.ctl[CTL_EPS] = a.eps;
}

struct Coef { float g_mul, decay, step, inv_bc2, eps, omb1, b2, omb2; };

// torch's single-tensor AdamW on one element (f32, no contraction): mul_(1 - lr wd), lerp_(g, 1 - b1), mul_(b2).addcmul_(g, g,
// 1 - b2), addcdiv_(m, sqrt(v) * inv_bc2 + eps, -step)
__device__ __forceinline__ void adamw_one(float &p, float g, float &m, float &v, const Coef &c) {
    g = g * c.g_mul;
    p = p * c.decay;
    m = m + (g - m) * c.omb1;
    v = v * c.b2 + (c.omb2 * g) * g;
    const float denom = sqrtf(v) * c.inv_bc2 + c.eps;
    p = p - c.step * (m / denom);
}

__global__ __launch_bounds__(OPT_THREADS) void optim_adamw_update(const long long *__restrict__ table, const float *__restrict__ grad,
                                                                   float *__restrict__ mom, float *__restrict__ var, long long n,
                                                                   const double *__restrict__ ctl, float omb1, float b2, float omb2) {
    if (ctl[CTL_SKIP] != 0.0) return;
    const long long *e = table + 3 * (long long)blockIdx.x;
    float *p = reinterpret_cast<float *>((uintptr_t)e[0]);
    const long long off = e[1], cnt = e[2];
    if (!p || off < 0 || cnt < 1 || cnt > OPT_CHUNK || off + cnt > n) return;       // a malformed entry touches nothing
    Coef c;
    c.g_mul = (float)ctl[CTL_GMUL]; c.decay = (float)ctl[CTL_DECAY]; c.step = (float)ctl[CTL_STEP];
    c.inv_bc2 = (float)ctl[CTL_INV_BC2]; c.eps = (float)ctl[CTL_EPS];
    c.omb1 = omb1; c.b2 = b2; c.omb2 = omb2;
    const float *g = grad + off;
    float *m = mom + off, *v = var + off;
    const int tid = threadIdx.x, count = (int)cnt;
    const bool aligned = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15u) == 0;
    if (aligned) {
        const int nvec = count >> 2;
        float4 *pv = reinterpret_cast<float4 *>(p), *mv = reinterpret_cast<float4 *>(m), *vv = reinterpret_cast<float4 *>(v);
        const float4 *gv = reinterpret_cast<const float4 *>(g);
        for (int i = tid; i < nvec; i += OPT_THREADS) {
            float4 P = pv[i], M = mv[i], V = vv[i];
            const float4 G = gv[i];
            adamw_one(P.x, G.x, M.x, V.x, c);
            adamw_one(P.y, G.y, M.y, V.y, c);
            adamw_one(P.z, G.z, M.z, V.z, c);
            adamw_one(P.w, G.w, M.w, V.w, c);
            pv[i] = P; mv[i] = M; vv[i] = V;
        }
        const int i = (nvec << 2) + tid;
        if (i < count) {
            float P = p[i], M = m[i], V = v[i];
            adamw_one(P, g[i], M, V, c);
            p[i] = P; m[i] = M; v[i] = V;
        }
    } else {
        for (int i = tid; i < count; i += OPT_THREADS) {
            float P = p[i], M = m[i], V = v[i];
            adamw_one(P, g[i], M, V, c);
            p[i] = P; m[i] = M; v[i] = V;
        }
    }
}

constexpr size_t WS_PARTIAL = 0, WS_FLAGS = OPT_G * sizeof(double), WS_CTL = WS_FLAGS + OPT_G * sizeof(int),
                 WS_BYTES = (WS_CTL + 8 * sizeof(double) + 255) & ~(size_t)255;

bool unit_ok(double x) { return x >= 0.0 && x < 1.0; }
bool nonneg_finite(double x) { return x >= 0.0 && x <= 1.7976931348623157e308; }

}  // namespace

extern "C" size_t mvx_optim_workspace_bytes(int64_t n) {
    (void)n;                      // the norm pass has a constant grid: the scratch does not grow with the buffer
    return WS_BYTES;
}

extern "C" int mvx_optim_adamw_step(const int64_t *chunk_table, int32_t n_chunks, const float *grad_flat, float *m_flat, float *v_flat,
                                    int64_t n, const float *count_or_null, double *state, double lr, double beta1, double beta2,
                                    double eps, double weight_decay, double max_norm, int32_t guard, void *workspace,
                                    size_t workspace_bytes, void *stream) {
    MVX_CHECK_ARG(chunk_table && grad_flat && m_flat && v_flat && state && workspace);
    MVX_CHECK_ARG(n >= 1 && n < (1ll << 31) && n_chunks >= 1 && (int64_t)n_chunks <= n && (int64_t)n_chunks * OPT_CHUNK >= n);
    MVX_CHECK_ARG(((uintptr_t)grad_flat & 3) == 0 && ((uintptr_t)m_flat & 3) == 0 && ((uintptr_t)v_flat & 3) == 0);
    MVX_CHECK_ARG(((uintptr_t)chunk_table & 7) == 0 && ((uintptr_t)state & 7) == 0 && ((uintptr_t)workspace & 7) == 0);
    MVX_CHECK_ARG(!count_or_null || ((uintptr_t)count_or_null & 3) == 0);
    MVX_CHECK_ARG(m_flat != v_flat && (const float *)m_flat != grad_flat && (const float *)v_flat != grad_flat);
    MVX_CHECK_ARG(nonneg_finite(lr) && unit_ok(beta1) && unit_ok(beta2) && nonneg_finite(eps) && nonneg_finite(weight_decay));
    MVX_CHECK_ARG(nonneg_finite(max_norm));
    MVX_CHECK_ARG(workspace_bytes >= WS_BYTES);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    double *partial = (double *)(ws + WS_PARTIAL), *ctl = (double *)(ws + WS_CTL);
    int *flags = (int *)(ws + WS_FLAGS);
    const long long per = (((long long)n + OPT_G - 1) / OPT_G + 3) & ~3ll;
    hipLaunchKernelGGL(optim_norm_partial, dim3(OPT_G), dim3(OPT_THREADS), 0, st, grad_flat, (long long)n, per, partial, flags);
    MVX_LAUNCH_CHECK();
    PrepArgs a = {partial, flags, count_or_null, state, ctl, lr, beta1, beta2, eps, weight_decay, max_norm, guard != 0};
    hipLaunchKernelGGL(optim_prepare, dim3(1), dim3(64), 0, st, a);
    MVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(optim_adamw_update, dim3(n_chunks), dim3(OPT_THREADS), 0, st, (const long long *)chunk_table, grad_flat, m_flat,
                       v_flat, (long long)n, (const double *)ctl, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2));
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}
