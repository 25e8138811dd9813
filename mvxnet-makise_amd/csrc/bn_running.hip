// Running BatchNorm statistics of a step's sites (include/mvx_hip.h "Running BatchNorm statistics"): every BatchNorm site of the
// frame-set path hands its consumer mean_inv f32 [F][2][C]; with `bntrack` the training step folds those tensors into the
// modules' running_mean / running_var / num_batches_tracked, and an eval forward fills them from the buffers.  Both
// directions walk a table of sites that travels BY VALUE in the kernel arguments (like mvx_frames_t): no host
// synchronisation, no staging buffer with a lifetime, one launch for up to MVX_BN_SITES_PER_LAUNCH sites.
#include "common.h"
#include <string.h>
#include <vector>

namespace {

constexpr int POPS = 8;            // distinct per-frame population vectors of one launch (rows, three CML depths, three RPN maps)
constexpr int BLOCK = 128;

struct DevSite {
    float *mean_inv;               // [F][2][C]
    float *rm, *rv;                // [C]
    long long *nbt;                // [1]
    double momentum;
    int C, pop;
};

struct SiteChunk {
    DevSite s[MVX_BN_SITES_PER_LAUNCH];
    double pop[POPS][MVX_MAX_FRAMES];        // population of frame f; 0 = the frame takes no part
};
static_assert(sizeof(SiteChunk) + 64 <= 4096, "the table travels in the kernel arguments");

// one thread per (site, channel): the F sequential PyTorch updates of the reference's batch-1 forwards, in frame order, in
// float64 registers; every buffer element is stored once
__global__ __launch_bounds__(BLOCK) void bn_running_update(SiteChunk t, int F, double eps) {
    const DevSite &s = t.s[blockIdx.y];
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= s.C) return;
    const double m = s.momentum;
    const double *pop = t.pop[s.pop];
    double rm = (double)s.rm[c], rv = (double)s.rv[c];
    long long live = 0;
    for (int f = 0; f < F; ++f) {
        const double n = pop[f];
        if (!(n > 0.0)) continue;
        const double mean = (double)s.mean_inv[((size_t)f * 2) * s.C + c];
        const double inv = (double)s.mean_inv[((size_t)f * 2 + 1) * s.C + c];
        double var = 1.0 / (inv * inv) - eps;
        if (!(var > 0.0)) var = 0.0;
        rm = (1.0 - m) * rm + m * mean;
        if (n > 1.0) rv = (1.0 - m) * rv + m * (var * n / (n - 1.0));      // a population of one has no unbiased variance
        ++live;
    }
    s.rm[c] = (float)rm;
    s.rv[c] = (float)rv;
    if (c == 0) s.nbt[0] += live;
}

// one thread per (site, channel): (running_mean, 1 / sqrt(running_var + eps)) for every frame of the set
__global__ __launch_bounds__(BLOCK) void bn_running_mean_inv(SiteChunk t, int F, double eps) {
    const DevSite &s = t.s[blockIdx.y];
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= s.C) return;
    const float mean = s.rm[c];
    const float inv = (float)(1.0 / sqrt((double)s.rv[c] + eps));
    for (int f = 0; f < F; ++f) {
        s.mean_inv[((size_t)f * 2) * s.C + c] = mean;
        s.mean_inv[((size_t)f * 2 + 1) * s.C + c] = inv;
    }
}

bool site_ok(const mvx_bn_site_t &h, bool update) {
    if (!h.mean_inv || !h.running_mean || !h.running_var || h.channels <= 0) return false;
    if (!update) return true;
    return h.num_batches_tracked && h.rows >= 0 && h.momentum >= 0.0 && h.momentum <= 1.0;
}

// Per-frame populations of a site, from where the finalisers take them: the frame map of its row layout.
bool site_pops(const mvx_bn_site_t &h, const mvx_frames_t *fr, int F, uint32_t live_mask, double *pop) {
    mvx_frames_t grid;
    if (h.row_kind == MVX_ROWS_GRID) {          // equal shares: only the frame count matters
        grid.n_frames = F;
        grid.t = 1;
        for (int k = 0; k <= MVX_MAX_FRAMES; ++k) grid.real_off[k] = grid.vox_off[k] = 0;
        fr = &grid;
    } else if (!fr || fr->n_frames != F || h.row_kind == MVX_ROWS_SINGLE) {
        return false;
    }
    FrameMap fm;
    if (!mvx_build_frame_map(fm, fr, h.row_kind, h.rows, 1.0)) return false;
    for (int f = 0; f < MVX_MAX_FRAMES; ++f) pop[f] = (f < F && ((live_mask >> f) & 1u)) ? fm.count[f] : 0.0;
    return true;
}

template <typename Kernel>
int launch_chunk(Kernel kernel, const SiteChunk &chunk, int n, int max_c, int F, double eps, hipStream_t st) {
    hipLaunchKernelGGL(kernel, dim3(mvx_cdiv(max_c, BLOCK), n), dim3(BLOCK), 0, st, chunk, F, eps);
    MVX_LAUNCH_CHECK();
    return MVX_OK;
}

// index of `pop` among the chunk's n_pop population vectors; n_pop when it is not there yet
int find_pop(const SiteChunk &chunk, int n_pop, const double *pop) {
    int p = 0;
    while (p < n_pop && memcmp(chunk.pop[p], pop, sizeof(chunk.pop[p])) != 0) ++p;
    return p;
}

int run_sites(const mvx_bn_site_t *sites, int n_sites, const mvx_frames_t *fr, int F, uint32_t live_mask, double eps,
              bool update, hipStream_t st) {
    MVX_CHECK_ARG(sites && n_sites >= 0 && F >= 1 && F <= MVX_MAX_FRAMES && eps >= 0.0);
    // every site is checked, and its populations are formed, before the first launch: a refused call has changed no buffer
    struct Pop { double n[MVX_MAX_FRAMES]; };
    std::vector<Pop> pops(update ? n_sites : 0);
    for (int i = 0; i < n_sites; ++i) {
        MVX_CHECK_ARG(site_ok(sites[i], update));
        if (update) MVX_CHECK_ARG(site_pops(sites[i], fr, F, live_mask, pops[i].n));
    }
    const auto kernel = update ? bn_running_update : bn_running_mean_inv;
    SiteChunk chunk = {};
    int n = 0, n_pop = 0, max_c = 0;
    for (int i = 0; i < n_sites; ++i) {
        const mvx_bn_site_t &h = sites[i];
        int p = update ? find_pop(chunk, n_pop, pops[i].n) : 0;
        if (n == MVX_BN_SITES_PER_LAUNCH || p == POPS) {          // no room for the site or for its populations: the table goes out
            const int rc = launch_chunk(kernel, chunk, n, max_c, F, eps, st);
            if (rc != MVX_OK) return rc;
            n = n_pop = max_c = p = 0;                            // ... and this site opens the next one
        }
        if (update && p == n_pop) memcpy(chunk.pop[n_pop++], pops[i].n, sizeof(chunk.pop[0]));
        DevSite &d = chunk.s[n++];
        d.mean_inv = h.mean_inv;
        d.rm = h.running_mean;
        d.rv = h.running_var;
        d.nbt = (long long *)h.num_batches_tracked;
        d.momentum = h.momentum;
        d.C = h.channels;
        d.pop = p;
        max_c = h.channels > max_c ? h.channels : max_c;
    }
    return n ? launch_chunk(kernel, chunk, n, max_c, F, eps, st) : MVX_OK;
}

}  // namespace

extern "C" int mvx_bn_running_update_sites(const mvx_bn_site_t *sites_host, int32_t n_sites, const mvx_frames_t *frames_host,
                                           int32_t n_frames, uint32_t live_mask, double eps, void *stream) {
    return run_sites(sites_host, n_sites, frames_host, n_frames, live_mask, eps, true, (hipStream_t)stream);
}

extern "C" int mvx_bn_running_mean_inv_sites(const mvx_bn_site_t *sites_host, int32_t n_sites, int32_t n_frames, double eps,
                                             void *stream) {
    return run_sites(sites_host, n_sites, nullptr, n_frames, 0u, eps, false, (hipStream_t)stream);
}
