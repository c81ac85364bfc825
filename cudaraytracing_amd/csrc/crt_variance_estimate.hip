// cudaraytracing_amd/csrc/crt_variance_estimate.hip -- per-pixel variance from the temporal moments that crt_temporal_moments carries
// (crt_variance_estimate / crt_variance_estimate_device, contract: include/crt.h): kernel and host code.  An image operation without a
// scene handle and without scratch, the step of SVGF between its temporal accumulation and its variance-guided filter.
//
// One call = one launch of k_variance_estimate: one thread per pixel, block = 64 x 4 pixels, a wave = 64 consecutive pixels of one row
// (the denoiser's pass).  A pixel whose history is long enough takes m2 - m1^2 of its own moments: two loads and three operations per
// channel.  A pixel with a short history takes the same statistic of the (2 radius + 1)^2 pixels around it, weighted by the denoiser's
// normal and depth terms, and boosts it by min_history / history; its taps (40 B each) are read straight from the caller's buffers.  One
// ballot per wave decides whether the wave enters the tap loop at all -- after a few frames the short histories lie along disocclusion
// edges and most waves have none -- and the same mask is the wave's share of the count of such pixels (one popcount, one atomic).
#include "crt_filter_host.h"

#include <cstring>
#include <string>

namespace crtk {

struct VeParams {
    uint32_t width, height, tiles_x;
    int radius;
    float min_history;                        // (float)min_history
    float sig2_n, sigma_d;                    // sigma_normal^2, sigma_depth
    uint32_t of_mean;
    float history_cap;
    const float* m1; const float* m2; const float* history;
    const float* normal; const float* depth;  // either may be null: its term is +0
    float* out;
    unsigned long long* count;                // pixels that took the spatial branch (null: not counted)
};

__device__ __forceinline__ float ve_clamp0(const float e) { return e < 0.0f ? 0.0f : e; } // (NaN stays NaN)

__global__ __launch_bounds__(256) void k_variance_estimate(const VeParams P)
{
    const uint32_t by = blockIdx.x / P.tiles_x, bx = blockIdx.x - by * P.tiles_x;
    const int x = (int)(bx * 64u + (threadIdx.x & 63u)), y = (int)(by * 4u + (threadIdx.x >> 6));
    const int W = (int)P.width, H = (int)P.height;
    const bool inside = x < W && y < H;
    const size_t p = inside ? (size_t)y * P.width + (size_t)x : 0;
    const float n = inside ? P.history[p] : 0.0f;
    const bool spatial = inside && !(n >= P.min_history); // (a NaN history length lands here)
    const unsigned long long mask = __ballot(spatial);
    F3 var = f3(0.0f, 0.0f, 0.0f);
    if (inside && !spatial) {
        const float ax = P.m1[p * 3], ay = P.m1[p * 3 + 1], az = P.m1[p * 3 + 2];
        var = f3(ve_clamp0(P.m2[p * 3] - ax * ax), ve_clamp0(P.m2[p * 3 + 1] - ay * ay), ve_clamp0(P.m2[p * 3 + 2] - az * az));
    }
    if (mask != 0ull && spatial) { // every tap is tested against the image, so every read is inside it
        F3 np = f3(0.0f, 0.0f, 0.0f);
        if (P.normal) np = f3(P.normal[p * 3], P.normal[p * 3 + 1], P.normal[p * 3 + 2]);
        const float dp = P.depth ? P.depth[p] : 0.0f;
        F3 s1 = f3(0.0f, 0.0f, 0.0f), s2 = f3(0.0f, 0.0f, 0.0f);
        float sw = 0.0f;
        for (int dy = -P.radius; dy <= P.radius; dy++) {
            const int qy = y + dy;
            if (qy < 0 || qy >= H) continue;
            for (int dx = -P.radius; dx <= P.radius; dx++) {
                const int qx = x + dx;
                if (qx < 0 || qx >= W) continue;
                const size_t q = (size_t)qy * P.width + (size_t)qx;
                float e_n = 0.0f, e_d = 0.0f;
                if (P.normal) {
                    const float dnx = np.x - P.normal[q * 3], dny = np.y - P.normal[q * 3 + 1], dnz = np.z - P.normal[q * 3 + 2];
                    e_n = (dnx * dnx + dny * dny + dnz * dnz) / P.sig2_n;
                }
                if (P.depth) {
                    const float dq = P.depth[q];
                    const float m = dp > dq ? dp : dq;
                    const float r = (dp - dq) / (P.sigma_d * m);
                    e_d = m > 0.0f ? r * r : 0.0f;
                }
                const float w = det_expf(-(e_n + e_d));
                s1.x = s1.x + P.m1[q * 3] * w;
                s1.y = s1.y + P.m1[q * 3 + 1] * w;
                s1.z = s1.z + P.m1[q * 3 + 2] * w;
                s2.x = s2.x + P.m2[q * 3] * w;
                s2.y = s2.y + P.m2[q * 3 + 1] * w;
                s2.z = s2.z + P.m2[q * 3 + 2] * w;
                sw = sw + w;
            }
        }
        const float mx = s1.x / sw, my = s1.y / sw, mz = s1.z / sw;
        const float boost = P.min_history / n;
        var = f3(ve_clamp0(s2.x / sw - mx * mx) * boost, ve_clamp0(s2.y / sw - my * my) * boost, ve_clamp0(s2.z / sw - mz * mz) * boost);
    }
    if (inside) {
        if (P.of_mean) {
            const float ne = n > P.history_cap ? P.history_cap : n;
            var = f3(var.x / ne, var.y / ne, var.z / ne);
        }
        P.out[p * 3] = var.x; P.out[p * 3 + 1] = var.y; P.out[p * 3 + 2] = var.z;
    }
    if (!P.count || mask == 0ull) return;
    if ((int)(threadIdx.x & 63u) == __ffsll((long long)mask) - 1)
        __hip_atomic_fetch_add(P.count, (unsigned long long)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

} // namespace crtk

using namespace crtk;

namespace {

// Argument checks of both forms, before any device call
int estimate_check(const char* who, const crt_variance_estimate_params* prm, const crt_variance_estimate_inputs* in, const void* out_variance)
{
    const std::string w(who);
    if (!prm || !in) return fail(CRT_ERR_INVALID_ARG, w + ": null argument");
    if (!in->m1 || !in->m2 || !in->history) return fail(CRT_ERR_INVALID_ARG, w + ": m1, m2 and history are required");
    if (!out_variance) return fail(CRT_ERR_INVALID_ARG, w + ": null output buffer");
    if (const int rc = size_positive(w, prm->width, prm->height)) return rc;
    if (prm->min_history < 1) return fail(CRT_ERR_INVALID_ARG, w + ": min_history must be >= 1");
    if (prm->radius < 1 || prm->radius > 3) return fail(CRT_ERR_INVALID_ARG, w + ": radius must be 1 .. 3");
    if (!sigma_ok(prm->sigma_normal) || !sigma_ok(prm->sigma_depth))
        return fail(CRT_ERR_INVALID_ARG, w + ": every sigma must be > 0 (+inf switches a term off)");
    if (!(prm->history_cap >= 1.0f)) return fail(CRT_ERR_INVALID_ARG, w + ": history_cap must be >= 1 (+inf: no cap)"); // (false for NaN)
    return size_supported(w, prm->width, prm->height, 64, 4);
}

int estimate_impl(const char* who, int device, const crt_variance_estimate_params* prm, const crt_variance_estimate_inputs* in, void* d_out,
                  hipStream_t st, crt_variance_estimate_info* info)
{
    const int rc = estimate_check(who, prm, in, d_out);
    if (rc != CRT_OK) return rc;
    VeParams P;
    std::memset(&P, 0, sizeof(P));
    P.width = prm->width; P.height = prm->height;
    P.tiles_x = (prm->width + 63) / 64;
    P.radius = (int)prm->radius;
    P.min_history = (float)prm->min_history;
    P.sig2_n = prm->sigma_normal * prm->sigma_normal;
    P.sigma_d = prm->sigma_depth;
    P.of_mean = prm->of_mean;
    P.history_cap = prm->history_cap;
    P.m1 = in->m1; P.m2 = in->m2; P.history = in->history; P.normal = in->normal; P.depth = in->depth;
    P.out = (float*)d_out;
    unsigned long long spatial = 0;
    const int status = timed_launch(who, device, st, info, &spatial, 1, [&](unsigned long long* d_count) {
        P.count = d_count;
        hipLaunchKernelGGL(k_variance_estimate, dim3(P.tiles_x * ((prm->height + 3) / 4)), dim3(256), 0, st, P);
    });
    if (status == CRT_OK && info) info->spatial = spatial;
    return status;
}

} // namespace

extern "C" {

int crt_variance_estimate_defaults(crt_variance_estimate_params* prm)
{
    if (!prm) return fail(CRT_ERR_INVALID_ARG, "crt_variance_estimate_defaults: null argument");
    std::memset(prm, 0, sizeof(*prm));
    prm->min_history = 4; prm->radius = 3;
    prm->sigma_normal = 0.5f; prm->sigma_depth = 0.05f;
    prm->of_mean = 0; prm->history_cap = 39.0f;
    return CRT_OK;
}

int crt_variance_estimate_device(int device, const crt_variance_estimate_params* prm, const crt_variance_estimate_inputs* dev_in, void* d_out_variance,
                                 void* stream, crt_variance_estimate_info* info)
{
    return estimate_impl("crt_variance_estimate_device", device, prm, dev_in, d_out_variance, (hipStream_t)stream, info);
}

// The host-buffer form: the argument checks, device copies of the inputs, the device form, then the copy back.
int crt_variance_estimate(int device, const crt_variance_estimate_params* prm, const crt_variance_estimate_inputs* host_in, float* out_variance,
                          crt_variance_estimate_info* info)
{
    const int rc0 = estimate_check("crt_variance_estimate", prm, host_in, out_variance);
    if (rc0 != CRT_OK) return rc0;
    const uint64_t npix = (uint64_t)prm->width * prm->height;
    return host_form("crt_variance_estimate", device, [&](HostCopies& c) {
        crt_variance_estimate_inputs d{};
        d.m1 = c.in(host_in->m1, npix * 3);
        d.m2 = c.in(host_in->m2, npix * 3);
        d.history = c.in(host_in->history, npix);
        d.normal = c.in(host_in->normal, npix * 3);
        d.depth = c.in(host_in->depth, npix);
        return estimate_impl("crt_variance_estimate", device, prm, &d, c.out(out_variance, npix * 3), nullptr, info);
    });
}

} // extern "C"
