// cudaraytracing_amd/csrc/crt_upsample.hip -- crt_upsample / crt_upsample_device (contract: include/crt.h): the host side of guide-driven
// upsampling, which brings an image rendered at a fraction of the resolution (irradiance, as crt_demodulate makes it) to the output's
// resolution along albedo, normal and depth at both sizes.  An image operation without a scene handle and without scratch, like
// crt_temporal.  One call = one launch of k_upsample, whose phases are in crt_upsample.h in a form the host can compile as well
// (tools/upsample_host_check.cpp): the workgroup stages the low-resolution pixels its 64 x 4 output pixels can tap in LDS, then one
// thread per output pixel.  The count of fallback pixels is one ballot, one popcount and one atomic per wave, as k_temporal counts,
// and only when the caller asks for the info.
#include "crt_filter_host.h"
#include "crt_upsample.h"

#include <cstring>
#include <limits>
#include <string>

namespace crtk {

// dynamic LDS: upsample_lds_bytes(P) -- 7 072 bytes at factor 2 and radius 1, at most 40 612 (radius 4 at equal sizes)
__global__ __launch_bounds__(256) void k_upsample(const UpParams P)
{
    extern __shared__ float s_tile[];
    const UpTile T = upsample_tile(P, blockIdx.x);
    upsample_stage(P, T, (int)threadIdx.x, s_tile);
    __syncthreads();
    const uint32_t by = blockIdx.x / P.tiles_x, bx = blockIdx.x - by * P.tiles_x;
    const uint32_t x = bx * kUpsampleTileW + (threadIdx.x & 63u), y = by * kUpsampleTileH + (threadIdx.x >> 6);
    bool fell_back = false;
    if (x < P.width && y < P.height) fell_back = !upsample_pixel_staged(P, T, x, y, s_tile);
    if (!P.count) return;
    const unsigned long long mask = __ballot(fell_back);
    if (mask == 0ull) return;
    if ((int)(threadIdx.x & 63u) == __ffsll((long long)mask) - 1)
        __hip_atomic_fetch_add(P.count, (unsigned long long)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

} // namespace crtk

using namespace crtk;

namespace {

// Argument checks of both forms, before any device call
int upsample_check(const char* who, const crt_upsample_params* prm, const crt_upsample_low* low, const crt_upsample_guides* guides, const void* out_color,
                   const void* out_variance, const void* out_rgb)
{
    const std::string w(who);
    if (!prm || !low) return fail(CRT_ERR_INVALID_ARG, w + ": null argument");
    if (!low->color) return fail(CRT_ERR_INVALID_ARG, w + ": null colour buffer");
    if (const int rc = size_positive(w, prm->width, prm->height)) return rc;
    if (const int rc = size_positive(w, prm->low_width, prm->low_height)) return rc;
    if (prm->low_width > prm->width || prm->low_height > prm->height)
        return fail(CRT_ERR_INVALID_ARG, w + ": the low-resolution image is larger than the output");
    if (prm->radius < 1 || prm->radius > 4) return fail(CRT_ERR_INVALID_ARG, w + ": radius must be 1 .. 4");
    if (!(prm->min_weight >= 0.0f && prm->min_weight < std::numeric_limits<float>::infinity()))
        return fail(CRT_ERR_INVALID_ARG, w + ": min_weight must be >= 0 and finite");
    if (!sigma_ok(prm->sigma_normal) || !sigma_ok(prm->sigma_albedo) || !sigma_ok(prm->sigma_depth))
        return fail(CRT_ERR_INVALID_ARG, w + ": every sigma must be > 0 (+inf switches a term off)");
    if (guides) {
        if ((low->albedo != nullptr) != (guides->albedo != nullptr) || (low->normal != nullptr) != (guides->normal != nullptr) ||
            (low->depth != nullptr) != (guides->depth != nullptr))
            return fail(CRT_ERR_INVALID_ARG, w + ": a guide must be given at both resolutions or at neither");
    }
    if ((low->variance != nullptr) != (out_variance != nullptr)) return fail(CRT_ERR_INVALID_ARG, w + ": variance and out_variance go together");
    if (!out_color && !out_rgb) return fail(CRT_ERR_INVALID_ARG, w + ": no output buffer");
    return size_supported(w, prm->width, prm->height, kUpsampleTileW, kUpsampleTileH);
}

// (the caller has checked the arguments; guides == nullptr: no guide term, whatever `low` holds)
int upsample_impl(const char* who, int device, const crt_upsample_params* prm, const crt_upsample_low* low, const crt_upsample_guides* guides,
                  float* out_color, float* out_variance, uint8_t* out_rgb, hipStream_t st, crt_upsample_info* info)
{
    UpParams P;
    std::memset(&P, 0, sizeof(P));
    P.width = prm->width; P.height = prm->height; P.low_width = prm->low_width; P.low_height = prm->low_height;
    P.tiles_x = (prm->width + kUpsampleTileW - 1) / kUpsampleTileW;
    P.radius = (int)prm->radius; P.fradius = (float)prm->radius;
    P.sx = (float)prm->low_width / (float)prm->width;
    P.sy = (float)prm->low_height / (float)prm->height;
    P.min_weight = prm->min_weight;
    P.color = low->color; P.variance = low->variance;
    if (guides) {
        P.albedo = guides->albedo; P.normal = guides->normal; P.depth = guides->depth;
        P.lalbedo = low->albedo; P.lnormal = low->normal; P.ldepth = low->depth;
    }
    P.sig2_n = P.normal ? prm->sigma_normal * prm->sigma_normal : 1.0f;
    P.sig2_a = P.albedo ? prm->sigma_albedo * prm->sigma_albedo : 1.0f;
    P.sigma_d = prm->sigma_depth;
    P.out_mean = out_color; P.out_rgb = out_rgb; P.out_variance = out_variance;
    P.cap = upsample_stage_cap(P);
    unsigned long long n = 0;
    const int rc = timed_launch(who, device, st, info, &n, 1, [&](unsigned long long* d_count) {
        P.count = d_count;
        hipLaunchKernelGGL(k_upsample, dim3(P.tiles_x * ((P.height + kUpsampleTileH - 1) / kUpsampleTileH)), dim3(256), upsample_lds_bytes(P), st, P);
    });
    if (rc == CRT_OK && info) info->fallback_pixels = n;
    return rc;
}

} // namespace

extern "C" {

int crt_upsample_defaults(crt_upsample_params* prm)
{
    if (!prm) return fail(CRT_ERR_INVALID_ARG, "crt_upsample_defaults: null argument");
    std::memset(prm, 0, sizeof(*prm));
    prm->radius = 1;
    prm->min_weight = 0.015625f;
    prm->sigma_normal = 0.5f; prm->sigma_albedo = 0.1f; prm->sigma_depth = 0.05f;
    return CRT_OK;
}

int crt_upsample_device(int device, const crt_upsample_params* prm, const crt_upsample_low* dev_low, const crt_upsample_guides* dev_guides,
                        void* d_out_color, void* d_out_variance, void* d_out_rgb, void* stream, crt_upsample_info* info)
{
    const int rc = upsample_check("crt_upsample_device", prm, dev_low, dev_guides, d_out_color, d_out_variance, d_out_rgb);
    if (rc != CRT_OK) return rc;
    return upsample_impl("crt_upsample_device", device, prm, dev_low, dev_guides, (float*)d_out_color, (float*)d_out_variance, (uint8_t*)d_out_rgb,
                         (hipStream_t)stream, info);
}

int crt_upsample(int device, const crt_upsample_params* prm, const crt_upsample_low* host_low, const crt_upsample_guides* host_guides, float* out_color,
                 float* out_variance, uint8_t* out_rgb, crt_upsample_info* info)
{
    const int rc0 = upsample_check("crt_upsample", prm, host_low, host_guides, out_color, out_variance, out_rgb);
    if (rc0 != CRT_OK) return rc0;
    const uint64_t npix = (uint64_t)prm->width * prm->height, nlow = (uint64_t)prm->low_width * prm->low_height;
    return host_form("crt_upsample", device, [&](HostCopies& c) {
        crt_upsample_low dl{};
        crt_upsample_guides dg{};
        dl.color = c.in(host_low->color, nlow * 3);
        dl.variance = c.in(host_low->variance, nlow * 3);
        if (host_guides) { // (without them the low-resolution guides are not read)
            dl.albedo = c.in(host_low->albedo, nlow * 3);
            dl.normal = c.in(host_low->normal, nlow * 3);
            dl.depth = c.in(host_low->depth, nlow);
            dg.albedo = c.in(host_guides->albedo, npix * 3);
            dg.normal = c.in(host_guides->normal, npix * 3);
            dg.depth = c.in(host_guides->depth, npix);
        }
        return upsample_impl("crt_upsample_device", device, prm, &dl, host_guides ? &dg : nullptr, c.out(out_color, npix * 3), c.out(out_variance, npix * 3),
                             c.out(out_rgb, npix * 3), nullptr, info);
    });
}

} // extern "C"
