// cudaraytracing_amd/csrc/crt_nlm.hip -- non-local means with variance-normalised patch distances, joint with the guides
// (crt_denoise_nlm / crt_denoise_nlm_device, contract: include/crt.h): kernels and host code.  An image operation without a scene handle.
//
// One call = k_nlm_pack ((r, g, b, g(p)), (normal.xyz, depth) and (albedo.xyz, v(p)) into three float4 planes of the caller's scratch)
// and one filter launch.  The arithmetic of a pair, of a weight and every index of the LDS staging are in crt_nlm.h, which
// tools/nlm_host_check.cpp compiles for the host.  Two forms of the filter, the same bits from both:
//   k_nlm_direct  one thread per pixel, a wave = 64 pixels of a row, the contract as written with every tap through the caches;
//   k_nlm_shared  a workgroup per 32 x 8 tile: the colour plane of tile + halo in LDS once, per window offset each pair term once, each
//                 row sum once, then per pixel the column of row sums, the guide terms and the weight; sums in registers across offsets.
// CRT_NLM_FORM=direct|shared (read per call; tests and tools/denoise_probe.py) selects the form; unset: the faster one at 800x600
// (docs/experiments.md, "The non-local-means filter").
#include "crt_filter_host.h"
#include "crt_nlm.h"

#include <cmath>
#include <cstring>
#include <string>

namespace crtk {

__global__ __launch_bounds__(256) void k_nlm_pack(const NlmPack K)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= (uint64_t)K.width * K.height) return;
    const uint32_t y = (uint32_t)(p / K.width);
    nlm_pack_pixel(K, (int)(p - (uint64_t)y * K.width), (int)y);
}

// Block = 64 x 4 pixels, as the a-trous passes
__global__ __launch_bounds__(256) void k_nlm_direct(const NlmParams P)
{
    const uint32_t by = blockIdx.x / P.tiles_x, bx = blockIdx.x - by * P.tiles_x;
    const int x = (int)(bx * 64u + (threadIdx.x & 63u)), y = (int)(by * 4u + (threadIdx.x >> 6));
    if (x >= (int)P.width || y >= (int)P.height) return;
    nlm_direct_pixel(P, x, y);
}

// Block = one tile of kNlmTileW x kNlmTileH pixels; dynamic LDS: nlm_lds_bytes(radius, patch).  No thread leaves before the last
// barrier: the pixels of a ragged tile that lie outside the image still take their share of the three shared phases.
__global__ __launch_bounds__(kNlmThreads) void k_nlm_shared(const NlmParams P)
{
    extern __shared__ float4 s_c[];
    const NlmTile T = nlm_tile(P, blockIdx.x);
    float* const s_d = (float*)(s_c + T.sw * T.sh);
    float* const s_row = s_d + T.dw * T.dh;
    const int tid = (int)threadIdx.x, lx = tid & (kNlmTileW - 1), ly = tid / kNlmTileW;
    const int W = (int)P.width, H = (int)P.height, R = P.radius;
    const bool inside = T.x0 + lx < W && T.y0 + ly < H;
    const size_t p = inside ? (size_t)(T.y0 + ly) * P.width + (size_t)(T.x0 + lx) : 0;
    const float4 gp = P.g0[p], ap = P.g1[p];
    nlm_stage(P, T, tid, s_c);
    __syncthreads();
    NlmSum s = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int oy = -R; oy <= R; oy++) {
        for (int ox = -R; ox <= R; ox++) {
            if (nlm_offset_misses_tile(T, ox, oy, W, H)) continue; // (the same for every thread of the workgroup)
            nlm_phase_d(P, T, ox, oy, tid, s_c, s_d);
            __syncthreads();   // s_d of this offset is whole; the pixels are done with s_row of the offset before
            nlm_phase_row(P, T, ox, oy, tid, s_d, s_row);
            __syncthreads();   // s_row is whole; nobody reads s_d any more
            if (inside) nlm_phase_pixel(P, T, ox, oy, lx, ly, s_c, s_row, gp, ap, s);
        }
    }
    if (inside) nlm_finish(P, p, s);
}

} // namespace crtk

using namespace crtk;

namespace {

uint64_t scratch_bytes_of(uint32_t width, uint32_t height) { return (uint64_t)width * height * 3u * sizeof(float4); }

// 0: the default form, 1: direct, 2: shared, -1: a value that is neither
int form_of_environment()
{
    const char* e = std::getenv("CRT_NLM_FORM");
    if (!e || !*e) return 0;
    if (std::strcmp(e, "direct") == 0) return 1;
    if (std::strcmp(e, "shared") == 0) return 2;
    return -1;
}

// Argument checks of both forms, before any device call
int nlm_check(const char* who, const crt_nlm_params* prm, const crt_denoise_var_inputs* in, const void* out_mean, const void* out_rgb)
{
    const std::string w(who);
    if (!prm || !in) return fail(CRT_ERR_INVALID_ARG, w + ": null argument");
    if (!in->color) return fail(CRT_ERR_INVALID_ARG, w + ": null colour buffer");
    if (!in->variance) return fail(CRT_ERR_INVALID_ARG, w + ": null variance buffer");
    if (const int rc = size_positive(w, prm->width, prm->height)) return rc;
    if (prm->radius < 1 || prm->radius > (uint32_t)kNlmMaxRadius) return fail(CRT_ERR_INVALID_ARG, w + ": radius must be 1 .. 8");
    if (prm->patch > (uint32_t)kNlmMaxPatch) return fail(CRT_ERR_INVALID_ARG, w + ": patch must be 0 .. 3");
    if (!(prm->k > 0.0f) || !std::isfinite(prm->k)) return fail(CRT_ERR_INVALID_ARG, w + ": k must be > 0 and finite");
    if (!(prm->alpha >= 0.0f) || !std::isfinite(prm->alpha)) return fail(CRT_ERR_INVALID_ARG, w + ": alpha must be >= 0 and finite");
    if (!sigma_ok(prm->sigma_normal) || !sigma_ok(prm->sigma_albedo) || !sigma_ok(prm->sigma_depth))
        return fail(CRT_ERR_INVALID_ARG, w + ": every sigma must be > 0 (+inf switches a term off)");
    if (!out_mean && !out_rgb) return fail(CRT_ERR_INVALID_ARG, w + ": no output buffer");
    return size_supported(w, prm->width, prm->height, kNlmTileW, 4); // (the narrower tile with the lower one: no fewer blocks than either form launches)
}

int nlm_impl(const char* who, int device, const crt_nlm_params* prm, const crt_denoise_var_inputs* in, void* d_out_mean, void* d_out_rgb, float* d_out_var,
             void* d_scratch, uint64_t scratch_bytes, hipStream_t st, crt_denoise_info* info)
{
    const std::string w(who);
    int rc = nlm_check(who, prm, in, d_out_mean, d_out_rgb);
    if (rc == CRT_OK) rc = scratch_ok(w, d_scratch, scratch_bytes, scratch_bytes_of(prm->width, prm->height), "crt_denoise_nlm_scratch_bytes");
    if (rc != CRT_OK) return rc;
    const int form = form_of_environment();
    if (form < 0 && device >= 0) // (a bad device index is reported first: timed_launch's test)
        return fail(CRT_ERR_INVALID_ARG, w + ": CRT_NLM_FORM must be direct or shared");
    rc = timed_launch(w, device, st, info, [&] {
        const uint64_t npix = (uint64_t)prm->width * prm->height;
        float4* plane = (float4*)d_scratch;
        NlmPack K;
        K.width = prm->width; K.height = prm->height;
        K.color = in->color; K.variance = in->variance; K.albedo = in->albedo; K.normal = in->normal; K.depth = in->depth;
        K.c = plane; K.g0 = plane + npix; K.g1 = plane + 2 * npix;
        hipLaunchKernelGGL(k_nlm_pack, dim3((uint32_t)((npix + 255) / 256)), dim3(256), 0, st, K);
        HIP_CHECK(hipGetLastError());
        NlmParams P;
        std::memset(&P, 0, sizeof(P));
        P.width = prm->width; P.height = prm->height;
        P.radius = (int)prm->radius; P.patch = (int)prm->patch;
        P.k2 = prm->k * prm->k; P.alpha = prm->alpha;
        P.sig2_n = in->normal ? prm->sigma_normal * prm->sigma_normal : 1.0f;
        P.sig2_a = in->albedo ? prm->sigma_albedo * prm->sigma_albedo : 1.0f;
        P.sigma_d = prm->sigma_depth;
        P.c = K.c; P.g0 = K.g0; P.g1 = K.g1;
        P.out_mean = (float*)d_out_mean; P.out_rgb = (uint8_t*)d_out_rgb; P.out_var = d_out_var;
        if (form == 1) {
            P.tiles_x = (prm->width + 63) / 64;
            hipLaunchKernelGGL(k_nlm_direct, dim3(P.tiles_x * ((prm->height + 3) / 4)), dim3(256), 0, st, P);
        } else {
            P.tiles_x = (prm->width + kNlmTileW - 1) / kNlmTileW;
            hipLaunchKernelGGL(k_nlm_shared, dim3(P.tiles_x * ((prm->height + kNlmTileH - 1) / kNlmTileH)), dim3(kNlmThreads),
                               nlm_lds_bytes(P.radius, P.patch), st, P);
        }
    });
    if (rc == CRT_OK && info) info->passes = 1;
    return rc;
}

} // namespace

extern "C" {

int crt_denoise_nlm_defaults(crt_nlm_params* prm)
{
    if (!prm) return fail(CRT_ERR_INVALID_ARG, "crt_denoise_nlm_defaults: null argument");
    std::memset(prm, 0, sizeof(*prm));
    prm->radius = 5; prm->patch = 1; prm->k = 0.7f;
    prm->alpha = 1.0f;
    prm->sigma_normal = 0.5f; prm->sigma_albedo = 0.1f; prm->sigma_depth = 0.05f;
    return CRT_OK;
}

int crt_denoise_nlm_scratch_bytes(uint32_t width, uint32_t height, uint64_t* bytes)
{
    if (!bytes || width == 0 || height == 0) return fail(CRT_ERR_INVALID_ARG, "crt_denoise_nlm_scratch_bytes: bad arguments");
    *bytes = scratch_bytes_of(width, height);
    return CRT_OK;
}

int crt_denoise_nlm_device(int device, const crt_nlm_params* prm, const crt_denoise_var_inputs* dev_in, void* d_out_mean, void* d_out_rgb,
                           void* d_out_variance, void* d_scratch, uint64_t scratch_bytes, void* stream, crt_denoise_info* info)
{
    return nlm_impl("crt_denoise_nlm_device", device, prm, dev_in, d_out_mean, d_out_rgb, (float*)d_out_variance, d_scratch, scratch_bytes,
                    (hipStream_t)stream, info);
}

int crt_denoise_nlm(int device, const crt_nlm_params* prm, const crt_denoise_var_inputs* host_in, float* out_mean, uint8_t* out_rgb, float* out_variance,
                    crt_denoise_info* info)
{
    const int rc0 = nlm_check("crt_denoise_nlm", prm, host_in, out_mean, out_rgb);
    if (rc0 != CRT_OK) return rc0;
    const uint64_t npix = (uint64_t)prm->width * prm->height;
    return host_form("crt_denoise_nlm", device, [&](HostCopies& c) {
        crt_denoise_var_inputs d{};
        d.color = c.in(host_in->color, npix * 3);
        d.variance = c.in(host_in->variance, npix * 3);
        d.albedo = c.in(host_in->albedo, npix * 3);
        d.normal = c.in(host_in->normal, npix * 3);
        d.depth = c.in(host_in->depth, npix);
        float* d_mean = c.out(out_mean, npix * 3);
        uint8_t* d_rgb = c.out(out_rgb, npix * 3);
        float* d_ovar = c.out(out_variance, npix);
        return nlm_impl("crt_denoise_nlm_device", device, prm, &d, d_mean, d_rgb, d_ovar, c.scratch<float4>(npix * 3), npix * 3 * sizeof(float4), nullptr, info);
    });
}

} // extern "C"
