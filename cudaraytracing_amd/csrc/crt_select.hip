// cudaraytracing_amd/csrc/crt_select.hip -- crt_filter_select / crt_filter_select_device (contract: include/crt.h): per pixel the one of K
// filtered candidates whose error, estimated against the independent other half frame (crt_half_buffers), is smallest, and the frame
// blended from the candidates by the choices around each pixel.  An image operation without a scene handle, like the denoisers.  One
// call = two launches, k_select_choose and k_select_blend, with the choice map in the caller's scratch in between; their phases are in
// crt_select.h in a form the host can compile as well (tools/select_host_check.cpp).  The pixels per candidate are counted with one
// ballot, one popcount and one atomic per wave and candidate, as k_upsample counts, and only when the caller asks for the info.
#include "crt_filter_host.h"
#include "crt_select.h"

#include <cstring>
#include <string>

namespace crtk {

// dynamic LDS: select_choose_lds_bytes(P) -- 7 840 bytes at the defaults (K 2, error_radius 3), at most 30 720 (K 4, error_radius 8)
__global__ __launch_bounds__(256) void k_select_choose(const SelParams P)
{
    extern __shared__ float s_sel[];
    const SelTile T = select_tile(P, blockIdx.x);
    select_stage_errors(P, T, (int)threadIdx.x, s_sel);
    __syncthreads();
    select_row_sums(P, T, (int)threadIdx.x, s_sel);
    __syncthreads();
    const int tx = (int)(threadIdx.x & (kSelectTileW - 1u)), ty = (int)(threadIdx.x / kSelectTileW);
    int best = -1;
    if (T.x0 + tx < (int)P.width && T.y0 + ty < (int)P.height) best = select_choose_pixel(P, T, tx, ty, s_sel);
    if (!P.count) return;
    for (int k = 0; k < P.K; k++) {
        const unsigned long long mask = __ballot(best == k);
        if (mask != 0ull && (int)(threadIdx.x & 63u) == __ffsll((long long)mask) - 1)
            __hip_atomic_fetch_add(P.count + k, (unsigned long long)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// dynamic LDS: select_blend_lds_bytes(P) -- 340 bytes at blend_radius 1, at most 640
__global__ __launch_bounds__(256) void k_select_blend(const SelParams P)
{
    extern __shared__ float s_sel[];
    uint8_t* const cl = (uint8_t*)s_sel;
    const SelTile T = select_tile(P, blockIdx.x);
    select_stage_choice(P, T, (int)threadIdx.x, cl);
    __syncthreads();
    const int tx = (int)(threadIdx.x & (kSelectTileW - 1u)), ty = (int)(threadIdx.x / kSelectTileW);
    if (T.x0 + tx < (int)P.width && T.y0 + ty < (int)P.height) select_blend_pixel(P, T, tx, ty, cl);
}

} // namespace crtk

using namespace crtk;

namespace {

uint64_t select_scratch_bytes(uint32_t width, uint32_t height) { return ((uint64_t)width * height + 15ull) & ~15ull; }

// Argument checks of both forms, before any device call
int select_check(const char* who, const crt_filter_select_params* prm, const crt_filter_select_inputs* in, const void* out_mean, const void* out_rgb)
{
    const std::string w(who);
    if (!prm || !in) return fail(CRT_ERR_INVALID_ARG, w + ": null argument");
    if (const int rc = size_positive(w, prm->width, prm->height)) return rc;
    if (prm->n_candidates < 1 || prm->n_candidates > (uint32_t)kSelectMaxK) return fail(CRT_ERR_INVALID_ARG, w + ": n_candidates must be 1 .. 4");
    if (prm->error_radius > (uint32_t)kSelectMaxErrorRadius) return fail(CRT_ERR_INVALID_ARG, w + ": error_radius must be 0 .. 8");
    if (prm->blend_radius > (uint32_t)kSelectMaxBlendRadius) return fail(CRT_ERR_INVALID_ARG, w + ": blend_radius must be 0 .. 4");
    if (!in->half_a || !in->half_b) return fail(CRT_ERR_INVALID_ARG, w + ": null half buffer");
    if (!in->half_variance) return fail(CRT_ERR_INVALID_ARG, w + ": null half_variance buffer");
    for (uint32_t k = 0; k < prm->n_candidates; k++)
        if (!in->filtered_a[k] || !in->filtered_b[k]) return fail(CRT_ERR_INVALID_ARG, w + ": null filtered image of candidate " + std::to_string(k));
    if (!out_mean && !out_rgb) return fail(CRT_ERR_INVALID_ARG, w + ": no output buffer");
    return size_supported(w, prm->width, prm->height, kSelectTileW, kSelectTileH);
}

// (the caller has checked the arguments)
int select_impl(const char* who, int device, const crt_filter_select_params* prm, const crt_filter_select_inputs* in, float* out_mean, uint8_t* out_rgb,
                uint8_t* out_choice, float* out_error, void* d_scratch, hipStream_t st, crt_filter_select_info* info)
{
    SelParams P;
    std::memset(&P, 0, sizeof(P));
    P.width = prm->width; P.height = prm->height;
    P.tiles_x = (prm->width + kSelectTileW - 1) / kSelectTileW;
    P.K = (int)prm->n_candidates; P.r = (int)prm->error_radius; P.s = (int)prm->blend_radius;
    P.a = in->half_a; P.b = in->half_b; P.v = in->half_variance;
    for (int k = 0; k < P.K; k++) { P.fa[k] = in->filtered_a[k]; P.fb[k] = in->filtered_b[k]; }
    P.out_mean = out_mean; P.out_rgb = out_rgb; P.out_choice = out_choice; P.out_error = out_error;
    P.choice = (uint8_t*)d_scratch;
    const dim3 grid(P.tiles_x * ((P.height + kSelectTileH - 1) / kSelectTileH));
    unsigned long long n[kSelectMaxK] = {0, 0, 0, 0};
    const int rc = timed_launch(who, device, st, info, n, (size_t)kSelectMaxK, [&](unsigned long long* d_count) {
        P.count = d_count;
        hipLaunchKernelGGL(k_select_choose, grid, dim3(256), select_choose_lds_bytes(P), st, P);
        hipLaunchKernelGGL(k_select_blend, grid, dim3(256), select_blend_lds_bytes(P), st, P);
    });
    if (rc == CRT_OK && info)
        for (int k = 0; k < kSelectMaxK; k++) info->chosen[k] = n[k];
    return rc;
}

} // namespace

extern "C" {

int crt_filter_select_defaults(crt_filter_select_params* prm)
{
    if (!prm) return fail(CRT_ERR_INVALID_ARG, "crt_filter_select_defaults: null argument");
    std::memset(prm, 0, sizeof(*prm));
    prm->n_candidates = 2;
    prm->error_radius = 3;
    prm->blend_radius = 1;
    return CRT_OK;
}

int crt_filter_select_scratch_bytes(uint32_t width, uint32_t height, uint64_t* bytes)
{
    if (!bytes) return fail(CRT_ERR_INVALID_ARG, "crt_filter_select_scratch_bytes: null argument");
    if (const int rc = size_positive("crt_filter_select_scratch_bytes", width, height)) return rc;
    *bytes = select_scratch_bytes(width, height);
    return CRT_OK;
}

int crt_filter_select_device(int device, const crt_filter_select_params* prm, const crt_filter_select_inputs* dev_in, void* d_out_mean, void* d_out_rgb,
                             void* d_out_choice, void* d_out_error, void* d_scratch, uint64_t scratch_bytes, void* stream, crt_filter_select_info* info)
{
    const char* who = "crt_filter_select_device";
    if (const int rc = select_check(who, prm, dev_in, d_out_mean, d_out_rgb)) return rc;
    if (const int rc = scratch_ok(who, d_scratch, scratch_bytes, select_scratch_bytes(prm->width, prm->height), "crt_filter_select_scratch_bytes")) return rc;
    return select_impl(who, device, prm, dev_in, (float*)d_out_mean, (uint8_t*)d_out_rgb, (uint8_t*)d_out_choice, (float*)d_out_error, d_scratch,
                       (hipStream_t)stream, info);
}

int crt_filter_select(int device, const crt_filter_select_params* prm, const crt_filter_select_inputs* host_in, float* out_mean, uint8_t* out_rgb,
                      uint8_t* out_choice, float* out_error, crt_filter_select_info* info)
{
    if (const int rc = select_check("crt_filter_select", prm, host_in, out_mean, out_rgb)) return rc;
    const uint64_t npix = (uint64_t)prm->width * prm->height;
    return host_form("crt_filter_select", device, [&](HostCopies& c) {
        crt_filter_select_inputs d{};
        d.half_a = c.in(host_in->half_a, npix * 3);
        d.half_b = c.in(host_in->half_b, npix * 3);
        d.half_variance = c.in(host_in->half_variance, npix * 3);
        for (uint32_t k = 0; k < prm->n_candidates; k++) {
            d.filtered_a[k] = c.in(host_in->filtered_a[k], npix * 3);
            d.filtered_b[k] = c.in(host_in->filtered_b[k], npix * 3);
        }
        return select_impl("crt_filter_select", device, prm, &d, c.out(out_mean, npix * 3), c.out(out_rgb, npix * 3), c.out(out_choice, npix),
                           c.out(out_error, npix), c.scratch<uint8_t>(select_scratch_bytes(prm->width, prm->height)), nullptr, info);
    });
}

} // extern "C"
