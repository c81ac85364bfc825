// cudaraytracing_amd/csrc/crt_regress.hip -- first-order feature regression with non-local-means weights (crt_denoise_regress /
// crt_denoise_regress_device, contract: include/crt.h): kernels and host code.  An image operation without a scene handle.
//
// One call = k_regress_pack ((weight colour, g of the weight variance), (normal.xyz, depth), (albedo.xyz, -) and (colour, 0) into four
// float4 planes of the caller's scratch) and one launch of k_regress<MASK>, the instantiation of the call's feature mask.  The arithmetic
// and every LDS index are in crt_nlm.h (everything up to the weight) and crt_regress.h (what follows it), which
// tools/regress_host_check.cpp compiles for the host.  The filter has one form, the shared one, k_nlm_shared's: a workgroup per 32 x 8
// tile, the weight plane of tile + halo in LDS once, per window offset each pair term once and each row sum once, then per pixel the
// column of row sums, the weight, the regressors and the sums of the normal equations, which stay in registers across the window
// (up to 55 + 30 at the full mask; docs/experiments.md, "The feature-regression filter", has the register counts per instantiation).
// The fallback pixels are counted with one ballot, one popcount and one atomic per wave, as k_upsample counts, and only with an info.
#include "crt_filter_host.h"
#include "crt_nlm.h"
#include "crt_regress.h"

#include <cmath>
#include <cstring>
#include <string>

namespace crtk {

__global__ __launch_bounds__(256) void k_regress_pack(const RegPack K)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= (uint64_t)K.n.width * K.n.height) return;
    const uint32_t y = (uint32_t)(p / K.n.width);
    regress_pack_pixel(K, (int)(p - (uint64_t)y * K.n.width), (int)y);
}

// Block = one tile of kNlmTileW x kNlmTileH pixels; dynamic LDS: nlm_lds_bytes(radius, patch).  No thread leaves before the last
// barrier nor before the ballot: the pixels of a ragged tile that lie outside the image take their share of the shared phases.
template <int MASK> __global__ __launch_bounds__(kNlmThreads) void k_regress(const RegParams P)
{
    constexpr int F = regress_features(MASK);
    extern __shared__ float4 s_c[];
    const NlmTile T = nlm_tile(P.n, blockIdx.x);
    float* const s_d = (float*)(s_c + T.sw * T.sh);
    float* const s_row = s_d + T.dw * T.dh;
    const int tid = (int)threadIdx.x, lx = tid & (kNlmTileW - 1), ly = tid / kNlmTileW;
    const int W = (int)P.n.width, H = (int)P.n.height, R = P.n.radius;
    const bool inside = T.x0 + lx < W && T.y0 + ly < H;
    const size_t p = inside ? (size_t)(T.y0 + ly) * P.n.width + (size_t)(T.x0 + lx) : 0;
    const float4 gp = P.n.g0[p], ap = P.n.g1[p];
    nlm_stage(P.n, T, tid, s_c);
    __syncthreads();
    RegSums<F> s;
    regress_zero<F>(s);
    for (int oy = -R; oy <= R; oy++) {
        for (int ox = -R; ox <= R; ox++) {
            if (nlm_offset_misses_tile(T, ox, oy, W, H)) continue; // (the same for every thread of the workgroup)
            nlm_phase_d(P.n, T, ox, oy, tid, s_c, s_d);
            __syncthreads();   // s_d of this offset is whole; the pixels are done with s_row of the offset before
            nlm_phase_row(P.n, T, ox, oy, tid, s_d, s_row);
            __syncthreads();   // s_row is whole; nobody reads s_d any more
            if (inside) regress_phase_pixel<MASK>(P, T, ox, oy, lx, ly, s_row, gp, ap, s);
        }
    }
    bool fell_back = false;
    if (inside) fell_back = regress_finish<F>(P, p, s);
    if (!P.count) return;
    const unsigned long long mask = __ballot(fell_back);
    if (mask == 0ull) return;
    if ((int)(threadIdx.x & 63u) == __ffsll((long long)mask) - 1)
        __hip_atomic_fetch_add(P.count, (unsigned long long)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

} // namespace crtk

using namespace crtk;

namespace {

const uint64_t kPlanes = 4;
uint64_t scratch_bytes_of(uint32_t width, uint32_t height) { return (uint64_t)width * height * kPlanes * sizeof(float4); }

template <int MASK> void launch_mask(const RegParams& P, uint32_t blocks, uint32_t lds, hipStream_t st)
{
    hipLaunchKernelGGL(k_regress<MASK>, dim3(blocks), dim3(kNlmThreads), lds, st, P);
}

void launch(uint32_t mask, const RegParams& P, uint32_t blocks, uint32_t lds, hipStream_t st)
{
    switch (mask) {
#define CRT_REGRESS_CASE(m) case m: launch_mask<m>(P, blocks, lds, st); break;
        CRT_REGRESS_CASE(0) CRT_REGRESS_CASE(1) CRT_REGRESS_CASE(2) CRT_REGRESS_CASE(3) CRT_REGRESS_CASE(4) CRT_REGRESS_CASE(5) CRT_REGRESS_CASE(6)
        CRT_REGRESS_CASE(7) CRT_REGRESS_CASE(8) CRT_REGRESS_CASE(9) CRT_REGRESS_CASE(10) CRT_REGRESS_CASE(11) CRT_REGRESS_CASE(12) CRT_REGRESS_CASE(13)
        CRT_REGRESS_CASE(14) CRT_REGRESS_CASE(15)
#undef CRT_REGRESS_CASE
    }
}

// Argument checks of both forms, before any device call
int regress_check(const char* who, const crt_regress_params* prm, const crt_regress_inputs* in, const void* out_mean, const void* out_rgb)
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
    if (!sigma_ok(prm->sigma_normal) || !sigma_ok(prm->sigma_albedo) || !sigma_ok(prm->sigma_depth) || !sigma_ok(prm->sigma_position))
        return fail(CRT_ERR_INVALID_ARG, w + ": every sigma must be > 0");
    if (!(prm->ridge >= 0.0f) || !std::isfinite(prm->ridge)) return fail(CRT_ERR_INVALID_ARG, w + ": ridge must be >= 0 and finite");
    if (prm->features & ~(uint32_t)kRegAllFeatures) return fail(CRT_ERR_INVALID_ARG, w + ": unknown bits in the features mask");
    if ((prm->features & CRT_REGRESS_NORMAL) && !in->normal) return fail(CRT_ERR_INVALID_ARG, w + ": the normal feature without a normal buffer");
    if ((prm->features & CRT_REGRESS_ALBEDO) && !in->albedo) return fail(CRT_ERR_INVALID_ARG, w + ": the albedo feature without an albedo buffer");
    if ((prm->features & CRT_REGRESS_DEPTH) && !in->depth) return fail(CRT_ERR_INVALID_ARG, w + ": the depth feature without a depth buffer");
    if (!out_mean && !out_rgb) return fail(CRT_ERR_INVALID_ARG, w + ": no output buffer");
    return size_supported(w, prm->width, prm->height, kNlmTileW, kNlmTileH);
}

int regress_impl(const char* who, int device, const crt_regress_params* prm, const crt_regress_inputs* in, void* d_out_mean, void* d_out_rgb, void* d_scratch,
                 uint64_t scratch_bytes, hipStream_t st, crt_regress_info* info)
{
    const std::string w(who);
    int rc = regress_check(who, prm, in, d_out_mean, d_out_rgb);
    if (rc == CRT_OK) rc = scratch_ok(w, d_scratch, scratch_bytes, scratch_bytes_of(prm->width, prm->height), "crt_denoise_regress_scratch_bytes");
    if (rc != CRT_OK) return rc;
    unsigned long long n = 0;
    rc = timed_launch(w, device, st, info, &n, 1, [&](unsigned long long* d_count) {
        const uint64_t npix = (uint64_t)prm->width * prm->height;
        float4* plane = (float4*)d_scratch;
        RegPack K;
        std::memset(&K, 0, sizeof(K));
        K.n.width = prm->width; K.n.height = prm->height;
        K.n.color = in->weight_color ? in->weight_color : in->color;
        K.n.variance = in->weight_variance ? in->weight_variance : in->variance;
        K.n.normal = (prm->features & CRT_REGRESS_NORMAL) ? in->normal : nullptr;
        K.n.albedo = (prm->features & CRT_REGRESS_ALBEDO) ? in->albedo : nullptr;
        K.n.depth = (prm->features & CRT_REGRESS_DEPTH) ? in->depth : nullptr;
        K.n.c = plane; K.n.g0 = plane + npix; K.n.g1 = plane + 2 * npix;
        K.color = in->color; K.col = plane + 3 * npix;
        hipLaunchKernelGGL(k_regress_pack, dim3((uint32_t)((npix + 255) / 256)), dim3(256), 0, st, K);
        HIP_CHECK(hipGetLastError());
        RegParams P;
        std::memset(&P, 0, sizeof(P));
        P.n.width = prm->width; P.n.height = prm->height;
        P.n.tiles_x = (prm->width + kNlmTileW - 1) / kNlmTileW;
        P.n.radius = (int)prm->radius; P.n.patch = (int)prm->patch;
        P.n.k2 = prm->k * prm->k; P.n.alpha = prm->alpha;
        P.n.sig2_n = 1.0f; P.n.sig2_a = 1.0f; P.n.sigma_d = 1.0f;
        P.n.c = K.n.c; P.n.g0 = K.n.g0; P.n.g1 = K.n.g1;
        P.n.out_mean = (float*)d_out_mean; P.n.out_rgb = (uint8_t*)d_out_rgb;
        P.col = K.col;
        P.sigma_n = prm->sigma_normal; P.sigma_a = prm->sigma_albedo; P.sigma_d = prm->sigma_depth;
        P.pos_den = prm->sigma_position * (float)prm->radius;
        P.ridge = prm->ridge;
        P.count = d_count;
        launch(prm->features, P, P.n.tiles_x * ((prm->height + kNlmTileH - 1) / kNlmTileH), nlm_lds_bytes(P.n.radius, P.n.patch), st);
    });
    if (rc == CRT_OK && info) info->fallback_pixels = n;
    return rc;
}

} // namespace

extern "C" {

int crt_denoise_regress_defaults(crt_regress_params* prm)
{
    if (!prm) return fail(CRT_ERR_INVALID_ARG, "crt_denoise_regress_defaults: null argument");
    std::memset(prm, 0, sizeof(*prm));
    prm->radius = 5; prm->patch = 1; prm->k = 0.6f;
    prm->alpha = 1.0f;
    prm->sigma_normal = 0.5f; prm->sigma_albedo = 0.1f; prm->sigma_depth = 0.05f;
    prm->sigma_position = 2.0f;
    prm->ridge = 0.4f;
    prm->features = CRT_REGRESS_NORMAL | CRT_REGRESS_ALBEDO | CRT_REGRESS_DEPTH | CRT_REGRESS_POSITION;
    return CRT_OK;
}

int crt_denoise_regress_scratch_bytes(uint32_t width, uint32_t height, uint64_t* bytes)
{
    if (!bytes || width == 0 || height == 0) return fail(CRT_ERR_INVALID_ARG, "crt_denoise_regress_scratch_bytes: bad arguments");
    *bytes = scratch_bytes_of(width, height);
    return CRT_OK;
}

int crt_denoise_regress_device(int device, const crt_regress_params* prm, const crt_regress_inputs* dev_in, void* d_out_mean, void* d_out_rgb, void* d_scratch,
                               uint64_t scratch_bytes, void* stream, crt_regress_info* info)
{
    return regress_impl("crt_denoise_regress_device", device, prm, dev_in, d_out_mean, d_out_rgb, d_scratch, scratch_bytes, (hipStream_t)stream, info);
}

int crt_denoise_regress(int device, const crt_regress_params* prm, const crt_regress_inputs* host_in, float* out_mean, uint8_t* out_rgb, crt_regress_info* info)
{
    const int rc0 = regress_check("crt_denoise_regress", prm, host_in, out_mean, out_rgb);
    if (rc0 != CRT_OK) return rc0;
    const uint64_t npix = (uint64_t)prm->width * prm->height;
    return host_form("crt_denoise_regress", device, [&](HostCopies& c) {
        crt_regress_inputs d{};
        d.color = c.in(host_in->color, npix * 3);
        d.variance = c.in(host_in->variance, npix * 3);
        d.weight_color = c.in(host_in->weight_color, npix * 3);
        d.weight_variance = c.in(host_in->weight_variance, npix * 3);
        d.albedo = c.in(host_in->albedo, npix * 3);
        d.normal = c.in(host_in->normal, npix * 3);
        d.depth = c.in(host_in->depth, npix);
        float* d_mean = c.out(out_mean, npix * 3);
        uint8_t* d_rgb = c.out(out_rgb, npix * 3);
        return regress_impl("crt_denoise_regress_device", device, prm, &d, d_mean, d_rgb, c.scratch<float4>(npix * kPlanes), npix * kPlanes * sizeof(float4), nullptr,
                            info);
    });
}

} // extern "C"
