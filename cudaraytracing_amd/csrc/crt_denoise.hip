// cudaraytracing_amd/csrc/crt_denoise.hip -- the AOV-guided edge-avoiding a-trous filter (crt_denoise / crt_denoise_device, contract:
// include/crt.h) and its variance-guided form (crt_denoise_var / crt_denoise_var_device): kernels and host code.  An image operation without a scene handle.
// The two forms are one pack kernel, one templated pass body (its two instantiations keep their kernel names) and one host path.
//
// One call = k_denoise_pack (colour and guides into four float4 planes of the caller's scratch: a colour ping-pong pair, (normal.xyz,
// depth) and (albedo.xyz, 0) -- three 16-byte loads per tap, coalesced along a row whatever the spacing) and one filter launch per pass.
// A pass is one thread per pixel, 25 taps in the contract's order, every tap read from global memory through the caches; the last pass
// writes out_mean and the tone-mapped RGB8 itself.  (A form that staged the tile and its halo in LDS for spacing 1 and 2 was measured and
// dropped: the pass is bound by vector-ALU issue, not by its loads -- docs/experiments.md, "The a-trous denoiser".)
#include "crt_filter_host.h"

#include <cstring>
#include <limits>
#include <string>

namespace crtk {

struct DnParams {
    uint32_t width, height, tiles_x;
    float sig2_c, sig2_n, sig2_a, sigma_d;   // sig * sig of the pass, sigma_normal^2, sigma_albedo^2 (1 for a NULL guide: 0 / 1 = +0), sigma_depth
    const float4* c_in;                       // c_i: (r, g, b, -)
    const float4* g0;                         // (normal.xyz, depth); zeros for NULL guides
    const float4* g1;                         // (albedo.xyz, 0)
    float4* c_out;                            // c_{i+1}; not written by the last pass
    float* out_mean;                          // last pass only (either may be null)
    uint8_t* out_rgb;
    uint32_t last;
};

struct DnPack {
    uint64_t npix;
    const float* color; const float* albedo; const float* normal; const float* depth;
    const float* variance;                    // crt_denoise_var; null: the plain form, .w of the colour plane 0
    float4* c0; float4* g0; float4* g1;
};

__global__ __launch_bounds__(256) void k_denoise_pack(const DnPack K)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= K.npix) return;
    const float v0 = K.variance ? (K.variance[p * 3] + K.variance[p * 3 + 1]) + K.variance[p * 3 + 2] : 0.0f;
    K.c0[p] = make_float4(K.color[p * 3], K.color[p * 3 + 1], K.color[p * 3 + 2], v0);
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f), a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (K.normal) { g.x = K.normal[p * 3]; g.y = K.normal[p * 3 + 1]; g.z = K.normal[p * 3 + 2]; }
    if (K.depth) g.w = K.depth[p];
    if (K.albedo) { a.x = K.albedo[p * 3]; a.y = K.albedo[p * 3 + 1]; a.z = K.albedo[p * 3 + 2]; }
    K.g0[p] = g;
    K.g1[p] = a;
}

struct DnSum { float x, y, z, den, vnum; };

// one tap of the contract (include/crt.h), operation by operation; hw = h[dy+2] * h[dx+2]; n_c: the divisor of the colour term (the
// pass's sigma^2, or the variance-guided form's sigma^2 g(p) + 1e-10); VAR: also the variance's numerator
template <bool VAR>
__device__ __forceinline__ void dn_tap(const DnParams& P, const float n_c, const float4 cp, const float4 gp, const float4 ap, const float4 cq,
                                       const float4 gq, const float4 aq, const float hw, DnSum& s)
{
    const float dcx = cp.x - cq.x, dcy = cp.y - cq.y, dcz = cp.z - cq.z;
    const float e_c = (dcx * dcx + dcy * dcy + dcz * dcz) / n_c;
    const float dnx = gp.x - gq.x, dny = gp.y - gq.y, dnz = gp.z - gq.z;
    const float e_n = (dnx * dnx + dny * dny + dnz * dnz) / P.sig2_n;
    const float dax = ap.x - aq.x, day = ap.y - aq.y, daz = ap.z - aq.z;
    const float e_a = (dax * dax + day * day + daz * daz) / P.sig2_a;
    const float m = gp.w > gq.w ? gp.w : gq.w;
    const float r = (gp.w - gq.w) / (P.sigma_d * m);
    const float e_d = m > 0.0f ? r * r : 0.0f;
    const float w = hw * det_expf(-(((e_c + e_n) + e_a) + e_d));
    s.x = s.x + cq.x * w;
    s.y = s.y + cq.y * w;
    s.z = s.z + cq.z * w;
    s.den = s.den + w;
    if (VAR) s.vnum = s.vnum + cq.w * (w * w);
}

__device__ __forceinline__ float dn_h(const int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }
__device__ __forceinline__ float dn_k(const int d) { return d == 0 ? 0.5f : 0.25f; }

// A pass of either form.  Block = 64 x 4 pixels, a wave = 64 consecutive pixels of one row.
// VAR (crt_denoise_var, contract: include/crt.h): the same planes; the scalar variance v_i rides in the .w of the colour ping-pong pair.
// A pass adds, per pixel, nine 4-byte loads for g(p) (the .w of the pixels around p: lines the spacing-1 taps touch anyway) and a
// multiply-add pair per tap; P.sig2_c = sigma_color * sigma_color (the same in every pass); out_var: v_iterations of the last pass (may be
// null).  No LDS staging in either form: the pass sits at the vector-ALU issue rate (docs/experiments.md, "The variance-guided filter").
template <bool VAR> __device__ __forceinline__ void denoise_pass(const DnParams& P, const int step, float* const out_var)
{
    const uint32_t by = blockIdx.x / P.tiles_x, bx = blockIdx.x - by * P.tiles_x;
    const int x = (int)(bx * 64u + (threadIdx.x & 63u)), y = (int)(by * 4u + (threadIdx.x >> 6));
    const int W = (int)P.width, H = (int)P.height;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * P.width + (size_t)x;
    float n_c = P.sig2_c;
    if (VAR) { // g(p): the 3x3 Gaussian of v_i at spacing 1, whatever the spacing of the pass
        float gn = 0.0f, gd = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
            const int ty = y + dy;
            if (ty < 0 || ty >= H) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int tx = x + dx;
                if (tx < 0 || tx >= W) continue;
                const float k = dn_k(dy) * dn_k(dx);
                gn = gn + k * P.c_in[(size_t)ty * P.width + (size_t)tx].w;
                gd = gd + k;
            }
        }
        n_c = P.sig2_c * (gn / gd) + 1e-10f;
    }
    const float4 cp = P.c_in[p], gp = P.g0[p], ap = P.g1[p];
    DnSum s = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * step;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * step;
            if (qx < 0 || qx >= W) continue;
            const size_t q = (size_t)qy * P.width + (size_t)qx;
            dn_tap<VAR>(P, n_c, cp, gp, ap, P.c_in[q], P.g0[q], P.g1[q], dn_h(dy) * dn_h(dx), s);
        }
    }
    const F3 c = f3(s.x / s.den, s.y / s.den, s.z / s.den);
    const float v = VAR ? s.vnum / (s.den * s.den) : 0.0f;
    if (!P.last) { P.c_out[p] = make_float4(c.x, c.y, c.z, v); return; }
    write_color(P, p, true, c);
    if (VAR && out_var) out_var[p] = v;
}

// (the two kernel names are what the docs and profiler traces cite)
__global__ __launch_bounds__(256) void k_denoise_pass(const DnParams P, const int step) { denoise_pass<false>(P, step, nullptr); }
__global__ __launch_bounds__(256) void k_denoise_var_pass(const DnParams P, const int step, float* const out_var) { denoise_pass<true>(P, step, out_var); }

} // namespace crtk

using namespace crtk;

namespace {

// Argument checks of both forms, before any device call
int denoise_check(const char* who, const crt_denoise_params* prm, const crt_denoise_inputs* in, const void* out_mean, const void* out_rgb)
{
    const std::string w(who);
    if (!prm || !in) return fail(CRT_ERR_INVALID_ARG, w + ": null argument");
    if (!in->color) return fail(CRT_ERR_INVALID_ARG, w + ": null colour buffer");
    if (const int rc = size_positive(w, prm->width, prm->height)) return rc;
    if (prm->iterations < 1 || prm->iterations > 5) return fail(CRT_ERR_INVALID_ARG, w + ": iterations must be 1 .. 5");
    if (!sigma_ok(prm->sigma_color) || !sigma_ok(prm->sigma_normal) || !sigma_ok(prm->sigma_albedo) || !sigma_ok(prm->sigma_depth))
        return fail(CRT_ERR_INVALID_ARG, w + ": every sigma must be > 0 (+inf switches a term off)");
    if (!out_mean && !out_rgb) return fail(CRT_ERR_INVALID_ARG, w + ": no output buffer");
    return size_supported(w, prm->width, prm->height, 64, 4);
}

uint64_t scratch_bytes_of(uint32_t width, uint32_t height) { return (uint64_t)width * height * 4u * sizeof(float4); }

// The extra checks of the variance-guided form (after denoise_check on the fields the two forms share)
int denoise_var_check(const char* who, const crt_denoise_params* prm, const crt_denoise_var_inputs* in, const void* out_mean, const void* out_rgb)
{
    const std::string w(who);
    if (!prm || !in) return fail(CRT_ERR_INVALID_ARG, w + ": null argument");
    const crt_denoise_inputs plain = {in->color, in->albedo, in->normal, in->depth};
    const int rc = denoise_check(who, prm, &plain, out_mean, out_rgb);
    if (rc != CRT_OK) return rc;
    if (!in->variance) return fail(CRT_ERR_INVALID_ARG, w + ": null variance buffer");
    if (!(prm->sigma_color < std::numeric_limits<float>::infinity()))
        return fail(CRT_ERR_INVALID_ARG, w + ": sigma_color must be finite (inf x a variance of 0 is NaN; crt_denoise drops the colour term)");
    return CRT_OK;
}

// Both forms of the filter on device buffers: d_variance == nullptr is crt_denoise_device (the caller has checked the arguments that
// the two forms do not share); otherwise the variance-guided passes, d_out_var optional.
int denoise_impl(const char* who, int device, const crt_denoise_params* prm, const crt_denoise_inputs* in, const float* d_variance, void* d_out_mean,
                 void* d_out_rgb, float* d_out_var, void* d_scratch, uint64_t scratch_bytes, hipStream_t st, crt_denoise_info* info)
{
    const std::string w(who);
    int rc = denoise_check(who, prm, in, d_out_mean, d_out_rgb);
    if (rc == CRT_OK) rc = scratch_ok(w, d_scratch, scratch_bytes, scratch_bytes_of(prm->width, prm->height), "crt_denoise_scratch_bytes");
    if (rc != CRT_OK) return rc;
    rc = timed_launch(w, device, st, info, [&] {
        const uint64_t npix = (uint64_t)prm->width * prm->height;
        float4* plane = (float4*)d_scratch;
        float4* c[2] = {plane, plane + npix};
        DnPack K;
        K.npix = npix;
        K.color = in->color; K.albedo = in->albedo; K.normal = in->normal; K.depth = in->depth;
        K.variance = d_variance;
        K.c0 = c[0]; K.g0 = plane + 2 * npix; K.g1 = plane + 3 * npix;
        hipLaunchKernelGGL(k_denoise_pack, dim3((uint32_t)((npix + 255) / 256)), dim3(256), 0, st, K);
        HIP_CHECK(hipGetLastError());
        DnParams P;
        std::memset(&P, 0, sizeof(P));
        P.width = prm->width; P.height = prm->height;
        P.sig2_n = in->normal ? prm->sigma_normal * prm->sigma_normal : 1.0f;
        P.sig2_a = in->albedo ? prm->sigma_albedo * prm->sigma_albedo : 1.0f;
        P.sigma_d = prm->sigma_depth;
        P.g0 = K.g0; P.g1 = K.g1;
        P.tiles_x = (prm->width + 63) / 64;
        for (uint32_t i = 0; i < prm->iterations; i++) {
            const float sig = prm->sigma_color / (float)(1 << i);
            P.sig2_c = sig * sig;
            P.c_in = c[i & 1]; P.c_out = c[(i + 1) & 1];
            P.last = i + 1 == prm->iterations;
            P.out_mean = P.last ? (float*)d_out_mean : nullptr;
            P.out_rgb = P.last ? (uint8_t*)d_out_rgb : nullptr;
            if (d_variance) {
                P.sig2_c = prm->sigma_color * prm->sigma_color; // (no halving per pass: the filtered variance shrinks instead)
                hipLaunchKernelGGL(k_denoise_var_pass, dim3(P.tiles_x * ((prm->height + 3) / 4)), dim3(256), 0, st, P, 1 << i, P.last ? d_out_var : (float*)nullptr);
            } else {
                hipLaunchKernelGGL(k_denoise_pass, dim3(P.tiles_x * ((prm->height + 3) / 4)), dim3(256), 0, st, P, 1 << i);
            }
            HIP_CHECK(hipGetLastError());
        }
    });
    if (rc == CRT_OK && info) info->passes = prm->iterations;
    return rc;
}

// The host-buffer form of either filter (the caller has checked the arguments): device copies of the inputs, denoise_impl under the
// name `who_device`, then the copies back.  variance / out_variance: crt_denoise_var's, null for crt_denoise.
int denoise_host(const char* who, const char* who_device, int device, const crt_denoise_params* prm, const crt_denoise_inputs* host_in, const float* variance,
                 float* out_mean, uint8_t* out_rgb, float* out_variance, crt_denoise_info* info)
{
    const uint64_t npix = (uint64_t)prm->width * prm->height;
    return host_form(who, device, [&](HostCopies& c) {
        crt_denoise_inputs d{};
        d.color = c.in(host_in->color, npix * 3);
        const float* d_var = c.in(variance, npix * 3);
        d.albedo = c.in(host_in->albedo, npix * 3);
        d.normal = c.in(host_in->normal, npix * 3);
        d.depth = c.in(host_in->depth, npix);
        float* d_mean = c.out(out_mean, npix * 3);
        uint8_t* d_rgb = c.out(out_rgb, npix * 3);
        float* d_ovar = c.out(out_variance, npix);
        return denoise_impl(who_device, device, prm, &d, d_var, d_mean, d_rgb, d_ovar, c.scratch<float4>(npix * 4), npix * 4 * sizeof(float4), nullptr, info);
    });
}

} // namespace

extern "C" {

int crt_denoise_defaults(crt_denoise_params* prm)
{
    if (!prm) return fail(CRT_ERR_INVALID_ARG, "crt_denoise_defaults: null argument");
    std::memset(prm, 0, sizeof(*prm));
    prm->iterations = 3;
    prm->sigma_color = 4.0f; prm->sigma_normal = 0.5f; prm->sigma_albedo = 0.1f; prm->sigma_depth = 0.05f;
    return CRT_OK;
}

int crt_denoise_scratch_bytes(uint32_t width, uint32_t height, uint64_t* bytes)
{
    if (!bytes || width == 0 || height == 0) return fail(CRT_ERR_INVALID_ARG, "crt_denoise_scratch_bytes: bad arguments");
    *bytes = scratch_bytes_of(width, height);
    return CRT_OK;
}

int crt_denoise_device(int device, const crt_denoise_params* prm, const crt_denoise_inputs* dev_in, void* d_out_mean, void* d_out_rgb,
                       void* d_scratch, uint64_t scratch_bytes, void* stream, crt_denoise_info* info)
{
    return denoise_impl("crt_denoise_device", device, prm, dev_in, nullptr, d_out_mean, d_out_rgb, nullptr, d_scratch, scratch_bytes, (hipStream_t)stream, info);
}

int crt_denoise(int device, const crt_denoise_params* prm, const crt_denoise_inputs* host_in, float* out_mean, uint8_t* out_rgb,
                crt_denoise_info* info)
{
    const int rc0 = denoise_check("crt_denoise", prm, host_in, out_mean, out_rgb);
    if (rc0 != CRT_OK) return rc0;
    return denoise_host("crt_denoise", "crt_denoise_device", device, prm, host_in, nullptr, out_mean, out_rgb, nullptr, info);
}

int crt_denoise_var_defaults(crt_denoise_params* prm)
{
    if (!prm) return fail(CRT_ERR_INVALID_ARG, "crt_denoise_var_defaults: null argument");
    std::memset(prm, 0, sizeof(*prm));
    prm->iterations = 3;
    prm->sigma_color = 6.0f; prm->sigma_normal = 0.5f; prm->sigma_albedo = 0.1f; prm->sigma_depth = 0.05f;
    return CRT_OK;
}

int crt_denoise_var_device(int device, const crt_denoise_params* prm, const crt_denoise_var_inputs* dev_in, void* d_out_mean, void* d_out_rgb,
                           void* d_out_variance, void* d_scratch, uint64_t scratch_bytes, void* stream, crt_denoise_info* info)
{
    const int rc = denoise_var_check("crt_denoise_var_device", prm, dev_in, d_out_mean, d_out_rgb);
    if (rc != CRT_OK) return rc;
    const crt_denoise_inputs plain = {dev_in->color, dev_in->albedo, dev_in->normal, dev_in->depth};
    return denoise_impl("crt_denoise_var_device", device, prm, &plain, dev_in->variance, d_out_mean, d_out_rgb, (float*)d_out_variance, d_scratch,
                        scratch_bytes, (hipStream_t)stream, info);
}

int crt_denoise_var(int device, const crt_denoise_params* prm, const crt_denoise_var_inputs* host_in, float* out_mean, uint8_t* out_rgb,
                    float* out_variance, crt_denoise_info* info)
{
    const int rc0 = denoise_var_check("crt_denoise_var", prm, host_in, out_mean, out_rgb);
    if (rc0 != CRT_OK) return rc0;
    const crt_denoise_inputs plain = {host_in->color, host_in->albedo, host_in->normal, host_in->depth};
    return denoise_host("crt_denoise_var", "crt_denoise_var_device", device, prm, &plain, host_in->variance, out_mean, out_rgb, out_variance, info);
}

} // extern "C"
