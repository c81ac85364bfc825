// cudaraytracing_amd/csrc/crt_modulate.hip -- crt_demodulate / crt_modulate (contract: include/crt.h): the host side of the two image
// operations that take a frame from radiance to irradiance and back, so that the denoiser and the temporal pass can filter what does
// not carry the surfaces' albedo or the lights.  Image operations without a scene handle and without scratch, like the denoiser.
// The kernels are in crt_modulate.h, in a form the host can compile as well (tools/modulate_host_check.cpp).
#include "crt_filter_host.h"
#include "crt_modulate.h"

#include <cstring>
#include <string>

using namespace crtk;

namespace {

// What both operations and both forms check, before any device call
int modulate_check(const std::string& w, const crt_modulate_params* prm, const void* image, const void* albedo)
{
    if (!prm) return fail(CRT_ERR_INVALID_ARG, w + ": null argument");
    if (!image || !albedo) return fail(CRT_ERR_INVALID_ARG, w + ": null image or albedo buffer");
    if (const int rc = size_positive(w, prm->width, prm->height)) return rc;
    if (!(prm->albedo_floor >= 0.0f)) return fail(CRT_ERR_INVALID_ARG, w + ": albedo_floor must be >= 0 and not NaN");
    return sides_supported(w, prm->width, prm->height); // (a flat launch over the floats: no tile count to bound)
}
int demodulate_check(const char* who, const crt_modulate_params* prm, const void* color, const void* albedo, const void* variance, const void* out,
                     const void* out_variance)
{
    const std::string w(who);
    const int rc = modulate_check(w, prm, color, albedo);
    if (rc != CRT_OK) return rc;
    if (!out) return fail(CRT_ERR_INVALID_ARG, w + ": null output buffer");
    if ((variance != nullptr) != (out_variance != nullptr)) return fail(CRT_ERR_INVALID_ARG, w + ": variance and out_variance go together");
    return CRT_OK;
}
int remodulate_check(const char* who, const crt_modulate_params* prm, const void* irradiance, const void* albedo, const void* out_mean, const void* out_rgb)
{
    const std::string w(who);
    const int rc = modulate_check(w, prm, irradiance, albedo);
    if (rc != CRT_OK) return rc;
    if (!out_mean && !out_rgb) return fail(CRT_ERR_INVALID_ARG, w + ": no output buffer");
    return CRT_OK;
}

bool aligned16(const void* p) { return (uintptr_t)p % 16u == 0; } // (a null pointer is)

int demodulate_impl(int device, const crt_modulate_params* prm, const float* color, const float* albedo, const float* emission, const float* variance,
                    float* out, float* out_variance, hipStream_t st, crt_modulate_info* info)
{
    DemodParams P;
    std::memset(&P, 0, sizeof(P));
    P.n = (uint64_t)prm->width * prm->height * 3u;
    P.floor = prm->albedo_floor;
    P.color = color; P.albedo = albedo; P.emission = emission; P.variance = variance; P.out = out; P.out_variance = out_variance;
    P.vec = aligned16(color) && aligned16(albedo) && aligned16(emission) && aligned16(variance) && aligned16(out) && aligned16(out_variance);
    return timed_launch("crt_demodulate_device", device, st, info, [&] { launch_demodulate(P, st); });
}

int modulate_impl(int device, const crt_modulate_params* prm, const float* irradiance, const float* albedo, const float* emission, float* out_mean,
                  uint8_t* out_rgb, hipStream_t st, crt_modulate_info* info)
{
    ModParams P;
    std::memset(&P, 0, sizeof(P));
    P.n = (uint64_t)prm->width * prm->height * 3u;
    P.floor = prm->albedo_floor;
    P.irradiance = irradiance; P.albedo = albedo; P.emission = emission; P.out_mean = out_mean; P.out_rgb = out_rgb;
    P.vec = aligned16(irradiance) && aligned16(albedo) && aligned16(emission) && aligned16(out_mean) && (uintptr_t)out_rgb % 4u == 0;
    return timed_launch("crt_modulate_device", device, st, info, [&] { launch_modulate(P, st); });
}

} // namespace

extern "C" {

int crt_modulate_defaults(crt_modulate_params* prm)
{
    if (!prm) return fail(CRT_ERR_INVALID_ARG, "crt_modulate_defaults: null argument");
    std::memset(prm, 0, sizeof(*prm));
    prm->albedo_floor = 0.0f;
    return CRT_OK;
}

int crt_demodulate_device(int device, const crt_modulate_params* prm, const void* d_color, const void* d_albedo, const void* d_emission,
                          const void* d_variance, void* d_out_irradiance, void* d_out_variance, void* stream, crt_modulate_info* info)
{
    const int rc = demodulate_check("crt_demodulate_device", prm, d_color, d_albedo, d_variance, d_out_irradiance, d_out_variance);
    if (rc != CRT_OK) return rc;
    return demodulate_impl(device, prm, (const float*)d_color, (const float*)d_albedo, (const float*)d_emission, (const float*)d_variance,
                           (float*)d_out_irradiance, (float*)d_out_variance, (hipStream_t)stream, info);
}

int crt_demodulate(int device, const crt_modulate_params* prm, const float* color, const float* albedo, const float* emission, const float* variance,
                   float* out_irradiance, float* out_variance, crt_modulate_info* info)
{
    const int rc0 = demodulate_check("crt_demodulate", prm, color, albedo, variance, out_irradiance, out_variance);
    if (rc0 != CRT_OK) return rc0;
    const uint64_t n = (uint64_t)prm->width * prm->height * 3u;
    return host_form("crt_demodulate", device, [&](HostCopies& c) {
        const float *d_color = c.in(color, n), *d_albedo = c.in(albedo, n), *d_emission = c.in(emission, n), *d_variance = c.in(variance, n);
        return demodulate_impl(device, prm, d_color, d_albedo, d_emission, d_variance, c.out(out_irradiance, n), c.out(out_variance, n), nullptr, info);
    });
}

int crt_modulate_device(int device, const crt_modulate_params* prm, const void* d_irradiance, const void* d_albedo, const void* d_emission,
                        void* d_out_mean, void* d_out_rgb, void* stream, crt_modulate_info* info)
{
    const int rc = remodulate_check("crt_modulate_device", prm, d_irradiance, d_albedo, d_out_mean, d_out_rgb);
    if (rc != CRT_OK) return rc;
    return modulate_impl(device, prm, (const float*)d_irradiance, (const float*)d_albedo, (const float*)d_emission, (float*)d_out_mean, (uint8_t*)d_out_rgb,
                         (hipStream_t)stream, info);
}

int crt_modulate(int device, const crt_modulate_params* prm, const float* irradiance, const float* albedo, const float* emission, float* out_mean,
                 uint8_t* out_rgb, crt_modulate_info* info)
{
    const int rc0 = remodulate_check("crt_modulate", prm, irradiance, albedo, out_mean, out_rgb);
    if (rc0 != CRT_OK) return rc0;
    const uint64_t n = (uint64_t)prm->width * prm->height * 3u;
    return host_form("crt_modulate", device, [&](HostCopies& c) {
        const float *d_irradiance = c.in(irradiance, n), *d_albedo = c.in(albedo, n), *d_emission = c.in(emission, n);
        return modulate_impl(device, prm, d_irradiance, d_albedo, d_emission, c.out(out_mean, n), c.out(out_rgb, n), nullptr, info);
    });
}

} // extern "C"
