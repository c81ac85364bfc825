// cudaraytracing_amd/csrc/crt_device_fn.hip -- crt_device_fn (contract: include/crt.h): one named device function per element, for
// value-level parity tests against the oracle.  The deterministic math (crt_detmath.h), the vector helpers and the short divisions
// (crt_device.h), the samplers (crt_trace.h), the per-vertex path formulas (crt_path.h) and the tone map (crt_stages.h) are called as the
// render kernels call them; this file holds no copy of their text.  Records are 32-bit words, floats and integers alike, passed as bits.
#include "crt_internal.h"

#include <cstring>
#include <string>

namespace crtk {

enum {
    FN_SIN = 0, FN_COS, FN_TAN, FN_ASIN, FN_ACOS, FN_ATAN, FN_EXP, FN_LOG, FN_LOG10, FN_UNIFORM, FN_SINCOS, FN_ATAN2, FN_POW,
    FN_DOT3, FN_CROSS3, FN_NORM3, FN_UNIT3, FN_DIV3, FN_MAKE_RAY,
    FN_TO_WORLD, FN_SAMPLE_HEMISPHERE, FN_SAMPLE_LOBE, FN_BOUNCE_DIR,
    FN_COS_TO_NEXT, FN_ROULETTE, FN_PROBE_DIR, FN_PROBE_TERM, FN_INDIRECT_STEP, FN_SEED_DIRECT, FN_SEED_EMITTER,
    FN_TONEMAP, FN_COUNT_
};
#define DEVICE_FN_MAX_IN 17
#define DEVICE_FN_MAX_OUT 6
struct DeviceFnRow {
    const char* name;
    uint32_t in_words, out_words;
};
// (in the order of the enum)
static const DeviceFnRow kDeviceFns[FN_COUNT_] = {
    {"sin", 1, 1}, {"cos", 1, 1}, {"tan", 1, 1}, {"asin", 1, 1}, {"acos", 1, 1}, {"atan", 1, 1}, {"exp", 1, 1}, {"log", 1, 1}, {"log10", 1, 1},
    {"uniform", 1, 1}, {"sincos", 1, 2}, {"atan2", 2, 1}, {"pow", 2, 1},
    {"dot3", 6, 1}, {"cross3", 6, 3}, {"norm3", 3, 1}, {"unit3", 3, 3}, {"div3", 4, 3}, {"make_ray", 3, 6},
    {"to_world", 6, 3}, {"sample_hemisphere", 5, 3}, {"sample_lobe", 7, 3}, {"bounce_dir", 5, 3},
    {"cos_to_next", 9, 1}, {"roulette", 6, 5}, {"probe_dir", 12, 3}, {"probe_term", 17, 3}, {"indirect_step", 11, 3}, {"seed_direct", 3, 3},
    {"seed_emitter", 4, 3},
    {"tonemap", 1, 1},
};

// Element i = thread i of a launch with 256-thread blocks: lane i % 64 of wave i / 64 (the wave-uniform branches of quot3_exact see the
// elements [64 w, 64 w + 64) together).  `fn` is the same in every thread.
__global__ __launch_bounds__(256) void k_device_fn(const int fn, const uint32_t n, const uint32_t* __restrict__ in, const uint32_t in_words,
                                                   uint32_t* __restrict__ out, const uint32_t out_words)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t w[DEVICE_FN_MAX_IN];
#pragma unroll
    for (uint32_t k = 0; k < DEVICE_FN_MAX_IN; k++) w[k] = k < in_words ? in[(size_t)i * in_words + k] : 0u;
    auto F = [&](const int k) { return __uint_as_float(w[k]); };
    auto V = [&](const int k) { return f3(__uint_as_float(w[k]), __uint_as_float(w[k + 1]), __uint_as_float(w[k + 2])); };
    uint32_t o[DEVICE_FN_MAX_OUT] = {0u, 0u, 0u, 0u, 0u, 0u};
    auto put1 = [&](const float v) { o[0] = __float_as_uint(v); };
    auto put3 = [&](const F3 v) { o[0] = __float_as_uint(v.x); o[1] = __float_as_uint(v.y); o[2] = __float_as_uint(v.z); };
    switch (fn) {
    case FN_SIN: put1(det_sinf(F(0))); break;
    case FN_COS: put1(det_cosf(F(0))); break;
    case FN_TAN: put1(det_tanf(F(0))); break;
    case FN_ASIN: put1(det_asinf(F(0))); break;
    case FN_ACOS: put1(det_acosf(F(0))); break;
    case FN_ATAN: put1(det_atanf(F(0))); break;
    case FN_EXP: put1(det_expf(F(0))); break;
    case FN_LOG: put1(det_logf(F(0))); break;
    case FN_LOG10: put1(det_log10f(F(0))); break;
    case FN_UNIFORM: put1(rng_uniform(w[0])); break;
    case FN_SINCOS: {
        float s, c;
        det_sincosf(F(0), &s, &c);
        o[0] = __float_as_uint(s); o[1] = __float_as_uint(c);
        break;
    }
    case FN_ATAN2: put1(det_atan2f(F(0), F(1))); break;
    case FN_POW: put1(det_powf(F(0), F(1))); break;
    case FN_DOT3: put1(dot3(V(0), V(3))); break;
    case FN_CROSS3: put3(cross3(V(0), V(3))); break;
    case FN_NORM3: put1(norm3(V(0))); break;
    case FN_UNIT3: put3(unit3(V(0))); break;
    case FN_DIV3: put3(div3(V(0), F(3))); break;
    case FN_MAKE_RAY: {
        const RayT r = make_ray(f3(0.0f, 0.0f, 0.0f), V(0));
        put3(r.d);
        o[3] = __float_as_uint(r.inv.x); o[4] = __float_as_uint(r.inv.y); o[5] = __float_as_uint(r.inv.z);
        break;
    }
    case FN_TO_WORLD: put3(to_world(V(0), V(3))); break;
    case FN_SAMPLE_HEMISPHERE: put3(sample_hemisphere(V(0), rng_uniform(w[3]), rng_uniform(w[4]))); break;
    case FN_SAMPLE_LOBE: put3(sample_lobe(V(0), F(3), F(4), rng_uniform(w[5]), rng_uniform(w[6]))); break;
    case FN_BOUNCE_DIR: {
        U4 rb;
        rb.x = 0u; rb.y = w[3]; rb.z = w[4]; rb.w = 0u;
        put3(bounce_dir(V(0), rb));
        break;
    }
    case FN_COS_TO_NEXT: put1(cos_to_next(V(0), V(3), V(6))); break;
    case FN_ROULETTE: {
        U4 rb;
        const bool stop = roulette((uint64_t)w[0] | ((uint64_t)w[1] << 32), w[2], w[3], w[4], F(5), rb);
        o[0] = stop ? 1u : 0u; o[1] = rb.x; o[2] = rb.y; o[3] = rb.z; o[4] = rb.w;
        break;
    }
    case FN_PROBE_DIR: put3(probe_dir((uint64_t)w[0] | ((uint64_t)w[1] << 32), w[2], w[3], w[4], F(5), V(6), V(9))); break;
    case FN_PROBE_TERM: put3(probe_term(V(0), V(3), V(6), V(9), V(12), F(15), F(16))); break;
    case FN_INDIRECT_STEP: put3(indirect_step(V(0), V(3), F(6), F(7), V(8))); break;
    case FN_SEED_DIRECT: put3(seed_direct(V(0))); break;
    case FN_SEED_EMITTER: put3(seed_emitter((int)w[0], V(1))); break;
    case FN_TONEMAP: o[0] = tonemap(F(0)); break;
    default: break;
    }
#pragma unroll
    for (uint32_t k = 0; k < DEVICE_FN_MAX_OUT; k++)
        if (k < out_words) out[(size_t)i * out_words + k] = o[k];
}

} // namespace crtk

using namespace crtk;

extern "C" int crt_device_fn(int device, const char* name, uint32_t n, const uint32_t* in, uint32_t in_words, uint32_t* out, uint32_t out_words)
{
    if (!name || !in || !out) return fail(CRT_ERR_INVALID_ARG, "crt_device_fn: null argument");
    int id = -1;
    for (int i = 0; i < FN_COUNT_; i++)
        if (std::strcmp(name, kDeviceFns[i].name) == 0) id = i;
    if (id < 0) return fail(CRT_ERR_INVALID_ARG, std::string("crt_device_fn: unknown function ") + name);
    const DeviceFnRow& row = kDeviceFns[id];
    static_assert(DEVICE_FN_MAX_IN == 17 && DEVICE_FN_MAX_OUT == 6, "the widest records of the table");
    if (in_words != row.in_words || out_words != row.out_words)
        return fail(CRT_ERR_INVALID_ARG, std::string("crt_device_fn: ") + name + " takes " + std::to_string(row.in_words) + " words per element and gives " +
                                             std::to_string(row.out_words));
    if (device < 0) return fail(CRT_ERR_INVALID_ARG, "crt_device_fn: device index out of range");
    if (n == 0) return CRT_OK;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(device));
        DevBuf<uint32_t> din, dout;
        din.upload(in, (size_t)n * in_words);
        dout.alloc((size_t)n * out_words);
        hipLaunchKernelGGL(k_device_fn, dim3((n + 255u) / 256u), dim3(256), 0, 0, id, n, (const uint32_t*)din.p, in_words, dout.p, out_words);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        dout.download(out, (size_t)n * out_words);
        return CRT_OK;
    });
}
