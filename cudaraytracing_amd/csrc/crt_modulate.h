// cudaraytracing_amd/csrc/crt_modulate.h -- the kernels of crt_demodulate / crt_modulate (contract: include/crt.h; host code:
// crt_modulate.hip): an image divided by its albedo after its emission is taken off, and the way back with the frame's tone map.
// Both operations are per component, so the kernels run over the flat 3 x width x height floats: a thread takes a quad of four
// consecutive components, a wave 64 consecutive quads (1 KiB per buffer and access), with 16-byte loads and stores and ONE 4-byte store
// for the quad's RGB8 bytes.  The quad that the image's end cuts short, and every quad when a base pointer is not 16-byte aligned
// (out_rgb: 4-byte), goes component by component through the same arithmetic.  No LDS, no atomics; the grid is capped and strides.
// Like crt_stages.h this file includes nothing, so that tools/modulate_host_check.cpp can compile this very text for the host behind
// stand-ins for what it takes from outside: float4 / make_float4, tonemap (crt_stages.h), blockIdx / threadIdx / gridDim.
#ifndef CRT_MODULATE_H
#define CRT_MODULATE_H

namespace crtk {

struct DemodParams {
    uint64_t n;                  // components: 3 x width x height
    float floor;                 // albedo_floor
    uint32_t vec;                // every buffer given is 16-byte aligned: whole quads take the 16-byte path
    const float* color;
    const float* albedo;
    const float* emission;       // may be null
    const float* variance;       // null together with out_variance
    float* out;                  // the irradiance
    float* out_variance;
};
struct ModParams {
    uint64_t n;
    float floor;
    uint32_t vec;                // as DemodParams'; out_rgb 4-byte aligned
    const float* irradiance;
    const float* albedo;
    const float* emission;       // may be null
    float* out_mean;             // either may be null
    uint8_t* out_rgb;
};

// the contract's lines, one IEEE operation per symbol; has_e: an emission buffer was given
__device__ __forceinline__ float demodulate_value(const float c, const float a, const float e, const bool has_e, const float floor)
{
    const float d = has_e ? c - e : c;
    return a > floor ? d / a : d;
}
__device__ __forceinline__ float demodulate_variance(const float v, const float a, const float floor) { return a > floor ? v / (a * a) : v; }
__device__ __forceinline__ float modulate_value(const float i, const float a, const float e, const bool has_e, const float floor)
{
    const float m = a > floor ? i * a : i;
    return has_e ? m + e : m;
}

__device__ __forceinline__ float4 load_quad(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void store_quad(float* p, const float4 v) { *reinterpret_cast<float4*>(p) = v; }

// A launch's quads are strided over its grid: quad q has k components (4, or what the image's end leaves of the last one).
__global__ __launch_bounds__(256) void k_demodulate(const DemodParams P)
{
    const bool has_e = P.emission != nullptr;
    const uint64_t quads = (P.n + 3u) / 4u, stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < quads; q += stride) {
        const uint64_t i0 = q * 4u;
        const uint32_t k = P.n - i0 < 4u ? (uint32_t)(P.n - i0) : 4u;
        if (P.vec && k == 4u) {
            const float4 c = load_quad(P.color + i0), a = load_quad(P.albedo + i0);
            const float4 e = has_e ? load_quad(P.emission + i0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (P.variance) v = load_quad(P.variance + i0);
            store_quad(P.out + i0, make_float4(demodulate_value(c.x, a.x, e.x, has_e, P.floor), demodulate_value(c.y, a.y, e.y, has_e, P.floor),
                                               demodulate_value(c.z, a.z, e.z, has_e, P.floor), demodulate_value(c.w, a.w, e.w, has_e, P.floor)));
            if (P.variance)
                store_quad(P.out_variance + i0, make_float4(demodulate_variance(v.x, a.x, P.floor), demodulate_variance(v.y, a.y, P.floor),
                                                            demodulate_variance(v.z, a.z, P.floor), demodulate_variance(v.w, a.w, P.floor)));
        } else {
            for (uint64_t i = i0; i < i0 + k; i++) {
                const float a = P.albedo[i];
                P.out[i] = demodulate_value(P.color[i], a, has_e ? P.emission[i] : 0.0f, has_e, P.floor);
                if (P.variance) P.out_variance[i] = demodulate_variance(P.variance[i], a, P.floor);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_modulate(const ModParams P)
{
    const bool has_e = P.emission != nullptr;
    const uint64_t quads = (P.n + 3u) / 4u, stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < quads; q += stride) {
        const uint64_t i0 = q * 4u;
        const uint32_t k = P.n - i0 < 4u ? (uint32_t)(P.n - i0) : 4u;
        if (P.vec && k == 4u) {
            const float4 r = load_quad(P.irradiance + i0), a = load_quad(P.albedo + i0);
            const float4 e = has_e ? load_quad(P.emission + i0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const float4 c = make_float4(modulate_value(r.x, a.x, e.x, has_e, P.floor), modulate_value(r.y, a.y, e.y, has_e, P.floor),
                                         modulate_value(r.z, a.z, e.z, has_e, P.floor), modulate_value(r.w, a.w, e.w, has_e, P.floor));
            if (P.out_mean) store_quad(P.out_mean + i0, c);
            if (P.out_rgb) // bytes i0 .. i0 + 3 in memory order
                *reinterpret_cast<uint32_t*>(P.out_rgb + i0) =
                    (uint32_t)tonemap(c.x) | ((uint32_t)tonemap(c.y) << 8) | ((uint32_t)tonemap(c.z) << 16) | ((uint32_t)tonemap(c.w) << 24);
        } else {
            for (uint64_t i = i0; i < i0 + k; i++) {
                const float c = modulate_value(P.irradiance[i], P.albedo[i], has_e ? P.emission[i] : 0.0f, has_e, P.floor);
                if (P.out_mean) P.out_mean[i] = c;
                if (P.out_rgb) P.out_rgb[i] = tonemap(c);
            }
        }
    }
}

// One thread per quad up to kModulateMaxBlocks blocks of 256; beyond that the grid strides.  max_blocks: a smaller cap (the host check
// drives the stride loop with it).
const uint32_t kModulateMaxBlocks = 2048;
inline uint32_t modulate_blocks(const uint64_t n, const uint32_t max_blocks)
{
    const uint64_t blocks = ((n + 3u) / 4u + 255u) / 256u;
    return (uint32_t)(blocks < max_blocks ? blocks : max_blocks);
}
inline void launch_demodulate(const DemodParams& P, hipStream_t st, const uint32_t max_blocks = kModulateMaxBlocks)
{
    hipLaunchKernelGGL(k_demodulate, dim3(modulate_blocks(P.n, max_blocks)), dim3(256), 0, st, P);
}
inline void launch_modulate(const ModParams& P, hipStream_t st, const uint32_t max_blocks = kModulateMaxBlocks)
{
    hipLaunchKernelGGL(k_modulate, dim3(modulate_blocks(P.n, max_blocks)), dim3(256), 0, st, P);
}

} // namespace crtk
#endif
