// tools/host_device.h -- what the tools/*_host_check.cpp programs put in the device's place, stated once.  Those programs compile kernel
// text of cudaraytracing_amd/csrc (headers that include nothing, crt_sample_map.hip, crt_adaptive.hip) for the HOST and run it against
// plain restatements under AddressSanitizer / UBSan; this header supplies what that text takes from outside: the HIP qualifiers and
// types, the atomics and bit casts, the few definitions of crt_device.h / crt_path.h it uses, and the launch with its indices.
// A program that defines CRT_HOST_WAVES before the include gets a wave of 64 host threads with the cross-lane operations (and needs
// -pthread), an 8-byte __shfl_down and LDS; without it a launch is a plain loop over blocks and threads, for kernels that have no
// cross-lane operation.
// A program that defines CRT_HOST_PATH before the include also gets what kernel text takes from the path code (crt_aov_direct.h, crt_aov_ao.h): the
// remaining vector types and bit casts, F3's other operations, the triangle row's material word, the ray kinds, shadow_blocked and
// bounce_dir with the samplers under it.
//
// Every program builds with one line (tests/host_program.py; the threaded ones add -pthread):
//   g++ -std=c++17 -ffp-contract=off -I cudaraytracing_amd/csrc -O1 -g -fsanitize=address,undefined,float-cast-overflow \
//       -fno-sanitize-recover=all tools/NAME_host_check.cpp -o /tmp/NAME_host_check && /tmp/NAME_host_check
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#ifdef CRT_HOST_WAVES
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>
#endif

#include "crt_detmath.h"
#include "crt_fastdiv.h"

// ---- stand-ins for the device ----
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(n)
#define CRT_TILE 8 // crt_device.h
struct dim3 { uint32_t x; dim3(uint32_t x_ = 1) : x(x_) {} };
typedef void* hipStream_t;
struct alignas(16) float4 { float x, y, z, w; };
static float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_load(p, order, scope) __atomic_load_n(p, order)
#define __hip_atomic_store(p, v, order, scope) __atomic_store_n(p, v, order)
#define __hip_atomic_fetch_add(p, v, order, scope) __atomic_fetch_add(p, v, order)
template <class T> static T __hip_atomic_fetch_max(T* p, T v, int, int) // (a compare-and-swap loop: gcc has no fetch-max)
{
    T seen = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (seen < v && !__atomic_compare_exchange_n(p, &seen, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return seen;
}
#define __builtin_amdgcn_fence(order, scope) __atomic_thread_fence(order) // crt_refit.h: the fences around an arrival
static float __uint_as_float(unsigned int u) { float f; std::memcpy(&f, &u, 4); return f; }
static unsigned int __float_as_uint(float f) { unsigned int u; std::memcpy(&u, &f, 4); return u; }
using std::max;
using std::min;

// ---- what the kernel text takes from crt_device.h / crt_path.h: the same text ----
namespace crtk {
using namespace crtdev; // FastDiv, make_fastdiv, det_powf, det_expf, U4, rng_draw, rng_uniform
// crt_device.h: fast_div (its host branch)
static uint32_t fast_div(uint32_t n, uint32_t m, uint32_t sh)
{
    const uint32_t t = (uint32_t)(((uint64_t)m * n) >> 32);
    return (t + ((n - t) >> (sh & 255u))) >> (sh >> 8);
}
// crt_device.h: F3, f3
struct F3 { float x, y, z; };
static F3 f3(float x, float y, float z) { return F3{x, y, z}; }
// crt_device.h: dot3, unit3 (there the quotient is built from a reciprocal and corrected to the rounded one: the same value)
static float dot3(F3 a, F3 b) { return a.x * b.x + (a.y * b.y + a.z * b.z); }
static F3 unit3(F3 a)
{
    const float z = dot3(a, a);
    if (z > 0.0f) { const float s = sqrt_f(z); return f3(a.x / s, a.y / s, a.z / s); }
    return a;
}
// crt_device.h: maxf_ref, minf_ref
static float maxf_ref(float x, float y) { return x > y ? x : y; }
static float minf_ref(float x, float y) { return x < y ? x : y; }
// crt_path.h: Rad3
struct Rad3 { float x, y, z; };
// crt_path.h: load_radiance (there one 12-byte load of the three floats)
static Rad3 load_radiance(const Rad3* p) { return *p; }
// crt_path.h: slot_to_pixel
static bool slot_to_pixel(uint32_t slot, uint32_t rank, uint32_t world, uint32_t n_tiles, uint32_t tiles_x, FastDiv tiles_x_div, uint32_t width, uint32_t height,
                          uint32_t& i, uint32_t& j)
{
    uint32_t tile = (slot >> 6) * world + rank;
    uint32_t pix = slot & 63u;
    if (tile >= n_tiles) return false;
    uint32_t ty = fast_div(tile, tiles_x_div.m, tiles_x_div.sh), tx = tile - ty * tiles_x;
    i = tx * CRT_TILE + (pix & 7u);
    j = ty * CRT_TILE + (pix >> 3);
    return i < width && j < height;
}
} // namespace crtk

#ifdef CRT_HOST_PATH
#include <cfloat>
struct alignas(8) float2 { float x, y; };
static float2 make_float2(float x, float y) { return float2{x, y}; }
struct alignas(16) uint4 { uint32_t x, y, z, w; };
static int __float_as_int(float f) { int i; std::memcpy(&i, &f, 4); return i; }
static float __int_as_float(int i) { float f; std::memcpy(&f, &i, 4); return f; }
// crt_device.h: the triangle row's material word, the reference's epsilon
#define TNM_MAT(w_) ((w_) & 0x3fffffffu)
#define TNM_EMITTER(w_) (((w_) >> 30) & 1u)
#define TNM_SPECULAR(w_) ((w_) >> 31)
#define CRT_EPSILON 0.00001f
namespace crtk {
// crt_device.h: F3's other operations (there div3 is built from a reciprocal and corrected to the rounded quotients: the same values)
static F3 add3(F3 a, F3 b) { return f3(a.x + b.x, a.y + b.y, a.z + b.z); }
static F3 sub3(F3 a, F3 b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }
static F3 mul3(F3 a, F3 b) { return f3(a.x * b.x, a.y * b.y, a.z * b.z); }
static F3 scale3(F3 a, float s) { return f3(a.x * s, a.y * s, a.z * s); }
static F3 scalel3(float s, F3 a) { return f3(s * a.x, s * a.y, s * a.z); }
static F3 div3(F3 a, float s) { return f3(a.x / s, a.y / s, a.z / s); }
static float norm3(F3 a) { return sqrt_f(dot3(a, a)); }
// crt_path.h: the ray kinds, shadow_blocked
enum { RAY_NONE = 0, RAY_CLOSEST = 1, RAY_SHADOW = 2 };
template <int MODE> static bool shadow_blocked(float tl, float T, int tri)
{
    if (MODE != 1) return tri >= 0 || tl - FLT_MAX > CRT_EPSILON;
    return tl - T > CRT_EPSILON;
}
// crt_device.h: cross3; crt_trace.h: to_world, sample_hemisphere; crt_path.h: bounce_dir (crt_aov_ao.h's directions) -- the same text
static F3 cross3(F3 a, F3 b) { return f3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
static F3 to_world(F3 a, F3 N)
{
    F3 C;
    if (absf(N.x) > absf(N.y)) {
        float invLen = 1.0f / sqrt_f(N.x * N.x + N.z * N.z);
        C = f3(N.z * invLen, 0.0f, -N.x * invLen);
    } else {
        float invLen = 1.0f / sqrt_f(N.y * N.y + N.z * N.z);
        C = f3(0.0f, N.z * invLen, -N.y * invLen);
    }
    F3 B = cross3(C, N);
    return add3(add3(scalel3(a.x, B), scalel3(a.y, C)), scalel3(a.z, N));
}
static F3 sample_hemisphere(F3 N, float x_1, float x_2)
{
    float z = absf(1.0f - 2.0f * x_1);
    float r = sqrt_f(1.0f - z * z);
    float phi = (float)(2 * 3.14159265358979323846 * (double)x_2);
    float sn, cs;
    det_sincosf(phi, &sn, &cs);
    return to_world(f3(r * cs, r * sn, z), N);
}
static F3 bounce_dir(const F3 n, const U4 rb) { return unit3(sample_hemisphere(n, rng_uniform(rb.y), rng_uniform(rb.z))); }
} // namespace crtk
#endif

// ---- the launch: its indices, and with CRT_HOST_WAVES the wave ----
struct Idx { uint32_t x; };
static thread_local Idx blockIdx, threadIdx, gridDim;

#ifndef CRT_HOST_WAVES
// a launch of kernels without a cross-lane operation: a plain loop over blocks and threads
template <class K, class... P> static void hipLaunchKernelGGL(K kernel, dim3 grid, dim3 block, int, hipStream_t, P... params)
{
    gridDim.x = grid.x;
    for (uint32_t b = 0; b < grid.x; b++)
        for (uint32_t t = 0; t < block.x; t++) { blockIdx.x = b; threadIdx.x = t; kernel(params...); }
}
#else
// A wave is 64 host threads that meet at a barrier in every cross-lane operation, so a ballot sees all its lanes' predicates as the
// hardware's does.
struct Wave { // the 64 lanes of the wave that is running
    std::mutex m;
    std::condition_variable cv;
    int waiting = 0;
    unsigned long gen = 0;
    long long in[64], vals[64];
    // The barrier: every lane hands in a value and returns when all 64 have, with the 64 values in vals.  (vals is written again by
    // the last lane to reach the NEXT barrier, so after every lane has read it.)
    void barrier(long long v = 0)
    {
        std::unique_lock<std::mutex> l(m);
        in[threadIdx.x & 63] = v;
        const unsigned long g = gen;
        if (++waiting == 64) { waiting = 0; std::copy(in, in + 64, vals); gen++; cv.notify_all(); }
        else cv.wait(l, [&] { return gen != g; });
    }
};
static Wave g_wave;
static unsigned long long __ballot(bool p)
{
    g_wave.barrier(p);
    unsigned long long m = 0;
    for (int lane = 0; lane < 64; lane++) m |= (unsigned long long)(g_wave.vals[lane] != 0) << lane;
    return m;
}
static int __builtin_amdgcn_readlane(int v, int lane_from)
{
    g_wave.barrier(v);
    return (int)g_wave.vals[lane_from];
}
static int __builtin_amdgcn_readfirstlane(int v) { return __builtin_amdgcn_readlane(v, 0); } // (called with every lane active)
// the shuffle of an 8-byte value (double, unsigned long long): lane + delta's, a lane's own where that is beyond the wave
template <class T> static T __shfl_down(T v, unsigned int delta)
{
    static_assert(sizeof(T) == sizeof(long long), "an 8-byte value");
    long long bits;
    std::memcpy(&bits, &v, sizeof(bits));
    g_wave.barrier(bits);
    const unsigned int lane = threadIdx.x & 63u, from = lane + delta < 64u ? lane + delta : lane;
    bits = g_wave.vals[from];
    std::memcpy(&v, &bits, sizeof(bits));
    return v;
}
// LDS: one static array, which the waves of a block -- run one after another here -- all see; so the block-wide barrier is the
// wave's own, and is right for kernel text in which only the block's LAST wave reads what the others wrote (crt_frame_error.h)
#define __shared__ static
static void __syncthreads() { g_wave.barrier(); }
static int __ffsll(long long v) { return __builtin_ffsll(v); }
static int __popcll(unsigned long long v) { return __builtin_popcountll(v); }

// a launch: block after block, wave after wave (a block of 64 threads is one wave).  The 64 lane threads live for the whole launch
// and meet at the end of every wave, so a wave starts when the one before it has ended.
template <class K, class... P> static void hipLaunchKernelGGL(K kernel, dim3 grid, dim3 block, int, hipStream_t, P... params)
{
    std::vector<std::thread> lanes;
    for (uint32_t l = 0; l < 64; l++)
        lanes.emplace_back([=] {
            gridDim.x = grid.x;
            for (uint32_t b = 0; b < grid.x; b++)
                for (uint32_t w0 = 0; w0 < block.x; w0 += 64) {
                    blockIdx.x = b; threadIdx.x = w0 + l;
                    kernel(params...);
                    g_wave.barrier();
                }
        });
    for (std::thread& t : lanes) t.join();
}
#endif
