// cudaraytracing_amd/csrc/crt_mega3_wave.h -- what k_mega3's scheduler and every step share: scalar-unit helpers, the append to a ring of ray
// ids, the -DCRT_STAMPS clock.  Included by crt_mega3.hip only.
#ifndef CRT_MEGA3_WAVE_H
#define CRT_MEGA3_WAVE_H
#include "crt_internal.h"

namespace crtk {

// max of two wave-uniform integers on the scalar unit
__device__ __forceinline__ int smax(const int a, const int b)
{
    int r;
    asm("s_max_i32 %0, %1, %2" : "=s"(r) : "s"(a), "s"(b) : "scc");
    return r;
}

// The rings are stacks: a batch is the NEWEST ids, no head, no tail, no wrap.
// (the count doubles as the place of the next id, i.e. as the addend of v_mbcnt, a vector operand: handed over as a scalar COPY, or the
// compiler moves the count itself into a vector register, where the scheduler's scalar maxima cannot reach it)
__device__ __forceinline__ uint32_t scalar_copy(int x) { asm volatile("" : "+s"(x)); return (uint32_t)x; }

// -DCRT_STAMPS (a diagnostic build, tools/ab_build.sh): the wave's cycles by phase -- s_memtime at the end of every step, the difference to
// the stamp before it booked on the step that ended (the scheduler's share on "other") -- summed into crt_stats.phase_cycles:
// [0] LA [1] leaf step [2] inner step [3] scheduler / rest [4] LB [5] LC, and the steps of each kind in [6..11] (same order)
#ifdef CRT_STAMPS
struct Stamps {
    unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
    uint32_t n[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long prev = __builtin_amdgcn_s_memtime();
    __device__ __forceinline__ void step(const int k) { const unsigned long long t = __builtin_amdgcn_s_memtime(); acc[k] += t - prev; prev = t; n[k]++; }
    __device__ __forceinline__ void other() { const unsigned long long t = __builtin_amdgcn_s_memtime(); acc[3] += t - prev; prev = t; }
};
#else
struct Stamps {
    __device__ __forceinline__ void step(int) {}
    __device__ __forceinline__ void other() {}
};
#endif

// The ring append: the lanes with `mine` (m = its ballot) put ray `id` on a ring that holds n ids -- at n + the number of lanes below
// that do the same: the count rides in as mbcnt's addend.  Every phase's step and the decoupled inner step's re-queue end with it
// (the parking ring of the commit ring, which wraps, has its own in the LC phase).
// (the counting kernels keep more scalars: their count may live in a vector register and goes in as it is)
template <bool STATS>
__device__ __forceinline__ void ring_append(uint8_t* const rq, int& n, const bool mine, const unsigned long long m, const uint32_t id)
{
    if (m) {
        const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, STATS ? (uint32_t)n : scalar_copy(n)));
        if (mine) rq[slot] = (uint8_t)id;
        n += (int)__popcll(m);
    }
}

} // namespace crtk
#endif
