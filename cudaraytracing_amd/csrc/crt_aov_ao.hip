// cudaraytracing_amd/csrc/crt_aov_ao.hip -- the kernels of the ambient-occlusion AOV pass (crt_render_aov_ao, include/crt.h): what each
// thread does is stated in crt_aov_ao.h, which the host check program compiles too; here are the launches and the one cross-lane step,
// the sum of the call's occlusion rays for crt_aov_info.  Host side: ao_pass, crt_aov_pass.hip.
#include "crt_internal.h"

#include "crt_aov_ao.h"

namespace crtk {

// one thread per camera ray of the chunk
__global__ __launch_bounds__(256) void k_aov_ao_vertex(const AovAoParams D)
{
    const uint64_t item = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (item >= (uint64_t)D.n_samples * D.nslots) return;
    aov_ao_vertex(D, item);
}

// One thread per (entry, slot) of the sub-batch; consecutive lanes are consecutive slots and nslots is a multiple of 64, so a wave lies in
// one entry: its sample and q are the same in every lane.
__global__ __launch_bounds__(256) void k_aov_ao_setup(const AovAoParams D)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= D.e_count * D.nslots) return; // (whole waves: both factors of the bound are wave-uniform and nslots is a multiple of 64)
    aov_ao_setup(D, i, (uint32_t)__builtin_amdgcn_readfirstlane((int)(i / D.nslots)));
}

// One thread per pixel slot.  The call's last sub-batch also adds up the slots' occlusion rays: a wave's sum, one atomic per wave.
__global__ __launch_bounds__(256) void k_aov_ao_resolve(const AovAoParams D)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= D.nslots) return; // (whole waves)
    unsigned long long n = aov_ao_resolve(D, slot);
    if (!D.last_batch) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63u) == 0u && n != 0ull) (void)__hip_atomic_fetch_add(D.ray_total, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- exported to crt_aov_pass.hip ----
void launch_aov_ao_vertex(const AovAoParams& D, hipStream_t st)
{
    const uint64_t n = (uint64_t)D.n_samples * D.nslots;
    hipLaunchKernelGGL(k_aov_ao_vertex, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, D);
}
void launch_aov_ao_setup(const AovAoParams& D, hipStream_t st)
{
    const uint64_t n = (uint64_t)D.e_count * D.nslots; // (at most 2^31: a sub-batch is 2^25 entries, or one entry per slot of the shard)
    hipLaunchKernelGGL(k_aov_ao_setup, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, D);
}
void launch_aov_ao_resolve(const AovAoParams& D, hipStream_t st) { hipLaunchKernelGGL(k_aov_ao_resolve, slot_grid(D), dim3(256), 0, st, D); }

} // namespace crtk
