// cudaraytracing_amd/csrc/crt_aov_direct.hip -- the kernels of the direct-light AOV pass (crt_render_aov_direct, include/crt.h): what each
// thread does is stated in crt_aov_direct.h, which the host check program compiles too; here are the launches.  Host side: direct_pass,
// crt_aov_pass.hip.
#include "crt_internal.h"

#include "crt_aov_direct.h"

namespace crtk {

// one thread per camera ray of the chunk
__global__ __launch_bounds__(256) void k_aov_direct_vertex(const AovDirectParams D)
{
    const uint64_t item = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (item >= (uint64_t)D.n_samples * D.nslots) return;
    aov_direct_vertex(D, item);
}

// One thread per (group of kAovDirectWaveEntries entries, slot) of the sub-batch; consecutive lanes are consecutive slots and nslots is a
// multiple of 64, so a wave lies in one group: the q of each of its entries, and with it the light's table entry, is the same in every
// lane and loads once per wave.
__global__ __launch_bounds__(256) void k_aov_direct_setup(const AovDirectParams D)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    aov_direct_setup(D, i, (uint32_t)__builtin_amdgcn_readfirstlane((int)(i / D.nslots)));
}

// one thread per traced ray
__global__ __launch_bounds__(256) void k_aov_direct_answer(const AovDirectParams D)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= D.n_traced) return;
    aov_direct_answer(D, j);
}

// one thread per pixel slot
__global__ __launch_bounds__(256) void k_aov_direct_resolve(const AovDirectParams D)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= D.nslots) return;
    aov_direct_resolve(D, slot);
}

// ---- exported to crt_aov_pass.hip ----
void launch_aov_direct_vertex(const AovDirectParams& D, hipStream_t st)
{
    const uint64_t n = (uint64_t)D.n_samples * D.nslots;
    hipLaunchKernelGGL(k_aov_direct_vertex, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, D);
}
void launch_aov_direct_setup(const AovDirectParams& D, hipStream_t st)
{
    const uint64_t n = (uint64_t)((D.e_count + kAovDirectWaveEntries - 1) / kAovDirectWaveEntries) * D.nslots;
    hipLaunchKernelGGL(k_aov_direct_setup, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, D);
}
void launch_aov_direct_answer(const AovDirectParams& D, hipStream_t st) { hipLaunchKernelGGL(k_aov_direct_answer, dim3((D.n_traced + 255) / 256), dim3(256), 0, st, D); }
void launch_aov_direct_resolve(const AovDirectParams& D, hipStream_t st) { hipLaunchKernelGGL(k_aov_direct_resolve, slot_grid(D), dim3(256), 0, st, D); }

} // namespace crtk
