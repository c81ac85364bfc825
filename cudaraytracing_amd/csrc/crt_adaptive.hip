// cudaraytracing_amd/csrc/crt_adaptive.hip -- the kernels of crt_render_adaptive (contract: include/crt.h; host loop: crt_render.hip):
// between the passes of k_mega3, one thread per pixel slot decides which pixels go on (k_adaptive_select), a list turns the render kernel's
// work cursor into (sample, active pixel) (k_adaptive_items), the pass's radiance goes into the sums of the pixels that took it
// (k_adaptive_accumulate), and at the end the sums become the frame (k_adaptive_resolve).
// Memory: the sums, the active / sample-count planes, the list of active slots and its counter are uncached allocations accessed with
// agent-scope atomics only; the item list is written with agent-scope stores, as k_order_items writes it (docs/experiments.md 6).
// The slot map, the loads and stores of the sums, the sample fold and the output write are the frame kernels' (crt_internal.h).
#include "crt_internal.h"

namespace crtk {

__device__ __forceinline__ uint32_t word_load(const uint32_t* p) { return __hip_atomic_load((const unsigned int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void word_store(uint32_t* p, const uint32_t v) { __hip_atomic_store((unsigned int*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// After the warm-up: every pixel of the shard is active and has D.n samples; padding slots never are and have none.
__global__ __launch_bounds__(256) void k_adaptive_init(const AdaptiveParams D)
{
    const AParams& A = D.A;
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= A.nslots) return;
    const bool valid = slot_pixel(A, slot).valid;
    word_store(D.active + slot, valid ? 1u : 0u);
    word_store(D.nsamp + slot, valid ? D.n : 0u);
}

// The stop criterion of include/crt.h for every still-active slot at n = D.n samples, and the list of the slots that go on: per wave a
// ballot, a popcount and ONE atomic on the counter.  The order of the list is whatever the atomics make it: it decides which wave traces
// a path, never what the path is.
__global__ __launch_bounds__(256) void k_adaptive_select(const AdaptiveParams D)
{
    const AParams& A = D.A;
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    bool act = slot < A.nslots && word_load(D.active + slot) != 0u;
    if (act) {
        const float fn = (float)D.n, fs = (float)A.spp;
        const float r = fs / fn, rr = r * r;
        const F3 c = acc_load3(A.accum, A.nslots, slot);
        const F3 var = variance_of3(c, acc_load3(D.qacc, A.nslots, slot), fn, rr);
        const F3 p = f3(c.x * r, c.y * r, c.z * r);
        const float v = (var.x + var.y) + var.z, m = (p.x + p.y) + p.z;
        const float t = D.threshold * (m + D.mean_floor);
        if (v <= t * t) { // (false for NaN: such a pixel runs to the cap)
            act = false;
            word_store(D.active + slot, 0u);
        }
    }
    const unsigned long long mask = __ballot(act);
    if (mask == 0ull) return;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)mask) - 1;
    unsigned int base = 0;
    if (lane == leader) base = __hip_atomic_fetch_add(D.count, (unsigned int)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = (unsigned int)__builtin_amdgcn_readlane((int)base, leader);
    if (act) word_store(D.list + base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)), slot); // (base + rank < nslots: at most every slot is active)
}

// The item list of a pass's launch: cursor position pos = s * n_active + a stands for sample s of the chunk at active slot list[a], which
// in the frame's own item numbering (decode_item: item = s * nslots + slot) is what k_mega3 decodes and where it writes L.
__global__ __launch_bounds__(256) void k_adaptive_items(uint32_t* const item_list, const uint32_t* const list, const uint32_t n_active, const FastDiv n_active_div,
                                                        const uint32_t n_items, const uint32_t nslots)
{
    const uint32_t pos = blockIdx.x * 256u + threadIdx.x;
    if (pos >= n_items) return;
    const uint32_t s = fast_div(pos, n_active_div.m, n_active_div.sh), a = pos - s * n_active;
    const uint32_t slot = min(word_load(list + a), nslots - 1u); // (k_adaptive_select writes slots only; the clamp keeps every item inside L whatever the list holds)
    __hip_atomic_store(&item_list[pos], s * nslots + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// k_accumulate_var's fold (fold_samples) for the slots that took the pass.  Slots that did not take it are not touched (their entries of
// L hold whatever an earlier launch left).
__global__ __launch_bounds__(256) void k_adaptive_accumulate(const AdaptiveParams D)
{
    const AParams& A = D.A;
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= A.nslots || word_load(D.active + slot) == 0u) return;
    F3 c = acc_load3(A.accum, A.nslots, slot);
    F3 q = acc_load3(D.qacc, A.nslots, slot);
    fold_samples<true>(A, slot, c, q);
    acc_store3(A.accum, A.nslots, slot, c);
    acc_store3(D.qacc, A.nslots, slot, q);
    word_store(D.nsamp + slot, D.n);
}

// The frame: per pixel n_p, mean = c * (S / n_p), its tone map, and the variance of that mean, in the layout of crt_render's buffers
// (padding slots of a tiled shard 0 / +0).
__global__ __launch_bounds__(256) void k_adaptive_resolve(const AdaptiveParams D)
{
    const AParams& A = D.A;
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= A.nslots) return;
    const SlotPixel px = slot_pixel(A, slot);
    if (!px.out) return;
    F3 p = f3(0.0f, 0.0f, 0.0f), v = f3(0.0f, 0.0f, 0.0f);
    uint32_t n = 0;
    if (px.valid) {
        n = word_load(D.nsamp + slot);
        const float fn = (float)n, fs = (float)A.spp;
        const float r = fs / fn;
        const F3 c = acc_load3(A.accum, A.nslots, slot);
        p = f3(c.x * r, c.y * r, c.z * r);
        if (D.out_variance) v = variance_of3(c, acc_load3(D.qacc, A.nslots, slot), fn, r * r);
    }
    const uint64_t o = px.o;
    write_color(A, o, px.valid, p);
    if (D.out_samples) D.out_samples[o] = n;
    if (D.out_variance) { D.out_variance[o * 3 + 0] = v.x; D.out_variance[o * 3 + 1] = v.y; D.out_variance[o * 3 + 2] = v.z; }
}

// ---- exported to crt_render.hip ----
static dim3 slot_grid(const AdaptiveParams& D) { return dim3((D.A.nslots + 255) / 256); }
void launch_adaptive_init(const AdaptiveParams& D, hipStream_t st) { hipLaunchKernelGGL(k_adaptive_init, slot_grid(D), dim3(256), 0, st, D); }
void launch_adaptive_select(const AdaptiveParams& D, hipStream_t st) { hipLaunchKernelGGL(k_adaptive_select, slot_grid(D), dim3(256), 0, st, D); }
void launch_adaptive_items(uint32_t* item_list, const uint32_t* list, uint32_t n_active, uint32_t n_items, uint32_t nslots, hipStream_t st)
{
    hipLaunchKernelGGL(k_adaptive_items, dim3((n_items + 255) / 256), dim3(256), 0, st, item_list, list, n_active, make_fastdiv(n_active), n_items, nslots);
}
void launch_adaptive_accumulate(const AdaptiveParams& D, hipStream_t st) { hipLaunchKernelGGL(k_adaptive_accumulate, slot_grid(D), dim3(256), 0, st, D); }
void launch_adaptive_resolve(const AdaptiveParams& D, hipStream_t st) { hipLaunchKernelGGL(k_adaptive_resolve, slot_grid(D), dim3(256), 0, st, D); }

} // namespace crtk
