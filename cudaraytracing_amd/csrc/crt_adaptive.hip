// cudaraytracing_amd/csrc/crt_adaptive.hip -- the kernels of crt_render_adaptive (contract: include/crt.h; host loop: crt_sparse.hip):
// between the passes of k_mega3, one thread per pixel slot decides which pixels go on and counts the coming pass into their n_p
// (k_adaptive_select), a list turns the render kernel's work cursor into (sample, active pixel) (k_adaptive_items), and at the end the
// sums become the frame (k_adaptive_resolve, for every sparse frame).  A pass's radiance goes into the sums by k_map_fold
// (crt_sample_map.hip): a slot that goes on has n_p = the pass's end, one that has stopped has n_p <= the pass's begin.
// Memory: the sums, the sample-count plane, the list of active slots and its counter are uncached allocations accessed with
// agent-scope atomics only; the item list is written with agent-scope stores, as k_order_items writes it (docs/experiments.md 6).
// The slot map, the accessors, the stop criterion and the output write are the image-space kernels' (crt_stages.h).
#include "crt_internal.h"

namespace crtk {

// After the warm-up: every pixel of the shard has D.n samples; padding slots have none (and, D.n >= 2, never count as active).
__global__ __launch_bounds__(256) void k_adaptive_init(const AdaptiveParams D)
{
    const AParams& A = D.sums.A;
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= A.nslots) return;
    word_store(D.sums.nsamp + slot, slot_pixel(A, slot).valid ? D.n : 0u);
}

// The stop criterion of include/crt.h for every still-active slot -- n_p == D.n: a slot that stopped earlier has fewer -- and the list of
// the slots that go on, whose n_p becomes that of the end of the coming pass, D.n + D.ns_pass (a slot that stops keeps its count): per
// wave a ballot, a popcount and ONE atomic on the counter.  The order of the list is whatever the atomics make it: it decides which wave
// traces a path, never what the path is.
__global__ __launch_bounds__(256) void k_adaptive_select(const AdaptiveParams D)
{
    const AParams& A = D.sums.A;
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    bool act = slot < A.nslots && word_load(D.sums.nsamp + slot) == D.n;
    if (act) {
        const StopCriterion k = stop_criterion(A, D.sums.qacc, slot, D.n, D.threshold, D.mean_floor);
        if (k.v <= k.tt) act = false; // (false for NaN: such a pixel runs to the cap)
        else word_store(D.sums.nsamp + slot, D.n + D.ns_pass);
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

// The frame: per pixel n_p, mean = c * (S / n_p), its tone map, and the variance of that mean, in the layout of crt_render's buffers
// (padding slots of a tiled shard 0 / +0).
__global__ __launch_bounds__(256) void k_adaptive_resolve(const SumsParams D, uint32_t* const out_samples, float* const out_variance)
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
        if (out_variance) v = variance_of3(c, acc_load3(D.qacc, A.nslots, slot), fn, r * r);
    }
    const uint64_t o = px.o;
    write_color(A, o, px.valid, p);
    if (out_samples) out_samples[o] = n;
    if (out_variance) { out_variance[o * 3 + 0] = v.x; out_variance[o * 3 + 1] = v.y; out_variance[o * 3 + 2] = v.z; }
}

// ---- exported to crt_sparse.hip ----
void launch_adaptive_init(const AdaptiveParams& D, hipStream_t st) { hipLaunchKernelGGL(k_adaptive_init, slot_grid(D.sums.A), dim3(256), 0, st, D); }
void launch_adaptive_select(const AdaptiveParams& D, hipStream_t st) { hipLaunchKernelGGL(k_adaptive_select, slot_grid(D.sums.A), dim3(256), 0, st, D); }
void launch_adaptive_items(uint32_t* item_list, const uint32_t* list, uint32_t n_active, uint32_t n_items, uint32_t nslots, hipStream_t st)
{
    hipLaunchKernelGGL(k_adaptive_items, dim3((n_items + 255) / 256), dim3(256), 0, st, item_list, list, n_active, make_fastdiv(n_active), n_items, nslots);
}
void launch_adaptive_resolve(const SumsParams& D, uint32_t* out_samples, float* out_variance, hipStream_t st)
{
    hipLaunchKernelGGL(k_adaptive_resolve, slot_grid(D.A), dim3(256), 0, st, D, out_samples, out_variance);
}

} // namespace crtk
