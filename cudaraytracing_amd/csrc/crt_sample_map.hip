// cudaraytracing_amd/csrc/crt_sample_map.hip -- the kernels of crt_render_map, crt_sample_plan and crt_render_planned (contract:
// include/crt.h; host side: crt_sparse.hip): a frame in which pixel p gets samples sample_begin .. n_p - 1, n_p given per pixel, in ONE
// launch of k_mega3 per chunk of samples.  k_map_prepare turns the caller's map into the per-slot counts and their histogram, from which
// the host sizes every chunk; k_map_items writes a chunk's item list (sample-major, a wave's slots side by side); k_map_fold adds each
// slot's own number of the chunk's samples to its sums, for the passes of crt_render_adaptive too; k_sample_plan solves the adaptive stop
// criterion for n.  The frame itself is k_adaptive_resolve's (crt_adaptive.hip).
// Memory: the sums, the count plane, the histogram and the cursors are uncached allocations accessed with agent-scope atomics only; the
// item list is written with agent-scope stores, as k_order_items and k_adaptive_items write it (docs/experiments.md 6).
#include "crt_internal.h"

namespace crtk {

// n_p = min(max(map[p], max(sample_begin, 1)), S) per pixel slot (padding slots 0) into the count plane, and the histogram of n_p over
// 0 .. S.  The histogram is aggregated per wave before any atomic: the wave walks the distinct values among its lanes -- the first
// pending lane's value, a ballot of the lanes that share it, ONE atomic with their number -- so a uniform map costs one atomic per wave,
// not one per slot on one address.  Every lane of a wave stays in the loop (its condition is a ballot): no lane returns early.
__global__ __launch_bounds__(256) void k_map_prepare(const MapParams D)
{
    const AParams& A = D.sums.A;
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    const bool in = slot < A.nslots;
    uint32_t np = 0;
    if (in) {
        const SlotPixel px = slot_pixel(A, slot);
        if (px.valid) {
            const uint32_t m = D.map[D.map_per_slot ? (uint64_t)slot : (uint64_t)px.j * A.width + px.i];
            np = min(max(m, max(D.sample_begin, 1u)), A.spp);
        }
        word_store(D.sums.nsamp + slot, np);
    }
    const int lane = threadIdx.x & 63;
    bool todo = in;
    for (;;) {
        const unsigned long long pending = __ballot(todo);
        if (pending == 0ull) break;
        const int leader = __ffsll((long long)pending) - 1;
        const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)np, leader);
        const unsigned long long same = __ballot(todo && np == v);
        if (lane == leader) __hip_atomic_fetch_add(D.hist + v, (unsigned int)__popcll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (v <= spp: the histogram has spp + 1 words)
        if (np == v) todo = false;
    }
}

// The item list of the launch of samples [s0, s0 + ns): for every sample s of the chunk, in order, the slots with n_p > s -- per wave a
// ballot, a popcount and ONE atomic on that sample's cursor, which the host has set to the sample's first position in the list (the sum
// of the counts of the chunk's earlier samples).  So the list is sample-major and a wave's slots of a sample stand side by side, as the
// uniform hand-out has them; which wave's run comes first within a sample is whatever the atomics make it, and decides which wave traces
// a path, never what the path is.  Entry = the frame's own work item (s - s0) * nslots + slot (decode_item), where k_mega3 writes L.
// n_p > s only gets rarer as s grows, so the wave leaves the loop at the first sample none of its slots takes.
// (All waves walk s0, s0 + 1, ... in step, so the atomics of a moment meet on one cursor: 11.6 ms for the list of an 800x600 frame with
// 512 samples everywhere; docs/experiments.md, "Sample maps and planned adaptive frames", has the remedy that was not run on a device.)
__global__ __launch_bounds__(256) void k_map_items(const MapParams D)
{
    const AParams& A = D.sums.A;
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    const uint32_t np = slot < A.nslots ? word_load(D.sums.nsamp + slot) : 0u;
    const uint32_t hi = min(np, D.s0 + D.ns);
    const uint32_t last_item = D.ns * A.nslots - 1u; // (ns x nslots < 2^32: the chunk's cap)
    const int lane = threadIdx.x & 63;
    for (uint32_t s = D.s0;; s++) {
        const bool take = s < hi;
        const unsigned long long mask = __ballot(take);
        if (mask == 0ull) break;
        const int leader = __ffsll((long long)mask) - 1;
        unsigned int base = 0;
        if (lane == leader) base = __hip_atomic_fetch_add(D.cursor + s, (unsigned int)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (s < spp)
        base = (unsigned int)__builtin_amdgcn_readlane((int)base, leader);
        const uint32_t pos = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        // (pos < n_items by the histogram the host sized the list with; both clamps keep every access inside the list and every item inside L
        // whatever the planes hold)
        if (take && pos < D.n_items) __hip_atomic_store(&D.item_list[pos], min((s - D.s0) * A.nslots + slot, last_item), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The chunk's samples into c and q: slot p takes min(n_p, s0 + ns) - s0 of them (none if n_p <= s0: its entries of L hold whatever an
// earlier launch left).  The chunk that starts at sample 0 starts the sums of every slot at +0, padding included.
__global__ __launch_bounds__(256) void k_map_fold(const SumsParams D, const uint32_t s0, const uint32_t ns)
{
    const AParams& A = D.A;
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= A.nslots) return;
    const uint32_t np = word_load(D.nsamp + slot);
    const uint32_t count = np > s0 ? min(np, s0 + ns) - s0 : 0u;
    if (count == 0u && !A.first_chunk) return;
    F3 c = f3(0.0f, 0.0f, 0.0f), q = f3(0.0f, 0.0f, 0.0f);
    if (!A.first_chunk) { c = acc_load3(A.accum, A.nslots, slot); q = acc_load3(D.qacc, A.nslots, slot); }
    fold_samples_n<true>(A, slot, count, c, q);
    acc_store3(A.accum, A.nslots, slot, c);
    acc_store3(D.qacc, A.nslots, slot, q);
}

// crt_sample_plan: the adaptive criterion solved for n, from the sums of the frame in flight at n = D.n samples, in the frame's output
// layout (padding slots of a tiled shard 0).  Reads the sums only.
__global__ __launch_bounds__(256) void k_sample_plan(const MapParams D)
{
    const AParams& A = D.sums.A;
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= A.nslots) return;
    const SlotPixel px = slot_pixel(A, slot);
    if (!px.out) return;
    uint32_t np = 0;
    if (px.valid) {
        const float fn = (float)D.n, fs = (float)A.spp;
        const StopCriterion k = stop_criterion(A, D.sums.qacc, slot, D.n, D.threshold, D.mean_floor);
        const float w = (fn * k.v) / k.tt;
        np = (w < fs) ? max(D.n, (uint32_t)ceilf(w)) : A.spp; // (NaN, +inf and w >= S: the cap; w < S is below 2^32, and a negative w cannot occur: v >= 0)
    }
    D.out_map[px.o] = np;
}

// ---- exported to crt_sparse.hip ----
void launch_map_prepare(const MapParams& D, hipStream_t st) { hipLaunchKernelGGL(k_map_prepare, slot_grid(D.sums.A), dim3(256), 0, st, D); }
void launch_map_items(const MapParams& D, hipStream_t st) { hipLaunchKernelGGL(k_map_items, slot_grid(D.sums.A), dim3(256), 0, st, D); }
void launch_map_fold(const SumsParams& D, uint32_t s0, uint32_t ns, hipStream_t st) { hipLaunchKernelGGL(k_map_fold, slot_grid(D.A), dim3(256), 0, st, D, s0, ns); }
void launch_sample_plan(const MapParams& D, hipStream_t st) { hipLaunchKernelGGL(k_sample_plan, slot_grid(D.sums.A), dim3(256), 0, st, D); }

} // namespace crtk
