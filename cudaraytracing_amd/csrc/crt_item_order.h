// cudaraytracing_amd/csrc/crt_item_order.h -- k_order_items: the order in which the LAST order_window work items of every cursor shard
// are handed out (what the waves get when a launch ends), longest paths first.  Included by crt_mega3.hip alone, after crt_path.h; written so that
// tools/item_order_host_check.cpp can compile this very text for the host behind stand-ins for what it takes from outside:
// LParams (seed, p_rr, n_items, items_per_shard, order_window), decode_item, roulette (crt_path.h), CRT_BOUNCE_STACK_SIZE, the launch
// indices, __ballot, __popcll, __builtin_amdgcn_readlane and the agent-scope atomics.
#ifndef CRT_ITEM_ORDER_H
#define CRT_ITEM_ORDER_H

namespace crtk {

// The classes of the order: class c holds the paths whose roulette length lies in [lo[c], lo[c + 1]), the last one everything from its
// bound on; lo[0] = 1, ascending.  Class 0 also takes the padding slots of ragged tiles.  A shard's window lists class n - 1 first, class 0 last.
#define ORDER_CLASSES_MAX 8
struct OrderClasses {
    uint32_t n;
    uint32_t lo[ORDER_CLASSES_MAX];
};
// a class number is kept in 4 bits, 16 of them in a word
static_assert(ORDER_CLASSES_MAX <= 16, "k_order_items keeps a class in 4 bits");

// The number of vertices the roulette alone gives sample k of a pixel, capped at `cap` (>= 1): the first depth at which roulette
// (crt_path.h, which logic_B calls: Render.cuh:210-213) says stop, plus one -- its draws are addressed (crt_detmath.h), so this is known before
// anything is traced.  An upper bound of the path's real length, and equal to it unless the path leaves the scene or meets an emitter.
__device__ __forceinline__ uint32_t roulette_length(const uint64_t seed, const uint32_t pixel_index, const uint32_t k, const float p_rr, const uint32_t cap)
{
    uint32_t depth = 0;
    U4 rb;
    while (depth + 1u < cap && !roulette(seed, pixel_index, k, depth, p_rr, rb)) depth++;
    return depth + 1u;
}
__device__ __forceinline__ uint32_t order_class(const OrderClasses& C, const uint32_t length)
{
    uint32_t c = 0;
    for (uint32_t q = 1; q < C.n; q++)
        if (length >= C.lo[q]) c = q;
    return c;
}

// One wave per span of 1 024 items of one shard's window, in two launches.  PLACE = false counts the span's items per class into the
// shard's totals; PLACE = true takes, per class, a run of the class's part of the window as long as the span has items of it, and writes
// them there in item order: the camera rays of a span that are handed out together stay neighbours.  A shard's window is then class
// n - 1, ..., class 0, and the spans of a class follow one another in the order their atomics arrived -- the order of the work items cannot
// change a result (every path writes its own L[item]).  cnt: per shard and class one 128 B line (the atomics of a shard and class serialise
// on their line, those of different ones must not): word 0 the total, word 1 the place pass's cursor; zero before the count pass.
// Why: every launch ends with each wave running its pool dry, and the time that takes is the longest path started last.
template <bool RING, bool PLACE>
__global__ __launch_bounds__(64) void k_order_items(const LParams P, const OrderClasses C, uint32_t* list, unsigned int* cnt)
{
    const uint32_t spans = (P.order_window + 1023u) / 1024u;
    const uint32_t sh = blockIdx.x / spans, sp = blockIdx.x - sh * spans;
    const uint32_t slo = sh * P.items_per_shard;
    if (slo >= P.n_items) return;
    const uint32_t hi = min(slo + P.items_per_shard, P.n_items);
    const uint32_t lo = hi - min(P.order_window, hi - slo); // the window: the last order_window items of the shard
    const uint32_t b = lo + sp * 1024u;
    if (b >= hi) return;
    uint32_t* out = list + (size_t)sh * P.order_window; // out[k] = the item handed out in place of item lo + k
    const uint32_t lane = threadIdx.x;
    unsigned long long cls = 0; // bits 4 j .. 4 j + 3: the class of item b + 64 j + lane
    uint32_t exists = 0;        // bit j: that item exists
#pragma unroll 1
    for (uint32_t j = 0; j < 16; j++) {
        const uint32_t i = b + j * 64u + lane;
        if (i < hi) {
            bool valid; uint32_t pi, pj, pixel_index, k;
            decode_item<RING>(P, i, pixel_index, k, valid, pi, pj);
            exists |= 1u << j;
            if (valid) cls |= (unsigned long long)order_class(C, roulette_length(P.seed, pixel_index, k, P.p_rr, C.lo[C.n - 1u])) << (4u * j);
        }
    }
    // lane c < n: the span's items of class c
    uint32_t mine = 0;
#pragma unroll 1
    for (uint32_t c = 0; c < C.n; c++) {
        uint32_t n_c = 0;
#pragma unroll 1
        for (uint32_t j = 0; j < 16; j++) n_c += (uint32_t)__popcll(__ballot(((exists >> j) & 1u) && (uint32_t)((cls >> (4u * j)) & 15u) == c));
        if (lane == c) mine = n_c;
    }
    unsigned int* line = cnt + ((size_t)sh * C.n + min(lane, C.n - 1u)) * 32u; // (of lane c < n)
    if (!PLACE) {
        if (lane < C.n && mine) __hip_atomic_fetch_add(line, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    // lane c < n: where the span's items of class c begin -- behind every longer class and the spans of its own that came before
    uint32_t total = 0, base = 0;
    if (lane < C.n) total = __hip_atomic_load(line, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll 1
    for (uint32_t q = 1; q < C.n; q++) {
        const uint32_t t_q = (uint32_t)__builtin_amdgcn_readlane((int)total, (int)q);
        if (lane < q) base += t_q;
    }
    if (lane < C.n && mine) base += __hip_atomic_fetch_add(line + 1, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll 1
    for (uint32_t j = 0; j < 16; j++) {
        const bool ex_j = (exists >> j) & 1u;
        const uint32_t cls_j = (uint32_t)((cls >> (4u * j)) & 15u);
#pragma unroll 1
        for (uint32_t c = 0; c < C.n; c++) {
            const unsigned long long m = __ballot(ex_j && cls_j == c);
            if (!m) continue; // (the same in every lane)
            const uint32_t at = (uint32_t)__builtin_amdgcn_readlane((int)base, (int)c);
            // (agent-scope stores, as logic_C's load: crt_mega3_logic.h)
            if (ex_j && cls_j == c) __hip_atomic_store(&out[at + (uint32_t)__popcll(m & below)], b + j * 64u + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (lane == c) base += (uint32_t)__popcll(m);
        }
    }
}

} // namespace crtk
#endif
