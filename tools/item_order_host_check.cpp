// tools/item_order_host_check.cpp -- k_order_items (cudaraytracing_amd/csrc/crt_item_order.h: the roulette length, the classes, the count
// pass and the place pass) compiled for the HOST and run against plain restatements, for AddressSanitizer / UBSan runs without a device.
// The header is included as it is; tools/host_device.h stands in for the device's launch indices, wave intrinsics and atomics and for
// slot_to_pixel, and this file for the rest of what the header takes from crt_path.h (the same text: decode_item, roulette, the fields of
// LParams they read).  A wave is 64 host threads that meet at a barrier in every cross-lane operation, as in
// tools/sample_map_host_check.cpp; every block here is one wave.
// Every buffer is sized exactly (std::vector of the element count the host code allocates), so an access one element out is a report.
//
// tests/test_host_checks.py builds and runs it:
//   g++ -std=c++17 -ffp-contract=off -I cudaraytracing_amd/csrc -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       -pthread tools/item_order_host_check.cpp -o /tmp/item_order_host_check && /tmp/item_order_host_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CRT_HOST_WAVES
#include "host_device.h"

// ---- what the header takes from crt_path.h beyond host_device.h: the same text ----
#define CRT_BOUNCE_STACK_SIZE 64
namespace crtk {
struct LParams { // (the fields k_order_items and decode_item read)
    uint32_t width, height;
    float p_rr;
    uint64_t seed;
    uint32_t rank, world, tiles_x, n_tiles;
    uint32_t nslots, sample_begin, n_items, items_per_shard;
    FastDiv nslots_div, tiles_x_div;
    uint32_t order_window;
    FastDiv items_per_shard_div;
    uint32_t spsh;
    FastDiv spsh_div;
};
template <bool RING = false>
static void decode_item(const LParams& P, uint32_t item, uint32_t& pixel_index, uint32_t& k, bool& valid, uint32_t& pi, uint32_t& pj)
{
    uint32_t s, slot;
    if (RING) { // cursor shard = a range of pixel slots, sample-major inside it (commit ring)
        const uint32_t sh = fast_div(item, P.items_per_shard_div.m, P.items_per_shard_div.sh), c = item - sh * P.items_per_shard;
        s = fast_div(c, P.spsh_div.m, P.spsh_div.sh);
        slot = sh * P.spsh + (c - s * P.spsh);
    } else {
        s = fast_div(item, P.nslots_div.m, P.nslots_div.sh);
        slot = item - s * P.nslots;
    }
    k = P.sample_begin + s;
    valid = (!RING || slot < P.nslots) && slot_to_pixel(slot, P.rank, P.world, P.n_tiles, P.tiles_x, P.tiles_x_div, P.width, P.height, pi, pj);
    pixel_index = pj * P.width + pi; // Render.cuh:336
}
static bool roulette(const uint64_t seed, const uint32_t pixel_index, const uint32_t k, const uint32_t depth, const float p_rr, U4& rb)
{
    bool stop = depth == CRT_BOUNCE_STACK_SIZE - 1; // bounce stack full
    rb.x = rb.y = rb.z = rb.w = 0;
    if (!stop) {
        rb = rng_draw(seed, pixel_index, k, depth, RNG_BOUNCE, 0);
        stop = rng_uniform(rb.x) > p_rr;
    }
    return stop;
}
} // namespace crtk

#include "crt_item_order.h"

using namespace crtk;

static int g_fail = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fail++; } \
    } while (0)

// ---- plain restatements ----
// a work item's pixel and sample, with / and %
static bool restated_item(const LParams& P, bool ring, uint32_t item, uint32_t& pixel_index, uint32_t& k)
{
    uint32_t s, slot;
    if (ring) { const uint32_t sh = item / P.items_per_shard, c = item % P.items_per_shard; s = c / P.spsh; slot = sh * P.spsh + c % P.spsh; }
    else { s = item / P.nslots; slot = item % P.nslots; }
    k = P.sample_begin + s;
    if (slot >= P.nslots) return false;
    const uint32_t tile = (slot / 64) * P.world + P.rank, pix = slot % 64;
    if (tile >= P.n_tiles) return false;
    const uint32_t i = (tile % P.tiles_x) * 8 + pix % 8, j = (tile / P.tiles_x) * 8 + pix / 8;
    pixel_index = j * P.width + i;
    return i < P.width && j < P.height;
}
// vertices of the path by its addressed draws alone: roulette() stepped depth by depth until it says stop
static uint32_t stepped_length(uint64_t seed, uint32_t pixel_index, uint32_t k, float p_rr)
{
    uint32_t depth = 0;
    U4 rb;
    while (!roulette(seed, pixel_index, k, depth, p_rr, rb)) depth++;
    return depth + 1;
}
// the same from the draw itself (Render.cuh:210-213)
static uint32_t drawn_length(uint64_t seed, uint32_t pixel_index, uint32_t k, float p_rr)
{
    for (uint32_t depth = 0; depth < CRT_BOUNCE_STACK_SIZE - 1; depth++)
        if (rng_uniform(rng_draw(seed, pixel_index, k, depth, RNG_BOUNCE, 0).x) > p_rr) return depth + 1;
    return CRT_BOUNCE_STACK_SIZE;
}
static uint32_t restated_class(const OrderClasses& C, uint32_t length)
{
    for (uint32_t c = C.n; c-- > 1;)
        if (length >= C.lo[c]) return c;
    return 0;
}

// One launch: a w x h frame as shard rank / world, ns samples from sample_begin, n_sh cursor shards, the window, the classes
static void run_case(uint32_t w, uint32_t h, uint32_t rank, uint32_t world, uint32_t sample_begin, uint32_t ns, uint32_t n_sh, bool ring, uint32_t window,
                     const OrderClasses& C, uint64_t seed, float p_rr)
{
    LParams P{};
    P.width = w; P.height = h; P.p_rr = p_rr; P.seed = seed; P.rank = rank; P.world = world;
    P.tiles_x = (w + 7) / 8; P.n_tiles = P.tiles_x * ((h + 7) / 8);
    P.nslots = (P.n_tiles + world - 1) / world * 64; P.sample_begin = sample_begin;
    P.nslots_div = make_fastdiv(P.nslots); P.tiles_x_div = make_fastdiv(P.tiles_x);
    if (ring) { // cursor shard = spsh pixel slots x ns samples (plan_ring, render_mega)
        P.spsh = ((P.nslots + n_sh - 1) / n_sh + 63u) & ~63u;
        P.items_per_shard = P.spsh * ns;
        P.n_items = P.items_per_shard * n_sh;
    } else {
        P.spsh = 1;
        P.n_items = P.nslots * ns;
        P.items_per_shard = (P.n_items + n_sh - 1) / n_sh;
    }
    P.spsh_div = make_fastdiv(P.spsh);
    P.items_per_shard_div = make_fastdiv(std::max(1u, P.items_per_shard));
    P.order_window = std::min(P.items_per_shard, window);
    const uint32_t spans = (P.order_window + 1023u) / 1024u;
    const uint32_t sentinel = 0xfffffffeu;
    std::vector<uint32_t> list((size_t)n_sh * P.order_window, sentinel);
    std::vector<unsigned int> cnt((size_t)n_sh * C.n * 32, 0u);
    const dim3 grid(n_sh * spans), block(64); // one wave per block
    if (ring) {
        hipLaunchKernelGGL(k_order_items<true, false>, grid, block, 0, nullptr, P, C, list.data(), cnt.data());
        hipLaunchKernelGGL(k_order_items<true, true>, grid, block, 0, nullptr, P, C, list.data(), cnt.data());
    } else {
        hipLaunchKernelGGL(k_order_items<false, false>, grid, block, 0, nullptr, P, C, list.data(), cnt.data());
        hipLaunchKernelGGL(k_order_items<false, true>, grid, block, 0, nullptr, P, C, list.data(), cnt.data());
    }
    const uint32_t cap = C.lo[C.n - 1];
    for (uint32_t sh = 0; sh < n_sh; sh++) {
        const uint32_t slo = sh * P.items_per_shard;
        const uint32_t* out = list.data() + (size_t)sh * P.order_window;
        if (slo >= P.n_items) { // the shard has no items: nothing of its part is written
            for (uint32_t q = 0; q < P.order_window; q++) CHECK(out[q] == sentinel, "shard %u is empty, entry %u was written", sh, q);
            continue;
        }
        const uint32_t hi = std::min(slo + P.items_per_shard, P.n_items), lo = hi - std::min(P.order_window, hi - slo), wn = hi - lo;
        const uint32_t n_spans = (wn + 1023u) / 1024u;
        std::vector<uint8_t> seen(wn, 0), left((size_t)C.n * n_spans, 0);
        uint32_t prev_cls = C.n, prev_item = 0, first_short = wn;
        bool prev_ok = false;
        for (uint32_t q = 0; q < wn; q++) {
            const uint32_t item = out[q];
            CHECK(item >= lo && item < hi, "shard %u entry %u is %u, outside the window [%u, %u)", sh, q, item, lo, hi);
            if (item < lo || item >= hi) { prev_ok = false; continue; }
            CHECK(!seen[item - lo], "shard %u lists item %u twice", sh, item);
            seen[item - lo] = 1;
            uint32_t pixel_index = 0, k = 0;
            const bool valid = restated_item(P, ring, item, pixel_index, k);
            uint32_t len = 1;
            if (valid) {
                len = stepped_length(seed, pixel_index, k, p_rr);
                CHECK(len == drawn_length(seed, pixel_index, k, p_rr), "item %u: stepping roulette() gives %u vertices, the draws another number", item, len);
                CHECK(roulette_length(seed, pixel_index, k, p_rr, cap) == std::min(len, cap), "item %u: roulette_length capped at %u is not min(%u, cap)", item, cap, len);
            }
            const uint32_t cls = restated_class(C, len);
            CHECK(cls <= prev_cls, "shard %u entry %u: class %u follows class %u", sh, q, cls, prev_cls);
            if ((!valid || len == 1) && first_short == wn) first_short = q;
            if (q > first_short) CHECK(!valid || len == 1, "shard %u entry %u: a path of %u vertices behind a padding slot or a one-vertex path", sh, q, len);
            // inside a class the items of a span stay together and in item order
            if (prev_ok && cls == prev_cls && (item - lo) / 1024u == (prev_item - lo) / 1024u) CHECK(item > prev_item, "shard %u entry %u: item %u follows %u of its span", sh, q, item, prev_item);
            // ... and a span that was left does not come back within the class
            if (prev_ok && cls == prev_cls && (item - lo) / 1024u != (prev_item - lo) / 1024u) left[(size_t)cls * n_spans + (prev_item - lo) / 1024u] = 1;
            CHECK(!left[(size_t)cls * n_spans + (item - lo) / 1024u], "shard %u entry %u: the span of item %u is split inside class %u", sh, q, item, cls);
            prev_cls = cls; prev_item = item; prev_ok = true;
        }
        for (uint32_t q = 0; q < wn; q++) CHECK(seen[q], "shard %u never lists item %u", sh, lo + q);
        for (uint32_t q = wn; q < P.order_window; q++) CHECK(out[q] == sentinel, "shard %u: entry %u beyond its %u items was written", sh, q, wn);
    }
}

int main()
{
    // roulette_length against roulette() stepped depth by depth, over seeds, p_rr values and caps (p_rr 1: the bounce stack's limit)
    for (uint64_t seed : {0ull, 1ull, 0x9e3779b97f4a7c15ull})
        for (float p_rr : {0.0f, 0.3f, 0.6f, 0.95f, 1.0f})
            for (uint32_t pixel = 0; pixel < 40; pixel++) {
                const uint32_t len = stepped_length(seed, pixel * 977u, pixel % 7u, p_rr);
                CHECK(len == drawn_length(seed, pixel * 977u, pixel % 7u, p_rr), "stepped and drawn lengths differ");
                CHECK(len >= 1 && len <= CRT_BOUNCE_STACK_SIZE, "length %u", len);
                if (p_rr == 0.0f) CHECK(len == 1, "p_rr 0 stops every path at its first vertex");
                if (p_rr == 1.0f) CHECK(len == CRT_BOUNCE_STACK_SIZE, "p_rr 1 stops no path before the stack is full");
                for (uint32_t cap : {1u, 2u, 5u, 9u, 64u}) CHECK(roulette_length(seed, pixel * 977u, pixel % 7u, p_rr, cap) == std::min(len, cap), "cap %u", cap);
            }
    const OrderClasses two{2, {1, 2}}, five{5, {1, 2, 3, 5, 9}}, eight{8, {1, 2, 3, 4, 5, 7, 9, 13}};
    int cases = 0;
    // 52 x 44: ragged tiles in both directions (padding slots); 5 samples over 3 shards: 7 x 6 tiles x 64 x 5 = 13 440 items, 4 480 per shard
    // = 4 spans and 384 items; windows smaller than a shard (1 000: not a whole span; 2 048), equal to it and larger
    for (uint32_t window : {1000u, 2048u, 4480u, 1u << 19})
        for (const OrderClasses* C : {&two, &five, &eight}) { run_case(52, 44, 0, 1, 0, 5, 3, false, window, *C, 1, 0.6f); cases++; }
    // other seeds and p_rr values (0: every path one vertex; 1: every path the longest class), a later first sample
    for (float p_rr : {0.0f, 0.3f, 0.95f, 1.0f}) { run_case(52, 44, 0, 1, 7, 3, 3, false, 1u << 19, five, 0xabcdef12345ull + (uint64_t)(p_rr * 10), p_rr); cases++; }
    // rank 3 of 8 (its last tile lies beyond the frame), one pixel, a frame smaller than a span, more shards than there are items for
    run_case(52, 44, 3, 8, 0, 9, 3, false, 1000, five, 5, 0.6f); cases++;
    run_case(1, 1, 0, 1, 0, 3, 3, false, 1u << 19, five, 5, 0.6f); cases++;
    run_case(13, 9, 0, 1, 0, 1, 4, false, 1u << 19, eight, 6, 0.6f); cases++;
    // the commit ring's cursor shards (ranges of pixel slots, sample-major): 4 shards of 704 slots (the last one partly beyond the frame's slots)
    for (uint32_t window : {1000u, 704u * 3u, 1u << 19}) { run_case(52, 44, 0, 1, 0, 6, 4, true, window, five, 9, 0.6f); cases++; }
    run_case(52, 44, 1, 2, 2, 4, 4, true, 1u << 19, two, 9, 0.8f); cases++;
    std::printf("%d cases, %d failures\n", cases, g_fail);
    return g_fail ? 1 : 0;
}
