// tools/sample_map_host_check.cpp -- the kernels of cudaraytracing_amd/csrc/crt_sample_map.hip and crt_adaptive.hip compiled for the HOST
// and run against plain restatements, for AddressSanitizer / UBSan runs without a device.  The kernel files and the stages they share
// (crt_stages.h) are included as they are; tools/host_device.h stands in for what they take from crt_path.h and crt_device.h and for the
// device's launch indices, wave intrinsics and atomics.  A wave is 64 host threads that meet at a barrier in every cross-lane
// operation, so a ballot sees all its lanes' predicates as the hardware's does; a block is run wave after wave.
// Every buffer is sized exactly (std::vector of the element count the host code allocates), so an access one element out is a report.
//
// tests/test_host_checks.py builds and runs it:
//   g++ -std=c++17 -ffp-contract=off -I cudaraytracing_amd/csrc -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       -pthread tools/sample_map_host_check.cpp -o /tmp/sample_map_host_check && /tmp/sample_map_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#define CRT_INTERNAL_H // (the kernel files' only include: replaced by host_device.h)
#define CRT_HOST_WAVES
#include "host_device.h"

#include "crt_stages.h"
#include "crt_adaptive.hip"
#include "crt_sample_map.hip"

using namespace crtk;

static int g_fail = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fail++; } \
    } while (0)

static bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }

// The slot map of shard rank / world of a w x h frame of cap S
static AParams frame_of(uint32_t w, uint32_t h, uint32_t S, uint32_t rank, uint32_t world)
{
    AParams A{};
    A.width = w; A.height = h; A.rank = rank; A.world = world; A.tiles_x = (w + 7) / 8; A.n_tiles = A.tiles_x * ((h + 7) / 8);
    A.nslots = (A.n_tiles + world - 1) / world * 64; A.tiled_output = world > 1; A.tiles_x_div = make_fastdiv(A.tiles_x); A.spp = S;
    return A;
}

// ---- plain restatements, on planes c3 / q3 of nslots floats per channel ----
// the stop criterion at a slot whose sums hold n of S samples: (v, t * t)
static void restated_criterion(const std::vector<float>& c3, const std::vector<float>& q3, uint32_t nslots, uint32_t slot, uint32_t n, uint32_t S, float thr, float floor_,
                               float& v, float& tt)
{
    const float fn = (float)n, r = (float)S / fn;
    float v3[3], p3[3];
    for (int ch = 0; ch < 3; ch++) {
        const float c = c3[(size_t)ch * nslots + slot], q = q3[(size_t)ch * nslots + slot];
        const float d = fn * q - c * c;
        v3[ch] = ((r * r) * (d < 0.0f ? 0.0f : d)) / (fn - 1.0f);
        p3[ch] = c * r;
    }
    v = (v3[0] + v3[1]) + v3[2];
    const float t = thr * (((p3[0] + p3[1]) + p3[2]) + floor_);
    tt = t * t;
}
// the first `count` samples of the chunk L into the sums of a slot
static void restated_fold(std::vector<float>& c3, std::vector<float>& q3, const std::vector<Rad3>& L, uint32_t nslots, uint32_t slot, uint32_t count, uint32_t S)
{
    for (int ch = 0; ch < 3; ch++)
        for (uint32_t s = 0; s < count; s++) {
            const Rad3& l = L[(size_t)s * nslots + slot];
            const float x = (ch == 0 ? l.x : ch == 1 ? l.y : l.z) / (float)S;
            c3[(size_t)ch * nslots + slot] = c3[(size_t)ch * nslots + slot] + x;
            q3[(size_t)ch * nslots + slot] = q3[(size_t)ch * nslots + slot] + x * x;
        }
}

// One frame of w x h, cap S, as shard rank / world, from sample_begin, in chunks of `chunk` samples: every kernel against its restatement
static void run_case(uint32_t w, uint32_t h, uint32_t S, uint32_t rank, uint32_t world, uint32_t sample_begin, uint32_t chunk)
{
    MapParams D{};
    AParams& A = D.sums.A;
    A = frame_of(w, h, S, rank, world);
    const uint32_t tiles_x = A.tiles_x, n_tiles = A.n_tiles, nslots = A.nslots;
    std::vector<uint32_t> map((size_t)w * h), nsamp(nslots, 0xdeadbeefu);
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) map[(size_t)y * w + x] = (7 * x + 3 * y * y) % (S + 3);
    std::vector<unsigned int> hist(S + 1, 0u), cursor(S, 0u);
    std::vector<float> accum((size_t)nslots * 3), qacc((size_t)nslots * 3);
    // the sums of samples [0, sample_begin): made-up values, as a range would have left them
    std::srand(w * 131 + h * 17 + S);
    auto rnd = [] { return (float)(std::rand() % 1000) / 250.0f; };
    for (float& v : accum) v = sample_begin ? rnd() : -7.0f; // (from sample 0 the first chunk must overwrite them)
    for (float& v : qacc) v = sample_begin ? rnd() : -7.0f;
    std::vector<float> c_ref = accum, q_ref = qacc;
    D.sums.qacc = qacc.data(); D.sums.nsamp = nsamp.data(); D.map = map.data(); D.hist = hist.data(); D.cursor = cursor.data(); A.accum = accum.data();
    D.sample_begin = sample_begin;
    launch_map_prepare(D, nullptr);
    // restated counts and histogram
    std::vector<uint32_t> np(nslots, 0u), hist_ref(S + 1, 0u);
    for (uint32_t slot = 0; slot < nslots; slot++) {
        uint32_t i = 0, j = 0;
        const uint32_t tile = (slot / 64) * world + rank, pix = slot % 64;
        const bool valid = tile < n_tiles && (i = (tile % tiles_x) * 8 + pix % 8) < w && (j = (tile / tiles_x) * 8 + pix / 8) < h;
        if (valid) np[slot] = std::min(std::max(map[(size_t)j * w + i], std::max(sample_begin, 1u)), S);
        hist_ref[np[slot]]++;
        CHECK(nsamp[slot] == np[slot], "%ux%u S %u: n_p of slot %u is %u, expected %u", w, h, S, slot, nsamp[slot], np[slot]);
    }
    for (uint32_t v = 0; v <= S; v++) CHECK(hist[v] == hist_ref[v], "%ux%u S %u: histogram[%u] is %u, expected %u", w, h, S, v, hist[v], hist_ref[v]);
    uint32_t max_np = 0;
    for (uint32_t v = 1; v <= S; v++)
        if (hist[v]) max_np = v;
    std::vector<uint32_t> count(S, 0u); // slots with n_p > s
    for (uint32_t s = 0; s < S; s++)
        for (uint32_t slot = 0; slot < nslots; slot++) count[s] += np[slot] > s;
    for (uint32_t s0 = sample_begin; s0 < max_np; s0 += chunk) {
        const uint32_t ns = std::min(chunk, max_np - s0);
        uint32_t n_items = 0;
        for (uint32_t s = s0; s < s0 + ns; s++) { cursor[s] = n_items; n_items += count[s]; }
        std::vector<uint32_t> list(n_items, 0xffffffffu); // exactly the chunk's work items
        std::vector<Rad3> L((size_t)ns * nslots);        // dense per chunk
        for (Rad3& l : L) l = Rad3{rnd(), rnd(), rnd()};
        D.item_list = list.data(); D.n_items = n_items; D.s0 = s0; D.ns = ns;
        launch_map_items(D, nullptr);
        // sample-major, every (sample, slot) that takes the sample exactly once
        std::vector<uint8_t> seen((size_t)ns * nslots, 0);
        uint32_t pos = 0;
        for (uint32_t s = s0; s < s0 + ns; s++)
            for (uint32_t k = 0; k < count[s]; k++, pos++) {
                const uint32_t item = list[pos];
                CHECK(item < ns * nslots, "item %u of the list is %u, outside L", pos, item);
                if (item >= ns * nslots) continue;
                CHECK(item / nslots == s - s0, "position %u holds sample %u in the run of sample %u", pos, item / nslots + s0, s);
                CHECK(np[item % nslots] > s, "position %u names slot %u, which does not take sample %u", pos, item % nslots, s);
                CHECK(!seen[item], "work item %u is listed twice", item);
                seen[item] = 1;
            }
        CHECK(pos == n_items, "list length");
        uint32_t end = 0; // every sample's cursor has moved from its first position to its last + 1
        for (uint32_t s = s0; s < s0 + ns; s++) { end += count[s]; CHECK(cursor[s] == end, "cursor of sample %u is %u, expected %u", s, cursor[s], end); }
        A.L = L.data(); A.first_chunk = s0 == 0;
        launch_map_fold(D.sums, s0, ns, nullptr);
        if (s0 == 0) { std::fill(c_ref.begin(), c_ref.end(), 0.0f); std::fill(q_ref.begin(), q_ref.end(), 0.0f); }
        for (uint32_t slot = 0; slot < nslots; slot++) restated_fold(c_ref, q_ref, L, nslots, slot, np[slot] > s0 ? std::min(np[slot] - s0, ns) : 0u, S);
    }
    if (max_np > sample_begin)
        for (size_t k = 0; k < accum.size(); k++)
            CHECK(same_bits(accum[k], c_ref[k]) && same_bits(qacc[k], q_ref[k]), "%ux%u S %u: sums of plane entry %zu differ", w, h, S, k);
    // the plan, at n = 2 samples' worth of sums (whatever the sums hold: the formula is what is compared), in the frame's output layout
    if (S >= 2) {
        const uint32_t n = 2, n_out = A.tiled_output ? nslots : w * h;
        std::vector<uint32_t> out(n_out, 0xdeadbeefu);
        for (float thr : {0.0f, 0.2f, 3.0f, INFINITY}) {
            D.n = n; D.threshold = thr; D.mean_floor = 0.01f; D.out_map = out.data();
            launch_sample_plan(D, nullptr);
            for (uint32_t slot = 0; slot < nslots; slot++) {
                const SlotPixel px = slot_pixel(A, slot);
                if (!px.out) continue;
                uint32_t want = 0;
                if (px.valid) {
                    float v, tt;
                    restated_criterion(accum, qacc, nslots, slot, n, S, thr, 0.01f, v, tt);
                    const float fs = (float)S, wv = ((float)n * v) / tt;
                    want = wv < fs ? std::max(n, (uint32_t)std::ceil(wv)) : S;
                }
                CHECK(out[px.o] == want, "%ux%u S %u threshold %g: plan of slot %u is %u, expected %u", w, h, S, thr, slot, out[px.o], want);
            }
        }
    }
}

// crt_render_adaptive's device side over two passes of `step` samples after a warm-up of n0, each pass in chunks of `chunk` samples:
// counts after the warm-up (k_adaptive_init), k_adaptive_select, k_adaptive_items, k_map_fold -- against a restatement that keeps an explicit `active` array and writes a slot's count after every chunk it took
static void run_adaptive_case(uint32_t w, uint32_t h, uint32_t S, uint32_t rank, uint32_t world, float thr, uint32_t n0, uint32_t step, uint32_t chunk)
{
    const float floor_ = 0.01f;
    AdaptiveParams D{};
    AParams& A = D.sums.A;
    A = frame_of(w, h, S, rank, world);
    const uint32_t nslots = A.nslots;
    std::vector<uint32_t> nsamp(nslots, 0xdeadbeefu), list(nslots, 0xffffffffu);
    std::vector<unsigned int> counter(1, 0u);
    std::vector<float> accum((size_t)nslots * 3, 0.0f), qacc((size_t)nslots * 3, 0.0f);
    std::srand(w * 131 + h * 17 + S + rank);
    auto rnd = [] { return (float)(1 + std::rand() % 1000) / 250.0f; };
    // the warm-up's sums, of every slot as the uniform fold leaves them: n0 samples that differ, so every variance is positive
    for (uint32_t s = 0; s < n0; s++)
        for (size_t k = 0; k < accum.size(); k++) { const float x = rnd() / (float)S; accum[k] = accum[k] + x; qacc[k] = qacc[k] + x * x; }
    std::vector<float> c_ref = accum, q_ref = qacc;
    A.accum = accum.data(); D.sums.qacc = qacc.data(); D.sums.nsamp = nsamp.data(); D.list = list.data(); D.count = counter.data();
    D.threshold = thr; D.mean_floor = floor_; D.n = n0;
    launch_adaptive_init(D, nullptr);
    std::vector<uint8_t> active(nslots, 0);
    std::vector<uint32_t> n_ref(nslots, 0u);
    for (uint32_t slot = 0; slot < nslots; slot++) {
        active[slot] = slot_pixel(A, slot).valid; n_ref[slot] = active[slot] ? n0 : 0u;
        CHECK(nsamp[slot] == n_ref[slot], "init: n_p of slot %u is %u, expected %u", slot, nsamp[slot], n_ref[slot]);
    }
    const size_t pixels = (size_t)std::count(active.begin(), active.end(), 1);
    uint32_t n = n0;
    for (int pass = 0; pass < 2 && n < S; pass++) {
        const uint32_t ns_pass = std::min(step, S - n);
        counter[0] = 0u; D.n = n; D.ns_pass = ns_pass;
        launch_adaptive_select(D, nullptr);
        std::set<uint32_t> on;
        for (uint32_t slot = 0; slot < nslots; slot++) {
            if (!active[slot]) continue;
            float v, tt;
            restated_criterion(c_ref, q_ref, nslots, slot, n, S, thr, floor_, v, tt);
            if (v <= tt) active[slot] = 0;
            else on.insert(slot);
        }
        // what the two extreme thresholds are there for, of the restatement itself: +inf stops every pixel at the first select, 0 none ever
        if (thr == INFINITY) CHECK(on.empty(), "pass %d: %zu slots go on at threshold +inf", pass, on.size());
        if (thr == 0.0f) CHECK(on.size() == pixels, "pass %d: %zu of the shard's %zu pixels go on at threshold 0", pass, on.size(), pixels);
        const uint32_t n_active = counter[0];
        CHECK(n_active == on.size(), "pass %d: %u slots go on, expected %zu", pass, n_active, on.size());
        if (n_active != on.size()) return;
        std::set<uint32_t> listed(list.begin(), list.begin() + n_active);
        CHECK(listed == on, "pass %d: the list does not name the active slots once each", pass);
        if (n_active == 0) break;
        for (uint32_t s0 = n; s0 < n + ns_pass; s0 += chunk) {
            const uint32_t ns = std::min(chunk, n + ns_pass - s0), n_items = ns * n_active;
            std::vector<uint32_t> items(n_items, 0xffffffffu); // exactly the chunk's work items
            launch_adaptive_items(items.data(), list.data(), n_active, n_items, nslots, nullptr);
            for (uint32_t pos = 0; pos < n_items; pos++)
                CHECK(items[pos] == (pos / n_active) * nslots + list[pos % n_active], "pass %d: item %u of the list is %u", pass, pos, items[pos]);
            std::vector<Rad3> L((size_t)ns * nslots); // dense per chunk
            for (Rad3& l : L) l = Rad3{rnd(), rnd(), rnd()};
            A.L = L.data(); A.first_chunk = 0; A.chunk_samples = ns;
            launch_map_fold(D.sums, s0, ns, nullptr);
            for (uint32_t slot = 0; slot < nslots; slot++) {
                if (!active[slot]) continue;
                restated_fold(c_ref, q_ref, L, nslots, slot, ns, S);
                n_ref[slot] = s0 + ns;
            }
        }
        n += ns_pass;
        for (uint32_t slot = 0; slot < nslots; slot++) CHECK(nsamp[slot] == n_ref[slot], "pass %d: n_p of slot %u is %u, expected %u", pass, slot, nsamp[slot], n_ref[slot]);
        for (size_t k = 0; k < accum.size(); k++) CHECK(same_bits(accum[k], c_ref[k]) && same_bits(qacc[k], q_ref[k]), "pass %d: sums of plane entry %zu differ", pass, k);
    }
}

int main()
{
    const uint32_t shapes[4][2] = {{1, 1}, {5, 3}, {65, 5}, {37, 27}};
    int cases = 0;
    for (const auto& sh : shapes)
        for (uint32_t S : {1u, 2u, 29u}) {
            run_case(sh[0], sh[1], S, 0, 1, 0, S);                       // one chunk
            run_case(sh[0], sh[1], S, 0, 1, 0, 3);                       // chunks of three samples
            cases += 2;
            if (S > 4) { run_case(sh[0], sh[1], S, 0, 1, 4, 3); cases++; } // continuing a frame of four samples
            for (uint32_t rank = 0; rank < 2; rank++, cases++) run_case(sh[0], sh[1], S, rank, 2, 0, 3); // two tiled shards
        }
    // crt_render_adaptive's kernels, 13 x 9 (ragged tiles in both directions) of cap 12: a warm-up of 4, passes of 5 (the second cut to 3) in
    // chunks of 2; every pixel stops at the first select (+inf), none does (0), some do
    for (float thr : {INFINITY, 0.0f, 0.15f}) {
        run_adaptive_case(13, 9, 12, 0, 1, thr, 4, 5, 2);
        for (uint32_t rank = 0; rank < 2; rank++) run_adaptive_case(13, 9, 12, rank, 2, thr, 4, 5, 2);
        cases += 3;
    }
    std::printf("%d cases, %d failures\n", cases, g_fail);
    return g_fail ? 1 : 0;
}
