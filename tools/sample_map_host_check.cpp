// tools/sample_map_host_check.cpp -- the kernels of cudaraytracing_amd/csrc/crt_sample_map.hip compiled for the HOST and run against plain
// restatements, for AddressSanitizer / UBSan runs without a device.  The kernel file is included as it is; this file stands in for what
// it takes from crt_internal.h (the slot map, the sums' accessors, the sample fold, the variance formula: the same text) and for the
// device's launch indices, wave intrinsics and atomics.  A wave is 64 host threads that meet at a barrier in every cross-lane operation,
// so a ballot sees all its lanes' predicates as the hardware's does; a block is run wave after wave.
// Every buffer is sized exactly (std::vector of the element count the host code allocates), so an access one element out is a report.
//
//   g++ -std=c++17 -O1 -g -pthread -ffp-contract=off -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       -I cudaraytracing_amd/csrc tools/sample_map_host_check.cpp -o /tmp/sample_map_host_check && /tmp/sample_map_host_check
#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "crt_fastdiv.h"

// ---- stand-ins for the device ----
#define CRT_INTERNAL_H // (crt_sample_map.hip's only include: replaced by what follows)
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(n)
#define CRT_TILE 8
struct Idx { uint32_t x; };
static thread_local Idx blockIdx, threadIdx;
struct dim3 { uint32_t x; dim3(uint32_t x_ = 1) : x(x_) {} };
typedef void* hipStream_t;

struct Wave { // the 64 lanes of the wave that is running
    std::mutex m;
    std::condition_variable cv;
    int waiting = 0;
    unsigned long gen = 0;
    std::atomic<unsigned long long> bits{0};
    int vals[64];
    void barrier()
    {
        std::unique_lock<std::mutex> l(m);
        const unsigned long g = gen;
        if (++waiting == 64) { waiting = 0; gen++; cv.notify_all(); }
        else cv.wait(l, [&] { return gen != g; });
    }
};
static Wave g_wave;
static unsigned long long __ballot(bool p)
{
    const int lane = threadIdx.x & 63;
    if (p) g_wave.bits.fetch_or(1ull << lane);
    g_wave.barrier();
    const unsigned long long m = g_wave.bits.load();
    g_wave.barrier();
    if (lane == 0) g_wave.bits.store(0);
    g_wave.barrier();
    return m;
}
static int __builtin_amdgcn_readlane(int v, int lane_from)
{
    g_wave.vals[threadIdx.x & 63] = v;
    g_wave.barrier();
    const int r = g_wave.vals[lane_from];
    g_wave.barrier();
    return r;
}
static int __ffsll(long long v) { return __builtin_ffsll(v); }
static int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_load(p, order, scope) __atomic_load_n(p, order)
#define __hip_atomic_store(p, v, order, scope) __atomic_store_n(p, v, order)
#define __hip_atomic_fetch_add(p, v, order, scope) __atomic_fetch_add(p, v, order)
using std::max;
using std::min;
static float __uint_as_float(unsigned int u) { float f; std::memcpy(&f, &u, 4); return f; }
static unsigned int __float_as_uint(float f) { unsigned int u; std::memcpy(&u, &f, 4); return u; }

// a launch: block after block, wave after wave, 64 threads each
template <class K, class P> static void hipLaunchKernelGGL(K kernel, dim3 grid, dim3 block, int, hipStream_t, const P& params)
{
    for (uint32_t b = 0; b < grid.x; b++)
        for (uint32_t w0 = 0; w0 < block.x; w0 += 64) {
            std::vector<std::thread> lanes;
            for (uint32_t l = 0; l < 64; l++)
                lanes.emplace_back([=] { blockIdx.x = b; threadIdx.x = w0 + l; kernel(params); });
            for (std::thread& t : lanes) t.join();
        }
}

// ---- what crt_sample_map.hip takes from crt_internal.h / crt_path.h / crt_device.h: the same text ----
namespace crtk {
using crtdev::FastDiv;
using crtdev::make_fastdiv;
static uint32_t fast_div(uint32_t n, uint32_t m, uint32_t sh)
{
    const uint32_t t = (uint32_t)(((uint64_t)m * n) >> 32);
    return (t + ((n - t) >> (sh & 255u))) >> (sh >> 8);
}
struct F3 { float x, y, z; };
static F3 f3(float x, float y, float z) { return F3{x, y, z}; }
struct Rad3 { float x, y, z; };
static Rad3 load_radiance(const Rad3* p) { return *p; }
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
struct SlotMap {
    uint32_t width, height, rank, world, tiles_x, n_tiles, nslots, tiled_output;
    FastDiv tiles_x_div;
};
struct SlotPixel {
    bool valid, out;
    uint32_t i, j;
    uint64_t o;
};
static SlotPixel slot_pixel(const SlotMap& m, const uint32_t slot)
{
    SlotPixel p;
    p.i = 0; p.j = 0;
    p.valid = slot_to_pixel(slot, m.rank, m.world, m.n_tiles, m.tiles_x, m.tiles_x_div, m.width, m.height, p.i, p.j);
    p.out = p.valid || m.tiled_output;
    p.o = m.tiled_output ? (uint64_t)slot : (uint64_t)p.j * m.width + p.i;
    return p;
}
struct AParams : SlotMap {
    uint32_t spp;
    uint32_t chunk_samples;
    uint32_t first_chunk, last_chunk;
    const Rad3* L;
    float* accum;
    uint8_t* out_rgb;
    float* out_mean;
};
static float acc_load(const float* p) { return __uint_as_float(__hip_atomic_load((const unsigned int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); }
static void acc_store(float* p, const float v) { __hip_atomic_store((unsigned int*)p, __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
static F3 acc_load3(const float* planes, const uint32_t nslots, const uint32_t slot)
{
    return f3(acc_load(planes + slot), acc_load(planes + nslots + slot), acc_load(planes + 2ull * nslots + slot));
}
static void acc_store3(float* planes, const uint32_t nslots, const uint32_t slot, const F3 v)
{
    acc_store(planes + slot, v.x); acc_store(planes + nslots + slot, v.y); acc_store(planes + 2ull * nslots + slot, v.z);
}
template <bool VAR> static void fold_samples_n(const AParams& A, const uint32_t slot, const uint32_t count, F3& c, F3& q)
{
    const float fspp = (float)A.spp;
    const Rad3* lp = A.L + slot;
    for (uint32_t s = 0; s < count; s++, lp += A.nslots) {
        const Rad3 l = load_radiance(lp);
        const float xx = l.x / fspp, xy = l.y / fspp, xz = l.z / fspp;
        c.x = c.x + xx; c.y = c.y + xy; c.z = c.z + xz;
        if (VAR) { q.x = q.x + xx * xx; q.y = q.y + xy * xy; q.z = q.z + xz * xz; }
    }
}
static float variance_of(const float c, const float q, const float fn, const float rr)
{
    float d = fn * q - c * c;
    d = d < 0.0f ? 0.0f : d;
    return (rr * d) / (fn - 1.0f);
}
static F3 variance_of3(const F3 c, const F3 q, const float fn, const float rr)
{
    return f3(variance_of(c.x, q.x, fn, rr), variance_of(c.y, q.y, fn, rr), variance_of(c.z, q.z, fn, rr));
}
struct MapParams {
    AParams A;
    float* qacc;
    uint32_t* nsamp;
    const uint32_t* map;
    uint32_t map_per_slot;
    uint32_t sample_begin;
    unsigned int* hist;
    unsigned int* cursor;
    uint32_t* item_list;
    uint32_t n_items;
    uint32_t s0, ns;
    uint32_t n;
    float threshold, mean_floor;
    uint32_t* out_map;
};
} // namespace crtk

#include "crt_sample_map.hip"

using namespace crtk;

static int g_fail = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fail++; } \
    } while (0)

static bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }

// One frame of w x h, cap S, as shard rank / world, from sample_begin, in chunks of `chunk` samples: every kernel against its restatement
static void run_case(uint32_t w, uint32_t h, uint32_t S, uint32_t rank, uint32_t world, uint32_t sample_begin, uint32_t chunk)
{
    const uint32_t tiles_x = (w + 7) / 8, tiles_y = (h + 7) / 8, n_tiles = tiles_x * tiles_y, nslots = (n_tiles + world - 1) / world * 64;
    MapParams D;
    std::memset(&D, 0, sizeof(D));
    AParams& A = D.A;
    A.width = w; A.height = h; A.rank = rank; A.world = world; A.tiles_x = tiles_x; A.n_tiles = n_tiles; A.nslots = nslots;
    A.tiled_output = world > 1; A.tiles_x_div = make_fastdiv(tiles_x); A.spp = S;
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
    D.qacc = qacc.data(); D.nsamp = nsamp.data(); D.map = map.data(); D.hist = hist.data(); D.cursor = cursor.data(); A.accum = accum.data();
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
        launch_map_fold(D, nullptr);
        for (uint32_t slot = 0; slot < nslots; slot++)
            for (int ch = 0; ch < 3; ch++) {
                float& c = c_ref[(size_t)ch * nslots + slot];
                float& q = q_ref[(size_t)ch * nslots + slot];
                if (s0 == 0) { c = 0.0f; q = 0.0f; }
                for (uint32_t s = s0; s < s0 + ns && s < np[slot]; s++) {
                    const Rad3& l = L[(size_t)(s - s0) * nslots + slot];
                    const float x = (ch == 0 ? l.x : ch == 1 ? l.y : l.z) / (float)S;
                    c = c + x; q = q + x * x;
                }
            }
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
                    const float fn = (float)n, fs = (float)S, r = fs / fn, rr = r * r;
                    float v3[3], p3[3];
                    for (int ch = 0; ch < 3; ch++) {
                        const float c = accum[(size_t)ch * nslots + slot], q = qacc[(size_t)ch * nslots + slot];
                        float d = fn * q - c * c;
                        d = d < 0.0f ? 0.0f : d;
                        v3[ch] = (rr * d) / (fn - 1.0f);
                        p3[ch] = c * r;
                    }
                    const float v = (v3[0] + v3[1]) + v3[2], m = (p3[0] + p3[1]) + p3[2];
                    const float t = thr * (m + 0.01f), tt = t * t, wv = (fn * v) / tt;
                    want = wv < fs ? std::max(n, (uint32_t)std::ceil(wv)) : S;
                }
                CHECK(out[px.o] == want, "%ux%u S %u threshold %g: plan of slot %u is %u, expected %u", w, h, S, thr, slot, out[px.o], want);
            }
        }
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
    std::printf("%d cases, %d failures\n", cases, g_fail);
    return g_fail ? 1 : 0;
}
