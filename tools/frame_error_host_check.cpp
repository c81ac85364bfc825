// tools/frame_error_host_check.cpp -- the device text of crt_frame_error (cudaraytracing_amd/csrc/crt_frame_error.h) compiled for the
// HOST and run on synthetic sums against a plain restatement of the contract (include/crt.h), for AddressSanitizer / UBSan runs without
// a device.  tools/host_device.h stands in for the device: a wave is 64 host threads that meet at a barrier in every cross-lane
// operation, a block's waves run one after another, LDS is a static array.  The two kernels here are the two of crt_frame_error.hip:
// the same bodies.  The sums hold NaN and +-inf in c and in q; the slot counts lie on both sides of 64, 256 and 64 x 256; one frame is a
// tiled shard with padding slots.  Every buffer is sized exactly, so an access one element out is a report.
// With an argument the program writes every summary it checked to that file: the plain and the sanitised build write the same bytes.
//
// tests/test_frame_error.py builds and runs it:
//   g++ -std=c++17 -ffp-contract=off -I cudaraytracing_amd/csrc -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       -pthread tools/frame_error_host_check.cpp -o /tmp/frame_error_host_check && /tmp/frame_error_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#define CRT_HOST_WAVES
#include "host_device.h"

#include "../include/crt.h"
#include "crt_stages.h"
#include "crt_frame_error.h"

using namespace crtk;

namespace crtk {
__global__ void k_frame_error_blocks(const FrameErrorParams D) { frame_error_block(D); }
__global__ void k_frame_error_finish(const FrameErrorParams D) { frame_error_finish(D); }
void launch_frame_error(const FrameErrorParams& D, hipStream_t st)
{
    hipLaunchKernelGGL(k_frame_error_blocks, dim3(D.n_blocks), dim3(256), 0, st, D);
    hipLaunchKernelGGL(k_frame_error_finish, dim3(kFeQuantities), dim3(64), 0, st, D);
}
} // namespace crtk

static int g_fail = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fail++; } \
    } while (0)

static unsigned long long bits_of(double d) { unsigned long long u; std::memcpy(&u, &d, 8); return u; }

// ---- the contract, restated plainly ----
// the tree of step 2 (and 5) on 64 values
static double tree64(const double* v)
{
    double x[64];
    for (int t = 0; t < 64; t++) x[t] = v[t];
    for (int s = 32; s >= 1; s /= 2)
        for (int t = 0; t < s; t++) x[t] = x[t] + x[t + s];
    return x[0];
}
// the sum of per-slot values in the contract's order
static double ordered_sum(std::vector<double> v)
{
    const size_t nb = (v.size() + 255) / 256;
    v.resize(nb * 256, 0.0);
    std::vector<double> P(nb);
    for (size_t b = 0; b < nb; b++) {
        double w[4];
        for (int g = 0; g < 4; g++) w[g] = tree64(&v[b * 256 + g * 64]);
        P[b] = ((w[0] + w[1]) + w[2]) + w[3];
    }
    double lane[64];
    for (size_t l = 0; l < 64; l++) {
        lane[l] = 0.0;
        for (size_t i = l; i < nb; i += 64) lane[l] = lane[l] + P[i];
    }
    return tree64(lane);
}

static crt_frame_error_info restated(const std::vector<float>& c3, const std::vector<float>& q3, uint32_t w, uint32_t h, uint32_t rank, uint32_t world, uint32_t nslots,
                                     uint32_t n, uint32_t S, float thr, float floor_)
{
    crt_frame_error_info E;
    std::memset(&E, 0, sizeof(E));
    E.samples_done = n; E.spp = S;
    const uint32_t tiles_x = (w + 7) / 8, n_tiles = tiles_x * ((h + 7) / 8);
    std::vector<double> sv(nslots, 0.0), sm(nslots, 0.0);
    for (uint32_t slot = 0; slot < nslots; slot++) {
        const uint32_t tile = (slot / 64) * world + rank, pix = slot % 64;
        if (tile >= n_tiles || (tile % tiles_x) * 8 + pix % 8 >= w || (tile / tiles_x) * 8 + pix / 8 >= h) continue;
        E.pixels++;
        const float fn = (float)n, r = (float)S / fn;
        float v3[3], p3[3];
        for (int ch = 0; ch < 3; ch++) {
            const float c = c3[(size_t)ch * nslots + slot], q = q3[(size_t)ch * nslots + slot];
            const float d = fn * q - c * c;
            v3[ch] = ((r * r) * (d < 0.0f ? 0.0f : d)) / (fn - 1.0f);
            p3[ch] = c * r;
        }
        const float v = (v3[0] + v3[1]) + v3[2], m = (p3[0] + p3[1]) + p3[2];
        const float t = thr * (m + floor_), tt = t * t;
        if (!(v <= tt)) E.above++;
        if (std::isnan(v) || std::isnan(tt)) { E.nan_pixels++; continue; }
        int bin = 0;
        for (int j = 0; j < 15; j++) bin += v > tt * std::ldexp(1.0f, 2 * (j - 7));
        E.hist[bin]++;
        sv[slot] = (double)v; sm[slot] = (double)m;
    }
    E.sum_variance = ordered_sum(sv); E.sum_mean = ordered_sum(sm);
    return E;
}

static std::vector<crt_frame_error_info> g_all;

static void run_case(uint32_t w, uint32_t h, uint32_t rank, uint32_t world, uint32_t n, uint32_t S, float thr, float floor_, bool specials)
{
    FrameErrorParams D{};
    AParams& A = D.A;
    A.width = w; A.height = h; A.rank = rank; A.world = world; A.tiles_x = (w + 7) / 8; A.n_tiles = A.tiles_x * ((h + 7) / 8);
    A.nslots = (A.n_tiles + world - 1) / world * 64; A.tiled_output = world > 1; A.tiles_x_div = make_fastdiv(A.tiles_x); A.spp = S;
    const uint32_t nslots = A.nslots;
    std::vector<float> accum((size_t)nslots * 3), qacc((size_t)nslots * 3);
    std::srand(w * 131 + h * 17 + S + rank);
    auto rnd = [] { return (float)(1 + std::rand() % 1000) / 250.0f; };
    // n samples' worth of sums at every slot, padding included (a padding slot's sums must count for nothing whatever they hold)
    for (size_t k = 0; k < accum.size(); k++) {
        accum[k] = qacc[k] = 0.0f;
        const float scale = (k % 7 == 0) ? 0.01f : 1.0f; // (some pixels much quieter than others: several bins)
        for (uint32_t s = 0; s < n; s++) { const float x = (1.0f + scale * rnd()) / (float)S; accum[k] = accum[k] + x; qacc[k] = qacc[k] + x * x; }
    }
    if (specials) {
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        const float sp[6] = {nan, inf, -inf, 0.0f, -0.0f, 3.0e38f};
        for (size_t k = 0; k < accum.size(); k += 5) accum[k] = sp[(k / 5) % 6];
        for (size_t k = 3; k < qacc.size(); k += 11) qacc[k] = sp[(k / 11) % 6];
    }
    D.qacc = qacc.data(); A.accum = accum.data();
    D.n = n; D.threshold = thr; D.mean_floor = floor_;
    D.n_blocks = slot_grid(A).x;
    std::vector<double> part_sum((size_t)kFeSums * D.n_blocks, -1.0);
    std::vector<uint32_t> part_cnt((size_t)kFeCounts * D.n_blocks, 0xdeadbeefu);
    crt_frame_error_info got;
    std::memset(&got, 0xa5, sizeof(got));
    D.part_sum = part_sum.data(); D.part_cnt = part_cnt.data(); D.out = &got;
    launch_frame_error(D, nullptr);
    const crt_frame_error_info want = restated(accum, qacc, w, h, rank, world, nslots, n, S, thr, floor_);
    const char* fmt = "%ux%u rank %u/%u n %u thr %g: %s is %llu, expected %llu";
#define SAME(f) CHECK(got.f == want.f, fmt, w, h, rank, world, n, (double)thr, #f, (unsigned long long)got.f, (unsigned long long)want.f)
    SAME(samples_done); SAME(spp); SAME(pixels); SAME(nan_pixels); SAME(above);
    for (int b = 0; b < 16; b++) SAME(hist[b]);
#undef SAME
    CHECK(bits_of(got.sum_variance) == bits_of(want.sum_variance), "%ux%u rank %u/%u n %u thr %g: sum_variance is %a, expected %a", w, h, rank, world, n, (double)thr,
          got.sum_variance, want.sum_variance);
    CHECK(bits_of(got.sum_mean) == bits_of(want.sum_mean), "%ux%u rank %u/%u n %u thr %g: sum_mean is %a, expected %a", w, h, rank, world, n, (double)thr, got.sum_mean,
          want.sum_mean);
    // the identities of the contract, of the kernels' own output
    uint64_t hs = 0, hi = 0;
    for (int b = 0; b < 16; b++) { hs += got.hist[b]; if (b >= 8) hi += got.hist[b]; }
    CHECK(hs + got.nan_pixels == got.pixels, "the bins and the NaN pixels do not add up to the pixels");
    CHECK(hi + got.nan_pixels == got.above, "above is not the upper bins and the NaN pixels");
    g_all.push_back(got);
}

int main(int argc, char** argv)
{
    // 1, 2, 3, 4, 5 tiles (64 .. 320 slots, around 64 and 256), 255 and 257 tiles (around 64 x 256 slots: 64 blocks, a partial for every
    // lane of the finishing wave, and 65, lane 0 two), most with ragged tiles
    const uint32_t shapes[][2] = {{1, 1}, {7, 5}, {8, 8}, {13, 5}, {17, 7}, {30, 8}, {32, 8}, {35, 3}, {2035, 7}, {2051, 5}};
    const float inf = std::numeric_limits<float>::infinity();
    int cases = 0;
    for (const auto& sh : shapes) {
        const bool big = sh[0] > 1000;
        run_case(sh[0], sh[1], 0, 1, 3, 8, 0.05f, 0.01f, true); cases++;
        if (big) continue; // (a big frame is 16 000 slots of host threads: once)
        run_case(sh[0], sh[1], 0, 1, 8, 8, 0.05f, 0.01f, false); cases++;
        for (float thr : {0.0f, 0.002f, 3.0f, inf}) { run_case(sh[0], sh[1], 0, 1, 2, 29, thr, 0.0f, true); cases++; }
    }
    // a tiled shard with padding: rank 1 of 3 of 61 x 47 (48 tiles: 16 each; ragged right and bottom), and one whose last tile is beyond the frame
    for (bool specials : {false, true}) { run_case(61, 47, 1, 3, 3, 8, 0.05f, 0.01f, specials); cases++; }
    run_case(20, 9, 2, 4, 5, 16, 0.01f, 0.01f, true); cases++;
    if (argc > 1) {
        std::FILE* f = std::fopen(argv[1], "wb");
        if (!f || std::fwrite(g_all.data(), sizeof(crt_frame_error_info), g_all.size(), f) != g_all.size()) { std::printf("cannot write %s\n", argv[1]); return 2; }
        std::fclose(f);
    }
    std::printf("%d cases, %d failures\n", cases, g_fail);
    return g_fail ? 1 : 0;
}
