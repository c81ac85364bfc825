// tools/select_host_check.cpp -- the two kernels of crt_filter_select (cudaraytracing_amd/csrc/crt_select.h) compiled for the HOST and run over
// the cases of a job file, for AddressSanitizer / UBSan runs without a device and for a bit comparison with the numpy restatement of
// include/crt.h (tests/test_filter_select.py).  crt_select.h and crt_stages.h (the tone map, write_color) are included as they are;
// tools/host_device.h stands in for what they take from outside.  The kernels (k_select_choose, k_select_blend,
// crt_select.hip) are their phases with a workgroup barrier in between; here a barrier is "every thread of the workgroup has run the
// phase": the same sequence as loops over the thread index.  The LDS arrays are std::vectors of exactly select_choose_lds_bytes /
// select_blend_lds_bytes, filled with NaN (0xff bytes) before a workgroup runs, and every image has exactly its entries: a staging, tap
// or output index one element out is a report, and a tap the staging did not write shows up in the comparison.
//
//   select_host_check JOB OUT
//   JOB: u32 cases; per case u32 width, height, K, r, s, outputs (bit 0 mean, 1 rgb, 2 choice, 3 error), then float32 images of
//        width x height x 3: half_a, half_b, half_variance, filtered_a[0 .. K), filtered_b[0 .. K)
//   OUT: per case mean (w h 3 f32), rgb (w h 3 u8), choice (w h u8), error (w h f32), chosen (4 u64); an output that was not asked for
//        keeps its fill (0x5a bytes)
//
// tests/test_filter_select.py builds it plain (-O2) and sanitised and runs both:
//   g++ -std=c++17 -ffp-contract=off -I cudaraytracing_amd/csrc -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       tools/select_host_check.cpp -o /tmp/select_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_device.h"

#include "crt_stages.h"
#include "crt_select.h"

using namespace crtk;

static int g_fail = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); g_fail++; } \
    } while (0)

// k_select_choose of crt_select.hip, a barrier = the end of a loop over the workgroup's threads
static void choose_block(const SelParams& P, const uint32_t block, unsigned long long* chosen)
{
    const SelTile T = select_tile(P, block);
    std::vector<float> lds(select_choose_lds_bytes(P) / 4u);
    std::memset(lds.data(), 0xff, lds.size() * 4u);
    for (int tid = 0; tid < 256; tid++) select_stage_errors(P, T, tid, lds.data());
    for (int tid = 0; tid < 256; tid++) select_row_sums(P, T, tid, lds.data());
    for (int tid = 0; tid < 256; tid++) {
        const int tx = tid & (int)(kSelectTileW - 1u), ty = tid / (int)kSelectTileW;
        if (T.x0 + tx < (int)P.width && T.y0 + ty < (int)P.height) {
            const int best = select_choose_pixel(P, T, tx, ty, lds.data());
            CHECK(best >= 0 && best < P.K, "block %u: choice %d of %d candidates", block, best, P.K);
            if (best >= 0 && best < kSelectMaxK) chosen[best]++;
        }
    }
}

static void blend_block(const SelParams& P, const uint32_t block)
{
    const SelTile T = select_tile(P, block);
    std::vector<uint8_t> cl(select_blend_lds_bytes(P), 0xa5);
    for (int tid = 0; tid < 256; tid++) select_stage_choice(P, T, tid, cl.data());
    for (int tid = 0; tid < 256; tid++) {
        const int tx = tid & (int)(kSelectTileW - 1u), ty = tid / (int)kSelectTileW;
        if (T.x0 + tx < (int)P.width && T.y0 + ty < (int)P.height) select_blend_pixel(P, T, tx, ty, cl.data());
    }
}

static bool read_exact(std::FILE* f, void* p, size_t bytes) { return std::fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: select_host_check JOB OUT\n"); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "select_host_check: cannot open the job or the output file\n"); return 2; }
    uint32_t cases = 0;
    if (!read_exact(in, &cases, 4)) return 2;
    size_t max_lds = 0;
    for (uint32_t c = 0; c < cases; c++) {
        uint32_t hdr[6];
        if (!read_exact(in, hdr, sizeof(hdr))) { std::fprintf(stderr, "case %u: short header\n", c); return 2; }
        const uint32_t w = hdr[0], h = hdr[1], K = hdr[2], r = hdr[3], s = hdr[4], outputs = hdr[5];
        if (w == 0 || h == 0 || K < 1 || K > (uint32_t)kSelectMaxK || r > (uint32_t)kSelectMaxErrorRadius || s > (uint32_t)kSelectMaxBlendRadius) {
            std::fprintf(stderr, "case %u: outside the contract\n", c);
            return 2;
        }
        const size_t n = (size_t)w * h;
        std::vector<std::vector<float>> img(3 + 2 * K, std::vector<float>(n * 3));
        for (auto& im : img)
            if (!read_exact(in, im.data(), n * 12)) { std::fprintf(stderr, "case %u: short image\n", c); return 2; }
        std::vector<float> mean(n * 3), error(n);
        std::vector<uint8_t> rgb(n * 3, 0x5a), choice(n, 0x5a), scratch(n, 0xee);
        std::memset(mean.data(), 0x5a, n * 12);
        std::memset(error.data(), 0x5a, n * 4);
        SelParams P;
        std::memset(&P, 0, sizeof(P));
        P.width = w; P.height = h; P.tiles_x = (w + kSelectTileW - 1) / kSelectTileW;
        P.K = (int)K; P.r = (int)r; P.s = (int)s;
        P.a = img[0].data(); P.b = img[1].data(); P.v = img[2].data();
        for (uint32_t k = 0; k < K; k++) { P.fa[k] = img[3 + k].data(); P.fb[k] = img[3 + K + k].data(); }
        P.out_mean = (outputs & 1u) ? mean.data() : nullptr;
        P.out_rgb = (outputs & 2u) ? rgb.data() : nullptr;
        P.out_choice = (outputs & 4u) ? choice.data() : nullptr;
        P.out_error = (outputs & 8u) ? error.data() : nullptr;
        P.choice = scratch.data();
        max_lds = select_choose_lds_bytes(P) > max_lds ? select_choose_lds_bytes(P) : max_lds;
        const uint32_t blocks = P.tiles_x * ((h + kSelectTileH - 1) / kSelectTileH);
        unsigned long long chosen[4] = {0, 0, 0, 0};
        for (uint32_t b = 0; b < blocks; b++) choose_block(P, b, chosen);
        for (size_t i = 0; i < n; i++) CHECK(scratch[i] < K, "case %u: pixel %zu has no choice", c, i);
        for (uint32_t b = 0; b < blocks; b++) blend_block(P, b);
        CHECK(chosen[0] + chosen[1] + chosen[2] + chosen[3] == n, "case %u: the counts do not add up to the pixels", c);
        std::fwrite(mean.data(), 4, n * 3, out); std::fwrite(rgb.data(), 1, n * 3, out);
        std::fwrite(choice.data(), 1, n, out); std::fwrite(error.data(), 4, n, out);
        std::fwrite(chosen, 8, 4, out);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::printf("%u cases, %d failures; the largest tile: %zu bytes of LDS\n", cases, g_fail, max_lds);
    return g_fail ? 1 : 0;
}
