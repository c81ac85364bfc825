// tools/nlm_host_check.cpp -- the two forms of crt_denoise_nlm (cudaraytracing_amd/csrc/crt_nlm.h) compiled for the HOST, for
// AddressSanitizer / UBSan runs without a device.  crt_nlm.h and crt_stages.h (the tone map, write_color) are included as they are;
// tools/host_device.h stands in for what they take from outside.
// The shared form's kernel (k_nlm_shared, crt_nlm.hip) is its phases with workgroup barriers in between; here a barrier is "every
// thread of the workgroup has run the phase": the same sequence as loops over the thread index.  The three LDS arrays are std::vectors of
// exactly nlm_stage_elems / nlm_d_elems / nlm_row_elems entries (what nlm_lds_bytes hands the launch) and every image plane has exactly
// width x height entries, so a staging, row-sum or column index one element out is a report.  Before a workgroup runs, its LDS arrays are
// filled with NaN: a phase that reads what the phase before it did not write shows up in the comparison.
// Checked: nlm_div against a plain division for every array width in use; nlm_taps_1d against counting; for images smaller than one
// tile, for ragged images of 2 x 2 and more tiles (tiles at all four corners) and for the limits radius 8 / patch 3, the shared order
// against the direct order on random inputs with zero-variance and zero-depth blocks and NULL guides: mean, RGB and variance bit for bit.
//
// tests/test_host_checks.py builds and runs it:
//   g++ -std=c++17 -ffp-contract=off -I cudaraytracing_amd/csrc -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       tools/nlm_host_check.cpp -o /tmp/nlm_host_check && /tmp/nlm_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "host_device.h"

#include "crt_stages.h"
#include "crt_nlm.h"

using namespace crtk;

static int g_fail = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fail++; } \
    } while (0)

static bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }

static void check_index_helpers()
{
    for (int R = 1; R <= kNlmMaxRadius; R++)
        for (int F = 0; F <= kNlmMaxPatch; F++) {
            const int sw = kNlmTileW + 2 * (R + F), dw = kNlmTileW + 2 * F;
            CHECK(nlm_lds_bytes(R, F) == nlm_stage_elems(R, F) * 16u + nlm_d_elems(F) * 4u + nlm_row_elems(F) * 4u, "nlm_lds_bytes");
            CHECK(nlm_lds_bytes(R, F) <= 64u * 1024u, "a workgroup's LDS");
            for (int i = 0; i < (int)nlm_stage_elems(R, F); i++) CHECK(nlm_div(i, nlm_div_m(sw)) == i / sw, "nlm_div(%d, %d)", i, sw);
            for (int i = 0; i < (int)nlm_d_elems(F); i++) CHECK(nlm_div(i, nlm_div_m(dw)) == i / dw, "nlm_div(%d, %d)", i, dw);
        }
    for (int W = 1; W <= 12; W++)
        for (int F = 0; F <= kNlmMaxPatch; F++)
            for (int x = 0; x < W; x++)
                for (int o = -kNlmMaxRadius; o <= kNlmMaxRadius; o++) {
                    int n = 0;
                    for (int px = -F; px <= F; px++) n += x + px >= 0 && x + px < W && x + px + o >= 0 && x + px + o < W;
                    CHECK(nlm_taps_1d(x, o, F, W) == n, "nlm_taps_1d(%d, %d, %d, %d)", x, o, F, W);
                }
}

struct Outputs {
    std::vector<float> mean, var;
    std::vector<uint8_t> rgb;
    Outputs(size_t npix) : mean(npix * 3, -7.0f), var(npix, -7.0f), rgb(npix * 3, 0x5a) {}
};

// k_nlm_shared of crt_nlm.hip, a barrier = the end of a loop over the workgroup's threads
static void shared_block(const NlmParams& P, const uint32_t block)
{
    const NlmTile T = nlm_tile(P, block);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float4> s_c(nlm_stage_elems(P.radius, P.patch), make_float4(nan, nan, nan, nan));
    std::vector<float> s_d(nlm_d_elems(P.patch), nan), s_row(nlm_row_elems(P.patch), nan);
    CHECK((int)s_c.size() == T.sw * T.sh && (int)s_d.size() == T.dw * T.dh && (int)s_row.size() == kNlmTileW * T.dh, "the tile's array sizes");
    const int W = (int)P.width, H = (int)P.height, R = P.radius;
    std::vector<NlmSum> s(kNlmThreads, NlmSum{0.0f, 0.0f, 0.0f, 0.0f, 0.0f});
    auto lx = [](int tid) { return tid & (kNlmTileW - 1); };
    auto ly = [](int tid) { return tid / kNlmTileW; };
    auto inside = [&](int tid) { return T.x0 + lx(tid) < W && T.y0 + ly(tid) < H; };
    auto pixel = [&](int tid) { return inside(tid) ? (size_t)(T.y0 + ly(tid)) * P.width + (size_t)(T.x0 + lx(tid)) : (size_t)0; };
    for (int tid = 0; tid < kNlmThreads; tid++) nlm_stage(P, T, tid, s_c.data());
    for (int oy = -R; oy <= R; oy++)
        for (int ox = -R; ox <= R; ox++) {
            if (nlm_offset_misses_tile(T, ox, oy, W, H)) {
                for (int tid = 0; tid < kNlmThreads; tid++) // (nothing is left out that a pixel would have taken)
                    CHECK(!inside(tid) || !nlm_inside(T.x0 + lx(tid) + ox, T.y0 + ly(tid) + oy, W, H), "an offset left out that a pixel needs");
                continue;
            }
            for (int tid = 0; tid < kNlmThreads; tid++) nlm_phase_d(P, T, ox, oy, tid, s_c.data(), s_d.data());
            for (int tid = 0; tid < kNlmThreads; tid++) nlm_phase_row(P, T, ox, oy, tid, s_d.data(), s_row.data());
            for (int tid = 0; tid < kNlmThreads; tid++)
                if (inside(tid)) nlm_phase_pixel(P, T, ox, oy, lx(tid), ly(tid), s_c.data(), s_row.data(), P.g0[pixel(tid)], P.g1[pixel(tid)], s[tid]);
            std::fill(s_d.begin(), s_d.end(), nan); // (the next offset must write what it reads)
        }
    for (int tid = 0; tid < kNlmThreads; tid++)
        if (inside(tid)) nlm_finish(P, pixel(tid), s[tid]);
}

static void run_case(uint32_t w, uint32_t h, int R, int F, float k, float alpha, int drop)
{
    const size_t npix = (size_t)w * h;
    std::vector<float> color(npix * 3), variance(npix * 3), albedo(npix * 3), normal(npix * 3), depth(npix);
    std::srand(w * 131 + h * 17 + (unsigned)(R * 7 + F));
    auto rnd = [] { return (float)(std::rand() % 2000) / 2000.0f; };
    for (size_t i = 0; i < npix * 3; i++) {
        color[i] = rnd() * 4.0f; variance[i] = rnd() * 0.5f; albedo[i] = 0.5f + rnd() * 0.05f; normal[i] = rnd() * 0.1f;
    }
    for (size_t p = 0; p < npix; p++) {
        depth[p] = 1.0f + rnd() * 0.02f;
        const uint32_t x = (uint32_t)(p % w), y = (uint32_t)(p / w);
        if (x % 16 < 5 && y % 8 < 3) variance[p * 3] = variance[p * 3 + 1] = variance[p * 3 + 2] = 0.0f; // zero-variance blocks
        if (x % 32 > 27 && y % 16 > 11) depth[p] = 0.0f;                                                 // "miss" blocks
    }
    std::vector<float4> c(npix), g0(npix), g1(npix);
    NlmPack K{};
    K.width = w; K.height = h;
    K.color = color.data(); K.variance = variance.data();
    K.albedo = (drop & 1) ? nullptr : albedo.data(); K.normal = (drop & 2) ? nullptr : normal.data(); K.depth = (drop & 4) ? nullptr : depth.data();
    K.c = c.data(); K.g0 = g0.data(); K.g1 = g1.data();
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) nlm_pack_pixel(K, (int)x, (int)y);

    NlmParams P{};
    P.width = w; P.height = h; P.radius = R; P.patch = F;
    P.k2 = k * k; P.alpha = alpha;
    P.sig2_n = K.normal ? 0.25f : 1.0f; P.sig2_a = K.albedo ? 0.01f : 1.0f; P.sigma_d = 0.05f;
    P.c = c.data(); P.g0 = g0.data(); P.g1 = g1.data();
    Outputs a(npix), b(npix);
    P.out_mean = a.mean.data(); P.out_rgb = a.rgb.data(); P.out_var = a.var.data();
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) nlm_direct_pixel(P, (int)x, (int)y);
    P.out_mean = b.mean.data(); P.out_rgb = b.rgb.data(); P.out_var = b.var.data();
    P.tiles_x = (w + kNlmTileW - 1) / kNlmTileW;
    const uint32_t blocks = P.tiles_x * ((h + kNlmTileH - 1) / kNlmTileH);
    for (uint32_t blk = 0; blk < blocks; blk++) shared_block(P, blk);
    size_t moved = 0;
    for (size_t i = 0; i < npix * 3; i++) {
        CHECK(same_bits(a.mean[i], b.mean[i]), "%ux%u r%d f%d: mean[%zu] direct %g shared %g", w, h, R, F, i, a.mean[i], b.mean[i]);
        CHECK(a.rgb[i] == b.rgb[i], "%ux%u r%d f%d: rgb[%zu]", w, h, R, F, i);
        CHECK(a.mean[i] == a.mean[i], "%ux%u: a NaN from finite inputs", w, h);
        moved += a.mean[i] != color[i];
    }
    for (size_t p = 0; p < npix; p++) CHECK(same_bits(a.var[p], b.var[p]), "%ux%u r%d f%d: variance[%zu] direct %g shared %g", w, h, R, F, p, a.var[p], b.var[p]);
    CHECK(npix < 16 || moved > 0, "%ux%u: the filter changed nothing", w, h); // (1 x 1 and 3 x 2 lie inside a zero-variance block: every other weight is 0)
}

int main()
{
    check_index_helpers();
    struct Case { uint32_t w, h; int R, F; };
    const Case cases[] = {{1, 1, 1, 1}, {3, 2, 1, 1}, {9, 7, 5, 2}, {31, 7, 8, 3},          // smaller than one tile
                          {32, 8, 3, 1}, {33, 9, 1, 0}, {40, 12, 5, 2}, {70, 20, 3, 1},     // one tile exactly; 2 x 2 ragged tiles; 3 x 3
                          {130, 9, 8, 3}, {61, 47, 5, 2}, {37, 19, 8, 3}, {35, 10, 2, 3}};  // the limits; the patch wider than the window
    int n = 0;
    for (const Case& cs : cases)
        for (int drop : {0, 7}) {
            run_case(cs.w, cs.h, cs.R, cs.F, 0.7f, 1.0f, drop);
            n++;
        }
    run_case(40, 12, 5, 2, 0.45f, 0.5f, 2);
    run_case(40, 12, 5, 2, 1.0f, 0.0f, 5);
    n += 2;
    std::printf("%d cases, %d failures\n", n, g_fail);
    return g_fail ? 1 : 0;
}
