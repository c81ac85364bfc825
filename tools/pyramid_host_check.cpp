// tools/pyramid_host_check.cpp -- the kernels of crt_pyramid_down and crt_pyramid_merge (cudaraytracing_amd/csrc/crt_pyramid.h on
// crt_upsample.h) compiled for the HOST and run against a scalar restatement of include/crt.h, for AddressSanitizer / UBSan runs without a
// device.  crt_pyramid.h, crt_upsample.h and crt_stages.h (the tone map, write_color) are included as they are; tools/host_device.h stands
// in for what they take from outside, and float2 is stated here.  The staged merge kernel (k_pyramid_merge_staged, crt_pyramid.hip) is its
// two phases with a workgroup barrier in between; here the barrier is "every thread of the workgroup has run the phase": the same
// sequence as loops over the thread index.  The LDS array is a std::vector of exactly 3 x pyramid_stage_cap entries (what
// pyramid_lds_bytes hands the launch), filled with NaN before a workgroup runs, and every image plane has exactly its image's entries: a
// staging, tap or output index one element out is a report, and a detail the staging did not write shows up in the comparison.
// Checked, bit for bit: down with every combination of the optional planes, with the 8-byte path and float by float; the merge's direct
// and staged form, with one output at a time and both; each on the sizes of tests/test_pyramid.py, with finite inputs and with NaN,
// +-inf, +-1e30, -0 and misses in every buffer.
// Run as `pyramid_host_check JOB OUT` (JOB is not read) it also writes every output of every case to OUT: tests/test_pyramid.py compares
// the bytes of the plain and the sanitised build.
//
// tests/test_pyramid.py builds and runs it (tests/host_program.py):
//   g++ -std=c++17 -ffp-contract=off -I cudaraytracing_amd/csrc -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       tools/pyramid_host_check.cpp -o /tmp/pyramid_host_check && /tmp/pyramid_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "host_device.h"

struct alignas(8) float2 { float x, y; };

#include "crt_stages.h"
#include "crt_upsample.h"
#include "crt_pyramid.h"

using namespace crtk;

static int g_fail = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fail++; } \
    } while (0)

static bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }

static std::FILE* g_out = nullptr;
static void dump(const void* p, size_t bytes) { if (g_out && bytes) std::fwrite(p, 1, bytes, g_out); }
static void dump(const std::vector<float>& v) // (a NaN as one bit pattern: which NaN an operation gives is the compiler's choice of instruction)
{
    for (float f : v) { const unsigned int u = f != f ? 0x7fc00000u : __float_as_uint(f); dump(&u, 4); }
}

// every plane on an 8-byte boundary of its own allocation (std::vector<float>'s storage is at least that), exactly its image's entries
struct Image {
    uint32_t w, h;
    std::vector<float> color, variance, albedo, normal, depth;
};

static Image make_image(uint32_t w, uint32_t h, unsigned seed, bool special)
{
    Image im;
    im.w = w; im.h = h;
    const size_t n = (size_t)w * h;
    std::srand(seed);
    auto rnd = [] { return (float)(std::rand() % 2000) / 2000.0f; };
    im.color.resize(n * 3); im.variance.resize(n * 3); im.albedo.resize(n * 3); im.normal.resize(n * 3); im.depth.resize(n);
    for (size_t i = 0; i < n * 3; i++) { im.color[i] = rnd() * 40.0f; im.variance[i] = rnd() * 3.0f; im.albedo[i] = 0.4f + rnd() * 0.2f; im.normal[i] = rnd() * 2.0f - 1.0f; }
    for (size_t p = 0; p < n; p++) im.depth[p] = std::rand() % 5 == 0 ? 0.0f : 5.0f + rnd() * 0.3f; // (0: a miss)
    if (special) {
        const float inf = std::numeric_limits<float>::infinity(), values[] = {-0.0f, std::numeric_limits<float>::quiet_NaN(), inf, -inf, 1e30f, -1e30f, 0.0f, -0.5f};
        std::vector<float>* all[] = {&im.color, &im.variance, &im.albedo, &im.normal, &im.depth};
        for (int k = 0; k < 5; k++)
            for (size_t j = 0; j < all[k]->size() / 9 + 1; j++) (*all[k])[(size_t)std::rand() % all[k]->size()] = values[(j + (size_t)k) % 8];
    }
    return im;
}

// ---- the contract of include/crt.h, restated ----
// kind 0: colour / albedo / normal, 1: variance, 2: depth; channel c of `channels`
static float restated_down(const std::vector<float>& plane, uint32_t w, uint32_t h, int channels, int c, uint32_t X, uint32_t Y, int kind)
{
    float sum = 0.0f, n = 0.0f, nd = 0.0f;
    for (uint32_t dy = 0; dy < 2; dy++)
        for (uint32_t dx = 0; dx < 2; dx++) {
            const uint32_t x = 2 * X + dx, y = 2 * Y + dy;
            if (x >= w || y >= h) continue;
            const float v = plane.at(((size_t)y * w + x) * (size_t)channels + (size_t)c);
            n = n + 1.0f;
            if (kind == 2) { if (v > 0.0f) { sum = sum + v; nd = nd + 1.0f; } }
            else sum = sum + v;
        }
    if (kind == 2) return nd > 0.0f ? sum / nd : 0.0f;
    return kind == 1 ? sum / (n * n) : sum / n;
}

static float restated_merge(const std::vector<float>& fine, const std::vector<float>& coarse, uint32_t w, uint32_t h, uint32_t x, uint32_t y, int c)
{
    const uint32_t lw = (w + 1) / 2, lh = (h + 1) / 2;
    const float sx = (float)lw / (float)w, sy = (float)lh / (float)h;
    const float u = ((float)x + 0.5f) * sx - 0.5f, v = ((float)y + 0.5f) * sy - 0.5f;
    const int x0 = (int)std::floor(u), y0 = (int)std::floor(v);
    float snum = 0.0f, sden = 0.0f;
    for (int ty = y0; ty <= y0 + 1; ty++)
        for (int tx = x0; tx <= x0 + 1; tx++) {
            if (tx < 0 || tx >= (int)lw || ty < 0 || ty >= (int)lh) continue;
            const float wx = 1.0f - std::fabs(u - (float)tx) / 1.0f, wy = 1.0f - std::fabs(v - (float)ty) / 1.0f;
            const float hw = wy * wx;
            const float d = coarse.at(((size_t)ty * lw + (size_t)tx) * 3 + (size_t)c) - restated_down(fine, w, h, 3, c, (uint32_t)tx, (uint32_t)ty, 0);
            snum = snum + d * hw;
            sden = sden + hw;
        }
    return fine.at(((size_t)y * w + x) * 3 + (size_t)c) + snum / sden;
}

static int g_cases = 0;
static size_t g_max_lds = 0;

// planes: bit 0 variance, 1 albedo, 2 normal, 3 depth; vec: the 8-byte path where the layout has it
static void down_case(uint32_t w, uint32_t h, int planes, bool vec, bool special)
{
    g_cases++;
    const Image im = make_image(w, h, w * 131 + h * 17 + (unsigned)planes, special);
    const uint32_t lw = (w + 1) / 2, lh = (h + 1) / 2;
    const size_t n2 = (size_t)lw * lh;
    std::vector<float> oc(n2 * 3, -7.0f), ov(n2 * 3, -7.0f), oa(n2 * 3, -7.0f), on(n2 * 3, -7.0f), od(n2, -7.0f);
    PyrDownParams P;
    std::memset(&P, 0, sizeof(P));
    P.width = w; P.height = h; P.low_width = lw; P.low_height = lh;
    P.tiles_x = (lw + kPyramidDownTileW - 1) / kPyramidDownTileW;
    P.vec = vec && w % 2 == 0;
    P.color = im.color.data(); P.out_color = oc.data();
    if (planes & 1) { P.variance = im.variance.data(); P.out_variance = ov.data(); }
    if (planes & 2) { P.albedo = im.albedo.data(); P.out_albedo = oa.data(); }
    if (planes & 4) { P.normal = im.normal.data(); P.out_normal = on.data(); }
    if (planes & 8) { P.depth = im.depth.data(); P.out_depth = od.data(); }
    for (uint32_t blk = 0; blk < P.tiles_x * ((lh + kPyramidDownTileH - 1) / kPyramidDownTileH); blk++) // k_pyramid_down
        for (uint32_t tid = 0; tid < 256; tid++) {
            const uint32_t by = blk / P.tiles_x, bx = blk - by * P.tiles_x;
            const uint32_t X = bx * kPyramidDownTileW + (tid & 63u), Y = by * kPyramidDownTileH + (tid >> 6);
            if (X < lw && Y < lh) pyramid_down_pixel(P, X, Y);
        }
    size_t finite = 0;
    for (uint32_t Y = 0; Y < lh; Y++)
        for (uint32_t X = 0; X < lw; X++) {
            const size_t Q = (size_t)Y * lw + X;
            for (int c = 0; c < 3; c++) {
                const size_t i = Q * 3 + (size_t)c;
                const float want = restated_down(im.color, w, h, 3, c, X, Y, 0);
                finite += want == want;
                CHECK(same_bits(oc[i], want), "down %ux%u planes %d vec %d: colour[%zu] %g, restated %g", w, h, planes, vec, i, oc[i], want);
                if (planes & 1) CHECK(same_bits(ov[i], restated_down(im.variance, w, h, 3, c, X, Y, 1)), "down %ux%u planes %d vec %d: variance[%zu]", w, h, planes, vec, i);
                else CHECK(ov[i] == -7.0f, "variance written without a buffer");
                if (planes & 2) CHECK(same_bits(oa[i], restated_down(im.albedo, w, h, 3, c, X, Y, 0)), "down %ux%u planes %d vec %d: albedo[%zu]", w, h, planes, vec, i);
                else CHECK(oa[i] == -7.0f, "albedo written without a buffer");
                if (planes & 4) CHECK(same_bits(on[i], restated_down(im.normal, w, h, 3, c, X, Y, 0)), "down %ux%u planes %d vec %d: normal[%zu]", w, h, planes, vec, i);
                else CHECK(on[i] == -7.0f, "normal written without a buffer");
            }
            if (planes & 8) CHECK(same_bits(od[Q], restated_down(im.depth, w, h, 1, 0, X, Y, 2)), "down %ux%u planes %d vec %d: depth[%zu] %g", w, h, planes, vec, Q, od[Q]);
            else CHECK(od[Q] == -7.0f, "depth written without a buffer");
        }
    CHECK(special || finite == n2 * 3, "a NaN from finite inputs");
    CHECK(finite > 0, "every value NaN: the case checks nothing");
    dump(oc); dump(ov); dump(oa); dump(on); dump(od);
}

// k_pyramid_merge_staged of crt_pyramid.hip, a barrier = the end of a loop over the workgroup's threads
static void staged_block(const PyrMergeParams& P, const uint32_t block)
{
    const PyrTile T = pyramid_tile(P, block);
    CHECK(T.tw >= 1 && T.th >= 1 && T.tw * T.th <= P.cap, "block %u: a tile of %d x %d for a plane of %d", block, T.tw, T.th, P.cap);
    CHECK(T.lx0 >= 0 && T.lx0 + T.tw <= (int)P.low_width && T.ly0 >= 0 && T.ly0 + T.th <= (int)P.low_height, "block %u: the tile leaves the coarse image", block);
    std::vector<float> s_tile((size_t)3 * (size_t)P.cap, std::numeric_limits<float>::quiet_NaN());
    CHECK(s_tile.size() * 4u == pyramid_lds_bytes(P), "pyramid_lds_bytes");
    for (int tid = 0; tid < 256; tid++) pyramid_stage(P, T, tid, s_tile.data());
    const uint32_t by = block / P.tiles_x, bx = block - by * P.tiles_x;
    for (uint32_t tid = 0; tid < 256; tid++) {
        const uint32_t x = bx * kPyramidMergeTileW + (tid & 31u), y = by * kPyramidMergeTileH + (tid >> 5);
        if (x < P.width && y < P.height) pyramid_merge_pixel_staged(P, T, x, y, s_tile.data());
    }
}

// outputs: bit 0 the colour, bit 1 the RGB; coarse_is_down: the coarse image is D(fine), so the merge returns fine's values
static void merge_case(uint32_t w, uint32_t h, int outputs, bool special, bool coarse_is_down)
{
    g_cases++;
    const uint32_t lw = (w + 1) / 2, lh = (h + 1) / 2;
    const Image fine = make_image(w, h, w * 31 + h * 7 + (unsigned)outputs, special);
    Image coarse = make_image(lw, lh, w * 3 + h * 59 + (unsigned)outputs, special);
    if (coarse_is_down)
        for (uint32_t Y = 0; Y < lh; Y++)
            for (uint32_t X = 0; X < lw; X++)
                for (int c = 0; c < 3; c++) coarse.color[((size_t)Y * lw + X) * 3 + (size_t)c] = restated_down(fine.color, w, h, 3, c, X, Y, 0);
    const size_t n = (size_t)w * h;
    PyrMergeParams P;
    std::memset(&P, 0, sizeof(P));
    P.width = w; P.height = h; P.low_width = lw; P.low_height = lh;
    P.tiles_x = (w + kPyramidMergeTileW - 1) / kPyramidMergeTileW;
    P.sx = (float)lw / (float)w; P.sy = (float)lh / (float)h;
    P.fine = fine.color.data(); P.coarse = coarse.color.data();
    P.cap = pyramid_stage_cap(P);
    CHECK(P.cap <= 18 * 6, "%ux%u: a plane of %d details", w, h, P.cap);
    g_max_lds = std::max(g_max_lds, (size_t)pyramid_lds_bytes(P));
    const uint32_t blocks = P.tiles_x * ((h + kPyramidMergeTileH - 1) / kPyramidMergeTileH);
    for (int form = 0; form < 2; form++) { // 0: direct, 1: staged
        std::vector<float> out_c(n * 3, -7.0f);
        std::vector<uint8_t> out_rgb(n * 3, 0x5a);
        P.out_mean = (outputs & 1) ? out_c.data() : nullptr;
        P.out_rgb = (outputs & 2) ? out_rgb.data() : nullptr;
        if (form == 0) {
            for (uint32_t blk = 0; blk < blocks; blk++) // k_pyramid_merge_direct
                for (uint32_t tid = 0; tid < 256; tid++) {
                    const uint32_t by = blk / P.tiles_x, bx = blk - by * P.tiles_x;
                    const uint32_t x = bx * kPyramidMergeTileW + (tid & 31u), y = by * kPyramidMergeTileH + (tid >> 5);
                    if (x < w && y < h) pyramid_merge_pixel(P, x, y);
                }
        } else {
            for (uint32_t blk = 0; blk < blocks; blk++) staged_block(P, blk);
        }
        size_t finite = 0;
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++)
                for (int c = 0; c < 3; c++) {
                    const size_t i = ((size_t)y * w + x) * 3 + (size_t)c;
                    const float want = restated_merge(fine.color, coarse.color, w, h, x, y, c);
                    finite += want == want;
                    if (outputs & 1) CHECK(same_bits(out_c[i], want), "merge form %d %ux%u: colour[%zu] %g, restated %g", form, w, h, i, out_c[i], want);
                    else CHECK(out_c[i] == -7.0f, "colour written without a buffer");
                    if (outputs & 2) CHECK(out_rgb[i] == tonemap(want), "merge form %d %ux%u: rgb[%zu]", form, w, h, i);
                    else CHECK(out_rgb[i] == 0x5a, "rgb written without a buffer");
                    if (coarse_is_down && !special) CHECK(want == fine.color[i], "merge of D(fine) %ux%u: [%zu] %g, fine %g", w, h, i, want, fine.color[i]);
                }
        CHECK(special || finite == n * 3, "a NaN from finite inputs");
        CHECK(finite > 0, "every value NaN: the case checks nothing");
        dump(out_c); dump(out_rgb.data(), out_rgb.size());
    }
}

int main(int argc, char** argv)
{
    if (argc > 2) {
        g_out = std::fopen(argv[2], "wb");
        if (!g_out) { std::printf("cannot write %s\n", argv[2]); return 2; }
    }
    struct Size { uint32_t w, h; };
    const Size sizes[] = {{1, 1}, {2, 2}, {3, 5}, {33, 9}, {65, 17}, {70, 19}, {37, 21}, {130, 40}};
    for (const Size& s : sizes)
        for (int planes = 0; planes < 16; planes++)
            for (int special = 0; special < 2; special++) {
                down_case(s.w, s.h, planes, true, special != 0);
                if (planes == 15) down_case(s.w, s.h, planes, false, special != 0);
            }
    for (const Size& s : sizes)
        for (int special = 0; special < 2; special++) {
            merge_case(s.w, s.h, 3, special != 0, false);
            merge_case(s.w, s.h, 1, special != 0, false);
            merge_case(s.w, s.h, 2, special != 0, false);
            merge_case(s.w, s.h, 3, special != 0, true);
        }
    if (g_out) std::fclose(g_out);
    std::printf("%d cases, %d failures; the largest tile: %zu bytes of LDS\n", g_cases, g_fail, g_max_lds);
    return g_fail ? 1 : 0;
}
