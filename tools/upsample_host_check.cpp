// tools/upsample_host_check.cpp -- the two forms of crt_upsample (cudaraytracing_amd/csrc/crt_upsample.h) compiled for the HOST and run
// against a scalar restatement of include/crt.h, for AddressSanitizer / UBSan runs without a device.  crt_upsample.h and crt_stages.h
// (the tone map, write_color) are included as they are; tools/host_device.h stands in for what they take from
// outside.  The kernel (k_upsample, crt_upsample.hip) is its two phases with a workgroup barrier in between; here
// the barrier is "every thread of the workgroup has run the phase": the same sequence as loops over the thread index.  The LDS array is
// a std::vector of exactly kUpsamplePlanes x upsample_stage_cap entries (what upsample_lds_bytes hands the launch), filled with NaN
// before a workgroup runs, and every image plane has exactly its image's entries: a staging, tap or output index one element out is a
// report, and a tap the staging did not write shows up in the comparison.
// Checked: the staged form and the direct form against the restatement, bit for bit -- colour, variance, RGB and the count of fallback
// pixels.  Sizes: those of tests/test_upsample.py -- a ratio that is no integer with ragged blocks, a low image shorter than the tap
// window, one pixel in a second wave, a single tap, equal sizes -- and the widest tile (radius 4 at equal sizes), each with every
// combination of guide pairs, with and without a variance, with one output at a time, and with NaN, +-inf and -0 in every buffer.
//
// tests/test_host_checks.py builds and runs it:
//   g++ -std=c++17 -ffp-contract=off -I cudaraytracing_amd/csrc -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       tools/upsample_host_check.cpp -o /tmp/upsample_host_check && /tmp/upsample_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "host_device.h"

#include "crt_stages.h"
#include "crt_upsample.h"

using namespace crtk;

static int g_fail = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fail++; } \
    } while (0)

static bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }

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
    for (size_t i = 0; i < n * 3; i++) { im.color[i] = rnd() * 40.0f; im.variance[i] = rnd() * 3.0f; im.albedo[i] = 0.4f + rnd() * 0.2f; im.normal[i] = rnd() * 0.4f; }
    for (size_t p = 0; p < n; p++) im.depth[p] = 5.0f + rnd() * 0.3f;
    if (special && n > 2) {
        const float inf = std::numeric_limits<float>::infinity(), values[] = {0.0f, -0.0f, std::numeric_limits<float>::quiet_NaN(), inf, -inf, 1e30f, 1e-30f, -0.5f};
        std::vector<float>* all[] = {&im.color, &im.variance, &im.albedo, &im.normal, &im.depth};
        for (int k = 0; k < 5; k++)
            for (size_t j = 0; j < all[k]->size() / 12 + 1; j++) (*all[k])[(size_t)std::rand() % all[k]->size()] = values[(j + (size_t)k) % 8];
    }
    return im;
}

// ---- the contract of include/crt.h, restated: one pixel ----
struct Settings { uint32_t radius; float min_weight, sigma_normal, sigma_albedo, sigma_depth; }; // crt_upsample_params', without the sizes
struct Restated { float c[3], v[3]; bool guided; };
static Restated restated_pixel(const Image& lo, const Image& hi, uint32_t x, uint32_t y, const Settings& prm, bool use_a, bool use_n, bool use_d,
                               bool use_v)
{
    const float sx = (float)lo.w / (float)hi.w, sy = (float)lo.h / (float)hi.h;
    const float u = ((float)x + 0.5f) * sx - 0.5f, v = ((float)y + 0.5f) * sy - 0.5f;
    const int x0 = (int)std::floor(u), y0 = (int)std::floor(v), R = (int)prm.radius;
    const size_t p = (size_t)y * hi.w + x;
    float num[3] = {0, 0, 0}, snum[3] = {0, 0, 0}, vnum[3] = {0, 0, 0}, svnum[3] = {0, 0, 0}, den = 0.0f, sden = 0.0f;
    for (int ty = y0 - R + 1; ty <= y0 + R; ty++)
        for (int tx = x0 - R + 1; tx <= x0 + R; tx++) {
            if (tx < 0 || tx >= (int)lo.w || ty < 0 || ty >= (int)lo.h) continue;
            const size_t q = (size_t)ty * lo.w + (size_t)tx;
            const float wx = 1.0f - std::fabs(u - (float)tx) / (float)R, wy = 1.0f - std::fabs(v - (float)ty) / (float)R;
            const float hw = wy * wx;
            float e_n = 0.0f, e_a = 0.0f, e_d = 0.0f;
            if (use_n) {
                const float dx = hi.normal.at(p * 3) - lo.normal.at(q * 3), dy = hi.normal.at(p * 3 + 1) - lo.normal.at(q * 3 + 1), dz = hi.normal.at(p * 3 + 2) - lo.normal.at(q * 3 + 2);
                e_n = (dx * dx + dy * dy + dz * dz) / (prm.sigma_normal * prm.sigma_normal);
            }
            if (use_a) {
                const float dx = hi.albedo.at(p * 3) - lo.albedo.at(q * 3), dy = hi.albedo.at(p * 3 + 1) - lo.albedo.at(q * 3 + 1), dz = hi.albedo.at(p * 3 + 2) - lo.albedo.at(q * 3 + 2);
                e_a = (dx * dx + dy * dy + dz * dz) / (prm.sigma_albedo * prm.sigma_albedo);
            }
            if (use_d) {
                const float pd = hi.depth.at(p), qd = lo.depth.at(q);
                const float m = pd > qd ? pd : qd;
                const float r = (pd - qd) / (prm.sigma_depth * m);
                e_d = m > 0.0f ? r * r : 0.0f;
            }
            const float w = hw * det_expf(-((e_n + e_a) + e_d));
            for (int c = 0; c < 3; c++) {
                num[c] = num[c] + lo.color.at(q * 3 + c) * w;
                snum[c] = snum[c] + lo.color.at(q * 3 + c) * hw;
                if (use_v) {
                    vnum[c] = vnum[c] + lo.variance.at(q * 3 + c) * (w * w);
                    svnum[c] = svnum[c] + lo.variance.at(q * 3 + c) * (hw * hw);
                }
            }
            den = den + w;
            sden = sden + hw;
        }
    Restated r;
    r.guided = den > prm.min_weight * sden;
    for (int c = 0; c < 3; c++) {
        r.c[c] = r.guided ? num[c] / den : snum[c] / sden;
        r.v[c] = r.guided ? vnum[c] / (den * den) : svnum[c] / (sden * sden);
    }
    return r;
}

// k_upsample of crt_upsample.hip, a barrier = the end of a loop over the workgroup's threads; returns the pixels that fell back
static unsigned long long staged_block(const UpParams& P, const uint32_t block)
{
    const UpTile T = upsample_tile(P, block);
    CHECK(T.tw >= 1 && T.th >= 1 && T.tw * T.th <= P.cap, "block %u: a tile of %d x %d for a plane of %d", block, T.tw, T.th, P.cap);
    CHECK(T.lx0 >= 0 && T.lx0 + T.tw <= (int)P.low_width && T.ly0 >= 0 && T.ly0 + T.th <= (int)P.low_height, "block %u: the tile leaves the low image", block);
    std::vector<float> s_tile((size_t)kUpsamplePlanes * (size_t)P.cap, std::numeric_limits<float>::quiet_NaN());
    CHECK(s_tile.size() * 4u == upsample_lds_bytes(P), "upsample_lds_bytes");
    for (int tid = 0; tid < 256; tid++) upsample_stage(P, T, tid, s_tile.data());
    const uint32_t by = block / P.tiles_x, bx = block - by * P.tiles_x;
    unsigned long long fell = 0;
    for (uint32_t tid = 0; tid < 256; tid++) {
        const uint32_t x = bx * kUpsampleTileW + (tid & 63u), y = by * kUpsampleTileH + (tid >> 6);
        if (x < P.width && y < P.height) fell += !upsample_pixel_staged(P, T, x, y, s_tile.data());
    }
    return fell;
}

static size_t g_max_lds = 0;

// outputs: bit 0 the colour, bit 1 the RGB; drop: bit 0 albedo, 1 normal, 2 depth; use_v: with the variance
static void run_case(uint32_t w, uint32_t h, uint32_t lw, uint32_t lh, uint32_t radius, int drop, bool use_v, int outputs, bool special, float min_weight)
{
    const Image lo = make_image(lw, lh, w * 131 + h * 17 + radius, special), hi = make_image(w, h, lw * 29 + lh * 7 + radius, special);
    const bool use_a = !(drop & 1), use_n = !(drop & 2), use_d = !(drop & 4);
    const Settings prm = {radius, min_weight, 0.5f, 0.1f, 0.05f};
    const size_t n = (size_t)w * h;
    UpParams P;
    std::memset(&P, 0, sizeof(P));
    P.width = w; P.height = h; P.low_width = lw; P.low_height = lh;
    P.tiles_x = (w + kUpsampleTileW - 1) / kUpsampleTileW;
    P.radius = (int)radius; P.fradius = (float)radius;
    P.sx = (float)lw / (float)w; P.sy = (float)lh / (float)h;
    P.min_weight = min_weight;
    P.color = lo.color.data();
    if (use_v) P.variance = lo.variance.data();
    if (use_a) { P.lalbedo = lo.albedo.data(); P.albedo = hi.albedo.data(); }
    if (use_n) { P.lnormal = lo.normal.data(); P.normal = hi.normal.data(); }
    if (use_d) { P.ldepth = lo.depth.data(); P.depth = hi.depth.data(); }
    P.sig2_n = use_n ? prm.sigma_normal * prm.sigma_normal : 1.0f;
    P.sig2_a = use_a ? prm.sigma_albedo * prm.sigma_albedo : 1.0f;
    P.sigma_d = prm.sigma_depth;
    P.cap = upsample_stage_cap(P);
    g_max_lds = std::max(g_max_lds, (size_t)upsample_lds_bytes(P));
    const uint32_t blocks = P.tiles_x * ((h + kUpsampleTileH - 1) / kUpsampleTileH);
    for (int form = 0; form < 2; form++) { // 0: direct, 1: staged
        std::vector<float> out_c(n * 3, -7.0f), out_v(n * 3, -7.0f);
        std::vector<uint8_t> out_rgb(n * 3, 0x5a);
        P.out_mean = (outputs & 1) ? out_c.data() : nullptr;
        P.out_rgb = (outputs & 2) ? out_rgb.data() : nullptr;
        P.out_variance = use_v ? out_v.data() : nullptr;
        unsigned long long count = 0;
        if (form == 0) {
            for (uint32_t y = 0; y < h; y++)
                for (uint32_t x = 0; x < w; x++) count += !upsample_pixel(P, x, y);
        } else {
            for (uint32_t blk = 0; blk < blocks; blk++) count += staged_block(P, blk);
        }
        unsigned long long fell = 0;
        size_t nan_free = 0;
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) {
                const Restated r = restated_pixel(lo, hi, x, y, prm, use_a, use_n, use_d, use_v);
                fell += !r.guided;
                const size_t p = (size_t)y * w + x;
                for (int c = 0; c < 3; c++) {
                    const size_t i = p * 3 + (size_t)c;
                    if (outputs & 1) CHECK(same_bits(out_c[i], r.c[c]), "form %d %ux%u<-%ux%u r%u drop %d: colour[%zu] %g, restated %g", form, w, h, lw, lh, radius, drop, i, out_c[i], r.c[c]);
                    else CHECK(out_c[i] == -7.0f, "colour written without a buffer");
                    if (outputs & 2) CHECK(out_rgb[i] == tonemap(r.c[c]), "form %d %ux%u<-%ux%u r%u drop %d: rgb[%zu]", form, w, h, lw, lh, radius, drop, i);
                    else CHECK(out_rgb[i] == 0x5a, "rgb written without a buffer");
                    if (use_v) CHECK(same_bits(out_v[i], r.v[c]), "form %d %ux%u<-%ux%u r%u drop %d: variance[%zu] %g, restated %g", form, w, h, lw, lh, radius, drop, i, out_v[i], r.v[c]);
                    else CHECK(out_v[i] == -7.0f, "variance written without a buffer");
                    nan_free += r.c[c] == r.c[c];
                }
            }
        CHECK(count == fell, "form %d %ux%u<-%ux%u r%u drop %d: %llu fallback pixels, %llu restated", form, w, h, lw, lh, radius, drop, count, fell);
        CHECK(special || nan_free == n * 3, "a NaN from finite inputs");
        CHECK(nan_free > 0, "every value NaN: the case checks nothing");
    }
}

int main()
{
    struct Case { uint32_t w, h, lw, lh, radius; };
    const Case cases[] = {{61, 47, 31, 24, 1}, {130, 9, 33, 3, 2}, {65, 5, 17, 2, 4}, {7, 5, 1, 1, 3}, {13, 9, 13, 9, 1}, {64, 8, 16, 2, 2}, {129, 5, 128, 5, 4},
                          {200, 13, 200, 13, 4}, {192, 12, 96, 6, 1}};
    int n = 0;
    for (const Case& cs : cases)
        for (int drop = 0; drop < 8; drop++)
            for (int special = 0; special < 2; special++) {
                run_case(cs.w, cs.h, cs.lw, cs.lh, cs.radius, drop, true, 3, special != 0, 0.015625f);
                n++;
            }
    for (const Case& cs : cases) { // one output at a time, without the variance, other thresholds
        run_case(cs.w, cs.h, cs.lw, cs.lh, cs.radius, 0, false, 1, true, 0.0f);
        run_case(cs.w, cs.h, cs.lw, cs.lh, cs.radius, 0, false, 2, true, 0.5f);
        run_case(cs.w, cs.h, cs.lw, cs.lh, cs.radius, 7, true, 1, false, 0.015625f);
        n += 3;
    }
    std::printf("%d cases in both forms, %d failures; the largest tile: %zu bytes of LDS\n", n, g_fail, g_max_lds);
    return g_fail ? 1 : 0;
}
