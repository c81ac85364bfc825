// tools/modulate_host_check.cpp -- the kernels of crt_demodulate / crt_modulate (cudaraytracing_amd/csrc/crt_modulate.h) compiled for the
// HOST and run against a plain restatement, for AddressSanitizer / UBSan runs without a device.  crt_modulate.h and crt_stages.h (the
// tone map) are included as they are; tools/host_device.h stands in for what they take from outside.
// The kernels have no cross-lane operation, so a launch is a plain loop over blocks and threads.
// Every buffer is sized exactly (std::vector of the image's 3 x W x H values), so an access one element out is a report; float4 keeps
// its 16-byte alignment here, so a 16-byte access through a pointer that is not aligned is a report as well.  The sizes are ragged
// (3 x W x H is no multiple of four), each is run with aligned bases (the 16-byte path and the scalar tail), with bases one float off
// (the scalar path on every quad) and with a grid capped to one block (the stride loop).
//
// tests/test_host_checks.py builds and runs it:
//   g++ -std=c++17 -ffp-contract=off -I cudaraytracing_amd/csrc -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       tools/modulate_host_check.cpp -o /tmp/modulate_host_check && /tmp/modulate_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "host_device.h"

#include "crt_stages.h"
#include "crt_modulate.h"

using namespace crtk;

static int g_fail = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fail++; } \
    } while (0)

static bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }

// ---- the contract of include/crt.h, restated ----
static float restated_demodulate(float color, float albedo, const float* emission, float floor_)
{
    float d = color;
    if (emission) d = color - *emission;
    if (albedo > floor_) return d / albedo;
    return d;
}
static float restated_variance(float variance, float albedo, float floor_)
{
    if (albedo > floor_) return variance / (albedo * albedo);
    return variance;
}
static float restated_modulate(float irradiance, float albedo, const float* emission, float floor_)
{
    float m = irradiance;
    if (albedo > floor_) m = irradiance * albedo;
    if (emission) return m + *emission;
    return m;
}
static uint8_t restated_tonemap(float c)
{
    float cl = 1.0f < c ? 1.0f : c;    // Global.h:121-124, the operands in minf_ref's / maxf_ref's order: a NaN stays a NaN
    cl = 0.0f > cl ? 0.0f : cl;
    const float v = 255 * det_powf(cl, 0.6f);
    if (!(v == v) || v <= 0.0f) return 0;
    if (v >= 255.0f) return 255;
    return (uint8_t)v;
}

// n floats of a test image; `off` floats of slack in front, so that data() + off is the base the kernels get: off 0 is 16-byte aligned
// (checked), off 1 is not.  The vector holds exactly off + n values.
struct Image {
    std::vector<float, std::allocator<float>> v;
    size_t off;
    Image(size_t n, size_t off_) : v(off_ + n), off(off_) {}
    float* p() { return v.data() + off; }
};

static float special(int k)
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float s[] = {0.0f, -0.0f, -0.5f, nan, inf, -inf, 0.01f, 1e-30f, 0.75f, 300.0f};
    return s[k % 10];
}

static void run_case(uint32_t w, uint32_t h, size_t off, float floor_, bool with_emission, bool with_variance, uint32_t max_blocks)
{
    const size_t n = (size_t)w * h * 3;
    Image color(n, off), albedo(n, off), emission(n, off), variance(n, off), irr(n, off), ivar(n, off), mean(n, off);
    std::vector<uint8_t> rgb(n + (off ? 1 : 0), 0x5a); // (one byte in with the floats one float in: out_rgb is then not 4-byte aligned)
    uint8_t* rgb_p = rgb.data() + (off ? 1 : 0);
    if (off == 0) CHECK((uintptr_t)color.p() % 16 == 0 && (uintptr_t)albedo.p() % 16 == 0, "the allocator's arrays are not 16-byte aligned");
    std::srand(w * 131 + h * 17 + (unsigned)off);
    auto rnd = [] { return (float)(std::rand() % 2000) / 500.0f; };
    for (size_t i = 0; i < n; i++) {
        color.p()[i] = i % 7 == 3 ? special((int)(i / 7)) : rnd() * 8.0f;
        albedo.p()[i] = i % 5 == 1 ? special((int)(i / 5)) : (i % 11 == 0 ? floor_ : rnd() / 4.0f);
        emission.p()[i] = i % 13 == 2 ? special((int)(i / 13)) : (i % 3 == 0 ? rnd() * 50.0f : 0.0f);
        variance.p()[i] = i % 17 == 4 ? special((int)(i / 17)) : rnd();
    }
    std::fill(irr.v.begin(), irr.v.end(), -7.0f); std::fill(ivar.v.begin(), ivar.v.end(), -7.0f); std::fill(mean.v.begin(), mean.v.end(), -7.0f);
    const float* e = with_emission ? emission.p() : nullptr;
    auto al16 = [](const void* p) { return (uintptr_t)p % 16 == 0; };

    DemodParams D{};
    D.n = n; D.floor = floor_;
    D.color = color.p(); D.albedo = albedo.p(); D.emission = e; D.variance = with_variance ? variance.p() : nullptr;
    D.out = irr.p(); D.out_variance = with_variance ? ivar.p() : nullptr;
    D.vec = al16(D.color) && al16(D.albedo) && al16(D.emission) && al16(D.variance) && al16(D.out) && al16(D.out_variance); // (crt_modulate.hip's rule)
    CHECK((D.vec != 0) == (off == 0), "vec");
    launch_demodulate(D, nullptr, max_blocks);
    for (size_t i = 0; i < n; i++) {
        const float want = restated_demodulate(color.p()[i], albedo.p()[i], e ? e + i : nullptr, floor_);
        CHECK(same_bits(irr.p()[i], want) || (want != want && irr.p()[i] != irr.p()[i]), "%ux%u off %zu: irradiance[%zu] = %g, expected %g", w, h, off, i, irr.p()[i], want);
        if (with_variance) {
            const float wv = restated_variance(variance.p()[i], albedo.p()[i], floor_);
            CHECK(same_bits(ivar.p()[i], wv) || (wv != wv && ivar.p()[i] != ivar.p()[i]), "%ux%u off %zu: variance[%zu] = %g, expected %g", w, h, off, i, ivar.p()[i], wv);
        } else CHECK(ivar.p()[i] == -7.0f, "variance[%zu] written without a variance", i);
    }

    for (int outputs = 1; outputs <= 3; outputs++) { // out_mean, out_rgb, both
        ModParams M{};
        M.n = n; M.floor = floor_;
        M.irradiance = irr.p(); M.albedo = albedo.p(); M.emission = e;
        M.out_mean = (outputs & 1) ? mean.p() : nullptr; M.out_rgb = (outputs & 2) ? rgb_p : nullptr;
        M.vec = al16(M.irradiance) && al16(M.albedo) && al16(M.emission) && al16(M.out_mean) && (uintptr_t)M.out_rgb % 4 == 0;
        launch_modulate(M, nullptr, max_blocks);
        for (size_t i = 0; i < n; i++) {
            const float want = restated_modulate(irr.p()[i], albedo.p()[i], e ? e + i : nullptr, floor_);
            if (outputs & 1) CHECK(same_bits(mean.p()[i], want) || (want != want && mean.p()[i] != mean.p()[i]), "%ux%u off %zu: mean[%zu] = %g, expected %g", w, h, off, i, mean.p()[i], want);
            if (outputs & 2) CHECK(rgb_p[i] == restated_tonemap(want), "%ux%u off %zu: rgb[%zu] = %u, expected %u", w, h, off, i, rgb_p[i], restated_tonemap(want));
        }
    }
}

int main()
{
    const uint32_t shapes[5][2] = {{1, 1}, {7, 5}, {61, 47}, {130, 9}, {29, 13}}; // 3, 105, 8601, 3510, 1131 values: tails of 3, 1, 1, 2, 3
    int cases = 0;
    for (const auto& sh : shapes)
        for (size_t off : {(size_t)0, (size_t)1})
            for (float floor_ : {0.0f, 0.01f})
                for (int opt = 0; opt < 4; opt++)
                    for (uint32_t max_blocks : {kModulateMaxBlocks, 1u}) {
                        run_case(sh[0], sh[1], off, floor_, (opt & 1) != 0, (opt & 2) != 0, max_blocks);
                        cases++;
                    }
    std::printf("%d cases, %d failures\n", cases, g_fail);
    return g_fail ? 1 : 0;
}
