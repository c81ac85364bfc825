// tools/with_bits_check.cpp -- CPU property check of crtaccel::with_bits (csrc/crt_accel.h), the helper that moves a plane of the
// four-wide tree outwards to the nearest value whose low 12 mantissa bits carry a chunk of child indices (nodes4i, crt_scene_layout.h).
// For every input and all 4 096 chunks, in both directions:
//   * ok: the result is finite, has the chunk in its low 12 bits, lies on the asked side of f (<= f down, >= f up) and is the NEAREST
//     such value: the next value with the same low bits one chunk period further (across zero where the magnitude runs out) lies beyond f;
//   * ok == false exactly when no finite value with those bits lies on that side (f not finite, or |f| beyond the largest magnitude
//     with those bits on the side away from zero), and then f comes back unchanged.
// Inputs: signed zeros, the smallest denormals, the denormal / normal boundary and its neighbours, +-FLT_MAX and its neighbours,
// +-inf, NaN, and `n_random` random bit patterns (argv[1], default 1 000 000; seed argv[2]).  Prints one JSON line.
// Build: g++ -O2 -std=c++17 -pthread -I cudaraytracing_amd/csrc tools/with_bits_check.cpp  (tests/test_with_bits.py)
#include "crt_accel.h"

#include <cstdio>
#include <random>

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float flt(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

// the next value with low bits `chunk` strictly above (up = true) or below r, +-inf if none is finite: one chunk period in magnitude,
// or across zero to the smallest magnitude of the other sign
static float step(float r, uint32_t chunk, bool up)
{
    const uint32_t u = bits(r), m = u & 0x7fffffffu;
    const bool neg = (u >> 31) != 0;
    const bool grow = neg ? !up : up;
    if (grow) {
        const uint32_t n = m + 0x1000u;
        if (n >= 0x7f800000u) return up ? INFINITY : -INFINITY;
        return flt(n | (u & 0x80000000u));
    }
    if (m >= 0x1000u) return flt((m - 0x1000u) | (u & 0x80000000u));
    // m == chunk: the other sign's smallest magnitude with these bits -- strictly beyond r, so +-0 (equal to r when chunk == 0) is skipped
    const uint32_t other = chunk != 0 ? chunk : 0x1000u;
    return flt(other | (neg ? 0u : 0x80000000u));
}

struct Tally {
    uint64_t calls = 0, ok = 0, fail = 0, bad = 0;
    uint64_t crossed = 0;
    char first_bad[160] = {0};
};

static void check_one(float f, uint32_t chunk, bool up, Tally& t)
{
    bool ok = true;
    const float r = crtaccel::with_bits(f, chunk, up, ok);
    t.calls++;
    const uint32_t m = bits(f) & 0x7fffffffu;
    const bool neg = (bits(f) >> 31) != 0;
    // no finite value with these bits on the asked side: f not finite, or |f| above the largest such magnitude on the side away from zero
    const bool none = !(std::fabs(f) <= FLT_MAX) || (m > (0x7f7ff000u | chunk) && neg != up);
    bool good;
    if (!ok) {
        t.fail++;
        good = none && bits(r) == bits(f);
    } else {
        t.ok++;
        const float nx = step(r, chunk, !up); // one period back towards f
        good = !none && std::isfinite(r) && (bits(r) & 0xfffu) == chunk && (up ? r >= f : r <= f) && (up ? nx < f : nx > f);
        if (std::signbit(r) != std::signbit(f)) t.crossed++;
    }
    if (!good) {
        if (!t.bad) std::snprintf(t.first_bad, sizeof(t.first_bad), "f=%08x chunk=%03x up=%d ok=%d r=%08x", bits(f), chunk, (int)up, (int)ok, bits(r));
        t.bad++;
    }
}

int main(int argc, char** argv)
{
    const uint64_t n_random = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1000000ull;
    const uint32_t seed = argc > 2 ? (uint32_t)std::strtoul(argv[2], nullptr, 10) : 1u;
    std::vector<uint32_t> special;
    for (uint32_t s : {0u, 0x80000000u}) {
        for (uint32_t k = 0; k < 4; k++) special.push_back(s | k);                             // zero, the smallest denormals
        for (uint32_t k = 0xffdu; k <= 0x1002u; k++) special.push_back(s | k);                 // one chunk period in
        for (uint32_t k = 0x7ffffcu; k <= 0x800003u; k++) special.push_back(s | k);           // denormal / normal boundary
        for (uint32_t k = 0x7f7fe000u; k <= 0x7f7fe002u; k++) special.push_back(s | k);
        for (uint32_t k = 0x7f7feffeu; k <= 0x7f7ff001u; k++) special.push_back(s | k);
        for (uint32_t k = 0x7f7ffffcu; k <= 0x7f800001u; k++) special.push_back(s | k);       // FLT_MAX, its neighbours, inf, a NaN
        special.push_back(s | 0x7fc00000u);                                                    // quiet NaN
        special.push_back(s | 0x3f800000u);                                                    // 1.0
    }
    std::mt19937 rng(seed);
    const uint64_t n_all = special.size() + n_random;
    unsigned n_threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<Tally> tally(n_threads);
    std::vector<uint32_t> inputs(special);
    inputs.reserve(n_all);
    for (uint64_t i = 0; i < n_random; i++) inputs.push_back((uint32_t)rng());
    std::vector<std::thread> th;
    for (unsigned k = 0; k < n_threads; k++)
        th.emplace_back([&, k] {
            for (size_t i = k; i < inputs.size(); i += n_threads)
                for (uint32_t c = 0; c < 4096; c++) {
                    check_one(flt(inputs[i]), c, false, tally[k]);
                    check_one(flt(inputs[i]), c, true, tally[k]);
                }
        });
    for (auto& t : th) t.join();
    Tally s;
    for (const Tally& t : tally) {
        s.calls += t.calls; s.ok += t.ok; s.fail += t.fail; s.crossed += t.crossed;
        if (t.bad && !s.bad) std::memcpy(s.first_bad, t.first_bad, sizeof(s.first_bad));
        s.bad += t.bad;
    }
    std::printf("{\"inputs\": %llu, \"special\": %zu, \"calls\": %llu, \"ok\": %llu, \"gave_up\": %llu, \"crossed_zero\": %llu, \"violations\": %llu, \"first_violation\": \"%s\"}\n",
                (unsigned long long)n_all, special.size(), (unsigned long long)s.calls, (unsigned long long)s.ok, (unsigned long long)s.fail,
                (unsigned long long)s.crossed, (unsigned long long)s.bad, s.first_bad);
    return s.bad ? 1 : 0;
}
