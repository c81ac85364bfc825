// tools/detmath_host_check.cpp -- csrc/crt_detmath.h compiled for the host, as it is, over a file of inputs (tests/test_device_fn.py).
//
//   detmath_host_check in.bin out.bin
//
// in.bin  (little-endian): u32 n1, f32 x[n1], u32 n2, f32 a[n2], f32 b[n2]
// out.bin: n1 floats each of sin cos tan asin acos atan exp log log10 sincos.s sincos.c uniform(bits of x), then n2 floats each of
//          atan2(a, b) and pow(a, b)
// Build: g++ -O2 -std=c++17 -ffp-contract=off (the test also builds it with -fsanitize=address,undefined,float-cast-overflow and expects
// the same bytes and exit status 0).  Exit status 2: bad arguments or a short file.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "crt_detmath.h"

using namespace crtdev;

namespace {
bool read_u32(FILE* f, uint32_t& v) { return std::fread(&v, 4, 1, f) == 1; }
bool read_f32(FILE* f, std::vector<float>& v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), 4, n, f) == n;
}
template <class Fn> void emit(FILE* f, const std::vector<float>& x, Fn fn)
{
    std::vector<float> o(x.size());
    for (size_t i = 0; i < x.size(); i++) o[i] = fn(x[i]);
    if (!o.empty()) std::fwrite(o.data(), 4, o.size(), f);
}
} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: detmath_host_check in.bin out.bin\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "detmath_host_check: cannot read %s\n", argv[1]); return 2; }
    uint32_t n1 = 0, n2 = 0;
    std::vector<float> x, a, b;
    const bool ok = read_u32(in, n1) && read_f32(in, x, n1) && read_u32(in, n2) && read_f32(in, a, n2) && read_f32(in, b, n2);
    std::fclose(in);
    if (!ok) { std::fprintf(stderr, "detmath_host_check: %s is too short\n", argv[1]); return 2; }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "detmath_host_check: cannot write %s\n", argv[2]); return 2; }
    emit(out, x, [](float v) { return det_sinf(v); });
    emit(out, x, [](float v) { return det_cosf(v); });
    emit(out, x, [](float v) { return det_tanf(v); });
    emit(out, x, [](float v) { return det_asinf(v); });
    emit(out, x, [](float v) { return det_acosf(v); });
    emit(out, x, [](float v) { return det_atanf(v); });
    emit(out, x, [](float v) { return det_expf(v); });
    emit(out, x, [](float v) { return det_logf(v); });
    emit(out, x, [](float v) { return det_log10f(v); });
    emit(out, x, [](float v) { float s, c; det_sincosf(v, &s, &c); return s; });
    emit(out, x, [](float v) { float s, c; det_sincosf(v, &s, &c); return c; });
    emit(out, x, [](float v) { return rng_uniform(f2u(v)); });
    {
        std::vector<float> o(n2);
        for (size_t i = 0; i < n2; i++) o[i] = det_atan2f(a[i], b[i]);
        if (n2) std::fwrite(o.data(), 4, n2, out);
        for (size_t i = 0; i < n2; i++) o[i] = det_powf(a[i], b[i]);
        if (n2) std::fwrite(o.data(), 4, n2, out);
    }
    return std::fclose(out) == 0 ? 0 : 2;
}
