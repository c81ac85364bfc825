// cudaraytracing_amd/csrc/crt_fastdiv.h -- the host half of the exact division by a run-time constant: plain C++, so that the kernels'
// header (crt_device.h) and the HIP-free scene layout (crt_scene_layout.h: the `lights` rows) share one definition.
#ifndef CRT_FASTDIV_H
#define CRT_FASTDIV_H

#include <stdint.h>

namespace crtdev {

// Exact unsigned 32-bit division by a run-time constant without the ~40-instruction hardware-less
// divide sequence (Granlund & Montgomery / Hacker's Delight 10-9): q = (t + ((n - t) >> sh1)) >> sh2,
// t = mulhi(m, n).  Valid for every n and every d >= 1 (tests/test_host_layer.py checks the host maths).
struct FastDiv {
    uint32_t m, sh; // sh = sh1 | sh2 << 8
};
inline FastDiv make_fastdiv(uint32_t d)
{
    uint32_t l = 0;
    while (l < 32 && (1ull << l) < d) l++;
    FastDiv f;
    f.m = (uint32_t)((((1ull << l) - d) << 32) / d + 1);
    f.sh = (l < 1 ? l : 1u) | ((l > 0 ? l - 1 : 0u) << 8);
    return f;
}

} // namespace crtdev
#endif
