// tools/upsample_ab.hip -- the A/B of the two forms of crt_upsample that cudaraytracing_amd/csrc/crt_upsample.h states, in one process,
// taking turns:
//   direct  one thread per output pixel, every tap through the caches (upsample_pixel);
//   staged  k_upsample as crt_upsample.hip has it: the workgroup first copies the low-resolution pixels its 64 x 4 output pixels can
//           tap into LDS (upsample_stage), then every thread takes its taps from there (upsample_pixel_staged).
// Both run the same upsample_tap / upsample_finish, so they give the same bits -- which this program checks on every output.  The
// verdict and the figures are in docs/experiments.md, "Guide-driven upsampling": the staged form won and is the library's kernel.
// Inputs: smooth synthetic guides with an edge every 37 output columns, so that both outcomes of `guided` and weights of every size
// occur; all guides, variance, all three outputs, no counter.  Per size pair: --calls timed launches of each form after --warmup,
// HIP events around each launch; median, best and worst, and the compulsory bytes (28 B of guides in, 27 B out per output pixel, 52 B
// per low-resolution pixel) over the median.  The spread of the SAME form between the two halves of its calls is the noise to judge by.
//
//   hipcc -O3 -std=c++17 -ffp-contract=off -fno-fast-math --offload-arch=gfx950 -fhip-fp32-correctly-rounded-divide-sqrt \
//         -I cudaraytracing_amd/csrc tools/upsample_ab.hip -o /tmp/upsample_ab && /tmp/upsample_ab [--calls 50] [--warmup 5]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "crt_detmath.h"
#include "crt_fastdiv.h"

// ---- what crt_stages.h takes from crt_path.h / crt_device.h: the same text ----
#define CRT_TILE 8
namespace crtk {
using namespace crtdev; // FastDiv, det_powf, det_expf
struct F3 { float x, y, z; };
__host__ __device__ inline F3 f3(float x, float y, float z) { return F3{x, y, z}; }
__host__ __device__ inline float maxf_ref(float x, float y) { return x > y ? x : y; }
__host__ __device__ inline float minf_ref(float x, float y) { return x < y ? x : y; }
struct Rad3 { float x, y, z; };
__device__ inline Rad3 load_radiance(const Rad3* p) { return *p; }
__device__ inline bool slot_to_pixel(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, FastDiv, uint32_t, uint32_t, uint32_t&, uint32_t&) { return false; } // (no slot map here)
} // namespace crtk

#include "crt_stages.h"
#include "crt_upsample.h"

namespace crtk {

__global__ __launch_bounds__(256) void k_upsample_direct(const UpParams P)
{
    const uint32_t by = blockIdx.x / P.tiles_x, bx = blockIdx.x - by * P.tiles_x;
    const uint32_t x = bx * kUpsampleTileW + (threadIdx.x & 63u), y = by * kUpsampleTileH + (threadIdx.x >> 6);
    if (x < P.width && y < P.height) (void)upsample_pixel(P, x, y);
}

// (crt_upsample.hip's kernel without the counter, which neither form has here)
__global__ __launch_bounds__(256) void k_upsample_staged(const UpParams P)
{
    extern __shared__ float s_tile[];
    const UpTile T = upsample_tile(P, blockIdx.x);
    upsample_stage(P, T, (int)threadIdx.x, s_tile);
    __syncthreads();
    const uint32_t by = blockIdx.x / P.tiles_x, bx = blockIdx.x - by * P.tiles_x;
    const uint32_t x = bx * kUpsampleTileW + (threadIdx.x & 63u), y = by * kUpsampleTileH + (threadIdx.x >> 6);
    if (x < P.width && y < P.height) (void)upsample_pixel_staged(P, T, x, y, s_tile);
}

} // namespace crtk

using namespace crtk;

#define HIP_OK(call)                                                                                  \
    do {                                                                                              \
        const hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); std::exit(1); } \
    } while (0)

template <typename T> static T* upload(const std::vector<T>& h)
{
    T* d = nullptr;
    HIP_OK(hipMalloc((void**)&d, h.size() * sizeof(T)));
    HIP_OK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}

// guides of a w x h image: surfaces that change every 37 columns OF THE OUTPUT (the two sizes describe one scene), smooth inside
static void make_guides(uint32_t w, uint32_t h, uint32_t out_w, std::vector<float>& albedo, std::vector<float>& normal, std::vector<float>& depth)
{
    albedo.resize((size_t)w * h * 3); normal.resize((size_t)w * h * 3); depth.resize((size_t)w * h);
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const size_t p = (size_t)y * w + x;
            const float fx = ((float)x + 0.5f) * (float)out_w / (float)w, fy = ((float)y + 0.5f) / (float)h;
            const int surface = (int)(fx / 37.0f) % 3;
            for (int c = 0; c < 3; c++) {
                albedo[p * 3 + c] = 0.2f + 0.25f * (float)surface + 0.01f * fy;
                normal[p * 3 + c] = c == surface ? 1.0f : 0.0f;
            }
            depth[p] = 10.0f + 2.0f * (float)surface + 0.001f * fx;
        }
}

struct Stats { float median, best, worst, half_a, half_b; };
static Stats stats_of(std::vector<float> ms)
{
    const size_t n = ms.size();
    std::vector<float> a(ms.begin(), ms.begin() + n / 2), b(ms.begin() + n / 2, ms.end());
    auto med = [](std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    Stats s;
    s.half_a = med(a); s.half_b = med(b);
    std::sort(ms.begin(), ms.end());
    s.median = ms[n / 2]; s.best = ms.front(); s.worst = ms.back();
    return s;
}

static int run(uint32_t w, uint32_t h, uint32_t lw, uint32_t lh, uint32_t radius, int calls, int warmup)
{
    const size_t n = (size_t)w * h, nl = (size_t)lw * lh;
    std::vector<float> color(nl * 3), variance(nl * 3), la, ln, ld, ha, hn, hd;
    std::srand(w + lw + radius);
    for (size_t i = 0; i < nl * 3; i++) { color[i] = (float)(std::rand() % 4000) / 100.0f; variance[i] = (float)(std::rand() % 300) / 100.0f; }
    make_guides(lw, lh, w, la, ln, ld);
    make_guides(w, h, w, ha, hn, hd);
    UpParams P;
    std::memset(&P, 0, sizeof(P));
    P.width = w; P.height = h; P.low_width = lw; P.low_height = lh;
    P.tiles_x = (w + kUpsampleTileW - 1) / kUpsampleTileW;
    P.radius = (int)radius; P.fradius = (float)radius;
    P.sx = (float)lw / (float)w; P.sy = (float)lh / (float)h;
    P.min_weight = 0.015625f;
    P.sig2_n = 0.25f; P.sig2_a = 0.1f * 0.1f; P.sigma_d = 0.05f;
    P.color = upload(color); P.variance = upload(variance);
    P.lalbedo = upload(la); P.lnormal = upload(ln); P.ldepth = upload(ld);
    P.albedo = upload(ha); P.normal = upload(hn); P.depth = upload(hd);
    float* out_c[2]; float* out_v[2]; uint8_t* out_rgb[2];
    for (int f = 0; f < 2; f++) {
        HIP_OK(hipMalloc((void**)&out_c[f], n * 12)); HIP_OK(hipMalloc((void**)&out_v[f], n * 12)); HIP_OK(hipMalloc((void**)&out_rgb[f], n * 3));
        HIP_OK(hipMemset(out_c[f], 0x55, n * 12)); HIP_OK(hipMemset(out_v[f], 0x55, n * 12)); HIP_OK(hipMemset(out_rgb[f], 0x55, n * 3));
    }
    P.cap = upsample_stage_cap(P);
    const size_t lds = upsample_lds_bytes(P);
    const uint32_t blocks = P.tiles_x * ((h + kUpsampleTileH - 1) / kUpsampleTileH);
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
    std::vector<float> ms[2];
    for (int k = 0; k < warmup + calls; k++)
        for (int f = 0; f < 2; f++) { // 0: direct, 1: staged
            UpParams Q = P;
            Q.out_mean = out_c[f]; Q.out_variance = out_v[f]; Q.out_rgb = out_rgb[f];
            HIP_OK(hipEventRecord(e0, nullptr));
            if (f == 0) hipLaunchKernelGGL(k_upsample_direct, dim3(blocks), dim3(256), 0, nullptr, Q);
            else hipLaunchKernelGGL(k_upsample_staged, dim3(blocks), dim3(256), lds, nullptr, Q);
            HIP_OK(hipEventRecord(e1, nullptr));
            HIP_OK(hipGetLastError());
            HIP_OK(hipEventSynchronize(e1));
            float t = 0.0f;
            HIP_OK(hipEventElapsedTime(&t, e0, e1));
            if (k >= warmup) ms[f].push_back(t);
        }
    // the same bits
    std::vector<uint32_t> a(n * 3), b(n * 3);
    std::vector<uint8_t> ra(n * 3), rb(n * 3);
    size_t differ = 0, unwritten = 0;
    for (int which = 0; which < 2; which++) {
        HIP_OK(hipMemcpy(a.data(), which ? out_v[0] : out_c[0], n * 12, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(b.data(), which ? out_v[1] : out_c[1], n * 12, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n * 3; i++) { differ += a[i] != b[i]; unwritten += a[i] == 0x55555555u; }
    }
    HIP_OK(hipMemcpy(ra.data(), out_rgb[0], n * 3, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(rb.data(), out_rgb[1], n * 3, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n * 3; i++) differ += ra[i] != rb[i];
    const Stats d = stats_of(ms[0]), s = stats_of(ms[1]);
    const double bytes = 55.0 * (double)n + 52.0 * (double)nl;
    std::printf("{\"width\": %u, \"height\": %u, \"low_width\": %u, \"low_height\": %u, \"radius\": %u, \"calls\": %d, "
                "\"direct_ms_median\": %.4f, \"direct_ms_best\": %.4f, \"direct_ms_worst\": %.4f, \"direct_ms_halves\": [%.4f, %.4f], "
                "\"staged_ms_median\": %.4f, \"staged_ms_best\": %.4f, \"staged_ms_worst\": %.4f, \"staged_ms_halves\": [%.4f, %.4f], "
                "\"staged_over_direct\": %.4f, \"staged_lds_bytes\": %zu, \"direct_compulsory_TB_per_s\": %.4f, \"staged_compulsory_TB_per_s\": %.4f, "
                "\"values_that_differ\": %zu, \"values_unwritten\": %zu}\n",
                w, h, lw, lh, radius, calls, d.median, d.best, d.worst, d.half_a, d.half_b, s.median, s.best, s.worst, s.half_a, s.half_b, s.median / d.median, lds,
                bytes / (d.median * 1e-3) / 1e12, bytes / (s.median * 1e-3) / 1e12, differ, unwritten);
    std::fflush(stdout);
    for (const void* p : {(const void*)P.color, (const void*)P.variance, (const void*)P.lalbedo, (const void*)P.lnormal, (const void*)P.ldepth,
                          (const void*)P.albedo, (const void*)P.normal, (const void*)P.depth})
        HIP_OK(hipFree(const_cast<void*>(p)));
    for (int f = 0; f < 2; f++) { HIP_OK(hipFree(out_c[f])); HIP_OK(hipFree(out_v[f])); HIP_OK(hipFree(out_rgb[f])); }
    HIP_OK(hipEventDestroy(e0)); HIP_OK(hipEventDestroy(e1));
    return differ == 0 && unwritten == 0 ? 0 : 1;
}

int main(int argc, char** argv)
{
    int calls = 50, warmup = 5;
    for (int i = 1; i + 1 < argc; i += 2) {
        if (!std::strcmp(argv[i], "--calls")) calls = std::atoi(argv[i + 1]);
        else if (!std::strcmp(argv[i], "--warmup")) warmup = std::atoi(argv[i + 1]);
    }
    if (calls < 2 || warmup < 0) { std::fprintf(stderr, "usage: %s [--calls N >= 2] [--warmup N]\n", argv[0]); return 2; }
    int rc = 0;
    rc |= run(800, 600, 400, 300, 1, calls, warmup);
    rc |= run(3840, 2160, 1920, 1080, 1, calls, warmup);
    rc |= run(3840, 2160, 960, 540, 1, calls, warmup);
    rc |= run(3840, 2160, 960, 540, 2, calls, warmup);
    rc |= run(61, 47, 31, 24, 4, 2, 1); // ragged blocks, a ratio that is no integer, the widest window: the same bits there too
    return rc;
}
