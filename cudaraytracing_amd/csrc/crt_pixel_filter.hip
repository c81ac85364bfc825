// cudaraytracing_amd/csrc/crt_pixel_filter.hip -- the pixel reconstruction filters (contract: include/crt.h, CRT_FLAG_PIXEL_FILTER): the
// kernel that adds a chunk's samples to the filter's sums a and W, in two forms (crt_pixel_filter.h; CRT_PIXEL_FILTER_FORM=direct|staged,
// a test hook: the same bits from both), the read-out kernel, and the entry points crt_pixel_filter_defaults, crt_set_pixel_filter,
// crt_filtered_frame*.  crt_render.hip launches the chunk kernel after the chunk's accumulate kernel (launch_pixel_filter).
#include "crt_render.h"
#include "crt_pixel_filter.h"

#include <cstdlib>
#include <cstring>

using namespace crtk;

namespace crtk {

template <int REACH> __global__ __launch_bounds__(256) void k_pixel_filter_direct(const PixelFilterParams P)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= P.A.nslots) return;
    pixel_filter_direct<REACH>(P, slot);
}

template <int REACH> __global__ __launch_bounds__(256) void k_pixel_filter_staged(const PixelFilterParams P)
{
    __shared__ float s_lds[5 * kPixelFilterStageCap];
    const uint32_t tid = threadIdx.x;
    const PixelFilterTile T = pixel_filter_tile(P, blockIdx.x);
    int lx, ly;
    pixel_filter_thread_pixel(tid, lx, ly);
    const bool valid = pixel_filter_inside(P, T.x0 + lx, T.y0 + ly);
    const uint32_t slot = valid ? pixel_filter_slot(P, (uint32_t)(T.x0 + lx), (uint32_t)(T.y0 + ly)) : 0u;
    PixelFilterSum s = {0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) s = pixel_filter_load(P, slot);
    for (uint32_t smp = 0; smp < P.A.chunk_samples; smp++) { // (uniform: every thread of the workgroup reaches both barriers)
        pixel_filter_stage<REACH>(P, T, tid, smp, s_lds);
        __syncthreads();
        if (valid) pixel_filter_gather<REACH>(P, lx, ly, s_lds, s);
        __syncthreads();
    }
    if (valid) pixel_filter_store(P, slot, s);
}

__global__ __launch_bounds__(256) void k_pixel_filter_readout(const PixelFilterParams P)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= P.A.nslots) return;
    pixel_filter_readout(P, slot);
}

// The form of the chunk kernel: the default unless CRT_PIXEL_FILTER_FORM says otherwise (the measurement behind the default:
// docs/experiments.md, "Pixel reconstruction filters")
const bool kPixelFilterStagedDefault = true;
bool pixel_filter_staged_form()
{
    const char* e = std::getenv("CRT_PIXEL_FILTER_FORM");
    if (e && std::strcmp(e, "direct") == 0) return false;
    if (e && std::strcmp(e, "staged") == 0) return true;
    return kPixelFilterStagedDefault;
}

// The chunk A describes (L, chunk_samples, first_chunk) into the planes of filter `pf`; s0: the chunk's first sample in the frame
void launch_pixel_filter(const AParams& A, const crt_pixel_filter& pf, float* planes, uint64_t seed, uint32_t s0, hipStream_t st)
{
    PixelFilterParams P;
    std::memset(&P, 0, sizeof(P));
    P.A = A; P.planes = planes; P.seed = seed; P.s0 = s0; P.kind = pf.kind; P.radius = pf.radius;
    const int reach = pixel_filter_reach(pf.radius);
    if (pixel_filter_staged_form()) {
        const dim3 grid(pixel_filter_staged_blocks(P));
        if (reach == 0) hipLaunchKernelGGL(k_pixel_filter_staged<0>, grid, dim3(256), 0, st, P);
        else if (reach == 1) hipLaunchKernelGGL(k_pixel_filter_staged<1>, grid, dim3(256), 0, st, P);
        else hipLaunchKernelGGL(k_pixel_filter_staged<2>, grid, dim3(256), 0, st, P);
    } else {
        const dim3 grid = slot_grid(A);
        if (reach == 0) hipLaunchKernelGGL(k_pixel_filter_direct<0>, grid, dim3(256), 0, st, P);
        else if (reach == 1) hipLaunchKernelGGL(k_pixel_filter_direct<1>, grid, dim3(256), 0, st, P);
        else hipLaunchKernelGGL(k_pixel_filter_direct<2>, grid, dim3(256), 0, st, P);
    }
}

} // namespace crtk

namespace {

// what crt_filtered_frame needs of the handle
int filtered_check(const crt_scene* sc, const void* out_rgb, const void* out_mean)
{
    if (!sc || (!out_rgb && !out_mean)) return fail(CRT_ERR_INVALID_ARG, "crt_filtered_frame: null argument (a scene and at least one of the two buffers)");
    if (!sc->pf_mark.valid)
        return fail(CRT_ERR_INVALID_ARG, "crt_filtered_frame: no render with CRT_FLAG_PIXEL_FILTER on the handle yet, or the last render (or a range of the frame in "
                                         "flight) was submitted without it");
    return CRT_OK;
}

} // namespace

extern "C" {

int crt_pixel_filter_defaults(crt_pixel_filter* out)
{
    if (!out) return fail(CRT_ERR_INVALID_ARG, "crt_pixel_filter_defaults: null argument");
    out->kind = CRT_PIXEL_FILTER_TENT; out->radius = 1.0f;
    return CRT_OK;
}

int crt_set_pixel_filter(crt_scene* sc, const crt_pixel_filter* filter)
{
    if (!sc) return fail(CRT_ERR_INVALID_ARG, "crt_set_pixel_filter: null scene");
    if (!filter) { sc->pf_set = false; return CRT_OK; }
    if (!pixel_filter_allowed(filter->kind, filter->radius))
        return fail(CRT_ERR_INVALID_ARG, "crt_set_pixel_filter: allowed are CRT_PIXEL_FILTER_BOX with a radius in [0.5, 2], _TENT with a radius in [1, 2] and "
                                         "_MITCHELL with radius 2; got kind " + std::to_string(filter->kind) + ", radius " + std::to_string(filter->radius));
    sc->pf = *filter; sc->pf_set = true;
    return CRT_OK;
}

int crt_filtered_frame_device(crt_scene* sc, void* d_rgb, void* d_mean, void* stream, uint32_t* samples_done)
{
    const int rc = filtered_check(sc, d_rgb, d_mean);
    if (rc != CRT_OK) return rc;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        PixelFilterParams P;
        std::memset(&P, 0, sizeof(P));
        P.A = frame_aparams(sc, sc->pf_mark, make_shard(sc->pf_mark.width, sc->pf_mark.height, sc->pf_mark.world));
        P.A.out_rgb = (uint8_t*)d_rgb; P.A.out_mean = (float*)d_mean;
        P.planes = sc->accum_pf.p;
        P.scale_n = (float)sc->pf_mark.spp / (float)sc->pf_mark.samples;
        hipLaunchKernelGGL(k_pixel_filter_readout, slot_grid(P.A), dim3(256), 0, (hipStream_t)stream, P);
        HIP_CHECK(hipGetLastError());
        if (samples_done) *samples_done = sc->pf_mark.samples;
        return CRT_OK;
    });
}

int crt_filtered_frame(crt_scene* sc, uint8_t* out_rgb, float* out_mean, uint32_t* samples_done)
{
    const int rc0 = filtered_check(sc, out_rgb, out_mean);
    if (rc0 != CRT_OK) return rc0;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        Staging s(out_pixels(sc->pf_mark.width, sc->pf_mark.height, sc->pf_mark.world, sc->pf_mark.tiled != 0), out_rgb != nullptr, out_mean != nullptr);
        const int rc = crt_filtered_frame_device(sc, s.rgb.p, s.f32.p, nullptr, samples_done);
        if (rc != CRT_OK) return rc;
        s.download(out_rgb, out_mean);
        return CRT_OK;
    });
}

} // extern "C"
