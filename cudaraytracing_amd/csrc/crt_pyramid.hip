// cudaraytracing_amd/csrc/crt_pyramid.hip -- crt_pyramid_down / crt_pyramid_merge and their _device forms (contract: include/crt.h): the
// host side of the two image operations of a Laplacian pyramid over crt_denoise_var, crt_denoise_nlm and crt_denoise_regress -- a
// variance-aware 2 x reduction of a frame with its guides, and the merge that puts a coarser scale's finished result in the place of a
// finer result's low frequencies.  Image operations without a scene handle and without scratch, like crt_modulate and crt_upsample.
// One call = one launch; the kernels' phases are in crt_pyramid.h in a form the host can compile as well (tools/pyramid_host_check.cpp).
// CRT_PYRAMID_FORM=direct|staged (read per call; tests and tools/denoise_probe.py) selects the merge kernel's form; unset: the faster one
// (docs/experiments.md, "Multi-scale denoising").
#include "crt_filter_host.h"
#include "crt_upsample.h"
#include "crt_pyramid.h"

#include <cstdlib>
#include <cstring>
#include <string>

namespace crtk {

__global__ __launch_bounds__(256) void k_pyramid_down(const PyrDownParams P)
{
    const uint32_t by = blockIdx.x / P.tiles_x, bx = blockIdx.x - by * P.tiles_x;
    const uint32_t X = bx * kPyramidDownTileW + (threadIdx.x & 63u), Y = by * kPyramidDownTileH + (threadIdx.x >> 6);
    if (X < P.low_width && Y < P.low_height) pyramid_down_pixel(P, X, Y);
}

__global__ __launch_bounds__(256) void k_pyramid_merge_direct(const PyrMergeParams P)
{
    const uint32_t by = blockIdx.x / P.tiles_x, bx = blockIdx.x - by * P.tiles_x;
    const uint32_t x = bx * kPyramidMergeTileW + (threadIdx.x & 31u), y = by * kPyramidMergeTileH + (threadIdx.x >> 5);
    if (x < P.width && y < P.height) pyramid_merge_pixel(P, x, y);
}

// dynamic LDS: pyramid_lds_bytes(P) -- 1 296 bytes (3 planes of 18 x 6 floats)
__global__ __launch_bounds__(256) void k_pyramid_merge_staged(const PyrMergeParams P)
{
    extern __shared__ float s_tile[];
    const PyrTile T = pyramid_tile(P, blockIdx.x);
    pyramid_stage(P, T, (int)threadIdx.x, s_tile);
    __syncthreads();
    const uint32_t by = blockIdx.x / P.tiles_x, bx = blockIdx.x - by * P.tiles_x;
    const uint32_t x = bx * kPyramidMergeTileW + (threadIdx.x & 31u), y = by * kPyramidMergeTileH + (threadIdx.x >> 5);
    if (x < P.width && y < P.height) pyramid_merge_pixel_staged(P, T, x, y, s_tile);
}

} // namespace crtk

using namespace crtk;

namespace {

// What both operations and both forms check first, before any device call
int pyramid_check(const std::string& w, const crt_pyramid_params* prm)
{
    if (!prm) return fail(CRT_ERR_INVALID_ARG, w + ": null argument");
    if (const int rc = size_positive(w, prm->width, prm->height)) return rc;
    if (const int rc = sides_supported(w, prm->width, prm->height)) return rc;
    if (prm->low_width != (prm->width + 1) / 2 || prm->low_height != (prm->height + 1) / 2)
        return fail(CRT_ERR_INVALID_ARG, w + ": the coarse size must be ((width + 1) / 2, (height + 1) / 2)");
    return CRT_OK;
}

int down_check(const char* who, const crt_pyramid_params* prm, const crt_pyramid_planes* in, const crt_pyramid_out_planes* out)
{
    const std::string w(who);
    if (!prm || !in || !out) return fail(CRT_ERR_INVALID_ARG, w + ": null argument");
    if (!in->color || !out->color) return fail(CRT_ERR_INVALID_ARG, w + ": null colour buffer");
    if (const int rc = pyramid_check(w, prm)) return rc;
    if ((in->variance != nullptr) != (out->variance != nullptr) || (in->albedo != nullptr) != (out->albedo != nullptr) ||
        (in->normal != nullptr) != (out->normal != nullptr) || (in->depth != nullptr) != (out->depth != nullptr))
        return fail(CRT_ERR_INVALID_ARG, w + ": a plane must be given as input and output or as neither");
    return size_supported(w, prm->low_width, prm->low_height, kPyramidDownTileW, kPyramidDownTileH);
}

int merge_check(const char* who, const crt_pyramid_params* prm, const void* fine, const void* coarse, const void* out_color, const void* out_rgb)
{
    const std::string w(who);
    if (const int rc = pyramid_check(w, prm)) return rc;
    if (!fine || !coarse) return fail(CRT_ERR_INVALID_ARG, w + ": null fine or coarse image");
    if (!out_color && !out_rgb) return fail(CRT_ERR_INVALID_ARG, w + ": no output buffer");
    return size_supported(w, prm->width, prm->height, kPyramidMergeTileW, kPyramidMergeTileH);
}

// 0: the default form, 1: direct, 2: staged, -1: a value that is neither
int form_of_environment()
{
    const char* e = std::getenv("CRT_PYRAMID_FORM");
    if (!e || !*e) return 0;
    if (std::strcmp(e, "direct") == 0) return 1;
    if (std::strcmp(e, "staged") == 0) return 2;
    return -1;
}

bool aligned8(const void* p) { return (uintptr_t)p % 8u == 0; } // (a null pointer is)

int down_impl(const char* who, int device, const crt_pyramid_params* prm, const crt_pyramid_planes* in, const crt_pyramid_out_planes* out, hipStream_t st,
              crt_pyramid_info* info)
{
    PyrDownParams P;
    std::memset(&P, 0, sizeof(P));
    P.width = prm->width; P.height = prm->height; P.low_width = prm->low_width; P.low_height = prm->low_height;
    P.tiles_x = (P.low_width + kPyramidDownTileW - 1) / kPyramidDownTileW;
    P.color = in->color; P.variance = in->variance; P.albedo = in->albedo; P.normal = in->normal; P.depth = in->depth;
    P.out_color = out->color; P.out_variance = out->variance; P.out_albedo = out->albedo; P.out_normal = out->normal; P.out_depth = out->depth;
    P.vec = P.width % 2u == 0 && aligned8(P.color) && aligned8(P.variance) && aligned8(P.albedo) && aligned8(P.normal) && aligned8(P.depth);
    return timed_launch(who, device, st, info, [&] {
        hipLaunchKernelGGL(k_pyramid_down, dim3(P.tiles_x * ((P.low_height + kPyramidDownTileH - 1) / kPyramidDownTileH)), dim3(256), 0, st, P);
    });
}

int merge_impl(const char* who, int device, const crt_pyramid_params* prm, const float* fine, const float* coarse, float* out_color, uint8_t* out_rgb,
               hipStream_t st, crt_pyramid_info* info)
{
    const int form = form_of_environment();
    if (form < 0 && device >= 0) // (a bad device index is reported first: timed_launch's test)
        return fail(CRT_ERR_INVALID_ARG, std::string(who) + ": CRT_PYRAMID_FORM must be direct or staged");
    PyrMergeParams P;
    std::memset(&P, 0, sizeof(P));
    P.width = prm->width; P.height = prm->height; P.low_width = prm->low_width; P.low_height = prm->low_height;
    P.tiles_x = (P.width + kPyramidMergeTileW - 1) / kPyramidMergeTileW;
    P.sx = (float)P.low_width / (float)P.width;
    P.sy = (float)P.low_height / (float)P.height;
    P.fine = fine; P.coarse = coarse; P.out_mean = out_color; P.out_rgb = out_rgb;
    P.cap = pyramid_stage_cap(P);
    const dim3 grid(P.tiles_x * ((P.height + kPyramidMergeTileH - 1) / kPyramidMergeTileH));
    return timed_launch(who, device, st, info, [&] {
        if (form == 1) hipLaunchKernelGGL(k_pyramid_merge_direct, grid, dim3(256), 0, st, P);
        else hipLaunchKernelGGL(k_pyramid_merge_staged, grid, dim3(256), pyramid_lds_bytes(P), st, P);
    });
}

} // namespace

extern "C" {

int crt_pyramid_size(uint32_t width, uint32_t height, uint32_t* low_width, uint32_t* low_height)
{
    if (!low_width || !low_height) return fail(CRT_ERR_INVALID_ARG, "crt_pyramid_size: null argument");
    if (const int rc = size_positive("crt_pyramid_size", width, height)) return rc;
    *low_width = width / 2 + width % 2; *low_height = height / 2 + height % 2;
    return CRT_OK;
}

int crt_pyramid_down_device(int device, const crt_pyramid_params* prm, const crt_pyramid_planes* dev_in, const crt_pyramid_out_planes* dev_out, void* stream,
                            crt_pyramid_info* info)
{
    const int rc = down_check("crt_pyramid_down_device", prm, dev_in, dev_out);
    if (rc != CRT_OK) return rc;
    return down_impl("crt_pyramid_down_device", device, prm, dev_in, dev_out, (hipStream_t)stream, info);
}

int crt_pyramid_down(int device, const crt_pyramid_params* prm, const crt_pyramid_planes* host_in, const crt_pyramid_out_planes* host_out,
                     crt_pyramid_info* info)
{
    const int rc0 = down_check("crt_pyramid_down", prm, host_in, host_out);
    if (rc0 != CRT_OK) return rc0;
    const uint64_t n = (uint64_t)prm->width * prm->height, n2 = (uint64_t)prm->low_width * prm->low_height;
    return host_form("crt_pyramid_down", device, [&](HostCopies& c) {
        crt_pyramid_planes di{};
        crt_pyramid_out_planes dout{};
        di.color = c.in(host_in->color, n * 3); di.variance = c.in(host_in->variance, n * 3); di.albedo = c.in(host_in->albedo, n * 3);
        di.normal = c.in(host_in->normal, n * 3); di.depth = c.in(host_in->depth, n);
        dout.color = c.out(host_out->color, n2 * 3); dout.variance = c.out(host_out->variance, n2 * 3); dout.albedo = c.out(host_out->albedo, n2 * 3);
        dout.normal = c.out(host_out->normal, n2 * 3); dout.depth = c.out(host_out->depth, n2);
        return down_impl("crt_pyramid_down_device", device, prm, &di, &dout, nullptr, info);
    });
}

int crt_pyramid_merge_device(int device, const crt_pyramid_params* prm, const void* d_fine, const void* d_coarse, void* d_out_color, void* d_out_rgb,
                             void* stream, crt_pyramid_info* info)
{
    const int rc = merge_check("crt_pyramid_merge_device", prm, d_fine, d_coarse, d_out_color, d_out_rgb);
    if (rc != CRT_OK) return rc;
    return merge_impl("crt_pyramid_merge_device", device, prm, (const float*)d_fine, (const float*)d_coarse, (float*)d_out_color, (uint8_t*)d_out_rgb,
                      (hipStream_t)stream, info);
}

int crt_pyramid_merge(int device, const crt_pyramid_params* prm, const float* fine, const float* coarse, float* out_color, uint8_t* out_rgb,
                      crt_pyramid_info* info)
{
    const int rc0 = merge_check("crt_pyramid_merge", prm, fine, coarse, out_color, out_rgb);
    if (rc0 != CRT_OK) return rc0;
    const uint64_t n = (uint64_t)prm->width * prm->height, n2 = (uint64_t)prm->low_width * prm->low_height;
    return host_form("crt_pyramid_merge", device, [&](HostCopies& c) {
        const float *d_fine = c.in(fine, n * 3), *d_coarse = c.in(coarse, n2 * 3);
        return merge_impl("crt_pyramid_merge_device", device, prm, d_fine, d_coarse, c.out(out_color, n * 3), c.out(out_rgb, n * 3), nullptr, info);
    });
}

} // extern "C"
