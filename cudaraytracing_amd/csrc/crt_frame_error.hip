// cudaraytracing_amd/csrc/crt_frame_error.hip -- crt_frame_error* (the error of the frame in flight as one small struct, reduced on the
// device) and crt_render_until* (a uniform frame rendered in ranges until that summary meets a target, and left in flight), contracts:
// include/crt.h.  The device text is crt_frame_error.h's; here are its two kernels, the scratch they meet in (on the handle: the blocks'
// partials, a summary and the pinned words a check is read through) and the host side.  The loop is ranges of render_impl
// (crt_render.hip, through crt_render.h) with CRT_FLAG_VARIANCE, exactly as crt_render_range submits them: the render kernel, its
// parameters and the frame's sums are untouched, and a summary only reads.
#include "crt_render.h"
#include "crt_frame_error.h"

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <string>

namespace crtk {

__global__ __launch_bounds__(256) void k_frame_error_blocks(const FrameErrorParams D) { frame_error_block(D); }
__global__ __launch_bounds__(64) void k_frame_error_finish(const FrameErrorParams D) { frame_error_finish(D); }

// Both launches on st: the second reads what the first wrote, across the kernel boundary
void launch_frame_error(const FrameErrorParams& D, hipStream_t st)
{
    hipLaunchKernelGGL(k_frame_error_blocks, dim3(D.n_blocks), dim3(256), 0, st, D);
    hipLaunchKernelGGL(k_frame_error_finish, dim3(kFeQuantities), dim3(64), 0, st, D);
}

} // namespace crtk

using namespace crtk;

namespace {

int criterion_check(const char* who, float threshold, float mean_floor)
{
    if (!(threshold >= 0.0f)) return fail(CRT_ERR_INVALID_ARG, std::string(who) + ": threshold must be >= 0 and not NaN");
    if (!(mean_floor >= 0.0f) || mean_floor > FLT_MAX) return fail(CRT_ERR_INVALID_ARG, std::string(who) + ": mean_floor must be >= 0 and finite");
    return CRT_OK;
}

// Argument checks of both forms of crt_frame_error, before any device call
int frame_error_check(const crt_scene* sc, float threshold, float mean_floor, const void* out)
{
    if (!out) return fail(CRT_ERR_INVALID_ARG, "crt_frame_error: null output");
    const int rc = criterion_check("crt_frame_error", threshold, mean_floor); // the scene comes last, so that the message names what is wrong with the other arguments even where there is no scene
    return rc != CRT_OK ? rc : sums_check("crt_frame_error", sc, out);
}

// The summary of the sums on the handle (sums_check has passed) into d_out, enqueued on st
void enqueue_frame_error(crt_scene* sc, float threshold, float mean_floor, crt_frame_error_info* d_out, hipStream_t st)
{
    FrameErrorParams D{};
    D.A = frame_aparams(sc, sc->var, make_shard(sc->var.width, sc->var.height, sc->var.world));
    D.qacc = sc->accum_q.p;
    D.n = sc->var.samples; D.threshold = threshold; D.mean_floor = mean_floor;
    D.n_blocks = slot_grid(D.A).x;
    sc->fe_sum.ensure((size_t)kFeSums * D.n_blocks); sc->fe_cnt.ensure((size_t)kFeCounts * D.n_blocks);
    D.part_sum = sc->fe_sum.p; D.part_cnt = sc->fe_cnt.p;
    D.out = d_out;
    launch_frame_error(D, st);
    HIP_CHECK(hipGetLastError());
}

// Pixels of the shard (its pixel slots without the padding of ragged tiles and of tiles beyond the frame)
uint64_t shard_pixels(const crt_params& p, const Shard& sh)
{
    SlotMap m;
    fill_slot_map(m, p, (p.flags & CRT_FLAG_TILED_OUTPUT) != 0, sh);
    uint64_t n = 0;
    for (uint32_t lt = 0; lt < sh.local_tiles; lt++) n += tile_pixels(m, lt);
    return n;
}

// Argument checks of both forms of crt_render_until, before any device call; what the first range's render_impl refuses it refuses
// itself, before it touches the handle
int until_check(const crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_until_params* up, uint32_t s_begin, const void* out_rgb)
{
    const std::string w("crt_render_until");
    if (!cam) return fail(CRT_ERR_INVALID_ARG, w + ": null camera");
    if (!prm) return fail(CRT_ERR_INVALID_ARG, w + ": null params");
    if (!up) return fail(CRT_ERR_INVALID_ARG, w + ": null until params");
    if (!out_rgb) return fail(CRT_ERR_INVALID_ARG, w + ": null frame buffer (out_rgb)");
    if (up->min_samples < 2 || up->min_samples > prm->spp) return fail(CRT_ERR_INVALID_ARG, w + ": min_samples must be in [2, spp] (the variance needs two samples)");
    if (up->step_samples == 0) return fail(CRT_ERR_INVALID_ARG, w + ": step_samples must be positive");
    const int rc_c = criterion_check("crt_render_until", up->threshold, up->mean_floor);
    if (rc_c != CRT_OK) return rc_c;
    const int rc_p = params_check("crt_render", prm);
    if (rc_p != CRT_OK) return rc_p;
    if (!sc) return fail(CRT_ERR_INVALID_ARG, w + ": null scene");
    if (s_begin > 0) {
        const bool tiled = (prm->flags & CRT_FLAG_TILED_OUTPUT) != 0;
        if (!continues_frame(sc->acc, prm, s_begin, tiled) || !sc->var.valid || !continues_frame(sc->var, prm, s_begin, tiled))
            return fail(CRT_ERR_INVALID_ARG, w + ": sample_begin " + std::to_string(s_begin) + " must continue the frame in flight: exactly samples [0, sample_begin) of every pixel "
                                             "with CRT_FLAG_VARIANCE from sample 0 on, and the same spp, width, height, rank, world and CRT_FLAG_TILED_OUTPUT (" +
                                             sc->acc.in_flight(std::string(sc->var.valid ? ", with" : ", without") + " valid variance sums") + ")");
    }
    return CRT_OK;
}

int until_impl(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_until_params* up, uint32_t s_begin, void* d_rgb, void* d_mean, void* d_var,
               hipStream_t st, crt_until_info* info)
{
    const int rc0 = until_check(sc, cam, prm, up, s_begin, d_rgb);
    if (rc0 != CRT_OK) return rc0;
    crt_params p = *prm;
    p.flags |= CRT_FLAG_VARIANCE;
    const uint32_t S = p.spp;
    const bool timed = info != nullptr, mega = choose_pipeline(sc) == 4;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        crt_until_info I;
        std::memset(&I, 0, sizeof(I));
        double kernel_ms = 0.0;
        bool kernel_unread = false; // a range's launches have been enqueued whose time (ev_k0 .. ev_k1) has not been added yet
        uint32_t n = s_begin;
        // one range of the frame, as crt_render_range_device submits it; the first one's refusals come before anything has changed
        auto range = [&](uint32_t ns) -> int {
            const int rc = render_impl(sc, cam, &p, d_rgb, d_mean, st, nullptr, n, ns);
            if (rc != CRT_OK) return rc;
            kernel_unread = true;
            n += ns; I.passes++;
            return CRT_OK;
        };
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (timed) {
            ensure_events(sc);
            e0 = sc->ev[0]; e1 = sc->ev[1];
            HIP_CHECK(hipEventRecord(e0, st));
        }
        if (n < up->min_samples) {
            const int rc = range(up->min_samples - n);
            if (rc != CRT_OK) return rc;
        }
        sc->fe_info.ensure(1);
        if (!sc->h_fe) HIP_CHECK(hipHostMalloc((void**)&sc->h_fe, sizeof(crt_frame_error_info), hipHostMallocDefault));
        for (;;) {
            enqueue_frame_error(sc, up->threshold, up->mean_floor, sc->fe_info.p, st);
            HIP_CHECK(hipMemcpyAsync(&sc->h_fe->above, &sc->fe_info.p->above, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st)); // the one synchronization of a check: how many pixels are above the target
            if (timed && kernel_unread && mega && sc->last_launches) {
                float ms = 0.0f;
                HIP_CHECK(hipEventElapsedTime(&ms, sc->ev_k0, sc->ev_k1));
                kernel_ms += ms;
            }
            kernel_unread = false;
            const uint64_t above = sc->h_fe->above;
            if (I.checks < CRT_UNTIL_CHECKS_REPORTED) I.above[I.checks] = above;
            I.checks++;
            if (above <= up->max_above || n == S) break;
            const int rc = range(std::min(up->step_samples, S - n));
            if (rc != CRT_OK) return rc;
        }
        // n == S: the last range has written the frame.  Else the preview of the sums, and the frame stays in flight
        if (n < S) {
            const int rc = crt_preview_device(sc, d_rgb, d_mean, st, nullptr);
            if (rc != CRT_OK) return rc;
        }
        if (d_var) {
            const int rc = crt_variance_device(sc, d_var, st, nullptr);
            if (rc != CRT_OK) return rc;
        }
        if (!info) return CRT_OK;
        HIP_CHECK(hipMemcpyAsync(sc->h_fe, sc->fe_info.p, sizeof(crt_frame_error_info), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipEventRecord(e1, st));
        HIP_CHECK(hipStreamSynchronize(st));
        I.samples_done = n;
        I.paths = shard_pixels(p, make_shard(p.width, p.height, p.world)) * (uint64_t)(n - s_begin);
        I.kernel_ms = (float)kernel_ms;
        HIP_CHECK(hipEventElapsedTime(&I.total_ms, e0, e1));
        I.last = *sc->h_fe;
        *info = I;
        return CRT_OK;
    });
}

} // namespace

extern "C" {

int crt_frame_error_defaults(float* threshold, float* mean_floor)
{
    if (!threshold || !mean_floor) return fail(CRT_ERR_INVALID_ARG, "crt_frame_error_defaults: null argument");
    *threshold = 0.05f; *mean_floor = 0.01f;
    return CRT_OK;
}

int crt_frame_error_device(crt_scene* sc, float threshold, float mean_floor, void* d_out, void* stream)
{
    const int rc = frame_error_check(sc, threshold, mean_floor, d_out);
    if (rc != CRT_OK) return rc;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        enqueue_frame_error(sc, threshold, mean_floor, (crt_frame_error_info*)d_out, (hipStream_t)stream);
        return CRT_OK;
    });
}

int crt_frame_error(crt_scene* sc, float threshold, float mean_floor, crt_frame_error_info* out)
{
    const int rc0 = frame_error_check(sc, threshold, mean_floor, out);
    if (rc0 != CRT_OK) return rc0;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        sc->fe_info.ensure(1);
        enqueue_frame_error(sc, threshold, mean_floor, sc->fe_info.p, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        sc->fe_info.download(out, 1);
        return CRT_OK;
    });
}

int crt_until_defaults(crt_until_params* up)
{
    if (!up) return fail(CRT_ERR_INVALID_ARG, "crt_until_defaults: null argument");
    up->min_samples = 16; up->step_samples = 64; up->threshold = 0.05f; up->mean_floor = 0.01f; up->max_above = 0;
    return CRT_OK;
}

int crt_render_until_device(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_until_params* up, uint32_t sample_begin, void* d_rgb, void* d_mean,
                            void* d_variance, void* stream, crt_until_info* info)
{
    return until_impl(sc, cam, prm, up, sample_begin, d_rgb, d_mean, d_variance, (hipStream_t)stream, info);
}

int crt_render_until(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_until_params* up, uint32_t sample_begin, uint8_t* out_rgb, float* out_mean,
                     float* out_variance, crt_until_info* info)
{
    const int rc0 = until_check(sc, cam, prm, up, sample_begin, out_rgb);
    if (rc0 != CRT_OK) return rc0;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        const uint64_t npix = out_pixels(prm->width, prm->height, prm->world, (prm->flags & CRT_FLAG_TILED_OUTPUT) != 0);
        Staging s(npix, true, out_mean != nullptr), v(npix, false, out_variance != nullptr);
        const int rc = until_impl(sc, cam, prm, up, sample_begin, s.rgb.p, s.f32.p, v.f32.p, nullptr, info);
        if (rc != CRT_OK) return rc;
        s.download(out_rgb, out_mean);
        v.download(nullptr, out_variance);
        return CRT_OK;
    });
}

} // extern "C"
