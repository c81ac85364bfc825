// cudaraytracing_amd/csrc/crt_temporal.hip -- temporal accumulation with reprojection (crt_temporal, crt_temporal_clamped,
// crt_temporal_moments, crt_temporal_dual and their _device forms, contract: include/crt.h): kernels and host code.  An image operation
// without a scene handle, the temporal half of SVGF beside crt_denoise_var.  The pass is one operation with optional parts, and both
// halves of this file state it once: the kernels are launch shape and counting around the per-pixel text of crt_temporal.h (which
// tools/temporal_host_check.cpp compiles for the host, all of it), and every entry point is one bundle of arguments through one check,
// one parameter block and one launch.
//
// One call = one launch: one thread per pixel, block = 64 x 4 pixels, a wave = 64 consecutive pixels of one row (the denoiser's pass).
// A thread rebuilds the world point of its pixel from the current camera and the depth, projects it into the previous camera, gathers
// the four bilinear taps straight from the caller's buffers (neighbouring pixels of a row land on neighbouring taps unless the surface
// is seen at a grazing angle) and blends or resets.  The count of pixels that took the history is one ballot, one popcount and one
// atomic per wave, as k_adaptive_select counts its slots; it is kept only when the caller asks for the info.
//
// k_temporal<true, *> (crt_temporal_clamped) adds the neighbourhood clamp between the interpolation and the blend: mean and standard
// deviation of the current colour over the (2 radius + 1)^2 pixels around p, straight from the caller's buffer (a wave's 64 pixels share
// all but 2 radius columns of their taps), the history colour clamped to mean +- gamma deviations, and a second count on the same ballot
// path.  k_temporal<*, true> (crt_temporal_moments) carries two more history planes, the running first and second moments of the
// UNclamped colour: their taps ride on the predicates and the weight b of the colour's taps (24 B more per tap that counts), their blend
// on n, a and k, and 24 B more are stored per pixel.
//
// k_temporal_dual<CLAMP> (crt_temporal_dual) stays a kernel of its own, because it holds a ballot in the middle of the pixel's work: per
// pixel a second candidate history, fetched through the virtual image of what a mirror pixel shows (path_depth along its ray), and the
// choice between the two.  A wave in which no lane tries the second candidate skips it as one scalar branch.
#include "crt_filter_host.h"
#include "crt_temporal.h"

#include <cstring>
#include <string>

namespace crtk {

template <bool CLAMP, bool MOMENTS>
__global__ __launch_bounds__(256) void k_temporal(const TpParams P)
{
    const uint32_t by = blockIdx.x / P.tiles_x, bx = blockIdx.x - by * P.tiles_x;
    const int x = (int)(bx * 64u + (threadIdx.x & 63u)), y = (int)(by * 4u + (threadIdx.x >> 6));
    const bool inside = x < (int)P.width && y < (int)P.height;
    TpFlags fl = {};
    if (inside) fl = temporal_single<CLAMP, MOMENTS>(P, x, y);
    if (!P.count) return;
    const unsigned long long mask = __ballot(fl.took);
    if (mask == 0ull) return;
    const bool first = (int)(threadIdx.x & 63u) == __ffsll((long long)mask) - 1;
    if (first) __hip_atomic_fetch_add(P.count, (unsigned long long)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (CLAMP) { // (a clamped pixel took the history: the wave is still here, and `first` is one of its lanes)
        const unsigned long long cmask = __ballot(fl.clamped);
        if (cmask != 0ull && first)
            __hip_atomic_fetch_add(P.count + 1, (unsigned long long)__popcll(cmask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// crt_temporal_dual: the launch shape and the counting of k_temporal, the per-pixel work of crt_temporal.h.  The ballot between the two
// halves is held by every lane of the wave (lanes outside the image vote false), so its result is a scalar and the branch on it in
// temporal_dual_finish a scalar branch.
template <bool CLAMP>
__global__ __launch_bounds__(256) void k_temporal_dual(const TpDualParams P)
{
    const uint32_t by = blockIdx.x / P.tiles_x, bx = blockIdx.x - by * P.tiles_x;
    const int x = (int)(bx * 64u + (threadIdx.x & 63u)), y = (int)(by * 4u + (threadIdx.x >> 6));
    const bool inside = x < (int)P.width && y < (int)P.height;
    TpDualState st;
    st.tries = false;
    if (inside && P.pcolor) st = temporal_dual_begin(P, x, y);
    const unsigned long long tmask = __ballot(st.tries);
    const bool any_tries = tmask != 0ull;
    TpFlags fl = {};
    if (inside) fl = temporal_dual_finish<CLAMP>(P, x, y, st, any_tries);
    if (!P.count) return;
    // (a pixel can try V and take no history at all: the tried count comes before the wave leaves)
    if (any_tries && (int)(threadIdx.x & 63u) == __ffsll((long long)tmask) - 1)
        __hip_atomic_fetch_add(P.count + 2, (unsigned long long)__popcll(tmask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long mask = __ballot(fl.took);
    if (mask == 0ull) return;
    const bool first = (int)(threadIdx.x & 63u) == __ffsll((long long)mask) - 1;
    if (first) __hip_atomic_fetch_add(P.count, (unsigned long long)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (CLAMP) { // (a clamped pixel took the history: the wave is still here, and `first` is one of its lanes)
        const unsigned long long cmask = __ballot(fl.clamped);
        if (cmask != 0ull && first)
            __hip_atomic_fetch_add(P.count + 1, (unsigned long long)__popcll(cmask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned long long vmask = __ballot(fl.took_V);
    if (vmask != 0ull && first)
        __hip_atomic_fetch_add(P.count + 3, (unsigned long long)__popcll(vmask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

} // namespace crtk

using namespace crtk;

namespace {

const uint32_t CLAMP_DEFAULT_RADIUS = 1;   // crt_temporal_clamp_defaults: chosen by the sweep of docs/experiments.md
const float CLAMP_DEFAULT_GAMMA = 1.0f;
bool tolerance_ok(float t) { return t > 0.0f; } // (false for NaN)

// The arguments of every form of the pass, on host buffers or on device buffers: what all eight entry points take, then the parts that
// only crt_temporal_moments / _device and only crt_temporal_dual / _device have (null in the other forms)
enum TemporalForm { FORM_PLAIN, FORM_MOMENTS, FORM_DUAL };
struct TemporalArgs {
    const crt_temporal_params* prm;
    const crt_temporal_clamp* clamp;                // null: no clamp (always null for crt_temporal / _device)
    const crt_temporal_frame* cur;
    const crt_temporal_history* prev;
    void* out_color; void* out_variance; void* out_history; void* out_rgb;
    TemporalForm form = FORM_PLAIN;
    const crt_temporal_moment_planes* prev_moments = nullptr; // FORM_MOMENTS: the history's moment planes (null iff there is no history) and the two outputs
    void* out_m1 = nullptr; void* out_m2 = nullptr;
    const crt_temporal_dual_params* dual = nullptr; // FORM_DUAL
    const crt_temporal_specular_planes* cur_spec = nullptr; const crt_temporal_specular_planes* prev_spec = nullptr;
};

// The argument checks of every form, before any device call.  (The dual arguments first: the checks end with the sizes the launch cannot cover.)
int temporal_check(const char* who, const TemporalArgs& a)
{
    const std::string w(who);
    const crt_temporal_params* prm = a.prm;
    const crt_temporal_frame* cur = a.cur;
    const crt_temporal_history* prev = a.prev;
    if (a.form == FORM_DUAL && prm && cur) {
        const crt_temporal_specular_planes *cur_spec = a.cur_spec, *prev_spec = a.prev_spec;
        if (!a.dual || !cur_spec) return fail(CRT_ERR_INVALID_ARG, w + ": null argument");
        if (a.dual->radius < 1 || a.dual->radius > 3) return fail(CRT_ERR_INVALID_ARG, w + ": the dual reprojection's radius must be 1 .. 3");
        if (!(a.dual->min_bounces > 0.0f)) return fail(CRT_ERR_INVALID_ARG, w + ": min_bounces must be > 0 (+inf never tries)"); // (false for NaN)
        if ((prev != nullptr) != (prev_spec != nullptr))
            return fail(CRT_ERR_INVALID_ARG, w + ": a history and its specular planes go together");
        if (!cur_spec->path_depth || !cur_spec->bounces || (prev_spec && (!prev_spec->path_depth || !prev_spec->bounces)))
            return fail(CRT_ERR_INVALID_ARG, w + ": the specular planes need path_depth and bounces");
        if (prev_spec && (cur_spec->last_normal != nullptr) != (prev_spec->last_normal != nullptr))
            return fail(CRT_ERR_INVALID_ARG, w + ": last normals must be given in both frames or in neither");
    }
    if (!prm || !cur) return fail(CRT_ERR_INVALID_ARG, w + ": null argument");
    if (!cur->color || !cur->depth) return fail(CRT_ERR_INVALID_ARG, w + ": the current frame needs colour and depth");
    if (!a.out_color || !a.out_history) return fail(CRT_ERR_INVALID_ARG, w + ": out_color and out_history are required");
    if (const int rc = size_positive(w, prm->width, prm->height)) return rc;
    if (!tolerance_ok(prm->depth_tolerance) || !tolerance_ok(prm->normal_tolerance))
        return fail(CRT_ERR_INVALID_ARG, w + ": every tolerance must be > 0 (+inf switches a test off)");
    if (!(prm->alpha_min > 0.0f && prm->alpha_min <= 1.0f)) return fail(CRT_ERR_INVALID_ARG, w + ": alpha_min must be in (0, 1]");
    if ((cur->variance != nullptr) != (a.out_variance != nullptr))
        return fail(CRT_ERR_INVALID_ARG, w + ": the current variance and out_variance go together");
    if (prev) {
        if (!prev->color || !prev->history || !prev->depth) return fail(CRT_ERR_INVALID_ARG, w + ": a history needs colour, history length and depth");
        if (cur->variance && !prev->variance) return fail(CRT_ERR_INVALID_ARG, w + ": the history has no variance");
        if ((cur->normal != nullptr) != (prev->normal != nullptr)) return fail(CRT_ERR_INVALID_ARG, w + ": normals must be given in both frames or in neither");
        if ((cur->id != nullptr) != (prev->id != nullptr)) return fail(CRT_ERR_INVALID_ARG, w + ": IDs must be given in both frames or in neither");
    }
    if (a.form == FORM_MOMENTS) {
        if (!a.out_m1 || !a.out_m2) return fail(CRT_ERR_INVALID_ARG, w + ": out_m1 and out_m2 are required");
        if ((prev != nullptr) != (a.prev_moments != nullptr))
            return fail(CRT_ERR_INVALID_ARG, w + ": a history and its moment planes go together");
        if (a.prev_moments && (!a.prev_moments->m1 || !a.prev_moments->m2)) return fail(CRT_ERR_INVALID_ARG, w + ": the moment planes need m1 and m2");
    }
    if (a.clamp) {
        if (a.clamp->radius < 1 || a.clamp->radius > 3) return fail(CRT_ERR_INVALID_ARG, w + ": the clamp's radius must be 1 .. 3");
        if (!(a.clamp->gamma >= 0.0f)) return fail(CRT_ERR_INVALID_ARG, w + ": the clamp's gamma must be >= 0 (+inf never clamps)"); // (false for NaN)
    }
    return size_supported(w, prm->width, prm->height, 64, 4);
}

void set_camera(const crt_camera& cam, float* eye, float* iv, float& scale)
{
    std::memcpy(eye, cam.eye, sizeof(cam.eye));
    std::memcpy(iv, cam.inv_view, sizeof(cam.inv_view));
    scale = det_tanf(cam.fov_y / 2);
}

// what the info structs are filled from
struct TemporalCounts { float total_ms; unsigned long long reprojected, clamped, tried, taken; };

// the parameter block of a checked call on device buffers (count: the launch's)
void fill_params(TpDualParams& P, const TemporalArgs& a)
{
    const crt_temporal_params* prm = a.prm;
    std::memset(&P, 0, sizeof(P));
    P.width = prm->width; P.height = prm->height;
    P.tiles_x = (prm->width + 63) / 64;
    set_camera(prm->cur, P.eye, P.iv, P.scale);
    set_camera(prm->prev, P.peye, P.piv, P.pscale);
    P.ar = (float)prm->width / (float)prm->height;
    P.depth_tol = prm->depth_tolerance;
    P.normal_tol2 = prm->normal_tolerance * prm->normal_tolerance;
    P.alpha_min = prm->alpha_min;
    P.color = a.cur->color; P.variance = a.cur->variance; P.depth = a.cur->depth;
    if (a.prev) {
        P.normal = a.cur->normal; P.id = a.cur->id; // (without a history nothing reads the guides)
        P.pcolor = a.prev->color; P.pvariance = a.prev->variance; P.phistory = a.prev->history; P.pdepth = a.prev->depth;
        P.pnormal = a.prev->normal; P.pid = a.prev->id;
    }
    P.out_mean = (float*)a.out_color; P.out_rgb = (uint8_t*)a.out_rgb;
    P.out_variance = (float*)a.out_variance; P.out_history = (float*)a.out_history;
    if (a.clamp) { P.radius = (int)a.clamp->radius; P.gamma = a.clamp->gamma; }
    if (a.form == FORM_MOMENTS) {
        if (a.prev_moments) { P.pm1 = a.prev_moments->m1; P.pm2 = a.prev_moments->m2; }
        P.out_m1 = (float*)a.out_m1; P.out_m2 = (float*)a.out_m2;
    }
    if (a.form == FORM_DUAL) {
        P.dual_radius = (int)a.dual->radius; P.min_bounces = a.dual->min_bounces;
        if (a.prev) { // (without a history nothing reads the specular planes)
            P.path_depth = a.cur_spec->path_depth; P.bounces = a.cur_spec->bounces; P.last_normal = a.cur_spec->last_normal;
            P.ppath_depth = a.prev_spec->path_depth; P.pbounces = a.prev_spec->bounces; P.plast_normal = a.prev_spec->last_normal;
        }
    }
}

// A checked call on device buffers: its one kernel, and with an info its counts (two, the dual form's four)
int temporal_launch(const char* who, int device, const TemporalArgs& a, hipStream_t st, TemporalCounts* info)
{
    TpDualParams P;
    fill_params(P, a);
    unsigned long long n[4] = {0, 0, 0, 0};
    const int status = timed_launch(who, device, st, info, n, a.form == FORM_DUAL ? 4 : 2, [&](unsigned long long* d_count) {
        P.count = d_count;
        const dim3 grid(P.tiles_x * ((P.height + 3) / 4)), block(256);
        const TpParams& S = P; // (k_temporal takes the base alone)
        if (a.form == FORM_DUAL) {
            if (a.clamp) hipLaunchKernelGGL((k_temporal_dual<true>), grid, block, 0, st, P);
            else hipLaunchKernelGGL((k_temporal_dual<false>), grid, block, 0, st, P);
        } else if (a.form == FORM_MOMENTS) {
            if (a.clamp) hipLaunchKernelGGL((k_temporal<true, true>), grid, block, 0, st, S);
            else hipLaunchKernelGGL((k_temporal<false, true>), grid, block, 0, st, S);
        } else if (a.clamp) hipLaunchKernelGGL((k_temporal<true, false>), grid, block, 0, st, S);
        else hipLaunchKernelGGL((k_temporal<false, false>), grid, block, 0, st, S);
    });
    if (status == CRT_OK && info) { info->reprojected = n[0]; info->clamped = n[1]; info->tried = n[2]; info->taken = n[3]; }
    return status;
}

// the info structs, filled from the counts of a call that succeeded
void fill_info(crt_temporal_info* info, const TemporalCounts& n)
{
    std::memset(info, 0, sizeof(*info));
    info->total_ms = n.total_ms; info->reprojected = n.reprojected;
}
void fill_info(crt_temporal_clamp_info* info, const TemporalCounts& n)
{
    std::memset(info, 0, sizeof(*info));
    info->total_ms = n.total_ms; info->reprojected = n.reprojected; info->clamped = n.clamped;
}
void fill_info(crt_temporal_dual_info* info, const TemporalCounts& n)
{
    std::memset(info, 0, sizeof(*info));
    info->total_ms = n.total_ms; info->reprojected = n.reprojected; info->clamped = n.clamped;
    info->virtual_tried = n.tried; info->virtual_taken = n.taken;
}

// The device-buffer form: the argument checks, then the launch on the caller's stream.
template <class Info> int temporal_device_form(const char* who, int device, const TemporalArgs& a, void* stream, Info* info)
{
    const int rc0 = temporal_check(who, a);
    if (rc0 != CRT_OK) return rc0;
    TemporalCounts n{};
    const int rc = temporal_launch(who, device, a, (hipStream_t)stream, info ? &n : nullptr);
    if (rc == CRT_OK && info) fill_info(info, n);
    return rc;
}

// device copies of the planes of a frame, of a history and of a frame's specular planes (a plane that is not given stays null)
crt_temporal_frame copy_in(HostCopies& c, const crt_temporal_frame& f, uint64_t npix)
{
    return {c.in(f.color, npix * 3), c.in(f.variance, npix * 3), c.in(f.depth, npix), c.in(f.normal, npix * 3), c.in(f.id, npix)};
}
crt_temporal_history copy_in(HostCopies& c, const crt_temporal_history& f, uint64_t npix)
{
    return {c.in(f.color, npix * 3), c.in(f.variance, npix * 3), c.in(f.history, npix), c.in(f.depth, npix), c.in(f.normal, npix * 3), c.in(f.id, npix)};
}
crt_temporal_specular_planes copy_in(HostCopies& c, const crt_temporal_specular_planes& f, uint64_t npix)
{
    return {c.in(f.path_depth, npix), c.in(f.bounces, npix), c.in(f.last_normal, npix * 3)};
}

// The host-buffer form: the argument checks, the same call on device copies of its buffers, then the copies back.
template <class Info> int temporal_host_form(const char* who, int device, const TemporalArgs& a, Info* info)
{
    const int rc0 = temporal_check(who, a);
    if (rc0 != CRT_OK) return rc0;
    const uint64_t npix = (uint64_t)a.prm->width * a.prm->height;
    TemporalCounts n{};
    const int rc = host_form(who, device, [&](HostCopies& c) {
        TemporalArgs d = a;
        const crt_temporal_frame cur = copy_in(c, *a.cur, npix);
        crt_temporal_history prev{};
        crt_temporal_specular_planes cur_spec{}, prev_spec{};
        crt_temporal_moment_planes prev_moments{};
        d.cur = &cur;
        if (a.prev) { prev = copy_in(c, *a.prev, npix); d.prev = &prev; }
        if (a.form == FORM_DUAL) {
            cur_spec = copy_in(c, *a.cur_spec, npix); d.cur_spec = &cur_spec;
            if (a.prev) { prev_spec = copy_in(c, *a.prev_spec, npix); d.prev_spec = &prev_spec; }
        }
        if (a.prev_moments) {
            prev_moments = {c.in(a.prev_moments->m1, npix * 3), c.in(a.prev_moments->m2, npix * 3)};
            d.prev_moments = &prev_moments;
        }
        d.out_color = c.out((float*)a.out_color, npix * 3); d.out_history = c.out((float*)a.out_history, npix);
        d.out_variance = c.out((float*)a.out_variance, npix * 3); d.out_rgb = c.out((uint8_t*)a.out_rgb, npix * 3);
        d.out_m1 = c.out((float*)a.out_m1, npix * 3); d.out_m2 = c.out((float*)a.out_m2, npix * 3);
        return temporal_launch(who, device, d, nullptr, info ? &n : nullptr);
    });
    if (rc == CRT_OK && info) fill_info(info, n);
    return rc;
}

// the bundles of the three kinds of entry point
TemporalArgs plain_args(const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_frame* cur, const crt_temporal_history* prev,
                        void* out_color, void* out_variance, void* out_history, void* out_rgb)
{
    return {prm, clamp, cur, prev, out_color, out_variance, out_history, out_rgb};
}
TemporalArgs moments_args(TemporalArgs a, const crt_temporal_moment_planes* prev_moments, void* out_m1, void* out_m2)
{
    a.form = FORM_MOMENTS; a.prev_moments = prev_moments; a.out_m1 = out_m1; a.out_m2 = out_m2;
    return a;
}
TemporalArgs dual_args(TemporalArgs a, const crt_temporal_dual_params* dual, const crt_temporal_specular_planes* cur_spec, const crt_temporal_specular_planes* prev_spec)
{
    a.form = FORM_DUAL; a.dual = dual; a.cur_spec = cur_spec; a.prev_spec = prev_spec;
    return a;
}

} // namespace

extern "C" {

int crt_temporal_defaults(crt_temporal_params* prm)
{
    if (!prm) return fail(CRT_ERR_INVALID_ARG, "crt_temporal_defaults: null argument");
    std::memset(prm, 0, sizeof(*prm));
    prm->depth_tolerance = 0.05f; prm->normal_tolerance = 0.5f; prm->alpha_min = 0.05f;
    return CRT_OK;
}

int crt_temporal_clamp_defaults(crt_temporal_clamp* clamp)
{
    if (!clamp) return fail(CRT_ERR_INVALID_ARG, "crt_temporal_clamp_defaults: null argument");
    std::memset(clamp, 0, sizeof(*clamp));
    clamp->radius = CLAMP_DEFAULT_RADIUS; clamp->gamma = CLAMP_DEFAULT_GAMMA;
    return CRT_OK;
}

int crt_temporal_dual_defaults(crt_temporal_dual_params* dual)
{
    if (!dual) return fail(CRT_ERR_INVALID_ARG, "crt_temporal_dual_defaults: null argument");
    std::memset(dual, 0, sizeof(*dual));
    dual->radius = 1; dual->min_bounces = 0.5f; // tuned on nothing (include/crt.h)
    return CRT_OK;
}

int crt_temporal_device(int device, const crt_temporal_params* prm, const crt_temporal_frame* dev_cur, const crt_temporal_history* dev_prev,
                        void* d_out_color, void* d_out_variance, void* d_out_history, void* d_out_rgb, void* stream, crt_temporal_info* info)
{
    return temporal_device_form("crt_temporal_device", device, plain_args(prm, nullptr, dev_cur, dev_prev, d_out_color, d_out_variance, d_out_history, d_out_rgb),
                                stream, info);
}

int crt_temporal(int device, const crt_temporal_params* prm, const crt_temporal_frame* host_cur, const crt_temporal_history* host_prev, float* out_color,
                 float* out_variance, float* out_history, uint8_t* out_rgb, crt_temporal_info* info)
{
    return temporal_host_form("crt_temporal", device, plain_args(prm, nullptr, host_cur, host_prev, out_color, out_variance, out_history, out_rgb), info);
}

int crt_temporal_clamped_device(int device, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_frame* dev_cur,
                                const crt_temporal_history* dev_prev, void* d_out_color, void* d_out_variance, void* d_out_history, void* d_out_rgb,
                                void* stream, crt_temporal_clamp_info* info)
{
    return temporal_device_form("crt_temporal_clamped_device", device,
                                plain_args(prm, clamp, dev_cur, dev_prev, d_out_color, d_out_variance, d_out_history, d_out_rgb), stream, info);
}

int crt_temporal_clamped(int device, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_frame* host_cur,
                         const crt_temporal_history* host_prev, float* out_color, float* out_variance, float* out_history, uint8_t* out_rgb,
                         crt_temporal_clamp_info* info)
{
    return temporal_host_form("crt_temporal_clamped", device, plain_args(prm, clamp, host_cur, host_prev, out_color, out_variance, out_history, out_rgb), info);
}

int crt_temporal_moments_device(int device, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_frame* dev_cur,
                                const crt_temporal_history* dev_prev, const crt_temporal_moment_planes* dev_prev_moments, void* d_out_color,
                                void* d_out_variance, void* d_out_history, void* d_out_m1, void* d_out_m2, void* d_out_rgb, void* stream,
                                crt_temporal_clamp_info* info)
{
    return temporal_device_form("crt_temporal_moments_device", device,
                                moments_args(plain_args(prm, clamp, dev_cur, dev_prev, d_out_color, d_out_variance, d_out_history, d_out_rgb), dev_prev_moments,
                                             d_out_m1, d_out_m2),
                                stream, info);
}

int crt_temporal_moments(int device, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_frame* host_cur,
                         const crt_temporal_history* host_prev, const crt_temporal_moment_planes* host_prev_moments, float* out_color,
                         float* out_variance, float* out_history, float* out_m1, float* out_m2, uint8_t* out_rgb, crt_temporal_clamp_info* info)
{
    return temporal_host_form("crt_temporal_moments", device,
                              moments_args(plain_args(prm, clamp, host_cur, host_prev, out_color, out_variance, out_history, out_rgb), host_prev_moments, out_m1,
                                           out_m2),
                              info);
}

int crt_temporal_dual_device(int device, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_dual_params* dual,
                             const crt_temporal_frame* dev_cur, const crt_temporal_specular_planes* dev_cur_spec, const crt_temporal_history* dev_prev,
                             const crt_temporal_specular_planes* dev_prev_spec, void* d_out_color, void* d_out_variance, void* d_out_history,
                             void* d_out_rgb, void* stream, crt_temporal_dual_info* info)
{
    return temporal_device_form("crt_temporal_dual_device", device,
                                dual_args(plain_args(prm, clamp, dev_cur, dev_prev, d_out_color, d_out_variance, d_out_history, d_out_rgb), dual, dev_cur_spec,
                                          dev_prev_spec),
                                stream, info);
}

int crt_temporal_dual(int device, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_dual_params* dual,
                      const crt_temporal_frame* cur, const crt_temporal_specular_planes* cur_spec, const crt_temporal_history* prev,
                      const crt_temporal_specular_planes* prev_spec, float* out_color, float* out_variance, float* out_history, uint8_t* out_rgb,
                      crt_temporal_dual_info* info)
{
    return temporal_host_form("crt_temporal_dual", device,
                              dual_args(plain_args(prm, clamp, cur, prev, out_color, out_variance, out_history, out_rgb), dual, cur_spec, prev_spec), info);
}

} // extern "C"
