// cudaraytracing_amd/csrc/crt_temporal.hip -- temporal accumulation with reprojection (crt_temporal / crt_temporal_device, contract:
// include/crt.h): kernel and host code.  An image operation without a scene handle, the temporal half of SVGF beside crt_denoise_var.
//
// One call = one launch of k_temporal: one thread per pixel, block = 64 x 4 pixels, a wave = 64 consecutive pixels of one row (the
// denoiser's pass).  A thread rebuilds the world point of its pixel from the current camera and the depth, projects it into the
// previous camera, gathers the four bilinear taps straight from the caller's buffers (neighbouring pixels of a row land on neighbouring
// taps unless the surface is seen at a grazing angle) and blends or resets.  The count of pixels that took the history is one ballot,
// one popcount and one atomic per wave, as k_adaptive_select counts its slots; it is kept only when the caller asks for the info.
//
// k_temporal<true> (crt_temporal_clamped) adds the neighbourhood clamp between the interpolation and the blend: mean and standard
// deviation of the current colour over the (2 radius + 1)^2 pixels around p, straight from the caller's buffer (a wave's 64 pixels share
// all but 2 radius columns of their taps), the history colour clamped to mean +- gamma deviations, and a second count on the same ballot
// path.  The statistics run INSIDE the branch of the pixels that take the history, not before it: see docs/experiments.md.
//
// k_temporal<CLAMP, true> (crt_temporal_moments) carries two more history planes, the running first and second moments of the UNclamped
// colour: their taps ride on the predicates and the weight b of the colour's taps (24 B more per tap that counts), their blend on n, a
// and k, and 24 B more are stored per pixel.  <false, false> and <true, false> are the kernels of the older entry points, instruction
// for instruction what they were before the third parameter (the new fields of TpParams stand at its end).
//
// k_temporal_dual<CLAMP> (crt_temporal_dual) is a sibling, not a third parameter, so that those four keep their instructions: per pixel a
// second candidate history, fetched through the virtual image of what a mirror pixel shows (path_depth along its ray), and the choice
// between the two (crt_temporal.h has the arithmetic; tools/temporal_host_check.cpp runs that text on the host).  A wave in which no lane
// tries the second candidate skips it as one scalar branch.  TpParams and history_channel live in crt_temporal.h.
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
    const int W = (int)P.width, H = (int)P.height;
    const bool inside = x < W && y < H;
    bool took = false, clamped = false;
    if (inside) {
        const size_t p = (size_t)y * P.width + (size_t)x;
        const F3 c = f3(P.color[p * 3], P.color[p * 3 + 1], P.color[p * 3 + 2]);
        F3 v = f3(0.0f, 0.0f, 0.0f);
        if (P.variance) v = f3(P.variance[p * 3], P.variance[p * 3 + 1], P.variance[p * 3 + 2]);
        F3 oc = c, ov = v;
        float oh = 1.0f;
        F3 o1 = c, o2 = f3(0.0f, 0.0f, 0.0f);
        if (MOMENTS) o2 = f3(c.x * c.x, c.y * c.y, c.z * c.z);
        if (P.pcolor) {
            const float fw = (float)W, fh = (float)H, dp = P.depth[p];
            // the pixel-centre ray of the current camera (camera_dir without the jitter) and the point it reaches at the stored depth
            const float sx = (((2 * ((float)x + 0.5f)) / fw - 1) * P.scale) * P.ar;
            const float sy = (1 - (2 * ((float)y + 0.5f)) / fh) * P.scale;
            const F3 cd = unit3(f3(-sx, sy, 1));
            const F3 d = unit3(f3(P.iv[0] * cd.x + (P.iv[3] * cd.y + P.iv[6] * cd.z),
                                  P.iv[1] * cd.x + (P.iv[4] * cd.y + P.iv[7] * cd.z),
                                  P.iv[2] * cd.x + (P.iv[5] * cd.y + P.iv[8] * cd.z)));
            const F3 wp = f3(P.eye[0] + d.x * dp, P.eye[1] + d.y * dp, P.eye[2] + d.z * dp);
            // into the previous camera: inverse of its rotation (the transpose), then the inverse of the image-plane map
            const F3 pv = f3(wp.x - P.peye[0], wp.y - P.peye[1], wp.z - P.peye[2]);
            const float cx = P.piv[0] * pv.x + (P.piv[1] * pv.y + P.piv[2] * pv.z);
            const float cy = P.piv[3] * pv.x + (P.piv[4] * pv.y + P.piv[5] * pv.z);
            const float cz = P.piv[6] * pv.x + (P.piv[7] * pv.y + P.piv[8] * pv.z);
            const float tp = sqrt_f(dot3(pv, pv));
            const float fx = (((((-cx) / cz) / (P.pscale * P.ar)) + 1) * fw) / 2 - 0.5f;
            const float fy = (((1 - (cy / cz) / P.pscale) * fh) / 2) - 0.5f;
            const bool ok = dp > 0.0f && cz > 0.0f && fx > -1.0f && fx < fw && fy > -1.0f && fy < fh; // (false for NaN)
            if (ok) {
                const float flx = floorf(fx), fly = floorf(fy);
                const float wx = fx - flx, wy = fy - fly;
                const int x0 = (int)flx, y0 = (int)fly; // -1 .. W - 1, -1 .. H - 1
                const float tol = P.depth_tol * tp;
                F3 n = f3(0.0f, 0.0f, 0.0f);
                if (P.normal) n = f3(P.normal[p * 3], P.normal[p * 3 + 1], P.normal[p * 3 + 2]);
                const int32_t idp = P.id ? P.id[p] : 0;
                F3 hc = f3(0.0f, 0.0f, 0.0f), hv = f3(0.0f, 0.0f, 0.0f), h1 = f3(0.0f, 0.0f, 0.0f), h2 = f3(0.0f, 0.0f, 0.0f);
                float hn = 0.0f, ws = 0.0f;
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const int qy = y0 + j;
                    if (qy < 0 || qy >= H) continue;
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const int qx = x0 + i;
                        if (qx < 0 || qx >= W) continue;
                        const size_t q = (size_t)qy * P.width + (size_t)qx;
                        const float pd = P.pdepth[q];
                        if (!(pd > 0.0f)) continue;
                        if (!(fabsf(pd - tp) <= tol)) continue;
                        if (P.normal) {
                            const float dnx = n.x - P.pnormal[q * 3], dny = n.y - P.pnormal[q * 3 + 1], dnz = n.z - P.pnormal[q * 3 + 2];
                            if (!(dnx * dnx + dny * dny + dnz * dnz <= P.normal_tol2)) continue;
                        }
                        if (P.id && idp != P.pid[q]) continue;
                        const float b = (i ? wx : 1 - wx) * (j ? wy : 1 - wy);
                        hc.x = hc.x + P.pcolor[q * 3] * b;
                        hc.y = hc.y + P.pcolor[q * 3 + 1] * b;
                        hc.z = hc.z + P.pcolor[q * 3 + 2] * b;
                        if (P.variance) {
                            hv.x = hv.x + P.pvariance[q * 3] * b;
                            hv.y = hv.y + P.pvariance[q * 3 + 1] * b;
                            hv.z = hv.z + P.pvariance[q * 3 + 2] * b;
                        }
                        if (MOMENTS) {
                            h1.x = h1.x + P.pm1[q * 3] * b;
                            h1.y = h1.y + P.pm1[q * 3 + 1] * b;
                            h1.z = h1.z + P.pm1[q * 3 + 2] * b;
                            h2.x = h2.x + P.pm2[q * 3] * b;
                            h2.y = h2.y + P.pm2[q * 3 + 1] * b;
                            h2.z = h2.z + P.pm2[q * 3 + 2] * b;
                        }
                        hn = hn + P.phistory[q] * b;
                        ws = ws + b;
                    }
                }
                if (ws > 0.015625f) {
                    took = true;
                    hn = hn / ws;
                    oh = hn + 1;
                    float a = 1 / oh;
                    a = a < P.alpha_min ? P.alpha_min : a;
                    const float k = 1 - a;
                    // sums of the current colour and its squares around p; every tap is tested against the image, so every read is inside it
                    F3 s1 = f3(0.0f, 0.0f, 0.0f), s2 = f3(0.0f, 0.0f, 0.0f);
                    float cnt = 0.0f;
                    if (CLAMP) {
                        for (int dy = -P.radius; dy <= P.radius; dy++) {
                            const int ty = y + dy;
                            if (ty < 0 || ty >= H) continue;
                            for (int dx = -P.radius; dx <= P.radius; dx++) {
                                const int tx = x + dx;
                                if (tx < 0 || tx >= W) continue;
                                const size_t t = ((size_t)ty * P.width + (size_t)tx) * 3;
                                const float tr = P.color[t], tg = P.color[t + 1], tb = P.color[t + 2];
                                s1.x = s1.x + tr; s1.y = s1.y + tg; s1.z = s1.z + tb;
                                s2.x = s2.x + tr * tr; s2.y = s2.y + tg * tg; s2.z = s2.z + tb * tb;
                                cnt = cnt + 1;
                            }
                        }
                    }
                    oc = f3(history_channel<CLAMP>(hc.x, ws, s1.x, s2.x, cnt, P.gamma, clamped) * k + c.x * a,
                            history_channel<CLAMP>(hc.y, ws, s1.y, s2.y, cnt, P.gamma, clamped) * k + c.y * a,
                            history_channel<CLAMP>(hc.z, ws, s1.z, s2.z, cnt, P.gamma, clamped) * k + c.z * a);
                    if (P.variance) {
                        const float kk = k * k, aa = a * a;
                        ov = f3((hv.x / ws) * kk + v.x * aa, (hv.y / ws) * kk + v.y * aa, (hv.z / ws) * kk + v.z * aa);
                    }
                    if (MOMENTS) { // never clamped: m1 is the running mean of what the pixel was seen to show
                        o1 = f3((h1.x / ws) * k + c.x * a, (h1.y / ws) * k + c.y * a, (h1.z / ws) * k + c.z * a);
                        o2 = f3((h2.x / ws) * k + o2.x * a, (h2.y / ws) * k + o2.y * a, (h2.z / ws) * k + o2.z * a);
                    }
                }
            }
        }
        write_color(P, p, true, oc);
        if (P.out_variance) { P.out_variance[p * 3] = ov.x; P.out_variance[p * 3 + 1] = ov.y; P.out_variance[p * 3 + 2] = ov.z; }
        P.out_history[p] = oh;
        if (MOMENTS) {
            P.out_m1[p * 3] = o1.x; P.out_m1[p * 3 + 1] = o1.y; P.out_m1[p * 3 + 2] = o1.z;
            P.out_m2[p * 3] = o2.x; P.out_m2[p * 3 + 1] = o2.y; P.out_m2[p * 3 + 2] = o2.z;
        }
    }
    if (!P.count) return;
    const unsigned long long mask = __ballot(took);
    if (mask == 0ull) return;
    const bool first = (int)(threadIdx.x & 63u) == __ffsll((long long)mask) - 1;
    if (first) __hip_atomic_fetch_add(P.count, (unsigned long long)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (CLAMP) { // (a clamped pixel took the history: the wave is still here, and `first` is one of its lanes)
        const unsigned long long cmask = __ballot(clamped);
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
    TpDualFlags fl;
    fl.took = false; fl.clamped = false; fl.tried = false; fl.took_V = false;
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

// crt_temporal_moments / _device: the history's moment planes (null iff there is no history) and the two outputs
struct MomentArgs { const crt_temporal_moment_planes* prev; void* out_m1; void* out_m2; };

// Argument checks of all six calls, before any device call (clamp: null for crt_temporal / crt_temporal_device; mom: null for all but
// crt_temporal_moments / _device)
int temporal_check(const char* who, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_frame* cur,
                   const crt_temporal_history* prev, const void* out_color, const void* out_variance, const void* out_history,
                   const MomentArgs* mom)
{
    const std::string w(who);
    if (!prm || !cur) return fail(CRT_ERR_INVALID_ARG, w + ": null argument");
    if (!cur->color || !cur->depth) return fail(CRT_ERR_INVALID_ARG, w + ": the current frame needs colour and depth");
    if (!out_color || !out_history) return fail(CRT_ERR_INVALID_ARG, w + ": out_color and out_history are required");
    if (const int rc = size_positive(w, prm->width, prm->height)) return rc;
    if (!tolerance_ok(prm->depth_tolerance) || !tolerance_ok(prm->normal_tolerance))
        return fail(CRT_ERR_INVALID_ARG, w + ": every tolerance must be > 0 (+inf switches a test off)");
    if (!(prm->alpha_min > 0.0f && prm->alpha_min <= 1.0f)) return fail(CRT_ERR_INVALID_ARG, w + ": alpha_min must be in (0, 1]");
    if ((cur->variance != nullptr) != (out_variance != nullptr))
        return fail(CRT_ERR_INVALID_ARG, w + ": the current variance and out_variance go together");
    if (prev) {
        if (!prev->color || !prev->history || !prev->depth) return fail(CRT_ERR_INVALID_ARG, w + ": a history needs colour, history length and depth");
        if (cur->variance && !prev->variance) return fail(CRT_ERR_INVALID_ARG, w + ": the history has no variance");
        if ((cur->normal != nullptr) != (prev->normal != nullptr)) return fail(CRT_ERR_INVALID_ARG, w + ": normals must be given in both frames or in neither");
        if ((cur->id != nullptr) != (prev->id != nullptr)) return fail(CRT_ERR_INVALID_ARG, w + ": IDs must be given in both frames or in neither");
    }
    if (mom) {
        if (!mom->out_m1 || !mom->out_m2) return fail(CRT_ERR_INVALID_ARG, w + ": out_m1 and out_m2 are required");
        if ((prev != nullptr) != (mom->prev != nullptr))
            return fail(CRT_ERR_INVALID_ARG, w + ": a history and its moment planes go together");
        if (mom->prev && (!mom->prev->m1 || !mom->prev->m2)) return fail(CRT_ERR_INVALID_ARG, w + ": the moment planes need m1 and m2");
    }
    if (clamp) {
        if (clamp->radius < 1 || clamp->radius > 3) return fail(CRT_ERR_INVALID_ARG, w + ": the clamp's radius must be 1 .. 3");
        if (!(clamp->gamma >= 0.0f)) return fail(CRT_ERR_INVALID_ARG, w + ": the clamp's gamma must be >= 0 (+inf never clamps)"); // (false for NaN)
    }
    return size_supported(w, prm->width, prm->height, 64, 4);
}

// crt_temporal_dual / _device: what they refuse beyond temporal_check, before any device call
int temporal_dual_check(const std::string& w, const crt_temporal_dual_params* dual, const crt_temporal_history* prev, const crt_temporal_specular_planes* cur_spec,
                        const crt_temporal_specular_planes* prev_spec)
{
    if (!dual || !cur_spec) return fail(CRT_ERR_INVALID_ARG, w + ": null argument");
    if (dual->radius < 1 || dual->radius > 3) return fail(CRT_ERR_INVALID_ARG, w + ": the dual reprojection's radius must be 1 .. 3");
    if (!(dual->min_bounces > 0.0f)) return fail(CRT_ERR_INVALID_ARG, w + ": min_bounces must be > 0 (+inf never tries)"); // (false for NaN)
    if ((prev != nullptr) != (prev_spec != nullptr))
        return fail(CRT_ERR_INVALID_ARG, w + ": a history and its specular planes go together");
    if (!cur_spec->path_depth || !cur_spec->bounces || (prev_spec && (!prev_spec->path_depth || !prev_spec->bounces)))
        return fail(CRT_ERR_INVALID_ARG, w + ": the specular planes need path_depth and bounces");
    if (prev_spec && (cur_spec->last_normal != nullptr) != (prev_spec->last_normal != nullptr))
        return fail(CRT_ERR_INVALID_ARG, w + ": last normals must be given in both frames or in neither");
    return CRT_OK;
}

void set_camera(const crt_camera& cam, float* eye, float* iv, float& scale)
{
    std::memcpy(eye, cam.eye, sizeof(cam.eye));
    std::memcpy(iv, cam.inv_view, sizeof(cam.inv_view));
    scale = det_tanf(cam.fov_y / 2);
}

// what crt_temporal_info and crt_temporal_clamp_info are filled from
struct TemporalCounts { float total_ms; unsigned long long reprojected, clamped, tried, taken; };

// the fields of TpParams every form of the pass fills from its arguments (the block is zeroed before)
void fill_params(TpParams& P, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_frame* cur, const crt_temporal_history* prev,
                 void* d_out_color, void* d_out_variance, void* d_out_history, void* d_out_rgb)
{
    P.width = prm->width; P.height = prm->height;
    P.tiles_x = (prm->width + 63) / 64;
    set_camera(prm->cur, P.eye, P.iv, P.scale);
    set_camera(prm->prev, P.peye, P.piv, P.pscale);
    P.ar = (float)prm->width / (float)prm->height;
    P.depth_tol = prm->depth_tolerance;
    P.normal_tol2 = prm->normal_tolerance * prm->normal_tolerance;
    P.alpha_min = prm->alpha_min;
    P.color = cur->color; P.variance = cur->variance; P.depth = cur->depth;
    if (prev) {
        P.normal = cur->normal; P.id = cur->id; // (without a history nothing reads the guides)
        P.pcolor = prev->color; P.pvariance = prev->variance; P.phistory = prev->history; P.pdepth = prev->depth;
        P.pnormal = prev->normal; P.pid = prev->id;
    }
    P.out_mean = (float*)d_out_color; P.out_rgb = (uint8_t*)d_out_rgb;
    P.out_variance = (float*)d_out_variance; P.out_history = (float*)d_out_history;
    if (clamp) { P.radius = (int)clamp->radius; P.gamma = clamp->gamma; }
}

int temporal_impl(const char* who, int device, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_frame* cur,
                  const crt_temporal_history* prev, void* d_out_color, void* d_out_variance, void* d_out_history, void* d_out_rgb, hipStream_t st,
                  TemporalCounts* info, const MomentArgs* mom = nullptr)
{
    const int rc = temporal_check(who, prm, clamp, cur, prev, d_out_color, d_out_variance, d_out_history, mom);
    if (rc != CRT_OK) return rc;
    TpParams P;
    std::memset(&P, 0, sizeof(P));
    fill_params(P, prm, clamp, cur, prev, d_out_color, d_out_variance, d_out_history, d_out_rgb);
    if (mom) {
        if (mom->prev) { P.pm1 = mom->prev->m1; P.pm2 = mom->prev->m2; }
        P.out_m1 = (float*)mom->out_m1; P.out_m2 = (float*)mom->out_m2;
    }
    unsigned long long n[2] = {0, 0};
    const int status = timed_launch(who, device, st, info, n, 2, [&](unsigned long long* d_count) {
        P.count = d_count;
        const dim3 grid(P.tiles_x * ((prm->height + 3) / 4));
        if (mom) {
            if (clamp) hipLaunchKernelGGL((k_temporal<true, true>), grid, dim3(256), 0, st, P);
            else hipLaunchKernelGGL((k_temporal<false, true>), grid, dim3(256), 0, st, P);
        } else if (clamp) hipLaunchKernelGGL((k_temporal<true, false>), grid, dim3(256), 0, st, P);
        else hipLaunchKernelGGL((k_temporal<false, false>), grid, dim3(256), 0, st, P);
    });
    if (status == CRT_OK && info) { info->reprojected = n[0]; info->clamped = n[1]; }
    return status;
}

// crt_temporal_dual / _device on device buffers (the checks made)
int temporal_dual_impl(const char* who, int device, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_dual_params* dual,
                       const crt_temporal_frame* cur, const crt_temporal_specular_planes* cur_spec, const crt_temporal_history* prev,
                       const crt_temporal_specular_planes* prev_spec, void* d_out_color, void* d_out_variance, void* d_out_history, void* d_out_rgb,
                       hipStream_t st, TemporalCounts* info)
{
    TpDualParams P;
    std::memset(&P, 0, sizeof(P));
    fill_params(P, prm, clamp, cur, prev, d_out_color, d_out_variance, d_out_history, d_out_rgb);
    P.dual_radius = (int)dual->radius; P.min_bounces = dual->min_bounces;
    if (prev) { // (without a history nothing reads the specular planes)
        P.path_depth = cur_spec->path_depth; P.bounces = cur_spec->bounces; P.last_normal = cur_spec->last_normal;
        P.ppath_depth = prev_spec->path_depth; P.pbounces = prev_spec->bounces; P.plast_normal = prev_spec->last_normal;
    }
    unsigned long long n[4] = {0, 0, 0, 0};
    const int status = timed_launch(who, device, st, info, n, 4, [&](unsigned long long* d_count) {
        P.count = d_count;
        const dim3 grid(P.tiles_x * ((prm->height + 3) / 4));
        if (clamp) hipLaunchKernelGGL((k_temporal_dual<true>), grid, dim3(256), 0, st, P);
        else hipLaunchKernelGGL((k_temporal_dual<false>), grid, dim3(256), 0, st, P);
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

template <class Info>
int temporal_device_form(const char* who, int device, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_frame* cur,
                         const crt_temporal_history* prev, void* d_out_color, void* d_out_variance, void* d_out_history, void* d_out_rgb, void* stream, Info* info,
                         const MomentArgs* mom = nullptr)
{
    TemporalCounts n{};
    const int rc = temporal_impl(who, device, prm, clamp, cur, prev, d_out_color, d_out_variance, d_out_history, d_out_rgb, (hipStream_t)stream,
                                 info ? &n : nullptr, mom);
    if (rc == CRT_OK && info) fill_info(info, n);
    return rc;
}

// The host-buffer form: the argument checks, device copies of the inputs, the device form, then the copies back.
template <class Info>
int temporal_host_form(const char* who, int device, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_frame* cur,
                       const crt_temporal_history* prev, float* out_color, float* out_variance, float* out_history, uint8_t* out_rgb, Info* info,
                       const MomentArgs* mom = nullptr)
{
    const int rc0 = temporal_check(who, prm, clamp, cur, prev, out_color, out_variance, out_history, mom);
    if (rc0 != CRT_OK) return rc0;
    const uint64_t npix = (uint64_t)prm->width * prm->height;
    TemporalCounts n{};
    const int rc = host_form(who, device, [&](HostCopies& c) {
        crt_temporal_frame dc{};
        crt_temporal_history dp{};
        crt_temporal_moment_planes dm{};
        MomentArgs dmom{};
        dc.color = c.in(cur->color, npix * 3);
        dc.variance = c.in(cur->variance, npix * 3);
        dc.depth = c.in(cur->depth, npix);
        dc.normal = c.in(cur->normal, npix * 3);
        dc.id = c.in(cur->id, npix);
        if (prev) {
            dp.color = c.in(prev->color, npix * 3);
            dp.variance = c.in(prev->variance, npix * 3);
            dp.history = c.in(prev->history, npix);
            dp.depth = c.in(prev->depth, npix);
            dp.normal = c.in(prev->normal, npix * 3);
            dp.id = c.in(prev->id, npix);
        }
        float *o_color = c.out(out_color, npix * 3), *o_hist = c.out(out_history, npix), *o_var = c.out(out_variance, npix * 3);
        uint8_t* o_rgb = c.out(out_rgb, npix * 3);
        if (mom) {
            if (mom->prev) {
                dm.m1 = c.in(mom->prev->m1, npix * 3);
                dm.m2 = c.in(mom->prev->m2, npix * 3);
                dmom.prev = &dm;
            }
            dmom.out_m1 = c.out((float*)mom->out_m1, npix * 3);
            dmom.out_m2 = c.out((float*)mom->out_m2, npix * 3);
        }
        return temporal_impl(who, device, prm, clamp, &dc, prev ? &dp : nullptr, o_color, o_var, o_hist, o_rgb, nullptr, info ? &n : nullptr,
                             mom ? &dmom : nullptr);
    });
    if (rc == CRT_OK && info) fill_info(info, n);
    return rc;
}

// every refusal of crt_temporal_dual / _device, crt_temporal_clamped's first
int temporal_dual_checks(const char* who, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_dual_params* dual,
                         const crt_temporal_frame* cur, const crt_temporal_specular_planes* cur_spec, const crt_temporal_history* prev,
                         const crt_temporal_specular_planes* prev_spec, const void* out_color, const void* out_variance, const void* out_history)
{
    // (the dual arguments first: temporal_check ends with the sizes the launch cannot cover)
    if (prm && cur)
        if (const int rc = temporal_dual_check(who, dual, prev, cur_spec, prev_spec)) return rc;
    return temporal_check(who, prm, clamp, cur, prev, out_color, out_variance, out_history, nullptr);
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

int crt_temporal_device(int device, const crt_temporal_params* prm, const crt_temporal_frame* dev_cur, const crt_temporal_history* dev_prev,
                        void* d_out_color, void* d_out_variance, void* d_out_history, void* d_out_rgb, void* stream, crt_temporal_info* info)
{
    return temporal_device_form("crt_temporal_device", device, prm, nullptr, dev_cur, dev_prev, d_out_color, d_out_variance, d_out_history, d_out_rgb, stream, info);
}

int crt_temporal(int device, const crt_temporal_params* prm, const crt_temporal_frame* host_cur, const crt_temporal_history* host_prev, float* out_color,
                 float* out_variance, float* out_history, uint8_t* out_rgb, crt_temporal_info* info)
{
    return temporal_host_form("crt_temporal", device, prm, nullptr, host_cur, host_prev, out_color, out_variance, out_history, out_rgb, info);
}

int crt_temporal_clamped_device(int device, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_frame* dev_cur,
                                const crt_temporal_history* dev_prev, void* d_out_color, void* d_out_variance, void* d_out_history, void* d_out_rgb,
                                void* stream, crt_temporal_clamp_info* info)
{
    return temporal_device_form("crt_temporal_clamped_device", device, prm, clamp, dev_cur, dev_prev, d_out_color, d_out_variance, d_out_history, d_out_rgb,
                                stream, info);
}

int crt_temporal_clamped(int device, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_frame* host_cur,
                         const crt_temporal_history* host_prev, float* out_color, float* out_variance, float* out_history, uint8_t* out_rgb,
                         crt_temporal_clamp_info* info)
{
    return temporal_host_form("crt_temporal_clamped", device, prm, clamp, host_cur, host_prev, out_color, out_variance, out_history, out_rgb, info);
}

int crt_temporal_moments_device(int device, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_frame* dev_cur,
                                const crt_temporal_history* dev_prev, const crt_temporal_moment_planes* dev_prev_moments, void* d_out_color,
                                void* d_out_variance, void* d_out_history, void* d_out_m1, void* d_out_m2, void* d_out_rgb, void* stream,
                                crt_temporal_clamp_info* info)
{
    const MomentArgs mom = {dev_prev_moments, d_out_m1, d_out_m2};
    return temporal_device_form("crt_temporal_moments_device", device, prm, clamp, dev_cur, dev_prev, d_out_color, d_out_variance, d_out_history, d_out_rgb,
                                stream, info, &mom);
}

int crt_temporal_moments(int device, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_frame* host_cur,
                         const crt_temporal_history* host_prev, const crt_temporal_moment_planes* host_prev_moments, float* out_color,
                         float* out_variance, float* out_history, float* out_m1, float* out_m2, uint8_t* out_rgb, crt_temporal_clamp_info* info)
{
    const MomentArgs mom = {host_prev_moments, out_m1, out_m2};
    return temporal_host_form("crt_temporal_moments", device, prm, clamp, host_cur, host_prev, out_color, out_variance, out_history, out_rgb, info, &mom);
}

int crt_temporal_dual_defaults(crt_temporal_dual_params* dual)
{
    if (!dual) return fail(CRT_ERR_INVALID_ARG, "crt_temporal_dual_defaults: null argument");
    std::memset(dual, 0, sizeof(*dual));
    dual->radius = 1; dual->min_bounces = 0.5f; // tuned on nothing (include/crt.h)
    return CRT_OK;
}

int crt_temporal_dual_device(int device, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_dual_params* dual,
                             const crt_temporal_frame* dev_cur, const crt_temporal_specular_planes* dev_cur_spec, const crt_temporal_history* dev_prev,
                             const crt_temporal_specular_planes* dev_prev_spec, void* d_out_color, void* d_out_variance, void* d_out_history,
                             void* d_out_rgb, void* stream, crt_temporal_dual_info* info)
{
    const char* who = "crt_temporal_dual_device";
    const int rc0 = temporal_dual_checks(who, prm, clamp, dual, dev_cur, dev_cur_spec, dev_prev, dev_prev_spec, d_out_color, d_out_variance, d_out_history);
    if (rc0 != CRT_OK) return rc0;
    TemporalCounts n{};
    const int rc = temporal_dual_impl(who, device, prm, clamp, dual, dev_cur, dev_cur_spec, dev_prev, dev_prev_spec, d_out_color, d_out_variance,
                                      d_out_history, d_out_rgb, (hipStream_t)stream, info ? &n : nullptr);
    if (rc == CRT_OK && info) fill_info(info, n);
    return rc;
}

int crt_temporal_dual(int device, const crt_temporal_params* prm, const crt_temporal_clamp* clamp, const crt_temporal_dual_params* dual,
                      const crt_temporal_frame* cur, const crt_temporal_specular_planes* cur_spec, const crt_temporal_history* prev,
                      const crt_temporal_specular_planes* prev_spec, float* out_color, float* out_variance, float* out_history, uint8_t* out_rgb,
                      crt_temporal_dual_info* info)
{
    const char* who = "crt_temporal_dual";
    const int rc0 = temporal_dual_checks(who, prm, clamp, dual, cur, cur_spec, prev, prev_spec, out_color, out_variance, out_history);
    if (rc0 != CRT_OK) return rc0;
    const uint64_t npix = (uint64_t)prm->width * prm->height;
    TemporalCounts n{};
    const int rc = host_form(who, device, [&](HostCopies& c) {
        crt_temporal_frame dc{};
        crt_temporal_history dp{};
        crt_temporal_specular_planes dcs{}, dps{};
        dc.color = c.in(cur->color, npix * 3);
        dc.variance = c.in(cur->variance, npix * 3);
        dc.depth = c.in(cur->depth, npix);
        dc.normal = c.in(cur->normal, npix * 3);
        dc.id = c.in(cur->id, npix);
        dcs.path_depth = c.in(cur_spec->path_depth, npix);
        dcs.bounces = c.in(cur_spec->bounces, npix);
        dcs.last_normal = c.in(cur_spec->last_normal, npix * 3);
        if (prev) {
            dp.color = c.in(prev->color, npix * 3);
            dp.variance = c.in(prev->variance, npix * 3);
            dp.history = c.in(prev->history, npix);
            dp.depth = c.in(prev->depth, npix);
            dp.normal = c.in(prev->normal, npix * 3);
            dp.id = c.in(prev->id, npix);
            dps.path_depth = c.in(prev_spec->path_depth, npix);
            dps.bounces = c.in(prev_spec->bounces, npix);
            dps.last_normal = c.in(prev_spec->last_normal, npix * 3);
        }
        float *o_color = c.out(out_color, npix * 3), *o_hist = c.out(out_history, npix), *o_var = c.out(out_variance, npix * 3);
        uint8_t* o_rgb = c.out(out_rgb, npix * 3);
        return temporal_dual_impl(who, device, prm, clamp, dual, &dc, &dcs, prev ? &dp : nullptr, prev ? &dps : nullptr, o_color, o_var, o_hist, o_rgb,
                                  nullptr, info ? &n : nullptr);
    });
    if (rc == CRT_OK && info) fill_info(info, n);
    return rc;
}

} // extern "C"
