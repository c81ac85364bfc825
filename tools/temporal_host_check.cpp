// tools/temporal_host_check.cpp -- the per-pixel text of all six temporal kernels (cudaraytracing_amd/csrc/crt_temporal.h) compiled for
// the HOST and run against a plain restatement of include/crt.h written here, scalar and straight down the contract's lines, for
// AddressSanitizer / UBSan runs without a device.  crt_temporal.h and crt_stages.h (the tone map, write_color) are included as they are;
// tools/host_device.h stands in for what they take from outside.  k_temporal_dual (crt_temporal.hip) is temporal_dual_begin, one ballot,
// temporal_dual_finish; here every pixel runs twice, once with its own `tries` as the ballot's result and once with `true` (a wave in
// which another lane tries), and both must write the restatement's bits.  k_temporal<CLAMP, MOMENTS> is temporal_single; every case also
// runs its four instantiations, with and without the clamp and the moment planes, against the restatement of a pixel that does not try V,
// plus crt_temporal_moments' two lines.  Every image has exactly its entries, so a tap one element out is a report.
//
// Cases: 70 x 19, 5 x 3 and 1 x 1; the choice's radius 1 and 3; with and without a clamp; min_bounces 0.5 and +inf; finite inputs and
// inputs with NaN and +-inf planted in the colours, in path_depth and in bounces of both frames (a bounces of +inf reaches a min_bounces of
// +inf: the one input with which that setting tries V); without a history.  Planted in every
// case that has room: a black history (both candidates 0: a tie), a block where the virtual point is the surface point, a block where
// only V's taps can count and one where only S's can.  Then the mirror scene of tests/test_temporal_dual.py: a camera that looks along
// +z at a mirror in z = 100 and sees in it a plane behind itself whose colour is linear in x and y; under four camera moves the history
// the dual pass takes is the analytic colour of the pixel to 1e-5 relative, and under the sideways ones crt_temporal's own reprojection
// (min_bounces = +inf) misses it by more than a hundred times that.
//
//   temporal_host_check [- OUT]     OUT: the outputs of every case, for a byte comparison between the plain and the sanitised build
//
// tests/test_temporal_dual.py builds it plain (-O2) and sanitised and runs both:
//   g++ -std=c++17 -ffp-contract=off -I cudaraytracing_amd/csrc -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       tools/temporal_host_check.cpp -o /tmp/temporal_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "host_device.h"

#include "crt_stages.h"
#include "crt_temporal.h"

using namespace crtk;

static int g_fail = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { if (g_fail < 40) { std::fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } g_fail++; } \
    } while (0)

static const float INF = std::numeric_limits<float>::infinity();
static const float QNAN = std::numeric_limits<float>::quiet_NaN();

struct Rng { // (a fixed sequence on every machine)
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    float uniform() { return (float)(next() & 0xffffffu) / 16777216.0f; }
};

struct Camera { float eye[3], iv[9], fov; };

// one frame with its specular planes, and the history's extra plane
struct Frame {
    std::vector<float> color, variance, depth, normal, path_depth, bounces, last_normal, history, m1, m2; // (m1, m2: a history's moment planes)
    std::vector<int32_t> id;
};

struct Case {
    int w, h;
    Camera cam, pcam;
    float depth_tol, normal_tol, alpha_min;
    bool clamp; int clamp_radius; float gamma;
    int radius; float min_bounces;
    bool with_history, with_normals, with_ids, with_variance, with_last_normals;
    bool with_moments = false; // prev has m1 and m2: the single-candidate form also runs with them
    Frame cur, prev;
};

struct Outputs {
    std::vector<float> color, variance, history, m1, m2;
    std::vector<uint8_t> rgb;
    unsigned long long took = 0, clamped = 0, tried = 0, took_V = 0, ties = 0, v_only = 0, s_kept = 0;
};

// ------------------------------------------------------------------------------------------------ the contract, restated --

struct RefCand { float hc[3], hv[3], h1[3], h2[3], hn, ws; bool valid; };

static void ref_unit3(float* a)
{
    const float z = a[0] * a[0] + (a[1] * a[1] + a[2] * a[2]);
    if (z > 0) { const float s = std::sqrt(z); a[0] = a[0] / s; a[1] = a[1] / s; a[2] = a[2] / s; }
}

// crt_temporal's lines from P to the tap loop, with `dist` for depth(p); virt: step 2's tap test in the place of crt_temporal's
static RefCand ref_candidate(const Case& c, const int x, const int y, const float dist, const bool virt)
{
    const int W = c.w, H = c.h;
    const float scale = det_tanf(c.cam.fov / 2), pscale = det_tanf(c.pcam.fov / 2), ar = (float)W / (float)H;
    const float* iv = c.cam.iv;
    const float* pi = c.pcam.iv;
    const float sx = (((2 * ((float)x + 0.5f)) / W - 1) * scale) * ar, sy = (1 - (2 * ((float)y + 0.5f)) / H) * scale;
    float cd[3] = {-sx, sy, 1};
    ref_unit3(cd);
    float d[3] = {iv[0] * cd[0] + (iv[3] * cd[1] + iv[6] * cd[2]), iv[1] * cd[0] + (iv[4] * cd[1] + iv[7] * cd[2]), iv[2] * cd[0] + (iv[5] * cd[1] + iv[8] * cd[2])};
    ref_unit3(d);
    float v[3];
    for (int k = 0; k < 3; k++) { const float P = c.cam.eye[k] + d[k] * dist; v[k] = P - c.pcam.eye[k]; }
    const float cx = pi[0] * v[0] + (pi[1] * v[1] + pi[2] * v[2]), cy = pi[3] * v[0] + (pi[4] * v[1] + pi[5] * v[2]), cz = pi[6] * v[0] + (pi[7] * v[1] + pi[8] * v[2]);
    const float tp = std::sqrt(v[0] * v[0] + (v[1] * v[1] + v[2] * v[2]));
    const float fx = (((((-cx) / cz) / (pscale * ar)) + 1) * W) / 2 - 0.5f, fy = (((1 - (cy / cz) / pscale) * H) / 2) - 0.5f;
    const bool ok = dist > 0 && cz > 0 && fx > -1 && fx < W && fy > -1 && fy < H;
    RefCand r;
    for (int k = 0; k < 3; k++) r.hc[k] = r.hv[k] = r.h1[k] = r.h2[k] = 0.0f;
    r.hn = 0.0f; r.ws = 0.0f; r.valid = false;
    if (!ok) return r;
    const float x0f = std::floor(fx), y0f = std::floor(fy), wx = fx - x0f, wy = fy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const size_t p = (size_t)y * W + x;
    const bool normals = virt ? c.with_last_normals : c.with_normals;
    const std::vector<float>& cn = virt ? c.cur.last_normal : c.cur.normal;
    const std::vector<float>& pn = virt ? c.prev.last_normal : c.prev.normal;
    const std::vector<float>& pdist = virt ? c.prev.path_depth : c.prev.depth;
    for (int j = 0; j < 2; j++)
        for (int i = 0; i < 2; i++) {
            const int qx = x0 + i, qy = y0 + j;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const size_t q = (size_t)qy * W + qx;
            if (virt && !(c.prev.bounces.at(q) >= c.min_bounces)) continue;
            if (!(pdist.at(q) > 0)) continue;
            if (!(std::fabs(pdist.at(q) - tp) <= c.depth_tol * tp)) continue;
            if (normals) {
                const float a = cn.at(p * 3) - pn.at(q * 3), b = cn.at(p * 3 + 1) - pn.at(q * 3 + 1), e = cn.at(p * 3 + 2) - pn.at(q * 3 + 2);
                if (!(a * a + b * b + e * e <= c.normal_tol * c.normal_tol)) continue;
            }
            if (c.with_ids && c.cur.id.at(p) != c.prev.id.at(q)) continue;
            const float b = (i ? wx : 1 - wx) * (j ? wy : 1 - wy);
            for (int k = 0; k < 3; k++) {
                r.hc[k] = r.hc[k] + c.prev.color.at(q * 3 + k) * b;
                if (c.with_variance) r.hv[k] = r.hv[k] + c.prev.variance.at(q * 3 + k) * b;
                if (c.with_moments) { r.h1[k] = r.h1[k] + c.prev.m1.at(q * 3 + k) * b; r.h2[k] = r.h2[k] + c.prev.m2.at(q * 3 + k) * b; }
            }
            r.hn = r.hn + c.prev.history.at(q) * b;
            r.ws = r.ws + b;
        }
    r.valid = r.ws > 0.015625f;
    return r;
}

static void ref_box(const Case& c, const int x, const int y, const int r, float* s1, float* s2, float& cnt)
{
    for (int k = 0; k < 3; k++) s1[k] = s2[k] = 0.0f;
    cnt = 0.0f;
    for (int dy = -r; dy <= r; dy++)
        for (int dx = -r; dx <= r; dx++) {
            const int tx = x + dx, ty = y + dy;
            if (tx < 0 || tx >= c.w || ty < 0 || ty >= c.h) continue;
            for (int k = 0; k < 3; k++) {
                const float t = c.cur.color.at(((size_t)ty * c.w + tx) * 3 + k);
                s1[k] = s1[k] + t;
                s2[k] = s2[k] + t * t;
            }
            cnt = cnt + 1;
        }
}

static float ref_distance(const RefCand& a, const float* s1, const float cnt)
{
    const float dx = a.hc[0] / a.ws - s1[0] / cnt, dy = a.hc[1] / a.ws - s1[1] / cnt, dz = a.hc[2] / a.ws - s1[2] / cnt;
    return dx * dx + (dy * dy + dz * dz);
}

static uint8_t ref_tonemap(const float v)
{
    const float cl = v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f; // maxf_ref(0, minf_ref(1, c)): a NaN gives 0
    const float t = 255 * det_powf(cl == cl ? cl : 0.0f, 0.6f);
    if (!(t == t) || t <= 0.0f) return 0;
    if (t >= 255.0f) return 255;
    return (uint8_t)t;
}

// dual false: no pixel tries V (crt_temporal, crt_temporal_clamped, crt_temporal_moments); clamp: the case's, or the caller's
static void ref_run(const Case& c, Outputs& o, const bool dual, const bool clamp)
{
    const size_t n = (size_t)c.w * c.h;
    o.color.assign(n * 3, 0); o.variance.assign(n * 3, 0); o.history.assign(n, 0); o.rgb.assign(n * 3, 0); o.m1.assign(n * 3, 0); o.m2.assign(n * 3, 0);
    for (int y = 0; y < c.h; y++)
        for (int x = 0; x < c.w; x++) {
            const size_t p = (size_t)y * c.w + x;
            float oc[3], ov[3] = {0, 0, 0}, o1[3], o2[3], oh = 1.0f;
            for (int k = 0; k < 3; k++) {
                oc[k] = o1[k] = c.cur.color.at(p * 3 + k);
                o2[k] = oc[k] * oc[k];
                if (c.with_variance) ov[k] = c.cur.variance.at(p * 3 + k);
            }
            if (c.with_history) {
                const RefCand S = ref_candidate(c, x, y, c.cur.depth.at(p), false);
                RefCand T = S;
                const bool tries = dual && c.cur.bounces.at(p) >= c.min_bounces && c.cur.path_depth.at(p) > 0;
                if (tries) {
                    o.tried++;
                    const RefCand V = ref_candidate(c, x, y, c.cur.path_depth.at(p), true);
                    if (V.valid) {
                        float s1[3], s2[3], cnt;
                        ref_box(c, x, y, c.radius, s1, s2, cnt);
                        bool take = !S.valid;
                        if (S.valid) {
                            const float eV = ref_distance(V, s1, cnt), eS = ref_distance(S, s1, cnt);
                            take = eV < eS;
                            if (eV == eS) o.ties++;
                            if (!take) o.s_kept++;
                        } else o.v_only++;
                        if (take) { T = V; o.took_V++; }
                    }
                }
                if (T.valid) {
                    o.took++;
                    const float hn = T.hn / T.ws;
                    oh = hn + 1;
                    float a = 1 / oh;
                    a = a < c.alpha_min ? c.alpha_min : a;
                    const float k1 = 1 - a;
                    float s1[3], s2[3], cnt = 0;
                    if (clamp) ref_box(c, x, y, c.clamp_radius, s1, s2, cnt);
                    bool moved = false;
                    for (int k = 0; k < 3; k++) {
                        float Hc = T.hc[k] / T.ws;
                        if (clamp) {
                            const float mu = s1[k] / cnt;
                            float e = s2[k] / cnt - mu * mu;
                            e = e < 0 ? 0 : e;
                            const float wd = c.gamma * std::sqrt(e), lo = mu - wd, hi = mu + wd;
                            if (Hc < lo) { Hc = lo; moved = true; }
                            if (Hc > hi) { Hc = hi; moved = true; }
                        }
                        oc[k] = Hc * k1 + c.cur.color.at(p * 3 + k) * a;
                        if (c.with_variance) ov[k] = (T.hv[k] / T.ws) * (k1 * k1) + c.cur.variance.at(p * 3 + k) * (a * a);
                        const float cc = c.cur.color.at(p * 3 + k);
                        o1[k] = (T.h1[k] / T.ws) * k1 + cc * a;      // (never clamped; the planes of S: compared only where no pixel tries V)
                        o2[k] = (T.h2[k] / T.ws) * k1 + (cc * cc) * a;
                    }
                    if (moved) o.clamped++;
                }
            }
            for (int k = 0; k < 3; k++) {
                o.color[p * 3 + k] = oc[k]; o.variance[p * 3 + k] = ov[k]; o.rgb[p * 3 + k] = ref_tonemap(oc[k]);
                o.m1[p * 3 + k] = o1[k]; o.m2[p * 3 + k] = o2[k];
            }
            o.history[p] = oh;
        }
}

// ------------------------------------------------------------------------------------------------ the kernel's text --

// the parameter block of a case as crt_temporal.hip's fill_params fills it, on the outputs of o (filled with what no pixel writes)
static TpDualParams text_params(const Case& c, const bool clamp, const bool moments, Outputs& o)
{
    const size_t n = (size_t)c.w * c.h;
    o.color.assign(n * 3, QNAN); o.variance.assign(n * 3, QNAN); o.history.assign(n, QNAN); o.rgb.assign(n * 3, 0x5a);
    o.m1.assign(moments ? n * 3 : 0, QNAN); o.m2.assign(moments ? n * 3 : 0, QNAN);
    TpDualParams P;
    std::memset(&P, 0, sizeof(P));
    P.width = (uint32_t)c.w; P.height = (uint32_t)c.h; P.tiles_x = ((uint32_t)c.w + 63) / 64;
    std::memcpy(P.eye, c.cam.eye, 12); std::memcpy(P.iv, c.cam.iv, 36); P.scale = det_tanf(c.cam.fov / 2);
    std::memcpy(P.peye, c.pcam.eye, 12); std::memcpy(P.piv, c.pcam.iv, 36); P.pscale = det_tanf(c.pcam.fov / 2);
    P.ar = (float)c.w / (float)c.h;
    P.depth_tol = c.depth_tol; P.normal_tol2 = c.normal_tol * c.normal_tol; P.alpha_min = c.alpha_min;
    P.color = c.cur.color.data(); P.depth = c.cur.depth.data();
    if (c.with_variance) P.variance = c.cur.variance.data();
    if (c.with_history) { // (without a history no guide and no specular plane)
        if (c.with_normals) { P.normal = c.cur.normal.data(); P.pnormal = c.prev.normal.data(); }
        if (c.with_ids) { P.id = c.cur.id.data(); P.pid = c.prev.id.data(); }
        P.pcolor = c.prev.color.data(); P.phistory = c.prev.history.data(); P.pdepth = c.prev.depth.data();
        if (c.with_variance) P.pvariance = c.prev.variance.data();
        P.path_depth = c.cur.path_depth.data(); P.bounces = c.cur.bounces.data();
        P.ppath_depth = c.prev.path_depth.data(); P.pbounces = c.prev.bounces.data();
        if (c.with_last_normals) { P.last_normal = c.cur.last_normal.data(); P.plast_normal = c.prev.last_normal.data(); }
    }
    P.out_mean = o.color.data(); P.out_rgb = o.rgb.data(); P.out_history = o.history.data();
    if (c.with_variance) P.out_variance = o.variance.data();
    if (clamp) { P.radius = c.clamp_radius; P.gamma = c.gamma; }
    P.dual_radius = c.radius; P.min_bounces = c.min_bounces;
    if (moments) {
        if (c.with_history) { P.pm1 = c.prev.m1.data(); P.pm2 = c.prev.m2.data(); }
        P.out_m1 = o.m1.data(); P.out_m2 = o.m2.data();
    }
    return P;
}

// k_temporal_dual<CLAMP>'s pixels
template <bool CLAMP> static void text_run(const Case& c, const bool every_wave_tries, Outputs& o)
{
    const TpDualParams P = text_params(c, CLAMP, false, o);
    for (int y = 0; y < c.h; y++)
        for (int x = 0; x < c.w; x++) {
            TpDualState st;
            std::memset(&st, 0, sizeof(st));
            if (P.pcolor) st = temporal_dual_begin(P, x, y);
            const TpFlags fl = temporal_dual_finish<CLAMP>(P, x, y, st, every_wave_tries || st.tries);
            o.took += fl.took; o.clamped += fl.clamped; o.tried += fl.tried; o.took_V += fl.took_V;
        }
    if (!c.with_variance) o.variance.assign((size_t)c.w * c.h * 3, 0);
}

// k_temporal<CLAMP, MOMENTS>'s pixels: the base of the block alone, as the kernel takes it
template <bool CLAMP, bool MOMENTS> static void text_single(const Case& c, Outputs& o)
{
    const TpParams P = text_params(c, CLAMP, MOMENTS, o);
    for (int y = 0; y < c.h; y++)
        for (int x = 0; x < c.w; x++) {
            const TpFlags fl = temporal_single<CLAMP, MOMENTS>(P, x, y);
            o.took += fl.took; o.clamped += fl.clamped; o.tried += fl.tried; o.took_V += fl.took_V;
        }
    if (!c.with_variance) o.variance.assign((size_t)c.w * c.h * 3, 0);
}

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b, size_t& at)
{
    for (size_t i = 0; i < a.size(); i++) {
        const bool na = a[i] != a[i], nb = b[i] != b[i];
        if (na != nb || (!na && __float_as_uint(a[i]) != __float_as_uint(b[i]))) { at = i; return false; }
    }
    return a.size() == b.size();
}

static void compare(const Case& c, const Outputs& want, const Outputs& got, const char* what, const int index)
{
    size_t at = 0;
    CHECK(same_bits(want.color, got.color, at), "case %d (%s): colour differs at %zu: %g, expected %g", index, what, at, got.color[at], want.color[at]);
    CHECK(same_bits(want.variance, got.variance, at), "case %d (%s): variance differs at %zu", index, what, at);
    CHECK(same_bits(want.history, got.history, at), "case %d (%s): history differs at %zu: %g, expected %g", index, what, at, got.history[at], want.history[at]);
    CHECK(want.rgb == got.rgb, "case %d (%s): rgb differs", index, what);
    if (!got.m1.empty()) { // (a run with the moment planes)
        CHECK(same_bits(want.m1, got.m1, at), "case %d (%s): m1 differs at %zu: %g, expected %g", index, what, at, got.m1[at], want.m1[at]);
        CHECK(same_bits(want.m2, got.m2, at), "case %d (%s): m2 differs at %zu: %g, expected %g", index, what, at, got.m2[at], want.m2[at]);
    }
    CHECK(want.took == got.took && want.clamped == got.clamped && want.tried == got.tried && want.took_V == got.took_V,
          "case %d (%s): counts %llu %llu %llu %llu, expected %llu %llu %llu %llu", index, what, got.took, got.clamped, got.tried, got.took_V, want.took,
          want.clamped, want.tried, want.took_V);
    (void)c;
}

// The four single-candidate kernels on a case, each against the restatement in which no pixel tries V; the moment planes where the case
// has them.  Adds the pixels that took a history and of those the clamped ones, over the runs; out: takes the bytes they wrote.
static void single_runs(const Case& c, const int index, unsigned long long& took, unsigned long long& clamped, std::FILE* out)
{
    Outputs want[2], got[4];
    ref_run(c, want[0], false, false);
    ref_run(c, want[1], false, true);
    text_single<false, false>(c, got[0]);
    text_single<true, false>(c, got[1]);
    compare(c, want[0], got[0], "one candidate", index);
    compare(c, want[1], got[1], "one candidate, clamped", index);
    if (c.with_moments) {
        text_single<false, true>(c, got[2]);
        text_single<true, true>(c, got[3]);
        compare(c, want[0], got[2], "one candidate, moments", index);
        compare(c, want[1], got[3], "one candidate, clamped, moments", index);
    }
    for (int r = 0; r < (c.with_moments ? 4 : 2); r++) {
        took += got[r].took; clamped += got[r].clamped;
        if (!out) continue;
        std::fwrite(got[r].color.data(), 4, got[r].color.size(), out); std::fwrite(got[r].history.data(), 4, got[r].history.size(), out);
        if (r >= 2) { std::fwrite(got[r].m1.data(), 4, got[r].m1.size(), out); std::fwrite(got[r].m2.data(), 4, got[r].m2.size(), out); }
    }
}

// ------------------------------------------------------------------------------------------------ the cases --

static void rotation_y(float* iv, const float t)
{
    const float s = std::sin(t), co = std::cos(t);
    const float m[9] = {co, 0, -s, 0, 1, 0, s, 0, co}; // columns: the camera's x, y and z axes in the world
    std::memcpy(iv, m, sizeof(m));
}

static void fill_frame(Frame& f, const int w, const int h, Rng& rng)
{
    const size_t n = (size_t)w * h;
    f.color.resize(n * 3); f.variance.resize(n * 3); f.depth.resize(n); f.normal.resize(n * 3); f.path_depth.resize(n); f.bounces.resize(n);
    f.last_normal.resize(n * 3); f.history.resize(n); f.id.assign(n, 3);
    for (size_t i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++) { f.color[i * 3 + k] = rng.uniform() * 100; f.variance[i * 3 + k] = rng.uniform() * 300; }
        f.depth[i] = 40.0f * (0.94f + rng.uniform() * 0.12f);
        f.path_depth[i] = 70.0f * (0.94f + rng.uniform() * 0.12f);
        f.bounces[i] = 0.25f * (float)(rng.next() % 5u);
        f.history[i] = 1.0f + (float)(rng.next() % 40u);
        float a[3] = {(rng.uniform() - 0.5f) * 0.5f, (rng.uniform() - 0.5f) * 0.5f, 1.0f}, b[3] = {(rng.uniform() - 0.5f) * 0.5f, 1.0f, (rng.uniform() - 0.5f) * 0.5f};
        ref_unit3(a); ref_unit3(b);
        for (int k = 0; k < 3; k++) { f.normal[i * 3 + k] = a[k]; f.last_normal[i * 3 + k] = b[k]; }
    }
}

template <class T, class V> static void block(std::vector<T>& plane, const int w, const int h, const int ch, int y0, int y1, int x0, int x1, const V value)
{
    for (int y = y0; y < y1 && y < h; y++)
        for (int x = x0; x < x1 && x < w; x++)
            for (int k = 0; k < ch; k++) plane[((size_t)y * w + x) * ch + k] = (T)value;
}

static Case synthetic(const int w, const int h, const uint64_t seed, const bool non_finite)
{
    Case c;
    c.w = w; c.h = h;
    const float eye[3] = {1, 2, 3}, peye[3] = {2.5f, 1.25f, 3.5f};
    std::memcpy(c.cam.eye, eye, 12); std::memcpy(c.pcam.eye, peye, 12);
    rotation_y(c.cam.iv, 0.0f); rotation_y(c.pcam.iv, 0.05f);
    c.cam.fov = 0.7f; c.pcam.fov = 0.75f;
    c.depth_tol = 0.05f; c.normal_tol = 0.5f; c.alpha_min = 0.05f;
    c.clamp = false; c.clamp_radius = 1; c.gamma = 1.0f; c.radius = 1; c.min_bounces = 0.5f;
    c.with_history = c.with_normals = c.with_ids = c.with_variance = c.with_last_normals = true;
    Rng rng{seed};
    fill_frame(c.cur, w, h, rng); fill_frame(c.prev, w, h, rng);
    block(c.cur.depth, w, h, 1, h / 3, h / 3 + 5, w / 4, w / 4 + 9, 0.0f);
    block(c.prev.depth, w, h, 1, h / 2, h / 2 + 5, w / 2, w / 2 + 11, 0.0f);         // only V's taps can count
    block(c.cur.path_depth, w, h, 1, 2, 6, 3 * w / 4, 3 * w / 4 + 8, 0.0f);
    block(c.prev.path_depth, w, h, 1, h / 4, h / 4 + 6, w / 8, w / 8 + 10, 0.0f);    // only S's
    block(c.prev.id, w, h, 1, 1, 5, w / 2, w / 2 + 9, 7);
    block(c.prev.color, w, h, 3, 3 * h / 4, h, 0, w / 3, 0.0f);                      // a black history: both H are 0, a tie
    for (int y = 0; y < h / 5 + 1 && y < h; y++)                                     // the virtual point is the surface point
        for (int x = 0; x < w / 5 + 1 && x < w; x++) {
            const size_t p = (size_t)y * w + x;
            for (Frame* f : {&c.cur, &c.prev}) {
                f->path_depth[p] = f->depth[p]; f->bounces[p] = 1.0f;
                for (int k = 0; k < 3; k++) f->last_normal[p * 3 + k] = f->normal[p * 3 + k];
            }
        }
    // the history's moment planes, from a sequence of their own (the other planes are what they were without them)
    Rng mrng{seed * 7919u + 13u};
    c.with_moments = true;
    c.prev.m1.resize((size_t)w * h * 3); c.prev.m2.resize((size_t)w * h * 3);
    for (size_t i = 0; i < c.prev.m1.size(); i++) { c.prev.m1[i] = mrng.uniform() * 100; c.prev.m2[i] = mrng.uniform() * 10000; }
    if (non_finite) {
        const float bad[3] = {QNAN, INF, -INF};
        for (std::vector<float>* plane : {&c.prev.m1, &c.prev.m2})
            for (int k = 0; k < 9; k++) (*plane)[(size_t)(mrng.next() % (uint32_t)plane->size())] = bad[k % 3];
        int i = 0;
        for (std::vector<float>* plane : {&c.cur.color, &c.prev.color, &c.cur.path_depth, &c.prev.path_depth, &c.cur.bounces, &c.prev.bounces, &c.cur.depth,
                                          &c.prev.depth, &c.prev.history, &c.prev.variance})
            for (int k = 0; k < 9; k++, i++) (*plane)[(size_t)(rng.next() % (uint32_t)plane->size())] = bad[i % 3];
    }
    return c;
}

// the mirror scene: see the head of this file.  zm = 100, zq = -50: the virtual plane lies at z = 250
static void mirror_frame(Frame& f, const Camera& cam, const int w, const int h, const bool history)
{
    const size_t n = (size_t)w * h;
    f.color.resize(n * 3); f.depth.resize(n); f.path_depth.resize(n); f.bounces.assign(n, 1.0f); f.id.assign(n, 5);
    if (history) f.history.assign(n, 1e6f);
    const double scale = std::tan((double)cam.fov / 2), ar = (double)w / h;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const double sx = ((2 * (x + 0.5)) / w - 1) * scale * ar, sy = (1 - (2 * (y + 0.5)) / h) * scale;
            double d[3] = {-sx, sy, 1};
            const double l = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            for (double& v : d) v /= l;
            const double depth = (100.0 - cam.eye[2]) / d[2], path = (250.0 - cam.eye[2]) / d[2];
            const double X = cam.eye[0] + d[0] * path, Y = cam.eye[1] + d[1] * path;
            const size_t p = (size_t)y * w + x;
            f.depth[p] = (float)depth; f.path_depth[p] = (float)path;
            f.color[p * 3] = (float)(300 + X + 0.5 * Y); f.color[p * 3 + 1] = (float)(400 - 2 * X + Y); f.color[p * 3 + 2] = (float)(1000 + 3 * X - 2 * Y);
        }
}

// Largest relative distance of the accumulated colour from the analytic one over the pixels whose taps are all inside the image: the four
// bilinear ones in the previous frame and the (2 radius + 1)^2 of the choice in the current one.  (On the image's border the mean of an
// affine colour over the clipped neighbourhood lies half a pixel's gradient from the pixel's own colour, and a surface history that errs
// by less than a pixel's gradient can lie nearer to it: three such pixels of the top row keep S under the move (3, 2, 15).)  With a history of 10^6 frames and alpha_min = 2^-20 the output is H k + c a with a = 2^-20 and c the
// analytic colour itself, so its distance from c is that of the history H, times k.
static double mirror_error(const int w, const int h, const float* move, const float min_bounces, size_t& inside, Outputs& out)
{
    Case c;
    c.w = w; c.h = h;
    const float zero[3] = {0, 0, 0};
    std::memcpy(c.pcam.eye, zero, 12); std::memcpy(c.cam.eye, move, 12);
    rotation_y(c.cam.iv, 0.0f); rotation_y(c.pcam.iv, 0.0f);
    c.cam.fov = c.pcam.fov = 0.69813174f; // 40 degrees
    c.depth_tol = 0.05f; c.normal_tol = 0.5f; c.alpha_min = 1.0f / 1048576.0f;
    c.clamp = false; c.clamp_radius = 1; c.gamma = 1.0f; c.radius = 1; c.min_bounces = min_bounces;
    c.with_history = c.with_ids = true;
    c.with_normals = c.with_variance = c.with_last_normals = false;
    mirror_frame(c.cur, c.cam, w, h, false);
    mirror_frame(c.prev, c.pcam, w, h, true);
    text_run<false>(c, false, out);
    Outputs want;
    ref_run(c, want, true, false);
    compare(c, want, out, "mirror", -1);
    unsigned long long took = 0, clamped = 0;
    single_runs(c, -1, took, clamped, nullptr);
    const double scale = std::tan((double)c.pcam.fov / 2), ar = (double)w / h;
    double worst = 0;
    inside = 0;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t p = (size_t)y * w + x;
            const double sx = ((2 * (x + 0.5)) / w - 1) * scale * ar, sy = (1 - (2 * (y + 0.5)) / h) * scale;
            const double t = (250.0 - move[2]), vx = move[0] - sx * t, vy = move[1] + sy * t, vz = 250.0; // the virtual point, from the previous eye
            const double fx = ((-vx / vz) / (scale * ar) + 1) * w / 2 - 0.5, fy = (1 - (vy / vz) / scale) * h / 2 - 0.5;
            if (!(fx >= 0 && fx <= w - 1 && fy >= 0 && fy <= h - 1)) continue;
            if (x < c.radius || x >= w - c.radius || y < c.radius || y >= h - c.radius) continue; // (see below)
            inside++;
            for (int k = 0; k < 3; k++) {
                const double wantc = c.cur.color[p * 3 + k];
                worst = std::max(worst, std::fabs(out.color[p * 3 + k] - wantc) / std::fabs(wantc));
            }
        }
    return worst;
}

int main(int argc, char** argv)
{
    if (argc != 1 && argc != 3) { std::fprintf(stderr, "usage: temporal_host_check [- OUT]\n"); return 2; }
    std::FILE* out = argc == 3 ? std::fopen(argv[2], "wb") : nullptr;
    if (argc == 3 && !out) { std::fprintf(stderr, "temporal_host_check: cannot open the output file\n"); return 2; }
    int cases = 0;
    unsigned long long ties = 0, v_only = 0, s_kept = 0, took_V = 0, non_finite_out = 0, single_took = 0, single_clamped = 0;
    const int sizes[3][2] = {{70, 19}, {5, 3}, {1, 1}};
    for (int s = 0; s < 3; s++)
        for (int radius : {1, 3})
            for (int clamp = 0; clamp < 2; clamp++)
                for (float min_bounces : {0.5f, INF})
                    for (int kind = 0; kind < 3; kind++) { // finite, non-finite, finite without variance / normals / last normals / ids
                        Case c = synthetic(sizes[s][0], sizes[s][1], 1000u + (uint64_t)cases, kind == 1);
                        c.radius = radius; c.min_bounces = min_bounces;
                        c.clamp = clamp != 0; c.clamp_radius = radius == 1 ? 1 : 2; // (the clamp's radius equal to the choice's, and not)
                        if (kind == 2) c.with_variance = c.with_normals = c.with_last_normals = c.with_ids = false;
                        Outputs want, got, got2;
                        ref_run(c, want, true, c.clamp);
                        if (c.clamp) { text_run<true>(c, false, got); text_run<true>(c, true, got2); }
                        else { text_run<false>(c, false, got); text_run<false>(c, true, got2); }
                        compare(c, want, got, "the pixel's own ballot", cases);
                        compare(c, want, got2, "a wave that tries", cases);
                        if (min_bounces == INF && kind != 1) CHECK(want.tried == 0 && want.took_V == 0, "case %d: min_bounces = +inf tried %llu pixels", cases, want.tried);
                        ties += want.ties; v_only += want.v_only; s_kept += want.s_kept; took_V += want.took_V;
                        for (float v : want.color) non_finite_out += !(v - v == 0);
                        if (out) { std::fwrite(got.color.data(), 4, got.color.size(), out); std::fwrite(got.history.data(), 4, got.history.size(), out); std::fwrite(got.rgb.data(), 1, got.rgb.size(), out); }
                        single_runs(c, cases, single_took, single_clamped, out);
                        cases++;
                    }
    for (int s = 0; s < 3; s++) { // without a history: every pixel resets, no plane of the history or of the specular AOVs is read
        Case c = synthetic(sizes[s][0], sizes[s][1], 77u + (uint64_t)s, false);
        c.with_history = false;
        c.prev = Frame();
        c.cur.path_depth.clear(); c.cur.bounces.clear(); c.cur.last_normal.clear();
        Outputs want, got;
        ref_run(c, want, true, true);
        text_run<true>(c, true, got);
        compare(c, want, got, "no history", cases);
        CHECK(want.took == 0 && want.tried == 0, "case %d: a call without a history took one", cases);
        unsigned long long took = 0, clamped = 0;
        single_runs(c, cases, took, clamped, out);
        CHECK(took == 0 && clamped == 0, "case %d: a single-candidate call without a history took one", cases);
        cases++;
    }
    CHECK(ties >= 20 && v_only >= 20 && s_kept >= 20 && took_V >= 100 && non_finite_out >= 20,
          "the cases do not reach every branch: %llu ties, %llu V with S invalid, %llu S kept, %llu V taken, %llu non-finite outputs", ties, v_only, s_kept, took_V,
          non_finite_out);
    CHECK(single_took >= 1000 && single_clamped >= 100 && single_took - single_clamped >= 1000,
          "the single-candidate runs do not reach every branch: %llu pixels took the history, %llu of them were clamped", single_took, single_clamped);
    // the mirror scene
    const float moves[4][3] = {{10, 0, 0}, {7.3f, -4.1f, 0}, {3, 2, 15}, {0, 0, -20}};
    double worst_dual = 0, least_surface = 1e30;
    for (const auto& size : {std::pair<int, int>(64, 48), std::pair<int, int>(61, 47)})
        for (int m = 0; m < 4; m++) {
            size_t inside = 0, inside_s = 0;
            Outputs dual, surface;
            const double e_dual = mirror_error(size.first, size.second, moves[m], 0.5f, inside, dual);
            const double e_surface = mirror_error(size.first, size.second, moves[m], INF, inside_s, surface);
            CHECK(inside > (size_t)(size.first * size.second / 4), "mirror %d: only %zu pixels inside", m, inside);
            CHECK(e_dual < 1e-5, "mirror %dx%d move %d: the dual pass misses the reflected colour by %.3g", size.first, size.second, m, e_dual);
            CHECK(dual.took_V >= inside, "mirror %dx%d move %d: %llu pixels took V, %zu with every tap inside", size.first, size.second, m, dual.took_V, inside);
            if (m < 2) {
                CHECK(e_surface > 1e-3, "mirror %dx%d move %d: crt_temporal's reprojection misses by %.3g only", size.first, size.second, m, e_surface);
                least_surface = std::min(least_surface, e_surface);
            }
            worst_dual = std::max(worst_dual, e_dual);
            if (out) std::fwrite(dual.color.data(), 4, dual.color.size(), out);
            cases += 2;
        }
    if (out && std::fclose(out) != 0) return 2;
    std::fprintf(stderr, "mirror: dual within %.3g of the reflected colour, crt_temporal's reprojection off by at least %.3g sideways; %llu ties, %llu V with S invalid, %llu S kept, %llu V taken\n",
                 worst_dual, least_surface, ties, v_only, s_kept, took_V);
    std::printf("%d cases, %d failures\n", cases, g_fail);
    return g_fail ? 1 : 0;
}
