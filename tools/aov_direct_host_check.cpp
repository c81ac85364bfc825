// tools/aov_direct_host_check.cpp -- the kernels of the direct-light AOV pass (cudaraytracing_amd/csrc/crt_aov_direct.h, launched by
// crt_aov_direct.hip) compiled for the HOST and run against a plain restatement of the contract of include/crt.h written here, for
// AddressSanitizer / UBSan runs without a device.  The two kernel files and crt_stages.h are included as they are; tools/host_device.h
// stands in for what they take from outside, a wave being 64 host threads that meet at a barrier in every cross-lane operation.  The
// program plays the host side of crt_aov_pass.hip: chunks of whole samples, sub-batches of (sample, q) entries, the count read back, the
// trace -- a brute-force any-hit (REFERENCE: closest-hit) over the scene's triangles -- between the set-up and the answer kernel.
// Every buffer is sized exactly, so an access one element out is a report.
// The scene is hand-made, 12 triangles: a floor, an occluder above it, a black patch (every contribution zero: not traced), a patch whose
// BSDF row is NaN (every contribution NaN: traced), and two lights, of 1 and of 3 triangles.  Frames of 9 x 8 pixels (pixel slots come in
// tiles of 64: a full wave and a partial one) and of 10 x 7 (70 pixels, two partial waves), spp 3 in chunks of 2 + 1 samples,
// light_sample_n 3 (the division) and 2 (the power of two), sub-batches of 5 entries, so that borders fall inside a sample; pixel 0 only
// misses and pixel 1 only hits the emitter.  The four outputs and the traced count must be the restatement's, bit for bit.
// Run as `aov_direct_host_check JOB OUT` (JOB is not read) it also writes every output of every case to OUT: tests/test_aov_direct.py
// compares the bytes of the plain and the sanitised build.
//
// tests/test_aov_direct.py builds and runs it (tests/host_program.py):
//   g++ -std=c++17 -ffp-contract=off -I cudaraytracing_amd/csrc -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       tools/aov_direct_host_check.cpp -pthread -o /tmp/aov_direct_host_check && /tmp/aov_direct_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#define CRT_INTERNAL_H // (the kernel file's only include: replaced by host_device.h)
#define CRT_HOST_WAVES
#define CRT_HOST_PATH
#include "host_device.h"

#include "crt_stages.h"
#include "crt_aov_direct.hip"

using namespace crtk;

static int g_fail = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fail++; } \
    } while (0)

static bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }

// ---- the scene, in plain arrays ----
struct V { float x, y, z; };
static V operator-(V a, V b) { return V{a.x - b.x, a.y - b.y, a.z - b.z}; }
static V cross(V a, V b) { return V{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static float dot(V a, V b) { return a.x * b.x + (a.y * b.y + a.z * b.z); }
struct Tri { V v1, v2, v3, n; int mat; };
struct Mat { V kd, ke; bool emit; };
struct Scene {
    std::vector<Tri> tris;
    std::vector<Mat> mats;
    std::vector<float4> tri_nm, mat_rows, ltri;
    std::vector<uint4> lights;
    std::vector<std::vector<int>> light_tris; // scene triangles of each light
};
static void quad(Scene& s, V a, V b, V c, V d, V n, int mat)
{
    s.tris.push_back(Tri{a, b, c, n, mat});
    s.tris.push_back(Tri{a, c, d, n, mat});
}
static Scene make_scene()
{
    Scene s;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    s.mats = {{{0.7f, 0.6f, 0.5f}, {0, 0, 0}, false},      // 0 floor
              {{0.3f, 0.8f, 0.2f}, {0, 0, 0}, false},      // 1 occluder
              {{0.0f, 0.0f, 0.0f}, {0, 0, 0}, false},      // 2 black
              {{nan, 0.5f, 0.5f}, {0, 0, 0}, false},       // 3 NaN
              {{0.0f, 0.0f, 0.0f}, {17.0f, 12.0f, 4.0f}, true},   // 4 light A
              {{0.0f, 0.0f, 0.0f}, {3.0f, 5.0f, 9.0f}, true}};    // 5 light B
    const V up{0, 1, 0}, down{0, -1, 0};
    quad(s, V{-3, 0, -3}, V{-3, 0, 3}, V{3, 0, 3}, V{3, 0, -3}, up, 0);
    quad(s, V{-0.5f, 1, -0.5f}, V{-0.5f, 1, 0.9f}, V{0.7f, 1, 0.9f}, V{0.7f, 1, -0.5f}, up, 1);
    quad(s, V{1.5f, 0.01f, 1.5f}, V{1.5f, 0.01f, 2.5f}, V{2.5f, 0.01f, 2.5f}, V{2.5f, 0.01f, 1.5f}, up, 2);
    quad(s, V{-2.5f, 0.01f, 1.5f}, V{-2.5f, 0.01f, 2.5f}, V{-1.5f, 0.01f, 2.5f}, V{-1.5f, 0.01f, 1.5f}, up, 3);
    const int a0 = (int)s.tris.size();
    s.tris.push_back(Tri{V{-0.4f, 3, -0.3f}, V{0.5f, 3, -0.3f}, V{0.1f, 3, 0.6f}, down, 4});
    const int b0 = (int)s.tris.size();
    s.tris.push_back(Tri{V{1.0f, 2.5f, -2.0f}, V{2.0f, 2.5f, -2.0f}, V{1.5f, 2.5f, -1.0f}, down, 5});
    s.tris.push_back(Tri{V{2.0f, 2.5f, -2.0f}, V{2.5f, 2.5f, -1.0f}, V{1.5f, 2.5f, -1.0f}, down, 5});
    s.tris.push_back(Tri{V{-2.0f, 2.0f, -2.0f}, V{-1.2f, 2.0f, -2.0f}, V{-1.6f, 2.0f, -1.1f}, down, 5});
    s.light_tris = {{a0}, {b0, b0 + 1, b0 + 2}};
    for (const Tri& t : s.tris) {
        const Mat& m = s.mats[t.mat];
        s.tri_nm.push_back(make_float4(t.n.x, t.n.y, t.n.z, __uint_as_float((uint32_t)t.mat | (m.emit ? 1u << 30 : 0u))));
    }
    for (const Mat& m : s.mats) {
        const float pi = (float)3.14159265358979323846;
        s.mat_rows.push_back(make_float4(m.kd.x / pi, m.kd.y / pi, m.kd.z / pi, 1.0f));
        s.mat_rows.push_back(make_float4(m.kd.x, m.kd.y, m.kd.z, 0.0f));
        s.mat_rows.push_back(make_float4(m.ke.x, m.ke.y, m.ke.z, 0.0f));
    }
    const float area[2] = {0.405f, 1.31f}; // (area_of_obj: any positive numbers do)
    uint32_t first = 0;
    for (size_t l = 0; l < s.light_tris.size(); l++) {
        for (int ti : s.light_tris[l]) {
            const Tri& t = s.tris[ti];
            const Mat& m = s.mats[t.mat];
            s.ltri.push_back(make_float4(t.v1.x, t.v1.y, t.v1.z, t.v2.x));
            s.ltri.push_back(make_float4(t.v2.y, t.v2.z, t.v3.x, t.v3.y));
            s.ltri.push_back(make_float4(t.v3.z, t.n.x, t.n.y, t.n.z));
            s.ltri.push_back(make_float4(m.ke.x, m.ke.y, m.ke.z, area[l]));
        }
        const uint32_t count = (uint32_t)s.light_tris[l].size();
        const FastDiv fd = make_fastdiv(count);
        s.lights.push_back(uint4{first, count, fd.m, fd.sh});
        first += count;
    }
    return s;
}

// brute force: the closest hit with t > epsilon (Moeller-Trumbore); any_below >= 0: the first triangle with epsilon < t and
// limit - t > epsilon instead (an any-hit ray's answer)
static void brute(const Scene& s, V o, V d, bool any_hit, float limit, float& T, int& tri)
{
    T = FLT_MAX; tri = -1;
    for (size_t i = 0; i < s.tris.size(); i++) {
        const Tri& t = s.tris[i];
        const V e1 = t.v2 - t.v1, e2 = t.v3 - t.v1, p = cross(d, e2);
        const float det = dot(e1, p);
        if (!(std::fabs(det) > 1e-12f)) continue;
        const V tv = o - t.v1, q = cross(tv, e1);
        const float u = dot(tv, p) / det, v = dot(d, q) / det, tt = dot(e2, q) / det;
        if (!(u >= 0.0f && v >= 0.0f && u + v <= 1.0f && tt > CRT_EPSILON)) continue;
        if (any_hit) {
            if (limit - tt > CRT_EPSILON) { T = tt; tri = (int)i; return; }
        } else if (tt < T) { T = tt; tri = (int)i; }
    }
}

static uint32_t hash3(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t h = a * 0x9e3779b1u ^ (b + 0x7f4a7c15u) * 0x85ebca6bu ^ (c + 0x165667b1u) * 0xc2b2ae35u;
    h ^= h >> 15; h *= 0x2c1b3c6du; h ^= h >> 12;
    return h;
}

// ---- the plain restatement of the contract: the four outputs of one pixel and its traced count ----
struct PixelOut { float direct[3], unshadowed[3], variance[3], visibility; uint32_t traced; };
static PixelOut restated_pixel(const Scene& sc, const std::vector<V>& eye_d, const std::vector<float>& cam_t, const std::vector<int>& cam_tri, V eye, uint32_t pixel,
                               uint32_t spp, int lsn, uint64_t seed, bool reference_mode)
{
    PixelOut r{};
    float c3[3] = {0, 0, 0}, q3[3] = {0, 0, 0}, u3[3] = {0, 0, 0};
    uint32_t traced = 0, lit = 0;
    const uint32_t n_lights = (uint32_t)sc.light_tris.size();
    for (uint32_t k = 0; k < spp; k++) {
        float Ld[3] = {0, 0, 0}, U[3] = {0, 0, 0};
        const int tri = cam_tri[(size_t)pixel * spp + k];
        if (tri >= 0 && !sc.mats[sc.tris[tri].mat].emit) {
            const V d = eye_d[(size_t)pixel * spp + k];
            const float t = cam_t[(size_t)pixel * spp + k];
            const V pos{eye.x + t * d.x, eye.y + t * d.y, eye.z + t * d.z};
            const Tri& T = sc.tris[tri];
            const float pi = (float)3.14159265358979323846;
            const float fr[3] = {sc.mats[T.mat].kd.x / pi, sc.mats[T.mat].kd.y / pi, sc.mats[T.mat].kd.z / pi};
            for (uint32_t li = 0; li < n_lights; li++)
                for (int sj = 0; sj < lsn; sj++) {
                    const uint32_t q = li * (uint32_t)lsn + (uint32_t)sj;
                    const U4 rl = rng_draw(seed, pixel, k, 0, RNG_NEE, q);
                    const Tri& L = sc.tris[sc.light_tris[li][rl.x % sc.light_tris[li].size()]];
                    const float alpha = rng_uniform(rl.y), beta = rng_uniform(rl.z) * (1 - alpha), gamma = 1 - alpha - beta;
                    const V lpos{(alpha * L.v1.x + beta * L.v2.x) + gamma * L.v3.x, (alpha * L.v1.y + beta * L.v2.y) + gamma * L.v3.y,
                                 (alpha * L.v1.z + beta * L.v2.z) + gamma * L.v3.z};
                    const V dist = lpos - pos;
                    const float z = dot(dist, dist);
                    V dir = dist;
                    if (z > 0.0f) { const float s = std::sqrt(z); dir = V{dist.x / s, dist.y / s, dist.z / s}; }
                    V rd = dir;
                    const float z2 = dot(dir, dir);
                    if (z2 > 0.0f) { const float s = std::sqrt(z2); rd = V{dir.x / s, dir.y / s, dir.z / s}; }
                    const float tl = dist.x / dir.x;
                    const float len = std::sqrt(dot(dist, dist)), t2 = len * len;
                    float ct = dot(dir, T.n), ct2 = -dot(dir, L.n);
                    ct = ct > 0.0f ? ct : 0.0f;
                    ct2 = ct2 > 0.0f ? ct2 : 0.0f;
                    const Mat& lm = sc.mats[L.mat];
                    const float ke[3] = {lm.ke.x, lm.ke.y, lm.ke.z};
                    const float area = li == 0 ? 0.405f : 1.31f;
                    float c[3];
                    for (int ch = 0; ch < 3; ch++) {
                        float x = ke[ch] * fr[ch];
                        x = x * ct; x = x * ct2; x = x * area; x = x / t2;
                        c[ch] = (lsn & (lsn - 1)) == 0 ? x * (1.0f / (float)lsn) : x / (float)lsn;
                    }
                    if (c[0] == 0.0f && c[1] == 0.0f && c[2] == 0.0f) continue; // not traced
                    traced++;
                    float Th; int th;
                    brute(sc, pos, rd, !reference_mode, tl, Th, th);
                    const bool blocked = reference_mode ? tl - Th > CRT_EPSILON : (th >= 0 || tl - FLT_MAX > CRT_EPSILON);
                    for (int ch = 0; ch < 3; ch++) U[ch] = U[ch] + c[ch];
                    if (!blocked) { lit++; for (int ch = 0; ch < 3; ch++) Ld[ch] = Ld[ch] + c[ch]; }
                }
        }
        for (int ch = 0; ch < 3; ch++) {
            const float x = Ld[ch] / (float)spp;
            c3[ch] = c3[ch] + x; q3[ch] = q3[ch] + x * x;
            u3[ch] = u3[ch] + U[ch] / (float)spp;
        }
    }
    for (int ch = 0; ch < 3; ch++) {
        r.direct[ch] = c3[ch]; r.unshadowed[ch] = u3[ch];
        float d = (float)spp * q3[ch] - c3[ch] * c3[ch];
        d = d < 0.0f ? 0.0f : d;
        r.variance[ch] = spp > 1 ? (1.0f * d) / ((float)spp - 1.0f) : 0.0f;
    }
    r.visibility = traced ? (float)lit / (float)traced : 1.0f;
    r.traced = traced;
    return r;
}

static std::vector<float> g_dump;

// One frame of w x h, spp samples in chunks of chunk_spp, sub-batches of batch (sample, q) entries
static void run_case(const Scene& sc, uint32_t w, uint32_t h, uint32_t spp, int lsn, uint32_t chunk_spp, uint32_t batch, bool reference_mode, bool some_null)
{
    const uint64_t seed = (7ull << 32) | 5u;
    const V eye{0.3f, 4.5f, -6.0f};
    AovDirectParams D{};
    D.width = w; D.height = h; D.rank = 0; D.world = 1; D.tiles_x = (w + 7) / 8; D.n_tiles = D.tiles_x * ((h + 7) / 8);
    D.nslots = D.n_tiles * 64; D.tiled_output = 0; D.tiles_x_div = make_fastdiv(D.tiles_x);
    const uint32_t nslots = D.nslots, npix = w * h, n_q = (uint32_t)sc.lights.size() * (uint32_t)lsn;
    // the camera rays of every (pixel, sample) and their answers
    std::vector<V> dir((size_t)npix * spp);
    std::vector<float> cam_t((size_t)npix * spp);
    std::vector<int> cam_tri((size_t)npix * spp);
    for (uint32_t p = 0; p < npix; p++)
        for (uint32_t k = 0; k < spp; k++) {
            const uint32_t hx = hash3(p, k, 1), hz = hash3(p, k, 2);
            V target{-2.9f + 5.8f * (float)(hx & 0xffffu) / 65536.0f, 0.0f, -2.9f + 5.8f * (float)(hz & 0xffffu) / 65536.0f};
            if (p == 0) target = V{target.x, 9.0f, 20.0f};                       // pixel 0 only misses
            if (p == 1) target = V{0.05f + 0.01f * (float)k, 3.0f, 0.0f};        // pixel 1 only hits light A
            if (p == 2) target = V{2.0f, 0.01f, 2.0f};                           // the black patch: zero contributions
            if (p == 3) target = V{-2.0f, 0.01f, 2.0f};                          // the NaN patch: NaN contributions
            if (p == 4) target = V{0.1f, 0.0f, 0.2f + 0.01f * (float)k};         // under the occluder
            const V dv = target - eye;
            const float s = std::sqrt(dot(dv, dv));
            const V d{dv.x / s, dv.y / s, dv.z / s};
            dir[(size_t)p * spp + k] = d;
            brute(sc, eye, d, false, 0.0f, cam_t[(size_t)p * spp + k], cam_tri[(size_t)p * spp + k]);
        }
    for (uint32_t k = 0; k < spp; k++) CHECK(cam_tri[k] < 0, "pixel 0 is meant to miss");
    CHECK(cam_tri[spp] >= 0 && sc.mats[sc.tris[cam_tri[spp]].mat].emit, "pixel 1 is meant to hit the emitter");
    CHECK(cam_tri[2 * spp] >= 0 && sc.tris[cam_tri[2 * spp]].mat == 2, "pixel 2 is meant to hit the black patch");
    CHECK(cam_tri[3 * spp] >= 0 && sc.tris[cam_tri[3 * spp]].mat == 3, "pixel 3 is meant to hit the NaN patch");

    D.seed = seed; D.spp = spp;
    D.tri_nm = sc.tri_nm.data(); D.mats = sc.mat_rows.data(); D.ltri = sc.ltri.data(); D.lights = sc.lights.data();
    D.n_q = n_q; D.lsn = lsn; D.inv_lsn_pow2 = (lsn & (lsn - 1)) == 0 ? 1.0f / (float)lsn : 0.0f; D.lsn_div = make_fastdiv((uint32_t)lsn);
    D.reference_mode = reference_mode ? 1u : 0u;
    const size_t max_rays = (size_t)chunk_spp * nslots, cap = (size_t)batch * nslots;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float4> cam_ro(max_rays), cam_rd(max_rays), vert(max_rays), plane(cap), out_ro(cap), out_rd(cap), acc((size_t)nslots * kAovDirectAccRows);
    std::vector<float2> res(max_rays), out_res(cap), ans(cap);
    std::vector<uint32_t> out_idx(cap);
    std::vector<unsigned int> count(1);
    std::vector<float> direct((size_t)npix * 3, nan), unshadowed((size_t)npix * 3, nan), variance((size_t)npix * 3, nan), visibility(npix, nan);
    for (float4& a : acc) a = make_float4(nan, nan, nan, nan); // (the first sub-batch must not read them)
    D.vert = vert.data(); D.plane = plane.data(); D.out_ro = out_ro.data(); D.out_rd = out_rd.data(); D.out_res = out_res.data(); D.out_idx = out_idx.data();
    D.count = count.data(); D.acc = acc.data();
    D.direct = direct.data(); D.unshadowed = some_null ? nullptr : unshadowed.data(); D.direct_variance = variance.data();
    D.visibility = some_null ? nullptr : visibility.data();
    uint64_t traced_total = 0;
    uint32_t batches = 0;
    for (uint32_t s0 = 0; s0 < spp; s0 += chunk_spp) {
        const uint32_t ns = std::min(chunk_spp, spp - s0);
        D.sample_begin = s0; D.n_samples = ns;
        // the chunk's camera rays and answers, item = sample of the chunk x nslots + slot; a padding slot: the forward axis, a hit nobody may read
        for (uint32_t s = 0; s < ns; s++)
            for (uint32_t slot = 0; slot < nslots; slot++) {
                const size_t item = (size_t)s * nslots + slot;
                const SlotPixel px = slot_pixel(D, slot);
                cam_ro[item] = make_float4(eye.x, eye.y, eye.z, 0.0f);
                if (px.valid) {
                    const size_t ps = (size_t)(px.j * w + px.i) * spp + s0 + s;
                    cam_rd[item] = make_float4(dir[ps].x, dir[ps].y, dir[ps].z, __uint_as_float((uint32_t)RAY_CLOSEST));
                    res[item] = make_float2(cam_t[ps], __int_as_float(cam_tri[ps]));
                } else {
                    cam_rd[item] = make_float4(0.0f, 0.0f, 1.0f, __uint_as_float((uint32_t)RAY_CLOSEST));
                    res[item] = make_float2(5.0f, __int_as_float(0)); // (the floor: it would be lit)
                }
            }
        D.cam_ro = cam_ro.data(); D.cam_rd = cam_rd.data(); D.res = &res[0].x; D.res_stride = 2;
        launch_aov_direct_vertex(D, nullptr);
        const uint64_t total = (uint64_t)ns * n_q;
        for (uint64_t e0 = 0; e0 < total; e0 += batch) {
            const uint32_t cnt = (uint32_t)std::min<uint64_t>(batch, total - e0);
            D.s_first = (uint32_t)(e0 / n_q); D.q_first = (uint32_t)(e0 % n_q); D.e_count = cnt;
            D.first_batch = s0 == 0 && e0 == 0; D.last_batch = s0 + ns == spp && e0 + cnt == total;
            count[0] = 0;
            for (float4& p : plane) p = make_float4(nan, nan, nan, __uint_as_float(0xffffffffu)); // (what the last sub-batch left must not matter)
            launch_aov_direct_setup(D, nullptr);
            const uint32_t n = count[0];
            CHECK(n <= cnt * nslots, "the set-up kernel counts %u traced rays of %u entries", n, cnt * nslots);
            if (n > cnt * nslots) return;
            for (uint32_t j = 0; j < n; j++) { // the trace
                CHECK(__float_as_uint(out_rd[j].w) == (uint32_t)RAY_SHADOW && out_res[j].x == FLT_MAX && __float_as_int(out_res[j].y) == -1, "ray %u is not primed as a visibility ray", j);
                float T; int tri;
                brute(sc, V{out_ro[j].x, out_ro[j].y, out_ro[j].z}, V{out_rd[j].x, out_rd[j].y, out_rd[j].z}, !reference_mode, out_ro[j].w, T, tri);
                ans[j] = make_float2(T, __int_as_float(tri));
            }
            D.ans = &ans[0].x; D.ans_stride = 2; D.n_traced = n;
            if (n) launch_aov_direct_answer(D, nullptr);
            launch_aov_direct_resolve(D, nullptr);
            traced_total += n;
            batches++;
        }
    }
    CHECK(batches > 1, "one sub-batch only");
    uint64_t traced_ref = 0;
    for (uint32_t p = 0; p < npix; p++) {
        const PixelOut r = restated_pixel(sc, dir, cam_t, cam_tri, eye, p, spp, lsn, seed, reference_mode);
        traced_ref += r.traced;
        for (int ch = 0; ch < 3; ch++) {
            CHECK(same_bits(direct[(size_t)p * 3 + ch], r.direct[ch]), "%ux%u lsn %d: direct of pixel %u, channel %d: %a, expected %a", w, h, lsn, p, ch, direct[(size_t)p * 3 + ch], r.direct[ch]);
            CHECK(same_bits(variance[(size_t)p * 3 + ch], r.variance[ch]), "%ux%u lsn %d: direct_variance of pixel %u, channel %d: %a, expected %a", w, h, lsn, p, ch, variance[(size_t)p * 3 + ch], r.variance[ch]);
            if (!some_null) CHECK(same_bits(unshadowed[(size_t)p * 3 + ch], r.unshadowed[ch]), "%ux%u lsn %d: unshadowed of pixel %u, channel %d: %a, expected %a", w, h, lsn, p, ch, unshadowed[(size_t)p * 3 + ch], r.unshadowed[ch]);
        }
        if (!some_null) CHECK(same_bits(visibility[p], r.visibility), "%ux%u lsn %d: visibility of pixel %u: %a, expected %a", w, h, lsn, p, visibility[p], r.visibility);
        if (p == 0 || p == 1 || p == 2) CHECK(r.traced == 0 && r.visibility == 1.0f && r.direct[0] == 0.0f, "pixel %u: nothing is meant to be traced", p);
        if (p == 3) CHECK(r.traced == spp * n_q && r.direct[0] != r.direct[0], "pixel 3: every sample is meant to be traced, with a NaN contribution");
    }
    CHECK(traced_total == traced_ref, "%ux%u lsn %d: %llu rays traced, expected %llu", w, h, lsn, (unsigned long long)traced_total, (unsigned long long)traced_ref);
    CHECK(traced_ref > 0, "nothing traced");
    if (some_null) { // (untouched)
        for (float v : unshadowed) CHECK(v != v, "a null output was written");
    }
    g_dump.insert(g_dump.end(), direct.begin(), direct.end());
    g_dump.insert(g_dump.end(), variance.begin(), variance.end());
    if (!some_null) { g_dump.insert(g_dump.end(), unshadowed.begin(), unshadowed.end()); g_dump.insert(g_dump.end(), visibility.begin(), visibility.end()); }
    g_dump.push_back((float)traced_total);
}

int main(int argc, char** argv)
{
    const Scene sc = make_scene();
    int cases = 0;
    const uint32_t shapes[2][2] = {{9, 8}, {10, 7}};
    for (const auto& sh : shapes)
        for (int lsn : {3, 2})
            for (bool reference_mode : {false, true}) {
                run_case(sc, sh[0], sh[1], 3, lsn, 2, 5, reference_mode, false); // chunks of 2 + 1 samples, sub-batches of 5 entries
                cases++;
            }
    run_case(sc, 9, 8, 3, 3, 3, 5, false, true);  // one chunk; two of the outputs null
    run_case(sc, 9, 8, 3, 2, 1, 1, false, false); // a chunk per sample, an entry per sub-batch
    run_case(sc, 10, 7, 1, 3, 1, 5, false, false); // one sample: no variance
    cases += 3;
    if (argc > 2) {
        std::FILE* f = std::fopen(argv[2], "wb");
        if (!f || std::fwrite(g_dump.data(), sizeof(float), g_dump.size(), f) != g_dump.size()) { std::printf("cannot write %s\n", argv[2]); return 2; }
        std::fclose(f);
    }
    std::printf("%d cases, %d failures\n", cases, g_fail);
    return g_fail ? 1 : 0;
}
