// tools/aov_ao_host_check.cpp -- the per-thread text of the ambient-occlusion AOV pass (cudaraytracing_amd/csrc/crt_aov_ao.h, launched by
// crt_aov_ao.hip) compiled for the HOST and run against a plain restatement of the contract of include/crt.h written here, for
// AddressSanitizer / UBSan runs without a device.  crt_aov_ao.h and crt_stages.h are included as they are; tools/host_device.h stands in
// for what they take from outside (with CRT_HOST_PATH: the path code's pieces, bounce_dir among them).  The text has no cross-lane
// operation, so a launch is a loop over its threads.
// The program plays the host side of crt_aov_pass.hip: chunks of whole samples, sub-batches of (sample, q) entries that begin and end
// inside a sample, and between set-up and resolve the trace -- here a table: the answer of the ray of (pixel, k, q) is a hash of the
// three, one of "nothing hit", "a hit well inside the limit" and "a hit beyond the limit" (which only CRT_TRAVERSAL_REFERENCE's closest
// hit ever reports; the any-hit form of blocked() then counts it as an occluder, as the contract's formula says).
// Every buffer is sized exactly, so an access one element out is a report.  The set-up kernel is checked by itself -- each entry's plane
// row and primed ray against the restated position, direction and cosine -- and the resolve through the outputs and the ray count.
// Camera answers are made up per (pixel, k); some pixels are special: 0 only misses; 1 has a NaN normal; 2 a normal with an infinite
// component; 3 a hit at t = +inf (a position that is not finite); 4 a hit at t = NaN; 5 only blocked rays (open == 0: bent_normal +0);
// 6 a zero normal (every direction NaN, every cosine 0: A == 0 with rays > 0, ao = 1.0f); 7 a normal facing away from the ray (nf = -n).
// Frames of 9 x 8 and 10 x 7 pixels (128 slots, partial tiles), and of a 20 x 9 frame the tiled shards of rank 1 of world 3 and of
// rank 3 of world 4, whose second tile lies beyond the image (padding slots: 1.0f, 1.0f, +0).
//
// tests/test_aov_ao.py builds and runs it (tests/host_program.py):
//   g++ -std=c++17 -ffp-contract=off -I cudaraytracing_amd/csrc -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       tools/aov_ao_host_check.cpp -o /tmp/aov_ao_host_check && /tmp/aov_ao_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#define CRT_HOST_PATH
#include "host_device.h"

#include "crt_stages.h"
#include "crt_aov_ao.h"

using namespace crtk;

static int g_fail = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fail++; } \
    } while (0)

static bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }

static uint32_t hash3(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t h = a * 0x9e3779b1u ^ (b + 0x7f4a7c15u) * 0x85ebca6bu ^ (c + 0x165667b1u) * 0xc2b2ae35u;
    h ^= h >> 15; h *= 0x2c1b3c6du; h ^= h >> 12;
    return h;
}
static float unit_of(uint32_t h) { return (float)(h & 0xffffu) / 65536.0f; }

static const float kNan = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();
static const float kEye[3] = {0.3f, 4.5f, -6.0f};

// ---- the made-up scene: 9 triangle normals (unit, except the special ones) ----
static std::vector<float4> make_normals()
{
    std::vector<float4> n;
    n.push_back(make_float4(0.0f, 1.0f, 0.0f, 0.0f));
    n.push_back(make_float4(0.6f, 0.0f, 0.8f, 0.0f));
    n.push_back(make_float4(-0.8f, 0.6f, 0.0f, 0.0f));
    n.push_back(make_float4(0.0f, -0.6f, -0.8f, 0.0f));
    n.push_back(make_float4(kNan, 0.5f, 0.5f, 0.0f));   // 4: pixel 1
    n.push_back(make_float4(0.0f, kInf, 1.0f, 0.0f));   // 5: pixel 2
    n.push_back(make_float4(0.0f, 0.0f, 0.0f, 0.0f));   // 6: pixel 6
    n.push_back(make_float4(0.0f, 0.0f, 1.0f, 0.0f));   // 7: pixel 7 (the camera looks along +z: dot > 0)
    n.push_back(make_float4(1.0f, 0.0f, 0.0f, 0.0f));
    return n;
}

// the camera ray of (pixel, k): its unit direction, and its answer (t, triangle or -1)
struct Cam { float d[3]; float t; int tri; };
static Cam camera_of(uint32_t pixel, uint32_t k)
{
    Cam c;
    float v[3] = {unit_of(hash3(pixel, k, 1)) - 0.5f, unit_of(hash3(pixel, k, 2)) - 0.5f, 0.25f + unit_of(hash3(pixel, k, 3))};
    const float len = std::sqrt(v[0] * v[0] + (v[1] * v[1] + v[2] * v[2]));
    for (int a = 0; a < 3; a++) c.d[a] = v[a] / len;
    c.t = 1.0f + 3.0f * unit_of(hash3(pixel, k, 4));
    const uint32_t h = hash3(pixel, k, 5);
    c.tri = (h & 7u) == 0u ? -1 : (int)((h >> 3) % 4u); // an eighth of the rays miss
    if (pixel == 8u && (h & 7u) == 0u) c.tri = 8;
    if (pixel == 0) c.tri = -1;
    if (pixel == 1) c.tri = 4;
    if (pixel == 2) c.tri = 5;
    if (pixel == 3) { c.tri = 0; c.t = kInf; }
    if (pixel == 4) { c.tri = 1; c.t = kNan; }
    if (pixel == 5) c.tri = 2;
    if (pixel == 6) c.tri = 6;
    if (pixel == 7) c.tri = 7;
    return c;
}

// the table that stands in for the trace: the answer of the occlusion ray of (pixel, k, q) with limit tl
static void answer_of(uint32_t pixel, uint32_t k, uint32_t q, float tl, bool reference_mode, float& T, int& tri)
{
    uint32_t kind = hash3(pixel, k, 100u + q) % 3u;
    if (pixel == 5) kind = 1;
    if (kind == 0) { T = FLT_MAX; tri = -1; }
    else if (kind == 1) { T = tl * 0.5f; tri = 3; }
    else if (reference_mode) { T = tl * 2.0f; tri = 5; } // the closest hit lies beyond the limit
    else { T = FLT_MAX; tri = -1; }                       // (an any-hit ray reports no such hit)
}

// ---- the plain restatement of the contract: one pixel ----
struct PixelOut { float ao, openness, bent[3]; uint32_t rays, open; };
struct EntryOut { bool vertex; float pos[3], dir[3], w; }; // per (k, q) of the pixel: what the set-up kernel must have written
static PixelOut restated_pixel(const std::vector<float4>& nrm, uint32_t pixel, uint32_t spp, uint32_t n_q, float tl, uint64_t seed, bool reference_mode,
                               std::vector<EntryOut>& entries)
{
    PixelOut r{};
    float A = 0.0f, V = 0.0f, b[3] = {0.0f, 0.0f, 0.0f};
    uint32_t rays = 0, open = 0;
    entries.assign((size_t)spp * n_q, EntryOut{});
    for (uint32_t k = 0; k < spp; k++) {
        const Cam c = camera_of(pixel, k);
        if (c.tri < 0) continue;
        float pos[3], nf[3];
        const float4 n = nrm[c.tri];
        const float nn[3] = {n.x, n.y, n.z};
        for (int a = 0; a < 3; a++) pos[a] = kEye[a] + c.t * c.d[a];
        const float dn = c.d[0] * nn[0] + (c.d[1] * nn[1] + c.d[2] * nn[2]);
        for (int a = 0; a < 3; a++) nf[a] = dn > 0.0f ? -nn[a] : nn[a];
        for (uint32_t q = 0; q < n_q; q++) {
            const U4 rr = rng_draw(seed, pixel, k, 0, 4u, q);
            const F3 dir = bounce_dir(f3(nf[0], nf[1], nf[2]), rr);
            float w = dir.x * nf[0] + (dir.y * nf[1] + dir.z * nf[2]);
            w = w > 0.0f ? w : 0.0f;
            EntryOut& e = entries[(size_t)k * n_q + q];
            e.vertex = true; e.w = w;
            e.dir[0] = dir.x; e.dir[1] = dir.y; e.dir[2] = dir.z;
            for (int a = 0; a < 3; a++) e.pos[a] = pos[a];
            float T; int tri;
            answer_of(pixel, k, q, tl, reference_mode, T, tri);
            const bool blocked = reference_mode ? tl - T > 0.00001f : (tri >= 0 || tl - FLT_MAX > 0.00001f);
            rays++;
            A = A + w;
            if (!blocked) {
                V = V + w; open++;
                b[0] = b[0] + dir.x; b[1] = b[1] + dir.y; b[2] = b[2] + dir.z;
            }
        }
    }
    r.ao = A == 0.0f ? 1.0f : V / A;
    r.openness = rays ? (float)open / (float)rays : 1.0f;
    if (open) {
        const float z = b[0] * b[0] + (b[1] * b[1] + b[2] * b[2]);
        if (z > 0.0f) { const float s = std::sqrt(z); for (int a = 0; a < 3; a++) r.bent[a] = b[a] / s; }
        else for (int a = 0; a < 3; a++) r.bent[a] = b[a];
    }
    r.rays = rays; r.open = open;
    return r;
}

// One frame: spp samples in chunks of chunk_spp, sub-batches of `batch` (sample, q) entries
static void run_case(uint32_t w, uint32_t h, uint32_t rank, uint32_t world, bool tiled, uint32_t spp, uint32_t n_q, uint32_t chunk_spp, uint32_t batch,
                     bool reference_mode, int null_mask)
{
    const uint64_t seed = (7ull << 32) | 5u;
    const float tl = 2.5f;
    const std::vector<float4> nrm = make_normals();
    AovAoParams D{};
    D.width = w; D.height = h; D.rank = rank; D.world = world; D.tiles_x = (w + 7) / 8; D.n_tiles = D.tiles_x * ((h + 7) / 8);
    D.nslots = ((D.n_tiles + world - 1) / world) * 64; D.tiled_output = tiled ? 1u : 0u; D.tiles_x_div = make_fastdiv(D.tiles_x);
    const uint32_t nslots = D.nslots, npix = w * h;
    const size_t nout = tiled ? nslots : npix;
    D.seed = seed; D.spp = spp; D.n_q = n_q; D.max_distance = tl; D.reference_mode = reference_mode ? 1u : 0u;
    D.tri_nm = nrm.data();
    const size_t max_rays = (size_t)chunk_spp * nslots, cap = (size_t)std::min<uint64_t>(batch, (uint64_t)chunk_spp * n_q) * nslots;
    std::vector<float4> cam_ro(max_rays), cam_rd(max_rays), vert(max_rays), vnf(max_rays), plane(cap), out_ro(cap), out_rd(cap), acc((size_t)nslots * kAovAoAccRows);
    std::vector<float2> res(max_rays), out_res(cap), ans(cap);
    std::vector<float> ao(nout, kNan), openness(nout, kNan), bent(nout * 3, kNan);
    for (float4& a : acc) a = make_float4(kNan, kNan, kNan, kNan); // (the first sub-batch must not read them)
    D.vert = vert.data(); D.vnf = vnf.data(); D.plane = plane.data(); D.out_ro = out_ro.data(); D.out_rd = out_rd.data(); D.out_res = out_res.data();
    D.acc = acc.data();
    D.ao = (null_mask & 1) ? nullptr : ao.data(); D.openness = (null_mask & 2) ? nullptr : openness.data(); D.bent_normal = (null_mask & 4) ? nullptr : bent.data();
    // the restatement, and what every entry must look like
    std::vector<PixelOut> want(npix);
    std::vector<std::vector<EntryOut>> want_entries(npix);
    uint64_t rays_ref = 0;
    for (uint32_t p = 0; p < npix; p++) want[p] = restated_pixel(nrm, p, spp, n_q, tl, seed, reference_mode, want_entries[p]);
    for (uint32_t slot = 0; slot < nslots; slot++) { // (the shard's pixels)
        const SlotPixel px = slot_pixel(D, slot);
        if (px.valid) rays_ref += want[px.j * w + px.i].rays;
    }
    uint64_t rays_total = 0;
    uint32_t batches = 0, cut_samples = 0;
    for (uint32_t s0 = 0; s0 < spp; s0 += chunk_spp) {
        const uint32_t ns = std::min(chunk_spp, spp - s0);
        D.sample_begin = s0; D.n_samples = ns;
        // the chunk's camera rays and answers; a padding slot: the forward axis and a hit nobody may use
        for (uint32_t s = 0; s < ns; s++)
            for (uint32_t slot = 0; slot < nslots; slot++) {
                const size_t item = (size_t)s * nslots + slot;
                const SlotPixel px = slot_pixel(D, slot);
                cam_ro[item] = make_float4(kEye[0], kEye[1], kEye[2], 0.0f);
                if (px.valid) {
                    const Cam c = camera_of(px.j * w + px.i, s0 + s);
                    cam_rd[item] = make_float4(c.d[0], c.d[1], c.d[2], __uint_as_float((uint32_t)RAY_CLOSEST));
                    res[item] = make_float2(c.t, __int_as_float(c.tri));
                } else {
                    cam_rd[item] = make_float4(0.0f, 0.0f, 1.0f, __uint_as_float((uint32_t)RAY_CLOSEST));
                    res[item] = make_float2(5.0f, __int_as_float(0));
                }
            }
        D.cam_ro = cam_ro.data(); D.cam_rd = cam_rd.data(); D.res = &res[0].x; D.res_stride = 2;
        for (uint64_t item = 0; item < (uint64_t)ns * nslots; item++) aov_ao_vertex(D, item);
        const uint64_t total = (uint64_t)ns * n_q;
        for (uint64_t e0 = 0; e0 < total; e0 += batch) {
            const uint32_t cnt = (uint32_t)std::min<uint64_t>(batch, total - e0);
            D.s_first = (uint32_t)(e0 / n_q); D.q_first = (uint32_t)(e0 % n_q); D.e_count = cnt;
            D.first_batch = s0 == 0 && e0 == 0; D.last_batch = s0 + ns == spp && e0 + cnt == total;
            if (D.q_first != 0 || (e0 + cnt) % n_q != 0) cut_samples++;
            for (float4& p : plane) p = make_float4(kNan, kNan, kNan, kNan); // (what the last sub-batch left must not matter)
            for (float2& a : ans) a = make_float2(kNan, kNan);
            for (uint32_t i = 0; i < cnt * nslots; i++) aov_ao_setup(D, i, i / nslots);
            // the set-up's entries against the restatement, and the trace
            for (uint32_t i = 0; i < cnt * nslots; i++) {
                const uint32_t entry = i / nslots, slot = i - entry * nslots;
                const uint64_t e = e0 + entry;
                const uint32_t k = s0 + (uint32_t)(e / n_q), q = (uint32_t)(e % n_q);
                const SlotPixel px = slot_pixel(D, slot);
                CHECK(__float_as_uint(out_rd[i].w) == (uint32_t)RAY_SHADOW && out_res[i].x == FLT_MAX && __float_as_int(out_res[i].y) == -1 && out_ro[i].w == tl,
                      "entry %u is not primed as a visibility ray of limit %a", i, tl);
                const EntryOut* eo = px.valid ? &want_entries[px.j * w + px.i][(size_t)k * n_q + q] : nullptr;
                if (!eo || !eo->vertex) {
                    CHECK(plane[i].w < 0.0f && plane[i].x == 0.0f && plane[i].y == 0.0f && plane[i].z == 0.0f, "entry %u has no vertex but a plane row", i);
                    CHECK(out_ro[i].x == kEye[0] && out_ro[i].y == kEye[1] && out_ro[i].z == kEye[2], "entry %u has no vertex: its ray starts at the eye", i);
                    ans[i] = make_float2(1.0f, __int_as_float(2)); // (an occluder nobody may count)
                    continue;
                }
                CHECK(same_bits(plane[i].x, eo->dir[0]) && same_bits(plane[i].y, eo->dir[1]) && same_bits(plane[i].z, eo->dir[2]) && same_bits(plane[i].w, eo->w),
                      "entry %u (pixel %u, k %u, q %u): plane row (%a %a %a, %a), expected (%a %a %a, %a)", i, px.j * w + px.i, k, q, plane[i].x, plane[i].y, plane[i].z,
                      plane[i].w, eo->dir[0], eo->dir[1], eo->dir[2], eo->w);
                CHECK(same_bits(out_ro[i].x, eo->pos[0]) && same_bits(out_ro[i].y, eo->pos[1]) && same_bits(out_ro[i].z, eo->pos[2]), "entry %u: ray origin", i);
                CHECK(same_bits(out_rd[i].x, eo->dir[0]) && same_bits(out_rd[i].y, eo->dir[1]) && same_bits(out_rd[i].z, eo->dir[2]), "entry %u: ray direction", i);
                float T; int tri;
                answer_of(px.j * w + px.i, k, q, tl, reference_mode, T, tri);
                ans[i] = make_float2(T, __int_as_float(tri));
            }
            D.ans = &ans[0].x; D.ans_stride = 2;
            for (uint32_t slot = 0; slot < nslots; slot++) {
                const uint32_t n = aov_ao_resolve(D, slot);
                CHECK(D.last_batch || n == 0, "a sub-batch that is not the last reports rays");
                rays_total += n;
            }
            batches++;
        }
    }
    CHECK(rays_total == rays_ref && rays_ref > 0, "%ux%u: %llu occlusion rays, expected %llu", w, h, (unsigned long long)rays_total, (unsigned long long)rays_ref);
    if (batch % n_q != 0 && batch < spp * n_q) CHECK(cut_samples > 0, "no sub-batch border inside a sample");
    // the outputs
    std::vector<char> seen(nout, 0);
    for (uint32_t slot = 0; slot < nslots; slot++) {
        const SlotPixel px = slot_pixel(D, slot);
        if (!px.out) continue;
        seen[px.o] = 1;
        PixelOut r{};
        r.ao = r.openness = 1.0f; // a padding slot
        if (px.valid) r = want[px.j * w + px.i];
        const size_t o = px.o;
        if (D.ao) CHECK(same_bits(ao[o], r.ao), "%ux%u: ao of slot %u: %a, expected %a", w, h, slot, ao[o], r.ao);
        if (D.openness) CHECK(same_bits(openness[o], r.openness), "%ux%u: openness of slot %u: %a, expected %a", w, h, slot, openness[o], r.openness);
        if (D.bent_normal)
            for (int a = 0; a < 3; a++) CHECK(same_bits(bent[o * 3 + a], r.bent[a]), "%ux%u: bent_normal of slot %u, component %d: %a, expected %a", w, h, slot, a, bent[o * 3 + a], r.bent[a]);
    }
    for (size_t o = 0; o < nout; o++) CHECK(seen[o], "output %zu has no slot", o);
    if (null_mask & 1) for (float v : ao) CHECK(v != v, "a null output was written");
    if (null_mask & 2) for (float v : openness) CHECK(v != v, "a null output was written");
    if (null_mask & 4) for (float v : bent) CHECK(v != v, "a null output was written");
    // the special pixels are what they are meant to be (frames of rank 0, world 1)
    if (!tiled) {
        CHECK(want[0].rays == 0 && want[0].ao == 1.0f && want[0].openness == 1.0f && same_bits(want[0].bent[0], 0.0f), "pixel 0 only misses");
        CHECK(want[5].rays == spp * n_q && want[5].open == 0 && want[5].ao == 0.0f && want[5].openness == 0.0f && same_bits(want[5].bent[1], 0.0f), "pixel 5: open == 0");
        CHECK(want[6].rays == spp * n_q && want[6].ao == 1.0f, "pixel 6: A == 0 with rays");
        CHECK(want[1].rays == spp * n_q && want[2].rays == spp * n_q && want[3].rays == spp * n_q && want[4].rays == spp * n_q, "pixels 1 - 4 hit on every sample");
        CHECK(want_entries[3][0].pos[0] != want_entries[3][0].pos[0] || std::isinf(want_entries[3][0].pos[0]) || std::isinf(want_entries[3][0].pos[2]), "pixel 3: a position that is not finite");
        CHECK(want_entries[4][0].pos[0] != want_entries[4][0].pos[0], "pixel 4: a NaN position");
    }
    (void)batches;
}

int main()
{
    int cases = 0;
    const uint32_t shapes[2][2] = {{9, 8}, {10, 7}};
    for (const auto& sh : shapes)
        for (bool reference_mode : {false, true}) {
            run_case(sh[0], sh[1], 0, 1, false, 3, 5, 2, 3, reference_mode, 0); // chunks of 2 + 1 samples, sub-batches of 3 of a sample's 5 entries
            cases++;
        }
    run_case(9, 8, 0, 1, false, 3, 5, 3, 7, false, 0);   // one chunk; sub-batches of 7 entries: longer than a sample, borders inside samples
    run_case(9, 8, 0, 1, false, 3, 2, 1, 1, true, 0);    // a chunk per sample, an entry per sub-batch
    run_case(10, 7, 0, 1, false, 1, 1, 1, 4, false, 0);  // one sample, one ray: a single sub-batch that is first and last
    run_case(10, 7, 0, 1, false, 2, 4, 2, 8, false, 0);  // the whole call in one sub-batch
    run_case(9, 8, 0, 1, false, 3, 5, 2, 3, false, 1);   // ao null
    run_case(9, 8, 0, 1, false, 3, 5, 2, 3, false, 6);   // openness and bent_normal null
    run_case(20, 9, 1, 3, true, 3, 5, 2, 3, false, 0);   // the tiled shard of rank 1 of world 3: 6 tiles, 2 per rank, ragged in both directions
    run_case(20, 9, 3, 4, true, 2, 3, 2, 4, true, 0);    // rank 3 of world 4: its second tile lies beyond the image
    cases += 8;
    std::printf("%d cases, %d failures\n", cases, g_fail);
    return g_fail ? 1 : 0;
}
