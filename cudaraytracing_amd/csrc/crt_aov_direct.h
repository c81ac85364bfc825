// cudaraytracing_amd/csrc/crt_aov_direct.h -- the per-thread text of the direct-light AOV pass (crt_render_aov_direct, contract:
// include/crt.h; kernels: crt_aov_direct.hip; host side: crt_aov_pass.hip).  Per camera ray of a chunk the pass recomputes, sample for
// sample, the next-event term L_dir of the first vertex of the frame's own path -- the draws (seed, pixel, k, 0, RNG_NEE, q) depend on
// nothing later in the path -- and folds it into the direct, unshadowed, direct_variance and visibility buffers.  Four stages:
//   vertex   one thread per camera ray: (pos, triangle or -1) of the first vertex, copied out of the camera answers before the first
//            shadow trace overwrites them (-1: a miss, an emitter, a padding slot)
//   set-up   the (sample, q, slot) entries of a sub-batch, eight per thread: the sample's contribution c and its shadow ray; (c, flags)
//            into the contribution plane, the traced rays compacted into the second region of the query pool
//   answer   one thread per traced ray: clears the blocked flag of its plane entry when the ray is unblocked
//   resolve  one thread per slot: walks the sub-batch's entries in order into the running sums of the slot's accumulator rows
// A sub-batch is a range of the chunk's linear (sample, q) order and may begin and end inside a sample: the sums of the sample in
// progress cross its borders in the accumulator rows.
// Like crt_nlm.h this file includes nothing, so that tools/aov_direct_host_check.cpp can compile this very text for the host behind
// tools/host_device.h's stand-ins for what it takes from outside: SlotMap / slot_pixel / variance_of3 (crt_stages.h), F3 and its
// operations, fast_div, TNM_* (crt_device.h), rng_draw / rng_uniform (crt_detmath.h), shadow_blocked, RAY_SHADOW (crt_path.h), the wave
// intrinsics and the atomics.
#ifndef CRT_AOV_DIRECT_H
#define CRT_AOV_DIRECT_H

namespace crtk {

const uint32_t kAovDirectAccRows = 5; // float4 rows of a slot's running sums (AovDirectParams::acc)
enum { AOVD_TRACED = 1u, AOVD_BLOCKED = 2u }; // flags of a contribution-plane entry
const uint32_t kAovDirectWaveEntries = 8; // entries of a sub-batch that one wave of the set-up kernel takes (aov_direct_setup)

struct AovDirectParams : SlotMap {
    uint64_t seed;
    uint32_t spp, sample_begin, n_samples;   // the chunk: samples [sample_begin, sample_begin + n_samples) of every slot
    // scene
    const float4* tri_nm;                    // normal.xyz, bits(material word) per triangle
    const float4* mats;                      // 3 rows per material, row 0 = (kd / pi .xyz, ns)
    const float4* ltri;                      // 4 rows per light triangle (crt_device.h)
    const uint4* lights;                     // (first, count, division magic, shifts) per light
    uint32_t n_q;                            // next-event samples per vertex: lights x lsn
    int32_t lsn;
    float inv_lsn_pow2;                      // as LParams'
    FastDiv lsn_div;
    uint32_t reference_mode;                 // CRT_TRAVERSAL_REFERENCE: blocked() compares the limit with the closest hit's distance
    // vertex kernel: the camera rays (item = sample of the chunk x nslots + slot) and their answers
    const float4* cam_ro;
    const float4* cam_rd;
    const float* res;                        // (t, bits(triangle or -1)) of item i at res[i * res_stride]
    uint32_t res_stride;
    float4* vert;                            // per item: pos.xyz, bits(triangle, or -1)
    // the sub-batch: e_count entries of the chunk's linear order (sample of the chunk x n_q + q), from (s_first, q_first) on
    uint32_t s_first, q_first, e_count;
    float4* plane;                           // [e_count][nslots]: c.xyz, bits(flags)
    // set-up kernel: the traced rays, compacted, in the form k_fill_rays writes a visibility ray
    float4* out_ro;                          // origin.xyz, limit
    float4* out_rd;                          // unit direction.xyz, bits(RAY_SHADOW)
    float2* out_res;
    uint32_t* out_idx;                       // the ray's plane entry
    unsigned int* count;                     // how many (zeroed by the host)
    // answer kernel
    uint32_t n_traced;
    const float* ans;                        // the rays' answers, as res
    uint32_t ans_stride;
    // resolve kernel
    float4* acc;                             // [nslots][kAovDirectAccRows]: (direct.xyz, bits(traced)), (unshadowed.xyz, bits(lit)), (sum of squares.xyz, -),
                                             // (Ld.xyz of the sample in progress, -), (U.xyz of the sample in progress, -)
    uint32_t first_batch, last_batch;        // of the call: the first starts the sums, the last writes the outputs
    float* direct;                           // outputs (any may be null): row-major W x H, or nslots with tiled_output
    float* unshadowed;
    float* direct_variance;
    float* visibility;
};

// Next-event sample q of a vertex at depth `depth`, as a function of values: the ray's unit direction and limit and the contribution.
// The twin of setup_shadow_lg (crt_path.h), which states the same arithmetic on k_mega3's lane state -- Render.cuh:262-272 and :274-283,
// operation for operation; the test of the pass against the frame at p_rr = 0 (tests/test_aov_direct.py) pins the two together.
// lg = lights[q / lsn]; the draw index is q itself.
struct NeeSample {
    F3 rd, c;
    float tl;
};
__device__ __forceinline__ NeeSample nee_sample(const uint64_t seed, const uint32_t pixel_index, const uint32_t k, const uint32_t depth, const uint32_t q, const uint4 lg,
                                                const float4* ltri, const F3 pos, const F3 nrm, const F3 f_r, const int32_t lsn, const float inv_lsn_pow2)
{
    const U4 rl = rng_draw(seed, pixel_index, k, depth, RNG_NEE, q);
    const uint32_t ti = rl.x - fast_div(rl.x, lg.z, lg.w) * lg.y; // rand % triangle count (DeviceLights.cuh:35)
    const float4* lt = ltri + (size_t)(lg.x + ti) * 4;
    const float4 l0 = lt[0], l1 = lt[1], l2 = lt[2], l3 = lt[3];
    const float alpha = rng_uniform(rl.y); // DeviceTriangle.cuh:69-71
    const float beta = rng_uniform(rl.z) * (1 - alpha);
    const float gamma = 1 - alpha - beta;
    const F3 lv1 = f3(l0.x, l0.y, l0.z), lv2 = f3(l0.w, l1.x, l1.y), lv3 = f3(l1.z, l1.w, l2.x);
    const F3 lpos = add3(add3(scalel3(alpha, lv1), scalel3(beta, lv2)), scalel3(gamma, lv3));
    const F3 dist = sub3(lpos, pos);
    const F3 dir = unit3(dist);
    NeeSample s;
    s.rd = unit3(dir);     // Ray normalises again (Ray.cuh:13)
    s.tl = dist.x / dir.x; // Render.cuh:272
    const float tl = norm3(dist);
    const float t2 = tl * tl;
    float cos_theta = dot3(dir, nrm);
    float cos_theta_2 = -dot3(dir, f3(l2.y, l2.z, l2.w));
    cos_theta = cos_theta > 0.0f ? cos_theta : 0.0f;
    cos_theta_2 = cos_theta_2 > 0.0f ? cos_theta_2 : 0.0f;
    // ((((Le*fr)*cos)*cos2)*inv_pdf)/t2)/lsn  (Render.cuh:283)
    F3 c = mul3(f3(l3.x, l3.y, l3.z), f_r);
    c = scale3(c, cos_theta);
    c = scale3(c, cos_theta_2);
    c = scale3(c, l3.w);
    c = div3(c, t2);
    if (inv_lsn_pow2 != 0.0f) c = scale3(c, inv_lsn_pow2); // == c / lsn bit for bit (LParams)
    else c = div3(c, (float)lsn);
    s.c = c;
    return s;
}

// ---- vertex: item = sample of the chunk x nslots + slot ----
__device__ __forceinline__ void aov_direct_vertex(const AovDirectParams& D, const uint64_t item)
{
    const uint32_t s = (uint32_t)(item / D.nslots), slot = (uint32_t)(item - (uint64_t)s * D.nslots);
    const float* r = D.res + (size_t)item * D.res_stride;
    const float t = r[0];
    int32_t tri = __float_as_int(r[1]);
    F3 pos = f3(0.0f, 0.0f, 0.0f);
    if (tri >= 0 && slot_pixel(D, slot).valid && !TNM_EMITTER(__float_as_uint(D.tri_nm[tri].w))) {
        const float4 o = D.cam_ro[item], d = D.cam_rd[item];
        pos = add3(f3(o.x, o.y, o.z), scalel3(t, f3(d.x, d.y, d.z))); // DeviceTriangle.cuh:50, as logic_A forms it
    } else tri = -1;
    D.vert[item] = make_float4(pos.x, pos.y, pos.z, __int_as_float(tri));
}

// ---- set-up: a wave takes kAovDirectWaveEntries consecutive entries of the sub-batch (group g: entries g x 8 .. g x 8 + 7) for 64
// consecutive slots; thread i = group i / nslots, slot i % nslots (nslots is a multiple of 64: a wave lies in one group).  Every lane of the
// wave runs it, in range or not (the ballots).  The rays of its entries wait in registers until the wave knows how many there are: ONE
// atomic per wave on the one counter, whose atomics serialise at the memory side -- with one entry per wave they were half of the pass.
__device__ __forceinline__ void aov_direct_setup(const AovDirectParams& D, const uint32_t i, const uint32_t group_of_wave)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t slot = i - group_of_wave * D.nslots;
    const SlotPixel px = slot_pixel(D, slot);
    float rdx[kAovDirectWaveEntries], rdy[kAovDirectWaveEntries], rdz[kAovDirectWaveEntries], tl[kAovDirectWaveEntries];
    uint32_t off[kAovDirectWaveEntries];
    uint32_t total = 0, mine = 0; // rays of the wave so far; bit k: this lane's entry k is traced
#pragma unroll
    for (uint32_t k = 0; k < kAovDirectWaveEntries; k++) {
        const uint32_t entry = group_of_wave * kAovDirectWaveEntries + k;
        bool traced = false;
        rdx[k] = rdy[k] = rdz[k] = tl[k] = 0.0f;
        if (entry < D.e_count) {
            const uint32_t e = D.q_first + entry, ds = e / D.n_q;
            const uint32_t s = D.s_first + ds, q = e - ds * D.n_q;
            const uint4 lg = D.lights[fast_div(q, D.lsn_div.m, D.lsn_div.sh)]; // (the same in every lane)
            const float4 v = D.vert[(size_t)s * D.nslots + slot];
            const int32_t tri = __float_as_int(v.w);
            F3 c = f3(0.0f, 0.0f, 0.0f);
            if (tri >= 0) {
                const float4 tn = D.tri_nm[tri];
                const float4 m0 = D.mats[(size_t)TNM_MAT(__float_as_uint(tn.w)) * 3];
                const NeeSample ns = nee_sample(D.seed, px.j * D.width + px.i, D.sample_begin + s, 0u, q, lg, D.ltri, f3(v.x, v.y, v.z), f3(tn.x, tn.y, tn.z),
                                                f3(m0.x, m0.y, m0.z), D.lsn, D.inv_lsn_pow2);
                c = ns.c;
                rdx[k] = ns.rd.x; rdy[k] = ns.rd.y; rdz[k] = ns.rd.z; tl[k] = ns.tl;
                traced = !(c.x == 0.0f && c.y == 0.0f && c.z == 0.0f); // logic_A's rule: a NaN contribution is traced
            }
            D.plane[(size_t)entry * D.nslots + slot] = make_float4(c.x, c.y, c.z, __uint_as_float(traced ? (uint32_t)(AOVD_TRACED | AOVD_BLOCKED) : 0u));
        }
        const unsigned long long mask = __ballot(traced);
        off[k] = total + (uint32_t)__popcll(mask & below);
        total += (uint32_t)__popcll(mask);
        mine |= traced ? 1u << k : 0u;
    }
    if (total == 0u) return; // (the same in every lane)
    // the traced rays, compacted: a popcount of the ballots and ONE atomic per wave, as k_aov_bounce
    unsigned int base = 0;
    if (lane == 0) base = __hip_atomic_fetch_add(D.count, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = (unsigned int)__builtin_amdgcn_readlane((int)base, 0);
#pragma unroll
    for (uint32_t k = 0; k < kAovDirectWaveEntries; k++) {
        if (!(mine & (1u << k))) continue;
        const uint32_t entry = group_of_wave * kAovDirectWaveEntries + k;
        const float4 v = D.vert[(size_t)(D.s_first + (D.q_first + entry) / D.n_q) * D.nslots + slot]; // (the ray leaves the vertex)
        const uint32_t j = base + off[k]; // (j < e_count * nslots: at most every entry is traced)
        D.out_ro[j] = make_float4(v.x, v.y, v.z, tl[k]);
        D.out_rd[j] = make_float4(rdx[k], rdy[k], rdz[k], __uint_as_float((uint32_t)RAY_SHADOW));
        D.out_res[j] = make_float2(FLT_MAX, __int_as_float(-1));
        D.out_idx[j] = entry * D.nslots + slot;
    }
}

// ---- answer: traced ray j ----
__device__ __forceinline__ void aov_direct_answer(const AovDirectParams& D, const uint32_t j)
{
    const float* a = D.ans + (size_t)j * D.ans_stride;
    const float tl = D.out_ro[j].w, T = a[0];
    const int32_t tri = __float_as_int(a[1]);
    const bool blocked = D.reference_mode ? shadow_blocked<1>(tl, T, tri) : shadow_blocked<0>(tl, T, tri);
    if (!blocked) D.plane[D.out_idx[j]].w = __uint_as_float((uint32_t)AOVD_TRACED);
}

// ---- resolve: the sub-batch's entries of a slot, in order ----
__device__ __forceinline__ void aov_direct_resolve(const AovDirectParams& D, const uint32_t slot)
{
    const SlotPixel px = slot_pixel(D, slot);
    if (!px.valid && (!px.out || !D.last_batch)) return;
    F3 dsum = f3(0.0f, 0.0f, 0.0f), usum = dsum, qsum = dsum, Ld = dsum, U = dsum;
    uint32_t traced = 0, lit = 0;
    if (px.valid) {
        float4* acc = D.acc + (size_t)slot * kAovDirectAccRows;
        if (!D.first_batch) {
            const float4 a0 = acc[0], a1 = acc[1], a2 = acc[2], a3 = acc[3], a4 = acc[4];
            dsum = f3(a0.x, a0.y, a0.z); traced = __float_as_uint(a0.w);
            usum = f3(a1.x, a1.y, a1.z); lit = __float_as_uint(a1.w);
            qsum = f3(a2.x, a2.y, a2.z);
            Ld = f3(a3.x, a3.y, a3.z); U = f3(a4.x, a4.y, a4.z);
        }
        const float fspp = (float)D.spp;
        uint32_t q = D.q_first;
        const float4* pl = D.plane + slot;
        for (uint32_t e = 0; e < D.e_count; e++, pl += D.nslots) {
            if (q == 0u) { Ld = f3(0.0f, 0.0f, 0.0f); U = Ld; }
            const float4 c = *pl;
            const uint32_t fl = __float_as_uint(c.w);
            if (fl & AOVD_TRACED) {
                U = add3(U, f3(c.x, c.y, c.z));
                traced++;
                if (!(fl & AOVD_BLOCKED)) { Ld = add3(Ld, f3(c.x, c.y, c.z)); lit++; }
            }
            if (++q == D.n_q) { // the sample is complete
                q = 0u;
                const float xx = Ld.x / fspp, xy = Ld.y / fspp, xz = Ld.z / fspp;
                dsum = f3(dsum.x + xx, dsum.y + xy, dsum.z + xz);
                qsum = f3(qsum.x + xx * xx, qsum.y + xy * xy, qsum.z + xz * xz);
                usum = f3(usum.x + U.x / fspp, usum.y + U.y / fspp, usum.z + U.z / fspp);
            }
        }
        if (!D.last_batch) {
            acc[0] = make_float4(dsum.x, dsum.y, dsum.z, __uint_as_float(traced));
            acc[1] = make_float4(usum.x, usum.y, usum.z, __uint_as_float(lit));
            acc[2] = make_float4(qsum.x, qsum.y, qsum.z, 0.0f);
            acc[3] = make_float4(Ld.x, Ld.y, Ld.z, 0.0f);
            acc[4] = make_float4(U.x, U.y, U.z, 0.0f);
            return;
        }
    }
    const size_t o = px.o;
    if (D.direct) { D.direct[o * 3 + 0] = dsum.x; D.direct[o * 3 + 1] = dsum.y; D.direct[o * 3 + 2] = dsum.z; }
    if (D.unshadowed) { D.unshadowed[o * 3 + 0] = usum.x; D.unshadowed[o * 3 + 1] = usum.y; D.unshadowed[o * 3 + 2] = usum.z; }
    if (D.direct_variance) {
        // crt_variance's statistic over all spp samples (fn = fs = spp, so (fs / fn)^2 = 1); one sample has no variance: +0
        F3 v = f3(0.0f, 0.0f, 0.0f);
        if (px.valid && D.spp > 1u) v = variance_of3(dsum, qsum, (float)D.spp, 1.0f);
        D.direct_variance[o * 3 + 0] = v.x; D.direct_variance[o * 3 + 1] = v.y; D.direct_variance[o * 3 + 2] = v.z;
    }
    if (D.visibility) D.visibility[o] = px.valid ? (traced ? (float)lit / (float)traced : 1.0f) : 0.0f;
}

// ---- the launches (crt_aov_direct.hip), enqueued on st ----
void launch_aov_direct_vertex(const AovDirectParams& D, hipStream_t st);
void launch_aov_direct_setup(const AovDirectParams& D, hipStream_t st);
void launch_aov_direct_answer(const AovDirectParams& D, hipStream_t st);
void launch_aov_direct_resolve(const AovDirectParams& D, hipStream_t st);

} // namespace crtk
#endif
