// cudaraytracing_amd/csrc/crt_aov.hip -- the first-hit AOV pass (crt_render_aov, include/crt.h): per pixel, the camera rays of samples
// 0 .. spp-1 -- the primary rays of the frame's paths, camera_dir -- traced by the render kernel's own closest-hit query, and the albedo,
// normal, depth, coverage, triangle and material buffers made of their hits in sample order.  The host side (chunks over samples, the
// trace) is in crt_aov_pass.hip; slot -> pixel -> output index is the frame kernels' (slot_pixel, crt_internal.h).  The same pass with the
// emission and non-emitter albedo buffers beside them (crt_render_aov_shading) is the resolve's second instantiation.
// Below it, the pass that follows perfect-mirror bounces from those hits (crt_render_aov_specular): a bounce kernel and its own resolve.
#include "crt_internal.h"

namespace crtk {

// The query rays of one chunk, in the form k_fill_rays writes them (limit 0, RAY_CLOSEST, result primed as a miss): item = sample offset
// x nslots + slot.  The direction is the camera ray's unit direction (unit3 of camera_dir, as the render kernels make it); the trace does
// not normalise it again.  A padding slot (ragged tile, a tile beyond the image) traces the camera's forward axis; its result is never read.
__global__ __launch_bounds__(256) void k_aov_rays(const AovParams A)
{
    const uint64_t item = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (item >= (uint64_t)A.n_samples * A.nslots) return;
    const uint32_t s = (uint32_t)(item / A.nslots), slot = (uint32_t)(item - (uint64_t)s * A.nslots);
    const SlotPixel px = slot_pixel(A, slot);
    const F3 d = unit3(px.valid ? camera_dir(A, px.j * A.width + px.i, A.sample_begin + s, px.i, px.j) : f3(A.inv_view[6], A.inv_view[7], A.inv_view[8])); // Ray.cuh:13
    A.pool.ro[item] = make_float4(A.eye[0], A.eye[1], A.eye[2], 0.0f);
    A.pool.rd[item] = make_float4(d.x, d.y, d.z, __uint_as_float((uint32_t)RAY_CLOSEST));
    A.pool.res[item] = make_float2(FLT_MAX, __int_as_float(-1));
}

// One thread per pixel slot: the chunk's samples in order, each hit adding kd / spp, normal / spp and t to the running sums (IEEE
// division and addition, no contraction: k_accumulate's c + L / spp), carried to the next chunk in A.acc.  The last chunk writes the
// outputs.
// SHADING (crt_render_aov_shading): the same trace also feeds two more sums -- ke / spp over the hits on emitters (TNM_EMITTER: the
// flag the render kernel ends a path on) and kd / spp over the others; ke is row 2 of the material whose row 1 the hit has fetched.
// They cross chunks in the two spare floats of accumulator row 2 and a fourth row, so a slot then has four rows, not three.
// The plain instantiation takes H and never reads it; its listing must stay the untemplated kernel's, instruction for instruction
// (crt_render_aov's bits and time do not depend on the shading form: docs/experiments.md, "Albedo demodulation").
template <bool SHADING> __global__ __launch_bounds__(256) void k_aov_resolve(const AovParams A, const AovShadingOut H)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= A.nslots) return;
    const SlotPixel px = slot_pixel(A, slot);
    if (!px.valid && (!px.out || !A.last_chunk)) return;
    F3 alb = f3(0.0f, 0.0f, 0.0f), nrm = f3(0.0f, 0.0f, 0.0f);
    F3 emi = f3(0.0f, 0.0f, 0.0f), dal = f3(0.0f, 0.0f, 0.0f);
    float dsum = 0.0f;
    uint32_t hits = 0;
    int32_t tri0 = -1, mat0 = -1;
    if (px.valid) {
        float4* acc = A.acc + (size_t)slot * (SHADING ? 4 : 3);
        if (!A.first_chunk) {
            const float4 a0 = acc[0], a1 = acc[1], a2 = acc[2];
            alb = f3(a0.x, a0.y, a0.z); dsum = a0.w;
            nrm = f3(a1.x, a1.y, a1.z); hits = __float_as_uint(a1.w);
            tri0 = __float_as_int(a2.x); mat0 = __float_as_int(a2.y);
            if (SHADING) {
                const float4 a3 = acc[3];
                emi = f3(a2.z, a2.w, a3.x); dal = f3(a3.y, a3.z, a3.w);
            }
        }
        const float fspp = (float)A.spp;
        for (uint32_t s = 0; s < A.n_samples; s++) {
            const float* r = A.res + ((size_t)s * A.nslots + slot) * A.res_stride;
            const float t = r[0];
            const int32_t tri = __float_as_int(r[1]);
            int32_t m = -1;
            if (tri >= 0) {
                const float4 tn = A.tri_nm[tri];
                m = (int32_t)TNM_MAT(__float_as_uint(tn.w));
                const float4 kd = A.mats[(size_t)m * 3 + 1];
                alb.x = alb.x + kd.x / fspp; alb.y = alb.y + kd.y / fspp; alb.z = alb.z + kd.z / fspp;
                nrm.x = nrm.x + tn.x / fspp; nrm.y = nrm.y + tn.y / fspp; nrm.z = nrm.z + tn.z / fspp;
                dsum = dsum + t;
                hits++;
                if (SHADING) {
                    if (TNM_EMITTER(__float_as_uint(tn.w))) {
                        const float4 ke = A.mats[(size_t)m * 3 + 2];
                        emi.x = emi.x + ke.x / fspp; emi.y = emi.y + ke.y / fspp; emi.z = emi.z + ke.z / fspp;
                    } else {
                        dal.x = dal.x + kd.x / fspp; dal.y = dal.y + kd.y / fspp; dal.z = dal.z + kd.z / fspp;
                    }
                }
            }
            if (A.first_chunk && s == 0) { tri0 = tri >= 0 ? tri : -1; mat0 = m; }
        }
        if (!A.last_chunk) {
            acc[0] = make_float4(alb.x, alb.y, alb.z, dsum);
            acc[1] = make_float4(nrm.x, nrm.y, nrm.z, __uint_as_float(hits));
            if (SHADING) {
                acc[2] = make_float4(__int_as_float(tri0), __int_as_float(mat0), emi.x, emi.y);
                acc[3] = make_float4(emi.z, dal.x, dal.y, dal.z);
            } else {
                acc[2] = make_float4(__int_as_float(tri0), __int_as_float(mat0), 0.0f, 0.0f);
            }
            return;
        }
    }
    const size_t o = px.o;
    if (A.albedo) { A.albedo[o * 3 + 0] = alb.x; A.albedo[o * 3 + 1] = alb.y; A.albedo[o * 3 + 2] = alb.z; }
    if (A.normal) { A.normal[o * 3 + 0] = nrm.x; A.normal[o * 3 + 1] = nrm.y; A.normal[o * 3 + 2] = nrm.z; }
    if (A.depth) A.depth[o] = hits ? dsum / (float)hits : 0.0f;
    if (A.coverage) A.coverage[o] = (float)hits / (float)A.spp;
    if (A.tri) A.tri[o] = tri0;
    if (A.material) A.material[o] = mat0;
    if (SHADING) {
        if (H.emission) { H.emission[o * 3 + 0] = emi.x; H.emission[o * 3 + 1] = emi.y; H.emission[o * 3 + 2] = emi.z; }
        if (H.diffuse_albedo) { H.diffuse_albedo[o * 3 + 0] = dal.x; H.diffuse_albedo[o * 3 + 1] = dal.y; H.diffuse_albedo[o * 3 + 2] = dal.z; }
    }
}

// ---- the pass that follows mirror bounces (crt_render_aov_specular, include/crt.h) ----

// One thread per ray traced last, a wave on 64 consecutive rays.  The hit adds its distance to the chain's length; at a SPECULAR
// triangle below the bounce cap the chain goes on: the throughput takes kd, and the reflected ray (origin P = o + d t, direction
// unit3(d - n (c + c)), the arithmetic of the contract, no contraction) goes to the other half of the query pool, primed as k_aov_rays
// primes a ray, with its item beside it -- at count + the rank among the wave's rays that go on: a ballot, a popcount and ONE atomic per
// wave, as k_adaptive_select.  The order of the compacted rays is whatever the atomics make it; the next stage finds the item by the
// index stored with the ray, so the order decides where a ray is traced and never what an item holds.
__global__ __launch_bounds__(256) void k_aov_bounce(const AovSpecParams S)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool go = false;
    uint32_t item = 0;
    F3 P = f3(0.0f, 0.0f, 0.0f), r = P;
    if (i < S.n_in) {
        item = S.stage0 ? i : S.in_item[i];
        const float* a = S.res + (size_t)i * S.res_stride;
        const float t = a[0];
        const int32_t tri = __float_as_int(a[1]);
        float4 st = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        int2 ax = make_int2(-1, 0);
        if (!S.stage0) { st = S.state[item]; ax = S.aux[item]; }
        ax.x = tri >= 0 ? tri : -1;
        if (tri >= 0) {
            st.w = st.w + t;
            const float4 tn = S.tri_nm[tri];
            const uint32_t w = __float_as_uint(tn.w);
            go = TNM_SPECULAR(w) != 0u && (uint32_t)ax.y < S.max_bounces;
            if (go && S.stage0) go = slot_pixel(S, i - (i / S.nslots) * S.nslots).valid; // (a padding slot's ray is never read: it does not go on)
            if (go) {
                const float4 kd = S.mats[(size_t)TNM_MAT(w) * 3 + 1];
                if (ax.y == 0) { st.x = kd.x; st.y = kd.y; st.z = kd.z; }
                else { st.x = st.x * kd.x; st.y = st.y * kd.y; st.z = st.z * kd.z; }
                const float4 o4 = S.in_ro[i], d4 = S.in_rd[i];
                const F3 o = f3(o4.x, o4.y, o4.z), d = f3(d4.x, d4.y, d4.z), n = f3(tn.x, tn.y, tn.z);
                P = add3(o, scale3(d, t));
                const float c = dot3(d, n), c2 = c + c;
                r = unit3(sub3(d, scale3(n, c2))); // Ray.cuh:13
                ax.y = ax.y + 1;
            }
        }
        S.state[item] = st;
        S.aux[item] = ax;
    }
    const unsigned long long mask = __ballot(go);
    if (mask == 0ull) return;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)mask) - 1;
    unsigned int base = 0;
    if (lane == leader) base = __hip_atomic_fetch_add(S.count, (unsigned int)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = (unsigned int)__builtin_amdgcn_readlane((int)base, leader);
    if (go) {
        const uint32_t j = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)); // (j < n_in: at most every ray goes on)
        S.out_ro[j] = make_float4(P.x, P.y, P.z, 0.0f);
        S.out_rd[j] = make_float4(r.x, r.y, r.z, __uint_as_float((uint32_t)RAY_CLOSEST));
        S.out_res[j] = make_float2(FLT_MAX, __int_as_float(-1));
        S.out_item[j] = item;
    }
}

// One thread per pixel slot, as k_aov_resolve: the chunk's samples in order, each finished chain adding G / spp, N / spp, D and B to the
// running sums (carried to the next chunk in S.acc); the last chunk writes the outputs.
__global__ __launch_bounds__(256) void k_aov_spec_resolve(const AovSpecParams S)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= S.nslots) return;
    const SlotPixel px = slot_pixel(S, slot);
    if (!px.valid && (!px.out || !S.last_chunk)) return;
    F3 alb = f3(0.0f, 0.0f, 0.0f), nrm = f3(0.0f, 0.0f, 0.0f);
    float dsum = 0.0f, bsum = 0.0f;
    uint32_t hits = 0;
    int32_t tri0 = -1;
    if (px.valid) {
        float4* acc = S.acc + (size_t)slot * 3;
        if (!S.first_chunk) {
            const float4 a0 = acc[0], a1 = acc[1], a2 = acc[2];
            alb = f3(a0.x, a0.y, a0.z); dsum = a0.w;
            nrm = f3(a1.x, a1.y, a1.z); hits = __float_as_uint(a1.w);
            bsum = a2.x; tri0 = __float_as_int(a2.y);
        }
        const float fspp = (float)S.spp;
        for (uint32_t s = 0; s < S.n_samples; s++) {
            const size_t item = (size_t)s * S.nslots + slot;
            const float4 st = S.state[item];
            const int2 ax = S.aux[item];
            if (S.first_chunk && s == 0) tri0 = ax.x >= 0 ? ax.x : -1;
            if (ax.x < 0 && ax.y == 0) continue; // the camera ray missed
            dsum = dsum + st.w;
            bsum = bsum + (float)ax.y;
            hits++;
            if (ax.x < 0) continue; // the chain ended at a miss: no G, no N
            const float4 tn = S.tri_nm[ax.x];
            const size_t m = TNM_MAT(__float_as_uint(tn.w));
            const float4 kd = S.mats[m * 3 + 1];
            F3 g = f3(kd.x, kd.y, kd.z);
            if (ax.y != 0) {
                const float4 ke = S.mats[m * 3 + 2];
                const F3 e = f3(ke.x < 1.0f ? ke.x : 1.0f, ke.y < 1.0f ? ke.y : 1.0f, ke.z < 1.0f ? ke.z : 1.0f);
                g = mul3(f3(st.x, st.y, st.z), add3(g, e));
            }
            alb.x = alb.x + g.x / fspp; alb.y = alb.y + g.y / fspp; alb.z = alb.z + g.z / fspp;
            nrm.x = nrm.x + tn.x / fspp; nrm.y = nrm.y + tn.y / fspp; nrm.z = nrm.z + tn.z / fspp;
        }
        if (!S.last_chunk) {
            acc[0] = make_float4(alb.x, alb.y, alb.z, dsum);
            acc[1] = make_float4(nrm.x, nrm.y, nrm.z, __uint_as_float(hits));
            acc[2] = make_float4(bsum, __int_as_float(tri0), 0.0f, 0.0f);
            return;
        }
    }
    const size_t o = px.o;
    if (S.guide_albedo) { S.guide_albedo[o * 3 + 0] = alb.x; S.guide_albedo[o * 3 + 1] = alb.y; S.guide_albedo[o * 3 + 2] = alb.z; }
    if (S.last_normal) { S.last_normal[o * 3 + 0] = nrm.x; S.last_normal[o * 3 + 1] = nrm.y; S.last_normal[o * 3 + 2] = nrm.z; }
    if (S.path_depth) S.path_depth[o] = hits ? dsum / (float)hits : 0.0f;
    if (S.bounces) S.bounces[o] = hits ? bsum / (float)hits : 0.0f;
    if (S.last_tri) S.last_tri[o] = tri0;
}

// ---- exported to crt_aov_pass.hip ----
void launch_aov_bounce(const AovSpecParams& S, hipStream_t st) { hipLaunchKernelGGL(k_aov_bounce, dim3((S.n_in + 255) / 256), dim3(256), 0, st, S); }
void launch_aov_spec_resolve(const AovSpecParams& S, hipStream_t st) { hipLaunchKernelGGL(k_aov_spec_resolve, dim3((S.nslots + 255) / 256), dim3(256), 0, st, S); }
void launch_aov_rays(const AovParams& A, hipStream_t st)
{
    const uint64_t n = (uint64_t)A.n_samples * A.nslots;
    hipLaunchKernelGGL(k_aov_rays, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, A);
}
void launch_aov_resolve(const AovParams& A, hipStream_t st) { hipLaunchKernelGGL(k_aov_resolve<false>, dim3((A.nslots + 255) / 256), dim3(256), 0, st, A, AovShadingOut{nullptr, nullptr}); }
void launch_aov_resolve_shading(const AovParams& A, const AovShadingOut& H, hipStream_t st)
{
    hipLaunchKernelGGL(k_aov_resolve<true>, dim3((A.nslots + 255) / 256), dim3(256), 0, st, A, H);
}

} // namespace crtk
