// cudaraytracing_amd/csrc/crt_aov_ao.h -- the per-thread text of the ambient-occlusion AOV pass (crt_render_aov_ao, contract:
// include/crt.h; kernels: crt_aov_ao.hip; host side: crt_aov_pass.hip).  Per camera ray of a chunk the pass sends ao_samples occlusion
// rays of at most max_distance over the hemisphere of the hit's facing normal -- the draws (seed, pixel, k, 0, RNG_AO, q), the
// directions the path's own bounce_dir -- and folds their answers into the ao, openness and bent_normal buffers.  Three stages around
// the trace:
//   vertex   one thread per camera ray: (pos, valid) and the facing normal nf of the first hit, copied out of the camera answers before
//            the first occlusion trace overwrites them.  A ray without a vertex (a miss, a padding slot) keeps its own origin and
//            direction there: its entries still need a ray, because nothing is compacted
//   set-up   one thread per (sample, q, slot) entry of a sub-batch: the entry's direction and cosine into the entry plane, its ray into
//            the second region of the query pool AT THE ENTRY'S OWN INDEX (every ray is traced: no counter, nothing for the host to read)
//   resolve  one thread per slot: walks the sub-batch's entries and their answers in order into the running sums of the slot's
//            accumulator rows; the call's last sub-batch writes the outputs
// A sub-batch is a range of the chunk's linear (sample, q) order and may begin and end inside a sample: the sums run over (k, q) in one
// order, so nothing but the accumulator rows crosses its borders.
// Like crt_aov_direct.h this file includes nothing, so that tools/aov_ao_host_check.cpp can compile this very text for the host behind
// tools/host_device.h's stand-ins for what it takes from outside: SlotMap / slot_pixel (crt_stages.h), F3 and its operations
// (crt_device.h), rng_draw, RNG_AO (crt_detmath.h), bounce_dir, shadow_blocked, RAY_SHADOW (crt_path.h).  No cross-lane operation.
#ifndef CRT_AOV_AO_H
#define CRT_AOV_AO_H

namespace crtk {

const uint32_t kAovAoAccRows = 2; // float4 rows of a slot's running sums (AovAoParams::acc)
#define AOVAO_NO_VERTEX (-1.0f)   /* the cosine of a plane entry whose camera ray has no vertex (a real cosine is max(.., 0): never negative) */

struct AovAoParams : SlotMap {
    uint64_t seed;
    uint32_t spp, sample_begin, n_samples;   // the chunk: samples [sample_begin, sample_begin + n_samples) of every slot
    uint32_t n_q;                            // occlusion rays per vertex: crt_aov_ao_params::ao_samples
    float max_distance;                      // their limit
    uint32_t reference_mode;                 // CRT_TRAVERSAL_REFERENCE: blocked() compares the limit with the closest hit's distance
    const float4* tri_nm;                    // scene: normal.xyz, bits(material word) per triangle
    // vertex kernel: the camera rays (item = sample of the chunk x nslots + slot) and their answers
    const float4* cam_ro;
    const float4* cam_rd;
    const float* res;                        // (t, bits(triangle or -1)) of item i at res[i * res_stride]
    uint32_t res_stride;
    float4* vert;                            // per item: pos.xyz, bits(1: a vertex, 0: none -- then the camera ray's origin)
    float4* vnf;                             // per item: nf.xyz (no vertex: the camera ray's direction), -
    // the sub-batch: e_count entries of the chunk's linear order (sample of the chunk x n_q + q), from (s_first, q_first) on
    uint32_t s_first, q_first, e_count;
    float4* plane;                           // [e_count][nslots]: dir.xyz, w (AOVAO_NO_VERTEX: no vertex)
    // set-up kernel: the ray of entry i = entry x nslots + slot at index i, in the form k_fill_rays writes a visibility ray
    float4* out_ro;                          // origin.xyz, limit
    float4* out_rd;                          // unit direction.xyz, bits(RAY_SHADOW)
    float2* out_res;
    // resolve kernel
    const float* ans;                        // the rays' answers, as res: entry i at ans[i * ans_stride]
    uint32_t ans_stride;
    float4* acc;                             // [nslots][kAovAoAccRows]: (A, V, bits(rays), bits(open)), (b.xyz, -)
    uint32_t first_batch, last_batch;        // of the call: the first starts the sums, the last writes the outputs
    unsigned long long* ray_total;           // the call's occlusion rays, summed by the last sub-batch (crt_aov_ao.hip; zeroed by the host)
    float* ao;                               // outputs (any may be null): row-major W x H, or nslots with tiled_output
    float* openness;
    float* bent_normal;
};

// ---- vertex: item = sample of the chunk x nslots + slot ----
__device__ __forceinline__ void aov_ao_vertex(const AovAoParams& D, const uint64_t item)
{
    const uint32_t s = (uint32_t)(item / D.nslots), slot = (uint32_t)(item - (uint64_t)s * D.nslots);
    const float* r = D.res + (size_t)item * D.res_stride;
    const float t = r[0];
    const int32_t tri = __float_as_int(r[1]);
    const float4 o = D.cam_ro[item], d = D.cam_rd[item];
    F3 pos = f3(o.x, o.y, o.z), nf = f3(d.x, d.y, d.z);
    uint32_t vertex = 0u;
    if (tri >= 0 && slot_pixel(D, slot).valid) {
        pos = add3(pos, scalel3(t, nf)); // DeviceTriangle.cuh:50, as logic_A forms it
        const float4 tn = D.tri_nm[tri];
        const F3 n = f3(tn.x, tn.y, tn.z);
        nf = dot3(nf, n) > 0.0f ? f3(-n.x, -n.y, -n.z) : n; // (a NaN dot keeps n)
        vertex = 1u;
    }
    D.vert[item] = make_float4(pos.x, pos.y, pos.z, __uint_as_float(vertex));
    D.vnf[item] = make_float4(nf.x, nf.y, nf.z, 0.0f);
}

// ---- set-up: i = entry x nslots + slot of the sub-batch; `entry` = i / nslots (the same in every lane of a wave: nslots is a multiple of 64) ----
__device__ __forceinline__ void aov_ao_setup(const AovAoParams& D, const uint32_t i, const uint32_t entry)
{
    const uint32_t slot = i - entry * D.nslots;
    const uint32_t e = D.q_first + entry, ds = e / D.n_q;
    const uint32_t s = D.s_first + ds, q = e - ds * D.n_q;
    const size_t item = (size_t)s * D.nslots + slot;
    const float4 v = D.vert[item], n4 = D.vnf[item];
    F3 dir = f3(n4.x, n4.y, n4.z); // (no vertex: the camera ray again, from its origin; its answer is never read)
    float4 pl = make_float4(0.0f, 0.0f, 0.0f, AOVAO_NO_VERTEX);
    if (__float_as_uint(v.w) != 0u) {
        const SlotPixel px = slot_pixel(D, slot);
        const F3 nf = dir;
        dir = bounce_dir(nf, rng_draw(D.seed, px.j * D.width + px.i, D.sample_begin + s, 0u, RNG_AO, q));
        float w = dot3(dir, nf);
        w = w > 0.0f ? w : 0.0f; // (a NaN: 0)
        pl = make_float4(dir.x, dir.y, dir.z, w);
    }
    D.plane[i] = pl;
    D.out_ro[i] = make_float4(v.x, v.y, v.z, D.max_distance);
    D.out_rd[i] = make_float4(dir.x, dir.y, dir.z, __uint_as_float((uint32_t)RAY_SHADOW));
    D.out_res[i] = make_float2(FLT_MAX, __int_as_float(-1));
}

// ---- resolve: the sub-batch's entries of a slot, in order.  Returns the slot's occlusion rays when the call ends here, else 0 ----
__device__ __forceinline__ uint32_t aov_ao_resolve(const AovAoParams& D, const uint32_t slot)
{
    const SlotPixel px = slot_pixel(D, slot);
    if (!px.valid && (!px.out || !D.last_batch)) return 0u;
    float A = 0.0f, V = 0.0f;
    F3 b = f3(0.0f, 0.0f, 0.0f);
    uint32_t rays = 0, open = 0;
    if (px.valid) {
        float4* acc = D.acc + (size_t)slot * kAovAoAccRows;
        if (!D.first_batch) {
            const float4 a0 = acc[0], a1 = acc[1];
            A = a0.x; V = a0.y; rays = __float_as_uint(a0.z); open = __float_as_uint(a0.w);
            b = f3(a1.x, a1.y, a1.z);
        }
        size_t i = slot;
        for (uint32_t e = 0; e < D.e_count; e++, i += D.nslots) {
            const float4 c = D.plane[i];
            if (c.w < 0.0f) continue; // AOVAO_NO_VERTEX
            rays++;
            A = A + c.w;
            const float* a = D.ans + i * D.ans_stride;
            const float T = a[0];
            const int32_t tri = __float_as_int(a[1]);
            const bool blocked = D.reference_mode ? shadow_blocked<1>(D.max_distance, T, tri) : shadow_blocked<0>(D.max_distance, T, tri);
            if (!blocked) {
                V = V + c.w;
                open++;
                b = add3(b, f3(c.x, c.y, c.z));
            }
        }
        if (!D.last_batch) {
            acc[0] = make_float4(A, V, __uint_as_float(rays), __uint_as_float(open));
            acc[1] = make_float4(b.x, b.y, b.z, 0.0f);
            return 0u;
        }
    }
    // a padding slot of a tiled output: nothing around it is known to be closed -- ao and openness 1.0f as at a pixel that only misses,
    // bent_normal +0
    const size_t o = px.o;
    if (D.ao) D.ao[o] = A == 0.0f ? 1.0f : V / A;
    if (D.openness) D.openness[o] = rays ? (float)open / (float)rays : 1.0f;
    if (D.bent_normal) {
        const F3 u = open ? unit3(b) : f3(0.0f, 0.0f, 0.0f);
        D.bent_normal[o * 3 + 0] = u.x; D.bent_normal[o * 3 + 1] = u.y; D.bent_normal[o * 3 + 2] = u.z;
    }
    return rays;
}

// ---- the launches (crt_aov_ao.hip), enqueued on st ----
void launch_aov_ao_vertex(const AovAoParams& D, hipStream_t st);
void launch_aov_ao_setup(const AovAoParams& D, hipStream_t st);
void launch_aov_ao_resolve(const AovAoParams& D, hipStream_t st);

} // namespace crtk
#endif
