// cudaraytracing_amd/csrc/crt_aov.hip -- the first-hit AOV pass (crt_render_aov, include/crt.h): per pixel, the camera rays of samples
// 0 .. spp-1 -- the primary rays of the frame's paths, camera_dir -- traced by the render kernel's own closest-hit query, and the albedo,
// normal, depth, coverage, triangle and material buffers made of their hits in sample order.  The host side (chunks over samples, the
// trace) is in crt_render.hip; slot -> pixel -> output index is the frame kernels' (slot_pixel, crt_internal.h).
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
__global__ __launch_bounds__(256) void k_aov_resolve(const AovParams A)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= A.nslots) return;
    const SlotPixel px = slot_pixel(A, slot);
    if (!px.valid && (!px.out || !A.last_chunk)) return;
    F3 alb = f3(0.0f, 0.0f, 0.0f), nrm = f3(0.0f, 0.0f, 0.0f);
    float dsum = 0.0f;
    uint32_t hits = 0;
    int32_t tri0 = -1, mat0 = -1;
    if (px.valid) {
        float4* acc = A.acc + (size_t)slot * 3;
        if (!A.first_chunk) {
            const float4 a0 = acc[0], a1 = acc[1], a2 = acc[2];
            alb = f3(a0.x, a0.y, a0.z); dsum = a0.w;
            nrm = f3(a1.x, a1.y, a1.z); hits = __float_as_uint(a1.w);
            tri0 = __float_as_int(a2.x); mat0 = __float_as_int(a2.y);
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
            }
            if (A.first_chunk && s == 0) { tri0 = tri >= 0 ? tri : -1; mat0 = m; }
        }
        if (!A.last_chunk) {
            acc[0] = make_float4(alb.x, alb.y, alb.z, dsum);
            acc[1] = make_float4(nrm.x, nrm.y, nrm.z, __uint_as_float(hits));
            acc[2] = make_float4(__int_as_float(tri0), __int_as_float(mat0), 0.0f, 0.0f);
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
}

// ---- exported to crt_render.hip ----
void launch_aov_rays(const AovParams& A, hipStream_t st)
{
    const uint64_t n = (uint64_t)A.n_samples * A.nslots;
    hipLaunchKernelGGL(k_aov_rays, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, A);
}
void launch_aov_resolve(const AovParams& A, hipStream_t st) { hipLaunchKernelGGL(k_aov_resolve, dim3((A.nslots + 255) / 256), dim3(256), 0, st, A); }

} // namespace crtk
