// cudaraytracing_amd/csrc/crt_pixel_filter.h -- the arithmetic, the index computations and the kernels' phases of the pixel reconstruction
// filters (CRT_FLAG_PIXEL_FILTER, crt_filtered_frame; contract: include/crt.h; kernels and host code: crt_pixel_filter.hip).  After a
// chunk's accumulate kernel, one more kernel adds the chunk's samples to the sums a (three planes) and W of every pixel: a sample counts
// for the pixels around its jittered position, which the kernel recomputes from the draw that placed the path's camera ray.
//   direct  one thread per pixel slot; for every sample of the chunk and every pixel q around its own it draws q's jitter, and where the
//           weight is not zero loads q's radiance.
//   staged  a workgroup of 256 threads owns four consecutive tiles of one tile row, 32 x 8 pixels.  Per sample it first computes jitter
//           and quotient once for every pixel of the rectangle and its halo -- (32 + 2 reach) x (8 + 2 reach) entries of five floats in
//           LDS, five planes (pixel_filter_stage) -- and after a barrier every thread gathers its taps from there (pixel_filter_gather).
// Both run pixel_filter_tap on the same values in the same order: the same bits.  The loops over the taps have constant bounds
// (REACH is a template argument), so that nothing is indexed at run time.
// Like crt_pyramid.h this file includes nothing, so that tools/pixel_filter_host_check.cpp can compile this very text for the host behind
// stand-ins for what it takes from outside: crt_stages.h (AParams, slot_pixel, the sums' accessors), Rad3, load_radiance, F3 / f3,
// rng_draw, rng_uniform.
#ifndef CRT_PIXEL_FILTER_H
#define CRT_PIXEL_FILTER_H

namespace crtk {

const uint32_t kPixelFilterBox = 0, kPixelFilterTent = 1, kPixelFilterMitchell = 2; // CRT_PIXEL_FILTER_*
const int kPixelFilterMaxReach = 2;
const uint32_t kPixelFilterTileW = 32, kPixelFilterTileH = 8; // the staged form's workgroup: four 8 x 8 tiles of one tile row
// the staged form's LDS: five planes (ux, uy, x.x, x.y, x.z) of the rectangle with its halo at the largest reach
const int kPixelFilterStageCap = (int)(kPixelFilterTileW + 2 * kPixelFilterMaxReach) * (int)(kPixelFilterTileH + 2 * kPixelFilterMaxReach);

struct PixelFilterParams {
    AParams A;        // the frame's slot map, spp, the chunk (L, chunk_samples, first_chunk) and, for the read-out, the sum c and the outputs
    float* planes;    // 4 planes of nslots: a.x, a.y, a.z, W
    uint64_t seed;
    uint32_t s0;      // the chunk's first sample, its index in the frame
    uint32_t kind;
    float radius;
    float scale_n;    // the read-out: (float)S / (float)n
};

// reach = ceil(R - 0.5): the pixels around p whose samples can lie in p's support (R - 0.5f is exact for the radii allowed)
inline int pixel_filter_reach(const float radius)
{
    const float t = radius - 0.5f;
    const int r = (int)t;
    return (float)r < t ? r + 1 : r;
}
// what crt_set_pixel_filter allows
inline bool pixel_filter_allowed(const uint32_t kind, const float radius)
{
    if (kind == kPixelFilterBox) return radius >= 0.5f && radius <= 2.0f;
    if (kind == kPixelFilterTent) return radius >= 1.0f && radius <= 2.0f;
    return kind == kPixelFilterMitchell && radius == 2.0f; // (every comparison is false for NaN)
}

// f(d) of the contract
__host__ __device__ __forceinline__ float pixel_filter_weight(const uint32_t kind, const float R, const float d)
{
    if (!(d > -R && d <= R)) return 0.0f;
    if (kind == kPixelFilterBox) return 1.0f;
    const float x = d < 0.0f ? -d : d;
    if (kind == kPixelFilterTent) return 1.0f - x / R;
    if (x < 1.0f) return ((((21.0f * x - 36.0f) * x) * x) + 16.0f) / 18.0f;
    return ((((-7.0f * x + 36.0f) * x - 60.0f) * x) + 32.0f) / 18.0f;
}

struct PixelFilterSum { float x, y, z, w; }; // a and W

// x = L / (float)S, the frame's own quotient
__host__ __device__ __forceinline__ F3 pixel_filter_quotient(const Rad3 l, const float fS) { return f3(l.x / fS, l.y / fS, l.z / fS); }

// One tap: the sample of pixel q = p + (di, dj) whose jitter is (ux, uy), for p.  quotient() gives the sample's x and is called only
// where the weight is not zero (a tap the contract skips reads nothing).
template <class Quotient>
__host__ __device__ __forceinline__ void pixel_filter_tap(const uint32_t kind, const float R, const int di, const int dj, const float ux, const float uy,
                                                          PixelFilterSum& s, Quotient quotient)
{
    const float dx = ((float)di + ux) - 0.5f, dy = ((float)dj + uy) - 0.5f;
    const float w = pixel_filter_weight(kind, R, dx) * pixel_filter_weight(kind, R, dy);
    if (w == 0.0f) return;
    const F3 x = quotient();
    s.x = s.x + w * x.x;
    s.y = s.y + w * x.y;
    s.z = s.z + w * x.z;
    s.w = s.w + w;
}

// the read-out of one pixel: a * (S / W) where W > 0, else c * (S / n) with scale_n = (float)S / (float)n (crt_preview's value)
__host__ __device__ __forceinline__ F3 pixel_filter_resolve(const F3 a, const float W, const F3 c, const float fS, const float scale_n)
{
    if (W > 0.0f) { // (false for NaN)
        const float r = fS / W;
        return f3(a.x * r, a.y * r, a.z * r);
    }
    return f3(c.x * scale_n, c.y * scale_n, c.z * scale_n);
}

// the jitter of sample k of pixel (i, j): camera_dir's draw (crt_path.h)
__host__ __device__ __forceinline__ void pixel_filter_jitter(const PixelFilterParams& P, const uint32_t i, const uint32_t j, const uint32_t k, float& ux, float& uy)
{
    const U4 rj = rng_draw(P.seed, j * P.A.width + i, k, 0, RNG_JITTER, 0);
    ux = rng_uniform(rj.x); uy = rng_uniform(rj.y);
}
// the slot of pixel (i, j), inside the frame, of an unsharded frame (world == 1): slot_to_pixel's inverse
__host__ __device__ __forceinline__ uint32_t pixel_filter_slot(const PixelFilterParams& P, const uint32_t i, const uint32_t j)
{
    return ((j >> 3) * P.A.tiles_x + (i >> 3)) * 64u + (j & 7u) * 8u + (i & 7u);
}
__host__ __device__ __forceinline__ bool pixel_filter_inside(const PixelFilterParams& P, const int i, const int j)
{
    return i >= 0 && j >= 0 && (uint32_t)i < P.A.width && (uint32_t)j < P.A.height;
}

// the sums of a slot
__device__ __forceinline__ PixelFilterSum pixel_filter_load(const PixelFilterParams& P, const uint32_t slot)
{
    PixelFilterSum s = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!P.A.first_chunk) {
        const F3 a = acc_load3(P.planes, P.A.nslots, slot);
        s.x = a.x; s.y = a.y; s.z = a.z; s.w = acc_load(P.planes + 3ull * P.A.nslots + slot);
    }
    return s;
}
__device__ __forceinline__ void pixel_filter_store(const PixelFilterParams& P, const uint32_t slot, const PixelFilterSum& s)
{
    acc_store3(P.planes, P.A.nslots, slot, f3(s.x, s.y, s.z));
    acc_store(P.planes + 3ull * P.A.nslots + slot, s.w);
}

// ---- the direct form: pixel slot `slot` takes the whole chunk ----
template <int REACH> __device__ __forceinline__ void pixel_filter_direct(const PixelFilterParams& P, const uint32_t slot)
{
    const SlotPixel px = slot_pixel(P.A, slot);
    if (!px.valid) return;
    PixelFilterSum s = pixel_filter_load(P, slot);
    const float fS = (float)P.A.spp;
    for (uint32_t smp = 0; smp < P.A.chunk_samples; smp++) {
        const Rad3* const Ls = P.A.L + (size_t)smp * P.A.nslots;
        const uint32_t k = P.s0 + smp;
#pragma unroll
        for (int dj = -REACH; dj <= REACH; dj++) {
#pragma unroll
            for (int di = -REACH; di <= REACH; di++) {
                const int qi = (int)px.i + di, qj = (int)px.j + dj;
                if (!pixel_filter_inside(P, qi, qj)) continue;
                float ux, uy;
                pixel_filter_jitter(P, (uint32_t)qi, (uint32_t)qj, k, ux, uy);
                pixel_filter_tap(P.kind, P.radius, di, dj, ux, uy, s, [&] { // (qi, qj) is inside the frame: its slot is one of the nslots
                    return pixel_filter_quotient(load_radiance(Ls + pixel_filter_slot(P, (uint32_t)qi, (uint32_t)qj)), fS);
                });
            }
        }
    }
    pixel_filter_store(P, slot, s);
}

// ---- the staged form ----
// Workgroup `block` owns the tiles 4 g .. 4 g + 3 of tile row ty (g = block % groups_x, ty = block / groups_x, groups_x =
// ceil(tiles_x / 4)): the pixels (x0 .. x0 + 31, y0 .. y0 + 7).  Thread tid has pixel (x0 + 8 (tid / 64) + tid % 8, y0 + (tid % 64) / 8),
// which is the thread's slot in slot order where its tile exists.
struct PixelFilterTile { int x0, y0; };
__host__ __device__ __forceinline__ uint32_t pixel_filter_groups_x(const PixelFilterParams& P) { return (P.A.tiles_x + 3u) / 4u; }
__host__ __device__ __forceinline__ uint32_t pixel_filter_staged_blocks(const PixelFilterParams& P) { return pixel_filter_groups_x(P) * (P.A.n_tiles / P.A.tiles_x); }
__host__ __device__ __forceinline__ PixelFilterTile pixel_filter_tile(const PixelFilterParams& P, const uint32_t block)
{
    const uint32_t gx = pixel_filter_groups_x(P), ty = block / gx, g = block - ty * gx;
    PixelFilterTile T;
    T.x0 = (int)(g * kPixelFilterTileW); T.y0 = (int)(ty * kPixelFilterTileH);
    return T;
}
__host__ __device__ __forceinline__ void pixel_filter_thread_pixel(const uint32_t tid, int& lx, int& ly)
{
    lx = (int)((tid >> 6) * 8u + (tid & 7u)); ly = (int)((tid & 63u) >> 3);
}

// Thread tid's share of sample smp of the chunk: entry e = hy * (32 + 2 REACH) + hx is pixel (x0 - REACH + hx, y0 - REACH + hy); outside
// the frame its ux is -1 (a jitter lies in (0, 1]) and nothing else of it is written or read.
template <int REACH> __device__ __forceinline__ void pixel_filter_stage(const PixelFilterParams& P, const PixelFilterTile& T, const uint32_t tid, const uint32_t smp, float* s_lds)
{
    const int HW = (int)kPixelFilterTileW + 2 * REACH, HH = (int)kPixelFilterTileH + 2 * REACH;
    const float fS = (float)P.A.spp;
    const Rad3* const Ls = P.A.L + (size_t)smp * P.A.nslots;
    for (int e = (int)tid; e < HW * HH; e += 256) {
        const int hy = e / HW, hx = e - hy * HW;
        const int qi = T.x0 - REACH + hx, qj = T.y0 - REACH + hy;
        if (!pixel_filter_inside(P, qi, qj)) { s_lds[e] = -1.0f; continue; }
        float ux, uy;
        pixel_filter_jitter(P, (uint32_t)qi, (uint32_t)qj, P.s0 + smp, ux, uy);
        const F3 x = pixel_filter_quotient(load_radiance(Ls + pixel_filter_slot(P, (uint32_t)qi, (uint32_t)qj)), fS);
        s_lds[e] = ux; s_lds[kPixelFilterStageCap + e] = uy;
        s_lds[2 * kPixelFilterStageCap + e] = x.x; s_lds[3 * kPixelFilterStageCap + e] = x.y; s_lds[4 * kPixelFilterStageCap + e] = x.z;
    }
}
// after the barrier that follows pixel_filter_stage: the taps of the thread's pixel (lx, ly) of the rectangle, a pixel of the frame
template <int REACH> __device__ __forceinline__ void pixel_filter_gather(const PixelFilterParams& P, const int lx, const int ly, const float* s_lds, PixelFilterSum& s)
{
    const int HW = (int)kPixelFilterTileW + 2 * REACH;
#pragma unroll
    for (int dj = -REACH; dj <= REACH; dj++) {
#pragma unroll
        for (int di = -REACH; di <= REACH; di++) {
            const int e = (ly + REACH + dj) * HW + (lx + REACH + di); // 0 <= lx + REACH + di < HW, likewise the row: inside the staged entries
            const float ux = s_lds[e];
            if (ux < 0.0f) continue; // outside the frame
            pixel_filter_tap(P.kind, P.radius, di, dj, ux, s_lds[kPixelFilterStageCap + e], s, [&] {
                return f3(s_lds[2 * kPixelFilterStageCap + e], s_lds[3 * kPixelFilterStageCap + e], s_lds[4 * kPixelFilterStageCap + e]);
            });
        }
    }
}

// ---- the read-out (crt_filtered_frame): one thread per pixel slot ----
__device__ __forceinline__ void pixel_filter_readout(const PixelFilterParams& P, const uint32_t slot)
{
    const SlotPixel px = slot_pixel(P.A, slot);
    if (!px.out) return;
    F3 v = f3(0.0f, 0.0f, 0.0f);
    if (px.valid)
        v = pixel_filter_resolve(acc_load3(P.planes, P.A.nslots, slot), acc_load(P.planes + 3ull * P.A.nslots + slot), acc_load3(P.A.accum, P.A.nslots, slot),
                                 (float)P.A.spp, P.scale_n);
    write_color(P.A, px.o, px.valid, v);
}

} // namespace crtk
#endif
