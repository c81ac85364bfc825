// cudaraytracing_amd/csrc/crt_pyramid.h -- the arithmetic, the index computations and the kernels' phases of crt_pyramid_down and
// crt_pyramid_merge (contract: include/crt.h; kernels and host code: crt_pyramid.hip): the two image operations of a Laplacian pyramid
// over the single-scale filters.
//   down   one thread per COARSE pixel, a workgroup = 64 x 4 coarse pixels, a wave = 64 consecutive coarse pixels of one row: the two
//          fine rows a wave reads are 2 x 1 536 consecutive bytes per 3-float plane.  A coarse pixel's two taps of a fine row are 24
//          consecutive bytes at 24 x (pixel index): 8-byte aligned, 16-byte only for every other pixel, and an output pixel is 12 bytes.
//          So the widest access the layout allows every lane is 8 bytes: a pixel with all four taps takes each row as three 8-byte loads
//          (depth: one) when every base pointer is 8-byte aligned and the width is even, so that the odd fine rows are aligned as well
//          (P.vec); edge pixels, odd widths and unaligned buffers go float by float through the same arithmetic.
//   merge  one thread per OUTPUT pixel, a workgroup = 32 x 8 output pixels.  Two forms, the same bits from both, since both run
//          pyramid_detail / pyramid_tap / pyramid_finish on the same values:
//            direct  a thread computes the detail d = coarse - D(fine) of each of its (up to) four coarse taps itself: four fine pixels
//                    and one coarse pixel per tap (pyramid_merge_pixel);
//            staged  the workgroup first computes d once for every coarse pixel its output pixels can tap -- (16 + 2) x (4 + 2) of them
//                    for a tile inside the image, three LDS planes of P.cap floats -- (pyramid_stage), and after a barrier every thread
//                    interpolates from there (pyramid_merge_pixel_staged).
//          The interpolation is crt_upsample's unguided one at radius 1, through crt_upsample.h's own upsample_coord, upsample_tent and
//          upsample_range: which coarse pixels a tile taps comes from the very arithmetic its threads run, not from a factor of 2.
// Like crt_upsample.h, which it needs included first, this file includes nothing, so that tools/pyramid_host_check.cpp can compile this
// very text for the host behind stand-ins for what it takes from outside: float2, F3 / f3 / write_color (crt_stages.h), floorf.
#ifndef CRT_PYRAMID_H
#define CRT_PYRAMID_H

namespace crtk {

const uint32_t kPyramidDownTileW = 64, kPyramidDownTileH = 4;
const uint32_t kPyramidMergeTileW = 32, kPyramidMergeTileH = 8;

struct PyrDownParams {
    uint32_t width, height, low_width, low_height, tiles_x; // tiles_x: workgroups per row of coarse tiles
    uint32_t vec;                                           // every buffer given is 8-byte aligned and the width is even
    const float* color; const float* variance; const float* albedo; const float* normal; const float* depth; // fine; all but color may be null
    float* out_color; float* out_variance; float* out_albedo; float* out_normal; float* out_depth;            // coarse; null with its input
};

struct PyrMergeParams {
    uint32_t width, height, low_width, low_height, tiles_x;
    int cap;                  // the floats of one LDS plane: pyramid_stage_cap
    float sx, sy;             // (float)low_width / (float)width, likewise
    const float* fine;        // width x height x 3
    const float* coarse;      // low_width x low_height x 3
    float* out_mean;          // out_color (write_color's names); either may be null
    uint8_t* out_rgb;
};

// The fine pixels of coarse pixel (X, Y), inside the coarse image, in the contract's order: (2X, 2Y), (2X + 1, 2Y), (2X, 2Y + 1),
// (2X + 1, 2Y + 1).  i[k]: the pixel index of tap k; in[k]: it lies inside the fine image (tap 0 always does); n: how many do (4, 2 or 1).
// Every loop over the taps below has four iterations with constant indices, so that the values stay in registers.
struct PyrTaps { bool in[4]; size_t i[4]; int n; };
__host__ __device__ __forceinline__ PyrTaps pyramid_taps(const uint32_t width, const uint32_t height, const uint32_t X, const uint32_t Y)
{
    PyrTaps t;
    const bool x1 = 2 * X + 1 < width, y1 = 2 * Y + 1 < height;
    t.i[0] = (size_t)(2 * Y) * width + (size_t)(2 * X);
    t.i[1] = t.i[0] + 1; t.i[2] = t.i[0] + width; t.i[3] = t.i[2] + 1;
    t.in[0] = true; t.in[1] = x1; t.in[2] = y1; t.in[3] = x1 && y1;
    t.n = (x1 ? 2 : 1) * (y1 ? 2 : 1);
    return t;
}

// the contract's lines over the taps taken, each sum from +0.0f in the taps' order, one IEEE operation per symbol
__device__ __forceinline__ float pyramid_sum(const float* v, const PyrTaps& t)
{
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (t.in[k]) s = s + v[k];
    return s;
}
__device__ __forceinline__ float pyramid_mean(const float* v, const PyrTaps& t) { return pyramid_sum(v, t) / (float)t.n; }
__device__ __forceinline__ float pyramid_variance(const float* v, const PyrTaps& t)
{
    const float fn = (float)t.n;
    return pyramid_sum(v, t) / (fn * fn);
}
__device__ __forceinline__ float pyramid_depth(const float* v, const PyrTaps& t)
{
    float s = 0.0f, nd = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (t.in[k] && v[k] > 0.0f) { s = s + v[k]; nd = nd + 1.0f; } // (false for NaN)
    return nd > 0.0f ? s / nd : 0.0f;
}

// the three channels of the taps taken of a 3-float plane, float by float (a tap that is not taken: +0, never read)
__device__ __forceinline__ void pyramid_gather3(const float* plane, const PyrTaps& t, float v[3][4])
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v[0][k] = 0.0f; v[1][k] = 0.0f; v[2][k] = 0.0f;
        if (t.in[k]) { v[0][k] = plane[t.i[k] * 3]; v[1][k] = plane[t.i[k] * 3 + 1]; v[2][k] = plane[t.i[k] * 3 + 2]; }
    }
}
// the same for a pixel with all four taps under P.vec: each fine row's two pixels are six consecutive floats, 8-byte aligned
__device__ __forceinline__ void pyramid_gather3_vec(const float* plane, const PyrTaps& t, float v[3][4])
{
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const float2* row = reinterpret_cast<const float2*>(plane + t.i[2 * r] * 3);
        const float2 a = row[0], b = row[1], c = row[2];
        v[0][2 * r] = a.x; v[1][2 * r] = a.y; v[2][2 * r] = b.x;
        v[0][2 * r + 1] = b.y; v[1][2 * r + 1] = c.x; v[2][2 * r + 1] = c.y;
    }
}

// D of the contract for one 3-float plane at coarse pixel Q whose taps are t; VAR: the variance line, else the mean
template <bool VAR> __device__ __forceinline__ float pyramid_line(const float* v, const PyrTaps& t) { return VAR ? pyramid_variance(v, t) : pyramid_mean(v, t); }
template <bool VAR> __device__ __forceinline__ void pyramid_down3(const float* plane, float* out, const size_t Q, const PyrTaps& t, const bool vec)
{
    float v[3][4];
    if (vec && t.n == 4) pyramid_gather3_vec(plane, t, v);
    else pyramid_gather3(plane, t, v);
    out[Q * 3] = pyramid_line<VAR>(v[0], t); out[Q * 3 + 1] = pyramid_line<VAR>(v[1], t); out[Q * 3 + 2] = pyramid_line<VAR>(v[2], t);
}

// coarse pixel (X, Y), inside the coarse image
__device__ __forceinline__ void pyramid_down_pixel(const PyrDownParams& P, const uint32_t X, const uint32_t Y)
{
    const PyrTaps t = pyramid_taps(P.width, P.height, X, Y);
    const size_t Q = (size_t)Y * P.low_width + (size_t)X;
    const bool vec = P.vec != 0;
    pyramid_down3<false>(P.color, P.out_color, Q, t, vec);
    if (P.albedo) pyramid_down3<false>(P.albedo, P.out_albedo, Q, t, vec);
    if (P.normal) pyramid_down3<false>(P.normal, P.out_normal, Q, t, vec);
    if (P.variance) pyramid_down3<true>(P.variance, P.out_variance, Q, t, vec);
    if (P.depth) {
        float v[4];
        if (vec && t.n == 4) {
            const float2 a = *reinterpret_cast<const float2*>(P.depth + t.i[0]), b = *reinterpret_cast<const float2*>(P.depth + t.i[2]);
            v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = t.in[k] ? P.depth[t.i[k]] : 0.0f;
        }
        P.out_depth[Q] = pyramid_depth(v, t);
    }
}

// ---- the merge ----
// d(Q) = coarse(Q) - D(fine)(Q) per channel, Q = (X, Y) inside the coarse image; D: crt_pyramid_down's colour line
__device__ __forceinline__ F3 pyramid_detail(const PyrMergeParams& P, const uint32_t X, const uint32_t Y)
{
    const PyrTaps t = pyramid_taps(P.width, P.height, X, Y);
    const size_t Q = (size_t)Y * P.low_width + (size_t)X;
    float v[3][4];
    pyramid_gather3(P.fine, t, v);
    return f3(P.coarse[Q * 3] - pyramid_mean(v[0], t), P.coarse[Q * 3 + 1] - pyramid_mean(v[1], t), P.coarse[Q * 3 + 2] - pyramid_mean(v[2], t));
}

struct PyrSum { float x, y, z, den; };
// one tap of crt_upsample's unguided sums: snum = snum + d * hw, sden = sden + hw
__device__ __forceinline__ void pyramid_tap(PyrSum& s, const F3 d, const float hw)
{
    s.x = s.x + d.x * hw;
    s.y = s.y + d.y * hw;
    s.z = s.z + d.z * hw;
    s.den = s.den + hw;
}
// out(p) = fine(p) + snum / sden
__device__ __forceinline__ void pyramid_finish(const PyrMergeParams& P, const size_t p, const PyrSum& s)
{
    write_color(P, p, true, f3(P.fine[p * 3] + s.x / s.den, P.fine[p * 3 + 1] + s.y / s.den, P.fine[p * 3 + 2] + s.z / s.den));
}

// Output pixel (x, y), inside the image: its taps in crt_upsample's order at radius 1, detail(tx, ty) for each one inside the coarse image
template <class Detail> __device__ __forceinline__ void pyramid_interpolate(const PyrMergeParams& P, const uint32_t x, const uint32_t y, Detail detail)
{
    const int LW = (int)P.low_width, LH = (int)P.low_height;
    const float u = upsample_coord(x, P.sx), v = upsample_coord(y, P.sy);
    const int x0 = (int)floorf(u), y0 = (int)floorf(v); // -1 .. LW - 1, -1 .. LH - 1
    PyrSum s = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int ty = y0; ty <= y0 + 1; ty++) {
        if (ty < 0 || ty >= LH) continue;
        const float wy = upsample_tent(v, ty, 1.0f);
        for (int tx = x0; tx <= x0 + 1; tx++) {
            if (tx < 0 || tx >= LW) continue; // every tap is tested against the coarse image: every read is inside it
            pyramid_tap(s, detail(tx, ty), wy * upsample_tent(u, tx, 1.0f));
        }
    }
    pyramid_finish(P, (size_t)y * P.width + (size_t)x, s);
}

// the direct form
__device__ __forceinline__ void pyramid_merge_pixel(const PyrMergeParams& P, const uint32_t x, const uint32_t y)
{
    pyramid_interpolate(P, x, y, [&](const int tx, const int ty) { return pyramid_detail(P, (uint32_t)tx, (uint32_t)ty); });
}

// ---- the staged form ----
// The coarse pixels a workgroup's output pixels can tap: columns lx0 .. lx0 + tw - 1, rows ly0 .. ly0 + th - 1, inside the coarse image
// (upsample_range at radius 1).  LDS: 3 planes of P.cap floats; coarse pixel (lx0 + i, ly0 + j) is entry j * tw + i of each.
struct PyrTile { int lx0, ly0, tw, th; };
__host__ __device__ __forceinline__ void pyramid_range_x(const PyrMergeParams& P, const uint32_t bx, int& lo, int& n)
{
    const uint32_t first = bx * kPyramidMergeTileW, last = first + kPyramidMergeTileW - 1 < P.width - 1 ? first + kPyramidMergeTileW - 1 : P.width - 1;
    upsample_range(first, last, P.sx, 1, (int)P.low_width, lo, n);
}
__host__ __device__ __forceinline__ void pyramid_range_y(const PyrMergeParams& P, const uint32_t by, int& lo, int& n)
{
    const uint32_t first = by * kPyramidMergeTileH, last = first + kPyramidMergeTileH - 1 < P.height - 1 ? first + kPyramidMergeTileH - 1 : P.height - 1;
    upsample_range(first, last, P.sy, 1, (int)P.low_height, lo, n);
}
__host__ __device__ __forceinline__ PyrTile pyramid_tile(const PyrMergeParams& P, const uint32_t block)
{
    PyrTile T;
    const uint32_t by = block / P.tiles_x, bx = block - by * P.tiles_x;
    pyramid_range_x(P, bx, T.lx0, T.tw);
    pyramid_range_y(P, by, T.ly0, T.th);
    return T;
}
// The largest tw x the largest th over the launch's workgroups, from the very arithmetic the workgroups run: no workgroup's tile has
// more pixels.  18 x 6 for every size whose coordinates float32 holds exactly.
inline int pyramid_stage_cap(const PyrMergeParams& P)
{
    int tw = 0, th = 0, lo, n;
    for (uint32_t bx = 0; bx < P.tiles_x; bx++) { pyramid_range_x(P, bx, lo, n); tw = n > tw ? n : tw; }
    for (uint32_t by = 0; by < (P.height + kPyramidMergeTileH - 1) / kPyramidMergeTileH; by++) { pyramid_range_y(P, by, lo, n); th = n > th ? n : th; }
    return tw * th;
}
inline uint32_t pyramid_lds_bytes(const PyrMergeParams& P) { return (uint32_t)(3 * P.cap) * 4u; }

// thread tid of the workgroup's 256 computes its share of the tile's details
__device__ __forceinline__ void pyramid_stage(const PyrMergeParams& P, const PyrTile& T, const int tid, float* s_tile)
{
    for (int i = tid; i < T.tw * T.th; i += 256) {
        const int j = i / T.tw;
        const F3 d = pyramid_detail(P, (uint32_t)(T.lx0 + (i - j * T.tw)), (uint32_t)(T.ly0 + j));
        s_tile[i] = d.x; s_tile[P.cap + i] = d.y; s_tile[2 * P.cap + i] = d.z;
    }
}
// output pixel (x, y) of the workgroup of tile T, inside the image, after the barrier that follows pyramid_stage
__device__ __forceinline__ void pyramid_merge_pixel_staged(const PyrMergeParams& P, const PyrTile& T, const uint32_t x, const uint32_t y, const float* s_tile)
{
    pyramid_interpolate(P, x, y, [&](const int tx, const int ty) { // a tap inside the coarse image lies inside the workgroup's tile (upsample_range)
        const int i = (ty - T.ly0) * T.tw + (tx - T.lx0);
        return f3(s_tile[i], s_tile[P.cap + i], s_tile[2 * P.cap + i]);
    });
}

} // namespace crtk
#endif
