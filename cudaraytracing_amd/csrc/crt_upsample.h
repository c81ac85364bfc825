// cudaraytracing_amd/csrc/crt_upsample.h -- the arithmetic and the index computations of crt_upsample (contract: include/crt.h; kernel and
// host code: crt_upsample.hip): an image rendered at low resolution brought to the output's resolution along guides that exist at both
// (joint bilateral upsampling).  One thread per OUTPUT pixel, a workgroup = 64 x 4 pixels, a wave = 64 consecutive pixels of one row (the
// denoiser's pass).  Two forms are stated here and give the same bits, since both run upsample_tap / upsample_finish on the same values:
//   direct  a thread gathers its (2 radius)^2 low-resolution taps straight from the caller's buffers (upsample_pixel): the contract as
//           written, what tools/upsample_host_check.cpp and tools/upsample_ab.hip compare the other form with;
//   staged  the workgroup first copies the low-resolution pixels its output pixels can tap -- colour, variance and guides, 13 floats
//           each, one LDS plane per float -- (upsample_stage), and after a barrier every thread takes its taps from there
//           (upsample_pixel_staged).  At factor 2 and radius 1 the 4 taps of a pixel are shared by its 15 neighbours; the staged form
//           is the kernel (8 % faster at 800 x 600 from 400 x 300, 13 to 19 % at 3840 x 2160: docs/experiments.md, "Guide-driven upsampling").
// A guide pair that is not given costs no divergent branch per tap: which pairs are given is uniform over the launch (a scalar test of
// the pointer), the pixel's value and the tap's are then both +0 and the squared sigma is 1, so the term is 0 / 1 = +0 (depth: m = 0,
// e_d = 0) through the same arithmetic.
// Like crt_nlm.h this file includes nothing, so that tools/upsample_host_check.cpp can compile this very text for the host behind
// stand-ins for what it takes from outside: det_expf (crt_detmath.h), F3 / f3 / write_color (crt_stages.h), floorf / fabsf.
#ifndef CRT_UPSAMPLE_H
#define CRT_UPSAMPLE_H

namespace crtk {

const uint32_t kUpsampleTileW = 64, kUpsampleTileH = 4;

struct UpParams {
    uint32_t width, height, low_width, low_height, tiles_x;
    int radius;
    int cap;                                  // the floats of one LDS plane: upsample_stage_cap
    float sx, sy, fradius;                    // (float)low_width / (float)width, likewise, (float)radius
    float min_weight;
    float sig2_n, sig2_a, sigma_d;            // sigma_normal^2, sigma_albedo^2 (1 for a pair that is not given: 0 / 1 = +0), sigma_depth
    const float* color; const float* variance;                          // low resolution; variance null together with out_variance
    const float* lalbedo; const float* lnormal; const float* ldepth;    // low-resolution guides; a pair is given whole or is null whole
    const float* albedo; const float* normal; const float* depth;       // output-resolution guides
    float* out_mean;                          // out_color (write_color's names); either may be null
    uint8_t* out_rgb;
    float* out_variance;
    unsigned long long* count;                // pixels with `guided` false (null: not counted)
};

struct UpSum { float x, y, z, den, vx, vy, vz; };
struct UpGuide { float nx, ny, nz, ax, ay, az, d; };           // normal, albedo, depth of a pixel or of a tap; +0 for a pair that is not given
struct UpTap { UpGuide g; float cx, cy, cz, vx, vy, vz; };      // a low-resolution pixel: its guides, colour and variance (+0 without one)

// the pixel's position among the low-resolution pixels along one axis
__host__ __device__ __forceinline__ float upsample_coord(const uint32_t i, const float scale) { return ((float)i + 0.5f) * scale - 0.5f; }
__device__ __forceinline__ float upsample_tent(const float u, const int t, const float fradius) { return 1.0f - fabsf(u - (float)t) / fradius; }

__device__ __forceinline__ UpGuide upsample_guide(const float* albedo, const float* normal, const float* depth, const size_t i)
{
    UpGuide g = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (normal) { g.nx = normal[i * 3]; g.ny = normal[i * 3 + 1]; g.nz = normal[i * 3 + 2]; }
    if (albedo) { g.ax = albedo[i * 3]; g.ay = albedo[i * 3 + 1]; g.az = albedo[i * 3 + 2]; }
    if (depth) g.d = depth[i];
    return g;
}
// low-resolution pixel q, inside the low image
__device__ __forceinline__ UpTap upsample_load_tap(const UpParams& P, const size_t q)
{
    UpTap t;
    t.g = upsample_guide(P.lalbedo, P.lnormal, P.ldepth, q);
    t.cx = P.color[q * 3]; t.cy = P.color[q * 3 + 1]; t.cz = P.color[q * 3 + 2];
    t.vx = 0.0f; t.vy = 0.0f; t.vz = 0.0f;
    if (P.variance) { t.vx = P.variance[q * 3]; t.vy = P.variance[q * 3 + 1]; t.vz = P.variance[q * 3 + 2]; }
    return t;
}

__device__ __forceinline__ void upsample_add(UpSum& s, const UpTap& q, const float w, const bool has_v)
{
    s.x = s.x + q.cx * w;
    s.y = s.y + q.cy * w;
    s.z = s.z + q.cz * w;
    s.den = s.den + w;
    if (has_v) {
        const float ww = w * w;
        s.vx = s.vx + q.vx * ww;
        s.vy = s.vy + q.vy * ww;
        s.vz = s.vz + q.vz * ww;
    }
}

// One tap of the contract, operation by operation: p the pixel's guides, q the tap, hw = wy * wx; g: num, den, vnum; s: snum, sden, svnum
__device__ __forceinline__ void upsample_tap(const UpParams& P, const UpGuide& p, const UpTap& q, const float hw, const bool has_v, UpSum& g, UpSum& s)
{
    const float dnx = p.nx - q.g.nx, dny = p.ny - q.g.ny, dnz = p.nz - q.g.nz;
    const float e_n = (dnx * dnx + dny * dny + dnz * dnz) / P.sig2_n;
    const float dax = p.ax - q.g.ax, day = p.ay - q.g.ay, daz = p.az - q.g.az;
    const float e_a = (dax * dax + day * day + daz * daz) / P.sig2_a;
    const float m = p.d > q.g.d ? p.d : q.g.d;
    const float r = (p.d - q.g.d) / (P.sigma_d * m);
    const float e_d = m > 0.0f ? r * r : 0.0f;
    const float w = hw * det_expf(-((e_n + e_a) + e_d));
    upsample_add(g, q, w, has_v);
    upsample_add(s, q, hw, has_v);
}

// The sums of output pixel p into the outputs; returns `guided`
__device__ __forceinline__ bool upsample_finish(const UpParams& P, const size_t p, const UpSum& g, const UpSum& s)
{
    const bool guided = g.den > P.min_weight * s.den; // (false for NaN)
    const UpSum& o = guided ? g : s;
    write_color(P, p, true, f3(o.x / o.den, o.y / o.den, o.z / o.den));
    if (P.out_variance) {
        const float dd = o.den * o.den;
        P.out_variance[p * 3] = o.vx / dd; P.out_variance[p * 3 + 1] = o.vy / dd; P.out_variance[p * 3 + 2] = o.vz / dd;
    }
    return guided;
}

// ---- the direct form: the contract as written ----
// Output pixel (x, y), inside the image, every tap straight from the caller's buffers.  Returns `guided`.
__device__ __forceinline__ bool upsample_pixel(const UpParams& P, const uint32_t x, const uint32_t y)
{
    const bool has_v = P.variance != nullptr;
    const int LW = (int)P.low_width, LH = (int)P.low_height, R = P.radius;
    const size_t p = (size_t)y * P.width + (size_t)x;
    const float u = upsample_coord(x, P.sx), v = upsample_coord(y, P.sy);
    const int x0 = (int)floorf(u), y0 = (int)floorf(v); // -1 .. LW - 1, -1 .. LH - 1
    const UpGuide gp = upsample_guide(P.albedo, P.normal, P.depth, p);
    UpSum g = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, s = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int ty = y0 - R + 1; ty <= y0 + R; ty++) {
        if (ty < 0 || ty >= LH) continue;
        const float wy = upsample_tent(v, ty, P.fradius);
        for (int tx = x0 - R + 1; tx <= x0 + R; tx++) {
            if (tx < 0 || tx >= LW) continue; // every tap is tested against the low image: every read is inside it
            upsample_tap(P, gp, upsample_load_tap(P, (size_t)ty * P.low_width + (size_t)tx), wy * upsample_tent(u, tx, P.fradius), has_v, g, s);
        }
    }
    return upsample_finish(P, p, g, s);
}

// ---- the staged form ----
// The low-resolution pixels a workgroup's output pixels can tap: columns lx0 .. lx0 + tw - 1, rows ly0 .. ly0 + th - 1, inside the low
// image.  LDS: kUpsamplePlanes planes of P.cap floats; pixel (lx0 + i, ly0 + j) is entry j * tw + i of each.
const int kUpsamplePlanes = 13; // colour 3, variance 3, albedo 3, normal 3, depth 1
struct UpTile { int lx0, ly0, tw, th; };

// along one axis, for the output pixels first .. last (u grows with the pixel, so every x0 in between lies between the two ends')
__host__ __device__ __forceinline__ void upsample_range(const uint32_t first, const uint32_t last, const float scale, const int R, const int L, int& lo, int& n)
{
    lo = (int)floorf(upsample_coord(first, scale)) - R + 1;
    int hi = (int)floorf(upsample_coord(last, scale)) + R;
    lo = lo < 0 ? 0 : lo;
    hi = hi > L - 1 ? L - 1 : hi;
    n = hi - lo + 1;
}
__host__ __device__ __forceinline__ void upsample_range_x(const UpParams& P, const uint32_t bx, int& lo, int& n)
{
    const uint32_t first = bx * kUpsampleTileW, last = first + kUpsampleTileW - 1 < P.width - 1 ? first + kUpsampleTileW - 1 : P.width - 1;
    upsample_range(first, last, P.sx, P.radius, (int)P.low_width, lo, n);
}
__host__ __device__ __forceinline__ void upsample_range_y(const UpParams& P, const uint32_t by, int& lo, int& n)
{
    const uint32_t first = by * kUpsampleTileH, last = first + kUpsampleTileH - 1 < P.height - 1 ? first + kUpsampleTileH - 1 : P.height - 1;
    upsample_range(first, last, P.sy, P.radius, (int)P.low_height, lo, n);
}
__host__ __device__ __forceinline__ UpTile upsample_tile(const UpParams& P, const uint32_t block)
{
    UpTile T;
    const uint32_t by = block / P.tiles_x, bx = block - by * P.tiles_x;
    upsample_range_x(P, bx, T.lx0, T.tw);
    upsample_range_y(P, by, T.ly0, T.th);
    return T;
}
// The largest tw x the largest th over the launch's workgroups, from the very arithmetic the workgroups run (the host compiles it
// without contraction, like the device): no workgroup's tile has more pixels.  At most (63 + 2 radius) x (3 + 2 radius), at equal sizes.
inline int upsample_stage_cap(const UpParams& P)
{
    int tw = 0, th = 0, lo, n;
    for (uint32_t bx = 0; bx < P.tiles_x; bx++) { upsample_range_x(P, bx, lo, n); tw = n > tw ? n : tw; }
    for (uint32_t by = 0; by < (P.height + kUpsampleTileH - 1) / kUpsampleTileH; by++) { upsample_range_y(P, by, lo, n); th = n > th ? n : th; }
    return tw * th;
}
inline uint32_t upsample_lds_bytes(const UpParams& P) { return (uint32_t)(kUpsamplePlanes * P.cap) * 4u; }

// thread tid of the workgroup's 256 copies its share of the tile
__device__ __forceinline__ void upsample_stage(const UpParams& P, const UpTile& T, const int tid, float* s_tile)
{
    for (int i = tid; i < T.tw * T.th; i += 256) {
        const int j = i / T.tw;
        const UpTap t = upsample_load_tap(P, (size_t)(T.ly0 + j) * P.low_width + (size_t)(T.lx0 + (i - j * T.tw)));
        s_tile[i] = t.cx; s_tile[P.cap + i] = t.cy; s_tile[2 * P.cap + i] = t.cz;
        s_tile[3 * P.cap + i] = t.vx; s_tile[4 * P.cap + i] = t.vy; s_tile[5 * P.cap + i] = t.vz;
        s_tile[6 * P.cap + i] = t.g.ax; s_tile[7 * P.cap + i] = t.g.ay; s_tile[8 * P.cap + i] = t.g.az;
        s_tile[9 * P.cap + i] = t.g.nx; s_tile[10 * P.cap + i] = t.g.ny; s_tile[11 * P.cap + i] = t.g.nz;
        s_tile[12 * P.cap + i] = t.g.d;
    }
}
__device__ __forceinline__ UpTap upsample_staged_tap(const UpParams& P, const float* s_tile, const int i)
{
    UpTap t;
    t.cx = s_tile[i]; t.cy = s_tile[P.cap + i]; t.cz = s_tile[2 * P.cap + i];
    t.vx = s_tile[3 * P.cap + i]; t.vy = s_tile[4 * P.cap + i]; t.vz = s_tile[5 * P.cap + i];
    t.g.ax = s_tile[6 * P.cap + i]; t.g.ay = s_tile[7 * P.cap + i]; t.g.az = s_tile[8 * P.cap + i];
    t.g.nx = s_tile[9 * P.cap + i]; t.g.ny = s_tile[10 * P.cap + i]; t.g.nz = s_tile[11 * P.cap + i];
    t.g.d = s_tile[12 * P.cap + i];
    return t;
}

// Output pixel (x, y) of the workgroup of tile T, inside the image, after the barrier that follows upsample_stage.  Returns `guided`.
__device__ __forceinline__ bool upsample_pixel_staged(const UpParams& P, const UpTile& T, const uint32_t x, const uint32_t y, const float* s_tile)
{
    const bool has_v = P.variance != nullptr;
    const int LW = (int)P.low_width, LH = (int)P.low_height, R = P.radius;
    const size_t p = (size_t)y * P.width + (size_t)x;
    const float u = upsample_coord(x, P.sx), v = upsample_coord(y, P.sy);
    const int x0 = (int)floorf(u), y0 = (int)floorf(v);
    const UpGuide gp = upsample_guide(P.albedo, P.normal, P.depth, p);
    UpSum g = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, s = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int ty = y0 - R + 1; ty <= y0 + R; ty++) {
        if (ty < 0 || ty >= LH) continue;
        const float wy = upsample_tent(v, ty, P.fradius);
        for (int tx = x0 - R + 1; tx <= x0 + R; tx++) {
            if (tx < 0 || tx >= LW) continue; // a tap inside the low image lies inside the workgroup's tile (upsample_range)
            upsample_tap(P, gp, upsample_staged_tap(P, s_tile, (ty - T.ly0) * T.tw + (tx - T.lx0)), wy * upsample_tent(u, tx, P.fradius), has_v, g, s);
        }
    }
    return upsample_finish(P, p, g, s);
}

} // namespace crtk
#endif
