// cudaraytracing_amd/csrc/crt_nlm.h -- the arithmetic and the index computations of crt_denoise_nlm (contract: include/crt.h; kernels and
// host code: crt_nlm.hip): non-local means with variance-normalised patch distances, joint with the guides.
// Two forms of the filter are stated here, phase by phase, and give the same bits:
//   direct  one thread per pixel evaluates the contract as written, every tap through the caches (nlm_direct_pixel);
//   shared  a workgroup of kNlmThreads owns a tile of kNlmTileW x kNlmTileH pixels and stages the packed colour plane of the tile and its
//           halo (radius + patch) in LDS once (nlm_stage).  Per window offset o it computes every pair term d_o(t) of the tile and its
//           patch halo once (nlm_phase_d), then every row sum row(x, ty, o) once (nlm_phase_row), then each pixel adds its column of row
//           sums and weighs the tap (nlm_phase_pixel); workgroup barriers separate the phases.  The pair term and whether a tap is
//           skipped depend on (t, o) only, and a row sum adds its terms in the contract's order, so sharing them changes no bit.
// Like crt_modulate.h this file includes nothing, so that tools/nlm_host_check.cpp can compile this very text for the host behind
// stand-ins for what it takes from outside: float4 / make_float4, det_expf (crt_detmath.h), F3 / f3 / write_color (crt_stages.h).
#ifndef CRT_NLM_H
#define CRT_NLM_H

namespace crtk {

const int kNlmMaxRadius = 8, kNlmMaxPatch = 3;
const int kNlmTileW = 32, kNlmTileH = 8, kNlmThreads = 256; // a wave = two tile rows: each 32-lane group of an LDS access is one row
const int kNlmDivShift = 20;                                 // nlm_div: exact for i < 2^11 and divisors below 64 (checked on the host)

struct NlmParams {
    uint32_t width, height, tiles_x;
    int radius, patch;
    float k2, alpha;                          // k * k
    float sig2_n, sig2_a, sigma_d;            // sigma_normal^2, sigma_albedo^2 (1 for a NULL guide: 0 / 1 = +0), sigma_depth
    const float4* c;                          // (r, g, b, g(p))
    const float4* g0;                         // (normal.xyz, depth); zeros for NULL guides
    const float4* g1;                         // (albedo.xyz, v(p))
    float* out_mean;                          // either may be null (write_color's names)
    uint8_t* out_rgb;
    float* out_var;                           // may be null
};

struct NlmPack {
    uint32_t width, height;
    const float* color; const float* variance; const float* albedo; const float* normal; const float* depth;
    float4* c; float4* g0; float4* g1;
};

struct NlmSum { float x, y, z, den, vnum; };

// ---- the contract's lines, one IEEE operation per symbol ----
__device__ __forceinline__ float nlm_v(const float* variance, const size_t p) { return (variance[p * 3] + variance[p * 3 + 1]) + variance[p * 3 + 2]; }
__device__ __forceinline__ float nlm_k3(const int d) { return d == 0 ? 0.5f : 0.25f; }
// g(p): crt_denoise_var's 3x3 Gaussian of v, pass 0
__device__ __forceinline__ float nlm_g(const float* variance, const int x, const int y, const int W, const int H)
{
    float gn = 0.0f, gd = 0.0f;
    for (int dy = -1; dy <= 1; dy++) {
        const int ty = y + dy;
        if (ty < 0 || ty >= H) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int tx = x + dx;
            if (tx < 0 || tx >= W) continue;
            const float k = nlm_k3(dy) * nlm_k3(dx);
            gn = gn + k * nlm_v(variance, (size_t)ty * (size_t)W + (size_t)tx);
            gd = gd + k;
        }
    }
    return gn / gd;
}

// one pixel of the pack kernel
__device__ __forceinline__ void nlm_pack_pixel(const NlmPack& K, const int x, const int y)
{
    const size_t p = (size_t)y * K.width + (size_t)x;
    K.c[p] = make_float4(K.color[p * 3], K.color[p * 3 + 1], K.color[p * 3 + 2], nlm_g(K.variance, x, y, (int)K.width, (int)K.height));
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f), a = make_float4(0.0f, 0.0f, 0.0f, nlm_v(K.variance, p));
    if (K.normal) { g.x = K.normal[p * 3]; g.y = K.normal[p * 3 + 1]; g.z = K.normal[p * 3 + 2]; }
    if (K.depth) g.w = K.depth[p];
    if (K.albedo) { a.x = K.albedo[p * 3]; a.y = K.albedo[p * 3 + 1]; a.z = K.albedo[p * 3 + 2]; }
    K.g0[p] = g;
    K.g1[p] = a;
}

// d of the pair (t, u = t + o): ct, cu = (colour, g) of the two
__device__ __forceinline__ float nlm_pair(const float4 ct, const float4 cu, const float k2, const float alpha)
{
    const float dcx = ct.x - cu.x, dcy = ct.y - cu.y, dcz = ct.z - cu.z;
    const float s = dcx * dcx + dcy * dcy + dcz * dcz;
    const float mn = cu.w < ct.w ? cu.w : ct.w;
    return (s - alpha * (ct.w + mn)) / (1e-10f + k2 * (ct.w + cu.w));
}

// the weight of q for p from the patch distance D over n taps and the guides (the guide terms: crt_denoise's)
__device__ __forceinline__ float nlm_weight(const NlmParams& P, const float D, const int n, const float4 gp, const float4 ap, const float4 gq, const float4 aq)
{
    const float Dm = D / (float)n;
    const float e_p = Dm < 0.0f ? 0.0f : Dm;
    const float dnx = gp.x - gq.x, dny = gp.y - gq.y, dnz = gp.z - gq.z;
    const float e_n = (dnx * dnx + dny * dny + dnz * dnz) / P.sig2_n;
    const float dax = ap.x - aq.x, day = ap.y - aq.y, daz = ap.z - aq.z;
    const float e_a = (dax * dax + day * day + daz * daz) / P.sig2_a;
    const float m = gp.w > gq.w ? gp.w : gq.w;
    const float r = (gp.w - gq.w) / (P.sigma_d * m);
    const float e_d = m > 0.0f ? r * r : 0.0f;
    return det_expf(-(((e_p + e_n) + e_a) + e_d));
}

__device__ __forceinline__ void nlm_add(NlmSum& s, const float4 cq, const float vq, const float w)
{
    s.x = s.x + cq.x * w;
    s.y = s.y + cq.y * w;
    s.z = s.z + cq.z * w;
    s.den = s.den + w;
    s.vnum = s.vnum + vq * (w * w);
}

template <class PB> __device__ __forceinline__ void nlm_finish(const PB& P, const size_t p, const NlmSum& s)
{
    write_color(P, p, true, f3(s.x / s.den, s.y / s.den, s.z / s.den));
    if (P.out_var) P.out_var[p] = s.vnum / (s.den * s.den);
}

__device__ __forceinline__ bool nlm_inside(const int x, const int y, const int W, const int H) { return x >= 0 && x < W && y >= 0 && y < H; }

// ---- the direct form: the contract as written ----
__device__ __forceinline__ void nlm_direct_pixel(const NlmParams& P, const int x, const int y)
{
    const int W = (int)P.width, H = (int)P.height, R = P.radius, F = P.patch;
    const size_t p = (size_t)y * P.width + (size_t)x;
    const float4 gp = P.g0[p], ap = P.g1[p];
    NlmSum s = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int oy = -R; oy <= R; oy++) {
        for (int ox = -R; ox <= R; ox++) {
            const int qx = x + ox, qy = y + oy;
            if (!nlm_inside(qx, qy, W, H)) continue;
            float D = 0.0f;
            int n = 0;
            for (int py = -F; py <= F; py++) {
                float row = 0.0f;
                const int ty = y + py, uy = ty + oy;
                if (ty >= 0 && ty < H && uy >= 0 && uy < H) {
                    for (int px = -F; px <= F; px++) {
                        const int tx = x + px, ux = tx + ox;
                        if (tx < 0 || tx >= W || ux < 0 || ux >= W) continue;
                        row = row + nlm_pair(P.c[(size_t)ty * P.width + (size_t)tx], P.c[(size_t)uy * P.width + (size_t)ux], P.k2, P.alpha);
                        n = n + 1;
                    }
                }
                D = D + row;
            }
            const size_t q = (size_t)qy * P.width + (size_t)qx;
            const float4 aq = P.g1[q];
            nlm_add(s, P.c[q], aq.w, nlm_weight(P, D, n, gp, ap, P.g0[q], aq));
        }
    }
    nlm_finish(P, p, s);
}

// ---- the shared form ----
// The tile of a workgroup and its three LDS arrays:
//   s_c    sw x sh float4: the colour plane of image pixels (x0 - halo .. x0 + TileW + halo) x (y0 - halo ..), halo = radius + patch;
//          pixels outside the image hold zeros that no phase reads
//   s_d    dw x dh floats: d_o(t) for t in the tile and its patch halo, dw = TileW + 2 patch, dh = TileH + 2 patch
//   s_row  TileW x dh floats: row(x, ty, o) for the tile's columns and the rows of s_d
struct NlmTile {
    int x0, y0, halo, sw, sh, dw, dh;
    uint32_t sw_m, dw_m;                      // nlm_div's multipliers for sw and dw
};
__device__ __forceinline__ uint32_t nlm_div_m(const int d) { return ((1u << kNlmDivShift) + (uint32_t)d - 1u) / (uint32_t)d; }
__device__ __forceinline__ int nlm_div(const int i, const uint32_t m) { return (int)(((uint32_t)i * m) >> kNlmDivShift); }
__device__ __forceinline__ NlmTile nlm_tile(const NlmParams& P, const uint32_t block)
{
    NlmTile T;
    const uint32_t by = block / P.tiles_x, bx = block - by * P.tiles_x;
    T.x0 = (int)bx * kNlmTileW; T.y0 = (int)by * kNlmTileH;
    T.halo = P.radius + P.patch;
    T.sw = kNlmTileW + 2 * T.halo; T.sh = kNlmTileH + 2 * T.halo;
    T.dw = kNlmTileW + 2 * P.patch; T.dh = kNlmTileH + 2 * P.patch;
    T.sw_m = nlm_div_m(T.sw); T.dw_m = nlm_div_m(T.dw);
    return T;
}
inline uint32_t nlm_stage_elems(const int radius, const int patch) { return (uint32_t)((kNlmTileW + 2 * (radius + patch)) * (kNlmTileH + 2 * (radius + patch))); }
inline uint32_t nlm_d_elems(const int patch) { return (uint32_t)((kNlmTileW + 2 * patch) * (kNlmTileH + 2 * patch)); }
inline uint32_t nlm_row_elems(const int patch) { return (uint32_t)(kNlmTileW * (kNlmTileH + 2 * patch)); }
// bytes of LDS of a workgroup: s_c, s_d, s_row in this order (29840 at radius 8, patch 3)
inline uint32_t nlm_lds_bytes(const int radius, const int patch) { return nlm_stage_elems(radius, patch) * 16u + (nlm_d_elems(patch) + nlm_row_elems(patch)) * 4u; }

// s_c's entry of image pixel (ix, iy), which lies within the halo of the tile
__device__ __forceinline__ int nlm_stage_index(const NlmTile& T, const int ix, const int iy) { return (iy - T.y0 + T.halo) * T.sw + (ix - T.x0 + T.halo); }

// no pixel of the tile has its q = p + o inside the image: the whole workgroup leaves the offset out
__device__ __forceinline__ bool nlm_offset_misses_tile(const NlmTile& T, const int ox, const int oy, const int W, const int H)
{
    const int x1 = (T.x0 + kNlmTileW < W ? T.x0 + kNlmTileW : W) - 1, y1 = (T.y0 + kNlmTileH < H ? T.y0 + kNlmTileH : H) - 1; // the tile's last pixel inside
    return x1 + ox < 0 || T.x0 + ox >= W || y1 + oy < 0 || T.y0 + oy >= H;
}

// the px of -F .. F with x + px and x + px + o inside [0, W): the taps of a patch along one axis
__device__ __forceinline__ int nlm_taps_1d(const int x, const int o, const int F, const int W)
{
    int lo = -F, hi = F;
    if (-x > lo) lo = -x;
    if (-x - o > lo) lo = -x - o;
    if (W - 1 - x < hi) hi = W - 1 - x;
    if (W - 1 - x - o < hi) hi = W - 1 - x - o;
    return hi >= lo ? hi - lo + 1 : 0;
}

__device__ __forceinline__ void nlm_stage(const NlmParams& P, const NlmTile& T, const int tid, float4* s_c)
{
    const int W = (int)P.width, H = (int)P.height;
    for (int i = tid; i < T.sw * T.sh; i += kNlmThreads) {
        const int sy = nlm_div(i, T.sw_m), sx = i - sy * T.sw;
        const int ix = T.x0 - T.halo + sx, iy = T.y0 - T.halo + sy;
        s_c[i] = nlm_inside(ix, iy, W, H) ? P.c[(size_t)iy * P.width + (size_t)ix] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

__device__ __forceinline__ void nlm_phase_d(const NlmParams& P, const NlmTile& T, const int ox, const int oy, const int tid, const float4* s_c, float* s_d)
{
    const int W = (int)P.width, H = (int)P.height;
    for (int i = tid; i < T.dw * T.dh; i += kNlmThreads) {
        const int dy = nlm_div(i, T.dw_m), dx = i - dy * T.dw;
        const int tx = T.x0 - P.patch + dx, ty = T.y0 - P.patch + dy;
        float d = 0.0f; // (a skipped tap: never read)
        if (nlm_inside(tx, ty, W, H) && nlm_inside(tx + ox, ty + oy, W, H))
            d = nlm_pair(s_c[nlm_stage_index(T, tx, ty)], s_c[nlm_stage_index(T, tx + ox, ty + oy)], P.k2, P.alpha);
        s_d[i] = d;
    }
}

__device__ __forceinline__ void nlm_phase_row(const NlmParams& P, const NlmTile& T, const int ox, const int oy, const int tid, const float* s_d, float* s_row)
{
    const int W = (int)P.width, H = (int)P.height, F = P.patch;
    for (int i = tid; i < kNlmTileW * T.dh; i += kNlmThreads) {
        const int ry = i / kNlmTileW, lx = i - ry * kNlmTileW;
        const int x = T.x0 + lx, ty = T.y0 - F + ry, uy = ty + oy;
        float row = 0.0f;
        if (x < W && ty >= 0 && ty < H && uy >= 0 && uy < H) {
            for (int px = -F; px <= F; px++) {
                const int tx = x + px, ux = tx + ox;
                if (tx < 0 || tx >= W || ux < 0 || ux >= W) continue;
                row = row + s_d[ry * T.dw + (lx + px + F)];
            }
        }
        s_row[i] = row;
    }
}

// pixel (lx, ly) of the tile, inside the image; gp, ap: its guide rows
__device__ __forceinline__ void nlm_phase_pixel(const NlmParams& P, const NlmTile& T, const int ox, const int oy, const int lx, const int ly, const float4* s_c,
                                                const float* s_row, const float4 gp, const float4 ap, NlmSum& s)
{
    const int W = (int)P.width, H = (int)P.height, F = P.patch;
    const int x = T.x0 + lx, y = T.y0 + ly, qx = x + ox, qy = y + oy;
    if (!nlm_inside(qx, qy, W, H)) return;
    float D = 0.0f;
    for (int py = -F; py <= F; py++) D = D + s_row[(ly + py + F) * kNlmTileW + lx];
    const int n = nlm_taps_1d(x, ox, F, W) * nlm_taps_1d(y, oy, F, H);
    const size_t q = (size_t)qy * P.width + (size_t)qx;
    const float4 aq = P.g1[q];
    nlm_add(s, s_c[nlm_stage_index(T, qx, qy)], aq.w, nlm_weight(P, D, n, gp, ap, P.g0[q], aq));
}

} // namespace crtk
#endif
