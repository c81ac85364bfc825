// cudaraytracing_amd/csrc/crt_select.h -- the arithmetic and the index computations of crt_filter_select (contract: include/crt.h; kernels and
// host code: crt_select.hip): per pixel, the one of K filtered candidates whose error, estimated against the independent other half
// frame, is smallest, and the blend of the candidates by the choices around the pixel.  A workgroup = 32 x 8 pixels (a wave = two rows
// of 32), two kernels:
//   k_select_choose  select_stage_errors: e_k of the tile and a halo of error_radius, straight from the caller's buffers, one LDS plane per
//                    candidate (the halves and the variance are read once per pixel, not once per candidate); barrier;
//                    select_row_sums: H_k for the tile's columns and the rows of the halo, a second set of LDS planes; barrier;
//                    select_choose_pixel: the column sums, E_k, the choice.  Every sum runs in the contract's order, whatever thread has it.
//   k_select_blend   select_stage_choice: the choices of the tile and a halo of blend_radius in LDS (bytes); barrier;
//                    select_blend_pixel: the counts m_k, the blend, the outputs.
// Pixels outside the image have no LDS entry that is ever read: every tap is tested against the image first.
// Like crt_upsample.h this file includes nothing, so that tools/select_host_check.cpp can compile this very text for the host behind
// stand-ins for what it takes from outside: F3 / f3 / write_color (crt_stages.h), __float_as_uint / __uint_as_float.
#ifndef CRT_SELECT_H
#define CRT_SELECT_H

namespace crtk {

const uint32_t kSelectTileW = 32, kSelectTileH = 8;
const int kSelectMaxK = 4, kSelectMaxErrorRadius = 8, kSelectMaxBlendRadius = 4;
const uint8_t kSelectNoPixel = 0xffu; // the staged choice of a position outside the image (never counted)

struct SelParams {
    uint32_t width, height, tiles_x;
    int K, r, s;                              // n_candidates, error_radius, blend_radius
    const float* a; const float* b; const float* v;           // half_a, half_b, half_variance
    const float* fa[kSelectMaxK]; const float* fb[kSelectMaxK];
    float* out_mean;                          // (write_color's names); either may be null
    uint8_t* out_rgb;
    uint8_t* out_choice;                      // may be null
    float* out_error;                         // may be null
    uint8_t* choice;                          // the choice map between the two kernels (scratch)
    unsigned long long* count;                // [K] pixels per candidate (null: not counted)
};

struct SelTile { int x0, y0; };               // the tile's first pixel
__host__ __device__ __forceinline__ SelTile select_tile(const SelParams& P, const uint32_t block)
{
    SelTile T;
    const uint32_t by = block / P.tiles_x, bx = block - by * P.tiles_x;
    T.x0 = (int)(bx * kSelectTileW); T.y0 = (int)(by * kSelectTileH);
    return T;
}
// k_select_choose's LDS, in floats: K planes of ew x eh errors (the tile and its halo), then K planes of 32 x eh row sums
__host__ __device__ __forceinline__ int select_ew(const int r) { return (int)kSelectTileW + 2 * r; }
__host__ __device__ __forceinline__ int select_eh(const int r) { return (int)kSelectTileH + 2 * r; }
__host__ __device__ __forceinline__ int select_ecap(const int r) { return select_ew(r) * select_eh(r); }
__host__ __device__ __forceinline__ int select_hcap(const int r) { return (int)kSelectTileW * select_eh(r); }
inline uint32_t select_choose_lds_bytes(const SelParams& P) { return (uint32_t)(P.K * (select_ecap(P.r) + select_hcap(P.r))) * 4u; }
// k_select_blend's LDS, in bytes
__host__ __device__ __forceinline__ int select_cw(const int s) { return (int)kSelectTileW + 2 * s; }
__host__ __device__ __forceinline__ int select_ch(const int s) { return (int)kSelectTileH + 2 * s; }
inline uint32_t select_blend_lds_bytes(const SelParams& P) { return (uint32_t)(select_cw(P.s) * select_ch(P.s)); }

__device__ __forceinline__ bool select_finite(const float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// step 1 of the contract for one channel: the two squared differences against the other half, each less that half's variance
__device__ __forceinline__ float select_term(const float fa, const float fb, const float a, const float b, const float v)
{
    const float da = fa - b, db = fb - a;
    return (da * da - v) + (db * db - v);
}
__device__ __forceinline__ float select_error(const float tx, const float ty, const float tz)
{
    const float e = ((tx + ty) + tz) / 6.0f;
    return select_finite(e) ? e : __uint_as_float(0x7f800000u);
}

// thread tid of the workgroup's 256: e_k of its share of the tile and its halo, for the positions inside the image
__device__ __forceinline__ void select_stage_errors(const SelParams& P, const SelTile& T, const int tid, float* lds)
{
    const int ew = select_ew(P.r), ecap = select_ecap(P.r);
    for (int i = tid; i < ecap; i += 256) {
        const int iy = i / ew, ix = i - iy * ew;
        const int gx = T.x0 - P.r + ix, gy = T.y0 - P.r + iy;
        if (gx < 0 || gx >= (int)P.width || gy < 0 || gy >= (int)P.height) continue;
        const size_t p = ((size_t)gy * P.width + (size_t)gx) * 3;
        const float ax = P.a[p], ay = P.a[p + 1], az = P.a[p + 2];
        const float bx = P.b[p], by = P.b[p + 1], bz = P.b[p + 2];
        const float vx = P.v[p], vy = P.v[p + 1], vz = P.v[p + 2];
#pragma unroll
        for (int k = 0; k < kSelectMaxK; k++) {
            if (k >= P.K) break;
            const float* fa = P.fa[k] + p;
            const float* fb = P.fb[k] + p;
            lds[k * ecap + i] = select_error(select_term(fa[0], fb[0], ax, bx, vx), select_term(fa[1], fb[1], ay, by, vy), select_term(fa[2], fb[2], az, bz, vz));
        }
    }
}

// after the barrier: H_k of its share of (the tile's columns) x (the rows of the tile and its halo), for the positions inside the image
__device__ __forceinline__ void select_row_sums(const SelParams& P, const SelTile& T, const int tid, float* lds)
{
    const int ew = select_ew(P.r), ecap = select_ecap(P.r), hcap = select_hcap(P.r);
    float* const hs = lds + P.K * ecap;
    for (int i = tid; i < hcap; i += 256) {
        const int row = i / (int)kSelectTileW, cx = i - row * (int)kSelectTileW;
        const int gx = T.x0 + cx, gy = T.y0 - P.r + row;
        if (gx >= (int)P.width || gy < 0 || gy >= (int)P.height) continue;
        for (int k = 0; k < P.K; k++) {
            const float* e = lds + k * ecap + row * ew + cx + P.r;
            float h = 0.0f;
            for (int dx = -P.r; dx <= P.r; dx++) {
                if (gx + dx < 0 || gx + dx >= (int)P.width) continue;
                h = h + e[dx];
            }
            hs[k * hcap + i] = h;
        }
    }
}

// after the second barrier: pixel (T.x0 + tx, T.y0 + ty), inside the image: E_k, the choice and its error into the outputs; returns the choice
__device__ __forceinline__ int select_choose_pixel(const SelParams& P, const SelTile& T, const int tx, const int ty, const float* lds)
{
    const int hcap = select_hcap(P.r), W = (int)P.width, H = (int)P.height;
    const float* const hs = lds + P.K * select_ecap(P.r);
    const int x = T.x0 + tx, y = T.y0 + ty;
    const int xlo = x - P.r < 0 ? 0 : x - P.r, xhi = x + P.r > W - 1 ? W - 1 : x + P.r;
    const int ylo = y - P.r < 0 ? 0 : y - P.r, yhi = y + P.r > H - 1 ? H - 1 : y + P.r;
    const float fn = (float)((xhi - xlo + 1) * (yhi - ylo + 1));
    int best = 0;
    float ebest = 0.0f;
    for (int k = 0; k < P.K; k++) {
        float vs = 0.0f;
        for (int gy = ylo; gy <= yhi; gy++) vs = vs + hs[k * hcap + (gy - T.y0 + P.r) * (int)kSelectTileW + tx];
        const float E = vs / fn;
        if (k == 0 || E < ebest) { best = k; ebest = E; }
    }
    const size_t p = (size_t)y * P.width + (size_t)x;
    P.choice[p] = (uint8_t)best;
    if (P.out_choice) P.out_choice[p] = (uint8_t)best;
    if (P.out_error) P.out_error[p] = ebest;
    return best;
}

// k_select_blend: thread tid's share of the choices of the tile and its halo; outside the image kSelectNoPixel
__device__ __forceinline__ void select_stage_choice(const SelParams& P, const SelTile& T, const int tid, uint8_t* cl)
{
    const int cw = select_cw(P.s), n = cw * select_ch(P.s);
    for (int i = tid; i < n; i += 256) {
        const int iy = i / cw, ix = i - iy * cw;
        const int gx = T.x0 - P.s + ix, gy = T.y0 - P.s + iy;
        const bool inside = gx >= 0 && gx < (int)P.width && gy >= 0 && gy < (int)P.height;
        cl[i] = inside ? P.choice[(size_t)gy * P.width + (size_t)gx] : kSelectNoPixel;
    }
}

// after the barrier: pixel (T.x0 + tx, T.y0 + ty), inside the image: the counts, the blend, the outputs
__device__ __forceinline__ void select_blend_pixel(const SelParams& P, const SelTile& T, const int tx, const int ty, const uint8_t* cl)
{
    const int cw = select_cw(P.s);
    int m[kSelectMaxK] = {0, 0, 0, 0};
    for (int dy = 0; dy <= 2 * P.s; dy++)
        for (int dx = 0; dx <= 2 * P.s; dx++) {
            const int c = (int)cl[(ty + dy) * cw + tx + dx];
#pragma unroll
            for (int k = 0; k < kSelectMaxK; k++) m[k] += c == k ? 1 : 0;
        }
    const float fm = (float)(((m[0] + m[1]) + m[2]) + m[3]);
    const size_t p = (size_t)(T.y0 + ty) * P.width + (size_t)(T.x0 + tx);
    F3 o = f3(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int k = 0; k < kSelectMaxK; k++) {
        if (m[k] == 0) continue; // (a candidate index >= K is never a choice)
        const float w = (float)m[k] / fm;
        const float* fa = P.fa[k] + p * 3;
        const float* fb = P.fb[k] + p * 3;
        o.x = o.x + w * ((fa[0] + fb[0]) * 0.5f);
        o.y = o.y + w * ((fa[1] + fb[1]) * 0.5f);
        o.z = o.z + w * ((fa[2] + fb[2]) * 0.5f);
    }
    write_color(P, p, true, o);
}

} // namespace crtk
#endif
