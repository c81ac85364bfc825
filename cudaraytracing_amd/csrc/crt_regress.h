// cudaraytracing_amd/csrc/crt_regress.h -- the arithmetic and the phases of crt_denoise_regress (contract: include/crt.h; kernel and host
// code: crt_regress.hip): first-order weighted local regression of the colour on the guides, the weights non-local-means patch distances.
// The weight of a tap is crt_denoise_nlm's patch term alone, so everything up to the patch distance D is crt_nlm.h's text: the pack of
// (weight colour, g) into a float4 plane, the staging of tile + halo in LDS (nlm_stage), the pair terms once per (t, o) (nlm_phase_d), the
// row sums once per (x, row, o) (nlm_phase_row) and the weight itself (nlm_weight with guide rows of zeros, whose three terms are +0.0f).
// What is stated here is what follows the weight: the regressors of a tap, the sums of the normal equations, and their solution.
// The kernel is instantiated per feature mask (16 instantiations), so a disabled feature has no row, no column and no load: the system
// of a smaller mask is the smaller system, and every index into the sums is a compile-time constant (the sums stay in registers).
// Like crt_nlm.h this file includes nothing, so that tools/regress_host_check.cpp can compile this very text for the host; it comes
// after crt_nlm.h and takes float4 / make_float4, det_expf, F3 / f3 / write_color from outside as that file does.
#ifndef CRT_REGRESS_H
#define CRT_REGRESS_H

namespace crtk {

const int kRegNormal = 1, kRegAlbedo = 2, kRegDepth = 4, kRegPosition = 8, kRegAllFeatures = 15; // CRT_REGRESS_*
const int kRegMaxFeatures = 9;
// F of a mask: the regressors before the constant
constexpr int regress_features(const int mask) { return ((mask & kRegNormal) ? 3 : 0) + ((mask & kRegAlbedo) ? 3 : 0) + ((mask & kRegDepth) ? 1 : 0) + ((mask & kRegPosition) ? 2 : 0); }

struct RegParams {
    NlmParams n;                              // size, tiles_x, radius, patch, k2, alpha, out_mean, out_rgb; c = (weight colour, g of the weight variance),
                                              // g0 = (normal.xyz, depth), g1 = (albedo.xyz, -); sig2_n = sig2_a = sigma_d = 1 (the weight has no guide term)
    const float4* col;                        // (colour.rgb, 0): what is regressed
    float sigma_n, sigma_a, sigma_d;          // the scales of the features
    float pos_den;                            // sigma_position * (float)radius
    float ridge;
    unsigned long long* count;                // fallback pixels; null: not counted
};

struct RegPack {
    NlmPack n;                                // color / variance: the weight pair; albedo, normal, depth: null unless their feature is enabled
    const float* color;
    float4* col;
};

__device__ __forceinline__ void regress_pack_pixel(const RegPack& K, const int x, const int y)
{
    nlm_pack_pixel(K.n, x, y);
    const size_t p = (size_t)y * K.n.width + (size_t)x;
    K.col[p] = make_float4(K.color[p * 3], K.color[p * 3 + 1], K.color[p * 3 + 2], 0.0f);
}

// the sums of one pixel: A[i][j] for j >= i (the rest is never touched), B[i][c]
template <int F> struct RegSums { float A[F + 1][F + 1]; float B[F + 1][3]; };

template <int F> __device__ __forceinline__ void regress_zero(RegSums<F>& s)
{
#pragma unroll
    for (int i = 0; i <= F; i++) {
#pragma unroll
        for (int j = 0; j <= F; j++) s.A[i][j] = 0.0f;
        s.B[i][0] = 0.0f; s.B[i][1] = 0.0f; s.B[i][2] = 0.0f;
    }
}

// w of a tap from its patch distance D over n taps: nlm_weight without guide terms
__device__ __forceinline__ float regress_weight(const NlmParams& P, const float D, const int n)
{
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return nlm_weight(P, D, n, z, z, z, z); // e_n = 0 / 1, e_a = 0 / 1, e_d = 0 (m = 0): -(((e_p + 0) + 0) + 0) = -e_p
}

// x(q) centred on p: the enabled features in the contract's order, then the constant
template <int MASK> __device__ __forceinline__ void regress_x(const RegParams& P, const float4 gp, const float4 ap, const float4 gq, const float4 aq, const int ox,
                                                              const int oy, float* x)
{
    int i = 0;
    if (MASK & kRegNormal) {
        x[i++] = (gq.x - gp.x) / P.sigma_n; x[i++] = (gq.y - gp.y) / P.sigma_n; x[i++] = (gq.z - gp.z) / P.sigma_n;
    }
    if (MASK & kRegAlbedo) {
        x[i++] = (aq.x - ap.x) / P.sigma_a; x[i++] = (aq.y - ap.y) / P.sigma_a; x[i++] = (aq.z - ap.z) / P.sigma_a;
    }
    if (MASK & kRegDepth) {
        const float m = gp.w > gq.w ? gp.w : gq.w;
        const float r = (gq.w - gp.w) / (P.sigma_d * m);
        x[i++] = m > 0.0f ? r : 0.0f;
    }
    if (MASK & kRegPosition) {
        x[i++] = (float)ox / P.pos_den; x[i++] = (float)oy / P.pos_den;
    }
    x[i] = 1.0f;
}

template <int F> __device__ __forceinline__ void regress_add(RegSums<F>& s, const float* x, const float w, const float4 cq)
{
#pragma unroll
    for (int i = 0; i <= F; i++) {
        const float wx = w * x[i];
#pragma unroll
        for (int j = i; j <= F; j++) s.A[i][j] = s.A[i][j] + wx * x[j];
        s.B[i][0] = s.B[i][0] + wx * cq.x;
        s.B[i][1] = s.B[i][1] + wx * cq.y;
        s.B[i][2] = s.B[i][2] + wx * cq.z;
    }
}

// ridge, elimination in the contract's order, the value at p; true: the pixel fell back to Z / S
template <int F> __device__ __forceinline__ bool regress_solve(RegSums<F>& s, const float ridge, float* out)
{
    const float S = s.A[F][F], Z0 = s.B[F][0], Z1 = s.B[F][1], Z2 = s.B[F][2];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < F; i++) s.A[i][i] = s.A[i][i] + ridge * S;
#pragma unroll
    for (int k = 0; k < F; k++) {
        const float d = s.A[k][k];
        if (!(d > 0.0f)) ok = false;          // (the rows below are then eliminated with numbers nobody uses)
#pragma unroll
        for (int i = k + 1; i <= F; i++) {
            const float f = s.A[k][i] / d;
#pragma unroll
            for (int j = i; j <= F; j++) s.A[i][j] = s.A[i][j] - f * s.A[k][j];
            s.B[i][0] = s.B[i][0] - f * s.B[k][0];
            s.B[i][1] = s.B[i][1] - f * s.B[k][1];
            s.B[i][2] = s.B[i][2] - f * s.B[k][2];
        }
    }
    const float d = s.A[F][F];
    if (!(d > 0.0f)) ok = false;
    out[0] = ok ? s.B[F][0] / d : Z0 / S;
    out[1] = ok ? s.B[F][1] / d : Z1 / S;
    out[2] = ok ? s.B[F][2] / d : Z2 / S;
    return !ok;
}

// pixel (lx, ly) of the tile, inside the image, at window offset o; gp, ap: its guide rows.  s_row: nlm_phase_row's of this offset
template <int MASK> __device__ __forceinline__ void regress_phase_pixel(const RegParams& P, const NlmTile& T, const int ox, const int oy, const int lx, const int ly,
                                                                        const float* s_row, const float4 gp, const float4 ap, RegSums<regress_features(MASK)>& s)
{
    const int W = (int)P.n.width, H = (int)P.n.height, Fp = P.n.patch;
    const int x = T.x0 + lx, y = T.y0 + ly, qx = x + ox, qy = y + oy;
    if (!nlm_inside(qx, qy, W, H)) return;
    float D = 0.0f;
    for (int py = -Fp; py <= Fp; py++) D = D + s_row[(ly + py + Fp) * kNlmTileW + lx];
    const int n = nlm_taps_1d(x, ox, Fp, W) * nlm_taps_1d(y, oy, Fp, H);
    const float w = regress_weight(P.n, D, n);
    const size_t q = (size_t)qy * P.n.width + (size_t)qx;
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 gq = (MASK & (kRegNormal | kRegDepth)) ? P.n.g0[q] : z, aq = (MASK & kRegAlbedo) ? P.n.g1[q] : z;
    float xv[regress_features(MASK) + 1];
    regress_x<MASK>(P, gp, ap, gq, aq, ox, oy, xv);
    regress_add<regress_features(MASK)>(s, xv, w, P.col[q]);
}

// the end of a pixel: true if it fell back
template <int F> __device__ __forceinline__ bool regress_finish(const RegParams& P, const size_t p, RegSums<F>& s)
{
    float o[3];
    const bool fell_back = regress_solve<F>(s, P.ridge, o);
    write_color(P.n, p, true, f3(o[0], o[1], o[2]));
    return fell_back;
}

} // namespace crtk
#endif
