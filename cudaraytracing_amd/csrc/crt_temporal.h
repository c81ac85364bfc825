// cudaraytracing_amd/csrc/crt_temporal.h -- the parameter blocks of the temporal pass and its whole per-pixel arithmetic (crt_temporal,
// crt_temporal_clamped, crt_temporal_moments, crt_temporal_dual; contract: include/crt.h; kernels and host code: crt_temporal.hip).  The
// pass is one operation with optional parts: reproject the pixel, gather four taps of the history, optionally fetch and choose a second
// candidate, optionally clamp, blend.  Every expression of the contract stands here once:
//   temporal_ray, temporal_project   the pixel's camera ray, and a point along it seen from the previous camera
//   temporal_gather                  the tap loop: surface taps, virtual taps, and the moment planes riding on either
//   temporal_box, history_channel    the neighbourhood sums and the clamp
//   temporal_reset, temporal_blend, temporal_write   what a pixel writes without a history, with one, and the stores
// and the two forms of a pixel are made of them:
//   temporal_single<CLAMP, MOMENTS>  one candidate (k_temporal)
//   temporal_dual_begin              the pixel's ray, candidate S, and whether the pixel tries V
//   temporal_dual_finish<CLAMP>      candidate V and the choice (behind the caller's wave-uniform `any lane tries`), then the same blend
// The dual form: a pixel of a planar mirror shows two things, its own shading, which moves with the surface, and the mirrored scene, which
// moves with its virtual image -- the point at path_depth along the pixel's camera ray.  The pass fetches a history through each
// (candidate S: crt_temporal's taps; candidate V: the same taps keyed on the specular planes) and blends the one that lies nearer the mean
// of the current frame's colours around the pixel.  Between begin and finish k_temporal_dual holds one ballot; a caller without waves
// passes the pixel's own `tries`.
// p is a pixel's index and p3 = 3 p its offset in a plane of three floats: the forms make the product once and hand it on, because a
// function that forms it itself is compiled to a multiply of its own that the inlined kernel then keeps (docs/experiments.md).
// Like crt_select.h this file includes nothing, so that tools/temporal_host_check.cpp can compile this very text for the host behind
// stand-ins for what it takes from outside: F3 / f3 / dot3 / unit3 (crt_device.h), sqrt_f (crt_detmath.h), write_color (crt_stages.h), floorf / fabsf.
#ifndef CRT_TEMPORAL_H
#define CRT_TEMPORAL_H

namespace crtk {

struct TpParams {
    uint32_t width, height, tiles_x;
    float eye[3], iv[9], scale, ar;           // current camera; scale / ar as camera_scale_ar (crt_render.hip)
    float peye[3], piv[9], pscale;            // the camera the history was made with
    float depth_tol, normal_tol2, alpha_min;  // normal_tol2 = normal_tolerance * normal_tolerance
    const float* color; const float* variance; const float* depth; const float* normal; const int32_t* id;          // current frame
    const float* pcolor; const float* pvariance; const float* phistory; const float* pdepth; const float* pnormal; const int32_t* pid;
    float* out_mean;                          // out_color (write_color's names)
    uint8_t* out_rgb;
    float* out_variance;
    float* out_history;
    unsigned long long* count;                // [0] pixels that took the history, [1] of those: moved by the clamp (null: not counted)
    int radius;                               // CLAMP only: crt_temporal_clamp
    float gamma;
    const float* pm1; const float* pm2;       // MOMENTS only: the history's moment planes (null without a history)
    float* out_m1; float* out_m2;
};

// k_temporal_dual: TpParams (pm1 .. out_m2 unused; count has four entries: [2] pixels that tried V, [3] pixels that took V) and the
// specular planes of both frames
struct TpDualParams : TpParams {
    const float* path_depth; const float* bounces; const float* last_normal;        // current frame (last_normal may be null)
    const float* ppath_depth; const float* pbounces; const float* plast_normal;     // the history's (null without a history)
    int dual_radius;                          // crt_temporal_dual
    float min_bounces;
};

// A point of the current frame seen from the previous camera: where it lands (fx, fy), how far from that eye it lies (tp), and
// crt_temporal's `ok` without its depth term
struct TpProj { float tp, fx, fy; bool ok; };
// The interpolated history of one candidate, before the division by ws
struct TpTaps { F3 hc, hv; float hn, ws; };
// The history's moment planes over the same taps (crt_temporal_moments' sums of m1 and m2)
struct TpMoments { F3 h1, h2; };
// The sums of the current colour around a pixel (crt_temporal_clamped's s1, s2, cnt)
struct TpBox { F3 s1, s2; float cnt; };
// A pixel's current colour and variance, and what it writes: the reset's values until temporal_blend replaces them
struct TpPixel { F3 c, v, oc, ov, o1, o2; float oh; };
// What temporal_dual_begin hands to temporal_dual_finish
struct TpDualState {
    F3 d;          // the pixel-centre camera ray
    TpTaps S;
    bool valid_S;  // ok && ws_S > 0.015625f
    bool tries;    // a history is given, bounces(p) >= min_bounces and path_depth(p) > 0
};
// What a pixel did, for the counts (tried, took_V: the dual form's)
struct TpFlags { bool took, clamped, tried, took_V; };

// the pixel-centre ray of the current camera (camera_dir without the jitter)
__device__ __forceinline__ F3 temporal_ray(const TpParams& P, const int x, const int y)
{
    const float fw = (float)(int)P.width, fh = (float)(int)P.height;
    const float sx = (((2 * ((float)x + 0.5f)) / fw - 1) * P.scale) * P.ar;
    const float sy = (1 - (2 * ((float)y + 0.5f)) / fh) * P.scale;
    const F3 cd = unit3(f3(-sx, sy, 1));
    return unit3(f3(P.iv[0] * cd.x + (P.iv[3] * cd.y + P.iv[6] * cd.z),
                    P.iv[1] * cd.x + (P.iv[4] * cd.y + P.iv[7] * cd.z),
                    P.iv[2] * cd.x + (P.iv[5] * cd.y + P.iv[8] * cd.z)));
}

// The point at distance t along ray d into the previous camera: inverse of its rotation (the transpose), then the inverse of the
// image-plane map.  ok is false for a NaN anywhere.
__device__ __forceinline__ TpProj temporal_project(const TpParams& P, const F3 d, const float t)
{
    const float fw = (float)(int)P.width, fh = (float)(int)P.height;
    const F3 wp = f3(P.eye[0] + d.x * t, P.eye[1] + d.y * t, P.eye[2] + d.z * t);
    const F3 pv = f3(wp.x - P.peye[0], wp.y - P.peye[1], wp.z - P.peye[2]);
    const float cx = P.piv[0] * pv.x + (P.piv[1] * pv.y + P.piv[2] * pv.z);
    const float cy = P.piv[3] * pv.x + (P.piv[4] * pv.y + P.piv[5] * pv.z);
    const float cz = P.piv[6] * pv.x + (P.piv[7] * pv.y + P.piv[8] * pv.z);
    TpProj r;
    r.tp = sqrt_f(dot3(pv, pv));
    r.fx = (((((-cx) / cz) / (P.pscale * P.ar)) + 1) * fw) / 2 - 0.5f;
    r.fy = (((1 - (cy / cz) / P.pscale) * fh) / 2) - 0.5f;
    r.ok = t > 0.0f && cz > 0.0f && r.fx > -1.0f && r.fx < fw && r.fy > -1.0f && r.fy < fh;
    return r;
}

// The four bilinear taps of a projection that is ok.  VIRTUAL false: crt_temporal's tap test (first-hit depth, normal, id).  VIRTUAL true
// (PB: TpDualParams): the tap must itself be a mirror pixel (bounces >= min_bounces, path_depth > 0), its path_depth must agree with tp,
// its last normal (if given) with the pixel's, and its first-hit id (if given) must be the pixel's: the same mirror.  MOMENTS: m takes the
// moment planes on the predicates and the weight of the colour's taps.  Every tap is tested against the image before anything is read at it.
template <bool VIRTUAL, bool MOMENTS, class PB>
__device__ __forceinline__ TpTaps temporal_gather(const PB& P, const size_t p, const size_t p3, const TpProj& pr, TpMoments& m)
{
    const int W = (int)P.width, H = (int)P.height;
    const float flx = floorf(pr.fx), fly = floorf(pr.fy);
    const float wx = pr.fx - flx, wy = pr.fy - fly;
    const int x0 = (int)flx, y0 = (int)fly; // -1 .. W - 1, -1 .. H - 1
    const float tol = P.depth_tol * pr.tp;
    const float* cn; const float* pn; const float* pdist;
    if constexpr (VIRTUAL) { cn = P.last_normal; pn = P.plast_normal; pdist = P.ppath_depth; }
    else { cn = P.normal; pn = P.pnormal; pdist = P.pdepth; }
    F3 n = f3(0.0f, 0.0f, 0.0f);
    if (cn) n = f3(cn[p3], cn[p3 + 1], cn[p3 + 2]);
    const int32_t idp = P.id ? P.id[p] : 0;
    TpTaps t;
    t.hc = f3(0.0f, 0.0f, 0.0f); t.hv = f3(0.0f, 0.0f, 0.0f); m.h1 = f3(0.0f, 0.0f, 0.0f); m.h2 = f3(0.0f, 0.0f, 0.0f);
    t.hn = 0.0f; t.ws = 0.0f;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int qy = y0 + j;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int qx = x0 + i;
            if (qx < 0 || qx >= W) continue;
            const size_t q = (size_t)qy * P.width + (size_t)qx;
            if constexpr (VIRTUAL)
                if (!(P.pbounces[q] >= P.min_bounces)) continue;
            const float pd = pdist[q];
            if (!(pd > 0.0f)) continue;
            if (!(fabsf(pd - pr.tp) <= tol)) continue;
            if (cn) {
                const float dnx = n.x - pn[q * 3], dny = n.y - pn[q * 3 + 1], dnz = n.z - pn[q * 3 + 2];
                if (!(dnx * dnx + dny * dny + dnz * dnz <= P.normal_tol2)) continue;
            }
            if (P.id && idp != P.pid[q]) continue;
            const float b = (i ? wx : 1 - wx) * (j ? wy : 1 - wy);
            t.hc.x = t.hc.x + P.pcolor[q * 3] * b;
            t.hc.y = t.hc.y + P.pcolor[q * 3 + 1] * b;
            t.hc.z = t.hc.z + P.pcolor[q * 3 + 2] * b;
            if (P.variance) {
                t.hv.x = t.hv.x + P.pvariance[q * 3] * b;
                t.hv.y = t.hv.y + P.pvariance[q * 3 + 1] * b;
                t.hv.z = t.hv.z + P.pvariance[q * 3 + 2] * b;
            }
            if (MOMENTS) {
                m.h1.x = m.h1.x + P.pm1[q * 3] * b;
                m.h1.y = m.h1.y + P.pm1[q * 3 + 1] * b;
                m.h1.z = m.h1.z + P.pm1[q * 3 + 2] * b;
                m.h2.x = m.h2.x + P.pm2[q * 3] * b;
                m.h2.y = m.h2.y + P.pm2[q * 3 + 1] * b;
                m.h2.z = m.h2.z + P.pm2[q * 3 + 2] * b;
            }
            t.hn = t.hn + P.phistory[q] * b;
            t.ws = t.ws + b;
        }
    }
    return t;
}

// no sums yet
__device__ __forceinline__ TpBox temporal_no_box()
{
    TpBox b;
    b.s1 = f3(0.0f, 0.0f, 0.0f); b.s2 = f3(0.0f, 0.0f, 0.0f);
    b.cnt = 0.0f;
    return b;
}

// sums of the current colour and its squares around (x, y); every tap is tested against the image, so every read is inside it
__device__ __forceinline__ TpBox temporal_box(const TpParams& P, const int x, const int y, const int radius)
{
    const int W = (int)P.width, H = (int)P.height;
    TpBox b = temporal_no_box();
    for (int dy = -radius; dy <= radius; dy++) {
        const int ty = y + dy;
        if (ty < 0 || ty >= H) continue;
        for (int dx = -radius; dx <= radius; dx++) {
            const int tx = x + dx;
            if (tx < 0 || tx >= W) continue;
            const size_t t = ((size_t)ty * P.width + (size_t)tx) * 3;
            const float tr = P.color[t], tg = P.color[t + 1], tb = P.color[t + 2];
            b.s1.x = b.s1.x + tr; b.s1.y = b.s1.y + tg; b.s1.z = b.s1.z + tb;
            b.s2.x = b.s2.x + tr * tr; b.s2.y = b.s2.y + tg * tg; b.s2.z = b.s2.z + tb * tb;
            b.cnt = b.cnt + 1;
        }
    }
    return b;
}

// squared distance of a candidate's history colour from the neighbourhood's mean
__device__ __forceinline__ float temporal_distance(const TpTaps& t, const TpBox& b)
{
    const float dx = t.hc.x / t.ws - b.s1.x / b.cnt, dy = t.hc.y / t.ws - b.s1.y / b.cnt, dz = t.hc.z / t.ws - b.s1.z / b.cnt;
    return dx * dx + (dy * dy + dz * dz);
}

// The choice of a pixel whose candidate V is valid: V iff S is not valid or V lies strictly nearer the mean (a tie or a NaN keeps S)
__device__ __forceinline__ bool temporal_takes_virtual(const bool valid_S, const TpTaps& S, const TpTaps& V, const TpBox& b)
{
    if (!valid_S) return true;
    return temporal_distance(V, b) < temporal_distance(S, b);
}

// One channel of the interpolated history, hc / ws; with CLAMP clamped into [mu - gamma sd, mu + gamma sd] of the neighbourhood sums
// (`moved` is set if that changed it).  A NaN in the history or in the box fails both comparisons and the history passes through.
template <bool CLAMP>
__device__ __forceinline__ float history_channel(float hc, float ws, float s1, float s2, float cnt, float gamma, bool& moved)
{
    float h = hc / ws;
    if (CLAMP) {
        const float mu = s1 / cnt;
        float e = s2 / cnt - mu * mu;
        e = e < 0.0f ? 0.0f : e;
        const float w = gamma * sqrt_f(e);
        const float lo = mu - w, hi = mu + w;
        const bool below = h < lo;
        h = below ? lo : h;
        const bool above = h > hi;
        h = above ? hi : h;
        moved |= below | above;
    }
    return h;
}

// The current colour and variance of the pixel at p3, and the outputs of a pixel that takes no history
template <bool MOMENTS>
__device__ __forceinline__ TpPixel temporal_reset(const TpParams& P, const size_t p3)
{
    TpPixel o;
    o.c = f3(P.color[p3], P.color[p3 + 1], P.color[p3 + 2]);
    o.v = f3(0.0f, 0.0f, 0.0f);
    if (P.variance) o.v = f3(P.variance[p3], P.variance[p3 + 1], P.variance[p3 + 2]);
    o.oc = o.c; o.ov = o.v;
    o.oh = 1.0f;
    o.o1 = o.c; o.o2 = f3(0.0f, 0.0f, 0.0f);
    if (MOMENTS) o.o2 = f3(o.c.x * o.c.x, o.c.y * o.c.y, o.c.z * o.c.z);
    return o;
}

// The blend of pixel (x, y) with the history T it takes (T.ws > 0.015625f).  CLAMP: have_box says that box holds the sums of the clamp's
// radius already, else they are summed here; `clamped` is set if the clamp moved a channel.  MOMENTS: m's planes, never clamped --
// m1 is the running mean of what the pixel was seen to show.
template <bool CLAMP, bool MOMENTS>
__device__ __forceinline__ void temporal_blend(const TpParams& P, const int x, const int y, const TpTaps& T, const TpMoments& m, TpBox box, const bool have_box,
                                               TpPixel& o, bool& clamped)
{
    const float hn = T.hn / T.ws;
    o.oh = hn + 1;
    float a = 1 / o.oh;
    a = a < P.alpha_min ? P.alpha_min : a;
    const float k = 1 - a;
    if (CLAMP) {
        if (!have_box) box = temporal_box(P, x, y, P.radius);
    }
    o.oc = f3(history_channel<CLAMP>(T.hc.x, T.ws, box.s1.x, box.s2.x, box.cnt, P.gamma, clamped) * k + o.c.x * a,
              history_channel<CLAMP>(T.hc.y, T.ws, box.s1.y, box.s2.y, box.cnt, P.gamma, clamped) * k + o.c.y * a,
              history_channel<CLAMP>(T.hc.z, T.ws, box.s1.z, box.s2.z, box.cnt, P.gamma, clamped) * k + o.c.z * a);
    if (P.variance) {
        const float kk = k * k, aa = a * a;
        o.ov = f3((T.hv.x / T.ws) * kk + o.v.x * aa, (T.hv.y / T.ws) * kk + o.v.y * aa, (T.hv.z / T.ws) * kk + o.v.z * aa);
    }
    if (MOMENTS) {
        o.o1 = f3((m.h1.x / T.ws) * k + o.c.x * a, (m.h1.y / T.ws) * k + o.c.y * a, (m.h1.z / T.ws) * k + o.c.z * a);
        o.o2 = f3((m.h2.x / T.ws) * k + o.o2.x * a, (m.h2.y / T.ws) * k + o.o2.y * a, (m.h2.z / T.ws) * k + o.o2.z * a);
    }
}

// the pixel's stores
template <bool MOMENTS>
__device__ __forceinline__ void temporal_write(const TpParams& P, const size_t p, const size_t p3, const TpPixel& o)
{
    write_color(P, p, true, o.oc);
    if (P.out_variance) { P.out_variance[p3] = o.ov.x; P.out_variance[p3 + 1] = o.ov.y; P.out_variance[p3 + 2] = o.ov.z; }
    P.out_history[p] = o.oh;
    if (MOMENTS) {
        P.out_m1[p3] = o.o1.x; P.out_m1[p3 + 1] = o.o1.y; P.out_m1[p3 + 2] = o.o1.z;
        P.out_m2[p3] = o.o2.x; P.out_m2[p3 + 1] = o.o2.y; P.out_m2[p3 + 2] = o.o2.z;
    }
}

// Pixel (x, y), inside the image: the whole single-candidate form.  The neighbourhood sums run INSIDE the branch of the pixels that take
// the history, not before it: see docs/experiments.md.
template <bool CLAMP, bool MOMENTS>
__device__ __forceinline__ TpFlags temporal_single(const TpParams& P, const int x, const int y)
{
    const size_t p = (size_t)y * P.width + (size_t)x, p3 = p * 3;
    TpFlags fl = {};
    TpPixel o = temporal_reset<MOMENTS>(P, p3);
    if (P.pcolor) {
        const float dp = P.depth[p];
        const TpProj pr = temporal_project(P, temporal_ray(P, x, y), dp);
        if (pr.ok) {
            TpMoments m;
            const TpTaps T = temporal_gather<false, MOMENTS>(P, p, p3, pr, m);
            if (T.ws > 0.015625f) {
                fl.took = true;
                temporal_blend<CLAMP, MOMENTS>(P, x, y, T, m, temporal_no_box(), false, o, fl.clamped);
            }
        }
    }
    temporal_write<MOMENTS>(P, p, p3, o);
    return fl;
}

// Pixel (x, y), inside the image, of a call with a history: its ray, candidate S, whether it tries V
__device__ __forceinline__ TpDualState temporal_dual_begin(const TpDualParams& P, const int x, const int y)
{
    const size_t p = (size_t)y * P.width + (size_t)x, p3 = p * 3;
    TpDualState st;
    st.d = temporal_ray(P, x, y);
    st.S.hc = f3(0.0f, 0.0f, 0.0f); st.S.hv = f3(0.0f, 0.0f, 0.0f);
    st.S.hn = 0.0f; st.S.ws = 0.0f;
    const TpProj pr = temporal_project(P, st.d, P.depth[p]);
    TpMoments none;
    if (pr.ok) st.S = temporal_gather<false, false>(P, p, p3, pr, none);
    st.valid_S = pr.ok && st.S.ws > 0.015625f;
    st.tries = P.bounces[p] >= P.min_bounces && P.path_depth[p] > 0.0f; // (false for NaN)
    return st;
}

// Pixel (x, y), inside the image: everything after the ballot.  any_tries: some lane of the pixel's wave tries V (wave-uniform; a wave in
// which none does skips the second gather and the choice as one branch).  st is read only in a call with a history.
template <bool CLAMP>
__device__ __forceinline__ TpFlags temporal_dual_finish(const TpDualParams& P, const int x, const int y, const TpDualState& st, const bool any_tries)
{
    const size_t p = (size_t)y * P.width + (size_t)x, p3 = p * 3;
    TpFlags fl = {};
    TpPixel o = temporal_reset<false>(P, p3);
    if (P.pcolor) {
        TpTaps T = st.S;
        bool valid = st.valid_S;
        TpMoments none;
        none.h1 = f3(0.0f, 0.0f, 0.0f); none.h2 = f3(0.0f, 0.0f, 0.0f);
        TpBox box = temporal_no_box();
        int box_radius = 0; // the radius `box` holds the sums of (0: none yet)
        if (any_tries) {
            if (st.tries) {
                fl.tried = true;
                const TpProj pr = temporal_project(P, st.d, P.path_depth[p]);
                if (pr.ok) {
                    const TpTaps V = temporal_gather<true, false>(P, p, p3, pr, none);
                    if (V.ws > 0.015625f) {
                        box = temporal_box(P, x, y, P.dual_radius);
                        box_radius = P.dual_radius;
                        if (temporal_takes_virtual(st.valid_S, st.S, V, box)) { T = V; valid = true; fl.took_V = true; }
                    }
                }
            }
        }
        if (valid) {
            fl.took = true;
            temporal_blend<CLAMP, false>(P, x, y, T, none, box, box_radius == P.radius, o, fl.clamped); // (the same sums, bit for bit, when the radii agree)
        }
    }
    temporal_write<false>(P, p, p3, o);
    return fl;
}

} // namespace crtk
#endif
