// cudaraytracing_amd/csrc/crt_temporal.h -- the parameter blocks of the temporal pass and the per-pixel arithmetic of its dual-reprojection
// form (crt_temporal_dual, contract: include/crt.h; kernels and host code: crt_temporal.hip).  A pixel of a planar mirror shows two things:
// its own shading, which moves with the surface, and the mirrored scene, which moves with its virtual image -- the point at path_depth
// along the pixel's camera ray.  The pass fetches a history through each (candidate S: crt_temporal's taps; candidate V: the same taps
// keyed on the specular planes) and blends the one that lies nearer the mean of the current frame's colours around the pixel.
//   temporal_dual_begin    the pixel's ray, candidate S, and whether the pixel tries V
//   temporal_dual_finish   candidate V and the choice (behind the caller's wave-uniform `any lane tries`), the clamp, the blend, the outputs
// Between the two the kernel holds one ballot; a caller without waves passes the pixel's own `tries`.
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
    int radius;                               // k_temporal<true, *> only: crt_temporal_clamp
    float gamma;
    const float* pm1; const float* pm2;       // k_temporal<*, true> only: the history's moment planes (null without a history)
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
// The sums of the current colour around a pixel (crt_temporal_clamped's s1, s2, cnt)
struct TpBox { F3 s1, s2; float cnt; };
// What temporal_dual_begin hands to temporal_dual_finish
struct TpDualState {
    F3 d;          // the pixel-centre camera ray
    TpTaps S;
    bool valid_S;  // ok && ws_S > 0.015625f
    bool tries;    // a history is given, bounces(p) >= min_bounces and path_depth(p) > 0
};
// What a pixel did, for the counts
struct TpDualFlags { bool took, clamped, tried, took_V; };

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

// The four bilinear taps of a projection that is ok.  VIRTUAL false: crt_temporal's tap test (first-hit depth, normal, id).  VIRTUAL true:
// the tap must itself be a mirror pixel (bounces >= min_bounces, path_depth > 0), its path_depth must agree with tp, its last normal
// (if given) with the pixel's, and its first-hit id (if given) must be the pixel's: the same mirror.  Every tap is tested against the
// image before anything is read at it.
template <bool VIRTUAL>
__device__ __forceinline__ TpTaps temporal_gather(const TpDualParams& P, const size_t p, const TpProj& pr)
{
    const int W = (int)P.width, H = (int)P.height;
    TpTaps t;
    t.hc = f3(0.0f, 0.0f, 0.0f); t.hv = f3(0.0f, 0.0f, 0.0f);
    t.hn = 0.0f; t.ws = 0.0f;
    const float flx = floorf(pr.fx), fly = floorf(pr.fy);
    const float wx = pr.fx - flx, wy = pr.fy - fly;
    const int x0 = (int)flx, y0 = (int)fly; // -1 .. W - 1, -1 .. H - 1
    const float tol = P.depth_tol * pr.tp;
    const float* const cn = VIRTUAL ? P.last_normal : P.normal;
    const float* const pn = VIRTUAL ? P.plast_normal : P.pnormal;
    const float* const pdist = VIRTUAL ? P.ppath_depth : P.pdepth;
    F3 n = f3(0.0f, 0.0f, 0.0f);
    if (cn) n = f3(cn[p * 3], cn[p * 3 + 1], cn[p * 3 + 2]);
    const int32_t idp = P.id ? P.id[p] : 0;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int qy = y0 + j;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int qx = x0 + i;
            if (qx < 0 || qx >= W) continue;
            const size_t q = (size_t)qy * P.width + (size_t)qx;
            if (VIRTUAL && !(P.pbounces[q] >= P.min_bounces)) continue;
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
            t.hn = t.hn + P.phistory[q] * b;
            t.ws = t.ws + b;
        }
    }
    return t;
}

// sums of the current colour and its squares around (x, y); every tap is tested against the image, so every read is inside it
__device__ __forceinline__ TpBox temporal_box(const TpParams& P, const int x, const int y, const int radius)
{
    const int W = (int)P.width, H = (int)P.height;
    TpBox b;
    b.s1 = f3(0.0f, 0.0f, 0.0f); b.s2 = f3(0.0f, 0.0f, 0.0f);
    b.cnt = 0.0f;
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

// Pixel (x, y), inside the image, of a call with a history: its ray, candidate S, whether it tries V
__device__ __forceinline__ TpDualState temporal_dual_begin(const TpDualParams& P, const int x, const int y)
{
    const size_t p = (size_t)y * P.width + (size_t)x;
    TpDualState st;
    st.d = temporal_ray(P, x, y);
    st.S.hc = f3(0.0f, 0.0f, 0.0f); st.S.hv = f3(0.0f, 0.0f, 0.0f);
    st.S.hn = 0.0f; st.S.ws = 0.0f;
    const TpProj pr = temporal_project(P, st.d, P.depth[p]);
    if (pr.ok) st.S = temporal_gather<false>(P, p, pr);
    st.valid_S = pr.ok && st.S.ws > 0.015625f;
    st.tries = P.bounces[p] >= P.min_bounces && P.path_depth[p] > 0.0f; // (false for NaN)
    return st;
}

// Pixel (x, y), inside the image: everything after the ballot.  any_tries: some lane of the pixel's wave tries V (wave-uniform; a wave in
// which none does skips the second gather and the choice as one branch).  st is read only in a call with a history.
template <bool CLAMP>
__device__ __forceinline__ TpDualFlags temporal_dual_finish(const TpDualParams& P, const int x, const int y, const TpDualState& st, const bool any_tries)
{
    const size_t p = (size_t)y * P.width + (size_t)x;
    TpDualFlags fl;
    fl.took = false; fl.clamped = false; fl.tried = false; fl.took_V = false;
    const F3 c = f3(P.color[p * 3], P.color[p * 3 + 1], P.color[p * 3 + 2]);
    F3 v = f3(0.0f, 0.0f, 0.0f);
    if (P.variance) v = f3(P.variance[p * 3], P.variance[p * 3 + 1], P.variance[p * 3 + 2]);
    F3 oc = c, ov = v;
    float oh = 1.0f;
    if (P.pcolor) {
        TpTaps T = st.S;
        bool valid = st.valid_S;
        TpBox box;
        box.s1 = f3(0.0f, 0.0f, 0.0f); box.s2 = f3(0.0f, 0.0f, 0.0f);
        box.cnt = 0.0f;
        int box_radius = 0; // the radius `box` holds the sums of (0: none yet)
        if (any_tries) {
            if (st.tries) {
                fl.tried = true;
                const TpProj pr = temporal_project(P, st.d, P.path_depth[p]);
                if (pr.ok) {
                    const TpTaps V = temporal_gather<true>(P, p, pr);
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
            const float hn = T.hn / T.ws;
            oh = hn + 1;
            float a = 1 / oh;
            a = a < P.alpha_min ? P.alpha_min : a;
            const float k = 1 - a;
            if (CLAMP) {
                if (box_radius != P.radius) box = temporal_box(P, x, y, P.radius); // (the same sums, bit for bit, when the radii agree)
            }
            oc = f3(history_channel<CLAMP>(T.hc.x, T.ws, box.s1.x, box.s2.x, box.cnt, P.gamma, fl.clamped) * k + c.x * a,
                    history_channel<CLAMP>(T.hc.y, T.ws, box.s1.y, box.s2.y, box.cnt, P.gamma, fl.clamped) * k + c.y * a,
                    history_channel<CLAMP>(T.hc.z, T.ws, box.s1.z, box.s2.z, box.cnt, P.gamma, fl.clamped) * k + c.z * a);
            if (P.variance) {
                const float kk = k * k, aa = a * a;
                ov = f3((T.hv.x / T.ws) * kk + v.x * aa, (T.hv.y / T.ws) * kk + v.y * aa, (T.hv.z / T.ws) * kk + v.z * aa);
            }
        }
    }
    write_color(P, p, true, oc);
    if (P.out_variance) { P.out_variance[p * 3] = ov.x; P.out_variance[p * 3 + 1] = ov.y; P.out_variance[p * 3 + 2] = ov.z; }
    P.out_history[p] = oh;
    return fl;
}

} // namespace crtk
#endif
