// cudaraytracing_amd/csrc/crt_mega3_logic.h -- the path logic of k_mega3: how a ray is started and routed, what the three logic phases LA / LB / LC
// (and crt_intersect's form of LC) do with a finished ray, the backward recursion over the vertex records.  Included by crt_mega3.hip only.
#ifndef CRT_MEGA3_LOGIC_H
#define CRT_MEGA3_LOGIC_H
#include "crt_mega3_math.h"
#include "crt_mega3_wave.h"

namespace crtk {

struct NewRay {
    F3 o, d;
    float tl;
    uint32_t kind, flags;
};


// Where a ray goes once its traversal is over: a next-event sample to LA (LB after the last one of its vertex), a probe
// or a closest-hit ray that found a surface to LA, a closest-hit ray that found nothing to LC.
template <bool QUERY = false>
__device__ __forceinline__ uint32_t route_done(uint32_t rec_flags)
{
    if (QUERY) return PH3_LC;
    return ((rec_flags >> RR_ROUTE_SHIFT) & 3u) + (uint32_t)PH3_LA;
}
// the route bits of a new ray's record (NewRay flags -> record flags)
__device__ __forceinline__ uint32_t route_bits(uint32_t nr_flags)
{
    const uint32_t r = (nr_flags & RF_SHADOW) ? ((nr_flags & RF_LAST) ? 1u : 0u) : ((nr_flags & RF_PROBE) ? 0u : 2u);
    return r << RR_ROUTE_SHIFT;
}


// Writes the new ray into the pool record `id` and returns its first phase.
template <int MODE, bool QUERY = false, class LDS = Pool3Lds, bool IMPL = false>
__device__ __forceinline__ uint32_t start_ray(const DevScene& sc, LDS& S, uint32_t id, const NewRay& nr, PathCounters& cnt, const bool force_exact,
                                              bool& enters_exact)
{
    cnt.rays++;
    cnt.shadow += (nr.flags & RF_SHADOW) ? 1u : 0u;
    cnt.probe += (nr.flags & RF_PROBE) ? 1u : 0u;
    const F3 inv = inv3_exact(nr.d); // 1 / d (Ray.cuh:14)
    uint32_t flags = (nr.flags & ~(RF_SKIP | RF_SHADOW | RF_LAST | RF_PROBE)) | route_bits(nr.flags);
    // rays with a zero / denormal direction component can put NaNs into the slab test; they walk the reference
    // topology, whose box tests are the reference's own (crt_accel.h)
    // The 4-wide step (slab_quad_pruned) needs every plane distance (plane - o) * (1/d) of the tree to be FINITE: then no operand of
    // its v_max3 / v_min3 is a NaN, "+inf" can only mean "missed", and "no bound" can be any value >= FLT_MAX.  |plane - o| <=
    // coord_max + max |o|, so a product of that with max |1/d| at or below 2^126 cannot overflow (two roundings of 2^-24 on the way);
    // the comparison is false for a NaN anywhere and for an infinite origin, 1/d or scene coordinate.  A finite d keeps 1/d away from 0.
    const float max_o = __builtin_elementwise_maximum(__builtin_elementwise_maximum(absf(nr.o.x), absf(nr.o.y)), absf(nr.o.z));
    const float max_inv = __builtin_elementwise_maximum(__builtin_elementwise_maximum(absf(inv.x), absf(inv.y)), absf(inv.z));
    const bool finite = ((sc.coord_max + max_o) * max_inv <= 0x1p126f) & finite3(nr.d.x, nr.d.y, nr.d.z);
    if (MODE == 1 || !finite || force_exact) flags |= RF_EXACT;
    // (MODE 0 / 2: a ray that is not RF_EXACT walks the 4-wide tree)
    const int ref = (MODE != 1 && finite && !force_exact) ? (IMPL ? sc.root4i : sc.root4) : sc.root3_exact; // (IMPL: the tree without its rows of refs, visit_front)
    bool answered = false;
    float T = FLT_MAX;
    if (MODE != 1 && nr.kind == RAY_SHADOW) { // REFERENCE mode resolves shadow rays with the full closest-hit query, as blocked() does
        flags |= RF_ANYHIT;
        T = nr.tl;
        // a NaN or -inf limit can never be "blocked"; +inf is blocked by any hit
        answered = !(nr.tl == nr.tl) || nr.tl == -pinf() || (nr.flags & RF_SKIP) != 0;
    }
    if constexpr (LDS::DEC) {
        static_assert(!LDS::DEC || MODE == 2, "decoupled leaves: CRT_TRAVERSAL_EXACT");
        // (a scene that is one leaf has no inner node to start at: its rays take the reference-arithmetic arm, which hands leaf refs
        // to the queue one by one)
        if (ref < 0) flags |= RF_EXACT;
        S.A[id] = make_float4(nr.o.x, nr.o.y, nr.o.z, (flags & RF_ANYHIT) ? T : pinf());
        S.B[id] = make_float4(nr.d.x, nr.d.y, nr.d.z, __int_as_float(ref));
        S.best[id] = (unsigned long long)0x7f7fffffu << 32; // (FLT_MAX, no triangle)
        S.D[id] = flags;
        enters_exact = false;
        if (answered) return route_done<QUERY>(flags);
        enters_exact = (flags & RF_EXACT) != 0;
        return PH3_INNER;
    } else {
    S.A[id] = make_float4(nr.o.x, nr.o.y, nr.o.z, T);
    S.B[id] = make_float4(nr.d.x, nr.d.y, nr.d.z, __int_as_float(-1));
    S.node[id] = ref;
    S.D[id] = flags;
    enters_exact = false;
    if (answered) return route_done<QUERY>(flags);
    enters_exact = MODE != 1 && (flags & RF_EXACT) != 0; // (counted by the caller: the traversal steps of a pool without such rays skip their handling)
    return ref >= 0 ? PH3_INNER : PH3_LEAF;
    }
}

// DEC: the answer of a finished ray as the logic phases read it from the non-DEC record (A.w = distance, B.w = triangle)
template <class LDS>
__device__ __forceinline__ void ray_result(LDS& S, const uint32_t id, float4& qa, float4& qb)
{
    qa = S.A[id]; qb = S.B[id];
    if constexpr (LDS::DEC) {
        const unsigned long long b = S.best[id];
        qa.w = __uint_as_float((uint32_t)(b >> 32));
        qb.w = __uint_as_float(~(uint32_t)b);
    }
}
// DEC: where a complete ray goes (route_done); a closest-hit ray that has found a surface goes to LA instead of LC
template <bool QUERY>
__device__ __forceinline__ uint32_t route_complete(const uint32_t rec_flags, const bool has_hit)
{
    if (QUERY) return PH3_LC;
    const uint32_t r = (rec_flags >> RR_ROUTE_SHIFT) & 3u;
    return (has_hit ? (r & 1u) : r) + (uint32_t)PH3_LA;
}


#define ST_TL_INF (1u << 12) /* state word of the la plane, bits 12 .. 15 are free: the in-flight next-event ray's limit is +inf (shadow_blocked_bit) */

// Backward recursion over k_mega3's vertex records, deepest first (Render.cuh:238-326; crt_path.h: finish_path is the wavefront pipeline's,
// seed_emitter, seed_direct and indirect_step are both's).  Vertex j of a path that went ON from it has  rec_a[j] = (L_dir.xyz, bits(triangle-row word:
// material | flags)), written by LB when the roulette lets the path continue, and  rec_c[j] = cos to vertex j + 1, written when that
// vertex is found (rec_b[j].xyz, the direction that arrived at j, is written for SPECULAR vertices only: nothing else reads it).  The
// deepest vertex has no record: its L_dir arrives in the la plane (`have_ld`) when the path stopped there, is rec_a's when the ray that left
// it found nothing, and is not needed when it is an emitter.  Against one 16-byte record store more per vertex and one per path that stops.
__device__ __forceinline__ F3 finish_path_m3(const LParams& P, const Tables<false>& tb, const uint32_t slot, const int deepest, const bool emissive, const F3 ke,
                                            const bool have_ld, const F3 ld)
{
    const Pool& pl = P.pool;
    if (deepest < 0) return f3(0.0f, 0.0f, 0.0f);
    F3 L;
    if (emissive) L = seed_emitter(deepest, ke);
    else if (have_ld) L = seed_direct(ld);
    else {
        const float4 a = gld_rec(&pl.rec_a[(size_t)deepest * pl.n + slot]);
        L = seed_direct(f3(a.x, a.y, a.z));
    }
    // (the loads of CRT_FINISH_PF vertices are fetched together, as in finish_path)
    for (int v = deepest - 1; v >= 0; v -= CRT_FINISH_PF) {
        float4 a[CRT_FINISH_PF], fm[CRT_FINISH_PF];
        float cs[CRT_FINISH_PF];
#pragma unroll
        for (int j = 0; j < CRT_FINISH_PF; j++) {
            const int vj = v - j > 0 ? v - j : 0;
            a[j] = gld_rec(&pl.rec_a[(size_t)vj * pl.n + slot]);
            cs[j] = gld(&pl.rec_c[(size_t)vj * pl.n + slot]);
        }
#pragma unroll
        for (int j = 0; j < CRT_FINISH_PF; j++) fm[j] = mat_row(tb, TNM_MAT(__float_as_uint(a[j].w)), 0);
#pragma unroll
        for (int j = 0; j < CRT_FINISH_PF; j++) {
            if (v - j >= 0) L = indirect_step(L, f3(fm[j].x, fm[j].y, fm[j].z), cs[j], P.p_rr, f3(a[j].x, a[j].y, a[j].z));
        }
    }
    return L;
}


// LA: consumes the result of a next-event sample that is not the last one of its vertex, of a closest-hit ray
// that found a surface, or of a probe ray; enters the vertex if it is new; sets up the next next-event sample.
// Returns PH3_NONE when a ray was emitted into nr, else the phase the path has to visit instead.
template <int MODE, bool RING = false>
__device__ __forceinline__ uint32_t logic_A(const LParams& P, const Tables<false>& tb, const uint32_t g, const float4 qa, const float4 qb, NewRay& nr,
                                            PathCounters& cnt, const bool trace_all)
{
    const DevScene& sc = P.sc;
    const Pool& pl = P.pool;
    // The phase is a chain of dependent loads (path planes -> triangle / material / light tables -> light triangle), and a wave
    // that waits issues nothing: everything whose address is known is fetched up front, needed by this lane's stage or not.
    //   round 1: the path planes and the triangle record of the hit (the new vertex, if this ray found one)
    // TRI_CC (round 6, every mode but REFERENCE): the vertex's triangle rides in cc.w -- cc is written with every next-event sample and read
    // by every visit anyway -- instead of a store of its own into the id plane at every vertex; the limit of the sample's ray, which was
    // there, is needed as "is +inf" only (shadow_blocked) and is a bit of the state word.  REFERENCE compares the limit with the nearest
    // hit's distance and keeps the round-5 planes.  (docs/experiments.md 6.12: the store of the vertex position that went with it was the
    // gain, C2 75.8 -> 73.6 ms; this one is level in time and takes 6.7 % off the bytes written.)
    constexpr bool TRI_CC = MODE != 1;
    const float4 la = gld(&pl.la[g]);
    const uint4 idv = load_path_id<RING, !TRI_CC>(P, g);
    const float4 cc = gld(&pl.cc[g]); // pending next-event contribution; .w = bits(triangle of the vertex the samples belong to) (REFERENCE: distance to the light sample)
    const uint32_t st = __float_as_uint(la.w);
    const uint32_t stage = (st >> 8) & 15u;
    // (a path's first visit -- its camera ray found vertex 0 -- has no vertex in the planes yet: cc.w is what the slot's last path left, or
    // never written; the speculative row is then row 0 and is not used)
    const uint32_t vtri_old = TRI_CC ? ((st & 0xfffu) == ((uint32_t)ST_HIT << 8) ? 0u : __float_as_uint(cc.w)) : idv.w;
    const float4 vn = gld(&sc.tri_nm[vtri_old]); // (normal, material) of the vertex in the planes: from its triangle
    const float res_t = qa.w;
    const int res_tri = __float_as_int(qb.w);
    const float4 gq_hit = gld(&sc.tri_nm[res_tri >= 0 ? res_tri : 0]);
    //   round 2: material rows of the vertex the samples belong to after this visit (the new one for ST_HIT), row 1 of the
    //   vertex the ray left (specular flag, ST_HIT), and the light of the sample that is set up below
    //   (the material word of a slot's very first vertex comes from row 0, see vtri_old: the index is clamped into the table all the same)
    // (round 6: "is an emitter" / "is SPECULAR" ride in the two top bits of the triangle row's material word -- rows 1 of two materials were
    // fetched for those two bits alone, and what bounds this kernel is the NUMBER of vector-memory instructions)
    // (the material word of the samples' vertex in the id plane's free second word, so that its BSDF row is fetched WITH the triangle row instead
    // of after it, was measured in round 6: C2 +0.8 % -- one more store per vertex, and the round it saves is not the phase's last)
    const uint32_t mat_old = min(TNM_MAT(__float_as_uint(vn.w)), P.n_mats - 1u);
    const uint32_t mat_cur = stage == ST_HIT ? TNM_MAT(__float_as_uint(gq_hit.w)) : mat_old;
    uint32_t tnm_cur = stage == ST_HIT ? __float_as_uint(gq_hit.w) : __float_as_uint(vn.w);
    float4 m0_cur = mat_row(tb, mat_cur, 0);
    const uint32_t n_nee = (uint32_t)(sc.n_lights * P.lsn);
    const uint32_t q_next = stage == ST_SHADOW ? (st >> 16) + 1 : 0u;
    uint4 lg_next = make_uint4(0u, 1u, 0u, 0u);
    // A scene with ONE light has its table entry fetched through the scalar cache: one vector load per visit fewer (round 6: C2 72.11 -> 71.75 ms).
    // (The eight rows of a light of <= 2 triangles -- the quad of a Cornell box -- fetched the same way and picked per lane: C2 level, and
    // veach-mis, which does not take that path, +1.2 % from the second copy of the set-up code; not kept.)
    if (n_nee > 0) {
        if (sc.n_lights == 1) {
            const crt_u4v_ l0_ = *(const __attribute__((address_space(4))) crt_u4v_*)tb.lights;
            lg_next = make_uint4(l0_.x, l0_.y, l0_.z, l0_.w);
        } else lg_next = gld(&tb.lights[fast_div(q_next < n_nee ? q_next : 0u, P.lsn_div.m, P.lsn_div.sh)]);
    }
    Lane s;
    s.depth = st & 255u; s.q = st >> 16; s.stage = stage;
    s.Ld = f3(la.x, la.y, la.z);
    s.nrm = f3(vn.x, vn.y, vn.z); s.mat = TNM_MAT(__float_as_uint(vn.w));
    s.pixel_index = idv.x; s.k = idv.y; s.item = idv.z;
    s.ro = f3(qa.x, qa.y, qa.z); s.tl = 0.0f;
    s.rd = f3(qb.x, qb.y, qb.z);
    s.pos = s.ro; s.vtri = vtri_old; s.c = f3(0.0f, 0.0f, 0.0f); s.kind = RAY_NONE;
    bool do_enter = false;
    if (stage == ST_SHADOW) {
        // visibility of next-event sample q (Render.cuh:19-27, :272-284); shadow rays start at the vertex: s.pos == s.ro
        const bool blocked = TRI_CC ? shadow_blocked_bit((st & ST_TL_INF) != 0u, res_tri) : shadow_blocked<MODE>(cc.w, res_t, res_tri);
        if (!blocked) s.Ld = add3(s.Ld, f3(cc.x, cc.y, cc.z));
        s.q++;
    } else if (stage == ST_HIT) {
        // the camera / bounce ray found vertex `depth` (Render.cuh:207-213)
        const F3 pos = add3(s.ro, scalel3(res_t, s.rd)); // DeviceTriangle.cuh:50
        do_enter = true;
        if (s.depth > 0) {
            // the previous vertex (vn: its triangle's row) is not the deepest one: cosine of its indirect term (Render.cuh:291)
            const size_t pr = (size_t)(s.depth - 1) * pl.n + g;
            const F3 pn = s.nrm;
            const float cos_prev = cos_to_next(s.ro, pos, pn); // prev.pos == origin of this ray
            gst_rec(&pl.rec_c[pr], cos_prev);
            if (TNM_SPECULAR(__float_as_uint(vn.w))) { // SPECULAR: emitter probe, Render.cuh:294-303
                const float ns = mat_row(tb, s.mat, 0).w;
                const float4 pb = gld_rec(&pl.rec_b[pr]); // direction that arrived at the previous vertex
                const F3 refd = probe_dir(P.seed, s.pixel_index, s.k, s.depth - 1, ns, f3(pb.x, pb.y, pb.z), pn);
                // the probe leaves from prev.pos (= this ray's origin); the bounce direction waits in rec_b[depth]
                gst_rec(&pl.rec_b[(size_t)s.depth * pl.n + g], make_float4(s.rd.x, s.rd.y, s.rd.z, 0.0f));
                gst(&pl.vx[g], make_float4(pos.x, pos.y, pos.z, __int_as_float(res_tri)));
                gst(&pl.la[g], make_float4(s.Ld.x, s.Ld.y, s.Ld.z, __uint_as_float(s.depth | ((uint32_t)ST_PROBE << 8) | (s.q << 16))));
                nr.o = s.ro; nr.d = unit3(refd); /* Ray.cuh:13 */ nr.tl = 0.0f; nr.kind = RAY_CLOSEST; nr.flags = RF_PROBE;
                return PH3_NONE;
            }
        }
        s.pos = pos; s.vtri = (uint32_t)res_tri;
    } else { // ST_PROBE: the probe ray of vertex depth-1 (Render.cuh:304-313); vn still describes that vertex
        const float4 vx = gld(&pl.vx[g]);
        s.pos = f3(vx.x, vx.y, vx.z); s.vtri = __float_as_uint(vx.w);
        if (res_tri >= 0) {
            const int hmat = gld(&sc.tri_mat[res_tri]);
            const float4 h1 = mat_row(tb, hmat, 1);
            if (__float_as_uint(h1.w) & 1u) {
                const float4 h2 = mat_row(tb, hmat, 2);
                const size_t pr = (size_t)(s.depth - 1) * pl.n + g;
                const F3 pn = s.nrm;
                const float4 pm0 = mat_row(tb, s.mat, 0), pm1 = mat_row(tb, s.mat, 1);
                const F3 temp = probe_term(pn, f3(pm1.x, pm1.y, pm1.z), f3(h2.x, h2.y, h2.z), s.ro, s.rd, res_t, pm0.w); // the probe's origin is prev.pos
                float4 a = gld_rec(&pl.rec_a[pr]);
                a.x = a.x + temp.x; a.y = a.y + temp.y; a.z = a.z + temp.z;
                gst_rec(&pl.rec_a[pr], a);
            }
        }
        const float4 pb = gld_rec(&pl.rec_b[(size_t)s.depth * pl.n + g]); // the bounce direction that found the current vertex
        s.rd = f3(pb.x, pb.y, pb.z);
        do_enter = true;
    }
    if (do_enter) { // a new vertex (pos, vtri) at `depth`, reached along s.rd
        float4 gq = gq_hit;
        if (stage == ST_PROBE) { // the vertex was found by the ray before the probe: its triangle waits in the vx plane
            gq = gld(&sc.tri_nm[s.vtri]);
            m0_cur = mat_row(tb, TNM_MAT(__float_as_uint(gq.w)), 0); tnm_cur = __float_as_uint(gq.w);
        }
        s.nrm = f3(gq.x, gq.y, gq.z);
        s.mat = TNM_MAT(__float_as_uint(gq.w));
        // (the direction that arrived: read by the probe of a SPECULAR vertex when the next vertex is found, by nothing else)
        if (TNM_SPECULAR(tnm_cur)) gst_rec(&pl.rec_b[(size_t)s.depth * pl.n + g], make_float4(s.rd.x, s.rd.y, s.rd.z, 0.0f));
        // (round 6: the vertex position is not written to the vx plane any more -- LB takes it from the slot's ray record, which is a
        // next-event ray of this vertex or, for a vertex without one, is given the position below.  The plane lives on for the probe rays.)
        if (!TRI_CC) store_path_tri(P, g, s.vtri);
        if (TNM_EMITTER(tnm_cur)) { // emitter: the path ends here (Render.cuh:210); TRI_CC: LC finds the emitter's triangle in la.x
            gst(&pl.la[g], make_float4(TRI_CC ? __uint_as_float(s.vtri) : 0.0f, 0.0f, 0.0f, __uint_as_float(s.depth | ((uint32_t)ST_FIN << 8) | (1u << 16))));
            return PH3_LC;
        }
        s.Ld = f3(0.0f, 0.0f, 0.0f);
        s.q = 0;
        if (n_nee == 0) {
            gst(&pl.la[g], make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(s.depth | ((uint32_t)ST_NEED << 8))));
            if (TRI_CC) gst(&pl.cc[g].w, __uint_as_float(s.vtri)); // (a vertex without a sample: its triangle for LB and for the next vertex's visit)
            nr.o = s.pos; // (no ray: the caller puts the position into the slot's ray record for LB)
            return PH3_LB;
        }
    }
    // next-event samples of the current vertex, from q on.  The reference traces every shadow ray and then adds
    // Le (.) f_r * cos * cos' * ... to L_dir if it is unblocked (Render.cuh:272-284).  When that contribution is exactly
    // zero (the surface or the light faces away: the cosines are clamped to 0; a black BSDF) the addition is the identity
    // whatever the ray finds -- L_dir is never -0 -- so the FAST traversal answers the sample without tracing it.  It still
    // counts as a ray of the reference (`rays`, `shadow_rays`); `rays_untraced` says how many there were.  A NaN contribution
    // fails the comparison and is traced.  (CRT_TRAVERSAL_REFERENCE traces everything: its counters are the reference's visit set.)
    // The next sample of such a lane is set up right here while enough lanes of the batch need it (setup_shadow is the most
    // expensive section of the phase and the others wait); the last few stragglers are instead handed to start_ray as
    // "answered" (RF_SKIP) and go back to the ring of their consumer, which adds the zero contribution.
    constexpr int LA_LOOP_MIN = 16;
    const float4 m0 = m0_cur;
    bool skip;
    for (bool first = true;; first = false) {
        if (first) setup_shadow_lg(P, s, f3(m0.x, m0.y, m0.z), lg_next); // (s.q == q_next: the light entry is already here)
        else setup_shadow(P, tb, s, f3(m0.x, m0.y, m0.z));
        skip = MODE != 1 && !trace_all && (s.c.x == 0.0f && s.c.y == 0.0f && s.c.z == 0.0f);
        if (!skip) break;
        cnt.untraced++;
        if (__popcll(__builtin_amdgcn_ballot_w64(true)) < LA_LOOP_MIN) break; // (the lanes still in the loop are the ones that skip)
        cnt.rays++; cnt.shadow++;
        s.q++;
        if (s.q == n_nee) { // that was the last sample of the vertex: on to the roulette
            gst(&pl.la[g], make_float4(s.Ld.x, s.Ld.y, s.Ld.z, __uint_as_float(s.depth | ((uint32_t)ST_NEED << 8))));
            if (TRI_CC) gst(&pl.cc[g].w, __uint_as_float(s.vtri)); // (every sample of the vertex may have been answered here: none has written cc)
            nr.o = s.pos;
            return PH3_LB;
        }
    }
    gst(&pl.la[g], make_float4(s.Ld.x, s.Ld.y, s.Ld.z, __uint_as_float(s.depth | ((uint32_t)ST_SHADOW << 8) | (s.q << 16) | ((TRI_CC && s.tl == pinf()) ? ST_TL_INF : 0u))));
    gst(&pl.cc[g], make_float4(s.c.x, s.c.y, s.c.z, TRI_CC ? __uint_as_float(s.vtri) : s.tl));
    nr.o = s.ro; nr.d = s.rd; nr.tl = s.tl; nr.kind = RAY_SHADOW;
    nr.flags = RF_SHADOW | (s.q + 1 == n_nee ? RF_LAST : 0u) | (skip ? RF_SKIP : 0u);
    return PH3_NONE;
}

// LB: direct light of vertex `depth` is complete -> vertex record, Russian roulette, bounce (Render.cuh:210-228).
template <int MODE, bool RING = false>
__device__ __forceinline__ uint32_t logic_B(const LParams& P, const uint32_t g, const float4 qa, const float4 qb, NewRay& nr)
{
    const Pool& pl = P.pool;
    constexpr bool TRI_CC = MODE != 1; // (see logic_A)
    const float4 la = gld(&pl.la[g]);
    const uint4 idv = load_path_id<RING, !TRI_CC>(P, g);
    const float4 cc = gld(&pl.cc[g]); // (with the other planes, not after the stage is known: one round trip less, see logic_A)
    const uint32_t st = __float_as_uint(la.w);
    const uint32_t stage = (st >> 8) & 15u;
    uint32_t depth = st & 255u;
    F3 Ld = f3(la.x, la.y, la.z);
    if (stage == ST_SHADOW) { // the last next-event sample (Render.cuh:272-284)
        const bool blocked = TRI_CC ? shadow_blocked_bit((st & ST_TL_INF) != 0u, __float_as_int(qb.w)) : shadow_blocked<MODE>(cc.w, qa.w, __float_as_int(qb.w));
        if (!blocked) Ld = add3(Ld, f3(cc.x, cc.y, cc.z));
    }
    U4 rb;
    if (roulette(P.seed, idv.x, idv.y, depth, P.p_rr, rb)) { // the deepest vertex: its L_dir goes to LC in the la plane, it has no record (finish_path_m3)
        gst(&pl.la[g], make_float4(Ld.x, Ld.y, Ld.z, __uint_as_float(depth | ((uint32_t)ST_FIN << 8))));
        return PH3_LC;
    }
    // the vertex: the origin of the slot's last ray -- a next-event ray starts at its vertex (setup_shadow_lg) -- or what LA's caller put there
    const float4 vn = gld(&P.sc.tri_nm[TRI_CC ? __float_as_uint(cc.w) : idv.w]);
    const float4 vx = qa;
    gst_rec(&pl.rec_a[(size_t)depth * pl.n + g], make_float4(Ld.x, Ld.y, Ld.z, vn.w)); // the vertex's record: L_dir and its material (with the row's flag bits)
    const F3 ndir = bounce_dir(f3(vn.x, vn.y, vn.z), rb);
    // (leaving this store out -- the plane then still holds a state only LB consumes, which LA and LC can read as "the ray for vertex depth + 1
    // is in flight" -- was measured in round 6: C2 +0.4 %, veach-mis +0.3 %: LA's load of the line then misses the L2 the store had left it in)
    depth++;
    gst(&pl.la[g], make_float4(Ld.x, Ld.y, Ld.z, __uint_as_float(depth | ((uint32_t)ST_HIT << 8))));
    nr.o = f3(vx.x, vx.y, vx.z); nr.d = unit3(ndir); /* Ray.cuh:13 */ nr.tl = 0.0f; nr.kind = RAY_CLOSEST; nr.flags = 0;
    return PH3_NONE;
}

// LC: the path is complete (miss, emitter, roulette, stack full) -> backward recursion (Render.cuh:238-326), next
// work item and its camera ray (Render.cuh:344-347).  Returns LC_DEAD when the work items are exhausted (the ray slot dies), LC_RAY
// with the camera ray of a new path, or -- commit ring only -- LC_WAIT: the slot holds a work item it may not start yet and comes
// back to this phase.  fin_key: see ring_publish.
enum { LC_DEAD = 0, LC_RAY = 1, LC_WAIT = 2 };
template <int MODE, bool RING>
__device__ __forceinline__ int logic_C(const LParams& P, const Tables<false>& tb, const uint32_t g, PathCounters& cnt, NewRay& nr, uint32_t& fin_key)
{
    constexpr bool TRI_CC = MODE != 1; // (see logic_A: an emitter's triangle arrives in la.x)
    const Pool& pl = P.pool;
    const float4 la = gld(&pl.la[g]);
    const uint4 idv = load_path_id<RING, !TRI_CC>(P, g); // (with la, not after the stage is known: one round trip less, see logic_A)
    const uint32_t st = __float_as_uint(la.w);
    const uint32_t stage = (st >> 8) & 15u;
    const uint32_t depth = st & 255u;
    constexpr bool ring = RING;
    const bool waiting = ring && stage == ST_WAIT;
    // The next work item is asked for NOW -- one atomic on the wave's home cursor for all its lanes -- and looked at after the
    // backward recursion: the cursor's round trip hides behind the recursion's own loads (the earlier attempt read the answer with
    // a readfirstlane at once, which waits).  A home shard that has run dry (the end of a launch) falls back to grab_item below.
    const uint32_t home_ = RING ? blockIdx.x & (P.ring_shards - 1u) : blockIdx.x & (ITEM_SHARDS - 1);
    const uint32_t lo_ = home_ * P.items_per_shard, hi_ = min(lo_ + P.items_per_shard, P.n_items);
    const unsigned long long gmask_ = __ballot(!waiting);
    const int lane_ = threadIdx.x & 63;
    const uint32_t grank_ = (uint32_t)__popcll(gmask_ & ((1ull << lane_) - 1ull));
    unsigned int pre_base_ = 0;
    const bool pre_ok_ = lo_ < P.n_items && gmask_ != 0ull;
    if (pre_ok_ && lane_ == __ffsll((long long)gmask_) - 1) pre_base_ = __hip_atomic_fetch_add((CRT_GAS unsigned int*)(P.item_next + home_ * ITEM_STRIDE), (unsigned int)__popcll(gmask_), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t home_word_ = 0;
    if (RING) home_word_ = ring_load(P.ring_state + home_ * ITEM_STRIDE);
    if (stage != ST_NEW && !waiting) {
        int deepest = (int)depth;
        bool emissive = false;
        F3 ke = f3(0.0f, 0.0f, 0.0f);
        if (stage == ST_HIT) deepest = (int)depth - 1; // the ray that looked for vertex `depth` missed (Render.cuh:210)
        else if ((st >> 16) & 1u) {
            emissive = true;
            const float4 m2 = mat_row(tb, TNM_MAT(__float_as_uint(gld(&P.sc.tri_nm[TRI_CC ? __float_as_uint(la.x) : idv.w]).w)), 2);
            ke = f3(m2.x, m2.y, m2.z);
        }
        const F3 L = finish_path_m3(P, tb, g, deepest, emissive, ke, stage == ST_FIN && !emissive, f3(la.x, la.y, la.z));
        if (ring) {
            const uint32_t sh = fast_div(idv.z, P.items_per_shard_div.m, P.items_per_shard_div.sh), c = idv.z - sh * P.items_per_shard;
            const uint32_t s = fast_div(c, P.spsh_div.m, P.spsh_div.sh), rs = s & P.ring_mask;
            Rad3* Lr = P.L + (size_t)rs * P.ring_stride + (size_t)sh * P.spsh + (c - s * P.spsh);
            ring_store12(Lr, L.x, L.y, L.z);
            fin_key = (sh << 16) | rs;
        } else {
            // (ONE store -- three 4-byte ones until round 5, then a 16-byte one with a zero word: docs/experiments.md 6.14)
            store_radiance(&P.L[idv.z], L.x, L.y, L.z);
        }
    }
    bool first_ = pre_ok_ && !waiting;
    for (;;) {
        uint32_t item = ITEM_NONE;
        if (waiting) item = idv.z; // the item this slot was handed earlier
        else {
            if (first_) { // the answer of the atomic issued above (the leader is the first active lane)
                const unsigned long long idx_ = (unsigned long long)lo_ + (unsigned int)__builtin_amdgcn_readfirstlane((int)pre_base_) + grank_;
                if (idx_ < hi_) item = (uint32_t)idx_;
                first_ = false;
            }
            if (item == ITEM_NONE) item = RING ? grab_item_ring(P.item_next, P.items_per_shard, P.ring_shards, home_)
                                               : grab_item(P.item_next, P.items_per_shard, P.n_items, blockIdx.x & (ITEM_SHARDS - 1));
            if (item == ITEM_NONE) return LC_DEAD;
            if (P.item_list) { // the tail of every cursor shard is handed out "paths that stop at their first vertex last" (k_order_items)
                const uint32_t sh_ = fast_div(item, P.items_per_shard_div.m, P.items_per_shard_div.sh);
                const uint32_t slo_ = sh_ * P.items_per_shard, shi_ = min(slo_ + P.items_per_shard, P.n_items);
                const uint32_t wlo_ = shi_ - min(P.order_window, shi_ - slo_);
                // (agent-scope load, as k_order_items' stores: with plain accesses the FIRST frame of a render created after other renders of
                // the process came out with 10 - 400 work items of the 589 824 of a 96 x 64 x 96 frame never run -- their list entries read as
                // what an earlier kernel had left at the address -- in half of the runs once the launches' timing had changed; docs/experiments.md 6)
                if (item >= wlo_) item = __hip_atomic_load((CRT_GAS const unsigned int*)&P.item_list[sh_ * P.order_window + (item - wlo_)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        bool valid; uint32_t pi, pj, pixel_index, k;
        decode_item<RING>(P, item, pixel_index, k, valid, pi, pj);
        if (!valid) continue; // padding slot of a ragged tile: take another item
        if (ring && !ring_gate_open(P, item, home_, home_word_)) { // its sample's slot of the ring is not free yet: hold the item
            if (!waiting) {
                store_path_id<!TRI_CC>(P, g, item);
                gst(&pl.la[g], make_float4(0.0f, 0.0f, 0.0f, __uint_as_float((uint32_t)ST_WAIT << 8)));
            }
            return LC_WAIT;
        }
        cnt.paths++;
        if (!waiting) store_path_id<!TRI_CC>(P, g, item);
        const F3 wd = camera_dir(P, pixel_index, k, pi, pj);
        gst(&pl.la[g], make_float4(0.0f, 0.0f, 0.0f, __uint_as_float((uint32_t)ST_HIT << 8)));
        nr.o = f3(P.eye[0], P.eye[1], P.eye[2]); nr.d = unit3(wd); /* Ray.cuh:13 */ nr.tl = 0.0f; nr.kind = RAY_CLOSEST; nr.flags = 0;
        return LC_RAY;
    }
}

// crt_intersect's form of LC: the work items are query rays (origin, normalised direction); a finished ray's record holds
// the answer (T = distance or FLT_MAX, best triangle or -1), which goes to L[ray].  The rays walk exactly the traversal phases
// of the render (4-wide tree, packed pair tests, tie rule, pruning) -- DeviceBVH::intersect (DeviceBVH.cuh:128-170) per ray.
__device__ __forceinline__ bool query_C(const LParams& P, const uint32_t g, const float4 qa, const float4 qb, NewRay& nr)
{
    const Pool& pl = P.pool;
    const float4 la = gld(&pl.la[g]);
    const uint4 idv = load_path_id(P, g);
    if (((__float_as_uint(la.w) >> 8) & 15u) != ST_NEW) gst(&P.L4[idv.z], make_float4(qa.w, qb.w, 0.0f, 0.0f));
    const uint32_t item = grab_item(P.item_next, P.items_per_shard, P.n_items, blockIdx.x & (ITEM_SHARDS - 1));
    if (item == ITEM_NONE) return false;
    store_path_id(P, g, item);
    gst(&pl.la[g], make_float4(0.0f, 0.0f, 0.0f, __uint_as_float((uint32_t)ST_HIT << 8)));
    const float4 o = gld(&P.q_o[item]), d = gld(&P.q_d[item]);
    nr.o = f3(o.x, o.y, o.z); nr.d = f3(d.x, d.y, d.z); nr.tl = o.w; nr.kind = __float_as_uint(d.w); nr.flags = RF_QUERY;
    return true;
}

} // namespace crtk
#endif
