// cudaraytracing_amd/csrc/crt_mega3.hip -- k_mega3, the render kernel: one persistent launch per chunk of samples, path logic and traversal in the
// same waves, every wave the owner of a pool of rays in LDS (layouts, limits and tuning constants: crt_mega3.h; shared path logic: crt_path.h).
// This file holds the kernel itself -- the scheduler, the loop of alternating traversal steps, the dispatch to the named steps, the
// counters -- the launch of k_order_items (crt_item_order.h), the table of the kernel's instantiations and the tools/bbprof hook.  The steps live in headers that only this
// file includes: crt_mega3_math.h (box and triangle arithmetic), crt_mega3_wave.h (scalar helpers, the ring append, the -DCRT_STAMPS clock),
// crt_mega3_logic.h (start_ray, LA / LB / LC), crt_mega3_coupled.h and crt_mega3_decoupled.h (what the two forms of the traversal steps are made of).
// Replaces view_render_kernel / cast_ray_v2 / DeviceBVH::intersect (include/Render.cuh:199-354, include/DeviceBVH.cuh:87-170).
#include "crt_internal.h"
#include "crt_mega3_math.h"
#include "crt_mega3_wave.h"
#include "crt_mega3_logic.h"
#include "crt_mega3_coupled.h"
#include "crt_mega3_decoupled.h"
#include "crt_item_order.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

namespace crtk {

// Which combinations of k_mega3's template arguments exist: the kernel asserts it, and the table of instantiations below is every
// combination that passes.
constexpr bool mega3_legal(int MODE, bool STATS, bool ALL, bool QUERY, bool R16, bool RING, bool DEC, bool IMPL)
{
    return MODE >= 0 && MODE <= 2
        && (!IMPL || (DEC && R16))        // the tree without its rows of refs: decoupled leaves, 16-bit stack entries
        && !(RING && (QUERY || STATS))    // the commit ring is a render without counters
        && !(R16 && MODE == 1)            // CRT_TRAVERSAL_REFERENCE walks the 2-wide trees: 32-bit stack entries
        && (!DEC || MODE == 2)            // decoupled leaves: CRT_TRAVERSAL_EXACT
        && !(ALL && MODE == 1)            // REFERENCE traces every sample as it is: no instantiation of its own
        && !(QUERY && (STATS || ALL));    // the query form has no next-event samples and no traversal counters
}
// the pool of an instantiation
template <bool R16, bool RING, bool DEC> using Mega3Pool = typename std::conditional<DEC, Pool4LdsT<R16, RING>, Pool3LdsT<R16>>::type;

// ---- pieces of the kernel's body ----
// Macros, because they must be: each expands INSIDE k_mega3's body (and inside the arms it defines there) and names the locals it finds
// -- the ring counts qn[], the pool S, the batch's `lane`, `id`, `nph`, `on`, the counters dg_b / dg_l, the template parameter STATS.
// As functions that are handed those locals -- one by one, or as one struct of the wave's state -- they are optimised on their own
// before they are inlined, the kernel's values reach registers in another order, and the instruction streams of most of the 53
// instantiations change (what was tried, and what it moved: docs/experiments.md, "k_mega3 split by concern").  The ring append itself
// is a function (ring_append, crt_mega3_wave.h); these are its callers and the batch pop.

// appends the processed rays (lane active = `on`, ray `id`) to the ring of their new phase
#define PUSH3() _Pragma("unroll") for (int p = 0; p < PH3_N; p++) { const bool mine = nph == (uint32_t)p; ring_append<STATS>(S.rq(p), qn[p], mine, __ballot(mine), id); }
// after a traversal step: a ray goes on to an inner node or a leaf, or it is finished -- only then (one wave-uniform test
// for the three logic rings together) is its route worked out from the flag bits of its record
#define PUSH_TRAV() { if (on) nph = t_done ? route_done<QUERY>(t_flags) : (t_ref >= 0 ? PH3_INNER : PH3_LEAF); PUSH3() }
// takes the (up to) 64 newest rays of ring p
#define POP3(p)                                                                                                            \
    const int take = min(64, qn[p]);                                                                                       \
    if (STATS) { dg_b[p]++; dg_l[p] += (uint32_t)take; }                                                                   \
    const bool on = lane < take;                                                                                           \
    const uint32_t id = S.rq(p)[(uint32_t)(qn[p] - take) + (uint32_t)lane];                                                        \
    qn[p] -= take;                                                                                                         \
    const uint32_t g = base + id;                                                                                          \
    uint32_t nph = PH3_NONE;

// The logic phases read their parameters from the kernel-argument segment again, through a pointer the compiler cannot see
// through: parameters that are only needed there (camera, tiling, work-item cursors, pool planes ...) would otherwise be
// hoisted into scalar registers for the whole kernel and push the ring cursors of the traversal steps out into VGPR lanes.
#define LOGIC_PARAMS()                                                                                                     \
    const __attribute__((address_space(4))) char* ka_ = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr(); \
    asm volatile("" : "+s"(ka_));                                                                                          \
    union { LParams p; uint32_t w[sizeof(LParams) / 4]; } pu_;                                                             \
    {                                                                                                                      \
        const __attribute__((address_space(4))) uint32_t* src_ =                                                           \
            (const __attribute__((address_space(4))) uint32_t*)(ka_ + offsetof(MParams3, M) + offsetof(MParams, P));       \
        _Pragma("unroll") for (unsigned i_ = 0; i_ < sizeof(LParams) / 4; i_++) pu_.w[i_] = src_[i_];                      \
    }                                                                                                                      \
    const LParams& Pl = pu_.p;                                                                                             \
    Tables<false> tl;                                                                                                      \
    tl.mats = Pl.sc.mats; tl.lights = Pl.sc.lights;

// appends the lanes with `cond_` (ray `id`) to ring p_ (the decoupled steps: one ring at a time, LA / LB / LC only)
#define PUSH_ONE(p_, cond_) { const bool mine_ = (cond_); ring_append<STATS>(S.rq(p_), qn[p_], mine_, __builtin_amdgcn_ballot_w64(mine_), id); }

// ALL: every next-event sample is traced (CRT_FLAG_TRACE_ALL) -- its own instantiation, so that profiles of the default path
// are not mixed with it
// RING: the commit ring (in-order sum of the samples inside the launch, see ring_publish) -- its own instantiations: the kernels
// without it are, instruction for instruction, what they were before it existed
template <int MODE, bool STATS, bool ALL = false, bool QUERY = false, bool R16 = false, bool RING = false, bool DEC = false, bool IMPL = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(CRT_WAVES, CRT_WAVES))) void k_mega3(const MParams3 M3)
{
    static_assert(mega3_legal(MODE, STATS, ALL, QUERY, R16, RING, DEC, IMPL), "k_mega3: not an instantiation that exists (mega3_legal)");
    typedef Mega3Pool<R16, RING, DEC> LDS3;
    __shared__ LDS3 S;
    constexpr int QCAP = LDS3::QCAP;
    const MParams& M = M3.M;
    const LParams& P = M.P;
    const DevScene& sc = P.sc; // (one copy of the scene pointers in scalar registers: the logic phases use P.sc too)
    const Pool& pl = P.pool;
    const int lane = threadIdx.x;
    const uint32_t base = blockIdx.x * (uint32_t)LDS3::P; // first global slot of this wave's pool
    PathCounters cnt;
    cnt = PathCounters{};
    TravCounters tc;
    tc.inner = tc.leaf = tc.tests = tc.hits = 0;
    uint32_t max_sp = 0;
    int n_exact = 0; // rays on the reference-arithmetic path (RF_EXACT) that are in the traversal phases of this pool

    // ring state: wave-uniform scalars
    int qn[PH3_N]; // entries
#pragma unroll
    for (int p = 0; p < PH3_N; p++) qn[p] = 0;
    uint32_t dg_b[5] = {0, 0, 0, 0, 0}, dg_l[5] = {0, 0, 0, 0, 0}; // STATS: batches and rays per phase
    uint32_t dg_sp[6] = {0, 0, 0, 0, 0, 0};                         // STATS, per lane: inner steps that leave the stack deeper than 1 .. 6 entries
    uint32_t dg_ov[2] = {0, 0};                                     // STATS, per lane (DEC): visits taken back because the leaf queue was full (first visit: voided lanes; second visit: bailed, counted by its lanes)
    uint32_t lq_h = 0, lq_t = 0; // DEC: the leaf queue's head and tail, free-running (entries = tail - head, index = counter mod LEAFQ_CAP)
    Stamps stamps;
    if (RING && lane == 0) S.waitq = 0u;
    // every ray of the pool starts in LC with a path in stage NEW
    {
        // (readfirstlane: the value is wave-uniform, and left to itself the compiler may compute it -- and the LC ring's count that starts
        // from it -- in a vector register, which the scalar maxima of the scheduler cannot take)
        const int n_valid = __builtin_amdgcn_readfirstlane((int)min((uint32_t)LDS3::P, pl.n > base ? pl.n - base : 0u));
        for (int i = lane; i < n_valid; i += 64) {
            S.rq(PH3_LC)[i] = (uint8_t)i;
            pl.la[base + i] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float((uint32_t)ST_NEW << 8));
        }
        qn[PH3_LC] = n_valid;
    }

    for (;;) {
      int act;
      // The traversal steps -- nine of ten iterations -- are a loop of their own inside the scheduler loop: the register allocator
      // weighs a value by the depth of the loops that use it, and with all five phases at one depth it kept the (cold) inner loops of
      // the logic phases in registers and spilled the ring cursors and node pointers of the traversal steps (19 vector instructions
      // of spill / copy code per iteration: C2 106.6 -> 99.0 ms, veach-mis 99.4 -> 92.4 ms at spp 256).
      for (;;) {
        // ---- choose a phase: the ring with the fullest batch; among equals the logic phases first (they feed the traversal), then
        //      leaves, then inner nodes ----
        {
            // key = batch size * 8 + phase number (the phase numbers are the tie-break order)
            const int kC = min(qn[PH3_LC], 64) * 8 + PH3_LC, kA = min(qn[PH3_LA], 64) * 8 + PH3_LA, kB = min(qn[PH3_LB], 64) * 8 + PH3_LB;
            // (DEC: the leaf queue counts entries, not rays; with 64 or more it is the fullest there can be and wins over the inner ring)
            // (an inner step starts with fewer than LEAFQ_FIRST entries in the queue -- from that many on the leaf step goes first, here and
            // in the alternating loop -- and must find room for a reference-arithmetic batch, 64 entries appended outside the counted
            // ones, plus four entries, the least a 4-wide visit needs to keep one lane: otherwise it would take every lane back, for ever)
            const int nl_ = DEC ? (int)(lq_t - lq_h) : qn[PH3_LEAF];
            const int kL = ((DEC && nl_ >= LEAFQ_FIRST) ? 64 : min(nl_, 64)) * 8 + PH3_LEAF, kI = min(qn[PH3_INNER], 64) * 8 + PH3_INNER;
            // (s_max_i32 by hand: the compiler folds nested maxima of wave-uniform values into v_max3_i32 -- a vector instruction, plus
            // two moves in and a v_readfirstlane back)
            const int best = STATS ? max(max(max(kC, kA), max(kB, kL)), kI) // (the counting kernels keep more scalars: theirs may live in vector registers)
                                   : smax(smax(smax(kC, kA), smax(kB, kL)), kI);
            act = best < 8 ? PH3_NONE : (best & 7); // (best < 8: every ray of the pool is dead)
        }
        if (act > PH3_LEAF) break;
        // Rays with non-finite operands (RF_EXACT: a handful per frame) walk the 2-wide reference topology with the reference's own
        // box arithmetic and, in the 16-bit layout, keep their stack in the global area.  n_exact counts those in flight in this pool
        // (a wave-uniform scalar): while it is zero -- practically always -- the steps run in the form that has none of that handling.
        auto inner_arm = [&](auto may_exact_) __attribute__((always_inline)) {
            constexpr bool MAY_EXACT = decltype(may_exact_)::value;
            if constexpr (!DEC) {
            // ---- inner-node step: the child boxes, nearest child next, the other hit children pushed ----
            POP3(PH3_INNER)
            bool t_done = false;
            int t_ref = 0;
            uint32_t t_flags = 0;
            if (on) {
                const float4 qa = S.A[id], qbd = S.B[id];
                const uint32_t qd = S.D[id];
                int ref = S.node[id];
                // (EXACT, no ray of the batch on the reference-arithmetic path: the step takes the direction itself and forms 1 / d after its
                // loads are on their way)
                constexpr bool DIR_ = MODE == 2 && !MAY_EXACT;
                const F3 o = f3(qa.x, qa.y, qa.z), inv = DIR_ ? f3(qbd.x, qbd.y, qbd.z) : inv3_exact(f3(qbd.x, qbd.y, qbd.z));
                int sp = (int)(qd & 0xffu);
                // pruning bound: fixed by the light distance for shadow rays, shrinking with the best hit otherwise
                // (MODE 2 = CRT_TRAVERSAL_EXACT: the same traversal without this bound; +inf = no bound -- a box entered at +inf is still
                // a box the reference enters, which matters to the reference-arithmetic step of the rays with non-finite operands)
                const float bound = (MODE == 0 && (qd & (RF_ANYHIT | RF_HASHIT))) ? prune_bound(qa.w, o, inv) : pinf();
                bool done = false;
                if (MODE == 1) {
                    const float4 qb = S.B[id];
                    done = inner2_step<1, STATS>(sc, S, M3, id, g, o, inv, f3(qb.x, qb.y, qb.z), bound, ref, sp, tc, max_sp);
                } else if (!MAY_EXACT) {
                    done = inner4_step<STATS, CRT_SORT4(MODE), LDS3, DIR_>(sc, S, M3, id, g, o, inv, bound, ref, sp, tc, max_sp);
                } else {
                    const bool ex = (qd & RF_EXACT) != 0;
                    if (!ex) done = inner4_step<STATS, CRT_SORT4(MODE)>(sc, S, M3, id, g, o, inv, bound, ref, sp, tc, max_sp);
                    if (__builtin_amdgcn_ballot_w64(ex)) { // reference arithmetic on the reference topology
                        if (ex) {
                            const float4 qb = S.B[id];
                            done = inner2_step<0, STATS>(sc, S, M3, id, g, o, inv, f3(qb.x, qb.y, qb.z), bound, ref, sp, tc, max_sp);
                        }
                    }
                }
                S.node[id] = ref;
                S.D[id] = (qd & ~0xffu) | (uint32_t)sp;
                if (STATS) { for (int k = 0; k < 6; k++) dg_sp[k] += sp > k + 1 ? 1u : 0u; }
                if (STATS && done && (qd & RF_HASHIT)) tc.hits++; // (an any-hit ray that records a hit ends in the leaf step)
                t_done = done; t_ref = ref; t_flags = qd;
            }
            if (MAY_EXACT && MODE != 1) n_exact -= (int)__popcll(__ballot(on && t_done && (t_flags & RF_EXACT) != 0));
            PUSH_TRAV()
            }
        };
        auto leaf_arm = [&](auto may_exact_) __attribute__((always_inline)) {
            constexpr bool MAY_EXACT = decltype(may_exact_)::value;
            if constexpr (!DEC) {
            // ---- leaf step: the record's two triangles in one packed computation ----
            POP3(PH3_LEAF)
            bool t_done = false;
            int t_ref = 0;
            uint32_t t_flags = 0;
            if (on) {
                const float4 qa = S.A[id], qb = S.B[id];
                int ref = S.node[id];
                uint32_t qd = S.D[id];
                const F3 o = f3(qa.x, qa.y, qa.z), d = f3(qb.x, qb.y, qb.z);
                float T = qa.w;
                int tri = __float_as_int(qb.w);
                int sp = (int)(qd & 0xffu);
                const int lv = MAY_EXACT || MODE == 1 ? lds_levels<LDS3>((qd & RF_EXACT) != 0) : (int)LDS3::LV;
                const int top = stack_top_ahead(S, id, sp, lv);
                const bool any_hit = (qd & RF_ANYHIT) != 0;
                int best_leaf = tri - (int)((qd >> 8) & 0xffffu); // first triangle of the leaf that holds the best hit (-1 - 0 if none)
                bool done = false;
                uint32_t rec = (uint32_t)~ref;
                int it0 = 0, left = 1;
                for (int k = 0; left > 0 && !done; k++, rec++) { // one record per pair of triangles: a single pass with bvh_thresh_n <= 2
                    const float4* lg = (const float4*)((const char*)sc.leaf_geo + rec * 80u); // (32-bit byte offset, as for the nodes)
                    const float4 g0 = lg[0], g1 = lg[1], g2 = lg[2], g3 = lg[3], g4 = lg[4];
                    const int it = __float_as_int(g4.z);
                    if (k == 0) { it0 = it; left = __float_as_int(g4.w); }
                    const bool two = left > 1;
                    bool a0, a1;
                    float t0, t1;
                    tri_pair(g0, g1, g2, g3, g4, v2(qa.x, qa.y), v2(qa.z, qa.w), v2(qb.x, qb.y), v2(qb.z, qb.w), a0, a1, t0, t1);
                    a1 = a1 && two;
                    if (STATS) { tc.tests += two ? 2u : 1u; }
                    if (any_hit) {
                        const bool b0 = a0 & (T - t0 > CRT_EPSILON);
                        const bool b1 = a1 & (T - t1 > CRT_EPSILON);
                        done = b0 | b1;
                        tri = b0 ? it : (b1 ? it + 1 : tri);
                    } else {
                        // ascending index, strict <: the first of equal t inside a leaf wins (DeviceBVH.cuh:34-41); across leaves the
                        // larger leaf start wins (reference visit order, see crt_trace.h)
                        const bool w0 = a0 & ((t0 < T) | ((t0 == T) & (it0 > best_leaf)));
                        T = w0 ? t0 : T; tri = w0 ? it : tri; best_leaf = w0 ? it0 : best_leaf;
                        const bool w1 = a1 & ((t1 < T) | ((t1 == T) & (it0 > best_leaf)));
                        T = w1 ? t1 : T; tri = w1 ? it + 1 : tri; best_leaf = w1 ? it0 : best_leaf;
                    }
                    left -= 2;
                }
                if (STATS) tc.leaf++;
                if (!any_hit && tri >= 0) qd = (qd & ~RR_ROUTE_LC_BIT) | RF_HASHIT; // (a surface was found: LC -> LA)
                if (!done) done = stack_pop_ahead(S, M3, id, g, sp, ref, top, lv);
                qd = (qd & 0xff000000u) | ((uint32_t)(tri - best_leaf) << 8 & 0xffff00u) | (uint32_t)sp;
                if (!any_hit) S.A[id].w = T;
                S.B[id].w = __int_as_float(tri);
                S.node[id] = ref;
                S.D[id] = qd;
                if (STATS && done && tri >= 0) tc.hits++;
                t_done = done; t_ref = ref; t_flags = qd;
            }
            if (MAY_EXACT && MODE != 1) n_exact -= (int)__popcll(__ballot(on && t_done && (t_flags & RF_EXACT) != 0));
            PUSH_TRAV()
            }
        };
        // ---- DEC arms (Pool4LdsT): see there ----
        auto inner_arm_dec = [&](auto may_exact_) __attribute__((always_inline)) {
            constexpr bool MAY_EXACT = decltype(may_exact_)::value;
            if constexpr (DEC) {
            // ---- inner-node step: the child boxes; leaf children that are hit -> queue entries; nearest inner child next ----
            // All 64 lanes run the step (round 6): a lane without a ray of the batch (ON is the batch) steps at the EMPTY node like every other
            // lane that sits the visit out, so there is no divergent region around the step, every predicate is a wave mask and every
            // wave-uniform count -- queue entries appended, rays re-queued -- stays in a scalar register (until round 5 they left the region
            // in a vector register, through v_readfirstlane).  Stores and LDS atomics are predicated by `lanes(mask)`.
            // (the batch is not cut to the quarter of the free queue entries that could take four entries per ray: the entries of a visit
            // are counted before any is written, and should they not fit -- rarely: a ray adds 0.8 on average -- the lanes beyond that quarter are
            // taken out of the visit again and queued as they came, visit_front CHECK 1.  Batches 57 -> 62 rays: C2 80.4 -> 79.5 ms, veach 80.4 -> 79.2)
            const int take = min(64, qn[PH3_INNER]);
            if (STATS) { dg_b[PH3_INNER]++; dg_l[PH3_INNER] += (uint32_t)take; }
            const wmask ON = bal(lane < take);
            // (a lane beyond the batch reads an entry of the ring that is not part of it -- a ray id of this pool all the same, or the
            // ring's initial bytes: the id is forced into the pool)
            const uint32_t id_raw = S.rq(PH3_INNER)[(uint32_t)(qn[PH3_INNER] - take) + (uint32_t)lane];
            qn[PH3_INNER] -= take;
            const uint32_t id = lanes(ON) ? id_raw : 0u;
            const uint32_t g = base + id;
            uint32_t nph = PH3_NONE;      // a ray that is complete (its walk is over and none of its entries is in flight): where it goes
            uint32_t added = 0;           // entries of the batch so far (wave-uniform)
            wmask DONE, EXQ = 0ull;
            {
                const float4 qa = S.A[id], qb = S.B[id];
                const uint32_t qd = S.D[id];
                const uint32_t blo = (uint32_t)__hip_atomic_load(&S.best[id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                int ref = __float_as_int(qb.w);
                const F3 o = f3(qa.x, qa.y, qa.z), dir = f3(qb.x, qb.y, qb.z);
                int sp = (int)(qd & 0xffu);
                // an any-hit ray that has its answer looks no further (entries of it still in the queue are tested and change nothing)
                const wmask D0 = bal((qd & RF_ANYHIT) != 0) & bal(blo != 0u) & ON;
                const wmask GO = ON & ~D0;
                const wmask EX = MAY_EXACT ? bal((qd & RF_EXACT) != 0) : 0ull;
                DONE = D0;
                int n_leaf = 0;           // entries of this ray from its 4-wide visits
                wmask ANY = 0ull;         // rays that appended an entry in this step
                {
                    wmask VOID = 0ull;
                    RayPk R;
                    R.oxy = v2(qa.x, qa.y); R.oz.x = qa.z;
                    // (free entries, saturating: the scheduler drains the queue from LEAFQ_FIRST entries on and a step adds at most what is
                    // free, so the difference cannot be negative -- but a wrapped unsigned here would switch the overflow check off for good)
                    const uint32_t lq_used = (lq_t - lq_h) + (MAY_EXACT ? 64u : 0u);
                    const uint32_t lq_free = lq_used < (uint32_t)LEAFQ_CAP ? (uint32_t)LEAFQ_CAP - lq_used : 0u;
                    // (MAY_EXACT: the rays of the reference-arithmetic path append one entry each below, outside that count)
                    Visit4 V1, V2;
                    const wmask EN1 = GO & ~EX;
                    node_load<IMPL>(sc, ref, EN1, dir, V1);
                    const int top1 = stack_top_ahead(S, id, sp, LDS3::LV);
                    DONE |= visit_front<STATS, LDS3, 1, IMPL>(sc, M3, g, dir, R, V1, top1, ref, sp, tc, max_sp, lq_t, added, ANY, n_leaf, EN1, lq_free, nullptr, &VOID);
                    if (STATS && lanes(EN1 & VOID)) dg_ov[0]++;
                    // A SECOND NODE in the same step for the rays that go on, their record still in registers (in the form
                    // this pool allows: with the leaves decoupled a ray that is not finished always has an inner node next).  Taken while at
                    // least VISIT2_MIN lanes go on (crt_mega3.h); its leaf entries are counted before anything is written, and if the queue cannot take
                    // them the visit is dropped.  C2 82.7 -> 81.7 ms, veach-mis spp 256
                    // 81.8 -> 80.3 (40 .. 52: the same; 16 / 32: 82.6 / 82.1 and 80.8 / 80.6; as a loop, or three / four visits: worse).
                    // Round 6: its node is fetched BEFORE the first visit's appends and pushes are written (node_load / visit_back).
                    const wmask EN2 = ON & ~DONE;
                    const bool second = !MAY_EXACT && (int)__popcll(EN2) >= VISIT2_MIN;
                    if (second) node_load<IMPL>(sc, ref, EN2, dir, V2);
                    visit_back(S, M3, id, g, V1);
                    if (second) {
                        const uint32_t lq_used2 = (lq_t + added) - lq_h;
                        const uint32_t cap_left = lq_used2 < (uint32_t)LEAFQ_CAP ? (uint32_t)LEAFQ_CAP - lq_used2 : 0u;
                        bool bailed = false;
                        const int top2 = stack_top_ahead(S, id, sp, LDS3::LV);
                        DONE |= visit_front<STATS, LDS3, 2, IMPL>(sc, M3, g, dir, R, V2, top2, ref, sp, tc, max_sp, lq_t, added, ANY, n_leaf, EN2, cap_left, &bailed);
                        if (!bailed) visit_back(S, M3, id, g, V2);
                        if (STATS && bailed && lanes(EN2)) dg_ov[1]++;
                    }
                }
                if (MAY_EXACT) {
                    const wmask GX = GO & EX;
                    if (GX) { // reference arithmetic on the reference topology, one thing per visit: a leaf ref becomes a queue entry, an inner node is stepped
                        const wmask LF = GX & bal(ref < 0);
                        uint32_t lrec = (uint32_t)~ref; // (a leaf ref of nodes3: a record of leaf_geo)
                        if (IMPL) lrec = (uint32_t)sc.rec_map[lanes(LF) ? lrec : 0u]; // ... whose copy in leaf_geo_i the leaf step reads
                        leafq_push(S, id, lanes(LF), LF, (lrec << 8) | id, lq_t, added);
                        bool dn = false;
                        if (lanes(GX)) {
                            if (lanes(LF)) dn = stack_pop(S, M3, id, g, sp, ref, lds_levels<LDS3>(true));
                            else dn = inner2_step<0, STATS>(sc, S, M3, id, g, o, inv3_exact(dir), dir, pinf(), ref, sp, tc, max_sp);
                        }
                        ANY |= LF;
                        DONE |= bal(dn) & GX;
                    }
                    EXQ = DONE & EX; // rays of the reference-arithmetic path whose walk ended
                }
                // the record: node, stack depth, "the walk is over" -- the count of entries in flight in between is touched by atomics only
                // (leafq_push above: those additions are in LDS before this one, same wave, in order)
                if (STATS) { for (int k = 0; k < 6; k++) dg_sp[k] += (lanes(ON) && sp > k + 1) ? 1u : 0u; }
                if (lanes(ON)) {
                    S.B[id].w = __int_as_float(ref);
                    __hip_atomic_fetch_add(&S.D[id], (uint32_t)sp - (qd & 0xffu) + (lanes(DONE) ? RD_FIN : 0u) + ((uint32_t)n_leaf << RD_PEND_SHIFT), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                const wmask COMP = DONE & ~ANY & bal((qd & RD_PEND_MASK) == 0u);
                if (STATS && lanes(COMP) && blo != 0u) tc.hits++;
                if (COMP) nph = lanes(COMP) ? route_complete<QUERY>(qd, blo != 0u) : nph;
            }
            // re-queue the rays that go on
            const wmask MC = ON & ~DONE;
            // (the ring append written out, as the parent had it: through ring_append -- its predicate lanes(MC) formed before the call, or
            // inside it -- the streams of 11, or of the counting ones, of the 21 decoupled instantiations change)
            if (MC) {
                const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(MC >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)MC, STATS ? (uint32_t)qn[PH3_INNER] : scalar_copy(qn[PH3_INNER])));
                if (lanes(MC)) S.rq(PH3_INNER)[slot] = (uint8_t)id;
                const int c = (int)__popcll(MC);
                qn[PH3_INNER] += c;
            }
            lq_t += added;
            if (MAY_EXACT) n_exact -= (int)__popcll(EXQ);
            if (bal(nph != PH3_NONE)) {
                PUSH_ONE(PH3_LA, nph == PH3_LA) PUSH_ONE(PH3_LB, nph == PH3_LB) PUSH_ONE(PH3_LC, nph == PH3_LC)
            }
            }
        };
        auto leaf_arm_dec = [&]() __attribute__((always_inline)) {
            if constexpr (DEC) {
            // ---- leaf step: 64 entries of the queue, the record's two triangles in one packed computation ----
            // All 64 lanes run it (round 6, as the inner step): a lane beyond the batch takes entry 0 of record 0 -- valid addresses -- and its
            // result is dropped: the minimum and the count of entries in flight are touched under `lanes(ON)` only.
            const int take = min(64, (int)(lq_t - lq_h));
            if (STATS) { dg_b[PH3_LEAF]++; dg_l[PH3_LEAF] += (uint32_t)take; }
            const wmask ON = bal(lane < take);
            // (fetching these entries and their records from the inner step before this one -- they are known when the queue held 64 before it --
            // was measured in round 6: the values arrive in other registers than the step's own loads use, 20 copies and a full wait: +1.3 %)
            const uint32_t item_raw = S.leafq[(lq_h + (uint32_t)lane) & (uint32_t)(LEAFQ_CAP - 1)];
            lq_h += (uint32_t)take;
            const uint32_t item = lanes(ON) ? item_raw : 0u;
            const uint32_t id = item & 0xffu;
            wmask COMP = 0ull;
            uint32_t t_flags = 0;
            {
                const float4 qa = S.A[id], qb = S.B[id];
                const F3 o = f3(qa.x, qa.y, qa.z), d = f3(qb.x, qb.y, qb.z);
                const float Tl = qa.w;
                // The entry leaves the ray's count of entries in flight NOW (round 6): the returning LDS atomic's round trip hides behind the
                // record's loads instead of standing alone at the end of the step.  Every minimum of this step is in LDS before the step ends,
                // and nothing reads a ray's answer before the step that routes it has ended -- the order of the two atomics inside a step is free.
                if (lanes(ON)) t_flags = __hip_atomic_fetch_sub(&S.D[id], 1u << RD_PEND_SHIFT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                uint32_t rec = item >> 8;
                // the leaf's candidate: the first of its triangles among equal distances (ascending index, strict <: DeviceBVH.cuh:34-41)
                bool have = false;
                float bt = 0.0f;
                int bi = 0;
                int left = 1;
                // (a leaf step without this loop for scenes whose leaves are one record each -- bvh_thresh_n <= 2 -- was measured in round 5: eleven
                // instructions fewer per step, C2 +0.3 %, veach-mis +0.2 %: the second copy of the pair test costs what they save; not kept)
                for (int k = 0; left > 0; k++, rec++) { // one record per pair of triangles: a single pass with bvh_thresh_n <= 2
                    const float4* lg = (const float4*)((const char*)(IMPL ? sc.leaf_geo_i : sc.leaf_geo) + rec * 80u);
                    const float4 g0 = lg[0], g1 = lg[1], g2 = lg[2], g3 = lg[3], g4 = lg[4];
                    const int it = __float_as_int(g4.z);
                    if (k == 0) left = __float_as_int(g4.w);
                    const bool two = left > 1;
                    bool a0, a1;
                    float t0, t1;
                    tri_pair(g0, g1, g2, g3, g4, v2(qa.x, qa.y), v2(qa.z, qa.w), v2(qb.x, qb.y), v2(qb.z, qb.w), a0, a1, t0, t1);
                    if (STATS && lanes(ON)) { tc.tests += two ? 2u : 1u; }
                    // (Tl - t > EPSILON: the visibility test of an any-hit ray, Render.cuh:19-27; always true for Tl = +inf and a finite t,
                    // false for t = +inf, which the reference's t < best.t rejects as well)
                    const bool b0 = a0 & (Tl - t0 > CRT_EPSILON);
                    const bool b1 = a1 & two & (Tl - t1 > CRT_EPSILON);
                    const bool s1 = b1 & (!b0 | (t1 < t0));
                    const float ct = s1 ? t1 : t0;
                    const int ci = s1 ? it + 1 : it;
                    const bool up = (b0 | b1) & (!have | (ct < bt));
                    bt = up ? ct : bt; bi = up ? ci : bi; have = have | up;
                    left -= 2;
                }
                if (STATS && lanes(ON)) tc.leaf++;
                if (lanes(ON)) {
                    // across leaves: the smaller distance, among equal ones the larger leaf start (crt_trace.h) = the larger triangle index, as
                    // the leaves own disjoint ascending ranges -- one 64-bit minimum over (bits(t), ~triangle); t > EPSILON > 0, so its bits order as it does
                    if (have) __hip_atomic_fetch_min(&S.best[id], ((unsigned long long)__float_as_uint(bt) << 32) | (unsigned long long)(uint32_t)~bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                COMP = bal((t_flags & (RD_PEND_MASK | RD_FIN)) == ((1u << RD_PEND_SHIFT) | RD_FIN)); // the last entry of a ray whose walk is over (t_flags is 0 beyond the batch)
            }
            if (COMP) {
                uint32_t blo = 0;
                if (lanes(COMP)) blo = (uint32_t)__hip_atomic_load(&S.best[id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (STATS && lanes(COMP) && blo != 0u) tc.hits++;
                const uint32_t nph = lanes(COMP) ? route_complete<QUERY>(t_flags, blo != 0u) : (uint32_t)PH3_NONE;
                PUSH_ONE(PH3_LA, nph == PH3_LA) PUSH_ONE(PH3_LB, nph == PH3_LB) PUSH_ONE(PH3_LC, nph == PH3_LC)
            }
            }
        };
        const bool plain = MODE == 1 || n_exact == 0;
        // The two traversal steps ALTERNATE without going back to the scheduler while the other side holds a batch and no logic ring holds
        // a full one: the scheduler's comparison of the five rings (36 scalar instructions -- a third of them copies of the loop-carried
        // ring cursors -- and the dispatch on its result) stands between every two steps of the wave, and a wave issues one instruction
        // at a time whatever its kind.  Coupled form: C2 92.6 -> 91.1 ms, veach-mis spp 256 88.0 -> 84.8 with CHAIN_MIN 44
        // (56 / 48 / 40 / 32 / 20: 93.0 / 91.3 / 91.2 / 91.7 / 93.2 and 85.9 / 84.9 / 84.9 / 86.2 / 90.2); decoupled form: 92.2 -> 87.7 and
        // 89.5 -> 84.8 (32 / 52: the same).  Not taken: staying on the SAME ring while it holds another full batch (92.9 / 86.7); one chained
        // step only, each arm compiled twice (92.1 / 86.0); the same preference expressed in the scheduler's keys (no gain); a short-cut in
        // front of the scheduler (93.6 / 88.7).
        auto logic_waits = [&]() __attribute__((always_inline)) {
            if constexpr (STATS) return max(max(qn[PH3_LA], qn[PH3_LB]), qn[PH3_LC]) >= 64; // (the counting kernels' cursors may live in vector registers)
            else return smax(smax(qn[PH3_LA], qn[PH3_LB]), qn[PH3_LC]) >= 64;
        };
        if constexpr (DEC) {
            // (the leaf queue goes first while it holds LEAFQ_FIRST entries, as in the scheduler)
            if (plain) {
                bool do_inner = act == PH3_INNER;
                for (;;) {
                    if (do_inner) {
                        stamps.other();
                        inner_arm_dec(std::false_type{});
                        stamps.step(2);
                        if ((int)(lq_t - lq_h) < LEAFQ_FIRST || logic_waits()) break;
                    }
                    stamps.other();
                    leaf_arm_dec();
                    stamps.step(1);
                    if (logic_waits()) break;
                    do_inner = (int)(lq_t - lq_h) < LEAFQ_FIRST;
                    if (do_inner && qn[PH3_INNER] < CHAIN_MIN) break;
                }
            } else if (act == PH3_INNER) {
                inner_arm_dec(std::true_type{});
            } else {
                leaf_arm_dec();
            }
        } else {
        if (plain) {
            bool do_inner = act == PH3_INNER;
            for (;;) {
                if (do_inner) {
                    inner_arm(std::false_type{});
                    if (qn[PH3_LEAF] < CHAIN_MIN || logic_waits()) break;
                }
                leaf_arm(std::false_type{});
                if (qn[PH3_INNER] < CHAIN_MIN || logic_waits()) break;
                do_inner = true;
            }
        } else if (act == PH3_INNER) {
            inner_arm(std::true_type{});
        } else {
            leaf_arm(std::true_type{});
        }
        }
      }
        // (commit ring: a pool with nothing to do but slots that are held back looks at those)
        if (act == PH3_NONE && !(RING && (__builtin_amdgcn_readfirstlane((int)S.waitq) & 0xff) != 0)) break;
        stamps.other();
        if (act == PH3_LA) {
            POP3(PH3_LA)
            bool new_exact = false;
            if (on) {
                LOGIC_PARAMS()
                NewRay nr;
                float4 ra_, rb_;
                ray_result(S, id, ra_, rb_);
                nph = logic_A<MODE, RING>(Pl, tl, g, ra_, rb_, nr, cnt, ALL);
                if (nph == PH3_LB) { S.A[id].x = nr.o.x; S.A[id].y = nr.o.y; S.A[id].z = nr.o.z; } // (a vertex that goes to the roulette without a ray of its own)
                if (nph == PH3_NONE) nph = start_ray<MODE, false, LDS3, IMPL>(Pl.sc, S, id, nr, cnt, M3.force_exact != 0, new_exact);
            }
            n_exact += (int)__popcll(__ballot(new_exact));
            PUSH3()
            stamps.step(0);
        } else if (act == PH3_LB) {
            POP3(PH3_LB)
            bool new_exact = false;
            if (on) {
                LOGIC_PARAMS()
                NewRay nr;
                float4 ra_, rb_;
                ray_result(S, id, ra_, rb_);
                nph = logic_B<MODE, RING>(Pl, g, ra_, rb_, nr);
                if (nph == PH3_NONE) nph = start_ray<MODE, false, LDS3, IMPL>(Pl.sc, S, id, nr, cnt, M3.force_exact != 0, new_exact);
            }
            n_exact += (int)__popcll(__ballot(new_exact));
            PUSH3()
            stamps.step(4);
            // (going from here straight to LC when LC holds 16 / 32 paths -- LB's roulette stops feed it -- was measured in round 5: C2 +3.0 % / +0.7 %,
            // veach-mis +1.4 % / +1.0 %: it runs LC with emptier batches than the fullest-first rule; not kept)
        }
        if (act != PH3_LA && act != PH3_LB) {
            // LC, or -- commit ring -- a look at the slots that are held back (PH3_WAIT), through the same code: the held slots have
            // their turn when the pool has nothing else to do and, while there are any, at every second visit of this phase
            // (no loop around the phase: it would count as one more level of nesting in the compiler's register allocation)
            int wn = 0, wh = 0, wt = 0; // ring PH3_WAIT: entries, head, tail
            bool held = false;
            if (RING) {
                const uint32_t wq = (uint32_t)__builtin_amdgcn_readfirstlane((int)S.waitq);
                wn = (int)(wq & 0xffu); wh = (int)((wq >> 8) & 0xffu); wt = (int)((wq >> 16) & 0xffu);
                held = act == PH3_NONE || (wn > 0 && (wq >> 24) != 0u);
            }
            const int src_n = held ? wn : qn[PH3_LC];
            const int take = min(64, src_n);
            const int src_h = held ? wh : (int)(uint32_t)(qn[PH3_LC] - take);
            if (STATS) { dg_b[PH3_LC]++; dg_l[PH3_LC] += (uint32_t)take; }
            const bool on = lane < take;
            // (the parking ring of the commit ring is a FIFO: its wrap is by compare)
            const uint32_t pop_i = (uint32_t)(src_h + lane);
            const uint32_t id = held ? S.rq(PH3_WAIT)[min(pop_i, pop_i - (uint32_t)QCAP)] : S.rq(PH3_LC)[pop_i];
            if (held) {
                int nh = src_h + take;
                if (nh >= QCAP) nh -= QCAP;
                wh = nh; wn -= take;
            } else {
                qn[PH3_LC] -= take;
            }
            const uint32_t g = base + id;
            uint32_t nph = PH3_NONE;
            bool new_exact = false, wait = false;
            uint32_t fin_key = ~0u;
            if (on) {
                LOGIC_PARAMS()
                NewRay nr;
                float4 ra_ = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rb_ = ra_;
                if (QUERY) ray_result(S, id, ra_, rb_);
                const int got = QUERY ? (query_C(Pl, g, ra_, rb_, nr) ? LC_RAY : LC_DEAD) : logic_C<MODE, RING>(Pl, tl, g, cnt, nr, fin_key);
                if (got == LC_RAY) nph = start_ray<MODE, QUERY, LDS3, IMPL>(Pl.sc, S, id, nr, cnt, M3.force_exact != 0, new_exact);
                wait = got == LC_WAIT;
            }
            n_exact += (int)__popcll(__ballot(new_exact));
            PUSH3()
            if (RING) { // count the finished work items, commit what that completes; park the slots that are held back
                LOGIC_PARAMS()
                ring_publish(Pl, fin_key);
                const unsigned long long mw = __ballot(wait);
                if (mw) {
                    const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(mw >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mw, (uint32_t)wt));
                    if (wait) S.rq(PH3_WAIT)[min(slot, slot - (uint32_t)QCAP)] = (uint8_t)id;
                    const int add = (int)__popcll(mw);
                    wn += add;
                    wt += add;
                    if (wt >= QCAP) wt -= QCAP;
                }
                if (held && mw == __ballot(on)) __builtin_amdgcn_s_sleep(64); // (none of them may start yet: no hurry)
                if (lane == 0) S.waitq = (uint32_t)wn | ((uint32_t)wh << 8) | ((uint32_t)wt << 16) | (held ? 0u : 1u << 24);
            }
            stamps.step(5);
        }
    }

    // ---- counters ----
#ifdef CRT_STAMPS
    if (lane == 0) {
        unsigned long long* cs_ = M.counters + (blockIdx.x & (CNT_SHARDS - 1)) * CNT_STRIDE;
        atomicAdd(&cs_[C_CYC_LOGIC], stamps.acc[0]); atomicAdd(&cs_[C_CYC_LEAF], stamps.acc[1]); atomicAdd(&cs_[C_CYC_INNER], stamps.acc[2]); atomicAdd(&cs_[C_CYC_OTHER], stamps.acc[3]);
        atomicAdd(&cs_[C_DIAG + 0], stamps.acc[4]); atomicAdd(&cs_[C_DIAG + 1], stamps.acc[5]);
        for (int k = 0; k < 6; k++) atomicAdd(&cs_[C_DIAG + 2 + k], (unsigned long long)stamps.n[k]);
    }
#endif
    uint32_t r = wave_sum(cnt.rays), sh = wave_sum(cnt.shadow), pr = wave_sum(cnt.probe), pa = wave_sum(cnt.paths), un = wave_sum(cnt.untraced);
    unsigned long long* cs = M.counters + (blockIdx.x & (CNT_SHARDS - 1)) * CNT_STRIDE;
    if (lane == 0 && (r | pa)) {
        atomicAdd(&cs[C_RAYS], (unsigned long long)r);
        atomicAdd(&cs[C_SHADOW], (unsigned long long)sh);
        atomicAdd(&cs[C_PROBE], (unsigned long long)pr);
        atomicAdd(&cs[C_PATHS], (unsigned long long)pa);
        atomicAdd(&cs[C_UNTRACED], (unsigned long long)un);
    }
    if (STATS) {
        uint32_t a = wave_sum(tc.inner), b = wave_sum(tc.leaf), c = wave_sum(tc.tests), d = wave_sum(tc.hits);
        uint32_t ms = max_sp;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ms = max(ms, (uint32_t)__shfl_xor((int)ms, o, 64));
        if (lane == 0) {
            atomicAdd(&cs[C_INNER], (unsigned long long)a);
            atomicAdd(&cs[C_LEAF], (unsigned long long)b);
            atomicAdd(&cs[C_TESTS], (unsigned long long)c);
            atomicAdd(&cs[C_HITS], (unsigned long long)d);
            atomicMax(&cs[C_MAXSP], (unsigned long long)ms);
            for (int p = 0; p < 5; p++) {
                atomicAdd(&cs[C_DIAG + 2 * p], (unsigned long long)dg_b[p]);
                atomicAdd(&cs[C_DIAG + 2 * p + 1], (unsigned long long)dg_l[p]);
            }
        }
        for (int k = 0; k < 6; k++) {
            const uint32_t v = wave_sum(dg_sp[k]);
            if (lane == 0) atomicAdd(&cs[C_DIAG + 10 + k], (unsigned long long)v);
        }
        for (int k = 0; k < 2; k++) {
            const uint32_t v = wave_sum(dg_ov[k]);
            if (lane == 0) atomicAdd(&cs[C_DIAG + 16 + k], (unsigned long long)v);
        }
    }
}


// ---- exported to crt_render.hip ----
// k_order_items (crt_item_order.h): the count pass and the place pass over `blocks` spans (cnt: zero on entry)
void launch_order_items(bool ring, uint32_t blocks, hipStream_t st, const LParams& P, const OrderClasses& C, uint32_t* list, unsigned int* cnt)
{
    if (ring) {
        hipLaunchKernelGGL((k_order_items<true, false>), dim3(blocks), dim3(64), 0, st, P, C, list, cnt);
        hipLaunchKernelGGL((k_order_items<true, true>), dim3(blocks), dim3(64), 0, st, P, C, list, cnt);
    } else {
        hipLaunchKernelGGL((k_order_items<false, false>), dim3(blocks), dim3(64), 0, st, P, C, list, cnt);
        hipLaunchKernelGGL((k_order_items<false, true>), dim3(blocks), dim3(64), 0, st, P, C, list, cnt);
    }
}

// ---- the instantiations ----
// One descriptor per instantiation, made from the template arguments themselves: its key, the kernel, the rays per wave of its pool and
// the traversal-stack levels that pool keeps in LDS -- what the host sizes the launch and the spill area with cannot be another kernel's.
constexpr uint32_t mega3_key(int mode, bool stats, bool all, bool query, bool r16, bool ring, bool dec, bool impl)
{
    return (uint32_t)mode | (stats ? 4u : 0u) | (all ? 8u : 0u) | (query ? 16u : 0u) | (r16 ? 32u : 0u) | (ring ? 64u : 0u) | (dec ? 128u : 0u) | (impl ? 256u : 0u);
}
template <int MODE, bool STATS, bool ALL, bool QUERY, bool R16, bool RING, bool DEC, bool IMPL> Mega3Variant mega3_descriptor()
{
    typedef Mega3Pool<R16, RING, DEC> LDS;
    return Mega3Variant{mega3_key(MODE, STATS, ALL, QUERY, R16, RING, DEC, IMPL), (Mega3Kernel)k_mega3<MODE, STATS, ALL, QUERY, R16, RING, DEC, IMPL>, (uint32_t)LDS::P, (int)LDS::LV};
}
// every key of 9 bits whose arguments are legal: 53 kernels
template <uint32_t K> void mega3_add(std::vector<Mega3Variant>& t)
{
    constexpr int MODE = (int)(K & 3u);
    constexpr bool STATS = (K & 4u) != 0, ALL = (K & 8u) != 0, QUERY = (K & 16u) != 0, R16 = (K & 32u) != 0, RING = (K & 64u) != 0, DEC = (K & 128u) != 0, IMPL = (K & 256u) != 0;
    static_assert(mega3_key(MODE, STATS, ALL, QUERY, R16, RING, DEC, IMPL) == K, "mega3_add decodes what mega3_key encodes");
    if constexpr (mega3_legal(MODE, STATS, ALL, QUERY, R16, RING, DEC, IMPL)) t.push_back(mega3_descriptor<MODE, STATS, ALL, QUERY, R16, RING, DEC, IMPL>());
}
template <uint32_t... K> void mega3_add_all(std::vector<Mega3Variant>& t, std::integer_sequence<uint32_t, K...>) { (mega3_add<K>(t), ...); }
#if defined(CRT_ASM_ONLY_DEFAULT) && !defined(CRT_ASM_ONLY_ARGS)
#define CRT_ASM_ONLY_ARGS 2, false, false, false, true, false, true, true
#endif
static const std::vector<Mega3Variant>& mega3_table()
{
    static const std::vector<Mega3Variant> t = [] {
        std::vector<Mega3Variant> v;
#ifdef CRT_ASM_ONLY_DEFAULT /* tools/diet/asm_default.sh: the default instantiation alone (a quick assembly listing; never a library) */
        v.push_back(mega3_descriptor<CRT_ASM_ONLY_ARGS>());
#else
        mega3_add_all(v, std::make_integer_sequence<uint32_t, 512>{});
#endif
        return v;
    }();
    return t;
}
const Mega3Variant* mega3_variant(int mode, bool stats, bool all, bool query, bool r16, bool ring, bool dec, bool impl)
{
    // A request is first brought into the form the table holds.  Each line is a mapping the callers rely on:
    if (mode != 2) dec = false;                    // the leaves are decoupled in CRT_TRAVERSAL_EXACT only
    if (!(dec && r16)) impl = false;               // the tree without its rows of refs needs decoupled leaves and 16-bit entries
    if (mode == 1) { all = false; r16 = false; }   // REFERENCE traces every sample anyway and walks the 2-wide trees (32-bit entries)
    if (ring) { stats = false; query = false; }    // the commit ring is a render without counters
    if (query) { stats = false; all = false; }     // a query has neither counters of its own nor next-event samples
    // (after that every request with a mode of 0 .. 2 is in the table -- mega3_legal holds for it -- so no caller can reach the nullptr
    // today: it is what a mode outside that range, or a table cut down by -DCRT_ASM_ONLY_DEFAULT, gets instead of a neighbouring kernel)
    const uint32_t key = mega3_key(mode, stats, all, query, r16, ring, dec, impl);
    if (mode < 0 || mode > 2) return nullptr;
    for (const Mega3Variant& v : mega3_table())
        if (v.key == key) return &v;
    return nullptr;
}
// Diagnostic hook (tools/bbprof): CRT_BBPROF_CO names a code object holding the default instantiation of k_mega3 with a counting
// prologue in every basic block (tools/bbprof/instrument.py applied to the compiler's assembly of THIS file); the launch then goes
// to that copy, the address of its counter buffer travels in MParams3::dbg_loads / dbg_valu, and the summed counters
// (one u64 per block: executions << 32 | active lanes) are written to CRT_BBPROF_OUT after every launch.  Returns false when the
// variable is not set or the kernel is another instantiation: the caller launches as usual.
bool bbprof_launch(Mega3Kernel kern, MParams3 M3, uint32_t blocks, hipStream_t st)
{
    static const char* co = std::getenv("CRT_BBPROF_CO");
    // (the default instantiations: 16-bit stack entries, CRT_TRAVERSAL_EXACT, with the leaves decoupled or not)
#ifdef CRT_ASM_ONLY_DEFAULT
    const char* sym = nullptr;
#else
    const char* sym = kern == (Mega3Kernel)k_mega3<2, false, false, false, true, false, true, true>    ? "_ZN4crtk7k_mega3ILi2ELb0ELb0ELb0ELb1ELb0ELb1ELb1EEEvNS_8MParams3E"
                      : kern == (Mega3Kernel)k_mega3<2, false, false, false, true, false, true, false>  ? "_ZN4crtk7k_mega3ILi2ELb0ELb0ELb0ELb1ELb0ELb1ELb0EEEvNS_8MParams3E"
                      : kern == (Mega3Kernel)k_mega3<2, false, false, false, true, false, false, false> ? "_ZN4crtk7k_mega3ILi2ELb0ELb0ELb0ELb1ELb0ELb0ELb0EEEvNS_8MParams3E"
                                                                                                         : nullptr;
#endif
    if (!co || !*co || !sym) return false;
    enum { N_CNT = 4096, STRIDE = 128 };
    static hipModule_t mod = nullptr;
    static hipFunction_t fn = nullptr;
    static char* buf = nullptr;
    static char* cnt = nullptr;
    static std::vector<unsigned long long> sum(N_CNT, 0ull);
    if (!fn) {
        HIP_CHECK(hipModuleLoad(&mod, co));
        if (hipModuleGetFunction(&fn, mod, sym) != hipSuccess) { fn = nullptr; return false; } // (the code object holds the other form)
        HIP_CHECK(hipMalloc((void**)&buf, 2 * (size_t)N_CNT * STRIDE));
        // the prologues add block offsets to the low address word without a carry: the counters must not straddle a 4 GiB boundary
        cnt = buf;
        const uint64_t lo = (uint64_t)(uintptr_t)buf & 0xffffffffull;
        if (lo + (uint64_t)N_CNT * STRIDE > 0x100000000ull) cnt = buf + (0x100000000ull - lo);
    }
    HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)N_CNT * STRIDE, st));
    const uint64_t a = (uint64_t)(uintptr_t)cnt;
    M3.dbg_loads = (int32_t)(uint32_t)(a & 0xffffffffull);
    M3.dbg_valu = (int32_t)(uint32_t)(a >> 32);
    size_t sz = sizeof(M3);
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &M3, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
    HIP_CHECK(hipModuleLaunchKernel(fn, blocks, 1, 1, 64, 1, 1, 0, st, nullptr, cfg));
    HIP_CHECK(hipStreamSynchronize(st));
    std::vector<char> h((size_t)N_CNT * STRIDE);
    HIP_CHECK(hipMemcpy(h.data(), cnt, h.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < N_CNT; i++) { unsigned long long v; std::memcpy(&v, h.data() + (size_t)i * STRIDE, 8); sum[i] += v; }
    if (const char* out = std::getenv("CRT_BBPROF_OUT")) {
        if (FILE* f = std::fopen(out, "w")) {
            for (int i = 0; i < N_CNT; i++) if (sum[i]) std::fprintf(f, "%d %llu %llu\n", i, sum[i] >> 32, sum[i] & 0xffffffffull);
            std::fclose(f);
        }
    }
    return true;
}


} // namespace crtk

