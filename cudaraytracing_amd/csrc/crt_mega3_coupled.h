// cudaraytracing_amd/csrc/crt_mega3_coupled.h -- the coupled form of k_mega3's traversal (Pool3LdsT): a ray's stack in LDS with its spilled levels,
// and the steps at a node of the 4-wide and of the 2-wide trees (the inner and leaf steps of a batch are arms of the kernel).  Included by crt_mega3.hip only.
#ifndef CRT_MEGA3_COUPLED_H
#define CRT_MEGA3_COUPLED_H
#include "crt_mega3_logic.h"

namespace crtk {

// Pops the traversal stack of ray `id`; returns true when it is empty (the ray is finished).  An entry is the node ref alone:
// a node that has fallen behind the pruning bound since it was pushed is weeded out by its own step (keeping the entry
// distance to drop such entries here measured no gain on either scene and costs 4 B of LDS per level).  The LDS levels are
// read unconditionally and the (rare) spilled levels behind a wave-uniform branch: a per-lane choice between the two address
// spaces would compile to a flat load that waits on both memory pipes.
// LDS levels of a ray: all of them, except for a ray on the reference-arithmetic path in the 16-bit layout (none)
template <class LDS>
__device__ __forceinline__ int lds_levels(const bool exact) { return (LDS::R16 && exact) ? 0 : LDS::LV; }
template <class LDS>
__device__ __forceinline__ bool stack_pop(LDS& S, const MParams3& M3, const uint32_t id, const uint32_t g, int& sp, int& ref, const int lv)
{
    if (sp == 0) return true;
    sp--;
    int en = S.stk[sp < lv ? sp : 0][id];
    asm volatile("" : "+v"(en)); // (pins the LDS read: see above)
    if (__builtin_amdgcn_ballot_w64(sp >= lv)) {
        if (sp >= lv) en = M3.spill[(size_t)(sp - lv) * M3.M.spill_stride + g];
    }
    ref = en;
    return false;
}
// The same pop in two halves: the top LDS level is read when the step begins -- nothing a step pushes can land on it (pushes go to
// levels >= sp) -- so that its latency hides behind the node / leaf gather instead of standing alone at the end of the step.
template <class LDS>
__device__ __forceinline__ int stack_top_ahead(LDS& S, const uint32_t id, const int sp, const int lv)
{
    const int top = sp - 1;
    return S.stk[(top >= 0 && top < lv) ? top : 0][id];
}
template <class LDS>
__device__ __forceinline__ bool stack_pop_ahead(LDS& S, const MParams3& M3, const uint32_t id, const uint32_t g, int& sp, int& ref, const int top, const int lv)
{
    if (sp == 0) return true;
    sp--;
    int en = top;
    if (__builtin_amdgcn_ballot_w64(sp >= lv)) {
        if (sp >= lv) en = M3.spill[(size_t)(sp - lv) * M3.M.spill_stride + g];
    }
    ref = en;
    return false;
}
template <class LDS>
__device__ __forceinline__ void stack_push(LDS& S, const MParams3& M3, const uint32_t id, const uint32_t g, int& sp, const int ref, const int lv)
{
    if (sp < lv) S.stk[sp][id] = (typename LDS::stk_t)ref;
    if (__builtin_amdgcn_ballot_w64(sp >= lv)) {
        if (sp >= lv) M3.spill[(size_t)(sp - lv) * M3.M.spill_stride + g] = ref;
    }
    sp++;
}


// CRT_TRAVERSAL_EXACT visits every child that is hit whatever the order (no bound shrinks): it only brings the nearest to the front
// (three exchanges instead of five: what the any-hit rays gain from a full order is less than the two exchanges cost -- C2 -0.7 %,
// veach-mis -0.6 %)
#define CRT_SORT4(mode) ((mode) != 2)

// one exchange of the sorting network below: (distance, ref) a and b in ascending order of distance
__device__ __forceinline__ void order2(float& ta, int& ra, float& tb, int& rb)
{
    const bool sw = tb < ta;
    const float tt = sw ? tb : ta; tb = sw ? ta : tb; ta = tt;
    const int rr = sw ? rb : ra; rb = sw ? ra : rb; ra = rr;
}

// One step at a node of the 4-wide tree (rays with finite operands, CRT_TRAVERSAL_FAST / _EXACT): the four child boxes from their
// near and far planes (picked by the sign of the direction, the reference's own swap), the nearest hit child next, the others pushed
// farthest first.  Which children are visited, and in which order, does not change the result (crt_trace.h); the boxes and the test
// are the reference's (hit_AABB, exact for finite operands), so a leaf is entered iff its own box passes -- as in the 2-wide tree.
template <bool STATS, bool SORT = true, class LDS = Pool3Lds, bool DIR = false>
__device__ __forceinline__ bool inner4_step(const DevScene& sc, LDS& S, const MParams3& M, const uint32_t id, const uint32_t g, const F3 o, const F3 inv_or_d,
                                            const float bound, int& ref, int& sp, TravCounters& tc, uint32_t& max_sp
                                            )
{
    const char* nb = (const char*)sc.nodes4; // 32-bit byte offsets: scalar base + vector offset addressing
    const uint32_t noff = (uint32_t)ref * 128u;
    // (DIR: the argument is the direction itself -- 1 / d has d's sign -- and the reciprocals are formed after the loads are on their way)
    const uint32_t ox = noff + ((__float_as_uint(inv_or_d.x) >> 27) & 16u), oy = noff + ((__float_as_uint(inv_or_d.y) >> 27) & 16u),
                   oz = noff + ((__float_as_uint(inv_or_d.z) >> 27) & 16u); // + 16: the ray runs towards -axis, its near plane is hi
    const float4 a0 = *(const float4*)(nb + ox), a1 = *(const float4*)(nb + (ox ^ 16u));
    const float4 a2 = *(const float4*)((nb + oy) + 32), b0 = *(const float4*)((nb + (oy ^ 16u)) + 32);
    const float4 b1 = *(const float4*)((nb + oz) + 64), b2 = *(const float4*)((nb + (oz ^ 16u)) + 64);
    const float4 rf = *(const float4*)((nb + noff) + 96);
    const int top = stack_top_ahead(S, id, sp, LDS::LV);
    if (STATS) tc.inner++;
    const F3 inv = DIR ? inv3_exact(inv_or_d) : inv_or_d;
    float t0, t1, t2, t3; // entry distances; +inf = missed or beyond the pruning bound (sorts last)
    slab_quad_pruned<SORT>(a0, a1, a2, b0, b1, b2, o, inv, bound, t0, t1, t2, t3); // (SORT == pruning mode: CRT_SORT4)
    // (all four entry distances exist before the exchanges and pushes begin: left alone the compiler starts pushing the first pair's
    // loser while the second pair's boxes are still being computed, splits the arithmetic over two blocks and rebuilds the
    // broadcast operand pairs of the packed instructions in the second one -- nine extra moves per step)
    asm volatile("" : "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3));
    const float inf = pinf();
    int r0 = __float_as_int(rf.x), r1 = __float_as_int(rf.y), r2 = __float_as_int(rf.z), r3 = __float_as_int(rf.w);
    // ascending by entry distance: (0,1)(2,3)(0,2)(1,3)(1,2)
    // (leaving out the last exchange -- nearest first, farthest last, the middle two as they come -- saves 5 instructions per step
    // and costs more visits than that: C2 +1.5 %, veach-mis -0.3 %)
    if (SORT) {
        order2(t0, r0, t1, r1); order2(t2, r2, t3, r3); order2(t0, r0, t2, r2); order2(t1, r1, t3, r3); order2(t1, r1, t2, r2);
    } else { // (CRT_TRAVERSAL_EXACT: only the nearest child to the front, CRT_SORT4)
        order2(t0, r0, t1, r1); order2(t2, r2, t3, r3); order2(t0, r0, t2, r2);
    }
    // the children to visit are a prefix of the sorted four (the pushes below do not rely on that); all but the nearest go on the
    // stack, farthest first
    const bool c0 = t0 < inf, c1 = t1 < inf, c2 = t2 < inf, c3 = t3 < inf;
    const int l3 = sp, l2 = l3 + (c3 ? 1 : 0), l1 = l2 + (c2 ? 1 : 0);
    constexpr int LV = LDS::LV; // (a ray of this step is not on the reference-arithmetic path: all LDS levels are its own)
    typedef typename LDS::stk_t stk_t;
    if (c3 & (l3 < LV)) S.stk[l3][id] = (stk_t)r3;
    if (c2 & (l2 < LV)) S.stk[l2][id] = (stk_t)r2;
    if (c1 & (l1 < LV)) S.stk[l1][id] = (stk_t)r1;
    const int sp_new = l1 + (c1 ? 1 : 0);
    if (__builtin_amdgcn_ballot_w64((sp_new > l3) & (sp_new > LV))) { // one check per step for the levels beyond LDS (sp_new - 1 is the highest written)
        if (c3 & (l3 >= LV)) M.spill[(size_t)(l3 - LV) * M.M.spill_stride + g] = r3;
        if (c2 & (l2 >= LV)) M.spill[(size_t)(l2 - LV) * M.M.spill_stride + g] = r2;
        if (c1 & (l1 >= LV)) M.spill[(size_t)(l1 - LV) * M.M.spill_stride + g] = r1;
    }
    sp = sp_new;
    if (STATS && (uint32_t)sp > max_sp) max_sp = (uint32_t)sp;
    if (c0) { ref = r0; return false; }
    return stack_pop_ahead(S, M, id, g, sp, ref, top, LV); // (no child was hit: nothing was pushed, the top is the one read above)
}


// One step at a node of a 2-wide tree: the reference topology (CRT_TRAVERSAL_REFERENCE: reference box arithmetic, reference
// visit order, no pruning) or, for the handful of FAST rays with non-finite operands, reference arithmetic on that topology
// with ordering and pruning.  d = direction (the sign selects the near plane, DeviceBVH.cuh:101-119).
template <int MODE, bool STATS, class LDS>
__device__ __forceinline__ bool inner2_step(const DevScene& sc, LDS& S, const MParams3& M, const uint32_t id, const uint32_t g, const F3 o, const F3 inv,
                                            const F3 d, const float bound, int& ref, int& sp, TravCounters& tc, uint32_t& max_sp)
{
    const float4* nd = sc.nodes3 + (size_t)ref * 4;
    const float4 n0 = nd[0], n1 = nd[1], n2 = nd[2];
    const float2 n3 = *(const float2*)(nd + 3);
    if (STATS) tc.inner++;
    bool hl, hr;
    float tl, tr;
    slab_pair(n0, n1, n2, o, inv, d, true, hl, hr, tl, tr);
    const int lref = __float_as_int(n3.x), rref = __float_as_int(n3.y);
    bool left_first;
    if (MODE == 1) {
        left_first = false; // push lc, visit rc first (DeviceBVH.cuh:154-166)
    } else {
        hl = hl && !(tl > bound);
        hr = hr && !(tr > bound);
        left_first = tl <= tr;
    }
    const bool both = hl && hr, any = hl || hr;
    const int near_ref = both ? (left_first ? lref : rref) : (hl ? lref : rref);
    const int lv = lds_levels<LDS>(true); // (the rays of this step are on the reference-arithmetic path)
    if (both) {
        stack_push(S, M, id, g, sp, left_first ? rref : lref, lv);
        if (STATS && (uint32_t)sp > max_sp) max_sp = (uint32_t)sp;
    }
    if (any) { ref = near_ref; return false; }
    return stack_pop(S, M, id, g, sp, ref, lv);
}

// ---- the steps of a batch (MAY_EXACT: the pool holds rays on the reference-arithmetic path) ----
// Rays with non-finite operands (RF_EXACT: a handful per frame) walk the 2-wide reference topology with the reference's own
// box arithmetic and, in the 16-bit layout, keep their stack in the global area.  Wave3::n_exact counts those in flight in this pool
// (a wave-uniform scalar): while it is zero -- practically always -- the steps run in the form that has none of that handling.

} // namespace crtk
#endif
