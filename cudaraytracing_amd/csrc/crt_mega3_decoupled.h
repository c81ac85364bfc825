// cudaraytracing_amd/csrc/crt_mega3_decoupled.h -- the decoupled form of k_mega3's traversal (Pool4LdsT, crt_mega3.h): wave masks, the leaf queue,
// and a visit of a 4-wide node in three parts (the inner and leaf steps of a batch are arms of the kernel).  Included by crt_mega3.hip only.
#ifndef CRT_MEGA3_DECOUPLED_H
#define CRT_MEGA3_DECOUPLED_H
#include "crt_mega3_coupled.h"

namespace crtk {

// ---- wave masks (round 6) ----
// A predicate of the traversal steps lives as a WAVE MASK in a scalar register pair from the compare that makes it to the select, store or
// count that uses it: a ballot of a compare is the compare's own result, conjunctions / disjunctions / counts are scalar instructions, and
// `lanes` hands a mask back to the vector unit as it stands.  The compiler's own treatment of a bool that crosses a join or is combined
// before a ballot is a trip through a vector register (v_cndmask 0 / 1, v_cmp_ne: 3 % of the kernel's vector instructions in round 5).
typedef unsigned long long wmask;
__device__ __forceinline__ wmask bal(const bool b) { return __builtin_amdgcn_ballot_w64(b); }
__device__ __forceinline__ bool lanes(const wmask m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
// x + 1 / x - 1 in the lanes of m: the mask rides in as the carry (one instruction; the compiler's form is a select and an addition)
__device__ __forceinline__ int add_mask(const int x, const wmask m)
{
    int r;
    wmask co;
    asm("v_addc_co_u32_e64 %0, %1, 0, %2, %3" : "=v"(r), "=s"(co) : "v"(x), "s"(m));
    return r;
}
__device__ __forceinline__ int sub_mask(const int x, const wmask m)
{
    int r;
    wmask co;
    asm("v_subbrev_co_u32_e64 %0, %1, 0, %2, %3" : "=v"(r), "=s"(co) : "v"(x), "s"(m));
    return r;
}


// Appends one entry per lane with `hit` to the leaf queue (the reference-arithmetic rays of the inner step, which hand leaf refs over one by one)
// and counts it among the ray's entries in flight.  lq_t is the queue's tail before the batch, `added` the entries of the batch so far.
template <class LDS>
__device__ __forceinline__ void leafq_push(LDS& S, const uint32_t id, const bool hit, const unsigned long long m, const uint32_t entry, const uint32_t lq_t, uint32_t& added)
{
    // m = the ballot of `hit`, formed by the caller from the ballots of its compares (a ballot of their conjunction would cost a
    // select and another compare)
    if (m) {
        const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, lq_t + added));
        if (hit) {
            S.leafq[slot & (uint32_t)(LEAFQ_CAP - 1)] = entry;
            __hip_atomic_fetch_add(&S.D[id], 1u << RD_PEND_SHIFT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        added += (uint32_t)__popcll(m);
    }
}
// The same append without a branch, for the four children of a 4-wide step (m is empty for one child in five, and a taken branch costs
// more than the eight instructions it skips): a lane without an entry writes to the spare dword behind the queue, and the ray's count
// of entries in flight is the caller's (one addition for the four children).
template <class LDS>
__device__ __forceinline__ void leafq_push_all(LDS& S, const bool hit, const unsigned long long m, const uint32_t entry, uint32_t& tail)
{
    const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, tail));
    S.leafq[hit ? (slot & (uint32_t)(LEAFQ_CAP - 1)) : (uint32_t)LEAFQ_CAP] = entry;
    tail += (uint32_t)__popcll(m);
}

// A visit of the decoupled inner step, in three parts so that the caller can put the SECOND visit's loads in front of the first visit's
// stores (round 6: what a wave waits for in this step is the node's round trip, ~500 cycles; the first visit's appends and pushes -- some
// eighty instructions that touch LDS only -- now run while the second visit's node is on its way):
//   node_load    the six (seven) rows of the node
//   visit_front  boxes, accept masks, the queue-capacity check, entry counts, the nearest inner child, the new node and depth -- registers only
//   visit_back   the leaf-queue entries, the stack pushes (LDS; spilled levels: global memory)
struct Visit4 {
    float4 a0, a1, a2, b0, b1, b2, rf;     // near / far rows of x, y, z; the row of refs (not IMPL)
    wmask m0, m1, m2, m3;                  // leaf children that are hit
    wmask pd, pg, pb;                      // inner children that are hit and pushed: the loser of (2,3), of the final, of (0,1)
    uint32_t q0, q1, q2, q3, tail;         // queue entries (record << 8) and where the visit's first one goes
    int rd, rg, rb, l3, l2, l1, sp_new;    // the pushed refs, their levels, the depth after the pushes
};
template <bool IMPL>
__device__ __forceinline__ void node_load(const DevScene& sc, const int ref, const wmask EN, const F3 dir, Visit4& V)
{
    // IMPL: the copy of the tree without its rows of refs (crt_scene_layout.h "nodes4i": 96 B per node, SIX loads per visit instead of seven);
    // the children's refs and the leaves' records are implied.  A lane outside EN loads the EMPTY node.
    const char* nb = (const char*)(IMPL ? sc.nodes4i : sc.nodes4);
    const uint32_t noff = lanes(EN) ? (uint32_t)ref * (IMPL ? (uint32_t)(NODE4I_F4 * 16) : 128u) : (IMPL ? sc.empty4i_off : sc.empty4_off);
    // (the direction itself picks the planes -- 1 / d has d's sign -- and the reciprocals are formed after the loads are on their way)
    const uint32_t ox = noff + ((__float_as_uint(dir.x) >> 27) & 16u), oy = noff + ((__float_as_uint(dir.y) >> 27) & 16u),
                   oz = noff + ((__float_as_uint(dir.z) >> 27) & 16u);
    V.a0 = *(const float4*)(nb + ox); V.a1 = *(const float4*)(nb + (ox ^ 16u));
    V.a2 = *(const float4*)((nb + oy) + 32); V.b0 = *(const float4*)((nb + (oy ^ 16u)) + 32);
    V.b1 = *(const float4*)((nb + oz) + 64); V.b2 = *(const float4*)((nb + (oz ^ 16u)) + 64);
    V.rf = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!IMPL) V.rf = *(const float4*)((nb + noff) + 112);
}
// CHECK: what happens when the queue cannot take the visit's entries (they are counted before anything is written).  0: cannot happen;
// 1: the lanes from `cap_left / 4` on are taken out of the visit (*voided: they keep their state and are queued again); 2: the whole
// visit is dropped (*bailed; nothing has changed).
// EN: the lanes that take the visit.  A lane outside it -- a lane without a ray, an any-hit ray that has its answer, a ray of the
// reference-arithmetic path, a voided lane -- is at the EMPTY node and keeps its node and depth: it hits nothing, appends nothing,
// pushes nothing and does not pop.  Returns the lanes whose walk is over (a subset of EN); n_leaf and any_leaf accumulate.
// `top`: the stack's top level as it is when the visit begins (read after the visit before it has pushed).
template <bool STATS, class LDS, int CHECK = 0, bool IMPL = false>
__device__ __forceinline__ wmask visit_front(const DevScene& sc, const MParams3& M, const uint32_t g, const F3 dir, RayPk& R, Visit4& V, const int top,
                                             int& ref, int& sp, TravCounters& tc, uint32_t& max_sp, const uint32_t lq_t, uint32_t& added, wmask& any_leaf,
                                             int& n_leaf, const wmask EN, const uint32_t cap_left = 0, bool* bailed = nullptr, wmask* voided = nullptr)
{
    if (CHECK != 2) { // (the second visit of a step takes the first one's 1 / d: the same value, and a ballot of a predicate of another block is a trip through a vector register)
        const F3 inv = inv3_exact(dir);
        R.ixy = v2(inv.x, inv.y); R.iz.x = inv.z;
    }
    float t0, t1, t2, t3;
    int r0, r1, r2, r3;            // the children's refs (an inner child: its node)
    wmask N0, N1, N2, N3;          // the child is a leaf (or an empty slot, which is never hit)
    wmask H0, H1, H2, H3;
    slab_quad_hits(V.a0, V.a1, V.a2, V.b0, V.b1, V.b2, R, t0, t1, t2, t3, H0, H1, H2, H3);
    asm volatile("" : "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3));
    if constexpr (IMPL) {
        // 36 bits in the low 12 mantissa bits of child 0's three NEAR planes (the same bits in the lo and the hi plane of an axis): the first
        // mixed child fm (15), the first fringe child ff (15), the numbers of mixed and of fringe children (3 + 3).  A fringe node -- numbered
        // from n_mixed4i on -- has leaves only and no such bits.  Inner children come first: mixed, then fringe; leaf child k is record 4 n + k.
        const uint32_t cx = __float_as_uint(V.a0.x) & 0xfffu, cy = __float_as_uint(V.a2.x) & 0xfffu, cz = __float_as_uint(V.b1.x) & 0xfffu;
        const bool fr = (uint32_t)ref >= sc.n_mixed4i;
        const uint32_t fm = cx | ((cy & 7u) << 12), ff = (cy >> 3) | ((cz & 63u) << 9);
        const uint32_t cm = fr ? 0u : (cz >> 6) & 7u, ci = fr ? 0u : ((cz >> 6) & 7u) + (cz >> 9);
        N0 = bal(ci == 0u); N1 = bal(ci <= 1u); N2 = bal(ci <= 2u); N3 = bal(ci <= 3u);
        const uint32_t ffm = ff - cm;
        r0 = (int)(cm > 0u ? fm : ffm); r1 = (int)(cm > 1u ? fm + 1u : ffm + 1u); r2 = (int)(cm > 2u ? fm + 2u : ffm + 2u); r3 = (int)(cm > 3u ? fm + 3u : ffm + 3u);
        V.q0 = (uint32_t)ref << 10; V.q1 = V.q0 + 0x100u; V.q2 = V.q0 + 0x200u; V.q3 = V.q0 + 0x300u;
    } else {
        r0 = __float_as_int(V.rf.x); r1 = __float_as_int(V.rf.y); r2 = __float_as_int(V.rf.z); r3 = __float_as_int(V.rf.w);
        N0 = bal(r0 < 0); N1 = bal(r1 < 0); N2 = bal(r2 < 0); N3 = bal(r3 < 0);
        V.q0 = (uint32_t)r0 & 0x7fffff00u; V.q1 = (uint32_t)r1 & 0x7fffff00u; V.q2 = (uint32_t)r2 & 0x7fffff00u; V.q3 = (uint32_t)r3 & 0x7fffff00u;
    }
    wmask m0 = H0 & N0, m1 = H1 & N1, m2 = H2 & N2, m3 = H3 & N3;         // leaf children that are hit
    wmask i0 = H0 & ~N0, i1 = H1 & ~N1, i2 = H2 & ~N2, i3 = H3 & ~N3;     // inner children that are hit
    if (CHECK != 0) {
        if ((uint32_t)(__popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3)) > cap_left) {
            if (CHECK == 2) { *bailed = true; return 0ull; }
            // the lanes a quarter of the free entries has room for stay (lane numbers: the batch's lanes are 0 .. take - 1)
            const wmask km = bal((uint32_t)(threadIdx.x & 63) < (cap_left >> 2));
            m0 &= km; m1 &= km; m2 &= km; m3 &= km;
            i0 &= km; i1 &= km; i2 &= km; i3 &= km;
            *voided = ~km;
        }
    }
    const wmask EFF = CHECK == 1 ? EN & ~*voided : EN; // the lanes whose visit counts
    if (STATS && lanes(EFF)) tc.inner++;
    V.m0 = m0; V.m1 = m1; V.m2 = m2; V.m3 = m3;
    V.tail = lq_t + added;
    added += (uint32_t)(__popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3));
    n_leaf = add_mask(add_mask(add_mask(add_mask(n_leaf, m0), m1), m2), m3);
    any_leaf |= (m0 | m1) | (m2 | m3);
    // The nearest inner child that is hit goes to the front, by a tournament (0,1)(2,3)(winners) on (hit, distance): b beats a iff b is hit and
    // (a is not, or b is nearer).  Only the winner's distance is ever compared again, and "is hit" travels as a mask -- front = a | b, back = a & b --
    // so an exchange is a compare, a select of the winner's distance and two selects of the refs (round 5: distances forced to +inf for the
    // children that are not inner hits, five selects per exchange and a compare with +inf per child afterwards: 23 vector instructions, now 11).
    // The order of the visits is the one of round 5: the result cannot depend on it (crt_trace.h), the any-hit rays' visit counts do.
    const wmask S01 = i1 & (bal(t1 < t0) | ~i0), S23 = i3 & (bal(t3 < t2) | ~i2);
    const float tA = lanes(S01) ? t1 : t0, tC = lanes(S23) ? t3 : t2;
    const int rA = lanes(S01) ? r1 : r0, rC = lanes(S23) ? r3 : r2;
    V.rb = lanes(S01) ? r0 : r1; V.rd = lanes(S23) ? r2 : r3;
    const wmask IA = i0 | i1, IC = i2 | i3;
    V.pb = i0 & i1; V.pd = i2 & i3;
    const wmask S02 = IC & (bal(tC < tA) | ~IA);
    const int rF = lanes(S02) ? rC : rA;
    V.rg = lanes(S02) ? rA : rC;
    const wmask IF = IA | IC;
    V.pg = IA & IC;
    // pushed: the loser of (2,3), then the loser of the final, then the loser of (0,1) -- which is popped first
    V.l3 = sp; V.l2 = add_mask(V.l3, V.pd); V.l1 = add_mask(V.l2, V.pg); V.sp_new = add_mask(V.l1, V.pb);
    constexpr int LV = LDS::LV;
    // (of the lanes whose visit counts: a lane outside the batch carries the depth byte of slot 0, which is whatever LDS held if that slot has had no ray yet)
    if (STATS && lanes(EFF) && (uint32_t)V.sp_new > max_sp) max_sp = (uint32_t)V.sp_new;
    // the nearest inner child next; without one (nothing was pushed either: the top is the one read when the visit began) the stack's top, or the end
    const wmask NF = EFF & ~IF;
    const wmask POP = NF & bal(V.sp_new > 0);
    const wmask OVER = NF & ~POP;
    const int nref = lanes(IF) ? rF : top;
    ref = lanes(IF | POP) ? nref : ref;
    sp = sub_mask(V.sp_new, POP);
    const wmask DEEP = POP & bal(sp >= LV); // (of the new depth -- the carry instruction's own result: the compiler shares a compare of sp_new with the push block's and sends it through a vector register)
    if (DEEP) {
        if (lanes(DEEP)) ref = M.spill[(size_t)(sp - LV) * M.M.spill_stride + g];
    }
    return OVER;
}
template <class LDS>
__device__ __forceinline__ void visit_back(LDS& S, const MParams3& M, const uint32_t id, const uint32_t g, const Visit4& V)
{
    uint32_t tail = V.tail;
    leafq_push_all(S, lanes(V.m0), V.m0, V.q0 | id, tail);
    leafq_push_all(S, lanes(V.m1), V.m1, V.q1 | id, tail);
    leafq_push_all(S, lanes(V.m2), V.m2, V.q2 | id, tail);
    leafq_push_all(S, lanes(V.m3), V.m3, V.q3 | id, tail);
    constexpr int LV = LDS::LV;
    typedef typename LDS::stk_t stk_t;
    if (lanes(V.pd & bal(V.l3 < LV))) S.stk[V.l3][id] = (stk_t)V.rd;
    if (lanes(V.pg & bal(V.l2 < LV))) S.stk[V.l2][id] = (stk_t)V.rg;
    if (lanes(V.pb & bal(V.l1 < LV))) S.stk[V.l1][id] = (stk_t)V.rb;
    if (bal((V.sp_new > V.l3) & (V.sp_new > LV))) {
        if (lanes(V.pd & bal(V.l3 >= LV))) M.spill[(size_t)(V.l3 - LV) * M.M.spill_stride + g] = V.rd;
        if (lanes(V.pg & bal(V.l2 >= LV))) M.spill[(size_t)(V.l2 - LV) * M.M.spill_stride + g] = V.rg;
        if (lanes(V.pb & bal(V.l1 >= LV))) M.spill[(size_t)(V.l1 - LV) * M.M.spill_stride + g] = V.rb;
    }
}

} // namespace crtk
#endif
