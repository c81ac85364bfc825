// cudaraytracing_amd/csrc/crt_mega3_math.h -- k_mega3's box and triangle arithmetic: the slab tests of the 2-wide and 4-wide nodes, the packed
// operand-select forms they are built from, the pair of Moeller-Trumbore tests of a leaf record.  Included by crt_mega3.hip only.
#ifndef CRT_MEGA3_MATH_H
#define CRT_MEGA3_MATH_H
#include "crt_internal.h"

namespace crtk {

__device__ __forceinline__ float fmin3(float a, float b, float c) { return __builtin_fminf(__builtin_fminf(a, b), c); }
__device__ __forceinline__ float fmax3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }
__device__ __forceinline__ v2f v2(float a, float b) { v2f r; r.x = a; r.y = b; return r; }
__device__ __forceinline__ v2f v2s(float a) { v2f r; r.x = a; r.y = a; return r; }

// 1 / d per component (Ray.cuh:14), bit for bit the IEEE quotient: the short reciprocal where it is proven equal (rcp_ieee),
// the division itself for the other lanes behind a wave-uniform branch.
__device__ __forceinline__ F3 inv3_exact(const F3 d)
{
    F3 inv = f3(rcp_short(d.x), rcp_short(d.y), rcp_short(d.z));
    asm volatile("" : "+v"(inv.x), "+v"(inv.y), "+v"(inv.z));
    const bool ok = rcp_short_ok3(d.x, d.y, d.z);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(!ok) != 0, 0)) {
        if (!ok) inv = f3(1 / d.x, 1 / d.y, 1 / d.z);
    }
    return inv;
}


// Both child boxes of an inner node at once (hit_AABB, DeviceBVH.cuh:87-126); lane .x = left child, .y = right child.
// Node layout: crt_device.h (nodes3).  exact = reference arithmetic (sign-selected planes, x<y?x:y minima) for rays with
// non-finite operands; otherwise minima / maxima of the two plane distances, which are the same numbers.
__device__ __forceinline__ void slab_pair(const float4 n0, const float4 n1, const float4 n2, const F3 o, const F3 inv, const F3 d, const bool exact,
                                          bool& hl, bool& hr, float& tl, float& tr)
{
    const v2f tx0 = (v2(n0.x, n0.y) - v2s(o.x)) * v2s(inv.x), ty0 = (v2(n0.z, n0.w) - v2s(o.y)) * v2s(inv.y), tz0 = (v2(n1.x, n1.y) - v2s(o.z)) * v2s(inv.z);
    const v2f tx1 = (v2(n1.z, n1.w) - v2s(o.x)) * v2s(inv.x), ty1 = (v2(n2.x, n2.y) - v2s(o.y)) * v2s(inv.y), tz1 = (v2(n2.z, n2.w) - v2s(o.z)) * v2s(inv.z);
    float el, er, xl, xr;
    if (!exact) {
        el = fmax3(__builtin_fminf(tx0.x, tx1.x), __builtin_fminf(ty0.x, ty1.x), __builtin_fminf(tz0.x, tz1.x));
        er = fmax3(__builtin_fminf(tx0.y, tx1.y), __builtin_fminf(ty0.y, ty1.y), __builtin_fminf(tz0.y, tz1.y));
        xl = fmin3(__builtin_fmaxf(tx0.x, tx1.x), __builtin_fmaxf(ty0.x, ty1.x), __builtin_fmaxf(tz0.x, tz1.x));
        xr = fmin3(__builtin_fmaxf(tx0.y, tx1.y), __builtin_fmaxf(ty0.y, ty1.y), __builtin_fmaxf(tz0.y, tz1.y));
    } else {
        const bool nx = d.x < 0, ny = d.y < 0, nz = d.z < 0; // the swap of DeviceBVH.cuh:101-119
        el = maxf_ref(maxf_ref(nx ? tx1.x : tx0.x, ny ? ty1.x : ty0.x), nz ? tz1.x : tz0.x);
        er = maxf_ref(maxf_ref(nx ? tx1.y : tx0.y, ny ? ty1.y : ty0.y), nz ? tz1.y : tz0.y);
        xl = minf_ref(minf_ref(nx ? tx0.x : tx1.x, ny ? ty0.x : ty1.x), nz ? tz0.x : tz1.x);
        xr = minf_ref(minf_ref(nx ? tx0.y : tx1.y, ny ? ty0.y : ty1.y), nz ? tz0.y : tz1.y);
    }
    hl = (el <= xl + CRT_EPSILON) & (xl >= 0);
    hr = (er <= xr + CRT_EPSILON) & (xr >= 0);
    tl = el; tr = er;
}

// slab_pair for rays with finite operands, with the pruning test folded in: returns each child's entry distance, or +inf when
// the box is missed (hit_AABB: t_enter <= t_exit + EPSILON && t_exit >= 0) or entered beyond `bound`
// (t_enter <= min(t_exit + EPSILON, bound) is the conjunction of the two upper limits; a NaN box -- an empty slot -- fails).
__device__ __forceinline__ void slab_pair_pruned(const float4 n0, const float4 n1, const float4 n2, const F3 o, const F3 inv, const float bound,
                                                 float& tl, float& tr)
{
    const v2f tx0 = (v2(n0.x, n0.y) - v2s(o.x)) * v2s(inv.x), ty0 = (v2(n0.z, n0.w) - v2s(o.y)) * v2s(inv.y), tz0 = (v2(n1.x, n1.y) - v2s(o.z)) * v2s(inv.z);
    const v2f tx1 = (v2(n1.z, n1.w) - v2s(o.x)) * v2s(inv.x), ty1 = (v2(n2.x, n2.y) - v2s(o.y)) * v2s(inv.y), tz1 = (v2(n2.z, n2.w) - v2s(o.z)) * v2s(inv.z);
    const float el = fmax3(__builtin_fminf(tx0.x, tx1.x), __builtin_fminf(ty0.x, ty1.x), __builtin_fminf(tz0.x, tz1.x));
    const float er = fmax3(__builtin_fminf(tx0.y, tx1.y), __builtin_fminf(ty0.y, ty1.y), __builtin_fminf(tz0.y, tz1.y));
    const float xl = fmin3(__builtin_fmaxf(tx0.x, tx1.x), __builtin_fmaxf(ty0.x, ty1.x), __builtin_fmaxf(tz0.x, tz1.x));
    const float xr = fmin3(__builtin_fmaxf(tx0.y, tx1.y), __builtin_fmaxf(ty0.y, ty1.y), __builtin_fmaxf(tz0.y, tz1.y));
    const float inf = pinf();
    tl = ((el <= __builtin_fminf(xl + CRT_EPSILON, bound)) & (xl >= 0)) ? el : inf;
    tr = ((er <= __builtin_fminf(xr + CRT_EPSILON, bound)) & (xr >= 0)) ? er : inf;
}

// Plane-major nodes (CRT_NODE_SIGNSEL): the four children's near planes and far planes of each axis arrive as one float4 each,
// picked per ray by the sign of its direction -- hit_AABB's own swap (DeviceBVH.cuh:101-119) done by the load address instead
// of by comparisons: t_enter = max of the three near distances, t_exit = min of the three far ones (no operand is a NaN for a
// ray with finite origin and 1/d and a finite box: x>y?x:y and v_max3 / v_min3 are the same numbers).  An empty slot is the
// inverted box (+inf, -inf): t_enter = +inf, t_exit = -inf for either sign.
template <bool PRUNE = true>
__device__ __forceinline__ void slab_quad_pruned(const float4 nx, const float4 fx, const float4 ny, const float4 fy, const float4 nz, const float4 fz,
                                                 const F3 o, const F3 inv, const float bound, float& t0, float& t1, float& t2, float& t3)
{
    const v2f nxa = (v2(nx.x, nx.y) - v2s(o.x)) * v2s(inv.x), nxb = (v2(nx.z, nx.w) - v2s(o.x)) * v2s(inv.x);
    const v2f nya = (v2(ny.x, ny.y) - v2s(o.y)) * v2s(inv.y), nyb = (v2(ny.z, ny.w) - v2s(o.y)) * v2s(inv.y);
    const v2f nza = (v2(nz.x, nz.y) - v2s(o.z)) * v2s(inv.z), nzb = (v2(nz.z, nz.w) - v2s(o.z)) * v2s(inv.z);
    const v2f fxa = (v2(fx.x, fx.y) - v2s(o.x)) * v2s(inv.x), fxb = (v2(fx.z, fx.w) - v2s(o.x)) * v2s(inv.x);
    const v2f fya = (v2(fy.x, fy.y) - v2s(o.y)) * v2s(inv.y), fyb = (v2(fy.z, fy.w) - v2s(o.y)) * v2s(inv.y);
    const v2f fza = (v2(fz.x, fz.y) - v2s(o.z)) * v2s(inv.z), fzb = (v2(fz.z, fz.w) - v2s(o.z)) * v2s(inv.z);
    const float e0 = fmax3(nxa.x, nya.x, nza.x), e1 = fmax3(nxa.y, nya.y, nza.y), e2 = fmax3(nxb.x, nyb.x, nzb.x), e3 = fmax3(nxb.y, nyb.y, nzb.y);
    const float x0 = fmin3(fxa.x, fya.x, fza.x), x1 = fmin3(fxa.y, fya.y, fza.y), x2 = fmin3(fxb.x, fyb.x, fzb.x), x3 = fmin3(fxb.y, fyb.y, fzb.y);
    const float inf = pinf();
    if (PRUNE) {
        t0 = ((e0 <= __builtin_fminf(x0 + CRT_EPSILON, bound)) & (x0 >= 0)) ? e0 : inf;
        t1 = ((e1 <= __builtin_fminf(x1 + CRT_EPSILON, bound)) & (x1 >= 0)) ? e1 : inf;
        t2 = ((e2 <= __builtin_fminf(x2 + CRT_EPSILON, bound)) & (x2 >= 0)) ? e2 : inf;
        t3 = ((e3 <= __builtin_fminf(x3 + CRT_EPSILON, bound)) & (x3 >= 0)) ? e3 : inf;
    } else { // no bound (CRT_TRAVERSAL_EXACT): hit_AABB's own test
        t0 = ((e0 <= x0 + CRT_EPSILON) & (x0 >= 0)) ? e0 : inf;
        t1 = ((e1 <= x1 + CRT_EPSILON) & (x1 >= 0)) ? e1 : inf;
        t2 = ((e2 <= x2 + CRT_EPSILON) & (x2 >= 0)) ? e2 : inf;
        t3 = ((e3 <= x3 + CRT_EPSILON) & (x3 >= 0)) ? e3 : inf;
    }
}

// (plane pair - o_axis) * inv_axis for two children at once, with the ray's scalar BROADCAST by the instruction's own operand selects
// (op_sel / op_sel_hi pick the low or the high half of a 64-bit register pair for both result halves): the reference's two roundings per
// plane (DeviceBVH.cuh:95-100), and no move that builds a (x, x) pair -- left to itself the compiler builds such pairs for half of these
// instructions (nine v_mov per visit in round 5, and the duplicates cost registers: the second visit's 1 / d went to scratch memory).
// HALF: 0 = the scalar is the pair's low half, 1 = its high half.
#define CRT_PK_SUBMUL_IMPL(OH, IH)                                                                                          \
    v2f d_;                                                                                                                 \
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0," #OH "] op_sel_hi:[1," #OH "] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d_) : "v"(p), "v"(o)); \
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0," #IH "] op_sel_hi:[1," #IH "]" : "=v"(d_) : "v"(d_), "v"(i));                    \
    return d_;
__device__ __forceinline__ v2f pk_submul_ll(const v2f p, const v2f o, const v2f i) { CRT_PK_SUBMUL_IMPL(0, 0) }
__device__ __forceinline__ v2f pk_submul_hh(const v2f p, const v2f o, const v2f i) { CRT_PK_SUBMUL_IMPL(1, 1) }
#undef CRT_PK_SUBMUL_IMPL
// (pair.H, pair.H) * x and (pair.H, pair.H) - x: a ray's scalar against two triangles' values, the scalar picked from an aligned pair by the
// instruction (tri_pair).  The products and differences are the plain IEEE ones of the scalar form.
template <int H>
__device__ __forceinline__ v2f pk_bmul(const v2f pair, const v2f x)
{
    v2f d_;
    if (H == 0) asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(d_) : "v"(pair), "v"(x));
    else asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(d_) : "v"(pair), "v"(x));
    return d_;
}
template <int H>
__device__ __forceinline__ v2f pk_bsub(const v2f pair, const v2f x)
{
    v2f d_;
    if (H == 0) asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d_) : "v"(pair), "v"(x));
    else asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d_) : "v"(pair), "v"(x));
    return d_;
}
// the ray as the 4-wide step keeps it: (o.x, o.y), (o.z, -) and (1/d.x, 1/d.y), (1/d.z, -) in aligned register pairs
struct RayPk { v2f oxy, oz, ixy, iz; };

// The same four boxes with the accept test of hit_AABB (DeviceBVH.cuh:121-125) handed back as predicates beside the entry distances:
// the decoupled step needs "hit" as a wave mask (its leaf-queue appends) and as a lane predicate, and the distance only to put the
// nearest inner child first -- a distance forced to +inf and compared with +inf again costs a select and a compare per child.
__device__ __forceinline__ void slab_quad_hits(const float4 nx, const float4 fx, const float4 ny, const float4 fy, const float4 nz, const float4 fz,
                                               const RayPk& R, float& e0, float& e1, float& e2, float& e3,
                                               unsigned long long& h0, unsigned long long& h1, unsigned long long& h2, unsigned long long& h3)
{
    const v2f nxa = pk_submul_ll(v2(nx.x, nx.y), R.oxy, R.ixy), nxb = pk_submul_ll(v2(nx.z, nx.w), R.oxy, R.ixy);
    const v2f nya = pk_submul_hh(v2(ny.x, ny.y), R.oxy, R.ixy), nyb = pk_submul_hh(v2(ny.z, ny.w), R.oxy, R.ixy);
    const v2f nza = pk_submul_ll(v2(nz.x, nz.y), R.oz, R.iz), nzb = pk_submul_ll(v2(nz.z, nz.w), R.oz, R.iz);
    const v2f fxa = pk_submul_ll(v2(fx.x, fx.y), R.oxy, R.ixy), fxb = pk_submul_ll(v2(fx.z, fx.w), R.oxy, R.ixy);
    const v2f fya = pk_submul_hh(v2(fy.x, fy.y), R.oxy, R.ixy), fyb = pk_submul_hh(v2(fy.z, fy.w), R.oxy, R.ixy);
    const v2f fza = pk_submul_ll(v2(fz.x, fz.y), R.oz, R.iz), fzb = pk_submul_ll(v2(fz.z, fz.w), R.oz, R.iz);
    e0 = fmax3(nxa.x, nya.x, nza.x); e1 = fmax3(nxa.y, nya.y, nza.y); e2 = fmax3(nxb.x, nyb.x, nzb.x); e3 = fmax3(nxb.y, nyb.y, nzb.y);
    const float x0 = fmin3(fxa.x, fya.x, fza.x), x1 = fmin3(fxa.y, fya.y, fza.y), x2 = fmin3(fxb.x, fyb.x, fzb.x), x3 = fmin3(fxb.y, fyb.y, fzb.y);
    // (a wave mask per child: the AND of the two compares' own results -- a ballot of their conjunction would cost a select and a compare)
    h0 = __builtin_amdgcn_ballot_w64(e0 <= x0 + CRT_EPSILON) & __builtin_amdgcn_ballot_w64(x0 >= 0);
    h1 = __builtin_amdgcn_ballot_w64(e1 <= x1 + CRT_EPSILON) & __builtin_amdgcn_ballot_w64(x1 >= 0);
    h2 = __builtin_amdgcn_ballot_w64(e2 <= x2 + CRT_EPSILON) & __builtin_amdgcn_ballot_w64(x2 >= 0);
    h3 = __builtin_amdgcn_ballot_w64(e3 <= x3 + CRT_EPSILON) & __builtin_amdgcn_ballot_w64(x3 >= 0);
}

// The two triangles of a leaf record at once: Moeller-Trumbore exactly as DeviceTriangle.cuh:39-56 + inside() :58-65 +
// the t > EPSILON filter of DeviceBVHNode::hit (DeviceBVH.cuh:37); lane .x = first triangle, .y = second.
// (round 6: o and d arrive as the aligned register pairs their LDS records are read into -- (o.x, o.y), (o.z, -), (d.x, d.y), (d.z, -) -- and the
// twelve instructions that take one of their components against both triangles pick it with operand selects: no (x, x) pair is built)
__device__ __forceinline__ void tri_pair(const float4 g0, const float4 g1, const float4 g2, const float4 g3, const float4 g4, const v2f oxy, const v2f oz,
                                         const v2f dxy, const v2f dz, bool& a0, bool& a1, float& t0, float& t1)
{
    const v2f v1x = v2(g0.x, g0.y), v1y = v2(g0.z, g0.w), v1z = v2(g1.x, g1.y);
    const v2f e1x = v2(g1.z, g1.w), e1y = v2(g2.x, g2.y), e1z = v2(g2.z, g2.w);
    const v2f e2x = v2(g3.x, g3.y), e2y = v2(g3.z, g3.w), e2z = v2(g4.x, g4.y);
    const v2f sx = pk_bsub<0>(oxy, v1x), sy = pk_bsub<1>(oxy, v1y), sz = pk_bsub<0>(oz, v1z);
    // s1 = d x e2, s2 = s x e1 (OrthoMethods.h:106-108)
    const v2f s1x = pk_bmul<1>(dxy, e2z) - pk_bmul<0>(dz, e2y), s1y = pk_bmul<0>(dz, e2x) - pk_bmul<0>(dxy, e2z), s1z = pk_bmul<0>(dxy, e2y) - pk_bmul<1>(dxy, e2x);
    const v2f s2x = sy * e1z - sz * e1y, s2y = sz * e1x - sx * e1z, s2z = sx * e1y - sy * e1x;
    const v2f det = s1x * e1x + (s1y * e1y + s1z * e1z);
    v2f rcp; // 1 / det (DeviceTriangle.cuh:47), see rcp_ieee
    {
        v2f r0;
        r0.x = __builtin_amdgcn_rcpf(det.x); r0.y = __builtin_amdgcn_rcpf(det.y);
        rcp = __builtin_elementwise_fma(__builtin_elementwise_fma(-det, r0, v2s(1.0f)), r0, r0);
        asm volatile("" : "+v"(rcp)); // (keeps the short form ahead of the branch instead of in an else-arm)
        const bool ok = rcp_short_ok2(det.x, det.y);
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(!ok) != 0, 0)) {
            if (!ok) { rcp.x = 1 / det.x; rcp.y = 1 / det.y; }
        }
    }
    const v2f beta = (s1x * sx + (s1y * sy + s1z * sz)) * rcp;
    const v2f gamma = (pk_bmul<0>(dxy, s2x) + (pk_bmul<1>(dxy, s2y) + pk_bmul<0>(dz, s2z))) * rcp;
    const v2f t = (s2x * e2x + (s2y * e2y + s2z * e2z)) * rcp;
    const v2f alpha = v2s(1.0f) - beta - gamma;
    // inside(): 0 < alpha, beta, gamma < 1, each comparison false for a NaN.  v_minimum3_f32 / v_maximum3_f32 (IEEE 754-2019
    // minimum / maximum) return NaN if any operand is one, so two comparisons on them are the same six (and -0 fails "0 <" either way).
    const float lo0 = __builtin_elementwise_minimum(__builtin_elementwise_minimum(alpha.x, beta.x), gamma.x);
    const float hi0 = __builtin_elementwise_maximum(__builtin_elementwise_maximum(alpha.x, beta.x), gamma.x);
    const float lo1 = __builtin_elementwise_minimum(__builtin_elementwise_minimum(alpha.y, beta.y), gamma.y);
    const float hi1 = __builtin_elementwise_maximum(__builtin_elementwise_maximum(alpha.y, beta.y), gamma.y);
    a0 = (0 < lo0) & (hi0 < 1) & (t.x > CRT_EPSILON);
    a1 = (0 < lo1) & (hi1 < 1) & (t.y > CRT_EPSILON);
    t0 = t.x; t1 = t.y;
}


} // namespace crtk
#endif
