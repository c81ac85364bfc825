// cudaraytracing_amd/csrc/crt_refit.h -- the text of crt_scene_refit (contract: include/crt.h; kernels, the handle's state and the entry
// points: crt_refit.hip): new coordinates for the triangles of a scene handle whose every topology stays.  Two parts:
//   * the device text (namespace crtk): the coordinate check, the per-triangle rows, the leaf boxes, and the inner boxes bottom-up in
//     two forms -- `levels`, one launch per node height, and `walk`, one launch in which the last thread to arrive at a node computes it;
//   * the tables both forms walk (namespace crtrefit, plain C++): made from the arrays a handle already holds, at its first refit.
// Like crt_frame_error.h the device text includes nothing, so that tools/refit_host_check.cpp compiles this very text for the host behind
// tools/host_device.h's stand-ins (float4, the bit casts, __ballot, __popcll, the agent-scope atomics, the fence); crt_triangle is
// include/crt.h's.  The tables need <vector>, <cstdint>, <cstring>.
//
// One array of boxes is the source of every stored plane: box[l] of leaf l (kernel `leaf boxes`), box[n_leaves + t] of task t.  A task
// is one inner node of one tree -- a binary node of `nodes` (SAH range and reference range; `nodes3` is the same node transposed), a node
// of `nodes4`, or a node of `nodes4i` -- with up to four children, each a box index.  A task reads its children's boxes, writes them into
// its node's planes (the stored planes are COPIES of a child's box; child 0 of a mixed nodes4i node is moved outwards to the value that
// keeps the plane's low 12 bits), and writes their union as its own box.  min and max are taken in the order of crtaccel::Box::ord_lt
// (-0 < +0), a total order on the finite floats, so a union's bits depend neither on the order nor on the grouping of its operands: the
// four-wide trees' unions of up to four boxes are the binary tree's unions of two, bit for bit.
#ifndef CRT_REFIT_H
#define CRT_REFIT_H

namespace crtk {

// What one call leaves for the host (read once, through pinned memory): vertex coordinates that are not finite or beyond 2^126 in
// magnitude (then nothing else was written), the largest |plane| of the four-wide trees as bits, the box of the reference tree's root
struct RefitResult {
    uint32_t bad, coord_max_bits;
    float root_lo[3], root_hi[3];
};

const uint32_t kRefitTriWords = 15; // sizeof(crt_triangle) / 4: v1, v2, v3, normal, area, area_of_obj, material
// RefitParams::tasks, two float4 of bits per task: (child 0 .. 3) and (meta, node, parent, -).  A child is a box index or kRefitNone; a
// binary task has two, and carries the words of its rows' w (the refs of `nodes`) in the places of children 2 and 3.
const int32_t kRefitNone = -1;
const uint32_t kRefitBinary = 0, kRefitNode4 = 1, kRefitNode4i = 2;        // meta bits 0-1: which array the node is in
const uint32_t kRefitNudge = 4u, kRefitRoot = 8u, kRefitNeedShift = 4;     // meta: child 0 keeps its planes' low 12 bits; the reference tree's root; bits 4-6: inner children

struct RefitParams {
    const float* tris;       // n_tris crt_triangle, BVH order
    const float* ltris;      // n_ltris crt_triangle, shape order
    uint32_t n_tris, n_ltris, n_rec;
    float4 *tri_geo, *tri_nm, *leaf_geo, *leaf_geo_i, *ltri;
    const int32_t* rec_map;  // dense record -> record of leaf_geo_i, or null (no nodes4i set)
    const uint32_t* leaves;  // (first triangle, triangles) per leaf
    uint32_t n_leaves, n_tasks;
    const float4* tasks;
    float4 *nodes, *nodes3, *nodes4, *nodes4i;
    float4* box;             // [(n_leaves + n_tasks) * 2]: (lo.xyz, 0), (hi.xyz, 0)
    float* cm;               // [n_tasks] a four-wide task's largest |plane| (0 for a binary task)
    unsigned int* cnt;       // [n_tasks] walk: arrivals since the tables were made
    uint32_t gen;            // walk: this call's number since then, from 1
    uint32_t first, count;   // the tasks of this launch: [first, first + count)
    RefitResult* res;
};

__device__ __forceinline__ bool refit_ord_lt(const float x, const float y) { return x < y || (x == y && (__float_as_uint(x) >> 31) > (__float_as_uint(y) >> 31)); }
__device__ __forceinline__ float refit_min(const float a, const float b) { return refit_ord_lt(b, a) ? b : a; }
__device__ __forceinline__ float refit_max(const float a, const float b) { return refit_ord_lt(a, b) ? b : a; }
__device__ __forceinline__ float refit_abs(const float x) { return __uint_as_float(__float_as_uint(x) & 0x7fffffffu); }

// crtaccel::with_bits for a finite f of magnitude <= 2^126 (the coordinate check): no value it can return is beyond the finite floats
__device__ __forceinline__ float refit_with_bits(const float f, const uint32_t chunk, const bool up)
{
    const uint32_t r = __float_as_uint(f);
    const bool neg = (r >> 31) != 0u;
    const uint32_t m = r & 0x7fffffffu;
    const bool grow = neg ? !up : up;
    uint32_t c = (m & ~0xfffu) | chunk;
    if (grow) { if (c < m) c += 0x1000u; }
    else if (c > m) {
        if (c >= 0x1000u) c -= 0x1000u;
        else return __uint_as_float(chunk | (neg ? 0u : 0x80000000u));
    }
    return __uint_as_float(c | (neg ? 0x80000000u : 0u));
}

// ---- the coordinate check: one thread per triangle and light triangle, a ballot and one atomic per wave.  Every thread of the launch
//      reaches the ballot. ----
__device__ __forceinline__ void refit_check(const RefitParams& P)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool bad = false;
    if (i < P.n_tris + P.n_ltris) {
        const float* t = i < P.n_tris ? P.tris + (size_t)i * kRefitTriWords : P.ltris + (size_t)(i - P.n_tris) * kRefitTriWords;
#pragma unroll
        for (uint32_t k = 0; k < 9u; k++) bad = bad || (__float_as_uint(t[k]) & 0x7fffffffu) > 0x7e800000u; // not finite, or |x| > 2^126
    }
    const unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63u) == 0u && m != 0ull) __hip_atomic_fetch_add(&P.res->bad, (uint32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the three rows of tri_geo of a triangle: crtlayout::build_rows
struct RefitGeo { float4 r0, r1, r2; };
__device__ __forceinline__ RefitGeo refit_geo(const float* t)
{
    const float e1x = t[3] - t[0], e1y = t[4] - t[1], e1z = t[5] - t[2];
    const float e2x = t[6] - t[0], e2y = t[7] - t[1], e2z = t[8] - t[2];
    RefitGeo g;
    g.r0 = make_float4(t[0], t[1], t[2], e1x);
    g.r1 = make_float4(e1y, e1z, e2x, e2y);
    g.r2 = make_float4(e2z, t[9], t[10], t[11]);
    return g;
}

// ---- the rows: thread i < n_tris: tri_geo and the normal of tri_nm of triangle i; the next n_rec threads: both lanes of a dense leaf
//      record and its sparse copy (crtlayout::build_leaf_records; which triangles a record holds stands in its own last row); the next
//      n_ltris: a light triangle's rows.  16-byte stores. ----
__device__ __forceinline__ void refit_rows(const RefitParams& P)
{
    if (P.res->bad != 0u) return;
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < P.n_tris) {
        const RefitGeo g = refit_geo(P.tris + (size_t)i * kRefitTriWords);
        P.tri_geo[(size_t)i * 3] = g.r0; P.tri_geo[(size_t)i * 3 + 1] = g.r1; P.tri_geo[(size_t)i * 3 + 2] = g.r2;
        const float w = P.tri_nm[i].w; // the material and its flags stay
        P.tri_nm[i] = make_float4(g.r2.y, g.r2.z, g.r2.w, w);
        return;
    }
    i -= P.n_tris;
    if (i < P.n_rec) {
        const float4 last = P.leaf_geo[(size_t)i * 5 + 4];
        const uint32_t ia = __float_as_uint(last.z), ib = __float_as_uint(last.w) > 1u ? ia + 1u : ia; // odd tail: the second lane repeats the first
        if (ia >= P.n_tris || ib >= P.n_tris) return;
        const RefitGeo a = refit_geo(P.tris + (size_t)ia * kRefitTriWords), b = refit_geo(P.tris + (size_t)ib * kRefitTriWords);
        float4 r[5];
        r[0] = make_float4(a.r0.x, b.r0.x, a.r0.y, b.r0.y);
        r[1] = make_float4(a.r0.z, b.r0.z, a.r0.w, b.r0.w);
        r[2] = make_float4(a.r1.x, b.r1.x, a.r1.y, b.r1.y);
        r[3] = make_float4(a.r1.z, b.r1.z, a.r1.w, b.r1.w);
        r[4] = make_float4(a.r2.x, b.r2.x, last.z, last.w);
        float4* o = P.leaf_geo + (size_t)i * 5;
#pragma unroll
        for (int q = 0; q < 5; q++) o[q] = r[q];
        if (P.rec_map) {
            float4* s = P.leaf_geo_i + (size_t)P.rec_map[i] * 5;
#pragma unroll
            for (int q = 0; q < 5; q++) s[q] = r[q];
        }
        return;
    }
    i -= P.n_rec;
    if (i < P.n_ltris) {
        const float* t = P.ltris + (size_t)i * kRefitTriWords;
        float4* o = P.ltri + (size_t)i * 4;
        const float4 ke = o[3]; // the emission stays
        o[0] = make_float4(t[0], t[1], t[2], t[3]);
        o[1] = make_float4(t[4], t[5], t[6], t[7]);
        o[2] = make_float4(t[8], t[9], t[10], t[11]);
        o[3] = make_float4(ke.x, ke.y, ke.z, t[13]);
    }
}

// ---- the leaf boxes: one thread per leaf, min and max of the nine coordinates of each of its triangles ----
__device__ __forceinline__ void refit_leaf_box(const RefitParams& P)
{
    if (P.res->bad != 0u) return;
    const uint32_t l = blockIdx.x * 256u + threadIdx.x;
    if (l >= P.n_leaves) return;
    const uint32_t it = P.leaves[2 * (size_t)l], n = P.leaves[2 * (size_t)l + 1];
    const float* t = P.tris + (size_t)it * kRefitTriWords;
    float lo[3] = {t[0], t[1], t[2]}, hi[3] = {t[0], t[1], t[2]};
    for (uint32_t k = 0; k < n; k++, t += kRefitTriWords)
#pragma unroll
        for (int v = 0; v < 9; v++) { lo[v % 3] = refit_min(lo[v % 3], t[v]); hi[v % 3] = refit_max(hi[v % 3], t[v]); }
    P.box[2 * (size_t)l] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    P.box[2 * (size_t)l + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    if (P.n_tasks == 0u && l == 0u) { // a scene that is one leaf: its box is the root's
        for (int a = 0; a < 3; a++) { P.res->root_lo[a] = lo[a]; P.res->root_hi[a] = hi[a]; }
    }
}

// ---- one task: its children's boxes into its node's planes, their union into its own box ----
__device__ __forceinline__ void refit_task(const RefitParams& P, const uint32_t t)
{
    const float4 c4 = P.tasks[2 * (size_t)t], m4 = P.tasks[2 * (size_t)t + 1];
    const uint32_t meta = __float_as_uint(m4.x), node = __float_as_uint(m4.y), kind = meta & 3u;
    const int32_t ref[4] = {(int32_t)__float_as_uint(c4.x), (int32_t)__float_as_uint(c4.y), (int32_t)__float_as_uint(c4.z), (int32_t)__float_as_uint(c4.w)};
    const float pinf = __uint_as_float(0x7f800000u), ninf = __uint_as_float(0xff800000u);
    float lo[4][3], hi[4][3], olo[3] = {pinf, pinf, pinf}, ohi[3] = {ninf, ninf, ninf}, cm = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const bool used = (c < 2 || kind != kRefitBinary) && ref[c] >= 0;
        float4 a = make_float4(pinf, pinf, pinf, 0.0f), b = make_float4(ninf, ninf, ninf, 0.0f); // an empty slot: the inverted box, as it stands
        if (used) { a = P.box[2 * (size_t)ref[c]]; b = P.box[2 * (size_t)ref[c] + 1]; }
        lo[c][0] = a.x; lo[c][1] = a.y; lo[c][2] = a.z; hi[c][0] = b.x; hi[c][1] = b.y; hi[c][2] = b.z;
        if (used) {
#pragma unroll
            for (int x = 0; x < 3; x++) { olo[x] = refit_min(olo[x], lo[c][x]); ohi[x] = refit_max(ohi[x], hi[c][x]); }
        }
    }
    P.box[2 * ((size_t)P.n_leaves + t)] = make_float4(olo[0], olo[1], olo[2], 0.0f);
    P.box[2 * ((size_t)P.n_leaves + t) + 1] = make_float4(ohi[0], ohi[1], ohi[2], 0.0f);
    if (kind == kRefitBinary) {
        float4* o = P.nodes + (size_t)node * 4;
        o[0] = make_float4(lo[0][0], lo[0][1], lo[0][2], c4.z);
        o[1] = make_float4(hi[0][0], hi[0][1], hi[0][2], c4.w);
        o[2] = make_float4(lo[1][0], lo[1][1], lo[1][2], 0.0f);
        o[3] = make_float4(hi[1][0], hi[1][1], hi[1][2], 0.0f);
        float4* o3 = P.nodes3 + (size_t)node * 4; // crtlayout::build_nodes3: (left, right) pairs; row 3, the refs, stays
        o3[0] = make_float4(lo[0][0], lo[1][0], lo[0][1], lo[1][1]);
        o3[1] = make_float4(lo[0][2], lo[1][2], hi[0][0], hi[1][0]);
        o3[2] = make_float4(hi[0][1], hi[1][1], hi[0][2], hi[1][2]);
        if (meta & kRefitRoot) {
            for (int a = 0; a < 3; a++) { P.res->root_lo[a] = olo[a]; P.res->root_hi[a] = ohi[a]; }
        }
    } else {
        float4* o = kind == kRefitNode4 ? P.nodes4 + (size_t)node * 8 : P.nodes4i + (size_t)node * 6;
        if (meta & kRefitNudge) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const uint32_t chunk = __float_as_uint(o[2 * a].x) & 0xfffu; // the same bits stand in the plane's lo and hi
                lo[0][a] = refit_with_bits(lo[0][a], chunk, false);
                hi[0][a] = refit_with_bits(hi[0][a], chunk, true);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (ref[c] >= 0) {
#pragma unroll
                for (int a = 0; a < 3; a++) cm = refit_max(cm, refit_max(refit_abs(lo[c][a]), refit_abs(hi[c][a])));
            }
#pragma unroll
        for (int a = 0; a < 3; a++) { // plane-major: [2 a] = lo of axis a of the four children, [2 a + 1] = hi
            o[2 * a] = make_float4(lo[0][a], lo[1][a], lo[2][a], lo[3][a]);
            o[2 * a + 1] = make_float4(hi[0][a], hi[1][a], hi[2][a], hi[3][a]);
        }
    }
    P.cm[t] = cm;
}

// ---- form `levels`: the tasks of one height; the kernel boundary hands the boxes of the height below over ----
__device__ __forceinline__ void refit_level(const RefitParams& P)
{
    if (P.res->bad != 0u) return;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < P.count) refit_task(P, P.first + i);
}

// what stands between a task's stores and its arrival at the parent, and between the last arrival and the loads of the children's boxes
__device__ __forceinline__ void refit_release()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // (the fence's own wait may be dropped in front of an atomic whose result is used: kept by hand)
#endif
}
__device__ __forceinline__ void refit_acquire() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); }

// ---- form `walk`: one launch.  A thread starts at a task whose children are all leaves (tasks [0, count): height 0), computes it, and
//      arrives at the parent; of the arrivals at a node -- one per inner child -- the last computes the node and goes on up, the others
//      end.  Nobody waits: no spin, no poll, so the launch needs no residency and ends whatever the order its waves run in.
//      Ordering: a child's thread W writes the child's box (plain stores), then an agent-scope release fence, then adds to the parent's
//      counter; the last arriver R reads its own add's result, finds it complete, then an agent-scope acquire fence, then loads the
//      children's boxes.  R's add reads the value W's add wrote (or one a later add of the same chain wrote): the counter's modification
//      order puts W's add before R's, so W's release fence synchronizes with R's acquire fence and W's stores happen before R's loads.
//      On the device the release writes this wave's lines back to where every compute unit reads them, and the acquire drops the lines
//      R's compute unit holds, so that no plain load of a box can be answered from a copy older than the hand-off.  The boxes are read
//      through the vector path only (P.box is not const __restrict__).
//      A counter is never zeroed between calls: call number g finds it at (g - 1) * need and leaves it at g * need. ----
__device__ __forceinline__ void refit_walk(const RefitParams& P)
{
    if (P.res->bad != 0u) return;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.count) return;
    uint32_t t = i;
    for (;;) {
        refit_task(P, t);
        const int32_t parent = (int32_t)__float_as_uint(P.tasks[2 * (size_t)t + 1].z);
        if (parent < 0) return;
        const uint32_t need = (__float_as_uint(P.tasks[2 * (size_t)parent + 1].x) >> kRefitNeedShift) & 7u;
        refit_release();
        const uint32_t before = __hip_atomic_fetch_add(&P.cnt[parent], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (before + 1u != need * P.gen) return;
        refit_acquire();
        t = (uint32_t)parent;
    }
}

// ---- coord_max: one block; a non-negative float's order is its bits' ----
__device__ __forceinline__ void refit_finish(const RefitParams& P)
{
    if (P.res->bad != 0u) return;
    uint32_t m = 0u;
    for (uint32_t i = threadIdx.x; i < P.n_tasks; i += 256u) { const uint32_t b = __float_as_uint(P.cm[i]); m = b > m ? b : m; }
    if (m != 0u) __hip_atomic_fetch_max(&P.res->coord_max_bits, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

} // namespace crtk

// ---- the tables, from the arrays of a handle (or of a crtlayout::SceneLayout): rows of four floats each ----
namespace crtrefit {

struct Arrays {
    const float *nodes, *nodes4, *nodes4i, *leaf_geo; // nodes4i: null without the set
    size_t n_nodes2;                                  // binary nodes of `nodes`, both ranges (0: the tree is one leaf)
    size_t n_nodes4;                                  // crt_accel_info::n_nodes4
    size_t n_rec;                                     // dense leaf records
    const int32_t *rec_map, *leaf_count;
    int32_t root_fast, root_exact, root4, root4i;
    uint32_t n_mixed4i, n_tris;
};

struct Tables {
    std::vector<uint32_t> leaves;   // (first triangle, triangles) per leaf
    std::vector<uint32_t> tasks;    // 8 words per task, numbered by height
    std::vector<uint32_t> level;    // tasks of height h: [level[h], level[h + 1])
    uint32_t n_leaves = 0, n_tasks = 0, boxes = 0;
};

inline int32_t bits_of(float f) { int32_t v; std::memcpy(&v, &f, 4); return v; }

// false: an array is not what crt_scene_layout.h builds (a child that does not follow its parent, a ref out of range)
inline bool build_tables(const Arrays& A, Tables& T)
{
    T = Tables();
    std::vector<int32_t> leaf_of_it(A.n_tris, -1);
    auto leaf_of_ref = [&](int32_t r) -> int32_t { // a leaf ref of `nodes`: ~(first triangle << 4 | count, 0: leaf_count's)
        const uint32_t u = ~(uint32_t)r, it = u >> 4;
        if (it >= A.n_tris) return -1;
        if (leaf_of_it[it] < 0) {
            const uint32_t n = (u & 15u) ? (u & 15u) : (uint32_t)A.leaf_count[it];
            if (n == 0 || (uint64_t)it + n > A.n_tris) return -1;
            leaf_of_it[it] = (int32_t)(T.leaves.size() / 2);
            T.leaves.push_back(it); T.leaves.push_back(n);
        }
        return leaf_of_it[it];
    };
    struct Task { uint32_t kind, node, flags; int32_t child[4], parent; uint32_t raw[2]; int height; };
    std::vector<Task> tasks;
    bool ok = true;
    // a tree's nodes [0, n) as tasks [base, base + n); ref_of(node, slot): >= 0 a node of the tree, kNone, or ~leaf
    const int32_t kNone = INT32_MIN;
    auto add_tree = [&](uint32_t kind, size_t n, int slots, auto ref_of, auto flags_of) {
        const size_t base = tasks.size();
        if (n == 0) { ok = false; return; }
        tasks.resize(base + n);
        for (size_t q = 0; q < n; q++) {
            Task& t = tasks[base + q];
            t.kind = kind; t.node = (uint32_t)q; t.flags = flags_of(q); t.height = 0;
            t.parent = -1;
            for (int c = 0; c < 4; c++) {
                const int32_t r = c < slots ? ref_of(q, c) : kNone;
                if (r == kNone) { t.child[c] = kNone; continue; }
                if (r >= 0) {
                    if ((size_t)r == q || (size_t)r >= n) { ok = false; t.child[c] = kNone; continue; }
                    t.child[c] = (int32_t)(base + (size_t)r);
                } else t.child[c] = r; // ~leaf
            }
        }
        // from the root, node 0, breadth first: every node once (a tree), the parents, and the heights in the reverse order
        std::vector<size_t> order(1, base);
        std::vector<uint8_t> seen(n, 0);
        if (n) seen[0] = 1;
        for (size_t i = 0; i < order.size(); i++)
            for (int c = 0; c < 4; c++) {
                const int32_t k = tasks[order[i]].child[c];
                if (k < 0) continue;
                if (seen[(size_t)k - base]) { ok = false; tasks[order[i]].child[c] = kNone; continue; }
                seen[(size_t)k - base] = 1;
                tasks[(size_t)k].parent = (int32_t)order[i];
                order.push_back((size_t)k);
            }
        if (order.size() != n) ok = false;
        for (size_t i = order.size(); i-- > 0;) {
            Task& t = tasks[order[i]];
            for (int c = 0; c < 4; c++)
                if (t.child[c] >= 0) t.height = std::max(t.height, tasks[(size_t)t.child[c]].height + 1);
        }
    };
    // `nodes`: the SAH range [0, root_exact) and the reference range behind it, each numbered from its root
    if (A.n_nodes2) {
        const size_t a_n = (size_t)A.root_exact, r_n = A.n_nodes2 - a_n;
        for (int range = 0; range < 2; range++) {
            const size_t off = range ? a_n : 0, n = range ? r_n : a_n;
            const size_t base = tasks.size();
            add_tree(crtk::kRefitBinary, n, 2,
                     [&](size_t q, int c) -> int32_t {
                         const int32_t r = bits_of(A.nodes[((off + q) * 4 + (size_t)c) * 4 + 3]);
                         if (r >= 0) return (size_t)r >= off ? (int32_t)((size_t)r - off) : (int32_t)n; // (out of the range: refused)
                         const int32_t l = leaf_of_ref(r);
                         if (l < 0) { ok = false; return kNone; }
                         return ~l;
                     },
                     [&](size_t q) { return (range == 1 && q == 0) ? crtk::kRefitRoot : 0u; });
            for (size_t q = 0; q < n; q++) {
                Task& t = tasks[base + q];
                t.node = (uint32_t)(off + q);
                t.raw[0] = (uint32_t)bits_of(A.nodes[((off + q) * 4 + 0) * 4 + 3]); t.raw[1] = (uint32_t)bits_of(A.nodes[((off + q) * 4 + 1) * 4 + 3]);
            }
        }
    } else if (A.root_fast < 0) {
        if (leaf_of_ref(A.root_fast) < 0) ok = false;
    }
    // a leaf by its first dense record: the record's last row names its first triangle
    auto leaf_of_rec = [&](size_t rec) -> int32_t {
        if (rec >= A.n_rec) return -1;
        const uint32_t it = (uint32_t)bits_of(A.leaf_geo[(rec * 5 + 4) * 4 + 2]);
        return it < A.n_tris ? leaf_of_it[it] : -1;
    };
    if (A.root4 >= 0) {
        add_tree(crtk::kRefitNode4, A.n_nodes4, 4,
                 [&](size_t q, int c) -> int32_t {
                     const int32_t r = bits_of(A.nodes4[(q * 8 + 6) * 4 + (size_t)c]);
                     if (r >= 0) return r;
                     if (r == ~0x7ffffff0) return kNone;
                     const int32_t l = leaf_of_rec((size_t)~r);
                     if (l < 0) { ok = false; return kNone; }
                     return ~l;
                 },
                 [&](size_t) { return 0u; });
        if (A.nodes4i) {
            // the refs nodes4i implies (crtlayout::build_nodes4i): a mixed node's (fm, ff, mixed, fringe children) in the low 12 bits of
            // the planes of child 0; leaf child o of node n is record 4 n + o of the sparse copy
            std::vector<int32_t> dense_of((A.n_nodes4 + 1) * 4, -1);
            for (size_t r = 0; r < A.n_rec; r++)
                if (A.rec_map[r] >= 0 && (size_t)A.rec_map[r] < dense_of.size()) dense_of[(size_t)A.rec_map[r]] = (int32_t)r;
            // numbered from the root, which is node root4i = 0 of the mixed range (or of the fringe range when there is no mixed node)
            if (A.root4i != 0) ok = false;
            add_tree(crtk::kRefitNode4i, A.n_nodes4, 4,
                     [&](size_t q, int c) -> int32_t {
                         uint32_t fm = 0, ff = 0, n_m = 0, n_f = 0;
                         if (q < A.n_mixed4i) {
                             uint32_t ch[3];
                             for (int a = 0; a < 3; a++) ch[a] = (uint32_t)bits_of(A.nodes4i[(q * 6 + 2 * (size_t)a) * 4]) & 0xfffu;
                             fm = ch[0] | ((ch[1] & 7u) << 12); ff = ((ch[1] >> 3) & 0x1ffu) | ((ch[2] & 63u) << 9);
                             n_m = (ch[2] >> 6) & 7u; n_f = (ch[2] >> 9) & 7u;
                         }
                         if ((uint32_t)c < n_m) return (int32_t)(fm + (uint32_t)c);
                         if ((uint32_t)c < n_m + n_f) return (int32_t)(ff + ((uint32_t)c - n_m));
                         const int32_t dense = dense_of[q * 4 + (size_t)c];
                         if (dense < 0) return kNone;
                         const int32_t l = leaf_of_rec((size_t)dense);
                         if (l < 0) { ok = false; return kNone; }
                         return ~l;
                     },
                     [&](size_t q) { return q < A.n_mixed4i ? crtk::kRefitNudge : 0u; });
        }
    }
    if (!ok) return false;
    // number the tasks by height
    int top = -1;
    for (const Task& t : tasks) top = std::max(top, t.height);
    T.level.assign((size_t)(top + 2), 0);
    for (const Task& t : tasks) T.level[(size_t)t.height + 1]++;
    for (size_t h = 1; h < T.level.size(); h++) T.level[h] += T.level[h - 1];
    std::vector<uint32_t> number(tasks.size()), next(T.level.begin(), T.level.end());
    for (size_t i = 0; i < tasks.size(); i++) number[i] = next[(size_t)tasks[i].height]++;
    T.n_leaves = (uint32_t)(T.leaves.size() / 2);
    T.n_tasks = (uint32_t)tasks.size();
    T.tasks.assign(tasks.size() * 8, 0);
    for (size_t i = 0; i < tasks.size(); i++) {
        const Task& t = tasks[i];
        uint32_t* o = &T.tasks[(size_t)number[i] * 8];
        uint32_t need = 0;
        for (int c = 0; c < 4; c++) {
            int32_t b = crtk::kRefitNone;
            if (t.child[c] >= 0) { b = (int32_t)(T.n_leaves + number[(size_t)t.child[c]]); need++; }
            else if (t.child[c] != kNone) b = ~t.child[c];
            if (b >= 0) T.boxes += t.kind == crtk::kRefitBinary ? 2u : 1u; // (a binary node's child stands in nodes and in nodes3)
            o[c] = (uint32_t)b;
        }
        if (t.kind == crtk::kRefitBinary) { o[2] = t.raw[0]; o[3] = t.raw[1]; }
        o[4] = t.kind | t.flags | (need << crtk::kRefitNeedShift);
        o[5] = t.node;
        o[6] = t.parent < 0 ? 0xffffffffu : number[(size_t)t.parent];
        o[7] = 0;
    }
    return true;
}

} // namespace crtrefit
#endif
