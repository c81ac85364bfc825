// cudaraytracing_amd/csrc/crt_scene_layout.h -- everything crt_scene_create computes before it touches a device: the checks of a scene
// description and every array the kernels walk (layouts: crt_device.h) -- the two binary trees, the leaf records, the 4-wide collapse and
// its copy without refs (nodes4i).  Plain C++ (no HIP): crt_scene.hip uploads the arrays byte for byte; tools/scene_layout_dump.cpp builds
// them with g++ so that the invariants of the exactness proof (tests/tree_check.py) are checked on a CPU.
#ifndef CRT_SCENE_LAYOUT_H
#define CRT_SCENE_LAYOUT_H

#include "../../include/crt.h"
#include "crt_accel.h"
#include "crt_fastdiv.h"

#include <algorithm>
#include <array>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

namespace crtlayout {

struct Row4 { float x, y, z, w; };     // a row of four floats: float4's size and layout (crt_scene.hip asserts it)
struct URow4 { uint32_t x, y, z, w; }; // ... and uint4's
inline Row4 row4(float x, float y, float z, float w) { return Row4{x, y, z, w}; }

const int kNode4iF4 = 6;                // float4 per node of nodes4i (crt_device.h: NODE4I_F4)
const uint32_t kLeafRecMax = 0x7fffffu; // largest leaf record of a leaf-queue entry (crt_mega3.h: LEAF_REC_MAX)

// crtaccel::build_sah_device (crt_accel_build.hip), or null: the host builder
typedef int (*DeviceSah)(const std::vector<crtaccel::Prim>& prims, std::vector<crtaccel::Node>& nodes, int32_t& root_ref, float* device_ms, uint32_t* index_splits);

struct SceneLayout {
    std::vector<Row4> nodes, tri_geo, mats, ltri, nodes3, leaf_geo, tri_nm, nodes4, nodes4i, leaf_geo_i; // (the nodes4i set: empty without CAP_IMPL)
    std::vector<int32_t> tri_mat, leaf_count, rec_map;
    std::vector<URow4> lights;
    crt_tree_scalars scalars{}; // roots, offsets of the empty nodes, coord_max, stack_cap
    crt_accel_info accel{};     // the builder's counts and timings, depths, layout_caps (runtime_init_ms: the caller's)
    uint32_t max_leaf = 0;      // triangles in the largest leaf
};
// crt_accel_info::layout_caps: which pool layouts of the render kernel the scene allows
enum : uint32_t {
    CAP_REF16 = 1u,       // refs of the 4-wide tree and of the leaf records fit 16 bits (k_mega3's 16-bit stack layout)
    CAP_REF16_INNER = 2u, // refs of the 4-wide tree alone fit 16 bits (decoupled leaves: the stack holds inner nodes only)
    CAP_DEC = 4u,         // leaf records fit the 24 bits of a leaf-queue entry
    CAP_IMPL = 8u         // the implicit-refs copy of the 4-wide tree exists (nodes4i: leaves of one record, <= 32 768 nodes)
};

inline float as_float(int32_t v) { float f; std::memcpy(&f, &v, 4); return f; }
inline int32_t as_int(float f) { int32_t v; std::memcpy(&v, &f, 4); return v; }

// CRT_OK, or the status and the message crt_scene_create reports
inline int validate_desc(const crt_scene_desc* d, const char*& msg)
{
    auto bad = [&](int status, const char* m) { msg = m; return status; };
    if (!d || !d->nodes || !d->tris || !d->materials || d->n_nodes == 0 || d->n_tris == 0 || d->n_materials == 0)
        return bad(CRT_ERR_INVALID_ARG, "crt_scene_create: empty scene description");
    if (d->root < 0 || (uint32_t)d->root >= d->n_nodes) return bad(CRT_ERR_INVALID_ARG, "crt_scene_create: root index out of range");
    if (d->n_tris >= (1u << 27)) return bad(CRT_ERR_UNSUPPORTED, "crt_scene_create: more than 2^27 triangles");
    if (d->n_lights && (!d->lights || !d->light_tris)) return bad(CRT_ERR_INVALID_ARG, "crt_scene_create: lights without triangles");
    for (uint32_t i = 0; i < d->n_nodes; i++) {
        const crt_bvh_node& n = d->nodes[i];
        bool leaf = n.lc < 0 && n.rc < 0;
        if (leaf) {
            if (n.it < 0 || n.n == 0 || (uint64_t)n.it + n.n > d->n_tris) return bad(CRT_ERR_INVALID_ARG, "crt_scene_create: leaf range outside the triangle array");
        } else {
            // inner nodes of the reference builder always have two children (BVH.h:79-81) that precede them (post-order)
            if (n.lc < 0 || n.rc < 0 || (uint32_t)n.lc >= i || (uint32_t)n.rc >= i) return bad(CRT_ERR_INVALID_ARG, "crt_scene_create: inner node children must precede it (post-order)");
        }
    }
    {
        // every node must hang under the root exactly once (the reference builder emits a tree in post-order, BVH.h:37-84), and the
        // leaves must own disjoint triangle ranges: the FAST traversal builds its own tree over ALL leaves of the description, so a
        // leaf the reference topology cannot reach, or two leaves sharing triangles, would make the two modes disagree
        std::vector<uint8_t> seen(d->n_nodes, 0), owned(d->n_tris, 0);
        std::vector<int32_t> todo(1, d->root);
        uint32_t visited = 0;
        while (!todo.empty()) {
            const int32_t i = todo.back();
            todo.pop_back();
            if (seen[i]) return bad(CRT_ERR_INVALID_ARG, "crt_scene_create: a node is reachable from the root more than once");
            seen[i] = 1;
            visited++;
            const crt_bvh_node& n = d->nodes[i];
            if (n.lc < 0 && n.rc < 0) {
                for (uint32_t k = 0; k < n.n; k++) {
                    if (owned[(uint32_t)n.it + k]) return bad(CRT_ERR_INVALID_ARG, "crt_scene_create: two leaves share a triangle");
                    owned[(uint32_t)n.it + k] = 1;
                }
            } else { todo.push_back(n.lc); todo.push_back(n.rc); }
        }
        if (visited != d->n_nodes) return bad(CRT_ERR_INVALID_ARG, "crt_scene_create: nodes that the root does not reach");
    }
    if (d->n_materials >= (1u << 30)) return bad(CRT_ERR_INVALID_ARG, "crt_scene_create: more than 2^30 - 1 materials (the triangle rows keep two flag bits beside the index)");
    for (uint32_t i = 0; i < d->n_tris; i++)
        if (d->tris[i].material < 0 || (uint32_t)d->tris[i].material >= d->n_materials) return bad(CRT_ERR_INVALID_ARG, "crt_scene_create: triangle material index out of range");
    for (uint32_t i = 0; i < d->n_light_tris; i++)
        if (d->light_tris[i].material < 0 || (uint32_t)d->light_tris[i].material >= d->n_materials) return bad(CRT_ERR_INVALID_ARG, "crt_scene_create: light triangle material index out of range");
    for (uint32_t i = 0; i < d->n_lights; i++)
        if (d->lights[i].count == 0 || (uint64_t)d->lights[i].first_tri + d->lights[i].count > d->n_light_tris) return bad(CRT_ERR_INVALID_ARG, "crt_scene_create: light range outside the light triangle array");
    return CRT_OK;
}

// Builds the device node array (layout: crt_device.h) holding TWO trees over the same leaves:
//   [0, A)      the SAH tree of crt_accel.h, used by CRT_TRAVERSAL_FAST for rays with finite inv_dir
//   [A, A + R)  the reference's own topology (post-order BVH re-laid breadth-first), used by
//               CRT_TRAVERSAL_REFERENCE and by FAST rays whose inv_dir is not finite.
// Returns the larger tree depth (root = 1); the builder's counts and timings go to *ai.
inline int convert_bvh(const crt_scene_desc& d, std::vector<Row4>& nodes, std::vector<int32_t>& leaf_count, int32_t& root_fast, int32_t& root_exact, DeviceSah device_sah, crt_accel_info* ai = nullptr)
{
    auto is_leaf = [&](int32_t i) { return d.nodes[i].lc < 0 && d.nodes[i].rc < 0; };
    auto leaf_ref = [&](int32_t i) -> int32_t {
        const crt_bvh_node& n = d.nodes[i];
        uint32_t cnt = n.n <= 15 ? n.n : 0;
        if (n.n > 15) leaf_count[n.it] = (int32_t)n.n;
        return (int32_t)~(((uint32_t)n.it << 4) | cnt);
    };
    leaf_count.assign(d.n_tris ? d.n_tris : 1, 0);
    nodes.clear();
    if (is_leaf(d.root)) { root_fast = root_exact = leaf_ref(d.root); return 1; }

    // ---- SAH tree over the reference leaves ----
    std::vector<crtaccel::Prim> prims;
    for (uint32_t i = 0; i < d.n_nodes; i++) {
        if (!is_leaf((int32_t)i)) continue;
        crtaccel::Prim p;
        for (int a = 0; a < 3; a++) { p.box.lo[a] = d.nodes[i].aa[a]; p.box.hi[a] = d.nodes[i].bb[a]; }
        p.ref = leaf_ref((int32_t)i);
        prims.push_back(p);
    }
    std::vector<crtaccel::Node> acc;
    int32_t acc_root = 0;
    // the SAH tree over the reference leaves: on the device (crt_accel_build.hip; CRT_SAH_HOST=1 forces the host builder, which is
    // also the fallback); the 4-wide collapse stays on the host (linear, a few hundred microseconds)
    const auto sah_t0 = std::chrono::steady_clock::now();
    int depth_fast = -1;
    float dev_ms = 0.0f;
    const bool want_device = device_sah && !(std::getenv("CRT_SAH_HOST") && std::getenv("CRT_SAH_HOST")[0] == '1');
    uint32_t index_splits = 0;
    if (want_device) depth_fast = device_sah(prims, acc, acc_root, &dev_ms, &index_splits);
    const bool on_device = depth_fast >= 0;
    if (!on_device) depth_fast = crtaccel::build_sah(prims, acc, acc_root, &index_splits);
    // one pass of insertion-based optimisation over the built tree (crt_accel.h: optimize_sah; only moves that save half of what the
    // node costs where it is); CRT_SAH_OPT=<passes> / CRT_SAH_OPT_MARGIN=<fraction> override, CRT_SAH_OPT=0 leaves the tree as built
    {
        const char* opt_ = std::getenv("CRT_SAH_OPT");
        const int passes = opt_ ? std::atoi(opt_) : 1;
        const char* form_ = std::getenv("CRT_SAH_OPT_FORM"); // (A/B hook: "serial" = the pass of rounds 4 / 5, every search on the tree as the last move left it)
        if (!acc.empty() && passes > 0) depth_fast = (form_ && form_[0] == 's') ? crtaccel::optimize_sah_serial(acc, passes) : crtaccel::optimize_sah(acc, passes);
    }
    if (ai) {
        ai->n_leaves = (uint32_t)prims.size(); ai->n_nodes2 = (uint32_t)acc.size(); ai->sah_on_device = on_device ? 1u : 0u;
        ai->sah_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - sah_t0).count();
        ai->sah_device_ms = dev_ms;
        ai->index_splits = index_splits;
    }
    const int32_t A = (int32_t)acc.size();
    nodes.resize((size_t)A * 4);
    for (int32_t q = 0; q < A; q++) {
        const crtaccel::Node& n = acc[q];
        nodes[q * 4 + 0] = row4(n.box[0].lo[0], n.box[0].lo[1], n.box[0].lo[2], as_float(n.child[0]));
        nodes[q * 4 + 1] = row4(n.box[0].hi[0], n.box[0].hi[1], n.box[0].hi[2], as_float(n.child[1]));
        nodes[q * 4 + 2] = row4(n.box[1].lo[0], n.box[1].lo[1], n.box[1].lo[2], 0.0f);
        nodes[q * 4 + 3] = row4(n.box[1].hi[0], n.box[1].hi[1], n.box[1].hi[2], 0.0f);
    }
    root_fast = acc_root; // 0 (two or more leaves here)

    // ---- the reference topology, breadth-first numbering of inner nodes ----
    std::vector<int32_t> order, index(d.n_nodes, -1), depth_of;
    order.push_back(d.root);
    depth_of.push_back(1);
    index[d.root] = 0;
    int max_depth = 1;
    for (size_t q = 0; q < order.size(); q++) {
        const crt_bvh_node& n = d.nodes[order[q]];
        int32_t ch[2] = {n.lc, n.rc};
        for (int c = 0; c < 2; c++) {
            max_depth = std::max(max_depth, depth_of[q] + 1);
            if (!is_leaf(ch[c])) {
                index[ch[c]] = (int32_t)order.size();
                order.push_back(ch[c]);
                depth_of.push_back(depth_of[q] + 1);
            }
        }
    }
    nodes.resize(((size_t)A + order.size()) * 4);
    for (size_t q = 0; q < order.size(); q++) {
        const crt_bvh_node& n = d.nodes[order[q]];
        const crt_bvh_node& l = d.nodes[n.lc];
        const crt_bvh_node& r = d.nodes[n.rc];
        int32_t lref = is_leaf(n.lc) ? leaf_ref(n.lc) : A + index[n.lc];
        int32_t rref = is_leaf(n.rc) ? leaf_ref(n.rc) : A + index[n.rc];
        const size_t o = ((size_t)A + q) * 4;
        nodes[o + 0] = row4(l.aa[0], l.aa[1], l.aa[2], as_float(lref));
        nodes[o + 1] = row4(l.bb[0], l.bb[1], l.bb[2], as_float(rref));
        nodes[o + 2] = row4(r.aa[0], r.aa[1], r.aa[2], 0.0f);
        nodes[o + 3] = row4(r.bb[0], r.bb[1], r.bb[2], 0.0f);
    }
    root_exact = A;
    return std::max(max_depth, depth_fast);
}

// ---- step 1: the triangle, material and light rows (crt_device.h: tri_geo, tri_mat, tri_nm, mats, ltri, lights) ----
inline void build_rows(const crt_scene_desc& d, SceneLayout& L)
{
    L.tri_geo.resize(d.n_tris * 3ull); L.tri_mat.resize(d.n_tris); L.tri_nm.resize(d.n_tris);
    L.mats.resize(d.n_materials * 3ull); L.ltri.resize(d.n_light_tris * 4ull); L.lights.resize(d.n_lights);
    for (uint32_t i = 0; i < d.n_tris; i++) {
        const crt_triangle& t = d.tris[i];
        // e1 = v2 - v1, e2 = v3 - v1 as DeviceTriangle's constructor computes them (DeviceTriangle.cuh:27-28)
        float e1[3] = {t.v2[0] - t.v1[0], t.v2[1] - t.v1[1], t.v2[2] - t.v1[2]};
        float e2[3] = {t.v3[0] - t.v1[0], t.v3[1] - t.v1[1], t.v3[2] - t.v1[2]};
        L.tri_geo[i * 3ull + 0] = row4(t.v1[0], t.v1[1], t.v1[2], e1[0]);
        L.tri_geo[i * 3ull + 1] = row4(e1[1], e1[2], e2[0], e2[1]);
        L.tri_geo[i * 3ull + 2] = row4(e2[2], t.normal[0], t.normal[1], t.normal[2]);
        L.tri_mat[i] = t.material;
        const crt_material& m = d.materials[t.material];
        const int32_t w = (int32_t)((uint32_t)t.material | (m.has_emit ? 1u << 30 : 0u) | (m.mode == 1 ? 1u << 31 : 0u)); // TNM_* (crt_device.h)
        L.tri_nm[i] = row4(t.normal[0], t.normal[1], t.normal[2], as_float(w));
    }
    for (uint32_t i = 0; i < d.n_materials; i++) {
        const crt_material& m = d.materials[i];
        const float pi_f = (float)3.14159265358979323846;
        int32_t flags = (m.has_emit ? 1 : 0) | (m.mode == 1 ? 2 : 0);
        L.mats[i * 3ull + 0] = row4(m.kd[0] / pi_f, m.kd[1] / pi_f, m.kd[2] / pi_f, m.ns); // f_r = kd / float(M_PI) (Render.cuh:259)
        L.mats[i * 3ull + 1] = row4(m.kd[0], m.kd[1], m.kd[2], as_float(flags));
        L.mats[i * 3ull + 2] = row4(m.ke[0], m.ke[1], m.ke[2], 0.0f);
    }
    for (uint32_t i = 0; i < d.n_light_tris; i++) {
        const crt_triangle& t = d.light_tris[i];
        const crt_material& m = d.materials[t.material];
        L.ltri[i * 4ull + 0] = row4(t.v1[0], t.v1[1], t.v1[2], t.v2[0]);
        L.ltri[i * 4ull + 1] = row4(t.v2[1], t.v2[2], t.v3[0], t.v3[1]);
        L.ltri[i * 4ull + 2] = row4(t.v3[2], t.normal[0], t.normal[1], t.normal[2]);
        L.ltri[i * 4ull + 3] = row4(m.ke[0], m.ke[1], m.ke[2], t.area_of_obj);
    }
    for (uint32_t i = 0; i < d.n_lights; i++) {
        const crtdev::FastDiv fd = crtdev::make_fastdiv(d.lights[i].count);
        L.lights[i] = URow4{d.lights[i].first_tri, d.lights[i].count, fd.m, fd.sh};
    }
}

// ---- step 2: k_mega3's leaf records (crt_device.h: leaf_geo), triangle pairs per leaf; rec_of_it: first triangle of a leaf -> its first record ----
inline void build_leaf_records(const crt_scene_desc& d, SceneLayout& L, std::vector<int32_t>& rec_of_it)
{
    const std::vector<Row4>& geo = L.tri_geo;
    rec_of_it.assign(d.n_tris, -1);
    for (uint32_t i = 0; i < d.n_nodes; i++) {
        const crt_bvh_node& nn = d.nodes[i];
        if (!(nn.lc < 0 && nn.rc < 0)) continue;
        L.max_leaf = std::max(L.max_leaf, nn.n);
        rec_of_it[nn.it] = (int32_t)(L.leaf_geo.size() / 5);
        for (uint32_t k = 0; k < nn.n; k += 2) {
            const uint32_t ia = (uint32_t)nn.it + k, ib = k + 1 < nn.n ? ia + 1 : ia; // odd tail: the second lane repeats a and is masked
            const Row4 a0 = geo[ia * 3ull], a1 = geo[ia * 3ull + 1], a2 = geo[ia * 3ull + 2];
            const Row4 b0 = geo[ib * 3ull], b1 = geo[ib * 3ull + 1], b2 = geo[ib * 3ull + 2];
            L.leaf_geo.push_back(row4(a0.x, b0.x, a0.y, b0.y));  // v1.x, v1.y
            L.leaf_geo.push_back(row4(a0.z, b0.z, a0.w, b0.w));  // v1.z, e1.x
            L.leaf_geo.push_back(row4(a1.x, b1.x, a1.y, b1.y));  // e1.y, e1.z
            L.leaf_geo.push_back(row4(a1.z, b1.z, a1.w, b1.w));  // e2.x, e2.y
            L.leaf_geo.push_back(row4(a2.x, b2.x, as_float((int32_t)ia), as_float((int32_t)(nn.n - k)))); // e2.z, index, remaining
        }
    }
}

// old child ref -> k_mega3 child ref
inline int32_t ref3(const std::vector<int32_t>& rec_of_it, int32_t r) { return r >= 0 ? r : ~rec_of_it[(uint32_t)~r >> 4]; }

// ---- step 3: both binary trees with their child boxes as (left, right) pairs (crt_device.h: nodes3) ----
inline void build_nodes3(SceneLayout& L, const std::vector<int32_t>& rec_of_it)
{
    const std::vector<Row4>& nodes = L.nodes;
    L.nodes3.resize(nodes.size());
    for (size_t q = 0; q * 4 < nodes.size(); q++) {
        const Row4 a = nodes[q * 4], b = nodes[q * 4 + 1], c = nodes[q * 4 + 2], e = nodes[q * 4 + 3];
        L.nodes3[q * 4 + 0] = row4(a.x, c.x, a.y, c.y);
        L.nodes3[q * 4 + 1] = row4(a.z, c.z, b.x, e.x);
        L.nodes3[q * 4 + 2] = row4(b.y, e.y, b.z, e.z);
        L.nodes3[q * 4 + 3] = row4(as_float(ref3(rec_of_it, as_int(a.w))), as_float(ref3(rec_of_it, as_int(b.w))), 0.0f, 0.0f);
    }
    L.scalars.root3_fast = ref3(rec_of_it, L.scalars.root_fast); L.scalars.root3_exact = ref3(rec_of_it, L.scalars.root_exact);
}

struct Topo4 { bool used[4]; int32_t ref[4]; float lo[4][3], hi[4][3]; }; // the 4-wide tree as collapse4 builds it, by node: what the implicit-refs copy is made from

// ---- step 4: the 4-wide tree for the rays with finite operands: the SAH tree collapsed (crt_device.h: nodes4) ----
// Leaves nodes4 empty, and root4 the leaf's ref, when the scene is one leaf.
inline void collapse4(SceneLayout& L, std::vector<Topo4>& topo)
{
    const std::vector<Row4>& nodes3 = L.nodes3;
    std::vector<Row4>& nodes4 = L.nodes4;
    float coord_max = 0.0f; // largest |coordinate| of a box of the 4-wide tree (+inf if any is not finite): start_ray's overflow test
    int32_t root4 = L.scalars.root3_fast;
    int depth4 = 1;
    if (root4 >= 0) {
        struct Child { float lo[3], hi[3]; int32_t ref; }; // ref: nodes3 index (>= 0) or leaf ref (< 0)
        auto children_of = [&](int32_t q, Child out[2]) {
            const Row4 n0 = nodes3[q * 4ull], n1 = nodes3[q * 4ull + 1], n2 = nodes3[q * 4ull + 2], n3 = nodes3[q * 4ull + 3];
            out[0] = Child{{n0.x, n0.z, n1.x}, {n1.z, n2.x, n2.z}, 0};
            out[1] = Child{{n0.y, n0.w, n1.y}, {n1.w, n2.y, n2.w}, 0};
            std::memcpy(&out[0].ref, &n3.x, 4); std::memcpy(&out[1].ref, &n3.y, 4);
        };
        auto area = [](const Child& c) {
            const double dx = (double)c.hi[0] - c.lo[0], dy = (double)c.hi[1] - c.lo[1], dz = (double)c.hi[2] - c.lo[2];
            return dx * dy + dy * dz + dz * dx;
        };
        // ---- which binary nodes become 4-wide nodes: the collapse that minimises the summed area of the 4-wide nodes -- the SAH
        //      cost of the inner steps, every step costing the same whatever the number of children used (Ylitie et al. 2017,
        //      the leaves being fixed here): cost(q) = A(q) + min_k D(left, k) + D(right, 4 - k), D(c, j) = cheapest cover of
        //      subtree c by at most j children of the node above = min(D(c, j - 1), min_k D(c.left, k) + D(c.right, j - k)),
        //      D(c, 1) = cost(c), D(leaf, .) = 0.  Against the round-1 rule (CRT_COLLAPSE=greedy: open the child with the largest
        //      area until there are four): cornell-box 9 967 instead of 11 993 nodes, 4.62 instead of 5.02 inner steps per ray,
        //      C2 -3.7 %; veach-mis 842 / 974 nodes, 5.05 / 5.13 steps, same time.
        const char* collapse_env = std::getenv("CRT_COLLAPSE");
        const bool collapse_dp = !(collapse_env && std::strcmp(collapse_env, "greedy") == 0);
        struct DpNode { double D[3]; uint8_t kw, c2, c3; }; // D[j-1]; kw: left share of the node's own four; c2 / c3: choice for j = 2 / 3
        std::vector<DpNode> dpn;
        if (collapse_dp) {
            dpn.assign(nodes3.size() / 4, DpNode{{0, 0, 0}, 1, 0, 0});
            struct Fr { int32_t q; double area; int state; };
            std::vector<Fr> st;
            st.push_back(Fr{root4, 0.0, 0});
            auto Dof = [&](const Child& c, int j) { return c.ref < 0 ? 0.0 : dpn[(size_t)c.ref].D[j - 1]; };
            while (!st.empty()) {
                Fr& f = st.back();
                Child two[2];
                children_of(f.q, two);
                if (f.state == 0) {
                    f.state = 1;
                    for (int i = 0; i < 2; i++)
                        if (two[i].ref >= 0) st.push_back(Fr{two[i].ref, area(two[i]), 0}); // (invalidates f: not used below)
                    continue;
                }
                DpNode& n = dpn[(size_t)f.q];
                // the node as a 4-wide node: its own step + the cheapest forest of four under it
                double best = 0.0; int bk = 1;
                for (int k = 1; k <= 3; k++) {
                    const double v = Dof(two[0], k) + Dof(two[1], 4 - k);
                    if (k == 1 || v < best) { best = v; bk = k; }
                }
                n.kw = (uint8_t)bk;
                n.D[0] = f.area + best;
                const double open2 = Dof(two[0], 1) + Dof(two[1], 1);
                n.c2 = open2 < n.D[0] ? 1 : 0;
                n.D[1] = n.c2 ? open2 : n.D[0];
                const double o12 = Dof(two[0], 1) + Dof(two[1], 2), o21 = Dof(two[0], 2) + Dof(two[1], 1);
                n.c3 = 0; n.D[2] = n.D[1];
                if (o12 < n.D[2]) { n.D[2] = o12; n.c3 = 1; }
                if (o21 < n.D[2]) { n.D[2] = o21; n.c3 = 2; }
                st.pop_back();
            }
        }
        // the (at most j) roots that cover the subtree of child c in the cheapest way
        std::vector<Child> cover;
        struct Ex { Child c; int j; };
        auto expand = [&](const Child& c0, int j0) {
            std::vector<Ex> ex;
            ex.push_back(Ex{c0, j0});
            while (!ex.empty()) {
                Ex e = ex.back(); ex.pop_back();
                if (e.c.ref < 0 || e.j == 1) { cover.push_back(e.c); continue; }
                const DpNode& n = dpn[(size_t)e.c.ref];
                const int choice = e.j == 2 ? (n.c2 ? 1 : 0) : n.c3;
                if (choice == 0) { ex.push_back(Ex{e.c, e.j - 1}); continue; }
                Child two[2];
                children_of(e.c.ref, two);
                ex.push_back(Ex{two[1], e.j - choice});
                ex.push_back(Ex{two[0], choice});
            }
        };
        struct Todo { int32_t node2; int32_t slot; int depth; }; // slot: index of the BVH4 node to fill
        std::vector<Todo> todo;
        nodes4.resize(8);
        todo.push_back(Todo{root4, 0, 1});
        root4 = 0;
        for (size_t t = 0; t < todo.size(); t++) {
            const Todo cur = todo[t];
            depth4 = std::max(depth4, cur.depth + 1);
            std::vector<Child> ch(2);
            children_of(cur.node2, ch.data());
            if (collapse_dp) {
                const Child l = ch[0], r = ch[1];
                const int k = dpn[(size_t)cur.node2].kw;
                cover.clear();
                expand(l, k);
                expand(r, 4 - k);
                ch = cover;
            }
            while (!collapse_dp && ch.size() < 4) { // open the largest inner child
                int best = -1;
                double ba = -1.0;
                for (size_t i = 0; i < ch.size(); i++)
                    if (ch[i].ref >= 0 && area(ch[i]) > ba) { ba = area(ch[i]); best = (int)i; }
                if (best < 0) break;
                Child two[2];
                children_of(ch[best].ref, two);
                ch[best] = two[0];
                ch.push_back(two[1]);
            }
            int32_t refs[4];
            float lo[4][3], hi[4][3];
            if (topo.size() <= (size_t)cur.slot) topo.resize((size_t)cur.slot + 1);
            for (int i = 0; i < 4; i++) {
                if (i < (int)ch.size()) {
                    for (int a = 0; a < 3; a++) { lo[i][a] = ch[i].lo[a]; hi[i][a] = ch[i].hi[a]; }
                    if (ch[i].ref >= 0) {
                        refs[i] = (int32_t)(nodes4.size() / 8);
                        nodes4.resize(nodes4.size() + 8);
                        todo.push_back(Todo{ch[i].ref, refs[i], cur.depth + 1});
                    } else refs[i] = ch[i].ref;
                } else {
                    // empty slot: the inverted box (t_enter = +inf, t_exit = -inf whatever the signs of the direction)
                    for (int a = 0; a < 3; a++) { lo[i][a] = std::numeric_limits<float>::infinity(); hi[i][a] = -std::numeric_limits<float>::infinity(); }
                    refs[i] = ~0x7ffffff0; // (never followed)
                }
                Topo4& tp = topo[(size_t)cur.slot];
                tp.used[i] = i < (int)ch.size();
                tp.ref[i] = refs[i];
                for (int a = 0; a < 3; a++) { tp.lo[i][a] = lo[i][a]; tp.hi[i][a] = hi[i][a]; }
            }
            for (int i = 0; i < (int)ch.size() && i < 4; i++)
                for (int a = 0; a < 3; a++) {
                    const float m = std::max(std::fabs(lo[i][a]), std::fabs(hi[i][a]));
                    coord_max = (m <= FLT_MAX && coord_max <= FLT_MAX) ? std::max(coord_max, m) : std::numeric_limits<float>::infinity();
                }
            Row4* o = &nodes4[(size_t)cur.slot * 8];
            for (int a = 0; a < 3; a++) { // plane-major: [2a] = lo of axis a of the four children, [2a + 1] = hi
                o[2 * a + 0] = row4(lo[0][a], lo[1][a], lo[2][a], lo[3][a]);
                o[2 * a + 1] = row4(hi[0][a], hi[1][a], hi[2][a], hi[3][a]);
            }
            o[6] = row4(as_float(refs[0]), as_float(refs[1]), as_float(refs[2]), as_float(refs[3]));
            // the refs as the decoupled-leaves step wants them: a leaf as 0x80000000 | record << 8, ready to take the ray id
            // (records beyond 2^23 - 1 do not fit: CAP_DEC)
            auto dref = [](int32_t r) -> int32_t { return r >= 0 ? r : (int32_t)(0x80000000u | (((uint32_t)~r & 0x7fffffu) << 8)); };
            o[7] = row4(as_float(dref(refs[0])), as_float(dref(refs[1])), as_float(dref(refs[2])), as_float(dref(refs[3])));
        }
    }
    L.scalars.root4 = root4;
    L.scalars.coord_max = coord_max;
    L.accel.depth4 = (uint32_t)depth4;
}

// ---- step 5: the empty node behind the tree (DevScene::empty4_off): four inverted boxes, refs that are never followed ----
inline void append_empty_node4(SceneLayout& L)
{
    std::vector<Row4>& nodes4 = L.nodes4;
    if (nodes4.empty()) nodes4.resize(8);
    L.accel.n_nodes4 = (uint32_t)(nodes4.size() / 8);
    const float pinf_ = std::numeric_limits<float>::infinity();
    for (int a = 0; a < 3; a++) { nodes4.push_back(row4(pinf_, pinf_, pinf_, pinf_)); nodes4.push_back(row4(-pinf_, -pinf_, -pinf_, -pinf_)); }
    const float er = as_float(~0x7ffffff0);
    nodes4.push_back(row4(er, er, er, er)); nodes4.push_back(row4(er, er, er, er));
    L.scalars.empty4_off = (uint32_t)((size_t)L.accel.n_nodes4 * 128);
}

// ---- step 6: the same tree WITHOUT its rows of refs (round 6): nodes4i, 6 x float4 (96 B) per node ----
// What bounds k_mega3 is the number of divergent vector-memory instructions (one more 4-byte load per inner visit costs
// the stand-in 2.1 % and veach-mis 6.7 %; 9 % fewer vector ALU instructions cost nothing), and a visit loads seven float4 -- six rows
// of planes and the refs.  Here the refs are IMPLIED:
//   * nodes are numbered breadth first in two ranges: [0, n_mixed) the nodes with an inner child, [n_mixed, n) the nodes whose
//     children are all leaves ("fringe"); a node's children are ordered mixed, fringe, leaves, empty, so that its mixed children
//     are fm, fm + 1, .. and its fringe children ff, ff + 1, ..;
//   * leaf child k of node n is record 4 n + k of a SPARSE copy of the leaf records (leaf_geo_i; leaves of one record only:
//     bvh_thresh_n <= 2, else the layout is not offered);
//   * (fm, ff, number of mixed, number of fringe children) -- 36 bits -- live in the low 12 mantissa bits of the six planes of
//     child 0 of a mixed node, which is an INNER child: the same 12 bits in the lo and in the hi plane of an axis (a ray reads them
//     from the near plane whatever its direction), the planes moved OUTWARDS to the next value with those bits (a box grows by at
//     most 2^-11 of its coordinates).  An inner box may be any superset (crt_trace.h); a leaf's box stays the reference's own, bit
//     for bit -- which is why the bits can only live in an inner child, and why the fringe nodes are told apart by their number.
// Offered when it applies (CAP_IMPL); the decoupled-leaves kernels with 16-bit stack entries take it (CRT_IMPL=0: not).
inline void build_nodes4i(const crt_scene_desc& d, SceneLayout& L, const std::vector<Topo4>& topo)
{
    const size_t n4 = L.accel.n_nodes4;
    const std::vector<Row4>& leaf_geo = L.leaf_geo;
    if (!(L.scalars.root4 >= 0 && n4 <= 32768 && L.max_leaf <= 2 && topo.size() == n4)) return;
    std::vector<uint8_t> mixed(n4, 0);
    for (size_t i = 0; i < n4; i++)
        for (int k = 0; k < 4; k++) if (topo[i].used[k] && topo[i].ref[k] >= 0) mixed[i] = 1;
    // The children of a class are ordered by "occupancy", descending: the summed area of the triangles below a child over its box's half
    // area (round 6).  The traversal takes the NEAREST hit inner child first whatever the slots; the slots decide
    // the order of the others (the loser of (0,1) is popped before the loser of the final, visit_front), the order of a visit's queue
    // entries, and the breadth-first numbers.  Against the order the collapse happens to leave: C2 75.86 -> 75.35 ms, veach-mis spp 256
    // 71.17 -> 70.43, inner visits per ray 4.496 -> 4.490 / 6.740 -> 6.685 (by box area instead: 75.61 / 70.41).  Visiting the any-hit
    // rays' children in this static order INSTEAD of nearest first was measured in both directions and loses (docs/experiments.md 6.10).
    // CRT_CHILD_ORDER=none|area: A/B hooks.
    std::vector<double> prio4(n4 * 4, 0.0);
    const char* co_ = std::getenv("CRT_CHILD_ORDER");
    if (!(co_ && co_[0] == 'n')) {
        const bool by_area = co_ && co_[0] == 'a';
        std::vector<double> tri_area_below(n4, -1.0);
        auto leaf_area = [&](int32_t ref) {
            const size_t dense = (size_t)(~ref);
            const int it = as_int(leaf_geo[dense * 5 + 4].z), cnt = as_int(leaf_geo[dense * 5 + 4].w);
            double a = 0.0;
            for (int q = 0; q < cnt; q++) {
                const crt_triangle& tr = d.tris[(size_t)it + (size_t)q];
                const double e1[3] = {(double)tr.v2[0] - tr.v1[0], (double)tr.v2[1] - tr.v1[1], (double)tr.v2[2] - tr.v1[2]};
                const double e2[3] = {(double)tr.v3[0] - tr.v1[0], (double)tr.v3[1] - tr.v1[1], (double)tr.v3[2] - tr.v1[2]};
                const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
                a += 0.5 * std::sqrt(cx * cx + cy * cy + cz * cz);
            }
            return a;
        };
        std::vector<std::pair<int32_t, int>> st_(1, std::make_pair(0, 0)); // post-order over the 4-wide tree
        while (!st_.empty()) {
            const int32_t i = st_.back().first;
            int32_t next_ = -1;
            for (int k = 0; k < 4 && next_ < 0; k++)
                if (topo[(size_t)i].used[k] && topo[(size_t)i].ref[k] >= 0 && tri_area_below[(size_t)topo[(size_t)i].ref[k]] < 0.0) next_ = topo[(size_t)i].ref[k];
            if (next_ >= 0) { st_.push_back(std::make_pair(next_, 0)); continue; }
            double sum = 0.0;
            for (int c = 0; c < 4; c++) {
                const Topo4& t = topo[(size_t)i];
                if (!t.used[c]) continue;
                const double below = t.ref[c] < 0 ? leaf_area(t.ref[c]) : tri_area_below[(size_t)t.ref[c]];
                sum += below;
                const double ex = (double)t.hi[c][0] - t.lo[c][0], ey = (double)t.hi[c][1] - t.lo[c][1], ez = (double)t.hi[c][2] - t.lo[c][2];
                const double ha = ex * ey + ey * ez + ez * ex;
                prio4[(size_t)i * 4 + (size_t)c] = by_area ? ha : (ha > 0.0 ? below / ha : 1e30);
            }
            tri_area_below[(size_t)i] = sum;
            st_.pop_back();
        }
    }
    // children order: mixed, fringe, leaves, empty; then breadth-first numbers in the two ranges
    std::vector<std::array<int, 4>> order(n4);
    for (size_t i = 0; i < n4; i++) {
        int o = 0;
        for (int pass = 0; pass < 4; pass++) {
            const int o0 = o;
            for (int k = 0; k < 4; k++) {
                const Topo4& t = topo[i];
                const int cls = !t.used[k] ? 3 : (t.ref[k] < 0 ? 2 : (mixed[(size_t)t.ref[k]] ? 0 : 1));
                if (cls == pass) order[i][o++] = k;
            }
            std::stable_sort(order[i].begin() + o0, order[i].begin() + o, [&](int a, int b) { return prio4[i * 4 + (size_t)a] > prio4[i * 4 + (size_t)b]; });
        }
    }
    uint32_t n_mixed = 0;
    for (size_t i = 0; i < n4; i++) n_mixed += mixed[i];
    std::vector<int32_t> newid(n4, -1);
    {
        uint32_t cm_ = 0, cf_ = n_mixed;
        std::vector<int32_t> bfs;
        bfs.push_back(0);
        newid[0] = mixed[0] ? (int32_t)cm_++ : (int32_t)cf_++;
        for (size_t t = 0; t < bfs.size(); t++) {
            const int32_t i = bfs[t];
            for (int o = 0; o < 4; o++) {
                const int k = order[(size_t)i][o];
                if (!topo[(size_t)i].used[k] || topo[(size_t)i].ref[k] < 0) continue;
                const int32_t c = topo[(size_t)i].ref[k];
                newid[(size_t)c] = mixed[(size_t)c] ? (int32_t)cm_++ : (int32_t)cf_++;
                bfs.push_back(c);
            }
        }
    }
    bool ok = true;
    // the nearest value <= f (down) / >= f (up) whose low 12 bits are `chunk` (crt_accel.h)
    auto with_bits = [&](float f, uint32_t chunk, bool up) -> float { return crtaccel::with_bits(f, chunk, up, ok); };
    std::vector<Row4> n4i((n4 + 1) * (size_t)kNode4iF4, row4(0.0f, 0.0f, 0.0f, 0.0f));
    const size_t n_rec_i = (n4 + 1) * 4;
    std::vector<Row4> lgi(n_rec_i * 5, row4(0.0f, 0.0f, 0.0f, 0.0f));
    std::vector<int32_t> rec_map(leaf_geo.size() / 5, 0);
    float cmax_i = L.scalars.coord_max;
    for (size_t i = 0; i < n4 && ok; i++) {
        const Topo4& t = topo[i];
        const size_t ni = (size_t)newid[i];
        float lo[4][3], hi[4][3];
        uint32_t n_m = 0, n_f = 0, fm = 0, ff = 0;
        for (int o = 0; o < 4; o++) {
            const int k = order[i][o];
            for (int a = 0; a < 3; a++) { lo[o][a] = t.lo[k][a]; hi[o][a] = t.hi[k][a]; }
            if (t.used[k] && t.ref[k] >= 0) {
                const uint32_t id = (uint32_t)newid[(size_t)t.ref[k]];
                if (mixed[(size_t)t.ref[k]]) { if (n_m++ == 0) fm = id; } else { if (n_f++ == 0) ff = id; }
            } else if (t.used[k]) { // a leaf of one record: its copy at 4 n + o
                const size_t dense = (size_t)(~t.ref[k]);
                const size_t sparse = ni * 4 + (size_t)o;
                for (int q = 0; q < 5; q++) lgi[sparse * 5 + (size_t)q] = leaf_geo[dense * 5 + (size_t)q];
                rec_map[dense] = (int32_t)sparse;
            }
        }
        if (mixed[i]) {
            const uint32_t chunk[3] = {fm & 0xfffu, ((fm >> 12) & 7u) | ((ff & 0x1ffu) << 3), ((ff >> 9) & 63u) | (n_m << 6) | (n_f << 9)};
            for (int a = 0; a < 3; a++) {
                lo[0][a] = with_bits(lo[0][a], chunk[a], false);
                hi[0][a] = with_bits(hi[0][a], chunk[a], true);
                const float m = std::max(std::fabs(lo[0][a]), std::fabs(hi[0][a]));
                cmax_i = std::max(cmax_i, m);
            }
        }
        Row4* o6 = &n4i[ni * (size_t)kNode4iF4];
        for (int a = 0; a < 3; a++) {
            o6[2 * a + 0] = row4(lo[0][a], lo[1][a], lo[2][a], lo[3][a]);
            o6[2 * a + 1] = row4(hi[0][a], hi[1][a], hi[2][a], hi[3][a]);
        }
    }
    if (!(ok && cmax_i <= FLT_MAX)) return;
    const float pinf_ = std::numeric_limits<float>::infinity();
    for (int a = 0; a < 3; a++) { n4i[n4 * (size_t)kNode4iF4 + 2 * (size_t)a] = row4(pinf_, pinf_, pinf_, pinf_); n4i[n4 * (size_t)kNode4iF4 + 2 * (size_t)a + 1] = row4(-pinf_, -pinf_, -pinf_, -pinf_); }
    L.nodes4i.swap(n4i); L.leaf_geo_i.swap(lgi); L.rec_map.swap(rec_map);
    L.scalars.n_mixed4i = n_mixed;
    L.scalars.root4i = newid[0];
    L.scalars.empty4i_off = (uint32_t)(n4 * kNode4iF4 * 16);
    L.scalars.coord_max = cmax_i; // (start_ray's overflow test covers both copies of the tree)
    L.accel.layout_caps |= CAP_IMPL;
}

// Every array and scalar of a validated description.  device_sah: crtaccel::build_sah_device, or null for the host builder
// (CRT_SAH_HOST=1 forces the host builder either way).
inline void build_scene_layout(const crt_scene_desc& d, DeviceSah device_sah, SceneLayout& L)
{
    L = SceneLayout();
    L.accel.depth2 = (uint32_t)convert_bvh(d, L.nodes, L.leaf_count, L.scalars.root_fast, L.scalars.root_exact, device_sah, &L.accel);
    build_rows(d, L);
    std::vector<int32_t> rec_of_it;
    build_leaf_records(d, L, rec_of_it);
    build_nodes3(L, rec_of_it);
    std::vector<Topo4> topo;
    collapse4(L, topo);
    append_empty_node4(L);
    build_nodes4i(d, L, topo);
    const size_t n_nodes4 = L.accel.n_nodes4, n_records = L.leaf_geo.size() / 5;
    if (n_nodes4 <= 32768 && n_records <= 32768) L.accel.layout_caps |= CAP_REF16; // node refs 0 .. 32767, leaf refs ~0 .. ~32767
    if (n_nodes4 <= 32768) L.accel.layout_caps |= CAP_REF16_INNER;
    if (n_records <= (size_t)kLeafRecMax + 1) L.accel.layout_caps |= CAP_DEC;
    // Both traversal modes hold at most one pending sibling per tree level.
    L.scalars.stack_cap = (uint32_t)std::max((int)L.accel.depth2 + 2, 3 * (int)L.accel.depth4 + 2); // BVH2: one pending sibling per level; BVH4: up to three
    L.scalars.node4i_f4 = kNode4iF4;
}

} // namespace crtlayout
#endif
