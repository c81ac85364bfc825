// tools/sah_host_check.cpp -- CPU checks of two details of the host SAH builder (csrc/crt_accel.h) that the device builder
// (csrc/crt_accel_build.hip) must match for the two to give the same tree, node for node:
//   * box unions order -0.0 below +0.0 (the device's integer keys do): a box over both zeros has lo = -0.0 and hi = +0.0, whatever
//     order the leaves come in -- checked on Box::grow and on every box build_sah stores, with the leaves in two orders;
//   * a range whose centroid extent is denormal (scale NB / extent = +inf) is binned by the saturating sah_bin: the leaves split by
//     their centroids, not by index.
// Prints one JSON line; exit status 1 on a violation.  Build: g++ -O2 -std=c++17 -pthread -I cudaraytracing_amd/csrc (tests/test_sah_host.py)
#include "crt_accel.h"

#include <cstdio>
#include <limits>
#include <string>

using namespace crtaccel;

static std::string first;
static int bad = 0;
static void expect(bool ok, const char* what)
{
    if (!ok && bad++ == 0) first = what;
}

// the leaves below a child ref of the built tree
static void leaves_of(const std::vector<Node>& nodes, int32_t ref, std::vector<int>& out)
{
    if (ref < 0) { out.push_back(~ref); return; }
    for (int s = 0; s < 2; s++) leaves_of(nodes, nodes[(size_t)ref].child[s], out);
}

static int signed_zero_tree(bool reversed)
{
    // 64 unit boxes along y, flat in x at +-0.0 (lo and hi signs drawn independently), spread in z
    std::vector<Prim> prims;
    uint32_t r = 12345;
    for (int i = 0; i < 64; i++) {
        r = r * 1664525u + 1013904223u;
        Prim p;
        p.box.lo[0] = (r >> 8) & 1 ? -0.0f : 0.0f;
        p.box.hi[0] = (r >> 9) & 1 ? -0.0f : 0.0f;
        p.box.lo[1] = (float)i; p.box.hi[1] = (float)i + 1.0f;
        p.box.lo[2] = (float)(i % 7); p.box.hi[2] = (float)(i % 7) + 0.5f;
        p.ref = ~i;
        prims.push_back(p);
    }
    std::vector<Prim> in(prims);
    if (reversed) std::reverse(in.begin(), in.end());
    std::vector<Node> nodes;
    int32_t root = 0;
    build_sah(in, nodes, root, nullptr);
    int boxes = 0;
    for (const Node& n : nodes)
        for (int s = 0; s < 2; s++) {
            std::vector<int> lv;
            leaves_of(nodes, n.child[s], lv);
            bool any_neg_lo = false, any_pos_hi = false;
            for (int i : lv) { any_neg_lo |= std::signbit(prims[(size_t)i].box.lo[0]); any_pos_hi |= !std::signbit(prims[(size_t)i].box.hi[0]); }
            expect(n.box[s].lo[0] == 0.0f && std::signbit(n.box[s].lo[0]) == any_neg_lo, "build_sah: lo.x over +-0 is -0.0 iff a leaf's is");
            expect(n.box[s].hi[0] == 0.0f && std::signbit(n.box[s].hi[0]) == !any_pos_hi, "build_sah: hi.x over +-0 is +0.0 iff a leaf's is");
            boxes++;
        }
    return boxes;
}

int main()
{
    // Box::grow on the two zeros, in both orders
    for (int order = 0; order < 2; order++) {
        Box p, n, u;
        for (int a = 0; a < 3; a++) { p.lo[a] = p.hi[a] = 0.0f; n.lo[a] = n.hi[a] = -0.0f; }
        u.reset();
        if (order == 0) { u.grow(p); u.grow(n); } else { u.grow(n); u.grow(p); }
        for (int a = 0; a < 3; a++) {
            expect(u.lo[a] == 0.0f && std::signbit(u.lo[a]), "Box::grow: lo over +-0 is -0.0");
            expect(u.hi[a] == 0.0f && !std::signbit(u.hi[a]), "Box::grow: hi over +-0 is +0.0");
        }
    }
    const int boxes = signed_zero_tree(false) + signed_zero_tree(true);

    // eight leaves that differ only in x, at the smallest denormals: one centroid extent is 7 x 2^-149, NB / extent = +inf
    std::vector<Prim> prims;
    for (int i = 0; i < 8; i++) {
        uint32_t u = (uint32_t)i;
        float x;
        std::memcpy(&x, &u, 4);
        Prim p;
        p.box.lo[0] = p.box.hi[0] = x;
        p.box.lo[1] = p.box.lo[2] = 0.0f; p.box.hi[1] = p.box.hi[2] = 1.0f;
        p.ref = ~i;
        prims.push_back(p);
    }
    std::vector<Node> nodes;
    int32_t root = 0;
    uint32_t index_splits = 0;
    build_sah(prims, nodes, root, &index_splits);
    expect(index_splits == 0, "build_sah: a denormal centroid extent is split by index");
    expect(sah_bin(std::numeric_limits<float>::infinity(), 32) == 31 && sah_bin(std::numeric_limits<float>::quiet_NaN(), 32) == 0 &&
           sah_bin(-1.0f, 32) == 0 && sah_bin(30.99f, 32) == 30 && sah_bin(31.0f, 32) == 31 && sah_bin(1e30f, 32) == 31, "sah_bin: saturation");
    std::printf("{\"signed_zero_boxes\": %d, \"denormal_index_splits\": %u, \"denormal_nodes\": %zu, \"violations\": %d, \"first_violation\": \"%s\"}\n",
                boxes, index_splits, nodes.size(), bad, first.c_str());
    return bad ? 1 : 0;
}
