// tools/refit_host_check.cpp -- crt_scene_refit without a GPU: the kernel text of csrc/crt_refit.h compiled for the host behind
// host_device.h's stand-ins (a wave of 64 host threads, so the ballot of the check and the arrivals of the walk are real), run on the
// layout csrc/crt_scene_layout.h builds.  Reads a scene description as tools/scene_layout_dump.cpp does (<dir>/desc_*.bin), builds the
// layout with the host SAH builder, makes the tables as the library does at a handle's first refit, then refits once per pair of
// moved triangle files, in order, and writes into <out> the arrays in scene_layout_dump's format (the ten arrays of crt_scene_export,
// scalars.bin, accel.bin) plus ltri.bin and root.bin (the root box: lo.xyz, hi.xyz).  A refused refit (a coordinate that is not finite
// or beyond 2^126) ends the run with status 3 after the arrays, untouched by it, are written.  tests/test_refit.py.
// Build: g++ -std=c++17 -ffp-contract=off -fno-fast-math -pthread -I cudaraytracing_amd/csrc tools/refit_host_check.cpp
// Usage: refit_host_check <dir> <root> <levels|walk|a comma list of them, one per refit, taken round and round> <out> [<tris.bin> <light_tris.bin>]...
#define CRT_HOST_WAVES
#include "host_device.h"

#include "crt_scene_layout.h"

#include <cstdio>
#include <string>

#include "crt_refit.h"

using namespace crtk;

static void k_refit_check(const RefitParams P) { refit_check(P); }
static void k_refit_rows(const RefitParams P) { refit_rows(P); }
static void k_refit_leaves(const RefitParams P) { refit_leaf_box(P); }
static void k_refit_level(const RefitParams P) { refit_level(P); }
static void k_refit_walk(const RefitParams P) { refit_walk(P); }
static void k_refit_finish(const RefitParams P) { refit_finish(P); }

template <typename T> static std::vector<T> read_all(const std::string& path)
{
    std::vector<T> v;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return v;
    std::fseek(f, 0, SEEK_END);
    v.resize((size_t)std::ftell(f) / sizeof(T));
    std::fseek(f, 0, SEEK_SET);
    if (std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) v.clear();
    std::fclose(f);
    return v;
}

static bool write_all(const std::string& path, const void* p, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes;
    return std::fclose(f) == 0 && ok;
}

// a layout array in the kernels' element type (a byte copy; one spare element, as the library's empty uploads have)
static std::vector<float4> rows_of(const std::vector<crtlayout::Row4>& v)
{
    std::vector<float4> o(v.size() + 1);
    if (!v.empty()) std::memcpy(o.data(), v.data(), v.size() * sizeof(float4));
    return o;
}

int main(int argc, char** argv)
{
    if (argc < 5 || (argc - 5) % 2 != 0) { std::fprintf(stderr, "usage: %s <dir> <root> <levels|walk> <out> [<tris.bin> <light_tris.bin>]...\n", argv[0]); return 2; }
    const std::string dir = std::string(argv[1]) + "/", out = std::string(argv[4]) + "/";
    std::vector<std::string> forms; // one per refit, the list taken round and round
    for (std::string rest = argv[3]; !rest.empty();) {
        const size_t c = rest.find(',');
        forms.push_back(rest.substr(0, c));
        rest = c == std::string::npos ? std::string() : rest.substr(c + 1);
    }
    if (forms.empty()) forms.push_back("");
    for (const std::string& f : forms)
        if (f != "levels" && f != "walk") { std::fprintf(stderr, "form must be levels or walk, or a list of them\n"); return 2; }
    const std::vector<crt_bvh_node> dnodes = read_all<crt_bvh_node>(dir + "desc_nodes.bin");
    const std::vector<crt_triangle> tris = read_all<crt_triangle>(dir + "desc_tris.bin"), ltris = read_all<crt_triangle>(dir + "desc_light_tris.bin");
    const std::vector<crt_material> mats = read_all<crt_material>(dir + "desc_materials.bin");
    const std::vector<crt_light> lights = read_all<crt_light>(dir + "desc_lights.bin");
    crt_scene_desc d{};
    d.nodes = dnodes.data(); d.n_nodes = (uint32_t)dnodes.size(); d.root = std::atoi(argv[2]);
    d.tris = tris.data(); d.n_tris = (uint32_t)tris.size();
    d.light_tris = ltris.data(); d.n_light_tris = (uint32_t)ltris.size();
    d.materials = mats.data(); d.n_materials = (uint32_t)mats.size();
    d.lights = lights.data(); d.n_lights = (uint32_t)lights.size();
    const char* msg = nullptr;
    if (crtlayout::validate_desc(&d, msg) != CRT_OK) { std::fprintf(stderr, "%s\n", msg); return 1; }
    crtlayout::SceneLayout L;
    crtlayout::build_scene_layout(d, nullptr, L);
    const bool leaf_root = L.scalars.root_fast < 0, impl = (L.accel.layout_caps & crtlayout::CAP_IMPL) != 0;
    if (leaf_root) { L.nodes.clear(); L.nodes3.clear(); }

    // ---- what the library does at a handle's first refit ----
    crtrefit::Arrays A{};
    A.nodes = (const float*)L.nodes.data(); A.nodes4 = (const float*)L.nodes4.data(); A.nodes4i = impl ? (const float*)L.nodes4i.data() : nullptr;
    A.leaf_geo = (const float*)L.leaf_geo.data();
    A.n_nodes2 = L.nodes.size() / 4; A.n_nodes4 = L.accel.n_nodes4; A.n_rec = L.leaf_geo.size() / 5;
    A.rec_map = L.rec_map.data(); A.leaf_count = L.leaf_count.data();
    A.root_fast = L.scalars.root_fast; A.root_exact = L.scalars.root_exact; A.root4 = L.scalars.root4; A.root4i = L.scalars.root4i;
    A.n_mixed4i = L.scalars.n_mixed4i; A.n_tris = d.n_tris;
    crtrefit::Tables T;
    if (!crtrefit::build_tables(A, T)) { std::fprintf(stderr, "the tables could not be made\n"); return 1; }
    std::vector<float4> nodes = rows_of(L.nodes), nodes3 = rows_of(L.nodes3), nodes4 = rows_of(L.nodes4), nodes4i = rows_of(L.nodes4i), tri_geo = rows_of(L.tri_geo);
    std::vector<float4> tri_nm = rows_of(L.tri_nm), leaf_geo = rows_of(L.leaf_geo), leaf_geo_i = rows_of(L.leaf_geo_i), ltri = rows_of(L.ltri);
    std::vector<float4> tasks((size_t)T.n_tasks * 2 + 1), box(((size_t)T.n_leaves + T.n_tasks) * 2 + 1);
    if (T.n_tasks) std::memcpy(tasks.data(), T.tasks.data(), T.tasks.size() * 4);
    std::vector<float> cm(T.n_tasks + 1, 0.0f);
    std::vector<unsigned int> cnt(T.n_tasks + 1, 0u);
    RefitResult res{};
    float root[6];
    std::memcpy(root, dnodes[(size_t)d.root].aa, 12); std::memcpy(root + 3, dnodes[(size_t)d.root].bb, 12);
    uint32_t gen = 0;
    bool refused = false;

    for (int k = 5; k + 1 < argc && !refused; k += 2) {
        const std::vector<crt_triangle> mt = read_all<crt_triangle>(argv[k]), ml = read_all<crt_triangle>(argv[k + 1]);
        if (mt.size() != tris.size() || ml.size() != ltris.size()) { std::fprintf(stderr, "%s: counts other than the description's\n", argv[k]); return 2; }
        const std::string& form = forms[(size_t)((k - 5) / 2) % forms.size()];
        RefitParams P{};
        P.tris = (const float*)mt.data(); P.ltris = (const float*)ml.data();
        P.n_tris = d.n_tris; P.n_ltris = d.n_light_tris; P.n_rec = (uint32_t)A.n_rec;
        P.tri_geo = tri_geo.data(); P.tri_nm = tri_nm.data(); P.leaf_geo = leaf_geo.data(); P.leaf_geo_i = impl ? leaf_geo_i.data() : nullptr; P.ltri = ltri.data();
        P.rec_map = impl ? L.rec_map.data() : nullptr;
        P.leaves = T.leaves.data(); P.n_leaves = T.n_leaves; P.n_tasks = T.n_tasks; P.tasks = tasks.data();
        P.nodes = nodes.data(); P.nodes3 = nodes3.data(); P.nodes4 = nodes4.data(); P.nodes4i = impl ? nodes4i.data() : nullptr;
        P.box = box.data(); P.cm = cm.data(); P.cnt = cnt.data(); P.gen = gen + 1; P.res = &res;
        auto launch = [&](void (*kern)(const RefitParams), uint64_t threads) {
            if (threads) hipLaunchKernelGGL(kern, dim3((uint32_t)((threads + 255u) / 256u)), dim3(256), 0, nullptr, P);
        };
        res = RefitResult{};
        launch(k_refit_check, (uint64_t)P.n_tris + P.n_ltris);
        launch(k_refit_rows, (uint64_t)P.n_tris + P.n_rec + P.n_ltris);
        launch(k_refit_leaves, P.n_leaves);
        if (form == "levels") {
            for (size_t h = 0; h + 1 < T.level.size(); h++) {
                P.first = T.level[h]; P.count = T.level[h + 1] - T.level[h];
                launch(k_refit_level, P.count);
            }
        } else if (T.level.size() > 1) {
            P.first = 0; P.count = T.level[1];
            launch(k_refit_walk, P.count);
        }
        if (P.n_tasks) hipLaunchKernelGGL(k_refit_finish, dim3(1), dim3(256), 0, nullptr, P);
        if (res.bad != 0u) { refused = true; break; }
        if (form == "walk" && T.level.size() > 1) gen++; // only a walk advances the counters, as in the library
        std::memcpy(&L.scalars.coord_max, &res.coord_max_bits, 4);
        std::memcpy(root, res.root_lo, 12); std::memcpy(root + 3, res.root_hi, 12);
    }

    bool ok = true;
    auto rows = [&](const char* name, const std::vector<float4>& v, size_t n) { ok = write_all(out + name + ".bin", v.data(), n * sizeof(float4)) && ok; };
    auto ints = [&](const char* name, const std::vector<int32_t>& v) { ok = write_all(out + name + ".bin", v.data(), v.size() * sizeof(v[0])) && ok; };
    rows("nodes", nodes, L.nodes.size()); rows("nodes3", nodes3, L.nodes3.size()); rows("nodes4", nodes4, L.nodes4.size()); rows("nodes4i", nodes4i, L.nodes4i.size());
    rows("leaf_geo", leaf_geo, L.leaf_geo.size()); rows("leaf_geo_i", leaf_geo_i, L.leaf_geo_i.size()); ints("rec_map", L.rec_map);
    rows("tri_geo", tri_geo, L.tri_geo.size()); ints("leaf_count", L.leaf_count); rows("tri_nm", tri_nm, L.tri_nm.size()); rows("ltri", ltri, L.ltri.size());
    ok = write_all(out + "scalars.bin", &L.scalars, sizeof(L.scalars)) && ok;
    ok = write_all(out + "accel.bin", &L.accel, sizeof(L.accel)) && ok;
    ok = write_all(out + "root.bin", root, sizeof(root)) && ok;
    if (!ok) return 1;
    return refused ? 3 : 0;
}
