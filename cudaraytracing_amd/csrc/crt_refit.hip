// cudaraytracing_amd/csrc/crt_refit.hip -- crt_scene_refit / crt_scene_refit_device (contract: include/crt.h): the kernels around the
// text of crt_refit.h, what a handle keeps for its refits (made at the first one: the tables, from the arrays the handle holds in device
// memory; the box array, the counters of the walk, the result and its pinned copy, two events) and the two entry points.
//   k_refit_check    one thread per triangle and light triangle: the count of coordinates that are refused.  Every later kernel reads
//                    that count first and writes nothing unless it is 0, so a refused call leaves the handle as it was and the host
//                    reads the count once, at the end.
//   k_refit_rows     one thread per triangle, per leaf record and per light triangle
//   k_refit_leaves   one thread per leaf
//   k_refit_level    form `levels`: one launch per node height, one thread per inner node of any tree
//   k_refit_walk     form `walk`: one launch, one thread per inner node whose children are all leaves
//   k_refit_finish   one block: coord_max
// CRT_REFIT_FORM=levels|walk (read per call; tests and tools/refit_probe.py) selects the form; unset: kDefaultForm
// (docs/experiments.md, "Refitting a scene").
#include "crt_scene.h"

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "crt_refit.h"

using namespace crtdev;
using namespace crtk;

static_assert(sizeof(crt_triangle) == kRefitTriWords * 4, "crt_refit.h reads a crt_triangle as 15 words");
static_assert(sizeof(RefitResult) == 32, "the result is one 32-byte copy");

struct RefitState {
    DevBuf<uint32_t> leaves;
    DevBuf<float4> tasks, box;
    DevBuf<float> cm;
    DevBuf<unsigned int> cnt;
    DevBuf<RefitResult> res;
    DevBuf<float> up_tris, up_ltris; // the host form's uploads
    RefitResult* h_res = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::vector<uint32_t> level;
    std::vector<int32_t> tri_mat;    // the host form's material check (read back at its first use)
    uint32_t n_leaves = 0, n_tasks = 0, boxes = 0, n_rec = 0;
    uint32_t gen = 0;          // the WALK calls that ran to their end since cnt was zeroed: each leaves counter t at gen * need(t); a levels call touches neither
    bool walk_open = false;    // a walk call was enqueued and did not come back (a HIP error): the counters are anybody's
    ~RefitState()
    {
        if (h_res) (void)hipHostFree(h_res);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};
void refit_release(RefitState* r) { delete r; }

namespace {

const int kDefaultForm = 0; // 0: levels, 1: walk

__global__ __launch_bounds__(256) void k_refit_check(const RefitParams P) { refit_check(P); }
__global__ __launch_bounds__(256) void k_refit_rows(const RefitParams P) { refit_rows(P); }
__global__ __launch_bounds__(256) void k_refit_leaves(const RefitParams P) { refit_leaf_box(P); }
__global__ __launch_bounds__(256) void k_refit_level(const RefitParams P) { refit_level(P); }
__global__ __launch_bounds__(256) void k_refit_walk(const RefitParams P) { refit_walk(P); }
__global__ __launch_bounds__(256) void k_refit_finish(const RefitParams P) { refit_finish(P); }

uint32_t blocks_of(uint64_t threads) { return (uint32_t)((threads + 255u) / 256u); }

// -1: a value that is neither
int form_of_environment()
{
    const char* e = std::getenv("CRT_REFIT_FORM");
    if (!e || !*e) return kDefaultForm;
    if (std::strcmp(e, "levels") == 0) return 0;
    if (std::strcmp(e, "walk") == 0) return 1;
    return -1;
}

template <class T> std::vector<T> read_back(const DevBuf<T>& b, size_t n)
{
    std::vector<T> v(n);
    if (n) HIP_CHECK(hipMemcpy(v.data(), b.p, n * sizeof(T), hipMemcpyDeviceToHost));
    return v;
}

// The handle's first refit: the tables from the arrays in device memory, and the buffers of every later call
int prepare(crt_scene* sc)
{
    std::unique_ptr<RefitState> st(new RefitState()); // (the handle's once it is complete)
    const bool leaf_root = sc->dev.root_fast < 0, impl = sc->can(crtlayout::CAP_IMPL);
    const size_t n_nodes2 = leaf_root ? 0 : sc->nodes.n / 4, n_rec = sc->leaf_geo.n / 5;
    const std::vector<float4> nodes = read_back(sc->nodes, n_nodes2 * 4), nodes4 = read_back(sc->nodes4, sc->nodes4.n);
    const std::vector<float4> nodes4i = read_back(sc->nodes4i, impl ? sc->nodes4i.n : 0), leaf_geo = read_back(sc->leaf_geo, n_rec * 5);
    const std::vector<int32_t> rec_map = read_back(sc->rec_map, impl ? n_rec : 0), leaf_count = read_back(sc->leaf_count, sc->leaf_count.n);
    crtrefit::Arrays A{};
    A.nodes = (const float*)nodes.data(); A.nodes4 = (const float*)nodes4.data(); A.nodes4i = impl ? (const float*)nodes4i.data() : nullptr;
    A.leaf_geo = (const float*)leaf_geo.data();
    A.n_nodes2 = n_nodes2; A.n_nodes4 = sc->accel.n_nodes4; A.n_rec = n_rec;
    A.rec_map = rec_map.data(); A.leaf_count = leaf_count.data();
    A.root_fast = sc->scalars.root_fast; A.root_exact = sc->scalars.root_exact; A.root4 = sc->scalars.root4; A.root4i = sc->scalars.root4i;
    A.n_mixed4i = sc->scalars.n_mixed4i; A.n_tris = sc->n_tris;
    crtrefit::Tables T;
    const bool sized = sc->leaf_count.n >= sc->n_tris && sc->nodes4.n >= (size_t)A.n_nodes4 * 8 && (!impl || sc->nodes4i.n >= (size_t)A.n_nodes4 * 6);
    if (!sized || !crtrefit::build_tables(A, T))
        return fail(CRT_ERR_UNSUPPORTED, "crt_scene_refit: the handle's trees are not what crt_scene_create lays out");
    st->n_leaves = T.n_leaves; st->n_tasks = T.n_tasks; st->boxes = T.boxes; st->n_rec = (uint32_t)n_rec; st->level = T.level;
    st->leaves.upload(T.leaves);
    st->tasks.alloc((size_t)T.n_tasks * 2);
    if (T.n_tasks) HIP_CHECK(hipMemcpy(st->tasks.p, T.tasks.data(), T.tasks.size() * 4, hipMemcpyHostToDevice));
    st->box.alloc(((size_t)T.n_leaves + T.n_tasks) * 2);
    st->cm.alloc(T.n_tasks);
    st->cnt.alloc(T.n_tasks);
    HIP_CHECK(hipMemset(st->cnt.p, 0, st->cnt.n * sizeof(unsigned int))); // once: a call leaves each counter at a multiple of its arrivals
    st->res.alloc(1);
    HIP_CHECK(hipHostMalloc((void**)&st->h_res, sizeof(RefitResult), hipHostMallocDefault));
    HIP_CHECK(hipEventCreate(&st->e0));
    HIP_CHECK(hipEventCreate(&st->e1));
    sc->refit = st.release();
    return CRT_OK;
}

int refit_check_args(const crt_scene* sc, const void* tris, uint32_t n_tris, const void* ltris, uint32_t n_ltris)
{
    const std::string w("crt_scene_refit");
    if (!sc) return fail(CRT_ERR_INVALID_ARG, w + ": null scene");
    if (!tris) return fail(CRT_ERR_INVALID_ARG, w + ": null triangle array");
    if (n_tris != sc->n_tris) return fail(CRT_ERR_INVALID_ARG, w + ": " + std::to_string(n_tris) + " triangles, the handle has " + std::to_string(sc->n_tris));
    if (n_ltris != sc->ltri_mat.size())
        return fail(CRT_ERR_INVALID_ARG, w + ": " + std::to_string(n_ltris) + " light triangles, the handle has " + std::to_string(sc->ltri_mat.size()));
    if (n_ltris && !ltris) return fail(CRT_ERR_INVALID_ARG, w + ": null light triangle array");
    if (form_of_environment() < 0) return fail(CRT_ERR_INVALID_ARG, w + ": CRT_REFIT_FORM must be levels or walk");
    return CRT_OK;
}

int refit_impl(crt_scene* sc, const void* d_tris, const void* d_ltris, hipStream_t s, crt_refit_info* info)
{
    const int form = form_of_environment();
    float prepare_ms = 0.0f;
    if (!sc->refit) {
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = prepare(sc);
        if (rc != CRT_OK) return rc;
        prepare_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    RefitState* st = sc->refit;
    if (st->walk_open || st->gen >= (1u << 28)) { // (the walk's counters count arrivals since they were zeroed: start over long before they wrap)
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemset(st->cnt.p, 0, st->cnt.n * sizeof(unsigned int)));
        st->gen = 0;
        st->walk_open = false;
    }
    const bool impl = sc->can(crtlayout::CAP_IMPL);
    RefitParams P{};
    P.tris = (const float*)d_tris; P.ltris = (const float*)d_ltris;
    P.n_tris = sc->n_tris; P.n_ltris = (uint32_t)sc->ltri_mat.size(); P.n_rec = st->n_rec;
    P.tri_geo = sc->tri_geo.p; P.tri_nm = sc->tri_nm.p; P.leaf_geo = sc->leaf_geo.p; P.leaf_geo_i = impl ? sc->leaf_geo_i.p : nullptr; P.ltri = sc->ltri.p;
    P.rec_map = impl ? sc->rec_map.p : nullptr;
    P.leaves = st->leaves.p; P.n_leaves = st->n_leaves; P.n_tasks = st->n_tasks; P.tasks = st->tasks.p;
    P.nodes = sc->nodes.p; P.nodes3 = sc->nodes3.p; P.nodes4 = sc->nodes4.p; P.nodes4i = impl ? sc->nodes4i.p : nullptr;
    P.box = st->box.p; P.cm = st->cm.p; P.cnt = st->cnt.p; P.gen = st->gen + 1; P.res = st->res.p;
    uint32_t launches = 0;
    auto launch = [&](void (*k)(const RefitParams), uint64_t threads) {
        if (threads == 0) return;
        hipLaunchKernelGGL(k, dim3(blocks_of(threads)), dim3(256), 0, s, P);
        HIP_CHECK(hipGetLastError());
        launches++;
    };
    HIP_CHECK(hipEventRecord(st->e0, s));
    HIP_CHECK(hipMemsetAsync(st->res.p, 0, sizeof(RefitResult), s));
    launch(k_refit_check, (uint64_t)P.n_tris + P.n_ltris);
    launch(k_refit_rows, (uint64_t)P.n_tris + P.n_rec + P.n_ltris);
    launch(k_refit_leaves, P.n_leaves);
    if (form == 0) {
        for (size_t h = 0; h + 1 < st->level.size(); h++) {
            P.first = st->level[h]; P.count = st->level[h + 1] - st->level[h];
            launch(k_refit_level, P.count);
        }
    } else if (st->level.size() > 1) {
        P.first = 0; P.count = st->level[1];
        st->walk_open = true;
        launch(k_refit_walk, P.count);
    }
    if (P.n_tasks) {
        hipLaunchKernelGGL(k_refit_finish, dim3(1), dim3(256), 0, s, P);
        HIP_CHECK(hipGetLastError());
        launches++;
    }
    HIP_CHECK(hipMemcpyAsync(st->h_res, st->res.p, sizeof(RefitResult), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipEventRecord(st->e1, s));
    HIP_CHECK(hipStreamSynchronize(s)); // the one synchronization of a refit: was it refused, and the scalars the host keeps
    const RefitResult R = *st->h_res;
    st->walk_open = false;
    if (R.bad != 0u) // (no kernel wrote, the walk's counters included)
        return fail(CRT_ERR_INVALID_ARG, "crt_scene_refit: " + std::to_string(R.bad) + " triangles have a vertex coordinate that is not finite or beyond 2^126; the handle is as it was");
    if (form == 1 && st->level.size() > 1) st->gen++; // only a walk advances the counters
    float cmax;
    std::memcpy(&cmax, &R.coord_max_bits, 4);
    sc->scalars.coord_max = cmax; sc->dev.coord_max = cmax;
    std::memcpy(sc->root_aa, R.root_lo, sizeof(sc->root_aa));
    std::memcpy(sc->root_bb, R.root_hi, sizeof(sc->root_bb));
    sc->acc.samples = 0; sc->var.valid = false; sc->half.valid = false; sc->pf_mark.valid = false; // the frame in flight ends, as at a new frame's start
    if (info) {
        crt_refit_info I;
        std::memset(&I, 0, sizeof(I));
        I.n_tris = P.n_tris; I.n_light_tris = P.n_ltris; I.leaves = st->n_leaves; I.boxes_written = st->boxes; I.launches = launches; I.form = (uint32_t)form;
        std::memcpy(I.root_aa, sc->root_aa, sizeof(I.root_aa)); std::memcpy(I.root_bb, sc->root_bb, sizeof(I.root_bb));
        I.coord_max = cmax; I.prepare_ms = prepare_ms;
        HIP_CHECK(hipEventElapsedTime(&I.device_ms, st->e0, st->e1));
        *info = I;
    }
    return CRT_OK;
}

} // namespace

extern "C" {

int crt_scene_refit_device(crt_scene* sc, const void* d_tris, uint32_t n_tris, const void* d_light_tris, uint32_t n_light_tris, void* stream, crt_refit_info* info)
{
    const int rc = refit_check_args(sc, d_tris, n_tris, d_light_tris, n_light_tris);
    if (rc != CRT_OK) return rc;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        return refit_impl(sc, d_tris, d_light_tris, (hipStream_t)stream, info);
    });
}

int crt_scene_refit(crt_scene* sc, const crt_triangle* tris, uint32_t n_tris, const crt_triangle* light_tris, uint32_t n_light_tris, crt_refit_info* info)
{
    const int rc = refit_check_args(sc, tris, n_tris, light_tris, n_light_tris);
    if (rc != CRT_OK) return rc;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        float prepare_ms = 0.0f;
        if (!sc->refit) {
            const auto t0 = std::chrono::steady_clock::now();
            const int rcp = prepare(sc);
            if (rcp != CRT_OK) return rcp;
            prepare_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        RefitState* st = sc->refit;
        if (st->tri_mat.size() != sc->n_tris) st->tri_mat = read_back(sc->tri_mat, sc->n_tris);
        for (uint32_t i = 0; i < n_tris; i++)
            if (tris[i].material != st->tri_mat[i])
                return fail(CRT_ERR_INVALID_ARG, "crt_scene_refit: triangle " + std::to_string(i) + " has another material than the handle's (a refit moves triangles only)");
        for (uint32_t i = 0; i < n_light_tris; i++)
            if (light_tris[i].material != sc->ltri_mat[i])
                return fail(CRT_ERR_INVALID_ARG, "crt_scene_refit: light triangle " + std::to_string(i) + " has another material than the handle's (a refit moves triangles only)");
        st->up_tris.ensure((size_t)n_tris * kRefitTriWords);
        HIP_CHECK(hipMemcpy(st->up_tris.p, tris, (size_t)n_tris * sizeof(crt_triangle), hipMemcpyHostToDevice));
        if (n_light_tris) {
            st->up_ltris.ensure((size_t)n_light_tris * kRefitTriWords);
            HIP_CHECK(hipMemcpy(st->up_ltris.p, light_tris, (size_t)n_light_tris * sizeof(crt_triangle), hipMemcpyHostToDevice));
        }
        const int rcr = refit_impl(sc, st->up_tris.p, n_light_tris ? st->up_ltris.p : nullptr, nullptr, info);
        if (rcr == CRT_OK && info) info->prepare_ms = prepare_ms;
        return rcr;
    });
}

} // extern "C"
