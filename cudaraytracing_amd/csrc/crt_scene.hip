// cudaraytracing_amd/csrc/crt_scene.hip -- the scene handle's life in the C ABI of include/crt.h: crt_scene_create (check the description,
// build every array on the host -- crt_scene_layout.h -- and upload it byte for byte), crt_scene_accel_info, crt_scene_export,
// crt_scene_destroy, and the two entry points that need no handle (crt_device_count, crt_shard_slots).
#include "crt_scene.h"

#include <atomic>
#include <chrono>
#include <cstring>
#include <new>
#include <string>

using namespace crtdev;
using namespace crtk;
using crtlayout::SceneLayout;

static_assert(sizeof(crtlayout::Row4) == sizeof(float4) && offsetof(crtlayout::Row4, w) == offsetof(float4, w), "Row4 is float4's layout");
static_assert(sizeof(crtlayout::URow4) == sizeof(uint4) && offsetof(crtlayout::URow4, w) == offsetof(uint4, w), "URow4 is uint4's layout");
static_assert(crtlayout::kNode4iF4 == NODE4I_F4 && crtlayout::kLeafRecMax == LEAF_REC_MAX, "the layout's constants are the kernels'");

namespace {

// The HIP runtime starts with the first call that needs the device (context, the library's code objects): timed by itself so that it
// is not booked on whatever happens to come first (it was the SAH build's first upload: "147 ms" of tree building).  Returns the host
// clock in ms.
float warm_up_runtime(int device)
{
    const auto t0 = std::chrono::steady_clock::now();
    HIP_CHECK(hipSetDevice(device));
    // (round 6: the first copy from / to pageable memory beyond the runtime's small-copy path sets up its staging -- 7.3 - 8.7 ms once
    // per process, 0.03 ms from then on, tools/copy_probe.cpp -- and was booked on the tree build's first upload and download; the 3 MB
    // download of the built tree paid another 8.6 ms after a 512 KB warm-up: the path beyond 1 MB.  Once per device and process.)
    static std::atomic<uint64_t> warmed{0};
    const uint64_t bit = 1ull << (device & 63);
    if (!(warmed.fetch_or(bit) & bit)) {
        std::vector<char> page(4u << 20, 0);
        DevBuf<char> warm;
        warm.ensure(page.size());
        HIP_CHECK(hipMemcpy(warm.p, page.data(), page.size(), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(page.data(), warm.p, page.size(), hipMemcpyDeviceToHost));
    } else {
        HIP_CHECK(hipFree(nullptr)); // (the context, if this thread has none yet)
    }
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The layout's arrays to the device, byte for byte, and its scalars to the handle and its DevScene
void upload_layout(crt_scene* sc, const SceneLayout& L)
{
    DevScene& dev = sc->dev;
    if (L.accel.layout_caps & crtlayout::CAP_IMPL) {
        dev.nodes4i = sc->nodes4i.upload(L.nodes4i); dev.leaf_geo_i = sc->leaf_geo_i.upload(L.leaf_geo_i); dev.rec_map = sc->rec_map.upload(L.rec_map);
    }
    dev.nodes4 = sc->nodes4.upload(L.nodes4);
    dev.nodes3 = sc->nodes3.upload(L.nodes3); dev.leaf_geo = sc->leaf_geo.upload(L.leaf_geo); dev.tri_nm = sc->tri_nm.upload(L.tri_nm);
    dev.nodes = sc->nodes.upload(L.nodes); dev.tri_geo = sc->tri_geo.upload(L.tri_geo); dev.tri_mat = sc->tri_mat.upload(L.tri_mat);
    dev.mats = sc->mats.upload(L.mats); dev.ltri = sc->ltri.upload(L.ltri); dev.lights = sc->lights.upload(L.lights);
    dev.leaf_count = sc->leaf_count.upload(L.leaf_count);
    const crt_tree_scalars& s = L.scalars;
    dev.root_fast = s.root_fast; dev.root_exact = s.root_exact; dev.root3_fast = s.root3_fast; dev.root3_exact = s.root3_exact;
    dev.root4 = s.root4; dev.root4i = s.root4i; dev.n_mixed4i = s.n_mixed4i; dev.empty4_off = s.empty4_off; dev.empty4i_off = s.empty4i_off;
    dev.coord_max = s.coord_max;
    sc->scalars = s;
    sc->stack_cap = (int)s.stack_cap;
    sc->max_leaf = L.max_leaf;
    const float runtime_init_ms = sc->accel.runtime_init_ms;
    sc->accel = L.accel;
    sc->accel.runtime_init_ms = runtime_init_ms;
}

// What every frame on the handle needs beside the scene: cursors and counters, the second stream, events, the device's size
void create_frame_resources(crt_scene* sc)
{
    sc->counters.alloc((size_t)CNT_SHARDS * CNT_STRIDE);
    sc->item_next.alloc((size_t)1024 * ITEM_STRIDE); // (a commit-ring launch has up to 1 024 cursor shards)
    sc->slot_next[0].alloc((size_t)SLOT_SHARDS * SLOT_STRIDE);
    sc->slot_next[1].alloc((size_t)SLOT_SHARDS * SLOT_STRIDE);
    HIP_CHECK(hipStreamCreateWithFlags(&sc->aux_stream, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&sc->ev_fork, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&sc->ev_join, hipEventDisableTiming));
    HIP_CHECK(hipEventCreate(&sc->ev_k0));
    HIP_CHECK(hipEventCreate(&sc->ev_k1));
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, sc->device));
    sc->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIP_CHECK(hipHostMalloc((void**)&sc->h_counters, (size_t)CNT_SHARDS * CNT_STRIDE * sizeof(unsigned long long), hipHostMallocDefault));
}

} // namespace

extern "C" {

int crt_device_count(int* count)
{
    if (!count) return fail(CRT_ERR_INVALID_ARG, "crt_device_count: null argument");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(CRT_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
    *count = n;
    return CRT_OK;
}

int crt_shard_slots(uint32_t width, uint32_t height, uint32_t rank, uint32_t world, uint64_t* slots)
{
    if (!slots || width == 0 || height == 0 || world == 0 || rank >= world) return fail(CRT_ERR_INVALID_ARG, "crt_shard_slots: bad arguments");
    *slots = make_shard(width, height, world).nslots;
    return CRT_OK;
}

int crt_scene_create(const crt_scene_desc* d, int device, crt_scene** out)
{
    if (!out) return fail(CRT_ERR_INVALID_ARG, "crt_scene_create: null output");
    *out = nullptr;
    const char* msg = nullptr;
    int rc = crtlayout::validate_desc(d, msg);
    if (rc != CRT_OK) return fail(rc, msg);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(CRT_ERR_NO_DEVICE, "crt_scene_create: no HIP device available");
    if (device < 0 || device >= n) return fail(CRT_ERR_INVALID_ARG, "crt_scene_create: device index out of range");
    crt_scene* sc = nullptr;
    try {
        sc = new crt_scene();
        sc->device = device;
        sc->accel.runtime_init_ms = warm_up_runtime(device);
        SceneLayout L;
        crtlayout::build_scene_layout(*d, crtaccel::build_sah_device, L);
        upload_layout(sc, L);
        sc->dev.n_lights = (int32_t)d->n_lights;
        sc->n_tris = d->n_tris;
        sc->n_mats = d->n_materials;
        sc->ltri_mat.resize(d->n_light_tris);
        for (uint32_t i = 0; i < d->n_light_tris; i++) sc->ltri_mat[i] = d->light_tris[i].material;
        std::memcpy(sc->root_aa, d->nodes[d->root].aa, sizeof(sc->root_aa));
        std::memcpy(sc->root_bb, d->nodes[d->root].bb, sizeof(sc->root_bb));
        create_frame_resources(sc);
        *out = sc;
        return CRT_OK;
    } catch (const HipFail& f) {
        delete sc;
        return fail_hip(f);
    } catch (const std::bad_alloc&) {
        delete sc;
        return fail(CRT_ERR_OOM, "crt_scene_create: out of host memory");
    }
}

int crt_scene_accel_info(crt_scene* sc, crt_accel_info* out)
{
    if (!sc || !out) return fail(CRT_ERR_INVALID_ARG, "crt_scene_accel_info: null argument");
    *out = sc->accel;
    return CRT_OK;
}

int crt_scene_export(crt_scene* sc, const char* name, void* dst, size_t capacity, size_t* bytes)
{
    if (!bytes) return fail(CRT_ERR_INVALID_ARG, "crt_scene_export: null bytes");
    static const char* names[] = {"nodes", "nodes3", "nodes4", "nodes4i", "leaf_geo", "leaf_geo_i", "rec_map", "tri_geo", "leaf_count", "tri_nm", "scalars", "ltri"};
    int id = -1;
    for (int i = 0; name && i < 12; i++)
        if (std::strcmp(name, names[i]) == 0) id = i;
    if (id < 0) return fail(CRT_ERR_INVALID_ARG, std::string("crt_scene_export: unknown array ") + (name ? name : "(null)"));
    if (!sc) return fail(CRT_ERR_INVALID_ARG, "crt_scene_export: null scene");
    if (id == 10) {
        *bytes = sizeof(sc->scalars);
        if (!dst) return CRT_OK;
        if (capacity < sizeof(sc->scalars)) return fail(CRT_ERR_INVALID_ARG, "crt_scene_export: capacity below the size");
        std::memcpy(dst, &sc->scalars, sizeof(sc->scalars));
        return CRT_OK;
    }
    // the device arrays themselves (DevBuf::n: the uploaded count -- an empty upload allocates one unused element, reported as 0)
    const bool leaf_root = sc->dev.root_fast < 0, impl = sc->can(crtlayout::CAP_IMPL);
    const void* src = nullptr;
    size_t n = 0;
    auto arr = [&](const auto& b, bool have) { src = b.p; n = have ? b.n * sizeof(*b.p) : 0; };
    switch (id) {
    case 0: arr(sc->nodes, !leaf_root); break;
    case 1: arr(sc->nodes3, !leaf_root); break;
    case 2: arr(sc->nodes4, true); break;
    case 3: arr(sc->nodes4i, impl); break;
    case 4: arr(sc->leaf_geo, true); break;
    case 5: arr(sc->leaf_geo_i, impl); break;
    case 6: arr(sc->rec_map, impl); break;
    case 7: arr(sc->tri_geo, true); break;
    case 8: arr(sc->leaf_count, true); break;
    case 11: arr(sc->ltri, !sc->ltri_mat.empty()); break;
    default: arr(sc->tri_nm, true); break;
    }
    *bytes = n;
    if (!dst || n == 0) return CRT_OK;
    if (capacity < n) return fail(CRT_ERR_INVALID_ARG, "crt_scene_export: capacity below the size");
    try {
        HIP_CHECK(hipSetDevice(sc->device));
        HIP_CHECK(hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
        return CRT_OK;
    } catch (const HipFail& f) {
        return fail_hip(f);
    }
}

int crt_scene_destroy(crt_scene* sc)
{
    if (!sc) return CRT_OK;
    (void)hipSetDevice(sc->device);
    delete sc;
    return CRT_OK;
}

} // extern "C"
