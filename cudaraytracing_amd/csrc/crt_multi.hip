// cudaraytracing_amd/csrc/crt_multi.hip -- one process, N MI355X: the multi-device entry of libcrt.so.
//
// The reference selects device 0 and stops there (config_CUDA, src/main.cu:92-105; one kernel launch per
// frame, Render.cuh:435-440).  Pixels are independent and every random draw is keyed by the global pixel
// index, so the frame is sharded by interleaved 8x8 pixel tiles: tile t belongs to rank
// t % N.  A crt_multi owns one device replica of the scene per rank (crt_scene_create on each device),
// renders all shards concurrently (one host thread per device drives its own HIP stream), exchanges the
// compact tile buffers with ONE collective -- ncclAllGather over RCCL / xGMI, every link carries each
// peer's slice once -- and de-interleaves the gathered tiles into the row-major frame on rank 0.
// A frame is a set of planes (crt_multi_render_buffers: RGB8, the mean, the variance, the half buffers, the first-hit and the shading
// AOVs): a rank's block holds its tiles of every wanted plane, so the exchange stays ONE collective and the de-interleave ONE launch
// (crt_untile.h).  crt_multi_render is the frame of RGB8 and the mean; render_planes below is the one implementation of both.
//
// RCCL is bound at run time (dlopen "librccl.so.1"): libcrt.so stays loadable on a box without it, and a
// process that has already loaded PyTorch's RCCL shares that copy instead of mapping a second one.
// CRT_GATHER_COPY replaces the collective by peer copies into rank 0's buffer (hipMemcpyPeerAsync); it is
// also what runs when two ranks share one device (test configuration: RCCL refuses duplicate devices).
#include "../../include/crt.h"

#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// The handful of RCCL declarations this file needs, restated so that libcrt.so builds on a box without the RCCL headers (the
// library itself is bound with dlopen below).  Values as in rccl.h / nccl.h: ncclSuccess = 0, ncclUint8 = 1.
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef int ncclResult_t;
typedef int ncclDataType_t;
enum { ncclSuccess = 0 };
enum { ncclUint8 = 1 };
ncclResult_t ncclGetVersion(int* version);
ncclResult_t ncclCommInitAll(ncclComm_t* comms, int ndev, const int* devlist);
ncclResult_t ncclCommDestroy(ncclComm_t comm);
ncclResult_t ncclCommCount(const ncclComm_t comm, int* count);
ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype, ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclGroupStart(void);
ncclResult_t ncclGroupEnd(void);
const char* ncclGetErrorString(ncclResult_t result);
}

extern "C" void crt_set_last_error_(const char* msg);

namespace {

int mfail(int status, const std::string& msg)
{
    crt_set_last_error_(msg.c_str());
    return status;
}

struct HipErr {
    hipError_t e;
    const char* what;
};
#define MHIP(call)                                          \
    do {                                                    \
        hipError_t e_ = (call);                             \
        if (e_ != hipSuccess) throw HipErr{e_, #call};      \
    } while (0)

// ---- RCCL entry points, resolved once per process ----
struct Rccl {
    void* handle = nullptr;
    decltype(&ncclGetVersion) GetVersion = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string error;
    bool ok = false;
};

void rccl_load(Rccl& R);
Rccl& rccl()
{
    static Rccl R;
    static std::once_flag once;
    std::call_once(once, [] { rccl_load(R); });
    return R;
}
void rccl_load(Rccl& R)
{
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
        R.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (R.handle) break;
    }
    if (!R.handle) {
        const char* e = dlerror();
        R.error = std::string("cannot load librccl.so.1: ") + (e ? e : "?");
        return;
    }
#define SYM(field, name)                                                      \
    R.field = (decltype(R.field))dlsym(R.handle, name);                       \
    if (!R.field) { R.error = std::string("librccl: missing symbol ") + name; return; }
    SYM(GetVersion, "ncclGetVersion")
    SYM(CommInitAll, "ncclCommInitAll")
    SYM(CommDestroy, "ncclCommDestroy")
    SYM(CommCount, "ncclCommCount")
    SYM(AllGather, "ncclAllGather")
    SYM(GroupStart, "ncclGroupStart")
    SYM(GroupEnd, "ncclGroupEnd")
    SYM(GetErrorString, "ncclGetErrorString")
#undef SYM
    R.ok = true;
}

// Restores the calling thread's current device on every way out (the entry points walk over the ranks' devices).
struct DeviceGuard {
    int dev = -1;
    DeviceGuard() { if (hipGetDevice(&dev) != hipSuccess) dev = -1; }
    ~DeviceGuard() { if (dev >= 0) (void)hipSetDevice(dev); }
};

struct NcclErr {
    ncclResult_t r;
    const char* what;
};
#define MNCCL(call)                                         \
    do {                                                    \
        ncclResult_t r_ = (call);                           \
        if (r_ != ncclSuccess) throw NcclErr{r_, #call};    \
    } while (0)

} // namespace

// Gathered tile blocks -> row-major planes on rank 0: the index arithmetic and k_untile_planes
#include "crt_untile.h"

namespace {

// The planes a frame can be gathered as, in the order of their CRT_MULTI_* bits -- which is their order in a rank's block and the
// order of crt_multi_buffers' members.
struct PlaneKind { uint32_t bit, per_pixel, elem; };
const PlaneKind kPlanes[crtk::kUntileMaxPlanes] = {
    {CRT_MULTI_RGB, 3, 1},      {CRT_MULTI_MEAN, 3, 4},     {CRT_MULTI_VARIANCE, 3, 4}, {CRT_MULTI_HALF_A, 3, 4},   {CRT_MULTI_HALF_B, 3, 4},
    {CRT_MULTI_ALBEDO, 3, 4},   {CRT_MULTI_NORMAL, 3, 4},   {CRT_MULTI_DEPTH, 1, 4},    {CRT_MULTI_COVERAGE, 1, 4}, {CRT_MULTI_TRI, 1, 4},
    {CRT_MULTI_MATERIAL, 1, 4}, {CRT_MULTI_EMISSION, 3, 4}, {CRT_MULTI_DIFFUSE_ALBEDO, 3, 4}};
enum { P_RGB, P_MEAN, P_VARIANCE, P_HALF_A, P_HALF_B, P_ALBEDO, P_NORMAL, P_DEPTH, P_COVERAGE, P_TRI, P_MATERIAL, P_EMISSION, P_DIFFUSE_ALBEDO };
const uint32_t kFirstHitPlanes = CRT_MULTI_ALBEDO | CRT_MULTI_NORMAL | CRT_MULTI_DEPTH | CRT_MULTI_COVERAGE | CRT_MULTI_TRI | CRT_MULTI_MATERIAL;
const uint32_t kShadingPlanes = CRT_MULTI_EMISSION | CRT_MULTI_DIFFUSE_ALBEDO;

void* plane_of(const crt_multi_buffers& b, uint32_t k)
{
    void* const p[crtk::kUntileMaxPlanes] = {b.rgb, b.mean, b.variance, b.half_a, b.half_b, b.albedo, b.normal, b.depth, b.coverage, b.tri, b.material,
                                             b.emission, b.diffuse_albedo};
    return p[k];
}
crt_multi_buffers buffers_of(void* const* p)
{
    return crt_multi_buffers{(uint8_t*)p[P_RGB], (float*)p[P_MEAN], (float*)p[P_VARIANCE], (float*)p[P_HALF_A], (float*)p[P_HALF_B], (float*)p[P_ALBEDO],
                             (float*)p[P_NORMAL], (float*)p[P_DEPTH], (float*)p[P_COVERAGE], (int32_t*)p[P_TRI], (int32_t*)p[P_MATERIAL],
                             (float*)p[P_EMISSION], (float*)p[P_DIFFUSE_ALBEDO]};
}

// A rank's block for a request mask: the wanted planes one after the other, each from a 16-byte boundary; 64-bit byte offsets
struct BlockLayout {
    uint64_t off[crtk::kUntileMaxPlanes]; // of a wanted plane
    uint64_t stride = 0;
};
BlockLayout block_layout(uint32_t want, uint64_t slots)
{
    BlockLayout L;
    for (uint32_t k = 0; k < crtk::kUntileMaxPlanes; k++) {
        L.off[k] = L.stride;
        if (want & kPlanes[k].bit) L.stride += crtk::untile_plane_bytes(slots, kPlanes[k].per_pixel, kPlanes[k].elem);
    }
    return L;
}

struct Rank {
    int device = 0;
    crt_scene* scene = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    uint8_t* local = nullptr;    // this rank's block (stride bytes)
    uint8_t* gathered = nullptr; // world blocks (RCCL: every rank; COPY: rank 0 only)
    uint8_t* rgb_scratch = nullptr; // the shard's RGB8 tiles of a frame whose RGB plane is not wanted (crt_render_device always writes them)
    size_t local_cap = 0, gathered_cap = 0, rgb_scratch_cap = 0;
    ncclComm_t comm = nullptr;
};

} // namespace

struct crt_multi {
    std::vector<Rank> ranks;
    uint32_t gather = CRT_GATHER_COPY; // what runs
    int rccl_version = 0;
    int rccl_ranks = 0;
    uint8_t* plane[crtk::kUntileMaxPlanes] = {}; // rank 0: the row-major planes, in kPlanes' order (RGB8 first, then the mean)
    size_t plane_cap[crtk::kUntileMaxPlanes] = {};
    uint32_t last_want = 0;     // the planes the last render wrote (0: none yet, or it failed)
    crtk::UntileParams last_untile{}; // ... and the de-interleave that wrote them (crt_multi_untile_time)
    std::string fallback_reason; // CRT_GATHER_AUTO only: why RCCL was not used although the devices are distinct (empty: no fallback happened)
};

namespace {

void ensure(uint8_t*& p, size_t& cap, size_t bytes)
{
    if (cap >= bytes) return;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    MHIP(hipMalloc((void**)&p, bytes));
    cap = bytes;
}

void destroy(crt_multi* m)
{
    if (!m) return;
    Rccl& R = rccl();
    for (Rank& rk : m->ranks) {
        (void)hipSetDevice(rk.device);
        if (rk.comm && R.ok) (void)R.CommDestroy(rk.comm);
        if (rk.scene) (void)crt_scene_destroy(rk.scene);
        if (rk.local) (void)hipFree(rk.local);
        if (rk.gathered) (void)hipFree(rk.gathered);
        if (rk.rgb_scratch) (void)hipFree(rk.rgb_scratch);
        if (rk.done) (void)hipEventDestroy(rk.done);
        if (rk.stream) (void)hipStreamDestroy(rk.stream);
    }
    if (!m->ranks.empty()) (void)hipSetDevice(m->ranks[0].device);
    for (uint8_t* p : m->plane)
        if (p) (void)hipFree(p);
    delete m;
}

} // namespace

extern "C" {

int crt_multi_create(const crt_scene_desc* desc, const int* devices, uint32_t n_devices, uint32_t gather, crt_multi** out)
{
    if (!out) return mfail(CRT_ERR_INVALID_ARG, "crt_multi_create: null output");
    *out = nullptr;
    if (!desc || !devices || n_devices == 0 || n_devices > 64) return mfail(CRT_ERR_INVALID_ARG, "crt_multi_create: need 1..64 devices");
    if (gather > CRT_GATHER_COPY) return mfail(CRT_ERR_INVALID_ARG, "crt_multi_create: unknown gather mode");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return mfail(CRT_ERR_NO_DEVICE, "crt_multi_create: no HIP device available");
    bool distinct = true;
    for (uint32_t a = 0; a < n_devices; a++) {
        if (devices[a] < 0 || devices[a] >= n_dev) return mfail(CRT_ERR_INVALID_ARG, "crt_multi_create: device index out of range");
        for (uint32_t b = 0; b < a; b++) distinct = distinct && devices[a] != devices[b];
    }
    if (gather == CRT_GATHER_RCCL && !distinct) return mfail(CRT_ERR_INVALID_ARG, "crt_multi_create: RCCL needs one rank per device (duplicate device index)");
    const uint32_t requested = gather;
    // Test hooks (the fallback below could not run on a one-GPU box).  CRT_TEST_RCCL_AUTO_ONE_DEVICE=1: AUTO attempts RCCL with a
    // single device too (a one-rank communicator).  CRT_TEST_RCCL_FAIL=load | init | count: the binding of librccl is treated as failed /
    // the communicator is made, then treated as failed and destroyed / ncclCommCount is treated as reporting another number of ranks.
    const char* t_one_ = std::getenv("CRT_TEST_RCCL_AUTO_ONE_DEVICE");
    const char* t_fail_ = std::getenv("CRT_TEST_RCCL_FAIL");
    const std::string inject = t_fail_ ? t_fail_ : "";
    const bool auto_one = t_one_ && t_one_[0] == '1';
    if (gather == CRT_GATHER_AUTO) gather = (distinct && (n_devices > 1 || auto_one)) ? CRT_GATHER_RCCL : CRT_GATHER_COPY;
    DeviceGuard guard;
    crt_multi* m = nullptr;
    try {
        m = new crt_multi();
        m->gather = gather;
        m->ranks.resize(n_devices);
        for (uint32_t r = 0; r < n_devices; r++) {
            Rank& rk = m->ranks[r];
            rk.device = devices[r];
            int rc = crt_scene_create(desc, rk.device, &rk.scene); // (leaves the device current)
            if (rc != CRT_OK) { destroy(m); return rc; }
            MHIP(hipSetDevice(rk.device));
            MHIP(hipStreamCreateWithFlags(&rk.stream, hipStreamNonBlocking));
            MHIP(hipEventCreateWithFlags(&rk.done, hipEventDisableTiming));
        }
        // CRT_GATHER_AUTO prefers RCCL but does not depend on it: if the library cannot be bound or the communicator cannot be made (a
        // node whose fabric RCCL refuses, a container without the IPC mode it needs), the frame is gathered by peer copies instead and
        // crt_multi_info::fallback_reason says why.  An explicit CRT_GATHER_RCCL fails loudly, as before.
        const bool auto_mode = requested == CRT_GATHER_AUTO;
        if (gather == CRT_GATHER_RCCL) {
            std::string why;
            Rccl& R = rccl();
            if (!R.ok) why = R.error;
            else if (inject == "load") why = "cannot load librccl.so.1: (injected by CRT_TEST_RCCL_FAIL=load)";
            else {
                std::vector<ncclComm_t> comms(n_devices, nullptr);
                std::vector<int> devs(devices, devices + n_devices);
                ncclResult_t rv = R.GetVersion(&m->rccl_version);
                if (rv == ncclSuccess) rv = R.CommInitAll(comms.data(), (int)n_devices, devs.data());
                if (rv == ncclSuccess) {
                    for (uint32_t r = 0; r < n_devices; r++) m->ranks[r].comm = comms[r];
                    rv = R.CommCount(comms[0], &m->rccl_ranks);
                }
                if (rv == ncclSuccess && inject == "count") m->rccl_ranks = (int)n_devices + 1;
                if (rv != ncclSuccess || inject == "init") {
                    why = std::string("ncclCommInitAll / ncclCommCount: ") + (rv != ncclSuccess ? R.GetErrorString(rv) : "(injected by CRT_TEST_RCCL_FAIL=init)");
                    for (uint32_t r = 0; r < n_devices; r++) {
                        if (m->ranks[r].comm) { (void)hipSetDevice(m->ranks[r].device); (void)R.CommDestroy(m->ranks[r].comm); m->ranks[r].comm = nullptr; }
                    }
                    (void)hipGetLastError();
                } else if (m->rccl_ranks != (int)n_devices) {
                    why = "ncclCommCount reports " + std::to_string(m->rccl_ranks) + " ranks for " + std::to_string(n_devices) + " devices";
                }
            }
            if (!why.empty()) {
                if (!auto_mode) { destroy(m); return mfail(R.ok ? CRT_ERR_HIP : CRT_ERR_UNSUPPORTED, "crt_multi_create: " + why); }
                for (uint32_t r = 0; r < n_devices; r++) {
                    if (m->ranks[r].comm) { (void)hipSetDevice(m->ranks[r].device); (void)R.CommDestroy(m->ranks[r].comm); m->ranks[r].comm = nullptr; }
                }
                m->fallback_reason = why;
                m->rccl_ranks = 0;
                gather = CRT_GATHER_COPY;
                m->gather = gather;
            }
        }
        if (gather == CRT_GATHER_COPY && distinct && n_devices > 1) {
            // rank 0 receives peer writes
            for (uint32_t r = 1; r < n_devices; r++) {
                int can = 0;
                MHIP(hipDeviceCanAccessPeer(&can, m->ranks[r].device, m->ranks[0].device));
                if (can) {
                    MHIP(hipSetDevice(m->ranks[r].device));
                    hipError_t e = hipDeviceEnablePeerAccess(m->ranks[0].device, 0);
                    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) throw HipErr{e, "hipDeviceEnablePeerAccess"};
                    (void)hipGetLastError();
                }
            }
        }
        *out = m;
        return CRT_OK;
    } catch (const HipErr& f) {
        std::string msg = std::string("crt_multi_create: ") + f.what + ": " + hipGetErrorString(f.e);
        destroy(m);
        return mfail(CRT_ERR_HIP, msg);
    } catch (const NcclErr& f) {
        std::string msg = std::string("crt_multi_create: ") + f.what + ": " + rccl().GetErrorString(f.r);
        destroy(m);
        return mfail(CRT_ERR_HIP, msg);
    } catch (const std::bad_alloc&) {
        destroy(m);
        return mfail(CRT_ERR_OOM, "crt_multi_create: out of host memory");
    }
}

int crt_multi_destroy(crt_multi* m)
{
    destroy(m);
    return CRT_OK;
}

} // extern "C"

namespace {

// The one implementation of a multi-device frame: every rank renders its tiles of the wanted planes into its block, one exchange,
// rank 0 de-interleaves.  `who` names the entry point in messages; its argument checks have run.
int render_planes(const char* who_, crt_multi* m, const crt_camera* cam, const crt_params* prm, const uint32_t want, const crt_multi_buffers& host_out,
                  crt_stats* stats, crt_multi_info* info)
{
    const std::string who = who_;
    const uint32_t world = (uint32_t)m->ranks.size();
    const bool want_sums = (want & CRT_MULTI_VARIANCE) != 0, want_halves = (want & (CRT_MULTI_HALF_A | CRT_MULTI_HALF_B)) != 0;
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    DeviceGuard guard;
    // an error must not leave work in flight on buffers the next call may free or reallocate
    auto drain = [&]() {
        for (Rank& rk : m->ranks)
            if (hipSetDevice(rk.device) == hipSuccess && rk.stream) (void)hipStreamSynchronize(rk.stream);
    };
    m->last_want = 0;
    try {
        uint64_t slots = 0;
        int rc = crt_shard_slots(prm->width, prm->height, 0, world, &slots);
        if (rc != CRT_OK) return rc;
        const BlockLayout L = block_layout(want, slots);
        const uint64_t stride = L.stride;
        for (uint32_t r = 0; r < world; r++) {
            Rank& rk = m->ranks[r];
            MHIP(hipSetDevice(rk.device));
            ensure(rk.local, rk.local_cap, stride);
            if (!(want & CRT_MULTI_RGB)) ensure(rk.rgb_scratch, rk.rgb_scratch_cap, slots * 3);
            if (m->gather == CRT_GATHER_RCCL || r == 0) ensure(rk.gathered, rk.gathered_cap, stride * world);
        }
        MHIP(hipSetDevice(m->ranks[0].device));
        const uint64_t pixels = (uint64_t)prm->width * prm->height;
        auto plane_bytes = [&](uint32_t k) { return (size_t)(pixels * kPlanes[k].per_pixel * kPlanes[k].elem); };
        for (uint32_t k = 0; k < crtk::kUntileMaxPlanes; k++)
            if ((want & kPlanes[k].bit) || k == P_RGB) ensure(m->plane[k], m->plane_cap[k], plane_bytes(k)); // (RGB: crt_multi_frame_device has always had a frame to report)
        // ---- every rank renders its tiles: one host thread per device, each on its own stream ----
        std::vector<int> rcs(world, CRT_OK);
        std::vector<std::string> errs(world);
        std::vector<crt_stats> st(world);
        auto work = [&](uint32_t r) {
            Rank& rk = m->ranks[r];
            crt_params p = *prm;
            p.rank = r; p.world = world;
            p.flags |= CRT_FLAG_TILED_OUTPUT;
            // the sums of crt_variance and crt_half_buffers are kept exactly when a plane needs them (a frame of RGB and the mean: never)
            p.flags &= ~(uint32_t)(CRT_FLAG_VARIANCE | CRT_FLAG_HALF_BUFFERS | CRT_FLAG_PIXEL_FILTER); // (a shard keeps no filter sums: it does not hold its pixels' neighbours)
            if (want_sums) p.flags |= CRT_FLAG_VARIANCE;
            if (want_halves) p.flags |= CRT_FLAG_HALF_BUFFERS;
            auto at = [&](uint32_t k) -> uint8_t* { return (want & kPlanes[k].bit) ? rk.local + L.off[k] : nullptr; };
            auto step = [&](int status) {
                rcs[r] = status;
                if (status != CRT_OK) errs[r] = crt_last_error();
                return status == CRT_OK;
            };
            if (hipSetDevice(rk.device) != hipSuccess) { rcs[r] = CRT_ERR_HIP; errs[r] = "hipSetDevice failed"; return; }
            if (!step(crt_render_device(rk.scene, cam, &p, (want & CRT_MULTI_RGB) ? at(P_RGB) : rk.rgb_scratch, at(P_MEAN), rk.stream, &st[r]))) return;
            bool enqueued = false; // work behind the render, which crt_render_device has waited for
            if (want_sums) {
                if (!step(crt_variance_device(rk.scene, at(P_VARIANCE), rk.stream, nullptr))) return;
                enqueued = true;
            }
            if (want_halves) {
                if (!step(crt_half_buffers_device(rk.scene, at(P_HALF_A), at(P_HALF_B), rk.stream, nullptr))) return;
                enqueued = true;
            }
            if (want & (kFirstHitPlanes | kShadingPlanes)) { // ONE trace of the frame's camera rays for all of them
                const crt_aov_buffers first{(float*)at(P_ALBEDO), (float*)at(P_NORMAL), (float*)at(P_DEPTH), (float*)at(P_COVERAGE), (int32_t*)at(P_TRI),
                                            (int32_t*)at(P_MATERIAL)};
                const crt_aov_shading_buffers shading{(float*)at(P_EMISSION), (float*)at(P_DIFFUSE_ALBEDO)};
                const int status = (want & kShadingPlanes)
                                       ? crt_render_aov_shading_device(rk.scene, cam, &p, (want & kFirstHitPlanes) ? &first : nullptr, &shading, rk.stream, nullptr)
                                       : crt_render_aov_device(rk.scene, cam, &p, &first, rk.stream, nullptr);
                if (!step(status)) return;
                enqueued = true;
            }
            if (enqueued && hipStreamSynchronize(rk.stream) != hipSuccess) { rcs[r] = CRT_ERR_HIP; errs[r] = "hipStreamSynchronize failed"; } // (render_ms: until every shard is complete)
        };
        if (world == 1) work(0);
        else {
            std::vector<std::thread> th;
            for (uint32_t r = 0; r < world; r++) th.emplace_back(work, r);
            for (std::thread& t : th) t.join();
        }
        for (uint32_t r = 0; r < world; r++)
            if (rcs[r] != CRT_OK) { drain(); return mfail(rcs[r], who + ": rank " + std::to_string(r) + ": " + errs[r]); }
        const auto t1 = clk::now();
        // ---- one exchange: all-gather of the compact tile blocks ----
        if (m->gather == CRT_GATHER_RCCL) {
            Rccl& R = rccl();
            MNCCL(R.GroupStart());
            for (uint32_t r = 0; r < world; r++) {
                Rank& rk = m->ranks[r];
                MNCCL(R.AllGather(rk.local, rk.gathered, (size_t)stride, ncclUint8, rk.comm, rk.stream));
            }
            MNCCL(R.GroupEnd());
        } else {
            Rank& r0 = m->ranks[0];
            for (uint32_t r = 0; r < world; r++) {
                Rank& rk = m->ranks[r];
                MHIP(hipSetDevice(rk.device));
                if (rk.device == r0.device) MHIP(hipMemcpyAsync(r0.gathered + (uint64_t)r * stride, rk.local, stride, hipMemcpyDeviceToDevice, rk.stream));
                else MHIP(hipMemcpyPeerAsync(r0.gathered + (uint64_t)r * stride, r0.device, rk.local, rk.device, stride, rk.stream));
                if (r > 0) MHIP(hipEventRecord(rk.done, rk.stream));
            }
            MHIP(hipSetDevice(r0.device));
            for (uint32_t r = 1; r < world; r++) MHIP(hipStreamWaitEvent(r0.stream, m->ranks[r].done, 0));
        }
        // ---- rank 0 de-interleaves the tiles of every wanted plane with one launch ----
        crtk::UntileParams U{};
        {
            Rank& r0 = m->ranks[0];
            MHIP(hipSetDevice(r0.device));
            U.gathered = r0.gathered; U.stride = stride; U.world = world; U.width = prm->width; U.height = prm->height;
            U.tiles_x = crtk::untile_tiles_x(prm->width); U.chunks = crtk::untile_chunks(prm->width);
            for (uint32_t k = 0; k < crtk::kUntileMaxPlanes; k++)
                if (want & kPlanes[k].bit) U.plane[U.n_planes++] = crtk::UntilePlane{L.off[k], m->plane[k], kPlanes[k].per_pixel, kPlanes[k].elem};
            const uint64_t grid = crtk::untile_grid(U);
            if (grid > 0x7fffffffull) { drain(); return mfail(CRT_ERR_INVALID_ARG, who + ": the frame is too large for one de-interleave launch"); }
            hipLaunchKernelGGL(crtk::k_untile_planes, dim3((uint32_t)grid), dim3(crtk::kUntileBlock), 0, r0.stream, U);
            MHIP(hipGetLastError());
            for (uint32_t k = 0; k < crtk::kUntileMaxPlanes; k++) // (RGB8: Render.cuh:464)
                if ((want & kPlanes[k].bit) && plane_of(host_out, k)) MHIP(hipMemcpyAsync(plane_of(host_out, k), m->plane[k], plane_bytes(k), hipMemcpyDeviceToHost, r0.stream));
        }
        for (uint32_t r = 0; r < world; r++) {
            MHIP(hipSetDevice(m->ranks[r].device));
            MHIP(hipStreamSynchronize(m->ranks[r].stream));
        }
        const auto t2 = clk::now();
        m->last_want = want;
        m->last_untile = U;
        if (stats) std::memcpy(stats, st.data(), sizeof(crt_stats) * world);
        if (info) {
            std::memset(info, 0, sizeof(*info));
            info->n_ranks = world;
            info->gather = m->gather;
            info->rccl_ranks = m->gather == CRT_GATHER_RCCL ? (uint32_t)m->rccl_ranks : 0u;
            info->rccl_version = m->rccl_version;
            info->render_ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
            info->gather_ms = std::chrono::duration<float, std::milli>(t2 - t1).count();
            info->frame_ms = std::chrono::duration<float, std::milli>(t2 - t0).count();
            info->bytes_per_rank = stride;
            std::snprintf(info->fallback_reason, sizeof(info->fallback_reason), "%s", m->fallback_reason.c_str());
            for (uint32_t r = 0; r < world; r++) {
                info->rays += st[r].rays; info->paths += st[r].paths; info->rays_untraced += st[r].rays_untraced;
                info->max_kernel_ms = std::max(info->max_kernel_ms, st[r].kernel_ms);
            }
        }
        return CRT_OK;
    } catch (const HipErr& f) {
        drain();
        return mfail(CRT_ERR_HIP, who + ": " + f.what + ": " + hipGetErrorString(f.e));
    } catch (const NcclErr& f) {
        drain();
        return mfail(CRT_ERR_HIP, who + ": " + f.what + ": " + rccl().GetErrorString(f.r));
    } catch (const std::bad_alloc&) {
        drain();
        return mfail(CRT_ERR_OOM, who + ": out of host memory");
    }
}

} // namespace

extern "C" {

int crt_multi_render(crt_multi* m, const crt_camera* cam, const crt_params* prm, uint8_t* out_rgb, float* out_mean, crt_stats* stats,
                     crt_multi_info* info)
{
    if (!m || !cam || !prm) return mfail(CRT_ERR_INVALID_ARG, "crt_multi_render: null argument");
    if (prm->width == 0 || prm->height == 0) return mfail(CRT_ERR_INVALID_ARG, "crt_multi_render: width and height must be positive");
    if (out_mean && !out_rgb) return mfail(CRT_ERR_INVALID_ARG, "crt_multi_render: out_mean without out_rgb");
    crt_multi_buffers host{};
    host.rgb = out_rgb; host.mean = out_mean;
    return render_planes("crt_multi_render", m, cam, prm, CRT_MULTI_RGB | (out_mean ? CRT_MULTI_MEAN : 0u), host, stats, info);
}

int crt_multi_render_buffers(crt_multi* m, const crt_camera* cam, const crt_params* prm, uint32_t want, const crt_multi_buffers* host_out, crt_stats* stats,
                             crt_multi_info* info)
{
    if (!m || !cam || !prm) return mfail(CRT_ERR_INVALID_ARG, "crt_multi_render_buffers: null argument");
    if (prm->width == 0 || prm->height == 0) return mfail(CRT_ERR_INVALID_ARG, "crt_multi_render_buffers: width and height must be positive");
    if (want == 0 || (want & ~(uint32_t)CRT_MULTI_ALL)) return mfail(CRT_ERR_INVALID_ARG, "crt_multi_render_buffers: want must name at least one plane and only CRT_MULTI_* bits");
    if ((want & (CRT_MULTI_VARIANCE | CRT_MULTI_HALF_A | CRT_MULTI_HALF_B)) && prm->spp < 2)
        return mfail(CRT_ERR_INVALID_ARG, "crt_multi_render_buffers: the variance and the half planes need spp >= 2");
    const crt_multi_buffers none{};
    return render_planes("crt_multi_render_buffers", m, cam, prm, want, host_out ? *host_out : none, stats, info);
}

int crt_multi_frame_device(crt_multi* m, void** d_rgb, void** d_mean, int* device)
{
    if (!m) return mfail(CRT_ERR_INVALID_ARG, "crt_multi_frame_device: null argument");
    if (d_rgb) *d_rgb = (m->last_want == 0 || (m->last_want & CRT_MULTI_RGB)) ? m->plane[P_RGB] : nullptr;
    if (d_mean) *d_mean = (m->last_want & CRT_MULTI_MEAN) ? m->plane[P_MEAN] : nullptr;
    if (device) *device = m->ranks[0].device;
    return CRT_OK;
}

int crt_multi_untile_time(crt_multi* m, uint32_t calls, float* ms)
{
    if (!m || !ms || calls == 0) return mfail(CRT_ERR_INVALID_ARG, "crt_multi_untile_time: null argument or no calls");
    if (m->last_want == 0) return mfail(CRT_ERR_INVALID_ARG, "crt_multi_untile_time: no frame on the handle");
    DeviceGuard guard;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    try {
        Rank& r0 = m->ranks[0];
        MHIP(hipSetDevice(r0.device));
        MHIP(hipEventCreate(&e0));
        MHIP(hipEventCreate(&e1));
        for (uint32_t c = 0; c < calls; c++) {
            MHIP(hipEventRecord(e0, r0.stream));
            hipLaunchKernelGGL(crtk::k_untile_planes, dim3((uint32_t)crtk::untile_grid(m->last_untile)), dim3(crtk::kUntileBlock), 0, r0.stream, m->last_untile);
            MHIP(hipGetLastError());
            MHIP(hipEventRecord(e1, r0.stream));
            MHIP(hipEventSynchronize(e1));
            MHIP(hipEventElapsedTime(&ms[c], e0, e1));
        }
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        return CRT_OK;
    } catch (const HipErr& f) {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        return mfail(CRT_ERR_HIP, std::string("crt_multi_untile_time: ") + f.what + ": " + hipGetErrorString(f.e));
    }
}

int crt_multi_buffers_device(crt_multi* m, crt_multi_buffers* dev, int* device)
{
    if (!m || !dev) return mfail(CRT_ERR_INVALID_ARG, "crt_multi_buffers_device: null argument");
    void* p[crtk::kUntileMaxPlanes];
    for (uint32_t k = 0; k < crtk::kUntileMaxPlanes; k++) p[k] = (m->last_want & kPlanes[k].bit) ? m->plane[k] : nullptr;
    *dev = buffers_of(p);
    if (device) *device = m->ranks[0].device;
    return CRT_OK;
}

} // extern "C"
