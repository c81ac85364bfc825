// cudaraytracing_amd/csrc/crt_aov_pass.hip -- the host side of crt_aov.hip, crt_aov_direct.hip and crt_aov_ao.hip: the AOV passes (first hit, shading, mirror bounces, direct light,
// ambient occlusion) and their entry points in the C ABI of include/crt.h (crt_render_aov*, crt_aov_specular_defaults, crt_aov_ao_defaults).  Every pass is the camera rays of samples
// 0 .. spp-1 of every pixel slot of the shard, in chunks of whole samples of at most kAovChunkRays rays (32 B of query pool + 16 B of
// results per ray: 1.6 GB), each traced by trace_queries (crt_render.hip, through crt_render.h) and folded into the per-slot running sums
// in sample order.  Uses the handle's query pool and trace buffers, as crt_intersect does; the accumulator of a progressive render
// (accum, acc) is not touched.  What the passes share is stated once: aov_check, aov_pass, aov_host_form.
#include "crt_render.h"

#include "crt_aov_direct.h"
#include "crt_aov_ao.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

using namespace crtk;

namespace {

const uint32_t kAovChunkRays = 1u << 25;

bool any_buffer(const crt_aov_buffers* o) { return o && (o->albedo || o->normal || o->depth || o->coverage || o->tri || o->material); }
bool any_buffer(const crt_aov_shading_buffers* o) { return o && (o->emission || o->diffuse_albedo); }
bool any_buffer(const crt_aov_specular_buffers* o) { return o && (o->guide_albedo || o->last_normal || o->path_depth || o->bounces || o->last_tri); }
bool any_buffer(const crt_aov_direct_buffers* o) { return o && (o->direct || o->unshadowed || o->direct_variance || o->visibility); }
bool any_buffer(const crt_aov_ao_buffers* o) { return o && (o->ao || o->openness || o->bent_normal); }

// The argument check of all ten entry points (`who`: the entry's base name), before any device call.  missing: a pointer its form requires
// is null; unnamed: what to say when its structs name no output buffer (null: they name one); sp: the specular form's settings;
// camera_rays_only: false for the direct-light pass, which takes next-event samples and checks light_sample_n as a render does; ao: the
// ambient-occlusion form's settings.
int aov_check(const char* who, const crt_scene* sc, const crt_camera* cam, const crt_params* prm, bool missing, const char* unnamed,
              const crt_aov_specular_params* sp = nullptr, bool camera_rays_only = true, const crt_aov_ao_params* ao = nullptr)
{
    const std::string w(who);
    if (!sc || !cam || !prm || missing) return fail(CRT_ERR_INVALID_ARG, w + ": null argument");
    if (unnamed) return fail(CRT_ERR_INVALID_ARG, w + ": " + unnamed);
    if (sp && (sp->max_bounces < 1 || sp->max_bounces > 8)) return fail(CRT_ERR_INVALID_ARG, w + ": max_bounces must be in [1, 8]");
    if (ao && (ao->ao_samples < 1 || ao->ao_samples > 256)) return fail(CRT_ERR_INVALID_ARG, w + ": ao_samples must be in [1, 256]");
    if (ao && !(ao->max_distance > 0.0f && ao->max_distance <= FLT_MAX)) // (a NaN fails the first comparison)
        return fail(CRT_ERR_INVALID_ARG, w + ": max_distance must be finite and > 0");
    const int rc = params_check(who, prm, camera_rays_only);
    if (rc != CRT_OK) return rc;
    if ((uint64_t)make_shard(prm->width, prm->height, prm->world).local_tiles * 64u > 0x7fffffffull)
        return fail(CRT_ERR_UNSUPPORTED, w + ": more than 2^31 pixel slots in a shard");
    if (ao && (uint64_t)prm->spp * ao->ao_samples > 0xffffffffull) return fail(CRT_ERR_UNSUPPORTED, w + ": more than 2^32 occlusion rays per pixel");
    return CRT_OK;
}
// crt_render_aov_shading: `first` may be null (a struct that is given must name a buffer, as crt_render_aov's), `shading` not
const char* shading_unnamed(const crt_aov_buffers* first, const crt_aov_shading_buffers* shading)
{
    if (!any_buffer(shading)) return "no output buffer in shading";
    return first && !any_buffer(first) ? "no output buffer in first (pass NULL for none)" : nullptr;
}

// A pass on device buffers; the entry point has checked the arguments.  reserve(max_rays, A): every buffer of the pass -- the query pool
// among them -- at the size the largest chunk needs, and the pass's own fields of A (zeroed but for its slot map).  chunk(A): what the
// pass does with the answers of a chunk's camera rays (A.res, A.res_stride; A.pool.n of them), enqueued on st; returns the further rays
// it traced.
template <class Reserve, class Chunk>
int aov_pass(crt_scene* sc, const crt_camera* cam, const crt_params* prm, hipStream_t st, crt_aov_info* info, Reserve reserve, Chunk chunk)
{
    const bool tiled = (prm->flags & CRT_FLAG_TILED_OUTPUT) != 0;
    const Shard sh = make_shard(prm->width, prm->height, prm->world);
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        const uint32_t chunk_spp = std::min<uint32_t>(prm->spp, std::max<uint32_t>(1u, kAovChunkRays / sh.nslots));
        AovParams A;
        std::memset(&A, 0, sizeof(A));
        fill_slot_map(A, *prm, tiled, sh);
        reserve((uint64_t)chunk_spp * sh.nslots, A);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (info) {
            ensure_events(sc);
            e0 = sc->ev[0]; e1 = sc->ev[1];
            HIP_CHECK(hipEventRecord(e0, st));
        }
        std::memcpy(A.eye, cam->eye, sizeof(A.eye));
        std::memcpy(A.inv_view, cam->inv_view, sizeof(A.inv_view));
        camera_scale_ar(cam, prm, A.scale, A.ar);
        A.seed = prm->seed; A.spp = prm->spp;
        A.pool.ro = sc->p_ro.p; A.pool.rd = sc->p_rd.p; A.pool.res = sc->p_res.p;
        const bool force_exact = (prm->flags & CRT_FLAG_FORCE_EXACT) != 0;
        uint64_t rays = 0;
        uint32_t chunks = 0;
        for (uint32_t s0 = 0; s0 < prm->spp; s0 += chunk_spp) {
            const uint32_t ns = std::min(chunk_spp, prm->spp - s0);
            A.sample_begin = s0; A.n_samples = ns; A.pool.n = ns * sh.nslots;
            A.first_chunk = s0 == 0; A.last_chunk = s0 + ns == prm->spp;
            launch_aov_rays(A, st);
            HIP_CHECK(hipGetLastError());
            A.res = trace_queries(sc, A.pool.n, prm->traversal, force_exact, st, A.res_stride);
            rays += A.pool.n + chunk(A);
            HIP_CHECK(hipGetLastError());
            chunks++;
        }
        if (info) {
            HIP_CHECK(hipEventRecord(e1, st));
            HIP_CHECK(hipStreamSynchronize(st));
            std::memset(info, 0, sizeof(*info));
            info->rays = rays; info->chunks = chunks;
            HIP_CHECK(hipEventElapsedTime(&info->total_ms, e0, e1));
        }
        return CRT_OK;
    });
}

// crt_render_aov (shading null) and crt_render_aov_shading: k_aov_resolve folds a chunk's first hits.  With shading -- out may then be
// null -- the resolve's shading form writes both structs from the one trace and a slot has four accumulator rows.
int first_hit_pass(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_aov_buffers* out, const crt_aov_shading_buffers* shading,
                   hipStream_t st, crt_aov_info* info)
{
    return aov_pass(sc, cam, prm, st, info,
        [&](uint64_t max_rays, AovParams& A) {
            sc->p_ro.ensure(max_rays); sc->p_rd.ensure(max_rays); sc->p_res.ensure(max_rays);
            sc->aov_acc.ensure((size_t)A.nslots * (shading ? kAovAccRowsShading : kAovAccRows));
            A.tri_nm = sc->dev.tri_nm; A.mats = sc->dev.mats; A.acc = sc->aov_acc.p;
            if (!out) return;
            A.albedo = out->albedo; A.normal = out->normal; A.depth = out->depth; A.coverage = out->coverage; A.tri = out->tri; A.material = out->material;
        },
        [&](AovParams& A) -> uint64_t {
            if (shading) launch_aov_resolve_shading(A, AovShadingOut{shading->emission, shading->diffuse_albedo}, st);
            else launch_aov_resolve(A, st);
            return 0;
        });
}

// crt_render_aov_specular, the pass that follows mirror bounces.  After a chunk's camera rays are traced, k_aov_bounce advances every
// item's chain and compacts the reflected rays into the other half of the query pool (the halves alternate from bounce to bounce: a stage
// never writes the rays or answers another of its threads still reads); the host reads their count -- one 4-byte copy into pinned memory
// and one synchronization per bounce and chunk -- traces that many and runs the next stage on their answers.  A count of 0 ends the
// chunk's bounces; the stage after the last bounce allowed has nothing to compact and needs no count.
int specular_pass(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_aov_specular_params* sp, const crt_aov_specular_buffers* out,
                  hipStream_t st, crt_aov_info* info)
{
    AovSpecParams S;
    std::memset(&S, 0, sizeof(S));
    size_t half = 0; // of the query pool: the rays of the largest chunk
    return aov_pass(sc, cam, prm, st, info,
        [&](uint64_t max_rays, AovParams& A) {
            // every buffer at its final size before the first launch: growing one later would drop what a stage has left in it
            sc->p_ro.ensure(2 * max_rays); sc->p_rd.ensure(2 * max_rays); sc->p_res.ensure(2 * max_rays); sc->aovs_item.ensure(2 * max_rays);
            sc->aovs_state.ensure(max_rays); sc->aovs_aux.ensure(max_rays);
            if (choose_pipeline(sc) == 4) (void)sc->L.answers(max_rays);
            sc->aov_acc.ensure((size_t)A.nslots * kAovAccRows);
            sc->aovs_count.ensure_uncached(1);
            if (!sc->h_aovs_count) HIP_CHECK(hipHostMalloc((void**)&sc->h_aovs_count, sizeof(unsigned int), hipHostMallocDefault));
            half = max_rays;
            S.max_bounces = sp->max_bounces;
            S.count = sc->aovs_count.p; S.state = sc->aovs_state.p; S.aux = sc->aovs_aux.p;
            S.tri_nm = sc->dev.tri_nm; S.mats = sc->dev.mats; S.acc = sc->aov_acc.p;
            S.guide_albedo = out->guide_albedo; S.last_normal = out->last_normal; S.path_depth = out->path_depth; S.bounces = out->bounces; S.last_tri = out->last_tri;
        },
        [&](AovParams& A) -> uint64_t {
            static_cast<SlotMap&>(S) = A;
            S.spp = A.spp; S.n_samples = A.n_samples; S.first_chunk = A.first_chunk; S.last_chunk = A.last_chunk;
            S.res = A.res; S.res_stride = A.res_stride;
            const bool force_exact = (prm->flags & CRT_FLAG_FORCE_EXACT) != 0;
            uint64_t rays = 0;
            size_t in = 0, outh = half; // where in the pool the rays traced last are, and where those that go on are put
            uint32_t n_in = A.pool.n;
            for (uint32_t stage = 0; n_in > 0; stage++) {
                S.stage0 = stage == 0; S.n_in = n_in;
                S.in_ro = sc->p_ro.p + in; S.in_rd = sc->p_rd.p + in; S.in_item = sc->aovs_item.p + in;
                S.out_ro = sc->p_ro.p + outh; S.out_rd = sc->p_rd.p + outh; S.out_res = sc->p_res.p + outh; S.out_item = sc->aovs_item.p + outh;
                HIP_CHECK(hipMemsetAsync(sc->aovs_count.p, 0, sizeof(unsigned int), st));
                launch_aov_bounce(S, st);
                HIP_CHECK(hipGetLastError());
                if (stage == sp->max_bounces) break; // (every chain that came this far is at the cap)
                HIP_CHECK(hipMemcpyAsync(sc->h_aovs_count, sc->aovs_count.p, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipStreamSynchronize(st)); // the one synchronization of a bounce: how many rays go on
                n_in = std::min<uint32_t>(*sc->h_aovs_count, n_in);
                if (n_in == 0) break;
                S.res = trace_queries(sc, n_in, prm->traversal, force_exact, st, S.res_stride, outh);
                rays += n_in;
                std::swap(in, outh);
            }
            launch_aov_spec_resolve(S, st);
            return rays;
        });
}

// crt_render_aov_direct: the first-vertex next-event term of the frame's own paths (kernels: crt_aov_direct.hip).  After a chunk's
// camera rays are traced, k_aov_direct_vertex copies what the later stages need out of their answers -- on the megakernel pipeline
// trace_queries returns the handle's one answer array, which the next trace overwrites.  The chunk's (sample, q) entries are then walked in
// sub-batches of at most kAovChunkRays plane entries (CRT_AOV_DIRECT_BATCH: a test's smaller number): the set-up kernel writes the
// contributions and compacts the traced shadow rays into the query pool behind the camera rays, the host reads their count -- one 4-byte
// copy into pinned memory and one synchronization per sub-batch, as the specular pass per bounce --, traces that many, the answer kernel
// clears the blocked flags and the resolve folds the sub-batch into the slots' running sums.  batches: the sub-batches of the call.
int direct_pass(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_aov_direct_buffers* out, hipStream_t st, crt_aov_info* info)
{
    if ((uint64_t)sc->dev.n_lights * (uint64_t)prm->light_sample_n > 0xffffu) // (as crt_render)
        return fail(CRT_ERR_UNSUPPORTED, "crt_render_aov_direct: more than 65535 next-event samples per vertex");
    AovDirectParams D;
    std::memset(&D, 0, sizeof(D));
    const uint32_t n_q = (uint32_t)sc->dev.n_lights * (uint32_t)prm->light_sample_n;
    size_t second = 0;        // where in the query pool the shadow rays go: behind the camera rays of the largest chunk
    uint64_t batch_pairs = 1; // (sample, q) entries of a sub-batch
    uint32_t batches = 0;
    const int rc = aov_pass(sc, cam, prm, st, info,
        [&](uint64_t max_rays, AovParams& A) {
            batch_pairs = std::max<uint64_t>(1, env_u32("CRT_AOV_DIRECT_BATCH", kAovChunkRays) / A.nslots);
            batch_pairs = std::min<uint64_t>(batch_pairs, std::max<uint64_t>(1, max_rays / A.nslots * n_q)); // (no more than a chunk has)
            const uint64_t cap = batch_pairs * A.nslots;
            // every buffer at its final size before the first launch: growing one later would drop what a stage has left in it
            sc->p_ro.ensure(max_rays + cap); sc->p_rd.ensure(max_rays + cap); sc->p_res.ensure(max_rays + cap);
            sc->aovs_item.ensure(cap); sc->aovd_plane.ensure(cap); sc->aovd_vert.ensure(max_rays);
            if (choose_pipeline(sc) == 4) (void)sc->L.answers(std::max(max_rays, cap));
            sc->aov_acc.ensure((size_t)A.nslots * kAovDirectAccRows);
            sc->aovs_count.ensure_uncached(1);
            if (!sc->h_aovs_count) HIP_CHECK(hipHostMalloc((void**)&sc->h_aovs_count, sizeof(unsigned int), hipHostMallocDefault));
            second = max_rays;
            D.seed = prm->seed; D.spp = prm->spp;
            D.tri_nm = sc->dev.tri_nm; D.mats = sc->dev.mats; D.ltri = sc->dev.ltri; D.lights = sc->dev.lights;
            D.n_q = n_q; D.lsn = prm->light_sample_n; D.inv_lsn_pow2 = inv_if_pow2(prm->light_sample_n);
            D.lsn_div = make_fastdiv((uint32_t)std::max(1, prm->light_sample_n));
            D.reference_mode = prm->traversal == CRT_TRAVERSAL_REFERENCE ? 1u : 0u;
            D.vert = sc->aovd_vert.p; D.plane = sc->aovd_plane.p; D.count = sc->aovs_count.p; D.acc = sc->aov_acc.p;
            D.out_ro = sc->p_ro.p + second; D.out_rd = sc->p_rd.p + second; D.out_res = sc->p_res.p + second; D.out_idx = sc->aovs_item.p;
            D.direct = out->direct; D.unshadowed = out->unshadowed; D.direct_variance = out->direct_variance; D.visibility = out->visibility;
        },
        [&](AovParams& A) -> uint64_t {
            static_cast<SlotMap&>(D) = A;
            D.sample_begin = A.sample_begin; D.n_samples = A.n_samples;
            D.cam_ro = A.pool.ro; D.cam_rd = A.pool.rd; D.res = A.res; D.res_stride = A.res_stride;
            const bool force_exact = (prm->flags & CRT_FLAG_FORCE_EXACT) != 0;
            const uint64_t total = (uint64_t)A.n_samples * n_q;
            uint64_t rays = 0;
            if (total == 0) { // no next-event samples: the last chunk writes the outputs of sums that never started
                if (!A.last_chunk) return 0;
                D.s_first = D.q_first = D.e_count = 0; D.first_batch = D.last_batch = 1;
                launch_aov_direct_resolve(D, st);
                batches++;
                return 0;
            }
            launch_aov_direct_vertex(D, st); // (before the first shadow trace: it overwrites the camera answers)
            HIP_CHECK(hipGetLastError());
            for (uint64_t e0 = 0; e0 < total; e0 += batch_pairs) {
                const uint32_t cnt = (uint32_t)std::min<uint64_t>(batch_pairs, total - e0);
                D.s_first = (uint32_t)(e0 / n_q); D.q_first = (uint32_t)(e0 % n_q); D.e_count = cnt;
                D.first_batch = A.first_chunk && e0 == 0; D.last_batch = A.last_chunk && e0 + cnt == total;
                HIP_CHECK(hipMemsetAsync(sc->aovs_count.p, 0, sizeof(unsigned int), st));
                launch_aov_direct_setup(D, st);
                HIP_CHECK(hipGetLastError());
                HIP_CHECK(hipMemcpyAsync(sc->h_aovs_count, sc->aovs_count.p, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipStreamSynchronize(st)); // the one synchronization of a sub-batch: how many shadow rays are traced
                const uint32_t n = (uint32_t)std::min<uint64_t>(*sc->h_aovs_count, (uint64_t)cnt * A.nslots);
                if (n > 0) {
                    D.ans = trace_queries(sc, n, prm->traversal, force_exact, st, D.ans_stride, second);
                    D.n_traced = n;
                    launch_aov_direct_answer(D, st);
                    HIP_CHECK(hipGetLastError());
                    rays += n;
                }
                launch_aov_direct_resolve(D, st);
                HIP_CHECK(hipGetLastError());
                batches++;
            }
            return rays;
        });
    if (rc == CRT_OK && info) info->chunks = batches;
    return rc;
}

// crt_render_aov_ao: occlusion rays over the hemisphere of the first hit (kernels: crt_aov_ao.hip).  After a chunk's camera rays are
// traced, k_aov_ao_vertex copies what the later stages need out of their answers (as the direct-light pass: the next trace overwrites
// them).  The chunk's (sample, q) entries are then walked in sub-batches of at most kAovChunkRays plane entries (CRT_AOV_AO_BATCH: a
// test's smaller number): the set-up kernel writes every entry's direction and cosine and its ray into the query pool behind the camera
// rays, at the entry's own index; all of them are traced, and the resolve folds entries and answers into the slots' running sums.
// Every ray is traced, so the host knows each launch's size and reads nothing back: the pass only enqueues (a buffer that has to grow
// is freed first, which waits for the device).  The sum of the occlusion rays of the call stays on the device unless info is asked for.
int ao_pass(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_aov_ao_params* ap, const crt_aov_ao_buffers* out, hipStream_t st,
            crt_aov_info* info)
{
    AovAoParams D;
    std::memset(&D, 0, sizeof(D));
    const uint32_t n_q = ap->ao_samples;
    size_t second = 0;        // where in the query pool the occlusion rays go: behind the camera rays of the largest chunk
    uint64_t batch_pairs = 1; // (sample, q) entries of a sub-batch
    uint32_t batches = 0;
    const int rc = aov_pass(sc, cam, prm, st, info,
        [&](uint64_t max_rays, AovParams& A) {
            batch_pairs = std::max<uint64_t>(1, env_u32("CRT_AOV_AO_BATCH", kAovChunkRays) / A.nslots);
            batch_pairs = std::min<uint64_t>(batch_pairs, std::max<uint64_t>(1, max_rays / A.nslots * n_q)); // (no more than a chunk has)
            const uint64_t cap = batch_pairs * A.nslots;
            // every buffer at its final size before the first launch: growing one later would drop what a stage has left in it
            sc->p_ro.ensure(max_rays + cap); sc->p_rd.ensure(max_rays + cap); sc->p_res.ensure(max_rays + cap);
            sc->aovd_plane.ensure(cap); sc->aovd_vert.ensure(2 * max_rays);
            if (choose_pipeline(sc) == 4) (void)sc->L.answers(std::max(max_rays, cap));
            sc->aov_acc.ensure((size_t)A.nslots * kAovAoAccRows);
            sc->aovao_rays.ensure(1);
            HIP_CHECK(hipMemsetAsync(sc->aovao_rays.p, 0, sizeof(unsigned long long), st));
            second = max_rays;
            D.seed = prm->seed; D.spp = prm->spp;
            D.n_q = n_q; D.max_distance = ap->max_distance;
            D.reference_mode = prm->traversal == CRT_TRAVERSAL_REFERENCE ? 1u : 0u;
            D.tri_nm = sc->dev.tri_nm;
            D.vert = sc->aovd_vert.p; D.vnf = sc->aovd_vert.p + max_rays; D.plane = sc->aovd_plane.p; D.acc = sc->aov_acc.p;
            D.out_ro = sc->p_ro.p + second; D.out_rd = sc->p_rd.p + second; D.out_res = sc->p_res.p + second;
            D.ray_total = sc->aovao_rays.p;
            D.ao = out->ao; D.openness = out->openness; D.bent_normal = out->bent_normal;
        },
        [&](AovParams& A) -> uint64_t {
            static_cast<SlotMap&>(D) = A;
            D.sample_begin = A.sample_begin; D.n_samples = A.n_samples;
            D.cam_ro = A.pool.ro; D.cam_rd = A.pool.rd; D.res = A.res; D.res_stride = A.res_stride;
            const bool force_exact = (prm->flags & CRT_FLAG_FORCE_EXACT) != 0;
            const uint64_t total = (uint64_t)A.n_samples * n_q;
            launch_aov_ao_vertex(D, st); // (before the first occlusion trace: it overwrites the camera answers)
            HIP_CHECK(hipGetLastError());
            for (uint64_t e0 = 0; e0 < total; e0 += batch_pairs) {
                const uint32_t cnt = (uint32_t)std::min<uint64_t>(batch_pairs, total - e0);
                D.s_first = (uint32_t)(e0 / n_q); D.q_first = (uint32_t)(e0 % n_q); D.e_count = cnt;
                D.first_batch = A.first_chunk && e0 == 0; D.last_batch = A.last_chunk && e0 + cnt == total;
                launch_aov_ao_setup(D, st);
                HIP_CHECK(hipGetLastError());
                D.ans = trace_queries(sc, cnt * A.nslots, prm->traversal, force_exact, st, D.ans_stride, second);
                launch_aov_ao_resolve(D, st);
                HIP_CHECK(hipGetLastError());
                batches++;
            }
            return 0; // (the occlusion rays with a vertex are counted on the device)
        });
    if (rc != CRT_OK || !info) return rc;
    return hip_guard([&]() -> int {
        unsigned long long n = 0;
        HIP_CHECK(hipMemcpy(&n, sc->aovao_rays.p, sizeof(n), hipMemcpyDeviceToHost)); // (aov_pass has synchronized the stream for the info)
        info->rays += n; info->chunks = batches;
        return CRT_OK;
    });
}

// The host-buffer form of an entry: a device buffer for every plane whose host pointer is given, the pass on them (pass(d): d[i] the
// device pointer of plane i, null where the host's is), then a synchronization and the copies back.
struct HostPlane {
    void* host;
    uint32_t values; // 4-byte values per pixel
};
template <class Pass> int aov_host_form(crt_scene* sc, const crt_params* prm, std::initializer_list<HostPlane> planes, Pass pass)
{
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        const uint64_t npix = out_pixels(prm->width, prm->height, prm->world, (prm->flags & CRT_FLAG_TILED_OUTPUT) != 0);
        std::vector<DevBuf<float>> buf(planes.size());
        std::vector<float*> d;
        for (const HostPlane& pl : planes) {
            if (pl.host) buf[d.size()].alloc(npix * pl.values);
            d.push_back(buf[d.size()].p);
        }
        const int rc = pass(d.data());
        if (rc != CRT_OK) return rc;
        HIP_CHECK(hipDeviceSynchronize());
        size_t i = 0;
        for (const HostPlane& pl : planes) buf[i++].download((float*)pl.host, npix * pl.values);
        return CRT_OK;
    });
}

} // namespace

extern "C" {

int crt_render_aov_device(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_aov_buffers* dev_out, void* stream, crt_aov_info* info)
{
    const int rc = aov_check("crt_render_aov", sc, cam, prm, !dev_out, any_buffer(dev_out) ? nullptr : "no output buffer");
    if (rc != CRT_OK) return rc;
    return first_hit_pass(sc, cam, prm, dev_out, nullptr, (hipStream_t)stream, info);
}

int crt_render_aov(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_aov_buffers* host_out, crt_aov_info* info)
{
    const int rc = aov_check("crt_render_aov", sc, cam, prm, !host_out, any_buffer(host_out) ? nullptr : "no output buffer");
    if (rc != CRT_OK) return rc;
    const crt_aov_buffers& h = *host_out;
    return aov_host_form(sc, prm, {{h.albedo, 3}, {h.normal, 3}, {h.depth, 1}, {h.coverage, 1}, {h.tri, 1}, {h.material, 1}}, [&](float* const* d) {
        const crt_aov_buffers dev{d[0], d[1], d[2], d[3], (int32_t*)d[4], (int32_t*)d[5]};
        return first_hit_pass(sc, cam, prm, &dev, nullptr, nullptr, info);
    });
}

int crt_render_aov_shading_device(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_aov_buffers* dev_first,
                                  const crt_aov_shading_buffers* dev_shading, void* stream, crt_aov_info* info)
{
    const int rc = aov_check("crt_render_aov_shading", sc, cam, prm, !dev_shading, shading_unnamed(dev_first, dev_shading));
    if (rc != CRT_OK) return rc;
    return first_hit_pass(sc, cam, prm, dev_first, dev_shading, (hipStream_t)stream, info);
}

int crt_render_aov_shading(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_aov_buffers* host_first,
                           const crt_aov_shading_buffers* host_shading, crt_aov_info* info)
{
    const int rc = aov_check("crt_render_aov_shading", sc, cam, prm, !host_shading, shading_unnamed(host_first, host_shading));
    if (rc != CRT_OK) return rc;
    const crt_aov_buffers none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const crt_aov_buffers& h = host_first ? *host_first : none;
    const crt_aov_shading_buffers& hs = *host_shading;
    return aov_host_form(sc, prm, {{h.albedo, 3}, {h.normal, 3}, {h.depth, 1}, {h.coverage, 1}, {h.tri, 1}, {h.material, 1}, {hs.emission, 3}, {hs.diffuse_albedo, 3}},
                         [&](float* const* d) {
        const crt_aov_buffers dev{d[0], d[1], d[2], d[3], (int32_t*)d[4], (int32_t*)d[5]};
        const crt_aov_shading_buffers dev_shading{d[6], d[7]};
        return first_hit_pass(sc, cam, prm, host_first ? &dev : nullptr, &dev_shading, nullptr, info);
    });
}

int crt_aov_specular_defaults(crt_aov_specular_params* p)
{
    if (!p) return fail(CRT_ERR_INVALID_ARG, "crt_aov_specular_defaults: null argument");
    p->max_bounces = 2;
    return CRT_OK;
}

int crt_render_aov_specular_device(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_aov_specular_params* sp,
                                   const crt_aov_specular_buffers* dev_out, void* stream, crt_aov_info* info)
{
    const int rc = aov_check("crt_render_aov_specular", sc, cam, prm, !sp || !dev_out, any_buffer(dev_out) ? nullptr : "no output buffer", sp);
    if (rc != CRT_OK) return rc;
    return specular_pass(sc, cam, prm, sp, dev_out, (hipStream_t)stream, info);
}

int crt_render_aov_specular(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_aov_specular_params* sp,
                            const crt_aov_specular_buffers* host_out, crt_aov_info* info)
{
    const int rc = aov_check("crt_render_aov_specular", sc, cam, prm, !sp || !host_out, any_buffer(host_out) ? nullptr : "no output buffer", sp);
    if (rc != CRT_OK) return rc;
    const crt_aov_specular_buffers& h = *host_out;
    return aov_host_form(sc, prm, {{h.guide_albedo, 3}, {h.last_normal, 3}, {h.path_depth, 1}, {h.bounces, 1}, {h.last_tri, 1}}, [&](float* const* d) {
        const crt_aov_specular_buffers dev{d[0], d[1], d[2], d[3], (int32_t*)d[4]};
        return specular_pass(sc, cam, prm, sp, &dev, nullptr, info);
    });
}

int crt_render_aov_direct_device(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_aov_direct_buffers* dev_out, void* stream,
                                 crt_aov_info* info)
{
    const int rc = aov_check("crt_render_aov_direct", sc, cam, prm, !dev_out, any_buffer(dev_out) ? nullptr : "no output buffer", nullptr, false);
    if (rc != CRT_OK) return rc;
    return direct_pass(sc, cam, prm, dev_out, (hipStream_t)stream, info);
}

int crt_render_aov_direct(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_aov_direct_buffers* host_out, crt_aov_info* info)
{
    const int rc = aov_check("crt_render_aov_direct", sc, cam, prm, !host_out, any_buffer(host_out) ? nullptr : "no output buffer", nullptr, false);
    if (rc != CRT_OK) return rc;
    const crt_aov_direct_buffers& h = *host_out;
    return aov_host_form(sc, prm, {{h.direct, 3}, {h.unshadowed, 3}, {h.direct_variance, 3}, {h.visibility, 1}}, [&](float* const* d) {
        const crt_aov_direct_buffers dev{d[0], d[1], d[2], d[3]};
        return direct_pass(sc, cam, prm, &dev, nullptr, info);
    });
}

int crt_aov_ao_defaults(const crt_scene* sc, crt_aov_ao_params* p)
{
    if (!sc || !p) return fail(CRT_ERR_INVALID_ARG, "crt_aov_ao_defaults: null argument");
    double d2 = 0.0;
    for (int a = 0; a < 3; a++) d2 += ((double)sc->root_bb[a] - (double)sc->root_aa[a]) * ((double)sc->root_bb[a] - (double)sc->root_aa[a]);
    const float quarter = (float)(0.25 * std::sqrt(d2));
    p->ao_samples = 4;
    p->max_distance = (quarter > 0.0f && quarter <= FLT_MAX) ? quarter : 1.0f; // (a root box that is a point, or not finite)
    return CRT_OK;
}

int crt_render_aov_ao_device(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_aov_ao_params* ao, const crt_aov_ao_buffers* dev_out,
                             void* stream, crt_aov_info* info)
{
    const int rc = aov_check("crt_render_aov_ao", sc, cam, prm, !ao || !dev_out, any_buffer(dev_out) ? nullptr : "no output buffer", nullptr, true, ao);
    if (rc != CRT_OK) return rc;
    return ao_pass(sc, cam, prm, ao, dev_out, (hipStream_t)stream, info);
}

int crt_render_aov_ao(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_aov_ao_params* ao, const crt_aov_ao_buffers* host_out,
                      crt_aov_info* info)
{
    const int rc = aov_check("crt_render_aov_ao", sc, cam, prm, !ao || !host_out, any_buffer(host_out) ? nullptr : "no output buffer", nullptr, true, ao);
    if (rc != CRT_OK) return rc;
    const crt_aov_ao_buffers& h = *host_out;
    return aov_host_form(sc, prm, {{h.ao, 1}, {h.openness, 1}, {h.bent_normal, 3}}, [&](float* const* d) {
        const crt_aov_ao_buffers dev{d[0], d[1], d[2]};
        return ao_pass(sc, cam, prm, ao, &dev, nullptr, info);
    });
}

} // extern "C"
