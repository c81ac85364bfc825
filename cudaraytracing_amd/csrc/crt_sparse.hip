// cudaraytracing_amd/csrc/crt_sparse.hip -- the host side of the frames in which not every pixel takes every sample, and their entry
// points in the C ABI of include/crt.h: crt_render_adaptive* (passes over the pixels a selection kernel leaves active), crt_render_map*
// (per-pixel sample counts in one launch per chunk), crt_sample_plan* and crt_render_planned*.  Each is ranges of render_impl
// (crt_render.hip, through crt_render.h) with the variance sums; a range that not every slot takes whole carries an item source -- the
// compacted active list or the sample map -- which sizes, lists and folds its chunks.  The kernels: crt_adaptive.hip, crt_sample_map.hip.
#include "crt_render.h"

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <string>
#include <vector>

using namespace crtk;

namespace {

enum Call { ADAPTIVE, MAP, PLANNED };
const char* const kCallName[] = {"crt_render_adaptive", "crt_render_map", "crt_render_planned"};
const uint32_t kMaxMapSpp = 1u << 24; // (the histogram and the cursors: 8 B per sample of the cap on the device, as much pinned)

int threshold_check(const char* who, float threshold, float mean_floor)
{
    if (!(threshold >= 0.0f)) return fail(CRT_ERR_INVALID_ARG, std::string(who) + ": threshold must be >= 0 and not NaN");
    if (!(mean_floor >= 0.0f) || mean_floor > FLT_MAX) return fail(CRT_ERR_INVALID_ARG, std::string(who) + ": mean_floor must be >= 0 and finite");
    return CRT_OK;
}

// Argument checks of both forms of the three calls, before any device call: ap is crt_render_adaptive's and crt_render_planned's, map
// and s_begin are crt_render_map's.  The scene comes last so that the message names what is wrong with the other arguments even where
// there is no scene.
int sparse_check(Call call, const crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_adaptive_params* ap, const void* map, uint32_t s_begin,
                 const void* out_rgb, const void* out_mean)
{
    const char* who = kCallName[call];
    const std::string w(who);
    if (!cam) return fail(CRT_ERR_INVALID_ARG, w + ": null camera");
    if (!prm) return fail(CRT_ERR_INVALID_ARG, w + ": null params");
    if (call != MAP && !ap) return fail(CRT_ERR_INVALID_ARG, w + ": null adaptive params");
    if (call == MAP && !map) return fail(CRT_ERR_INVALID_ARG, w + ": null sample map");
    if (!out_rgb && !out_mean) return fail(CRT_ERR_INVALID_ARG, w + ": out_rgb and out_mean are both null");
    if (call != MAP) {
        if (ap->min_samples < 2 || ap->min_samples > prm->spp) return fail(CRT_ERR_INVALID_ARG, w + ": min_samples must be in [2, spp] (the variance needs two samples)");
        if (call == ADAPTIVE && ap->step_samples == 0) return fail(CRT_ERR_INVALID_ARG, w + ": step_samples must be positive");
        const int rc = threshold_check(who, ap->threshold, ap->mean_floor);
        if (rc != CRT_OK) return rc;
    }
    const int rc = params_check("crt_render", prm);
    if (rc != CRT_OK) return rc;
    if (call == MAP && s_begin >= prm->spp) return fail(CRT_ERR_INVALID_ARG, w + ": sample_begin must be below spp");
    if (call != ADAPTIVE) {
        if (prm->spp > kMaxMapSpp) return fail(CRT_ERR_UNSUPPORTED, w + ": spp above 2^24");
        if ((uint64_t)make_shard(prm->width, prm->height, prm->world).local_tiles * 64u > kMaxChunkItems) return fail(CRT_ERR_UNSUPPORTED, w + ": more than 2^30 pixel slots in a shard");
    }
    if (!sc) return fail(CRT_ERR_INVALID_ARG, w + ": null scene");
    if (choose_pipeline(sc) != 4) return fail(CRT_ERR_UNSUPPORTED, w + ": the fallback pipeline hands out its work items without the item list");
    if (call == MAP && s_begin > 0) {
        const bool tiled = (prm->flags & CRT_FLAG_TILED_OUTPUT) != 0;
        if (!continues_frame(sc->acc, prm, s_begin, tiled) || !sc->var.valid || !continues_frame(sc->var, prm, s_begin, tiled))
            return fail(CRT_ERR_INVALID_ARG, w + ": sample_begin " + std::to_string(s_begin) + " must continue the frame in flight: exactly samples [0, sample_begin) of every pixel "
                                             "with CRT_FLAG_VARIANCE from sample 0 on, and the same spp, width, height, rank, world and CRT_FLAG_TILED_OUTPUT (" +
                                             sc->acc.in_flight(std::string(sc->var.valid ? ", with" : ", without") + " valid variance sums") + ")");
    }
    return CRT_OK;
}

// Pixels of the shard (its pixel slots without the padding of ragged tiles and of tiles beyond the frame)
uint64_t shard_pixels(const SlotMap& m)
{
    uint64_t n = 0;
    for (uint32_t lt = 0; lt < m.nslots / 64u; lt++) n += tile_pixels(m, lt);
    return n;
}

// What the device forms share: the frame's ranges are rendered with the variance sums, without counters and without the commit ring;
// whatever happens from the constructor on, no frame is in flight on the handle afterwards (the sums are a sparse frame's: no range may
// continue them); a timed call (info != null) records its events and adds up the render kernel's launches; the sums become the frame.
struct SparseCall {
    crt_scene* sc;
    hipStream_t st;
    bool timed;
    crt_params p;
    Shard sh;
    double kernel_ms = 0.0;
    bool kernel_unread = false; // a range's launches have been enqueued whose time (ev_k0 .. ev_k1) has not been added yet
    hipEvent_t e0 = nullptr, e1 = nullptr;
    SparseCall(crt_scene* sc_, const crt_params* prm, hipStream_t st_, bool timed_) : sc(sc_), st(st_), timed(timed_), p(*prm)
    {
        p.flags = (p.flags | CRT_FLAG_VARIANCE) & ~(uint32_t)(CRT_FLAG_STATS | CRT_FLAG_BOUNDED_RADIANCE | CRT_FLAG_HALF_BUFFERS | CRT_FLAG_PIXEL_FILTER); // (a sparse frame keeps no halves and no filter sums)
        sh = make_shard(p.width, p.height, p.world);
    }
    ~SparseCall() { sc->acc.samples = 0; sc->var.valid = false; sc->half.valid = false; sc->pf_mark.valid = false; }
    void begin()
    {
        HIP_CHECK(hipSetDevice(sc->device));
        if (!timed) return;
        ensure_events(sc);
        e0 = sc->ev[0]; e1 = sc->ev[1];
        HIP_CHECK(hipEventRecord(e0, st));
    }
    // samples [s_begin, s_begin + s_count) of the frame: of every pixel slot (src == nullptr), or of the slots src lists
    int render(const crt_camera* cam, uint32_t s_begin, uint32_t s_count, const ItemSource* src)
    {
        const int rc = render_impl(sc, cam, &p, nullptr, nullptr, st, nullptr, s_begin, s_count, src, true);
        kernel_unread = rc == CRT_OK;
        return rc;
    }
    void read_kernel_ms() // after a synchronization
    {
        float ms = 0.0f;
        if (timed && kernel_unread) { HIP_CHECK(hipEventElapsedTime(&ms, sc->ev_k0, sc->ev_k1)); kernel_ms += ms; }
        kernel_unread = false;
    }
    // the frame's layout and planes (once they are allocated)
    SumsParams sums() const
    {
        FrameMark mark;
        mark.set(&p, 0, (p.flags & CRT_FLAG_TILED_OUTPUT) != 0);
        SumsParams H;
        H.A = frame_aparams(sc, mark, sh);
        H.qacc = sc->accum_q.p; H.nsamp = sc->ad_nsamp.p;
        return H;
    }
    // k_adaptive_resolve on the count plane and the sums; a timed call then synchronizes and reads its timers
    void resolve(SumsParams H, void* d_rgb, void* d_mean, void* d_samples, void* d_var, float* kernel_ms_out, float* total_ms_out)
    {
        H.A.out_rgb = (uint8_t*)d_rgb; H.A.out_mean = (float*)d_mean;
        launch_adaptive_resolve(H, (uint32_t*)d_samples, (float*)d_var, st);
        HIP_CHECK(hipGetLastError());
        if (!timed) return;
        HIP_CHECK(hipEventRecord(e1, st));
        HIP_CHECK(hipStreamSynchronize(st));
        read_kernel_ms();
        *kernel_ms_out = (float)kernel_ms;
        HIP_CHECK(hipEventElapsedTime(total_ms_out, e0, e1));
    }
};

// A pass of crt_render_adaptive: the n_active slots of `list` take every sample of the pass.  k_adaptive_select has set their counts to
// the pass's end already.
struct ActiveList : ItemSource {
    const uint32_t* list = nullptr;
    uint32_t n_active = 0;
    uint32_t items(uint32_t, uint32_t ns) const override { return (uint32_t)((uint64_t)ns * n_active); }
    void fill(uint32_t* item_list, uint32_t, uint32_t, uint32_t n_items, hipStream_t st) const override
    {
        launch_adaptive_items(item_list, list, n_active, n_items, sums.A.nslots, st);
    }
};

// The range of crt_render_map: every pixel slot takes its own number of the range's samples
struct SampleMap : ItemSource {
    MapParams D{};                     // the sums (ItemSource::sums again), the count plane and the cursors
    std::vector<uint32_t> chunk_items; // work items of chunk 0, 1, ... of the range: the slots with n_p > s, summed over the chunk's samples
    uint32_t items(uint32_t k, uint32_t) const override { return chunk_items[k]; }
    void fill(uint32_t* item_list, uint32_t s0, uint32_t ns, uint32_t n_items, hipStream_t st) const override
    {
        MapParams Q = D;
        Q.item_list = item_list; Q.n_items = n_items; Q.s0 = s0; Q.ns = ns;
        // (the kernel fills every position when the histogram is the count plane's; cleared first, so that a position it did not
        // fill names work item 0 of the chunk, inside L, not what an earlier launch left there)
        HIP_CHECK(hipMemsetAsync(item_list, 0, (size_t)n_items * sizeof(uint32_t), st));
        launch_map_items(Q, st);
    }
};

// ---------- crt_render_adaptive ----------
int adaptive_impl(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_adaptive_params* ap, void* d_rgb, void* d_mean, void* d_samples,
                  void* d_var, hipStream_t st, crt_adaptive_info* info)
{
    const int rc0 = sparse_check(ADAPTIVE, sc, cam, prm, ap, nullptr, 0, d_rgb, d_mean);
    if (rc0 != CRT_OK) return rc0;
    SparseCall call(sc, prm, st, info != nullptr);
    const Shard& sh = call.sh;
    const uint32_t S = call.p.spp;
    return hip_guard([&]() -> int {
        call.begin();
        int rc = call.render(cam, 0, ap->min_samples, nullptr); // the warm-up
        if (rc != CRT_OK) return rc;
        sc->ad_nsamp.ensure_uncached(sh.nslots); sc->ad_list.ensure_uncached(sh.nslots);
        sc->ad_count.ensure_uncached(1);
        if (!sc->h_ad_count) HIP_CHECK(hipHostMalloc((void**)&sc->h_ad_count, sizeof(unsigned int), hipHostMallocDefault));
        ActiveList pass;
        AdaptiveParams D{};
        D.sums = pass.sums = call.sums();
        D.list = sc->ad_list.p; D.count = sc->ad_count.p;
        pass.list = D.list;
        D.threshold = ap->threshold; D.mean_floor = ap->mean_floor;
        D.n = ap->min_samples;
        launch_adaptive_init(D, st);
        HIP_CHECK(hipGetLastError());
        crt_adaptive_info I;
        std::memset(&I, 0, sizeof(I));
        const uint64_t pixels = shard_pixels(D.sums.A);
        I.passes = 1; I.paths = pixels * ap->min_samples; I.paths_uniform = pixels * S;
        for (uint32_t n = ap->min_samples; n < S;) {
            const uint32_t ns = std::min(ap->step_samples, S - n);
            HIP_CHECK(hipMemsetAsync(sc->ad_count.p, 0, sizeof(unsigned int), st));
            D.n = n; D.ns_pass = ns;
            launch_adaptive_select(D, st);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(sc->h_ad_count, sc->ad_count.p, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st)); // the one synchronization of a pass: how many pixels go on
            call.read_kernel_ms();
            const uint32_t active = std::min<uint32_t>(*sc->h_ad_count, sh.nslots);
            if (active == 0) break;
            if (I.passes - 1u < CRT_ADAPTIVE_PASSES_REPORTED) I.pass_pixels[I.passes - 1u] = active;
            pass.n_active = active;
            rc = call.render(cam, n, ns, &pass);
            if (rc != CRT_OK) return rc;
            I.passes++; I.paths += (uint64_t)active * ns;
            n += ns;
        }
        call.resolve(D.sums, d_rgb, d_mean, d_samples, d_var, &I.kernel_ms, &I.total_ms);
        if (info) *info = I;
        return CRT_OK;
    });
}

// ---------- crt_render_map (call == MAP: d_map is the caller's W x H map and s_begin its sample_begin) and crt_render_planned (PLANNED:
// the warm-up range and the plan come first, and the map is the plan's, per pixel slot, on the device all the way) ----------
int map_impl(Call call_id, crt_scene* sc, const crt_camera* cam, const crt_params* prm, const uint32_t* d_map, uint32_t s_begin, const crt_adaptive_params* planned,
             void* d_rgb, void* d_mean, void* d_samples, void* d_var, hipStream_t st, crt_map_info* info)
{
    const int rc0 = sparse_check(call_id, sc, cam, prm, planned, d_map, s_begin, d_rgb, d_mean);
    if (rc0 != CRT_OK) return rc0;
    const bool is_planned = call_id == PLANNED;
    SparseCall call(sc, prm, st, info != nullptr);
    const Shard& sh = call.sh;
    const uint32_t S = call.p.spp;
    return hip_guard([&]() -> int {
        call.begin();
        // (before anything takes their addresses: render_impl's own calls then find them in place)
        sc->accum.ensure_uncached((size_t)sh.nslots * 3); sc->accum_q.ensure_uncached((size_t)sh.nslots * 3);
        sc->ad_nsamp.ensure_uncached(sh.nslots); sc->ad_list.ensure_uncached(sh.nslots);
        sc->map_hist.ensure_uncached((size_t)S + 1); sc->map_cursor.ensure_uncached(S);
        const size_t words = 2 * ((size_t)S + 1);
        if (sc->h_map_words < words) {
            if (sc->h_map) { (void)hipHostFree(sc->h_map); sc->h_map = nullptr; sc->h_map_words = 0; }
            HIP_CHECK(hipHostMalloc((void**)&sc->h_map, words * sizeof(unsigned int), hipHostMallocDefault));
            sc->h_map_words = words;
        }
        unsigned int* const h_hist = sc->h_map;
        unsigned int* const h_cursor = sc->h_map + S + 1;
        uint32_t warm_launches = 0;
        if (is_planned) { // the warm-up: crt_render_range(0, min_samples) with the variance sums
            s_begin = planned->min_samples;
            const int rc = call.render(cam, 0, s_begin, nullptr);
            if (rc != CRT_OK) return rc;
            warm_launches = sc->last_launches;
        }
        SampleMap src;
        MapParams& D = src.D;
        D.sums = src.sums = call.sums();
        D.hist = sc->map_hist.p; D.cursor = sc->map_cursor.p;
        D.sample_begin = s_begin;
        D.map = d_map;
        if (is_planned) { // the plan at n = min_samples, one count per pixel slot
            MapParams Q = D;
            Q.sums.A.tiled_output = 1u;
            Q.n = s_begin; Q.threshold = planned->threshold; Q.mean_floor = planned->mean_floor; Q.out_map = sc->ad_list.p;
            launch_sample_plan(Q, st);
            HIP_CHECK(hipGetLastError());
            D.map = sc->ad_list.p; D.map_per_slot = 1u;
        }
        HIP_CHECK(hipMemsetAsync(sc->map_hist.p, 0, ((size_t)S + 1) * sizeof(unsigned int), st));
        launch_map_prepare(D, st);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(h_hist, sc->map_hist.p, ((size_t)S + 1) * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st)); // the one synchronization of the call: how many slots take each sample
        call.read_kernel_ms();
        // count_s = slots with n_p > s, from the top of the histogram down (h_hist[0]: the padding slots)
        crt_map_info I;
        std::memset(&I, 0, sizeof(I));
        uint32_t max_np = 0;
        uint64_t pixels = 0, all_samples = 0;
        for (uint32_t v = 1; v <= S; v++) {
            const uint64_t c = std::min<uint32_t>(h_hist[v], sh.nslots);
            pixels += c; all_samples += c * v;
            if (c) max_np = v;
        }
        pixels = std::min<uint64_t>(pixels, sh.nslots); // (a histogram that is not one cannot size a list beyond the chunk)
        I.max_samples = max_np; I.launches = warm_launches;
        I.paths = all_samples - (is_planned ? 0u : pixels * s_begin); // (n_p >= sample_begin at every pixel)
        I.paths_uniform = pixels * S;
        if (max_np > s_begin) {
            const uint32_t s_count = max_np - s_begin, chunk = chunk_samples(sh.nslots, s_count);
            uint64_t above = 0; // slots with n_p > s
            std::vector<uint32_t> count(s_count);
            for (uint32_t s = max_np; s-- > s_begin;) {
                above = std::min<uint64_t>(above + h_hist[s + 1], sh.nslots);
                count[s - s_begin] = (uint32_t)above;
            }
            for (uint32_t s0 = s_begin; s0 < max_np; s0 += chunk) {
                uint64_t at = 0; // (at most chunk x nslots <= 2^30)
                for (uint32_t s = s0; s < std::min(s0 + chunk, max_np); s++) { h_cursor[s] = (unsigned int)at; at += count[s - s_begin]; }
                src.chunk_items.push_back((uint32_t)at);
            }
            HIP_CHECK(hipMemcpyAsync(sc->map_cursor.p + s_begin, h_cursor + s_begin, (size_t)s_count * sizeof(unsigned int), hipMemcpyHostToDevice, st));
            const int rc = call.render(cam, s_begin, s_count, &src);
            if (rc != CRT_OK) return rc;
            I.launches += (uint32_t)src.chunk_items.size();
        }
        call.resolve(D.sums, d_rgb, d_mean, d_samples, d_var, &I.kernel_ms, &I.total_ms);
        if (info) *info = I;
        return CRT_OK;
    });
}

// The host-buffer form of the three calls: after the argument checks (rc0), device buffers for the device form, then the copies back
template <class DeviceForm>
int host_form(int rc0, crt_scene* sc, const crt_params* prm, uint8_t* out_rgb, float* out_mean, uint32_t* out_samples, float* out_variance, DeviceForm device_form)
{
    if (rc0 != CRT_OK) return rc0;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        const uint64_t npix = out_pixels(prm->width, prm->height, prm->world, (prm->flags & CRT_FLAG_TILED_OUTPUT) != 0);
        Staging s(npix, out_rgb != nullptr, out_mean != nullptr), v(npix, false, out_variance != nullptr);
        DevBuf<uint32_t> n;
        if (out_samples) n.alloc(npix);
        const int rc = device_form(s.rgb.p, s.f32.p, n.p, v.f32.p);
        if (rc != CRT_OK) return rc;
        s.download(out_rgb, out_mean);
        v.download(nullptr, out_variance);
        n.download(out_samples, npix);
        return CRT_OK;
    });
}

// Argument checks of both forms of crt_sample_plan, before any device call
int plan_check(const crt_scene* sc, float threshold, float mean_floor, const void* out)
{
    if (!sc || !out) return sums_check("crt_sample_plan", sc, out); // a null argument is reported first ...
    const int rc = threshold_check("crt_sample_plan", threshold, mean_floor); // ... then the criterion's parameters, then what the handle holds
    return rc != CRT_OK ? rc : sums_check("crt_sample_plan", sc, out);
}

} // namespace

extern "C" {

int crt_adaptive_defaults(crt_adaptive_params* ap)
{
    if (!ap) return fail(CRT_ERR_INVALID_ARG, "crt_adaptive_defaults: null argument");
    ap->min_samples = 16; ap->step_samples = 64; ap->threshold = 0.05f; ap->mean_floor = 0.01f;
    return CRT_OK;
}

int crt_render_adaptive_device(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_adaptive_params* ap, void* d_rgb, void* d_mean,
                               void* d_samples, void* d_variance, void* stream, crt_adaptive_info* info)
{
    return adaptive_impl(sc, cam, prm, ap, d_rgb, d_mean, d_samples, d_variance, (hipStream_t)stream, info);
}

int crt_render_adaptive(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_adaptive_params* ap, uint8_t* out_rgb, float* out_mean,
                        uint32_t* out_samples, float* out_variance, crt_adaptive_info* info)
{
    return host_form(sparse_check(ADAPTIVE, sc, cam, prm, ap, nullptr, 0, out_rgb, out_mean), sc, prm, out_rgb, out_mean, out_samples, out_variance,
                     [&](void* rgb, void* mean, void* n, void* var) { return adaptive_impl(sc, cam, prm, ap, rgb, mean, n, var, nullptr, info); });
}

int crt_render_map_device(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const void* d_sample_map, uint32_t sample_begin, void* d_rgb, void* d_mean,
                          void* d_samples, void* d_variance, void* stream, crt_map_info* info)
{
    return map_impl(MAP, sc, cam, prm, (const uint32_t*)d_sample_map, sample_begin, nullptr, d_rgb, d_mean, d_samples, d_variance, (hipStream_t)stream, info);
}

int crt_render_map(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const uint32_t* sample_map, uint32_t sample_begin, uint8_t* out_rgb, float* out_mean,
                   uint32_t* out_samples, float* out_variance, crt_map_info* info)
{
    return host_form(sparse_check(MAP, sc, cam, prm, nullptr, sample_map, sample_begin, out_rgb, out_mean), sc, prm, out_rgb, out_mean, out_samples, out_variance,
                     [&](void* rgb, void* mean, void* n, void* var) {
                         DevBuf<uint32_t> m;
                         m.upload(sample_map, (size_t)prm->width * prm->height);
                         return map_impl(MAP, sc, cam, prm, m.p, sample_begin, nullptr, rgb, mean, n, var, nullptr, info);
                     });
}

int crt_render_planned_device(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_adaptive_params* ap, void* d_rgb, void* d_mean, void* d_samples,
                              void* d_variance, void* stream, crt_map_info* info)
{
    return map_impl(PLANNED, sc, cam, prm, nullptr, 0, ap, d_rgb, d_mean, d_samples, d_variance, (hipStream_t)stream, info);
}

int crt_render_planned(crt_scene* sc, const crt_camera* cam, const crt_params* prm, const crt_adaptive_params* ap, uint8_t* out_rgb, float* out_mean,
                       uint32_t* out_samples, float* out_variance, crt_map_info* info)
{
    return host_form(sparse_check(PLANNED, sc, cam, prm, ap, nullptr, 0, out_rgb, out_mean), sc, prm, out_rgb, out_mean, out_samples, out_variance,
                     [&](void* rgb, void* mean, void* n, void* var) { return map_impl(PLANNED, sc, cam, prm, nullptr, 0, ap, rgb, mean, n, var, nullptr, info); });
}

int crt_sample_plan_device(crt_scene* sc, float threshold, float mean_floor, void* d_map, void* stream, crt_plan_info* info)
{
    const int rc = plan_check(sc, threshold, mean_floor, d_map);
    if (rc != CRT_OK) return rc;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        MapParams D{};
        D.sums.A = frame_aparams(sc, sc->var, make_shard(sc->var.width, sc->var.height, sc->var.world));
        D.sums.qacc = sc->accum_q.p;
        D.n = sc->var.samples; D.threshold = threshold; D.mean_floor = mean_floor; D.out_map = (uint32_t*)d_map;
        launch_sample_plan(D, (hipStream_t)stream);
        HIP_CHECK(hipGetLastError());
        if (info) { info->samples = sc->var.samples; info->spp = sc->var.spp; }
        return CRT_OK;
    });
}

int crt_sample_plan(crt_scene* sc, float threshold, float mean_floor, uint32_t* out_map, crt_plan_info* info)
{
    const int rc0 = plan_check(sc, threshold, mean_floor, out_map);
    if (rc0 != CRT_OK) return rc0;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        const uint64_t npix = out_pixels(sc->var.width, sc->var.height, sc->var.world, sc->var.tiled != 0);
        DevBuf<uint32_t> m;
        m.alloc(npix);
        const int rc = crt_sample_plan_device(sc, threshold, mean_floor, m.p, nullptr, info);
        if (rc != CRT_OK) return rc;
        HIP_CHECK(hipDeviceSynchronize());
        m.download(out_map, npix);
        return CRT_OK;
    });
}

} // extern "C"
