// cudaraytracing_amd/csrc/crt_scene.h -- the scene handle of the device layer (struct crt_scene: the uploaded arrays, the buffers and
// events a frame uses, what a progressive render has accumulated) and the small helpers crt_scene.hip (create / export / destroy) and
// crt_render.hip / crt_sparse.hip / crt_aov_pass.hip (the launch logic) share: the shard of a frame, its slot map for the image-space kernels, the host's form of the slot rule.
#ifndef CRT_SCENE_H
#define CRT_SCENE_H
#include "crt_internal.h"
#include "crt_scene_layout.h"

#include <cstdlib>
#include <vector>

// What the sums of a frame in flight on a handle hold: samples [0, samples) of spp, for this size, shard and output layout.
struct FrameMark {
    uint32_t samples = 0, spp = 0, width = 0, height = 0, rank = 0, world = 1, tiled = 0;
    bool valid = false; // (crt_scene::var only) the last render call had CRT_FLAG_VARIANCE
    void set(const crt_params* prm, uint32_t samples_, bool tiled_)
    {
        samples = samples_; spp = prm->spp; width = prm->width; height = prm->height;
        rank = prm->rank; world = prm->world; tiled = tiled_ ? 1u : 0u;
    }
    // for the message of a range that does not continue the frame: what the sums hold, `tail` after the samples and spp
    std::string in_flight(const std::string& tail) const
    {
        return samples == 0 ? std::string("no frame is in flight on the handle")
                            : "the frame in flight holds samples [0, " + std::to_string(samples) + ") of spp " + std::to_string(spp) + tail;
    }
};

// Everything the list k_order_items writes depends on: the draws (seed, first sample, p_rr), the geometry of the work items and the cursor
// shards (what decode_item reads), the window, the classes -- and the stream the list was built on, which orders the build before its use.
// Camera, scene and traversal are not in it: a caller that renders a view again with a fixed seed finds the list built.
// Plain words, zeroed before they are filled, so that two keys compare with memcmp.
struct ItemOrderKey {
    uint64_t seed, stream;
    uint32_t valid, sample_begin, n_items, items_per_shard, order_window, shards, ring, spsh, nslots, rank, world, tiles_x, n_tiles, width, height, p_rr_bits;
    uint32_t n_classes, class_lo[8];
    uint32_t pad_;
};

// What a launch without the commit ring leaves per work item, in one allocation that grows to the larger use: a render's radiance (12
// bytes, crtk::Rad3) or the answers of k_mega3's query form (16 bytes: crt_intersect, the AOV pass).  Each form has its own accessor and
// its own element type, so an entry of one is never addressed with the stride of the other.
struct ItemResults {
    crtk::DevBuf<float> words;
    crtk::Rad3* radiance(size_t n) { words.ensure(n * 3); return reinterpret_cast<crtk::Rad3*>(words.p); }
    float4* answers(size_t n) { words.ensure(n * 4); return reinterpret_cast<float4*>(words.p); } // (hipMalloc's alignment)
};

// float4 rows of crt_scene::aov_acc per pixel slot (the layout: AovParams::acc, crt_internal.h): the AOV passes' three, and the four of
// the shading form, whose six extra sums fill the two spare floats of row 2 and a fourth row
const size_t kAovAccRows = 3, kAovAccRowsShading = 4;

struct RefitState;
void refit_release(RefitState* r); // crt_refit.hip

struct crt_scene {
    int device = 0;
    crtk::DevBuf<float4> nodes, tri_geo, mats, ltri, nodes3, leaf_geo, tri_nm, nodes4, nodes4i, leaf_geo_i;
    crtk::DevBuf<int32_t> rec_map;
    uint32_t max_leaf = 0; // triangles in the largest leaf
    crtk::DevBuf<int32_t> tri_mat, leaf_count;
    crtk::DevBuf<uint4> lights;
    // path pool + per-item radiance + cross-chunk accumulator
    crtk::DevBuf<float4> p_ro, p_rd, p_vx, p_la, p_cc, p_vn, p_rec_a, p_rec_b;
    crtk::DevBuf<float> p_rec_c; // k_mega3: the vertex records' cosine plane
    ItemResults L;
    crtk::DevBuf<uint4> p_id;
    uint32_t n_mats = 0;
    crtk::DevBuf<float2> p_res;
    crtk::DevBuf<float> accum;
    crtk::DevBuf<float4> aov_acc;                   // AOV pass: running sums of the pixel slots between its chunks (crt_render_aov): kAovAccRows per slot, kAovAccRowsShading for crt_render_aov_shading
    // crt_render_aov_specular: per camera ray of a chunk the chain state (thr.xyz, len) and (last triangle, bounces); the items of the
    // rays in the two halves of the query pool; the counter of the rays that go on (uncached) and the pinned word it is copied to
    crtk::DevBuf<float4> aovs_state;
    crtk::DevBuf<int2> aovs_aux;
    crtk::DevBuf<uint32_t> aovs_item;
    crtk::DevBuf<unsigned int> aovs_count;
    unsigned int* h_aovs_count = nullptr;
    // crt_render_aov_direct: per camera ray of a chunk its first vertex (pos.xyz, triangle or -1), and the contribution plane of a
    // sub-batch (c.xyz, flags per (sample, q, slot) entry); the plane entries of its traced rays are aovs_item, their counter aovs_count,
    // its running sums aov_acc (kAovDirectAccRows per slot, crt_aov_direct.h)
    crtk::DevBuf<float4> aovd_vert, aovd_plane;
    // crt_render_aov_ao uses the same two (per camera ray pos and facing normal: aovd_vert at twice the rays; the entry plane: aovd_plane),
    // aov_acc (kAovAoAccRows per slot, crt_aov_ao.h) and the sum of a call's occlusion rays, read only when crt_aov_info is asked for.
    // root_aa / root_bb: the box of the scene description's root node (crt_aov_ao_defaults)
    crtk::DevBuf<unsigned long long> aovao_rays;
    float root_aa[3] = {0.0f, 0.0f, 0.0f}, root_bb[3] = {0.0f, 0.0f, 0.0f};
    crtk::DevBuf<unsigned long long> counters;     // [CNT_SHARDS][CNT_STRIDE]
    crtk::DevBuf<unsigned int> item_next;           // [ITEM_SHARDS][ITEM_STRIDE]
    crtk::DevBuf<uint32_t> item_list;               // k_order_items: the order of the work items of a launch (small launches only)
    crtk::DevBuf<unsigned int> ring_done, ring_state; // commit ring: finished items per (shard, sample), shard words
    crtk::DevBuf<crtk::Rad3> ring_L;                     // commit ring: radiance of [ring samples][shards * slots per shard] (uncached memory)
    std::vector<unsigned int> ring_state_host;
    uint64_t last_radiance_bytes = 0;           // per-work-item (or ring) radiance storage the last render used
    uint32_t last_ring_samples = 0;             // its ring size in samples (0: one radiance per work item)
    crtk::DevBuf<unsigned int> order_cnt;           // k_order_items: [cursor shards][classes] counters, one 128 B line each
    ItemOrderKey order_key{};                        // what item_list holds (valid = false: nothing a launch may reuse)
    uint64_t order_built = 0, order_reused = 0;     // launches that built item_list with k_order_items / found it built (crt_item_order)
    uint32_t order_classes = 0, order_window = 0;   // of the handle's last launch of the render kernel (0: handed out in cursor order, or by a sparse frame's list)
    crtk::DevBuf<unsigned int> slot_next[2];        // [SLOT_SHARDS][SLOT_STRIDE], one per pool half
    crtk::DevBuf<int2> spill[2];                    // traversal stack overflow, one per pool half
    hipStream_t aux_stream = nullptr;         // second pool half runs here so that k_logic overlaps k_trace
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr; // around the k_mega3 launches of the last frame, recorded without synchronizing (crt_last_launch_ms)
    uint32_t last_launches = 0;
    int n_cus = 0;
    unsigned long long* h_counters = nullptr; // pinned copy of counters
    crtdev::DevScene dev{};
    crt_tree_scalars scalars{}; // (crt_scene_export)
    int stack_cap = 0;
    uint32_t n_tris = 0;
    crt_accel_info accel{};
    bool can(uint32_t cap) const { return (accel.layout_caps & cap) != 0; } // crtlayout::CAP_*
    FrameMark acc; // progressive render in flight: what the accumulator holds (crt_preview)
    // CRT_FLAG_VARIANCE: the sum of squares beside accum (3 planes of nslots, allocated when the flag is first used) and what the two
    // sums hold (crt_variance): samples so far of the frame the flag has been on for since sample 0; valid = the last render call had it
    crtk::DevBuf<float> accum_q;
    FrameMark var;
    // CRT_FLAG_HALF_BUFFERS: the sums of the even and of the odd samples (6 planes of nslots, allocated when the flag is first used) and
    // what they hold (crt_half_buffers), by var's rules: valid = the last render call had the flag, and so had every range since sample 0
    crtk::DevBuf<float> accum_h;
    FrameMark half;
    // CRT_FLAG_PIXEL_FILTER: the handle's filter (crt_set_pixel_filter), the sums a and W (4 planes of nslots, allocated when the flag is
    // first used), what they hold (crt_filtered_frame), by var's rules, and the filter they were made with
    crt_pixel_filter pf{};
    bool pf_set = false;
    crtk::DevBuf<float> accum_pf;
    FrameMark pf_mark;
    crt_pixel_filter pf_frame{};
    // crt_render_adaptive: per pixel slot its sample count, the compacted list of the slots that take the next pass and its counter
    // (uncached, agent-scope atomics only: crt_adaptive.hip), and the pinned word the counter is copied to once per pass
    crtk::DevBuf<uint32_t> ad_nsamp, ad_list;
    crtk::DevBuf<unsigned int> ad_count;
    unsigned int* h_ad_count = nullptr;
    // crt_render_map: the histogram of the per-slot counts (spp + 1 words) and the cursors of the item-list kernel (spp words), uncached
    // (crt_sample_map.hip; the counts themselves are ad_nsamp, a planned frame's map ad_list), and their pinned mirror: the histogram
    // the host sizes the chunks from in words [0, spp], the cursors' start values it uploads in words [spp + 1, 2 spp]
    crtk::DevBuf<unsigned int> map_hist, map_cursor;
    unsigned int* h_map = nullptr;
    size_t h_map_words = 0;
    // crt_frame_error: the blocks' partials of the two fp64 sums and of the counts (crt_frame_error.h: FrameErrorParams), the summary of
    // the host form and of crt_render_until's checks, and the pinned copy a check's `above` is read through
    crtk::DevBuf<double> fe_sum;
    crtk::DevBuf<uint32_t> fe_cnt;
    crtk::DevBuf<crt_frame_error_info> fe_info;
    crt_frame_error_info* h_fe = nullptr;
    // crt_scene_refit: the materials of the light triangles (the device keeps their emission only; the host form's check), and what
    // the handle's first refit makes: tables, scratch, events (crt_refit.hip)
    std::vector<int32_t> ltri_mat;
    struct RefitState* refit = nullptr;
    std::vector<hipEvent_t> ev;
    std::vector<hipEvent_t> ev_chunk; // a timed megakernel frame: (before, after) the launch of chunk i at [2 i], [2 i + 1]
    ~crt_scene()
    {
        refit_release(refit);
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_chunk) (void)hipEventDestroy(e);
        if (ev_k0) (void)hipEventDestroy(ev_k0);
        if (ev_k1) (void)hipEventDestroy(ev_k1);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (aux_stream) (void)hipStreamDestroy(aux_stream);
        if (h_counters) (void)hipHostFree(h_counters);
        if (h_ad_count) (void)hipHostFree(h_ad_count);
        if (h_aovs_count) (void)hipHostFree(h_aovs_count);
        if (h_map) (void)hipHostFree(h_map);
        if (h_fe) (void)hipHostFree(h_fe);
    }
};

namespace crtk {

struct Shard {
    uint32_t tiles_x, tiles_y, n_tiles, local_tiles, nslots;
};
inline Shard make_shard(uint32_t w, uint32_t h, uint32_t world)
{
    Shard s;
    s.tiles_x = (w + CRT_TILE - 1) / CRT_TILE;
    s.tiles_y = (h + CRT_TILE - 1) / CRT_TILE;
    s.n_tiles = s.tiles_x * s.tiles_y;
    s.local_tiles = (s.n_tiles + world - 1) / world; // padded so every rank writes the same number of slots
    s.nslots = s.local_tiles * 64u;
    return s;
}

// The slot map (crt_internal.h) of shard `sh` of a frame; F: crt_params or FrameMark (width, height, rank, world)
template <class F> inline void fill_slot_map(SlotMap& m, const F& f, bool tiled, const Shard& sh)
{
    m.width = f.width; m.height = f.height; m.rank = f.rank; m.world = f.world;
    m.tiles_x = sh.tiles_x; m.n_tiles = sh.n_tiles; m.nslots = sh.nslots;
    m.tiled_output = tiled ? 1u : 0u;
    m.tiles_x_div = make_fastdiv(sh.tiles_x);
}

// The host's form of the slot rule (slot_to_pixel, crt_path.h), a tile at a time: how many of the slots 64 * lt .. 64 * lt + 63 are
// pixels.  Slot 64 * lt + pix is one iff the tile lies in the frame and (pix & 7, pix >> 3) lies in the part of the tile the frame covers.
inline uint32_t tile_pixels(const SlotMap& m, uint32_t lt)
{
    const uint32_t tile = lt * m.world + m.rank;
    if (tile >= m.n_tiles) return 0;
    const uint32_t ty = tile / m.tiles_x, tx = tile - ty * m.tiles_x;
    const uint32_t w = m.width - tx * CRT_TILE, h = m.height - ty * CRT_TILE;
    return (w < CRT_TILE ? w : (uint32_t)CRT_TILE) * (h < CRT_TILE ? h : (uint32_t)CRT_TILE);
}

// What crt_variance and crt_sample_plan (`who`) need of the handle: sums of at least two samples of a frame with CRT_FLAG_VARIANCE
inline int sums_check(const char* who, const crt_scene* sc, const void* out)
{
    const std::string w(who);
    if (!sc || !out) return fail(CRT_ERR_INVALID_ARG, w + ": null argument");
    if (!sc->var.valid) return fail(CRT_ERR_INVALID_ARG, w + ": no render with CRT_FLAG_VARIANCE on the handle yet, or the last render (or a range of the frame in flight) was submitted without it");
    if (sc->var.samples < 2) return fail(CRT_ERR_INVALID_ARG, w + ": fewer than 2 samples accumulated (one sample has no variance)");
    return CRT_OK;
}

// What crt_half_buffers needs of the handle: half sums of at least two samples of a frame with CRT_FLAG_HALF_BUFFERS
inline int halves_check(const char* who, const crt_scene* sc, const void* out_a, const void* out_b)
{
    const std::string w(who);
    if (!sc || (!out_a && !out_b)) return fail(CRT_ERR_INVALID_ARG, w + ": null argument (a scene and at least one of the two buffers)");
    if (!sc->half.valid) return fail(CRT_ERR_INVALID_ARG, w + ": no render with CRT_FLAG_HALF_BUFFERS on the handle yet, or the last render (or a range of the frame in flight) was submitted without it");
    if (sc->half.samples < 2) return fail(CRT_ERR_INVALID_ARG, w + ": fewer than 2 samples accumulated (the half of the odd samples is empty)");
    return CRT_OK;
}

inline uint32_t env_u32(const char* name, uint32_t dflt)
{
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    long x = std::strtol(v, nullptr, 10);
    return x > 0 ? (uint32_t)x : dflt;
}

} // namespace crtk
#endif
