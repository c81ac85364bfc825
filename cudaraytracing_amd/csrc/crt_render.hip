// cudaraytracing_amd/csrc/crt_render.hip -- the launch logic of the device layer of libcrt.so: a frame (or a sample range of one) on either
// pipeline, ray queries, and their entry points in the C ABI of include/crt.h (crt_render*, crt_preview*, crt_variance*, crt_half_buffers*, crt_intersect,
// crt_device_*).  The frames in which not every pixel takes every sample (crt_render_adaptive*, crt_render_map*, crt_sample_plan*,
// crt_render_planned*) are ranges of render_impl with an item source: crt_sparse.hip; the AOV passes trace their rays with trace_queries:
// crt_aov_pass.hip.  Both see this file through crt_render.h.  The scene handle is made in crt_scene.hip (crt_scene.h); the kernels live
// in crt_mega3.hip, crt_wavefront.hip, crt_frame.hip, crt_adaptive.hip, crt_sample_map.hip.
// The slot map of a shard and the host's form of the slot rule: crt_scene.h; host-buffer copies: DevBuf::upload / download.
#include "crt_render.h"

#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace crtdev;
using namespace crtk;
using namespace crtlayout; // CAP_*

// 16-bit stack entries: the scene allows it (CAP_REF16 / CAP_REF16_INNER) and CRT_REF16=0 does not forbid it
static bool use_ref16(const crt_scene* sc, int mode, bool dec = false)
{
    if (mode == 1 || !sc->can(dec ? CAP_REF16_INNER : CAP_REF16)) return false;
    // CRT_REF16=0 ("the leaf refs do not fit 16 bits"): 32-bit entries for the coupled form -- the decoupled form keeps its 16-bit
    // entries; CRT_REF32=1: 32-bit stack entries in either form (tests, A/B)
    const char* e = std::getenv("CRT_REF16");
    const char* f = std::getenv("CRT_REF32");
    if (f && f[0] == '1') return false;
    return dec || !(e && e[0] == '0');
}

namespace {

const size_t kCountersBytes = (size_t)CNT_SHARDS * CNT_STRIDE * sizeof(unsigned long long);

struct RingPlan { uint32_t samples, spsh, shards; }; // commit ring of a launch: samples held (0 = one radiance per work item), pixel slots per cursor shard

// The decoupled-leaves form (Pool4LdsT) of a launch: CRT_TRAVERSAL_EXACT on a scene whose four-wide nodes fit the 16-bit entries of
// its stack (inner nodes only: up to about 160 000 triangles) and whose leaf records fit a queue entry.  Since the traversal steps
// alternate without the scheduler (crt_mega3.hip, CHAIN_MIN) it is the faster form on every scene measured (stand-in cornell-box
// - 4 %, veach-mis equal, the 102 412-triangle variant - 5 % against the coupled form with 32-bit entries), and the one whose
// layout does not change with the number of leaves.  CRT_DEC=1 / 0 forces / forbids it (tests, A/B).
static bool use_dec(const crt_scene* sc, int mode)
{
    if (mode != 2 || !sc->can(CAP_DEC)) return false;
    const char* e = std::getenv("CRT_DEC");
    if (e && e[0] == '0') return false;
    // (round 6: also beyond 32 768 four-wide nodes, where its stack has three 32-bit levels in LDS -- a 348 172-triangle cornell-box
    // --detail 7,5, 88 230 nodes: 14.6 ms at spp 64 against 16.1 ms of the coupled form with 32-bit entries, tools/big_mesh_probe.py)
    return true;
}
// The copy of the 4-wide tree without its rows of refs (nodes4i, round 6): the decoupled-leaves kernels with 16-bit stack entries take it
// whenever the scene offers it (CAP_IMPL: leaves of one record, <= 32 768 nodes); CRT_IMPL=0 keeps them on nodes4 (tests, A/B).
static bool use_impl(const crt_scene* sc, bool dec, bool r16)
{
    if (!dec || !r16 || !sc->can(CAP_IMPL)) return false;
    const char* e = std::getenv("CRT_IMPL");
    return !(e && e[0] == '0');
}

struct TraceSetup {
    TParams T;
    size_t lds;
    int mode_id;
    uint32_t blocks;
};
// Everything a k_trace launch over `pool` needs (grid sized to the device's residency: the kernel is persistent).
TraceSetup make_trace_setup(crt_scene* sc, const Pool& pool, uint32_t traversal, bool want_stats, int half = 0, int n_halves = 1)
{
    TraceSetup S;
    std::memset(&S.T, 0, sizeof(S.T));
    TParams& T = S.T;
    T.sc = sc->dev; T.pool = pool; T.counters = sc->counters.p;
    T.slot_next = sc->slot_next[half].p;
    T.refill_min = (int32_t)std::min<uint32_t>(64, env_u32("CRT_REFILL_MIN", REFILL_MIN));
    T.leaf_min = (int32_t)std::min<uint32_t>(64, env_u32("CRT_LEAF_MIN", LEAF_MIN));
    T.slots_per_shard = ((pool.n + SLOT_SHARDS - 1) / SLOT_SHARDS + 63u) & ~63u;
    // LDS holds the first levels of the traversal stack; the rest (rarely touched) spills to HBM/L2
    const int lds_cap = (int)std::min<uint32_t>((uint32_t)sc->stack_cap, std::max(2u, env_u32("CRT_STACK_LDS", 8)));
    T.stack_cap = lds_cap;
    S.lds = (size_t)lds_cap * 256 * sizeof(int2);
    S.mode_id = (traversal == CRT_TRAVERSAL_REFERENCE ? 2 : traversal == CRT_TRAVERSAL_EXACT ? 4 : 0) + (want_stats ? 1 : 0);
    int per_cu = trace_blocks_per_cu(S.mode_id, S.lds);
    // with two pool halves in flight leave room for the other half's k_logic blocks
    const uint32_t dflt_per_cu = n_halves > 1 ? 3u : 64u; // measured best on MI355X (C2): 3 trace blocks + logic blocks per CU
    per_cu = (int)std::min<uint32_t>((uint32_t)per_cu, env_u32("CRT_TRACE_BLOCKS_PER_CU", dflt_per_cu));
    S.blocks = std::min<uint32_t>((pool.n + 255) / 256, (uint32_t)(sc->n_cus * per_cu));
    const int spill_levels = std::max(1, sc->stack_cap - lds_cap);
    T.spill_stride = S.blocks * 256u;
    sc->spill[half].ensure((size_t)spill_levels * T.spill_stride);
    T.spill = sc->spill[half].p;
    return S;
}
void launch_trace_pass(crt_scene* sc, const TraceSetup& S, hipStream_t st)
{
    HIP_CHECK(hipMemsetAsync(S.T.slot_next, 0, (size_t)SLOT_SHARDS * SLOT_STRIDE * sizeof(unsigned int), st));
    launch_trace(S.mode_id, S.T, S.blocks, S.lds, st);
}

// How k_mega3 is launched on a scene: the instantiation (traversal mode, pool layout) and its persistent grid -- one wave per workgroup,
// pool_p rays per wave, as many workgroups as the device holds (at most per_cu_cap per CU) or as `items` work items fill.
struct MegaPlan {
    Mega3Kernel kern;
    bool r16;
    uint32_t blocks, lanes; // lanes: pool slots
    int lds_levels;         // levels of the traversal stack in LDS
    size_t spill_entries;   // the rest of the stack, per lane, in the global area
};
MegaPlan plan_mega3(const crt_scene* sc, uint32_t traversal, bool want_stats, bool trace_all, bool query, bool ring, uint64_t items, uint32_t per_cu_cap)
{
    MegaPlan m;
    const int mode3 = traversal == CRT_TRAVERSAL_REFERENCE ? 1 : traversal == CRT_TRAVERSAL_EXACT ? 2 : 0;
    const bool dec = use_dec(sc, mode3);
    m.r16 = use_ref16(sc, mode3, dec);
    const Mega3Variant* v = mega3_variant(mode3, want_stats, mode3 != 1 && trace_all, query, m.r16, ring, dec, use_impl(sc, dec, m.r16));
    if (!v) throw HipFail{hipErrorInvalidValue, "plan_mega3: no instantiation of k_mega3 for this request"};
    m.kern = v->kern;
    int per_cu = 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, m.kern, 64, 0) != hipSuccess || per_cu < 1) per_cu = 1;
    per_cu = (int)std::min<uint32_t>((uint32_t)per_cu, per_cu_cap);
    const uint32_t pool_p = v->pool_p; // (the pool and the LDS levels of the kernel that is launched, from its own descriptor)
    m.blocks = std::min<uint32_t>((uint32_t)std::min<uint64_t>((items + pool_p - 1) / pool_p, 0x7fffffffull), (uint32_t)(sc->n_cus * per_cu));
    m.lanes = m.blocks * pool_p;
    m.lds_levels = v->lds_levels;
    // (16-bit layout: a ray on the reference-arithmetic path keeps its whole stack in the global area)
    m.spill_entries = (size_t)(m.r16 ? std::max(1, sc->stack_cap) : std::max(1, sc->stack_cap - m.lds_levels)) * m.lanes;
    return m;
}

} // namespace

namespace crtk { // (declared in crt_render.h)

// The camera's half-height at distance 1 and aspect ratio (Render.cuh:338-339), as the camera rays of a frame (camera_dir) and of the AOV
// pass take them
void camera_scale_ar(const crt_camera* cam, const crt_params* prm, float& scale, float& ar)
{
    scale = det_tanf(cam->fov_y / 2);
    ar = (float)prm->width / (float)prm->height;
}

// Traces the n query rays in the handle's query pool (p_ro / p_rd, p_res primed: the form k_fill_rays writes) on stream st with the
// traversal phases of the render kernel itself -- k_mega3 in query form (work item = ray), or k_trace on the fallback pipeline -- and
// leaves the answers on the device: (t or FLT_MAX, bits(triangle or -1)) of ray i at the returned pointer + i * stride floats (the float4
// answers of the query form, stride 4, or p_res, stride 2).  Does not synchronize.  crt_intersect and the AOV passes.  first: the rays
// are those from `first` on in the pool (the pass that follows mirror bounces keeps its rays in two halves of the pool).
const float* trace_queries(crt_scene* sc, uint32_t n, uint32_t traversal, bool force_exact, hipStream_t st, uint32_t& stride, size_t first)
{
    if (choose_pipeline(sc) == 4) {
        const MegaPlan mp = plan_mega3(sc, traversal, false, false, true, false, n, 0xffffffffu);
        const uint32_t lanes = mp.lanes;
        sc->p_la.ensure(lanes); sc->p_id.ensure(lanes);
        float4* const answers = sc->L.answers(n);
        sc->spill[0].ensure(mp.spill_entries);
        MParams3 M3;
        std::memset(&M3, 0, sizeof(M3));
        LParams& P = M3.M.P;
        P.sc = sc->dev;
        P.pool.la = sc->p_la.p; P.pool.id = sc->p_id.p; P.pool.n = lanes;
        P.n_items = n;
        P.items_per_shard = ((n + ITEM_SHARDS - 1) / ITEM_SHARDS + 63u) & ~63u;
        P.item_next = sc->item_next.p; P.L4 = answers; P.counters = sc->counters.p;
        P.q_o = sc->p_ro.p + first; P.q_d = sc->p_rd.p + first;
        P.nslots = 1; P.nslots_div = make_fastdiv(1); P.tiles_x = 1; P.tiles_x_div = make_fastdiv(1); P.lsn_div = make_fastdiv(1);
        M3.M.sc = sc->dev; M3.M.counters = sc->counters.p; M3.M.spill_stride = lanes; M3.M.stack_cap = mp.lds_levels;
        M3.spill = (int*)sc->spill[0].p;
        M3.force_exact = force_exact ? 1u : 0u;
        HIP_CHECK(hipMemsetAsync(sc->item_next.p, 0, (size_t)ITEM_SHARDS * ITEM_STRIDE * sizeof(unsigned int), st));
        hipLaunchKernelGGL(mp.kern, dim3(mp.blocks), dim3(64), 0, st, M3);
        HIP_CHECK(hipGetLastError());
        stride = 4;
        return (const float*)answers;
    }
    Pool pool;
    std::memset(&pool, 0, sizeof(pool));
    pool.ro = sc->p_ro.p + first; pool.rd = sc->p_rd.p + first; pool.res = sc->p_res.p + first; pool.n = n;
    TraceSetup TS = make_trace_setup(sc, pool, traversal, false);
    launch_trace_pass(sc, TS, st);
    HIP_CHECK(hipGetLastError());
    stride = 2;
    return (const float*)(sc->p_res.p + first);
}


// Whether a range that begins at sample s_begin > 0 continues the frame `f` records (crt_scene::acc for the sum c, crt_scene::var for
// the sum of squares q): the samples before it are in the sums, and spp, size, shard and layout are the frame's.
bool continues_frame(const FrameMark& f, const crt_params* prm, uint32_t s_begin, bool tiled)
{
    return f.samples == s_begin && f.spp == prm->spp && f.width == prm->width && f.height == prm->height && f.rank == prm->rank &&
           f.world == prm->world && f.tiled == (tiled ? 1u : 0u);
}

// The events the timed forms record (a frame with stats, the AOV pass with info)
void ensure_events(crt_scene* sc)
{
    while (sc->ev.size() < (size_t)(4 * kMaxBatch + 4)) {
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        sc->ev.push_back(e);
    }
}

// Frame-kernel parameters (k_accumulate, k_preview, k_variance) of the frame `f` describes, on the handle's accumulator
AParams frame_aparams(const crt_scene* sc, const FrameMark& f, const Shard& sh)
{
    AParams A;
    std::memset(&A, 0, sizeof(A));
    fill_slot_map(A, f, f.tiled != 0, sh);
    A.spp = f.spp;
    A.accum = sc->accum.p;
    return A;
}

} // namespace crtk

namespace {

// The event pairs around the launches of a timed megakernel frame, one per chunk
void ensure_chunk_events(crt_scene* sc, uint32_t chunks)
{
    while (sc->ev_chunk.size() < 2 * (size_t)chunks) {
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        sc->ev_chunk.push_back(e);
    }
}

// One call of render_impl, as its two pipelines see it
struct Frame {
    crt_scene* sc;
    const crt_camera* cam;
    const crt_params* prm;
    hipStream_t st;
    crt_stats* stats;
    uint32_t s_begin, s_end;
    Shard sh;
    uint32_t chunk; // samples per launch (megakernel) or per pool fill (wavefront)
    uint64_t cap;   // radiance entries: work items of a chunk, or the ring
    Rad3* L;        // the chunk's radiance, cap entries (null with the ring, whose entries are crt_scene::ring_L)
    RingPlan ring;
    bool want_stats, tiled, want_var, var_frame, want_half, half_frame;
    bool pf_frame; // CRT_FLAG_PIXEL_FILTER on a frame that has had it since sample 0: every chunk also goes into the filter's sums
    AParams A;
    const ItemSource* src; // null: every pixel slot takes every sample of the range
    bool open;             // the frame is resolved by the caller, not by the range that ends at spp
};

// What both pipelines put into LParams: camera, size, shard, divisions, the handle's buffers
LParams frame_lparams(const Frame& f)
{
    const crt_scene* sc = f.sc;
    const crt_params* prm = f.prm;
    LParams P;
    std::memset(&P, 0, sizeof(P));
    P.sc = sc->dev;
    std::memcpy(P.eye, f.cam->eye, sizeof(P.eye));
    std::memcpy(P.inv_view, f.cam->inv_view, sizeof(P.inv_view));
    camera_scale_ar(f.cam, prm, P.scale, P.ar);
    P.width = prm->width; P.height = prm->height;
    P.p_rr = prm->p_rr; P.lsn = prm->light_sample_n; P.seed = prm->seed;
    P.rank = prm->rank; P.world = prm->world; P.tiles_x = f.sh.tiles_x; P.n_tiles = f.sh.n_tiles;
    P.nslots = f.sh.nslots;
    P.inv_lsn_pow2 = inv_if_pow2(prm->light_sample_n); P.lsn_div = make_fastdiv((uint32_t)std::max(1, prm->light_sample_n)); P.nslots_div = make_fastdiv(f.sh.nslots); P.tiles_x_div = make_fastdiv(f.sh.tiles_x);
    P.L = f.L; P.counters = sc->counters.p; P.item_next = sc->item_next.p; P.n_mats = sc->n_mats;
    return P;
}

// The n_items work items of the chunk of samples that starts at s0 -- one per pixel slot and sample, or what the range's item source
// lists -- in ITEM_SHARDS cursor shards
void set_chunk(LParams& P, uint32_t s0, uint32_t n_items)
{
    P.sample_begin = s0;
    P.n_items = n_items;
    P.items_per_shard = ((P.n_items + ITEM_SHARDS - 1) / ITEM_SHARDS + 63u) & ~63u;
}

// After the paths of samples [s0, s0 + ns) are done: their radiance into the frame's sum (the commit ring has made the sum already: the
// last range only tone-maps), and what the sums now hold into the handle's marks
void accumulate_chunk(Frame& f, uint32_t s0, uint32_t ns)
{
    crt_scene* sc = f.sc;
    AParams& A = f.A;
    A.chunk_samples = ns;
    A.first_chunk = s0 == 0; A.last_chunk = !f.open && s0 + ns >= f.prm->spp;
    if (f.ring.samples) { A.chunk_samples = 0; A.first_chunk = 0; } // the sum is in the accumulator already: tone mapping only
    if (!f.ring.samples || A.last_chunk) {
        // The filtered frame's read-out takes c where a pixel's W is not positive, and k_accumulate alone does not store c with the last
        // chunk: with the filter it folds that chunk as one that is not the last, and k_preview at scale 1 (c * 1.0f: c's bits) writes the frame.
        const bool keep_c = f.pf_frame && !f.want_var && A.last_chunk;
        if (keep_c) A.last_chunk = 0;
        if (f.src) f.src->fold(A, s0, ns, f.st);
        else if (f.want_half) launch_accumulate_half(A, sc->accum_q.p, sc->accum_h.p, s0 & 1u, f.st);
        else if (f.want_var) launch_accumulate_var(A, sc->accum_q.p, f.st);
        else launch_accumulate(A, f.st);
        if (keep_c) { A.last_chunk = 1; launch_preview(A, 1.0f, f.st); }
        if (f.pf_frame) launch_pixel_filter(A, sc->pf, sc->accum_pf.p, f.prm->seed, s0, f.st);
        HIP_CHECK(hipGetLastError());
        if (f.var_frame) { sc->var.valid = true; sc->var.set(f.prm, s0 + ns, f.tiled); }
        if (f.half_frame) { sc->half.valid = true; sc->half.set(f.prm, s0 + ns, f.tiled); }
        if (f.pf_frame) { sc->pf_mark.valid = true; sc->pf_mark.set(f.prm, s0 + ns, f.tiled); sc->pf_frame = sc->pf; }
    }
    sc->acc.set(f.prm, A.last_chunk ? 0u : s0 + ns, f.tiled);
}

unsigned long long counter_sum(const crt_scene* sc, int c)
{
    unsigned long long v = 0;
    for (int s = 0; s < CNT_SHARDS; s++) v += sc->h_counters[s * CNT_STRIDE + c];
    return v;
}

// crt_stats from the pinned copy of the counters; `mega`: the counters only k_mega3 keeps (rays_untraced, phase_cycles)
void read_stats(const crt_scene* sc, crt_stats* stats, bool mega, double kernel_ms, double logic_ms, float total_ms, uint32_t launches)
{
    std::memset(stats, 0, sizeof(*stats));
    stats->paths = counter_sum(sc, C_PATHS); stats->rays = counter_sum(sc, C_RAYS); stats->shadow_rays = counter_sum(sc, C_SHADOW);
    stats->probe_rays = counter_sum(sc, C_PROBE);
    stats->inner_pops = counter_sum(sc, C_INNER); stats->leaf_pops = counter_sum(sc, C_LEAF); stats->tri_tests = counter_sum(sc, C_TESTS);
    stats->hits = counter_sum(sc, C_HITS);
    stats->stack_sum = counter_sum(sc, C_SUMSP);
    for (int sh2 = 0; sh2 < CNT_SHARDS; sh2++) stats->stack_max = std::max<uint64_t>(stats->stack_max, sc->h_counters[sh2 * CNT_STRIDE + C_MAXSP]);
    if (mega) {
        stats->rays_untraced = counter_sum(sc, C_UNTRACED);
        stats->phase_cycles[0] = counter_sum(sc, C_CYC_LOGIC); stats->phase_cycles[1] = counter_sum(sc, C_CYC_LEAF);
        stats->phase_cycles[2] = counter_sum(sc, C_CYC_INNER); stats->phase_cycles[3] = counter_sum(sc, C_CYC_OTHER);
        for (int i = 0; i < 20; i++) stats->phase_cycles[4 + i] = counter_sum(sc, C_DIAG + i);
    }
    stats->kernel_ms = (float)kernel_ms;
    stats->logic_ms = (float)logic_ms;
    stats->total_ms = total_ms;
    stats->kernel_launches = launches;
}

// ---- commit ring (megakernel only, CRT_FLAG_BOUNDED_RADIANCE): radiance storage for a window of samples, the sum
// c += L_k / spp made inside the launch; the whole sample range is then ONE launch.  ring samples = 4 x the depth of the work in
// flight (pool slots / pixel slots), at least 32: a shard is held back only when one of its paths takes four times as long as
// the rest of the pool.  samples == 0: no ring for this call.
RingPlan plan_ring(const crt_scene* sc, const crt_params* prm, const Shard& sh, uint32_t s_count, bool mega, bool want_stats, bool want_var)
{
    RingPlan ring;
    std::memset(&ring, 0, sizeof(ring));
    if (!mega || want_stats || want_var) return ring; // (CRT_FLAG_VARIANCE squares the per-path radiance, which the ring does not keep; want_var: or CRT_FLAG_PIXEL_FILTER, which reads it too)
    // cursor shards: the commits of a shard are a serial chain (one wave, a memory round trip per 256 pixel slots), so a ring
    // launch has more and smaller shards than the 64 of a launch without: about 1 024 pixel slots each, at most 1 024 shards
    uint32_t shards = ITEM_SHARDS;
    while (shards < 1024u && sh.nslots / (shards * 2u) >= 1024u) shards *= 2u;
    const uint32_t spsh = ((sh.nslots + shards - 1) / shards + 63u) & ~63u;
    const uint64_t pool_slots = (uint64_t)sc->n_cus * 16u * (uint64_t)POOL3_P;
    uint32_t rs = 32;
    while (rs < 65536u && (uint64_t)rs * sh.nslots < 4ull * pool_slots) rs <<= 1;
    const uint32_t forced = env_u32("CRT_COMMIT_RING_LOG2", 0); // (test hook: a ring of 2^n samples, with or without the flag)
    if (forced) rs = 1u << std::min(16u, forced);
    const uint64_t per_shard = (uint64_t)spsh * s_count;
    const bool fits32 = per_shard * shards < 0xffffffffull;
    if ((forced || (prm->flags & CRT_FLAG_BOUNDED_RADIANCE)) && rs < s_count && fits32) { ring.samples = rs; ring.spsh = spsh; ring.shards = shards; }
    return ring;
}

// ---- the order of a launch's last work items (k_order_items): the window and the classes, chosen by measurement on C2
// (docs/experiments.md, "The order of a launch's last paths") ----
constexpr uint32_t kOrderWindow = 1u << 19; // work items at the end of every cursor shard
// CRT_ORDER_CLASSES: the lower bounds of the classes above the first, ascending roulette lengths from 2 on, at most seven ("2": the paths
// that stop at their first vertex last and nothing more).  Anything else: the default.
OrderClasses order_classes_from_env()
{
    OrderClasses C;
    std::memset(&C, 0, sizeof(C));
    const uint32_t dflt[] = {1, 2, 3, 5, 9};
    C.n = (uint32_t)(sizeof(dflt) / sizeof(dflt[0]));
    for (uint32_t c = 0; c < C.n; c++) C.lo[c] = dflt[c];
    const char* e = std::getenv("CRT_ORDER_CLASSES");
    if (!e || !*e) return C;
    OrderClasses E;
    std::memset(&E, 0, sizeof(E));
    E.n = 1; E.lo[0] = 1;
    for (const char* p = e; *p;) {
        char* end = nullptr;
        const long v = std::strtol(p, &end, 10);
        if (end == p || E.n == ORDER_CLASSES_MAX || v <= (long)E.lo[E.n - 1] || v > CRT_BOUNCE_STACK_SIZE) return C;
        E.lo[E.n++] = (uint32_t)v;
        p = end;
        if (*p == ',') p++;
        else if (*p) return C;
    }
    return E.n >= 2 ? E : C;
}

// ---------- fused persistent megakernel: one launch per chunk ----------
void render_mega(Frame& f)
{
    crt_scene* sc = f.sc;
    const crt_params* prm = f.prm;
    const Shard& sh = f.sh;
    const RingPlan& ring = f.ring;
    hipStream_t st = f.st;
    const bool timing = f.stats != nullptr;
    auto chunk_items = [&](uint32_t k, uint32_t ns) { return f.src ? f.src->items(k, ns) : (uint32_t)((uint64_t)ns * sh.nslots); };
    uint64_t most_items = ring.samples ? (uint64_t)(f.s_end - f.s_begin) * sh.nslots : f.cap;
    if (f.src) { // the largest chunk the source lists
        most_items = 0;
        for (uint32_t s0 = f.s_begin, k = 0; s0 < f.s_end; s0 += f.chunk, k++) most_items = std::max<uint64_t>(most_items, chunk_items(k, std::min(f.chunk, f.s_end - s0)));
    }
    const MegaPlan mp = plan_mega3(sc, prm->traversal, f.want_stats, (prm->flags & CRT_FLAG_TRACE_ALL) != 0, false, ring.samples != 0, most_items, env_u32("CRT_MEGA_BLOCKS_PER_CU", 64));
    const uint32_t lanes = mp.lanes;
    sc->p_vx.ensure(lanes); sc->p_la.ensure(lanes); sc->p_cc.ensure(lanes); sc->p_id.ensure(lanes);
    sc->p_rec_a.ensure((size_t)lanes * CRT_BOUNCE_STACK_SIZE);
    sc->p_rec_b.ensure((size_t)lanes * CRT_BOUNCE_STACK_SIZE);
    sc->p_rec_c.ensure((size_t)lanes * CRT_BOUNCE_STACK_SIZE);
    sc->spill[0].ensure(mp.spill_entries);
    LParams P = frame_lparams(f);
    P.pool.vx = sc->p_vx.p; P.pool.la = sc->p_la.p; P.pool.cc = sc->p_cc.p; P.pool.vn = sc->p_vn.p; P.pool.id = sc->p_id.p;
    P.pool.rec_a = sc->p_rec_a.p; P.pool.rec_b = sc->p_rec_b.p; P.pool.rec_c = sc->p_rec_c.p; P.pool.n = lanes;
    MParams M;
    std::memset(&M, 0, sizeof(M));
    M.sc = sc->dev; M.counters = sc->counters.p; M.spill = sc->spill[0].p; M.spill_stride = lanes; M.stack_cap = mp.lds_levels;
    // A timed frame: one event pair around every chunk's launch (crt_scene::ev_chunk), read after the frame's one synchronisation below --
    // the stream is never waited for between a launch and its fold
    hipEvent_t e0 = nullptr, e3 = nullptr;
    if (timing) {
        ensure_chunk_events(sc, (f.s_end - f.s_begin + f.chunk - 1) / f.chunk);
        e0 = sc->ev[0]; e3 = sc->ev[3];
        HIP_CHECK(hipEventRecord(e0, st));
    }
    uint32_t launches = 0;
    for (uint32_t s0 = f.s_begin; s0 < f.s_end; s0 += f.chunk) {
        uint32_t ns = std::min(f.chunk, f.s_end - s0);
        set_chunk(P, s0, chunk_items(launches, ns));
        if (ring.samples) { // cursor shard = ring.spsh pixel slots x ns samples
            P.items_per_shard = ring.spsh * ns;
            P.n_items = P.items_per_shard * ring.shards;
            P.ring_mask = ring.samples - 1u; P.spsh = ring.spsh; P.spsh_div = make_fastdiv(ring.spsh); P.ring_shards = ring.shards;
            P.ring_stride = ring.spsh * ring.shards; P.n_samples = ns; P.tail_first = P.items_per_shard; P.spp_f = (float)prm->spp;
            sc->ring_done.ensure_uncached((size_t)ring.shards * ring.samples);
            sc->ring_state.ensure_uncached((size_t)ring.shards * ITEM_STRIDE);
            P.ring_done = sc->ring_done.p; P.ring_state = sc->ring_state.p; P.accum = sc->accum.p; P.L = sc->ring_L.p;
            std::vector<unsigned int>& state = sc->ring_state_host; // (a member: the copy below may still read it after this scope)
            state.assign((size_t)ring.shards * ITEM_STRIDE, 0u);
            // word 1: the pixel slots of the shard that are pixels (ring.spsh is a multiple of 64: a tile's slots lie in one shard)
            for (uint32_t lt = 0; lt < sh.local_tiles; lt++) state[(size_t)(lt * 64u / ring.spsh) * ITEM_STRIDE + 1] += tile_pixels(f.A, lt);
            HIP_CHECK(hipMemcpyAsync(sc->ring_state.p, state.data(), state.size() * sizeof(unsigned int), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemsetAsync(sc->ring_done.p, 0, (size_t)ring.shards * ring.samples * sizeof(unsigned int), st));
        }
        // the end of every cursor shard is handed out longest roulette length first (k_order_items, crt_item_order.h; the measurements:
        // docs/experiments.md, "The order of a launch's last paths").  CRT_ITEM_ORDER=0 switches it off.
        P.item_list = nullptr;
        sc->order_classes = 0; sc->order_window = 0;
        if (f.src) {
            // the WHOLE cursor range goes through the source's list (order_window = the shard, so list index = cursor position)
            P.order_window = P.items_per_shard;
            sc->order_key.valid = 0; // (the source's list takes the buffer)
            sc->item_list.ensure(P.n_items);
            f.src->fill(sc->item_list.p, s0, ns, P.n_items, st);
            HIP_CHECK(hipGetLastError());
            P.item_list = sc->item_list.p;
        } else {
            const char* eo = std::getenv("CRT_ITEM_ORDER");
            const bool order = !(eo && eo[0] == '0');
            if (order && P.n_items > 0) {
                // the window: the last CRT_ORDER_WINDOW work items of every shard
                P.order_window = std::min<uint32_t>(P.items_per_shard, env_u32("CRT_ORDER_WINDOW", kOrderWindow));
                if (ring.samples) { // the window may span half the ring: its items stand for the launch's last sample at the gate, in whatever order
                    P.order_window = std::min<uint32_t>(P.order_window, (ring.samples / 2u) * ring.spsh);
                    P.tail_first = P.items_per_shard - P.order_window;
                }
                P.items_per_shard_div = make_fastdiv(std::max(1u, P.items_per_shard));
                const uint32_t n_sh = ring.samples ? ring.shards : (uint32_t)ITEM_SHARDS;
                const OrderClasses C = order_classes_from_env();
                // The list is a function of the key alone (crt_scene.h: ItemOrderKey), not of the camera or the scene: a launch whose key is the one the
                // handle's list was built for takes it as it is -- no memset, no order pass.  One list per handle: a frame of several chunks
                // builds one per chunk.
                ItemOrderKey key;
                std::memset(&key, 0, sizeof(key));
                key.valid = 1; key.seed = P.seed; key.stream = (uint64_t)(uintptr_t)st; key.sample_begin = P.sample_begin; key.n_items = P.n_items;
                key.items_per_shard = P.items_per_shard; key.order_window = P.order_window; key.shards = n_sh; key.ring = ring.samples ? 1u : 0u;
                key.spsh = ring.samples ? ring.spsh : 0u; key.nslots = P.nslots; key.rank = P.rank; key.world = P.world; key.tiles_x = P.tiles_x;
                key.n_tiles = P.n_tiles; key.width = P.width; key.height = P.height;
                std::memcpy(&key.p_rr_bits, &P.p_rr, sizeof(float));
                key.n_classes = C.n;
                for (uint32_t c = 0; c < C.n; c++) key.class_lo[c] = C.lo[c];
                const size_t list_n = (size_t)n_sh * P.order_window, cnt_n = (size_t)n_sh * C.n * 32;
                if (sc->item_list.n < list_n || sc->order_cnt.n < cnt_n) sc->order_key.valid = 0; // (a new allocation holds no list)
                sc->item_list.ensure(list_n);
                sc->order_cnt.ensure(cnt_n);
                if (std::memcmp(&key, &sc->order_key, sizeof(key)) == 0) sc->order_reused++;
                else {
                    sc->order_key.valid = 0;
                    HIP_CHECK(hipMemsetAsync(sc->order_cnt.p, 0, cnt_n * sizeof(unsigned int), st));
                    const uint32_t spans = (P.order_window + 1023u) / 1024u;
                    launch_order_items(ring.samples != 0, n_sh * spans, st, P, C, sc->item_list.p, sc->order_cnt.p);
                    HIP_CHECK(hipGetLastError());
                    sc->order_key = key;
                    sc->order_built++;
                }
                P.item_list = sc->item_list.p;
                sc->order_classes = C.n; sc->order_window = P.order_window;
            }
        }
        P.items_per_shard_div = make_fastdiv(std::max(1u, P.items_per_shard));
        M.P = P;
        HIP_CHECK(hipMemsetAsync(sc->item_next.p, 0, (size_t)(ring.samples ? ring.shards : (uint32_t)ITEM_SHARDS) * ITEM_STRIDE * sizeof(unsigned int), st));
        if (timing) HIP_CHECK(hipEventRecord(sc->ev_chunk[2 * launches], st));
        if (s0 == f.s_begin) HIP_CHECK(hipEventRecord(sc->ev_k0, st));
        {
            MParams3 M3;
            M3.M = M;
            M3.spill = (int*)sc->spill[0].p; // (one word per entry; the buffer is sized for the two-word entries of k_trace)
            M3.force_exact = (prm->flags & CRT_FLAG_FORCE_EXACT) ? 1u : 0u;
            M3.dbg_loads = 0; M3.dbg_valu = 0;
            if (!bbprof_launch(mp.kern, M3, mp.blocks, st)) hipLaunchKernelGGL(mp.kern, dim3(mp.blocks), dim3(64), 0, st, M3);
        }
        HIP_CHECK(hipGetLastError());
        if (s0 + ns >= f.s_end) HIP_CHECK(hipEventRecord(sc->ev_k1, st));
        if (timing) HIP_CHECK(hipEventRecord(sc->ev_chunk[2 * launches + 1], st));
        launches++;
        sc->last_launches = launches;
        accumulate_chunk(f, s0, ns);
    }
    if (f.stats) {
        HIP_CHECK(hipEventRecord(e3, st));
        HIP_CHECK(hipMemcpyAsync(sc->h_counters, sc->counters.p, kCountersBytes, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        double kernel_ms = 0.0;
        for (uint32_t c = 0; c < launches; c++) {
            float ms = 0.0f;
            HIP_CHECK(hipEventElapsedTime(&ms, sc->ev_chunk[2 * c], sc->ev_chunk[2 * c + 1]));
            kernel_ms += ms;
        }
        float total = 0.0f;
        HIP_CHECK(hipEventElapsedTime(&total, e0, e3));
        read_stats(sc, f.stats, true, kernel_ms, 0.0, total, launches);
    }
}

// ---------- the wavefront pipeline: rounds of k_logic + k_trace over a pool of paths, in batches, until no slot emits a ray ----------
void render_wavefront(Frame& f)
{
    crt_scene* sc = f.sc;
    const crt_params* prm = f.prm;
    const Shard& sh = f.sh;
    hipStream_t st = f.st;
    const bool timing = f.stats != nullptr;
    const uint32_t pool_log2 = std::min(26u, std::max(8u, env_u32("CRT_POOL_LOG2", 22)));
    const uint32_t pool_n = (uint32_t)std::min<uint64_t>((f.cap + 255) / 256 * 256, 1ull << pool_log2);
    const int batch_max = (int)std::min<uint32_t>(kMaxBatch, env_u32("CRT_ROUND_BATCH", 16));
    int batch = batch_max;
    unsigned long long alive_seen = 0;
    // The pool is split into halves that run on two streams: the HBM-bound k_logic of one half
    // overlaps the issue-bound k_trace of the other.
    const int n_halves = (pool_n >= 2 * 65536u && env_u32("CRT_STREAMS", 2) >= 2) ? 2 : 1;
    const uint32_t half_n = n_halves == 2 ? ((pool_n / 2 + 255) / 256 * 256) : pool_n;
    const size_t slots = (size_t)half_n * n_halves;
    sc->p_ro.ensure(slots); sc->p_rd.ensure(slots); sc->p_vx.ensure(slots); sc->p_la.ensure(slots); sc->p_cc.ensure(slots); sc->p_res.ensure(slots);
    sc->p_vn.ensure(slots); sc->p_id.ensure(slots);
    sc->p_rec_a.ensure(slots * CRT_BOUNCE_STACK_SIZE);
    sc->p_rec_b.ensure(slots * CRT_BOUNCE_STACK_SIZE);
    Pool pools[2];
    for (int h = 0; h < n_halves; h++) {
        Pool& pool = pools[h];
        const size_t o = (size_t)h * half_n;
        pool.ro = sc->p_ro.p + o; pool.rd = sc->p_rd.p + o; pool.vx = sc->p_vx.p + o; pool.la = sc->p_la.p + o; pool.cc = sc->p_cc.p + o;
        pool.vn = sc->p_vn.p + o; pool.id = sc->p_id.p + o; pool.res = sc->p_res.p + o;
        pool.rec_a = sc->p_rec_a.p + o * CRT_BOUNCE_STACK_SIZE; pool.rec_b = sc->p_rec_b.p + o * CRT_BOUNCE_STACK_SIZE;
        pool.n = half_n;
    }
    hipStream_t streams[2] = {st, sc->aux_stream};
    LParams P = frame_lparams(f);
    const bool lds_tables = sc->n_mats <= LOGIC_TABLE_MAX && (uint32_t)sc->dev.n_lights <= LOGIC_TABLE_MAX;
    TraceSetup TS[2];
    LParams PH[2];
    for (int h = 0; h < n_halves; h++) TS[h] = make_trace_setup(sc, pools[h], prm->traversal, f.want_stats, h, n_halves);

    double trace_ms = 0.0, logic_ms = 0.0;
    uint32_t trace_launches = 0;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    if (timing) {
        ev_begin = sc->ev[4 * kMaxBatch + 2];
        ev_end = sc->ev[4 * kMaxBatch + 3];
        HIP_CHECK(hipEventRecord(ev_begin, st));
    }
    const dim3 pool_grid((half_n + 255) / 256);
    const int evs_per_half = 2 * kMaxBatch + 1;
    for (uint32_t s0 = f.s_begin; s0 < f.s_end; s0 += f.chunk) {
        uint32_t ns = std::min(f.chunk, f.s_end - s0);
        set_chunk(P, s0, (uint32_t)((uint64_t)ns * P.nslots));
        HIP_CHECK(hipMemsetAsync(sc->item_next.p, 0, (size_t)ITEM_SHARDS * ITEM_STRIDE * sizeof(unsigned int), st));
        for (int h = 0; h < n_halves; h++) {
            PH[h] = P;
            PH[h].pool = pools[h];
            launch_pool_init(pool_grid.x, st, pools[h]);
        }
        HIP_CHECK(hipGetLastError());
        for (;;) {
            if (n_halves == 2) { // fork: the second half's chain follows what is queued on st so far
                HIP_CHECK(hipEventRecord(sc->ev_fork, st));
                HIP_CHECK(hipStreamWaitEvent(sc->aux_stream, sc->ev_fork, 0));
            }
            for (int h = 0; h < n_halves; h++)
                if (timing) HIP_CHECK(hipEventRecord(sc->ev[h * evs_per_half], streams[h]));
            for (int b = 0; b < batch; b++) {
                for (int h = 0; h < n_halves; h++) {
                    hipStream_t hs = streams[h];
                    hipEvent_t* ev = sc->ev.data() + h * evs_per_half;
                    launch_logic(lds_tables, pool_grid.x, hs, PH[h]);
                    if (timing) HIP_CHECK(hipEventRecord(ev[2 * b + 1], hs));
                    launch_trace_pass(sc, TS[h], hs);
                    if (timing) HIP_CHECK(hipEventRecord(ev[2 * b + 2], hs));
                }
            }
            HIP_CHECK(hipGetLastError());
            if (n_halves == 2) { // join
                HIP_CHECK(hipEventRecord(sc->ev_join, sc->aux_stream));
                HIP_CHECK(hipStreamWaitEvent(st, sc->ev_join, 0));
            }
            HIP_CHECK(hipMemcpyAsync(sc->h_counters, sc->counters.p, kCountersBytes, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (timing) {
                double bl = 0.0, bt = 0.0;
                for (int h = 0; h < n_halves; h++) {
                    hipEvent_t* ev = sc->ev.data() + h * evs_per_half;
                    for (int b = 0; b < batch; b++) {
                        float a = 0.0f, c = 0.0f;
                        HIP_CHECK(hipEventElapsedTime(&a, ev[2 * b], ev[2 * b + 1]));
                        HIP_CHECK(hipEventElapsedTime(&c, ev[2 * b + 1], ev[2 * b + 2]));
                        bl += a; bt += c;
                    }
                }
                logic_ms += bl; trace_ms += bt;
                if (std::getenv("CRT_TRACE_LOG"))
                    fprintf(stderr, "[crt] rounds %u..%u: rays in batch %llu, logic %.3f ms, trace %.3f ms\n", trace_launches, trace_launches + batch - 1,
                            (unsigned long long)(counter_sum(sc, C_ALIVE) - alive_seen), bl, bt);
            }
            trace_launches += (uint32_t)(batch * n_halves);
            unsigned long long alive_now = counter_sum(sc, C_ALIVE);
            if (alive_now == alive_seen) break; // no slot emitted a ray during the whole batch: chunk done
            // once the pool runs dry (no more regeneration) check more often, so that few empty rounds are launched
            const unsigned long long per_round = (alive_now - alive_seen) / (unsigned long long)batch;
            batch = per_round * 8 < (unsigned long long)half_n * n_halves ? std::min(batch_max, 4) : batch_max;
            if (per_round * 512 < (unsigned long long)half_n * n_halves) batch = std::min(batch_max, 2);
            alive_seen = alive_now;
        }
        accumulate_chunk(f, s0, ns);
    }
    if (f.stats) {
        HIP_CHECK(hipEventRecord(ev_end, st));
        HIP_CHECK(hipStreamSynchronize(st));
        float total = 0.0f;
        HIP_CHECK(hipEventElapsedTime(&total, ev_begin, ev_end));
        read_stats(sc, f.stats, false, trace_ms, logic_ms, total, trace_launches);
    }
}

} // namespace

namespace crtk { // (declared in crt_render.h)

// Which pipeline renders: 4 = k_mega3 (the product), 2 = the wavefront pipeline (k_logic + k_trace).  k_mega3 keeps the best
// triangle's offset inside its leaf in 16 bits, addresses nodes and leaf records with 32-bit byte offsets and the traversal stack
// depth in 8 bits; scenes beyond any of these fall back to the wavefront pipeline, which has no such limits.  The CRT_TEST_*
// variables lower the limits so that the tests can force each fallback on a small scene.
uint32_t choose_pipeline(const crt_scene* sc)
{
    uint32_t pipeline = env_u32("CRT_PIPELINE", 4);
    if (pipeline != 2) pipeline = 4;
    const uint64_t max_leaf = env_u32("CRT_TEST_MAX_LEAF", CRT_MEGA3_MAX_LEAF);
    const uint64_t max_bytes = std::getenv("CRT_TEST_MAX_BYTES") ? (uint64_t)env_u32("CRT_TEST_MAX_BYTES", 0xffffffffu) : (1ull << 32);
    const uint32_t max_stack = env_u32("CRT_TEST_MAX_STACK", CRT_MEGA3_MAX_STACK);
    if (pipeline == 4 && sc->max_leaf > max_leaf) pipeline = 2;
    if (pipeline == 4 && (sc->nodes4.n * sizeof(float4) >= max_bytes || sc->nodes3.n * sizeof(float4) >= max_bytes || sc->leaf_geo.n * sizeof(float4) >= max_bytes))
        pipeline = 2; // (33 M nodes / 53 M records)
    if (pipeline == 4 && (uint32_t)sc->stack_cap > max_stack) pipeline = 2; // a deeper stack would spill into the flag bits of word D
    return pipeline;
}

// Samples per launch of a range of s_count samples without the commit ring: as many whole samples of every pixel slot as kMaxChunkItems
// paths hold, at least one
uint32_t chunk_samples(uint32_t nslots, uint32_t s_count)
{
    const uint64_t max_items = std::min<uint64_t>(kMaxChunkItems, 1ull << std::min(30u, env_u32("CRT_CHUNK_LOG2", 30))); // (test hook: small chunks)
    return (uint32_t)std::min<uint64_t>(s_count, std::max<uint64_t>(1, max_items / nslots));
}

// What `who` (crt_render and, through it, every call that renders a frame; the AOV passes) refuses in a crt_params by itself (no scene,
// no sample range), before any device call.  `camera_rays_only`: an AOV pass takes no next-event samples, and its pixel count is tested last.
int params_check(const char* who, const crt_params* prm, bool camera_rays_only)
{
    const std::string w(who);
    const bool too_many_pixels = (uint64_t)prm->width * prm->height > 0xffffffffull;
    if (prm->width == 0 || prm->height == 0 || prm->spp == 0) return fail(CRT_ERR_INVALID_ARG, w + ": width, height and spp must be positive");
    if (prm->world == 0 || prm->rank >= prm->world) return fail(CRT_ERR_INVALID_ARG, w + ": need rank < world");
    if (!camera_rays_only && (prm->light_sample_n < 0 || prm->light_sample_n > 4096)) return fail(CRT_ERR_INVALID_ARG, w + ": light_sample_n must be in [0, 4096]");
    if (!camera_rays_only && too_many_pixels) return fail(CRT_ERR_UNSUPPORTED, w + ": more than 2^32 pixels"); // (a render reports it here ...)
    if (prm->traversal != CRT_TRAVERSAL_FAST && prm->traversal != CRT_TRAVERSAL_REFERENCE && prm->traversal != CRT_TRAVERSAL_EXACT)
        return fail(CRT_ERR_INVALID_ARG, w + ": unknown traversal mode");
    if (prm->world > 1 && !(prm->flags & CRT_FLAG_TILED_OUTPUT)) return fail(CRT_ERR_INVALID_ARG, w + ": world > 1 needs CRT_FLAG_TILED_OUTPUT");
    if (too_many_pixels) return fail(CRT_ERR_UNSUPPORTED, w + ": more than 2^32 pixels"); // (... the AOV pass here: a render has returned above)
    return CRT_OK;
}

// CRT_FLAG_PIXEL_FILTER: whether a range that begins at sample s_begin continues a frame whose filter sums are on the handle
static bool pixel_filter_continues(const crt_scene* sc, const crt_params* prm, uint32_t s_begin)
{
    return s_begin > 0 && sc->pf_mark.valid && continues_frame(sc->pf_mark, prm, s_begin, (prm->flags & CRT_FLAG_TILED_OUTPUT) != 0);
}
// What a render call with CRT_FLAG_PIXEL_FILTER refuses (contract: include/crt.h), before any device call -- the host forms ask before
// they stage their buffers, render_impl asks again
static int pixel_filter_check(const crt_scene* sc, const crt_params* prm, uint32_t s_begin)
{
    if (!sc->pf_set) return fail(CRT_ERR_INVALID_ARG, "crt_render: CRT_FLAG_PIXEL_FILTER with no filter on the handle (crt_set_pixel_filter)");
    if (prm->world > 1) return fail(CRT_ERR_UNSUPPORTED, "crt_render: CRT_FLAG_PIXEL_FILTER with world > 1 (a shard does not hold its pixels' neighbours)");
    if (pixel_filter_continues(sc, prm, s_begin) && (sc->pf_frame.kind != sc->pf.kind || std::memcmp(&sc->pf_frame.radius, &sc->pf.radius, sizeof(float)) != 0))
        return fail(CRT_ERR_INVALID_ARG, "crt_render_range: a range with sample_begin " + std::to_string(s_begin) + " and CRT_FLAG_PIXEL_FILTER must keep the filter of the frame "
                                         "in flight (kind " + std::to_string(sc->pf_frame.kind) + ", radius " + std::to_string(sc->pf_frame.radius) + "); the handle's is kind " +
                                         std::to_string(sc->pf.kind) + ", radius " + std::to_string(sc->pf.radius));
    return CRT_OK;
}

// Renders samples [s_begin, s_begin + s_count) of the prm->spp samples per pixel into the scene's accumulator
// (temp_color += L_k / spp in sample order, Render.cuh:348); the range that ends at spp also tone-maps and writes the frame.
// src, open: crt_render.h.
int render_impl(crt_scene* sc, const crt_camera* cam, const crt_params* prm, void* d_rgb, void* d_mean, hipStream_t st, crt_stats* stats, uint32_t s_begin,
                uint32_t s_count, const ItemSource* src, bool open)
{
    if (!sc || !cam || !prm) return fail(CRT_ERR_INVALID_ARG, "crt_render: null argument");
    if (s_count == 0xffffffffu) s_count = prm->spp > s_begin ? prm->spp - s_begin : 0;
    if (s_count == 0 || (uint64_t)s_begin + s_count > prm->spp) return fail(CRT_ERR_INVALID_ARG, "crt_render: sample range outside [0, spp)");
    const uint32_t s_end = s_begin + s_count;
    if (!d_rgb && s_end == prm->spp && !open) return fail(CRT_ERR_INVALID_ARG, "crt_render: null frame buffer");
    const int rc_prm = params_check("crt_render", prm);
    if (rc_prm != CRT_OK) return rc_prm;
    // CRT_FLAG_HALF_BUFFERS implies CRT_FLAG_VARIANCE: from here on the call is one with both
    crt_params prm_both;
    if (prm->flags & CRT_FLAG_HALF_BUFFERS) {
        prm_both = *prm;
        prm_both.flags |= CRT_FLAG_VARIANCE;
        prm = &prm_both;
    }
    Frame f;
    f.sc = sc; f.cam = cam; f.prm = prm; f.st = st; f.stats = stats; f.s_begin = s_begin; f.s_end = s_end; f.src = src; f.open = open;
    f.want_stats = (prm->flags & CRT_FLAG_STATS) != 0;
    f.tiled = (prm->flags & CRT_FLAG_TILED_OUTPUT) != 0;
    f.want_var = (prm->flags & CRT_FLAG_VARIANCE) != 0;
    f.want_half = (prm->flags & CRT_FLAG_HALF_BUFFERS) != 0 && !src; // (a sparse frame keeps no halves)
    if ((uint64_t)sc->dev.n_lights * (uint64_t)prm->light_sample_n > 0xffffu) return fail(CRT_ERR_UNSUPPORTED, "crt_render: more than 65535 next-event samples per vertex");
    // CRT_FLAG_PIXEL_FILTER (a sparse frame keeps no filter sums: crt_sparse.hip clears the flag)
    const bool want_pf = (prm->flags & CRT_FLAG_PIXEL_FILTER) != 0 && !src;
    const int rc_pf = want_pf ? pixel_filter_check(sc, prm, s_begin) : CRT_OK;
    if (rc_pf != CRT_OK) return rc_pf;
    const bool pf_continues = want_pf && pixel_filter_continues(sc, prm, s_begin);
    // a range that does not start a frame adds to the accumulator: it must hold exactly the samples before the range, of this frame
    if (s_begin > 0 && !continues_frame(sc->acc, prm, s_begin, f.tiled)) {
        const std::string have = sc->acc.in_flight(" at " + std::to_string(sc->acc.width) + " x " + std::to_string(sc->acc.height) + ", rank " + std::to_string(sc->acc.rank) +
                                                   " of " + std::to_string(sc->acc.world) + (sc->acc.tiled ? ", tiled" : ", row-major"));
        return fail(CRT_ERR_INVALID_ARG, "crt_render_range: a range with sample_begin " + std::to_string(s_begin) + " must continue the frame in flight: expected sample_begin == samples accumulated "
                                         "and the same spp, width, height, rank, world and CRT_FLAG_TILED_OUTPUT as its earlier ranges, or sample_begin 0 to start over (" + have + ")");
    }
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        f.sh = make_shard(prm->width, prm->height, prm->world);
        f.chunk = chunk_samples(f.sh.nslots, s_count);
        f.cap = (uint64_t)f.chunk * f.sh.nslots;
        const bool mega = choose_pipeline(sc) == 4;
        f.ring = plan_ring(sc, prm, f.sh, s_count, mega, f.want_stats, f.want_var || want_pf);
        if (f.ring.samples) {
            f.chunk = s_count;
            f.cap = (uint64_t)f.ring.samples * f.ring.spsh * f.ring.shards;
            sc->ring_L.ensure_uncached(f.cap);
            f.L = nullptr;
        } else f.L = sc->L.radiance(f.cap);
        sc->last_radiance_bytes = f.cap * sizeof(Rad3);
        sc->last_ring_samples = f.ring.samples;
        sc->accum.ensure_uncached((size_t)f.sh.nslots * 3); // (always uncached: a progressive render may switch between launches with and without the ring)
        // the variance sums: valid from a range that starts at sample 0 with the flag, through ranges that continue that frame with it
        f.var_frame = f.want_var && (s_begin == 0 || (sc->var.valid && continues_frame(sc->var, prm, s_begin, f.tiled)));
        sc->var.valid = false;
        if (f.want_var) sc->accum_q.ensure_uncached((size_t)f.sh.nslots * 3);
        // the half sums: by the same rule
        f.half_frame = f.want_half && (s_begin == 0 || (sc->half.valid && continues_frame(sc->half, prm, s_begin, f.tiled)));
        sc->half.valid = false;
        if (f.want_half) sc->accum_h.ensure_uncached((size_t)f.sh.nslots * 6);
        // the filter's sums: by the same rule
        f.pf_frame = want_pf && (s_begin == 0 || pf_continues);
        sc->pf_mark.valid = false;
        if (f.pf_frame) sc->accum_pf.ensure_uncached((size_t)f.sh.nslots * 4);
        FrameMark frame;
        frame.set(prm, 0, f.tiled);
        f.A = frame_aparams(sc, frame, f.sh);
        f.A.L = f.L;
        f.A.out_rgb = (uint8_t*)d_rgb; f.A.out_mean = (float*)d_mean;
        if (stats) ensure_events(sc);
        HIP_CHECK(hipMemsetAsync(sc->counters.p, 0, kCountersBytes, st));
        if (mega) render_mega(f);
        else render_wavefront(f);
        return CRT_OK;
    });
}

} // namespace crtk

extern "C" {

int crt_render_device(crt_scene* sc, const crt_camera* cam, const crt_params* prm, void* d_rgb, void* d_mean, void* stream, crt_stats* stats)
{
    return render_impl(sc, cam, prm, d_rgb, d_mean, (hipStream_t)stream, stats);
}

int crt_render(crt_scene* sc, const crt_camera* cam, const crt_params* prm, uint8_t* out_rgb, float* out_mean, crt_stats* stats)
{
    if (!sc || !prm || !out_rgb) return fail(CRT_ERR_INVALID_ARG, "crt_render: null argument");
    if (prm->world == 0 || prm->rank >= prm->world || prm->width == 0 || prm->height == 0) return fail(CRT_ERR_INVALID_ARG, "crt_render: bad shard or size");
    if (prm->flags & CRT_FLAG_PIXEL_FILTER) {
        const int rc_pf = pixel_filter_check(sc, prm, 0);
        if (rc_pf != CRT_OK) return rc_pf;
    }
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        Staging s(out_pixels(prm->width, prm->height, prm->world, (prm->flags & CRT_FLAG_TILED_OUTPUT) != 0), true, out_mean != nullptr);
        int rc = render_impl(sc, cam, prm, s.rgb.p, s.f32.p, nullptr, stats);
        if (rc != CRT_OK) return rc;
        s.download(out_rgb, out_mean);
        return CRT_OK;
    });
}

int crt_render_range_device(crt_scene* sc, const crt_camera* cam, const crt_params* prm, uint32_t sample_begin, uint32_t sample_count,
                            void* d_rgb, void* d_mean, void* stream, crt_stats* stats)
{
    if (sample_count == 0xffffffffu) return fail(CRT_ERR_INVALID_ARG, "crt_render_range: bad sample count");
    return render_impl(sc, cam, prm, d_rgb, d_mean, (hipStream_t)stream, stats, sample_begin, sample_count);
}

int crt_render_range(crt_scene* sc, const crt_camera* cam, const crt_params* prm, uint32_t sample_begin, uint32_t sample_count,
                     uint8_t* out_rgb, float* out_mean, crt_stats* stats)
{
    if (!sc || !prm) return fail(CRT_ERR_INVALID_ARG, "crt_render_range: null argument");
    if (prm->world == 0 || prm->rank >= prm->world || prm->width == 0 || prm->height == 0) return fail(CRT_ERR_INVALID_ARG, "crt_render_range: bad shard or size");
    if (sample_count == 0xffffffffu || sample_count == 0 || (uint64_t)sample_begin + sample_count > prm->spp)
        return fail(CRT_ERR_INVALID_ARG, "crt_render_range: sample range outside [0, spp)");
    const bool last = sample_begin + sample_count == prm->spp;
    if (last && !out_rgb) return fail(CRT_ERR_INVALID_ARG, "crt_render_range: the range that ends at spp needs a frame buffer");
    if (prm->flags & CRT_FLAG_PIXEL_FILTER) {
        const int rc_pf = pixel_filter_check(sc, prm, sample_begin);
        if (rc_pf != CRT_OK) return rc_pf;
    }
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        Staging s(out_pixels(prm->width, prm->height, prm->world, (prm->flags & CRT_FLAG_TILED_OUTPUT) != 0), last, last && out_mean);
        int rc = render_impl(sc, cam, prm, s.rgb.p, s.f32.p, nullptr, stats, sample_begin, sample_count);
        if (rc != CRT_OK) return rc;
        s.download(last ? out_rgb : nullptr, last ? out_mean : nullptr);
        return CRT_OK;
    });
}

int crt_last_launch_ms(crt_scene* sc, float* ms, uint32_t* launches)
{
    if (!sc || !ms) return fail(CRT_ERR_INVALID_ARG, "crt_last_launch_ms: null argument");
    if (sc->last_launches == 0) return fail(CRT_ERR_INVALID_ARG, "crt_last_launch_ms: no frame has been rendered by the megakernel on this handle");
    hipError_t e = hipEventElapsedTime(ms, sc->ev_k0, sc->ev_k1);
    if (e != hipSuccess) return fail(CRT_ERR_HIP, std::string("crt_last_launch_ms: hipEventElapsedTime: ") + hipGetErrorString(e) + " (synchronize the stream first)");
    if (launches) *launches = sc->last_launches;
    return CRT_OK;
}

int crt_radiance_storage(crt_scene* sc, uint64_t* bytes, uint32_t* ring_samples)
{
    if (!sc || !bytes) return fail(CRT_ERR_INVALID_ARG, "crt_radiance_storage: null argument");
    *bytes = sc->last_radiance_bytes;
    if (ring_samples) *ring_samples = sc->last_ring_samples;
    return CRT_OK;
}

int crt_item_order(crt_scene* sc, crt_item_order_info* info)
{
    if (!sc || !info) return fail(CRT_ERR_INVALID_ARG, "crt_item_order: null argument");
    info->lists_built = sc->order_built; info->lists_reused = sc->order_reused;
    info->classes = sc->order_classes; info->window = sc->order_window;
    return CRT_OK;
}

int crt_variance_device(crt_scene* sc, void* d_var, void* stream, uint32_t* samples_done)
{
    const int rc = sums_check("crt_variance", sc, d_var);
    if (rc != CRT_OK) return rc;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        AParams A = frame_aparams(sc, sc->var, make_shard(sc->var.width, sc->var.height, sc->var.world));
        A.out_mean = (float*)d_var;
        launch_variance(A, sc->accum_q.p, (float)sc->var.samples, (float)sc->var.spp, (hipStream_t)stream);
        HIP_CHECK(hipGetLastError());
        if (samples_done) *samples_done = sc->var.samples;
        return CRT_OK;
    });
}

int crt_variance(crt_scene* sc, float* out_var, uint32_t* samples_done)
{
    const int rc0 = sums_check("crt_variance", sc, out_var);
    if (rc0 != CRT_OK) return rc0;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        Staging s(out_pixels(sc->var.width, sc->var.height, sc->var.world, sc->var.tiled != 0), false, true);
        const int rc = crt_variance_device(sc, s.f32.p, nullptr, samples_done);
        if (rc != CRT_OK) return rc;
        s.download(nullptr, out_var);
        return CRT_OK;
    });
}

int crt_half_buffers_device(crt_scene* sc, void* d_a, void* d_b, void* stream, uint32_t* samples_done)
{
    const int rc = halves_check("crt_half_buffers", sc, d_a, d_b);
    if (rc != CRT_OK) return rc;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        const AParams A = frame_aparams(sc, sc->half, make_shard(sc->half.width, sc->half.height, sc->half.world));
        const uint32_t n = sc->half.samples;
        const float fs = (float)sc->half.spp;
        launch_half_buffers(A, sc->accum_h.p, (float*)d_a, (float*)d_b, fs / (float)((n + 1) / 2), fs / (float)(n / 2), (hipStream_t)stream);
        HIP_CHECK(hipGetLastError());
        if (samples_done) *samples_done = n;
        return CRT_OK;
    });
}

int crt_half_buffers(crt_scene* sc, float* out_a, float* out_b, uint32_t* samples_done)
{
    const int rc0 = halves_check("crt_half_buffers", sc, out_a, out_b);
    if (rc0 != CRT_OK) return rc0;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        const uint64_t npix = out_pixels(sc->half.width, sc->half.height, sc->half.world, sc->half.tiled != 0);
        Staging sa(npix, false, out_a != nullptr), sb(npix, false, out_b != nullptr);
        const int rc = crt_half_buffers_device(sc, sa.f32.p, sb.f32.p, nullptr, samples_done);
        if (rc != CRT_OK) return rc;
        if (out_a) sa.download(nullptr, out_a);
        if (out_b) sb.download(nullptr, out_b);
        return CRT_OK;
    });
}

int crt_preview_device(crt_scene* sc, void* d_rgb, void* d_mean, void* stream, uint32_t* samples_done)
{
    if (!sc || !d_rgb) return fail(CRT_ERR_INVALID_ARG, "crt_preview: null argument");
    if (sc->acc.samples == 0) return fail(CRT_ERR_INVALID_ARG, "crt_preview: no progressive render in flight (submit a range that ends before spp first)");
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        AParams A = frame_aparams(sc, sc->acc, make_shard(sc->acc.width, sc->acc.height, sc->acc.world));
        A.out_rgb = (uint8_t*)d_rgb; A.out_mean = (float*)d_mean;
        const float scale = (float)sc->acc.spp / (float)sc->acc.samples;
        launch_preview(A, scale, (hipStream_t)stream);
        HIP_CHECK(hipGetLastError());
        if (samples_done) *samples_done = sc->acc.samples;
        return CRT_OK;
    });
}

int crt_preview(crt_scene* sc, uint8_t* out_rgb, float* out_mean, uint32_t* samples_done)
{
    if (!sc || !out_rgb) return fail(CRT_ERR_INVALID_ARG, "crt_preview: null argument");
    if (sc->acc.samples == 0) return fail(CRT_ERR_INVALID_ARG, "crt_preview: no progressive render in flight (submit a range that ends before spp first)");
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        Staging s(out_pixels(sc->acc.width, sc->acc.height, sc->acc.world, sc->acc.tiled != 0), true, out_mean != nullptr);
        int rc = crt_preview_device(sc, s.rgb.p, s.f32.p, nullptr, samples_done);
        if (rc != CRT_OK) return rc;
        s.download(out_rgb, out_mean);
        return CRT_OK;
    });
}

int crt_intersect(crt_scene* sc, uint32_t n, const float* origins, const float* dirs, uint32_t traversal, int32_t* out_tri, float* out_t)
{
    if (!sc || !origins || !dirs || !out_tri || !out_t) return fail(CRT_ERR_INVALID_ARG, "crt_intersect: null argument");
    const bool raw_dir = (traversal & CRT_INTERSECT_RAW_DIRECTIONS) != 0;
    const bool force_exact = (traversal & CRT_INTERSECT_FORCE_EXACT) != 0;
    const bool any_hit = (traversal & CRT_INTERSECT_VISIBILITY) != 0;
    traversal &= ~(uint32_t)(CRT_INTERSECT_RAW_DIRECTIONS | CRT_INTERSECT_FORCE_EXACT | CRT_INTERSECT_VISIBILITY);
    if (traversal != CRT_TRAVERSAL_FAST && traversal != CRT_TRAVERSAL_REFERENCE && traversal != CRT_TRAVERSAL_EXACT)
        return fail(CRT_ERR_INVALID_ARG, "crt_intersect: unknown traversal mode");
    if (n == 0) return CRT_OK;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(sc->device));
        DevBuf<float> o, d, lim;
        o.upload(origins, n * 3ull); d.upload(dirs, n * 3ull);
        if (any_hit) lim.upload(out_t, n);
        // blocked() of Render.cuh:19-27 from a finished visibility ray (limit = out_t[i] on entry): shadow_blocked (crt_path.h)
        const bool reference_mode = traversal == CRT_TRAVERSAL_REFERENCE;
        auto answer = [&](uint32_t i, float T, int32_t tri) {
            if (!any_hit) { out_t[i] = T; out_tri[i] = tri; return; }
            const float tl = out_t[i];
            const bool blocked = reference_mode ? shadow_blocked<1>(tl, T, tri) : shadow_blocked<0>(tl, T, tri);
            out_t[i] = blocked ? 1.0f : 0.0f;
            out_tri[i] = blocked ? tri : -1;
        };
        sc->p_ro.ensure(n); sc->p_rd.ensure(n); sc->p_res.ensure(n);
        Pool pool;
        std::memset(&pool, 0, sizeof(pool));
        pool.ro = sc->p_ro.p; pool.rd = sc->p_rd.p; pool.res = sc->p_res.p; pool.n = n;
        launch_fill_rays(pool, n, o.p, d.p, raw_dir, lim.p);
        HIP_CHECK(hipGetLastError());
        uint32_t stride = 0;
        const float* d_res = trace_queries(sc, n, traversal, force_exact, nullptr, stride);
        HIP_CHECK(hipDeviceSynchronize());
        std::vector<float> res((size_t)n * stride);
        HIP_CHECK(hipMemcpy(res.data(), d_res, res.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; i++) {
            int32_t tri;
            std::memcpy(&tri, &res[(size_t)i * stride + 1], 4);
            answer(i, res[(size_t)i * stride], tri);
        }
        return CRT_OK;
    });
}

int crt_device_math(int device, const char* fn, uint32_t n, const float* a, const float* b, float* out)
{
    if (!fn || !a || !out) return fail(CRT_ERR_INVALID_ARG, "crt_device_math: null argument");
    static const char* names[] = {"sin", "cos", "tan", "acos", "atan2", "exp", "log10", "pow", "uniform", "sincos_s", "sincos_c", "div_short", "div_short_bounded"};
    int id = -1;
    for (int i = 0; i < 13; i++)
        if (std::strcmp(fn, names[i]) == 0) id = i;
    if (id < 0) return fail(CRT_ERR_INVALID_ARG, std::string("crt_device_math: unknown function ") + fn);
    if (n == 0) return CRT_OK;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(device));
        DevBuf<float> da, db, dout;
        da.upload(a, n); db.upload(b, n); dout.alloc(n);
        launch_math(id, n, da.p, db.p, dout.p);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        dout.download(out, n);
        return CRT_OK;
    });
}

int crt_device_philox(int device, uint32_t n, const uint32_t* ctr4, const uint32_t* key2, uint32_t* out4)
{
    if (!ctr4 || !key2 || !out4) return fail(CRT_ERR_INVALID_ARG, "crt_device_philox: null argument");
    if (n == 0) return CRT_OK;
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(device));
        DevBuf<uint32_t> c, k, o;
        c.upload(ctr4, n * 4ull); k.upload(key2, n * 2ull); o.alloc(n * 4ull);
        launch_philox(n, c.p, k.p, o.p);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        o.download(out4, n * 4ull);
        return CRT_OK;
    });
}

int crt_device_rcp_check(int device, uint64_t* mismatches, uint64_t* outside)
{
    if (!mismatches || !outside) return fail(CRT_ERR_INVALID_ARG, "crt_device_rcp_check: null argument");
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(device));
        DevBuf<unsigned long long> c;
        c.alloc(2);
        HIP_CHECK(hipMemset(c.p, 0, 2 * sizeof(unsigned long long)));
        launch_rcp_check(c.p);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        unsigned long long h[2];
        c.download(h, 2);
        *mismatches = h[0]; *outside = h[1];
        return CRT_OK;
    });
}

} // extern "C"
