/*
 * include/crt.h -- C ABI of libcrt.so, the MI355X-native drop-in for the
 * reference's rendering hot path.
 *
 * The reference (guomc9/CudaRayTracing) has no FFI layer: the boundary of the
 * hot path is the C++ class `Render` (reference: include/Render.cuh:357-557)
 * constructed from a `Scene*` and driven by `run_view` (src/main.cu:282,372).
 * Every entry point below names the reference interface it replaces.  All
 * signatures are plain C (pointers, sizes, PODs); no torch / HIP types.
 * All functions return CRT_OK (0) or a negative crt_status; nothing prints and
 * continues (the reference printf's CUDA errors and carries on,
 * Render.cuh:393-397,441-473).
 *
 * Threading: one host thread per scene handle; handles are not shared across
 * threads (the reference is single-threaded and not re-entrant either).
 */
#ifndef CRT_H
#define CRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: CRT_TRAVERSAL_* renumbered (0 = EXACT, the default of a zeroed crt_params; FAST moved to 2), crt_intersect's `traversal`
 *    argument carries flag bits (CRT_INTERSECT_RAW_DIRECTIONS 0x100, _FORCE_EXACT 0x200, _VISIBILITY 0x400), progressive /
 *    preview / multi-device / accel-info entry points and structs added.  A client built against version 2 must be rebuilt:
 *    check crt_abi_version() == CRT_ABI_VERSION at load time. */
#define CRT_ABI_VERSION 5

typedef enum {
    CRT_OK = 0,
    CRT_ERR_INVALID_ARG = -1,
    CRT_ERR_NO_DEVICE = -2,   /* no HIP device / HIP runtime failure at init (reference: src/main.cu:92-105) */
    CRT_ERR_HIP = -3,         /* a HIP call failed; see crt_last_error() */
    CRT_ERR_UNSUPPORTED = -4, /* valid for the reference but outside this build (e.g. a JPEG map_Kd texture) */
    CRT_ERR_IO = -5,          /* file missing / unreadable */
    CRT_ERR_PARSE = -6,       /* malformed OBJ / MTL / JSON */
    CRT_ERR_OOM = -7
} crt_status;

const char* crt_strerror(int status);
/* thread-local detail string of the last failure in this thread ("" if none) */
const char* crt_last_error(void);
int crt_abi_version(void);

/* ------------------------------------------------------------------------
 * Flat scene description handed to the device layer.
 * ---------------------------------------------------------------------- */

/* BVH node exactly as the reference uploads it (DeviceBVHNode,
 * include/DeviceBVH.cuh:9-15): post-order array, root = last; a node is a leaf
 * iff lc < 0 && rc < 0; leaf triangles are [it, it+n) of the BVH-ordered
 * triangle array. 40 bytes. */
typedef struct {
    int32_t lc, rc;
    uint32_t n;
    int32_t it;
    float aa[3];
    float bb[3];
} crt_bvh_node;

/* Triangle (reference DeviceTriangle, include/DeviceTriangle.cuh:12-37) with the
 * per-triangle material copy replaced by an index into crt_material[]. */
typedef struct {
    float v1[3], v2[3], v3[3];
    float normal[3];     /* geometric normal from winding (Triangle.h:27) */
    float area;          /* Triangle.h:39 */
    float area_of_obj;   /* Object.h:15-23 */
    int32_t material;
} crt_triangle;

/* reference DeviceMaterial (include/DeviceMaterial.cuh:5-37); ks/ka are never
 * read on the hot path and always zero (Loader.h:45,47,107). */
typedef struct {
    float kd[3];
    float ke[3];
    float ns;
    int32_t mode;      /* 0 = DIFFUSE, 1 = SPECULAR (Material.h:7-10) */
    int32_t has_emit;  /* Material.h:36-39 */
} crt_material;

/* One light object = a contiguous run of light_tris (reference DeviceLight,
 * include/DeviceLights.cuh:5-31: its own unsorted triangle copies). */
typedef struct {
    uint32_t first_tri;
    uint32_t count;
} crt_light;

typedef struct {
    const crt_bvh_node* nodes;     uint32_t n_nodes;  int32_t root;
    const crt_triangle* tris;      uint32_t n_tris;        /* BVH order */
    const crt_material* materials; uint32_t n_materials;
    const crt_triangle* light_tris; uint32_t n_light_tris;  /* shape order */
    const crt_light* lights;       uint32_t n_lights;
} crt_scene_desc;

typedef struct {
    float eye[3];
    float inv_view[9]; /* column-major 3x3 (Eigen::Matrix3f storage), from crt_inverse_view */
    float fov_y;       /* radians (src/main.cu:278) */
} crt_camera;

enum {
    CRT_TRAVERSAL_EXACT = 0,     /* THE DEFAULT (a zeroed crt_params): the 4-wide tree over the reference's leaves, nearest child first, any-hit
                                    visibility rays, zero-contribution samples answered without traversal -- every step of it provably
                                    result-neutral (docs/experiments.md 4.3), so the frame is REFERENCE's bit for bit (soak: 3.9e11 rays of
                                    full-size frames, 0 pixel slots differ) at 1/4 .. 1/6 of REFERENCE's time */
    CRT_TRAVERSAL_REFERENCE = 1, /* exhaustive traversal in the reference's visit order (DeviceBVH.cuh:128-170) */
    CRT_TRAVERSAL_FAST = 2       /* CRT_TRAVERSAL_EXACT plus distance pruning: skip a box entered beyond t_ref + 0.1 % + 1e-3 + 1e-4 x reach x steep
                                    (csrc/crt_trace.h; reach = max |origin coordinate| + t_ref, steep = max |1 / direction component|).  C2 -7 %,
                                    veach-mis -21 % frame time.  Exact unless a Moeller-Trumbore hit lies further in front of its own leaf box
                                    than that slack, which happens for rays lying in the plane of a triangle (det -> 0: unbounded error, and
                                    the reference has no determinant threshold).  MEASURED (tools/soak_fast_vs_reference.py,
                                    profiles/r02_soak_fast_vs_reference.jsonl): 2 rays in 3.66e11 on full 1920x1080x4096 veach-mis frames
                                    (tessellated spheres; each changes one next-event sample: the last bit of one pixel), 0 in 3.4e11 on full
                                    3840x2160x256 cornell-box frames; a larger slack only thins them out (docs/experiments.md 4.3).
                                    Bit-identical to REFERENCE on every frame and probe of the test-suite (two lost rays are kept as known
                                    answers in tests/test_adversarial_traversal.py); bench.py times it beside the default and re-checks a
                                    slice of the benchmark frame against REFERENCE in every run */
};
enum {
    CRT_FLAG_STATS = 1u,         /* fill the traversal counters of crt_stats (slower counting kernels) */
    CRT_FLAG_TILED_OUTPUT = 2u,  /* write this rank's pixels in compact 8x8-tile order instead of row-major */
    CRT_FLAG_TRACE_ALL = 8u,     /* CRT_TRAVERSAL_EXACT / _FAST trace every next-event sample, also those whose contribution is exactly
                                    zero (crt_stats.rays_untraced stays 0); same frame, for measuring the traversal alone */
    CRT_FLAG_FORCE_EXACT = 4u,   /* test hook: treat every ray of CRT_TRAVERSAL_FAST as one with non-finite operands (reference
                                    box arithmetic on the reference topology, still pruned / any-hit); results are unchanged */
    CRT_FLAG_BOUNDED_RADIANCE = 16u, /* keep the radiance of a WINDOW of samples instead of one value per path: the frame's sum c += L_k / spp
                                    (Render.cuh:348) is made in sample order inside the launch ("commit ring", docs/experiments.md section 9), the
                                    whole sample range is one launch whatever its size, and the handle needs 12 B x pixels x 32 ... 64
                                    samples (184 MB for 800x600) instead of 12 B per path (2.95 GB for 800x600 spp 512; 12.9 GB per 2^30 paths).
                                    Same bits.  Costs time (800x600 spp 512: 167 ms instead of 93): off by default -- memory is what this
                                    device has plenty of.  Ignored with CRT_FLAG_STATS, by the fallback pipeline, and when the sample range
                                    is no longer than the window, and switched off for the call by CRT_FLAG_VARIANCE (the ring keeps
                                    no per-path radiance to square: crt_radiance_storage then reports ring_samples = 0) */
    CRT_FLAG_VARIANCE = 32u,     /* keep, beside the frame's sum, the per-pixel sum of squares of the samples on the scene handle:
                                    crt_variance reads the variance of the frame's mean from it.  The frame is bit for bit the frame without
                                    the flag.  Switches the commit ring of CRT_FLAG_BOUNDED_RADIANCE (and of the CRT_COMMIT_RING_LOG2 test
                                    hook) off for the call, as CRT_FLAG_STATS does.  Cleared by crt_multi_render (it gathers no
                                    variance; crt_multi_render_buffers sets the flag itself when the VARIANCE plane is wanted) */
    CRT_FLAG_HALF_BUFFERS = 64u, /* keep, beside c and q, the sums of the even and of the odd samples of every pixel on the scene handle:
                                    crt_half_buffers reads two independent half-sample frames from them.  Implies CRT_FLAG_VARIANCE: the call
                                    behaves as if both were set (commit ring off included); frame, c and q are bit for bit those of
                                    CRT_FLAG_VARIANCE alone.  Cleared by crt_multi_render, as CRT_FLAG_VARIANCE is */
    CRT_FLAG_PIXEL_FILTER = 128u /* keep, beside whatever else the call keeps, the sums of the handle's pixel reconstruction filter
                                    (crt_set_pixel_filter): crt_filtered_frame reads the filtered frame from them.  The frame, c, q and the
                                    halves of the call are bit for bit those without the flag.  Switches the commit ring off for the call, as
                                    CRT_FLAG_VARIANCE does; implies no other flag.  One device only (world == 1).  Cleared by
                                    crt_multi_render and crt_multi_render_buffers; ignored by crt_render_adaptive, crt_render_map and
                                    crt_render_planned */
};

typedef struct {
    uint32_t width, height;      /* Scene::width/height (Scene.h:28-31) */
    uint32_t spp;                /* Render::spp (Render.cuh:362) */
    float p_rr;                  /* Render::P_RR */
    int32_t light_sample_n;      /* Render::light_sample_n */
    uint64_t seed;               /* replaces clock() (Render.cuh:341) */
    uint32_t rank, world;        /* pixel-tile shard: 8x8 tile t belongs to rank t % world; world >= 1 */
    uint32_t traversal;          /* CRT_TRAVERSAL_* */
    uint32_t flags;              /* CRT_FLAG_* */
} crt_params;

typedef struct {
    uint64_t paths;              /* W*H*spp of this shard */
    uint64_t rays;               /* closest-hit queries (= DeviceBVH::intersect calls) */
    uint64_t shadow_rays, probe_rays;
    uint64_t inner_pops, leaf_pops, tri_tests, hits; /* visit counters of the traversal that ran; CRT_FLAG_STATS only
                                                         (with CRT_TRAVERSAL_REFERENCE: the reference's visit set) */
    uint64_t stack_sum, stack_max;                   /* CRT_FLAG_STATS: sum / max over rays of the traversal stack high-water */
    uint64_t phase_cycles[24];                       /* reserved (zero): the per-phase cycle stamps of rounds 1-2 were replaced by the
                                                        basic-block profile of tools/bbprof */
    float kernel_ms;             /* sum of the HIP-event times of the render kernel's launches: k_mega3, one launch per chunk of at most
                                    2^30 work items (the wavefront fallback pipeline: the k_trace launches) */
    float logic_ms;              /* 0 for k_mega3 (the path logic is fused into it); the wavefront fallback: the k_logic launches */
    float total_ms;              /* HIP-event time of the whole device pipeline of this call (k_order_items, k_mega3, k_accumulate) */
    uint32_t kernel_launches;    /* number of k_mega3 (fallback: k_trace) launches */
    uint64_t rays_untraced;      /* of `shadow_rays`: next-event samples whose contribution is exactly zero (clamped cosine, black
                                    BSDF), answered without traversal by CRT_TRAVERSAL_EXACT / _FAST -- adding +0 cannot change L_dir;
                                    0 with CRT_FLAG_TRACE_ALL or CRT_TRAVERSAL_REFERENCE */
} crt_stats;

/* ------------------------------------------------------------------------
 * Device layer
 * ---------------------------------------------------------------------- */
typedef struct crt_scene crt_scene;

/* number of HIP devices visible (reference: config_CUDA, src/main.cu:92-105) */
int crt_device_count(int* count);

/* Upload a flat scene to `device` (replaces the DeviceBVH / DeviceLights /
 * DeviceTriangle / DeviceMaterial constructors, DeviceBVH.cuh:52-80,
 * DeviceLights.cuh:12-31,63-87, and the device half of Render's constructor,
 * Render.cuh:387-414).  The per-pixel stack allocations of Render.cuh:416-422
 * have no equivalent: traversal stacks live in LDS. */
int crt_scene_create(const crt_scene_desc* desc, int device, crt_scene** out);
/* How the acceleration trees of CRT_TRAVERSAL_FAST were built at crt_scene_create: a binned-SAH tree over the reference's leaves
 * (csrc/crt_accel.h; on the device by default, csrc/crt_accel_build.hip -- CRT_SAH_HOST=1 forces the host builder) collapsed to 4
 * children per node. */
typedef struct {
    uint32_t n_leaves, n_nodes2, n_nodes4, depth2, depth4;
    uint32_t sah_on_device;   /* 1: built by the device builder, 0: host builder (forced, or the device build could not run) */
    uint32_t index_splits;    /* ranges whose leaf centroids all coincide (duplicate leaves): split by index -- the only place where the
                                 device builder's tree may differ from the host builder's (equal leaves on different sides) */
    float sah_ms;             /* host clock: the whole SAH build (uploads and renumbering included) */
    float sah_device_ms;      /* HIP events around the level loop (0 for the host builder) */
    float runtime_init_ms;    /* host clock of crt_scene_create's first device calls (hipSetDevice, a 4-byte allocation and copy): the HIP
                                 runtime's one-off start in a process -- context creation, loading libcrt.so's code objects; about 150 ms
                                 for the first scene of a process, microseconds afterwards.  Not part of sah_ms. */
    uint32_t layout_caps;     /* which pool layouts of the render kernel the scene allows: bit 0 = node AND leaf refs fit 16-bit stack
                                 entries (coupled form, 8 LDS levels), bit 1 = the four-wide nodes alone do (decoupled leaves, 6 levels:
                                 what a scene of roughly 50 000 - 160 000 triangles renders with), bit 2 = leaf records fit a leaf-queue
                                 entry (decoupled leaves possible at all), bit 3 = the copy of the four-wide tree without its rows of refs
                                 exists (at most 32 768 nodes, leaves of one record -- bvh_thresh_n <= 2: six loads per inner visit instead of seven) */
} crt_accel_info;
int crt_scene_accel_info(crt_scene* scene, crt_accel_info* out);
/* replaces Render::free (Render.cuh:477-487) */
int crt_scene_destroy(crt_scene* scene);

/* Number of pixel slots a shard writes with CRT_FLAG_TILED_OUTPUT:
 * ceil(n_tiles_of_rank) * 64, n_tiles = ceil(W/8)*ceil(H/8). */
int crt_shard_slots(uint32_t width, uint32_t height, uint32_t rank, uint32_t world, uint64_t* slots);

/* Render one frame and copy it to host memory: replaces Render::run_view
 * (Render.cuh:435-475: kernel launch, synchronize, D2H copy; the OpenGL PBO
 * copy is dropped).  out_rgb: 3 bytes per pixel, row-major, row 0 = image top
 * (W*H*3 bytes, or slots*3 with CRT_FLAG_TILED_OUTPUT).  out_mean (optional,
 * may be NULL): pre-tone-map mean radiance, 3 floats per pixel, same order.
 * stats optional. */
int crt_render(crt_scene* scene, const crt_camera* cam, const crt_params* params, uint8_t* out_rgb,
               float* out_mean, crt_stats* stats);

/* Same, but outputs stay in device memory (d_rgb / d_mean are device pointers
 * on the scene's device, d_mean may be NULL) and the work is enqueued on
 * `hip_stream` (a hipStream_t, NULL = default stream) without synchronizing.
 * If stats != NULL the call synchronizes the stream to read counters/timers. */
int crt_render_device(crt_scene* scene, const crt_camera* cam, const crt_params* params, void* d_rgb,
                      void* d_mean, void* hip_stream, crt_stats* stats);

/* Device time of the render kernel launches of the LAST frame submitted on the handle (first launch's start to last launch's end, HIP
 * events recorded on the frame's stream without synchronizing): lets a caller that pipelines frames with crt_render_device(stats = NULL)
 * read every frame's kernel time afterwards.  The frame's stream must have been synchronized (CRT_ERR_HIP otherwise). */
int crt_last_launch_ms(crt_scene* scene, float* ms, uint32_t* launches);

/* Bytes of per-path radiance storage the handle's last render used, and the size of its commit ring in samples (0 = one radiance per
 * path of a chunk; otherwise one per pixel slot of a ring sample; 12 bytes each; see CRT_FLAG_BOUNDED_RADIANCE). */
int crt_radiance_storage(crt_scene* scene, uint64_t* bytes, uint32_t* ring_samples);

/* Progressive rendering (the reference re-renders all spp on every click, src/main.cu:368-377):
 * renders samples [sample_begin, sample_begin + sample_count) of params->spp into the accumulator the scene handle
 * owns (temp_color += L_k / spp, in sample order as Render.cuh:348).  Ranges must be submitted in ascending order
 * starting at 0, with the same camera / params, and no other render call on the handle in between; the range that
 * ends at spp tone-maps and writes out_rgb / out_mean -- bit-identical to one crt_render call.  For the other ranges
 * out_rgb / out_mean are not written and may be NULL.
 * A range with sample_begin == 0 always starts a frame over.  A range with sample_begin > 0 must continue the frame in flight on
 * the handle: sample_begin equals the number of samples accumulated so far, and spp, width, height, rank, world and
 * CRT_FLAG_TILED_OUTPUT are those of the frame's earlier ranges.  Anything else -- a first call with sample_begin > 0, a range after
 * a finished frame (crt_render* or the range that ended at spp), a gap, an overlap, another size, spp or shard -- would add to
 * sums that are uninitialised or belong to another frame, and is refused with CRT_ERR_INVALID_ARG before any device call
 * (crt_last_error names crt_render_range and what was expected).  A refused call leaves the handle as it was: the frame in flight
 * can still be previewed and continued.  Calls that do not touch the accumulator stay legal between ranges: crt_render_aov*,
 * crt_preview*, crt_variance*, crt_intersect, crt_denoise*.  Camera, seed, p_rr, light_sample_n and traversal are not recorded on
 * the handle and not checked: they must not change between the ranges of a frame. */
int crt_render_range(crt_scene* scene, const crt_camera* cam, const crt_params* params, uint32_t sample_begin,
                     uint32_t sample_count, uint8_t* out_rgb, float* out_mean, crt_stats* stats);
int crt_render_range_device(crt_scene* scene, const crt_camera* cam, const crt_params* params, uint32_t sample_begin,
                            uint32_t sample_count, void* d_rgb, void* d_mean, void* hip_stream, crt_stats* stats);

/* The displayable frame of a progressive render in flight -- the viewer half of SURVEY 8(f) row 4 (the reference shows nothing
 * until all spp are done and re-renders from scratch on every click, src/main.cu:368-377).  After a range that ends at
 * `done` < spp the accumulator holds sum_{k < done} L_k / spp; the preview is tone-map(accumulator * spp / done), written in the
 * layout of the range calls (row-major, or compact tiles with CRT_FLAG_TILED_OUTPUT).  Operation by operation, with S = spp of the
 * frame in flight and n = `done`, the samples accumulated:
 *   a     = the accumulator's value: c of the crt_variance contract below after samples 0 .. n-1 (c = c + L_k / (float)S from +0.0f)
 *   scale = (float)S / (float)n        one IEEE fp32 division
 *   p     = a * scale                  per channel: one IEEE fp32 multiply, no FMA -- neither (a * S) / n nor a * S * (1 / n)
 *   out_mean = p;  out_rgb = the frame's tone map of p
 * Padding slots of a tiled shard (slots of tiles beyond the frame, or of pixels beyond its right / bottom edge) are RGB 0 and mean
 * +0.0f; both forms write them (the device form writes every slot of d_rgb / d_mean itself).  It only READS the accumulator: the bits
 * of the final frame do not depend on whether, or how often, previews were taken.  *samples_done (optional) receives `done`.
 * crt_preview_device is enqueued on hip_stream (NULL = default stream) without synchronizing; the caller orders it after the
 * range calls (the same stream, or an event).  d_mean may be NULL and is then not touched.
 * CRT_ERR_INVALID_ARG, before any device call: a null scene or RGB buffer; no progressive render in flight (before the first range,
 * after the one that ends at spp). */
int crt_preview(crt_scene* scene, uint8_t* out_rgb, float* out_mean, uint32_t* samples_done);
int crt_preview_device(crt_scene* scene, void* d_rgb, void* d_mean, void* hip_stream, uint32_t* samples_done);

/* Per-pixel variance of the frame (CRT_FLAG_VARIANCE).  With the flag, crt_render, crt_render_device, crt_render_range and
 * crt_render_range_device keep, beside the frame's sum c, a second sum q per pixel slot and channel on the scene handle.  With
 * S = params->spp and x_k = L_k / (float)S (the quotient the frame adds, Render.cuh:348):
 *   c = c + x_k            (the frame; unchanged)
 *   q = q + x_k * x_k      from +0.0f, in sample order k = 0, 1, ...; one IEEE fp32 multiply and one add, no FMA
 * across chunks and progressive ranges exactly as c is carried.  crt_variance writes 3 floats per pixel in the layout of the render's
 * out_mean (row-major, or the compact tiles of the shard with CRT_FLAG_TILED_OUTPUT; padding slots +0.0f).  With n = samples accumulated
 * so far (n = S after the range that ends at spp; the buffer stays readable until the next render call on the handle), per channel:
 *   fn = (float)n;  fs = (float)S
 *   d  = fn * q - c * c;          d = d < 0.0f ? 0.0f : d        (NaN stays NaN)
 *   r  = fs / fn                                                  (exactly 1 for a finished frame)
 *   var = ((r * r) * d) / (fn - 1.0f)
 * every * - / one IEEE fp32 operation, no FMA, no reciprocal multiply.  This is the unbiased sample variance of the pixel's n radiance
 * samples divided by n: the estimated variance of the mean that the frame (or, mid-flight, crt_preview's accum * S / n) shows -- what a
 * progressive caller needs to decide when to stop, and what crt_denoise_var takes.  It only reads the handle's sums: calling it between
 * ranges changes no later result.  *samples_done (optional) receives n.
 * CRT_ERR_INVALID_ARG, checked before any device call: a null scene or buffer; no render with the flag on the handle yet; the last
 * render (or any range of the frame in flight, from sample 0 on) was submitted without the flag; n < 2 (a finished spp 1 frame
 * included: one sample has no variance).
 * Precision: a sum of squares, not Welford's update -- both carry two values per channel across chunks, this one adds one multiply and
 * one add per sample to a pass that is bound by reading 12 B per path, and keeps c the frame's own bits.  The sum of squares loses
 * accuracy where variance / mean^2 approaches n x 2^-24; a Welford form would not.  Measured against the float64 sample variance of the
 * same samples on 64x48 spp 8 and 32x24 spp 512 frames of the two shipped scenes: largest relative error 3.44e-6 / 2.75e-6 at spp 8 and
 * 2.68e-6 / 3.46e-6 at spp 512 (cornell-box / veach-mis), 99th percentile below 2.3e-6, smallest variance / mean^2 met 4.4e-4; every
 * value whose float64 variance is 0 came out exactly +0 and none came out negative (docs/experiments.md, "The variance buffer"). */
int crt_variance(crt_scene* scene, float* out_var, uint32_t* samples_done);
/* d_var: a device buffer on the scene's device; enqueued on hip_stream (NULL = default stream) without synchronizing */
int crt_variance_device(crt_scene* scene, void* d_var, void* hip_stream, uint32_t* samples_done);

/* Half-frame buffers (CRT_FLAG_HALF_BUFFERS): the frame as two independent estimates, one from the even and one from the odd samples of
 * every pixel -- what an error estimate of a filtered frame needs (Rousselle et al. 2012; crt_filter_select below).  With the flag,
 * crt_render, crt_render_device, crt_render_range and crt_render_range_device keep, beside c and q of the crt_variance contract, two more
 * sums per pixel slot and channel on the scene handle (6 planes of the shard's slots, uncached, allocated when the flag is first used).
 * With S = params->spp, x_k = L_k / (float)S (the very quotient the frame adds) and k the sample's index IN THE FRAME (not in the chunk
 * or in the range):
 *   h0 = h0 + x_k   for even k          h1 = h1 + x_k   for odd k          from +0.0f, in sample order, one IEEE fp32 add each
 * carried across chunks and progressive ranges as q is.  With n = samples accumulated so far, n_a = (n + 1) / 2 and n_b = n / 2
 * (integer divisions: the even and the odd samples among 0 .. n - 1), per channel:
 *   out_a = h0 * ((float)S / (float)n_a)          out_b = h1 * ((float)S / (float)n_b)
 * one fp32 division and one multiplication, as in crt_preview: the means of the two halves.  Layout: crt_variance's (row-major, or the
 * shard's compact tiles with CRT_FLAG_TILED_OUTPUT; padding slots +0.0f), 3 floats per pixel.  Either output may be NULL, not both.
 * Reads the sums only.  *samples_done (optional) receives n.  c is not h0 + h1 in fp32 (the sums differ in order by design); the mean
 * of the halves weighted by n_a and n_b agrees with the frame's mean to rounding.
 * CRT_ERR_INVALID_ARG, checked before any device call, the handle untouched: a null scene, or both buffers null; no render with the
 * flag on the handle yet; the last render (or any range of the frame in flight, from sample 0 on) was submitted without the flag;
 * n < 2 (the odd half is empty).  crt_render_adaptive, crt_render_map and crt_render_planned keep no halves: after them the call is
 * refused. */
int crt_half_buffers(crt_scene* scene, float* out_a, float* out_b, uint32_t* samples_done);
/* d_a, d_b: device buffers on the scene's device; enqueued on hip_stream (NULL = default stream) without synchronizing */
int crt_half_buffers_device(crt_scene* scene, void* d_a, void* d_b, void* hip_stream, uint32_t* samples_done);

/* Pixel reconstruction filters (CRT_FLAG_PIXEL_FILTER): the frame in which every radiance sample counts for the pixels around its
 * jittered position, weighted by a box, tent or Mitchell-Netravali filter, made from the very paths of the box-filtered frame (the
 * reference's, Render.cuh:348, which stays the default: sample k of pixel p counts for p with weight 1 and for nobody else).
 * crt_set_pixel_filter puts a filter on the handle (NULL: none).  Allowed: BOX with 0.5 <= radius <= 2, TENT with 1 <= radius <= 2,
 * MITCHELL (B = C = 1/3) with radius exactly 2; anything else, NaN included, is CRT_ERR_INVALID_ARG and the handle keeps its old filter.
 * With the flag, crt_render, crt_render_device, crt_render_range and crt_render_range_device keep four more planes per pixel slot on
 * the scene handle, beside whatever they keep without it: a (three planes) and W (uncached, allocated when the flag is first used,
 * carried across chunks and progressive ranges as q is).  The frame, c, q and the halves of the same call are bit for bit what they
 * are without the flag.
 * Tap weight.  For sample k (its index in the frame) of pixel q = (i', j') and output pixel p = (i, j), with S = params->spp and R the
 * radius:
 *   ux = rng_uniform(rj.x), uy = rng_uniform(rj.y) of rj = rng_draw(seed, j' * width + i', k, 0, RNG_JITTER, 0): the very values in
 *        (0, 1] that placed the path's camera ray in its pixel
 *   dx = ((float)(i' - i) + ux) - 0.5f          dy = ((float)(j' - j) + uy) - 0.5f
 *   f(d) = 0 unless d > -R && d <= R (half open, so that BOX with R = 0.5 is a partition: u lies in (0, 1]); inside the support
 *     BOX       f = 1
 *     TENT      f = 1 - |d| / R
 *     MITCHELL  x = |d|;  x < 1: f = ((((21 * x - 36) * x) * x) + 16) / 18;  otherwise f = ((((-7 * x + 36) * x - 60) * x) + 32) / 18
 *   w = f(dx) * f(dy)
 * every operation one IEEE fp32 operation, no FMA, no reciprocal.
 * Sums.  a (per channel) and W of every pixel p start from +0.0f; the samples come in frame order k = 0, 1, ...; within a sample the
 * pixels q around p in row-major order, j' - j = -reach .. reach outer, i' - i inner, reach = ceil(R - 0.5).  Pixels q outside the
 * frame and taps with w == 0.0f are skipped: nothing is added for them.  For every other tap
 *   x = L_{q,k} / (float)S (the frame's own quotient)          a = a + w * x   per channel          W = W + w
 * Read-out (crt_filtered_frame), n = samples accumulated so far (n = S after the range that ends at spp; the sums stay readable until
 * the next render call on the handle):
 *   out_mean = a * ((float)S / W)              where W > 0
 *   out_mean = c * ((float)S / (float)n)       elsewhere, a NaN W included: crt_preview's value
 *   out_rgb  = the frame's tone map of out_mean
 * in the layout of the render's outputs (row-major, or the compact tiles with CRT_FLAG_TILED_OUTPUT; padding slots RGB 0 and +0.0f).
 * So BOX with R = 0.5 gives crt_preview's bits and, at n = S, the frame's own out_mean and RGB.  Either output may be NULL, not both.
 * Reads the sums only.  *samples_done (optional) receives n.
 * Refused before any device call, the handle untouched, crt_last_error naming the call: the flag with no filter set
 * (CRT_ERR_INVALID_ARG); the flag with world > 1 -- a shard does not hold its neighbours -- (CRT_ERR_UNSUPPORTED); a range with
 * sample_begin > 0 whose filter differs from the filter of the frame in flight (CRT_ERR_INVALID_ARG: the frame in flight can still be
 * read and continued with its own filter).  crt_filtered_frame: CRT_ERR_INVALID_ARG with no render with the flag on the handle yet;
 * after a frame any of whose ranges, from sample 0 on, went without the flag; after crt_render_adaptive, crt_render_map or
 * crt_render_planned, which ignore the flag; with a null scene or both outputs NULL.
 * Not provided: a Gaussian filter (it needs exp: the three kinds keep the contract polynomial); a variance of the filtered frame, and
 * with it the filtered frame as a denoiser's input (its noise is correlated between neighbouring pixels); shards and crt_multi; sparse
 * frames; the sums inside the commit ring. */
enum { CRT_PIXEL_FILTER_BOX = 0, CRT_PIXEL_FILTER_TENT = 1, CRT_PIXEL_FILTER_MITCHELL = 2 };
typedef struct {
    uint32_t kind;   /* CRT_PIXEL_FILTER_* */
    float radius;    /* in pixels */
} crt_pixel_filter;
int crt_pixel_filter_defaults(crt_pixel_filter* out);                        /* TENT, radius 1 */
int crt_set_pixel_filter(crt_scene* scene, const crt_pixel_filter* filter);  /* NULL: none */
int crt_filtered_frame(crt_scene* scene, uint8_t* out_rgb, float* out_mean, uint32_t* samples_done);
/* d_rgb, d_mean: device buffers on the scene's device; enqueued on hip_stream (NULL = default stream) without synchronizing */
int crt_filtered_frame_device(crt_scene* scene, void* d_rgb, void* d_mean, void* hip_stream, uint32_t* samples_done);

/* Variance-driven adaptive sampling: one frame in which pixel p receives samples 0 .. n_p - 1 of its S = params->spp samples, n_p chosen
 * per pixel by a stop criterion on the running sums of the crt_variance contract.  Sample k of pixel p is the path it is in crt_render's
 * frame (same seed, same draws), S is the cap AND the divisor of every sample (x_k = L_k / (float)S, as the frame adds it), so a pixel
 * that runs to the cap has the uniform frame's bits.  Operation by operation, every * + - / one IEEE fp32 operation, no FMA:
 *   warm-up    every pixel gets samples 0 .. min_samples-1: c = c + x_k, q = q + x_k * x_k from +0.0f in sample order (the sums of
 *              crt_variance; the warm-up IS a crt_render_range(0, min_samples) with CRT_FLAG_VARIANCE).  n = min_samples, every pixel active.
 *   selection  while n < S, for each still-active pixel, with fn = (float)n, fs = (float)S:
 *                r = fs / fn;  rr = r * r
 *                per channel  d = fn * q - c * c;  d = d < 0.0f ? 0.0f : d;  var = (rr * d) / (fn - 1.0f)      (crt_variance's formula)
 *                per channel  p = c * r                                                                          (crt_preview's mean)
 *                v = (var.x + var.y) + var.z;   m = (p.x + p.y) + p.z
 *                t = threshold * (m + mean_floor);   stop = v <= t * t
 *              i.e. the pixel stops once the standard error of its mean is at most threshold x (mean + mean_floor), channels summed.
 *              A pixel stays active iff it was active and !stop; NaN never satisfies <=, so a NaN pixel runs to the cap; a stopped pixel
 *              never becomes active again.  No active pixel left: the loop ends.
 *   step       ns = min(step_samples, S - n): the active pixels get samples n .. n+ns-1 added to c and q in sample order; n += ns (all
 *              active pixels share n).
 *   outputs    in the layout of crt_render's buffers (row-major, or the shard's compact tiles with CRT_FLAG_TILED_OUTPUT and rank / world;
 *              padding slots 0 / +0.0f):  out_samples = n_p;  out_mean = c * ((float)S / (float)n_p) per channel -- one division, one
 *              multiply, exactly c when n_p = S;  out_rgb = the frame's tone map of out_mean;  out_variance (3 floats per pixel) = the
 *              variance formula above with fn = (float)n_p, what crt_denoise_var takes.  out_samples and out_variance may be NULL;
 *              out_rgb and out_mean not both.
 * The criterion looks at one pixel only, so rank / world shards and the chunking of a pass cannot change a result.
 * Flags: CRT_FLAG_VARIANCE is implied; CRT_FLAG_STATS and CRT_FLAG_BOUNDED_RADIANCE are ignored (there is no commit ring).
 * Handle state: afterwards NO frame is in flight on the handle -- crt_preview, crt_variance and a range with sample_begin > 0 are refused
 * as after a finished frame, and a later crt_render is unaffected.  An adaptive call in the middle of a progressive frame ends that frame.
 * Each pass traces only the active pixels' paths: a selection kernel compacts them, a list maps the render kernel's work cursor onto
 * (sample, active pixel), and the per-path radiance buffer (sized for step_samples x pixel slots, as a uniform chunk) is written
 * sparsely; the list costs 4 B per path of a pass beside it.
 * CRT_ERR_INVALID_ARG, before any device call: a null scene, camera, params or adaptive params; both image outputs NULL; min_samples < 2
 * or > spp; step_samples 0; a threshold that is negative or NaN (+inf is allowed: every pixel stops after the warm-up); a mean_floor
 * that is negative or not finite; anything crt_render refuses.  CRT_ERR_UNSUPPORTED: the fallback pipeline (CRT_PIPELINE=2, or a scene
 * beyond the render kernel's limits), which hands out its work items without the list.  crt_multi has no adaptive form.
 * Cost: every pass is a launch of the persistent render kernel and ends with that kernel's tail, about 2 ms on the 800x600 frames
 * measured whatever the number of active pixels, so the step size sets the price of the call (docs/experiments.md, "Adaptive sampling").
 * crt_adaptive_defaults fills min_samples 16, step_samples 64, threshold 0.05, mean_floor 0.01.  The step is the one setting that has been
 * measured -- 4, 16, 64 and 248 on 800x600 frames of the two shipped scenes with a cap of 512, where 16 took 1.4 times as long as 64 for
 * the same error; the other three are a starting point that has NOT been tuned on any scene. */
typedef struct {
    uint32_t min_samples;   /* warm-up: every pixel gets samples [0, min_samples); 2 <= min_samples <= spp */
    uint32_t step_samples;  /* samples a still-active pixel gets per pass; >= 1 */
    float    threshold;     /* relative standard error of the pixel's mean at which it stops; >= 0, not NaN, +inf allowed */
    float    mean_floor;    /* added to the mean in the criterion so dark pixels can stop; >= 0, finite */
} crt_adaptive_params;
#define CRT_ADAPTIVE_PASSES_REPORTED 64
typedef struct {
    uint32_t passes;        /* render passes that ran, the warm-up included */
    uint32_t pass_pixels[CRT_ADAPTIVE_PASSES_REPORTED]; /* pixels still active in adaptive pass 0, 1, ... (the warm-up is not listed; passes beyond 64 are not recorded) */
    uint64_t paths;         /* sum of n_p over the shard's pixels = paths traced */
    uint64_t paths_uniform; /* pixels x spp: what crt_render would have traced */
    float kernel_ms, total_ms; /* sum of the render kernel's launches (first launch's start to last launch's end of every pass) / the whole
                                  device pipeline of the call, HIP events on its stream */
} crt_adaptive_info;
int crt_adaptive_defaults(crt_adaptive_params* params);
/* host buffers: out_rgb 3 bytes, out_mean 3 floats, out_samples 1 uint32, out_variance 3 floats per pixel (or pixel slot); info optional */
int crt_render_adaptive(crt_scene* scene, const crt_camera* cam, const crt_params* params, const crt_adaptive_params* adaptive,
                        uint8_t* out_rgb, float* out_mean, uint32_t* out_samples, float* out_variance, crt_adaptive_info* info);
/* Device buffers on the scene's device, work enqueued on hip_stream (NULL = default stream).  Unlike crt_render_device this form
 * SYNCHRONIZES hip_stream once per pass: the host reads the number of active pixels (one 4-byte copy into pinned memory) to size the next
 * pass and to end the loop.  The outputs are enqueued after the last pass without a further synchronization, unless info != NULL (the
 * call then synchronizes once more to read the timers). */
int crt_render_adaptive_device(crt_scene* scene, const crt_camera* cam, const crt_params* params, const crt_adaptive_params* adaptive,
                               void* d_rgb, void* d_mean, void* d_samples, void* d_variance, void* hip_stream, crt_adaptive_info* info);

/* First-hit auxiliary buffers (AOVs: the guides of a denoiser, depth and coverage for compositing, IDs for masks), aligned sample for
 * sample with the frame crt_render draws with the same camera / params.  Per pixel, the S = params->spp camera rays of samples
 * k = 0 .. S-1 -- the primary rays of the frame's paths: same seed, jitter draws and arithmetic -- are traced for their closest hit
 * with params->traversal (EXACT, REFERENCE or FAST, as crt_intersect).  tri_k = the triangle sample k hits (BVH order), m_k its
 * crt_triangle.material, t_k the hit distance along the unit direction, n_hit the number of samples that hit:
 *   albedo   3 floats  a = a + kd(m_k) / S over the samples that hit, in sample order, from +0.0f (a miss adds nothing); kd = crt_material.kd
 *   normal   3 floats  the same with the triangle's stored normal (crt_triangle.normal; not renormalised, not flipped)
 *   depth    float     d = d + t_k over the hits in sample order, then d / (float)n_hit; 0.0f if n_hit = 0
 *   coverage float     (float)n_hit / (float)S
 *   tri      int32     tri_0 of sample 0, -1 if it missed
 *   material int32     m_0 of sample 0, -1 if it missed
 * IEEE divisions, no reciprocal multiply, no FMA.  Pixel order as crt_render's out_mean: row-major, or the compact 8x8 tiles of shard
 * rank / world with CRT_FLAG_TILED_OUTPUT (padding slots: 0 and -1).  Ignored: p_rr, light_sample_n, CRT_FLAG_STATS, _TRACE_ALL and
 * _BOUNDED_RADIANCE.  Any buffer may be NULL, not all six.  A null pointer, six NULL buffers, spp 0 or a size of 0 is
 * CRT_ERR_INVALID_ARG, checked before any device call.  The rays are traced in chunks of whole samples of at most 2^25 rays (48 B each
 * of the handle's query pool), so a pass never needs the frame's per-path storage.
 * The AOV calls leave a progressive render in flight on the handle as it is: ranges with AOV calls in between give the one-shot frame.
 * Render and AOV calls on one handle share its work buffers: calls with device outputs must be ordered by using one stream. */
typedef struct { float* albedo; float* normal; float* depth; float* coverage; int32_t* tri; int32_t* material; } crt_aov_buffers;
typedef struct {
    uint64_t rays;     /* camera rays traced: spp x the shard's pixel slots (padding slots of ragged tiles included) */
    uint32_t chunks;   /* trace launches (chunks of whole samples) */
    float total_ms;    /* HIP-event time of the pass on its stream */
} crt_aov_info;
/* host_out: host buffers (W*H or slots elements of 3 or 1 values each); info optional */
int crt_render_aov(crt_scene* scene, const crt_camera* cam, const crt_params* params, const crt_aov_buffers* host_out, crt_aov_info* info);
/* dev_out: device buffers on the scene's device; enqueued on hip_stream (NULL = default stream) without synchronizing, unless
 * info != NULL (the call then synchronizes the stream to read the timer) */
int crt_render_aov_device(crt_scene* scene, const crt_camera* cam, const crt_params* params, const crt_aov_buffers* dev_out,
                          void* hip_stream, crt_aov_info* info);

/* Shading AOVs: what the frame's radiance factors into, so that an image filter can work on irradiance instead (crt_demodulate below).
 * In the reference's path loop the radiance of sample k is ke(m_k) and nothing else if its camera ray hits an emitter, and carries the
 * factor kd(m_k) in every term otherwise; so  frame = emission + sum_k kd(m_k) * I_k / S.  crt_render_aov's albedo sums kd over ALL
 * hits, emitters included; these two buffers split the hits.
 * Rays, chunks, layout (row-major, or the tiled shard with CRT_FLAG_TILED_OUTPUT), the ignored params and the frame in flight on the
 * handle (left alone) are exactly crt_render_aov's; a sample is a hit when its camera ray hits a triangle tri_k with material m_k.  An
 * emitter is a material with the flag the render kernel ends a path on: crt_material.has_emit != 0.  S = params->spp; both sums start
 * at +0.0f and run in sample order:
 *   emission        3 floats  e = e + ke(m_k) / S over the hits on emitters          ke = crt_material.ke
 *   diffuse_albedo  3 floats  b = b + kd(m_k) / S over the hits on non-emitters      kd = crt_material.kd
 * IEEE fp32 divisions, no FMA, no reciprocal multiply; padding slots get 0.  At a pixel none of whose samples hits an emitter,
 * diffuse_albedo has albedo's bits and emission is +0.  ONE trace serves both structs: `first` may be NULL; when it is not, its
 * buffers (any may be NULL, not all six) get crt_render_aov's bits.  `shading` must not be NULL and must name at least one buffer.
 * A null scene, camera, params or shading, no buffer in shading, six NULL buffers in a `first` that is given, spp 0 or a size of 0 is
 * CRT_ERR_INVALID_ARG, checked before any device call, as is everything crt_render_aov refuses.  Works on both pipelines and with
 * EXACT, REFERENCE and FAST traversal.  info as crt_render_aov's.  Not followed: emission seen through a mirror (the SPECULAR probe
 * term keeps its kd factor and stays in the irradiance). */
typedef struct { float* emission; float* diffuse_albedo; } crt_aov_shading_buffers;   /* 3 floats per pixel each */
/* host buffers (W*H or slots elements of 3 or 1 values each); info optional */
int crt_render_aov_shading(crt_scene* scene, const crt_camera* cam, const crt_params* params, const crt_aov_buffers* host_first /* may be NULL */,
                           const crt_aov_shading_buffers* host_shading, crt_aov_info* info);
/* device buffers on the scene's device; enqueued on hip_stream (NULL = default stream) without synchronizing, unless info != NULL
 * (the call then synchronizes the stream to read the timer) */
int crt_render_aov_shading_device(crt_scene* scene, const crt_camera* cam, const crt_params* params, const crt_aov_buffers* dev_first /* may be NULL */,
                                  const crt_aov_shading_buffers* dev_shading, void* hip_stream, crt_aov_info* info);

/* AOVs that follow perfect-mirror bounces: what a SPECULAR surface reflects instead of the surface itself, as guides of the denoiser.
 * Per sample k of a pixel the first ray is crt_render_aov's (origin eye, the unit camera direction, closest hit with params->traversal).
 * If it misses, the sample is no hit and adds nothing anywhere.  Otherwise a chain starts with len = +0.0f, B = 0, thr unset, and at
 * every hit (triangle tri, distance t, material m; o, d the ray's origin and unit direction):
 *   len = len + t
 *   the chain goes on iff m is SPECULAR (the flag the render kernel reads: crt_material.mode == 1; the shipped loader: Ns > 1) and
 *   B < max_bounces.  Then, per channel / component,
 *     thr = (B == 0) ? kd(m) : thr * kd(m)
 *     n   = crt_triangle.normal of tri, as stored
 *     P   = o + d * t                                 one multiply, then one add
 *     c   = d.x * n.x + (d.y * n.y + d.z * n.z);  c2 = c + c
 *     r   = d - n * c2                                one multiply, then one subtract
 *   the next ray has origin P (no offset: a hit at t <= epsilon is rejected by the intersector, as for every ray) and the direction r
 *   normalised as crt_intersect normalises a raw direction;  B = B + 1;  it is traced for its closest hit.
 * The chain ends at a hit it does not go on from (tri_L, m_L), or at a miss.  Of a sample that is a hit:  D = len;  B = the reflected
 * rays traced;  if the chain ended at a hit, G = kd(m_L) if B == 0, else G = thr * (kd(m_L) + e) with e = ke(m_L) < 1 ? ke(m_L) : 1
 * per channel (one add, then one multiply), and N = the stored normal of tri_L;  if it ended at a miss, G and N are absent.
 * Per pixel, in sample order, from +0.0f, S = params->spp, n_hit = the samples that are hits:
 *   guide_albedo 3 floats  a = a + G / S over the samples that have a G
 *   last_normal  3 floats  the same with N
 *   path_depth   float     (sum of D) / (float)n_hit; 0.0f if n_hit = 0
 *   bounces      float     (sum of (float)B) / (float)n_hit; 0.0f if n_hit = 0
 *   last_tri     int32     tri_L of sample 0; -1 if sample 0 missed or its chain ended at a miss
 * IEEE fp32, no FMA, no reciprocal multiply.  A pixel none of whose samples hits a SPECULAR triangle has crt_render_aov's albedo, normal
 * and depth in guide_albedo, last_normal and path_depth bit for bit, bounces 0 and last_tri = tri.  No refraction; a rough (glossy)
 * SPECULAR surface is followed as a perfect mirror.
 * Layout (row-major, or tiled shards with CRT_FLAG_TILED_OUTPUT; padding slots 0 and -1), chunks of whole samples of at most 2^25
 * camera rays, the ignored params and the progressive frame in flight (left alone) are crt_render_aov's.  A chunk needs 104 B of the
 * handle's query buffers (two halves, which the bounces alternate between) and 24 B of chain state per camera ray.  Any buffer may be NULL, not all five.  A null pointer, five NULL
 * buffers, max_bounces outside 1 .. 8, spp 0 or a size of 0 is CRT_ERR_INVALID_ARG, checked before any device call.
 * info->rays counts the camera rays (as crt_render_aov's) and the reflected rays (of pixels; a padding slot's ray is not followed),
 * info->chunks the chunks of whole samples. */
typedef struct { uint32_t max_bounces; } crt_aov_specular_params;   /* 1 .. 8 */
typedef struct { float* guide_albedo; float* last_normal; float* path_depth; float* bounces; int32_t* last_tri; } crt_aov_specular_buffers;
int crt_aov_specular_defaults(crt_aov_specular_params* params);     /* max_bounces 2 */
/* host_out: host buffers (W*H or slots elements of 3 or 1 values each); info optional */
int crt_render_aov_specular(crt_scene* scene, const crt_camera* cam, const crt_params* params, const crt_aov_specular_params* specular,
                            const crt_aov_specular_buffers* host_out, crt_aov_info* info);
/* dev_out: device buffers on the scene's device, work enqueued on hip_stream (NULL = default stream).  Unlike crt_render_aov_device the
 * call is not asynchronous: after each bounce of each chunk the host reads how many rays go on -- one 4-byte copy into pinned memory and
 * one synchronization of the stream per bounce and chunk, as crt_render_adaptive_device per pass -- to trace only those and to stop at
 * 0 (a scene without SPECULAR triangles: one synchronization per chunk).  The last bounce allowed needs none.  The outputs are enqueued
 * after it without a further synchronization, unless info != NULL (the call then synchronizes once more to read the timer). */
int crt_render_aov_specular_device(crt_scene* scene, const crt_camera* cam, const crt_params* params, const crt_aov_specular_params* specular,
                                   const crt_aov_specular_buffers* dev_out, void* hip_stream, crt_aov_info* info);

/* Direct-light AOVs: what lights the first hit.  The renderer's draws are addressed by (seed, pixel, sample, depth, purpose, index), so the
 * next-event samples of a path's first vertex depend on the camera ray's hit alone -- not on p_rr, not on anything later in the path --
 * and this pass recomputes, sample for sample, the first-vertex direct light L_dir of the very paths the frame traces (Render.cuh:262-284).
 * fp32, one IEEE operation per symbol, no FMA, no reciprocal multiply.  Per pixel, for the samples k = 0 .. S-1 (S = params->spp) in order:
 *   camera ray and first hit: crt_render_aov's (origin o = eye, unit direction d, distance t, triangle tri).  A miss, or a hit on an
 *     emitter (crt_material.has_emit != 0), contributes nothing to any sum: Ld_k = U_k = +0, nothing traced.
 *   vertex: pos = o + t * d (one multiply, then one add); n = crt_triangle.normal of tri as stored; f_r = kd(m) / pi, the BSDF row of the
 *     material m of tri that the render kernel reads.
 *   for q = 0 .. n_lights * light_sample_n - 1 (light q / light_sample_n, repetition q % light_sample_n): the draw r = (seed, pixel, k, 0,
 *     next-event, q); the light's triangle r.x % count; alpha = u(r.y), beta = u(r.z) * (1 - alpha), gamma = 1 - alpha - beta;
 *     lpos = (alpha * v1 + beta * v2) + gamma * v3; dist = lpos - pos; dir = normalized(dist); the ray leaves pos along normalized(dir)
 *     with the limit tl = dist.x / dir.x; len = norm(dist); cos = max(dot(dir, n), 0), cos' = max(-dot(dir, n_light), 0) (a NaN: 0);
 *     c_q = ((((((ke_light * f_r) * cos) * cos') * area_of_obj) / (len * len)) / light_sample_n  -- the last division is the
 *     multiplication by 2^-j when light_sample_n = 2^j (the same bits).
 *   sample q is TRACED when !(c.x == 0 && c.y == 0 && c.z == 0) -- a NaN contribution is traced -- and a sample that is not traced adds
 *     nothing.  A traced sample is BLOCKED by the reference's blocked() (Render.cuh:19-27) evaluated as the render kernel of
 *     params->traversal evaluates it: tl - t_hit > 1e-5 with t_hit = FLT_MAX when nothing was hit (REFERENCE: the closest hit; EXACT and
 *     FAST: any hit that satisfies it).
 *   Ld_k = sum over q of c_q over the traced, unblocked samples;  U_k = the same over all traced samples; both from +0, in q order.
 * Outputs (any may be NULL, not all four), from +0.0f, in sample order:
 *   direct           3 floats  d = d + Ld_k / S
 *   unshadowed       3 floats  u = u + U_k / S
 *   direct_variance  3 floats  crt_variance's statistic of the S values Ld_k / S (misses and emitter hits included, as +0):
 *                              c = c + x, q = q + x * x, then max(S * q - c * c, 0) / (S - 1) per channel; +0 when S = 1
 *   visibility       float     (float)lit / (float)traced over the pixel's traced samples, lit = those not blocked; 1.0f when none was traced
 * Consequence: at p_rr = 0 the frame's paths end at their first vertex, so at a pixel none of whose samples hits an emitter `direct` is
 * crt_render's out_mean bit for bit; at any p_rr it is the first-vertex next-event term of the frame's own paths.
 * p_rr is not read.  light_sample_n is checked as crt_render checks it (0 .. 4096, at most 65535 samples per vertex); with 0, or a scene
 * without lights, direct, unshadowed and direct_variance are 0 and visibility is 1.  The other refusals, the layout (row-major, or the
 * tiled shard with CRT_FLAG_TILED_OUTPUT; padding slots 0), the ignored flags, the chunks of camera rays and the frame in flight on the
 * handle (left alone) are crt_render_aov's.  Inside a chunk the (sample, q) entries are walked in sub-batches of at most 2^25 entries
 * x pixel slots (16 B of contribution plane and 44 B of query buffers each; a sub-batch may begin and end inside a sample).
 * info->rays = camera rays (as crt_render_aov's) + traced shadow rays; info->chunks = sub-batches. */
typedef struct { float* direct; float* unshadowed; float* direct_variance; float* visibility; } crt_aov_direct_buffers;   /* 3, 3, 3, 1 floats per pixel */
/* host buffers (W*H or slots elements of 3 or 1 values each); info optional */
int crt_render_aov_direct(crt_scene* scene, const crt_camera* cam, const crt_params* params, const crt_aov_direct_buffers* host_out, crt_aov_info* info);
/* device buffers on the scene's device, work enqueued on hip_stream (NULL = default stream).  Like crt_render_aov_specular_device the
 * call is not asynchronous: per sub-batch the host reads how many shadow rays are traced -- one 4-byte copy into pinned memory and one
 * synchronization of the stream.  The outputs are enqueued after the last without a further synchronization, unless info != NULL. */
int crt_render_aov_direct_device(crt_scene* scene, const crt_camera* cam, const crt_params* params, const crt_aov_direct_buffers* dev_out,
                                 void* hip_stream, crt_aov_info* info);

/* Ambient-occlusion AOVs: the geometry around the first hit.  Per camera ray's hit the pass sends ao_samples rays of at most max_distance
 * over the hemisphere of the hit's facing normal and returns the cosine-weighted open fraction, the plain open fraction and the mean
 * open direction.  The draws have a purpose of their own (4, "ambient occlusion", beside jitter 0, bounce 1, next-event 2, probe 3): no
 * path consumes them, and no path's draws move.  fp32, one IEEE operation per symbol, no FMA, no reciprocal multiply.  Per pixel, for the
 * samples k = 0 .. S-1 (S = params->spp) in order:
 *   camera ray and first hit: crt_render_aov's (origin o = eye, unit direction d, distance t, triangle tri).  A miss contributes nothing
 *     to any sum.  Every hit is a vertex, a hit on an emitter too.
 *   vertex: pos = o + t * d (one multiply, then one add); n = crt_triangle.normal of tri as stored; nf = dot(d, n) > 0 ? -n : n (a NaN
 *     dot keeps n).
 *   for q = 0 .. ao_samples - 1: the draw r = (seed, pixel, k, 0, ambient occlusion, q); dir = bounce_dir(nf, r), the function the
 *     path's bounce uses: normalized(sample_hemisphere(nf, u(r.y), u(r.z))), a uniform hemisphere (Render.cuh:214, Ray.cuh:13);
 *     w = max(dot(dir, nf), 0) (a NaN: 0).  The ray leaves pos along dir -- the query is handed dir itself, as the path's bounce ray is;
 *     the reference's Ray would get sample_hemisphere's vector and normalise it once -- with the limit tl = max_distance, and is BLOCKED
 *     by the reference's blocked() (Render.cuh:19-27) evaluated as the render kernel of params->traversal evaluates it: tl - t_hit > 1e-5
 *     with t_hit = FLT_MAX when nothing was hit (REFERENCE: the closest hit; EXACT and FAST: any hit that satisfies it) -- what
 *     crt_render_aov_direct does with its shadow rays.  Every ray is traced: there is no "untraced" class.
 *   sums, from +0 in (k, q) order: A = A + w;  V = V + w over the unblocked rays;  the integer counts rays and open (unblocked);
 *     b = b + dir per component over the unblocked rays.
 * Outputs (any may be NULL, not all three):
 *   ao           float     V / A, and 1.0f when A == 0 (no hit, or every cosine zero)
 *   openness     float     (float)open / (float)rays, and 1.0f when rays == 0
 *   bent_normal  3 floats  normalized(b) -- b / sqrt(dot(b, b)) when dot(b, b) > 0, else b as it is --, and (+0, +0, +0) when open == 0
 * A mean distance of the open rays is deliberately not provided: an any-hit query knows no distance of a ray that is open.
 * ao_samples is 1 .. 256.  max_distance must be finite and > 0: with +inf, inf - FLT_MAX would block every ray that escapes, so +inf and
 * NaN are CRT_ERR_INVALID_ARG like 0 and negative values.  crt_aov_ao_defaults gives ao_samples 4 and max_distance = a quarter of the
 * diagonal of the box of the scene's root node (1 when that is not a positive finite number); BOTH DEFAULTS ARE TUNED ON NOTHING --
 * they are a starting point that no measurement stands behind.
 * p_rr and light_sample_n are not read.  The refusals, the layout (row-major, or the tiled shard with CRT_FLAG_TILED_OUTPUT), the ignored
 * flags, the chunks of camera rays and the frame in flight on the handle (left alone) are crt_render_aov's; spp x ao_samples above
 * 2^32 - 1 is CRT_ERR_UNSUPPORTED.  A padding slot of a tiled shard gets what a pixel that only misses gets: ao 1.0f, openness 1.0f,
 * bent_normal +0.  Inside a chunk the (sample, q) entries are walked in sub-batches of at most 2^25 entries x pixel slots (16 B of entry
 * plane and 56 B of query buffers and answers each; a sub-batch may begin and end inside a sample).
 * info->rays = camera rays (as crt_render_aov's) + occlusion rays (hits x ao_samples); info->chunks = sub-batches. */
typedef struct { uint32_t ao_samples; float max_distance; } crt_aov_ao_params;
typedef struct { float* ao; float* openness; float* bent_normal; } crt_aov_ao_buffers;   /* 1, 1, 3 floats per pixel */
int crt_aov_ao_defaults(const crt_scene* scene, crt_aov_ao_params* out);
/* host buffers (W*H or slots elements of 1 or 3 values each); info optional */
int crt_render_aov_ao(crt_scene* scene, const crt_camera* cam, const crt_params* params, const crt_aov_ao_params* ao, const crt_aov_ao_buffers* host_out,
                      crt_aov_info* info);
/* device buffers on the scene's device, work enqueued on hip_stream (NULL = default stream).  Every ray is traced, so the host knows the
 * size of each launch in advance: the call reads nothing back and enqueues its whole work without synchronizing the stream, unless
 * info != NULL (one synchronization at the end, then an 8-byte copy of the ray count).  Like every pass on a handle it may have to grow
 * the handle's buffers first, and freeing a device buffer waits for the device: the first call at a size is not asynchronous. */
int crt_render_aov_ao_device(crt_scene* scene, const crt_camera* cam, const crt_params* params, const crt_aov_ao_params* ao, const crt_aov_ao_buffers* dev_out,
                             void* hip_stream, crt_aov_info* info);

/* AOV-guided edge-avoiding denoiser: an a-trous ("with holes") wavelet filter with edge-stopping weights on colour, normal, albedo and
 * depth (Dammertz et al. 2010), run as `iterations` passes over a frame's pre-tone-map mean radiance (out_mean of crt_render), guided by
 * the buffers crt_render_aov returns.  An image operation: no scene handle.  Row-major images of width x height; color, albedo, normal
 * 3 floats per pixel, depth 1 float per pixel.  c_0 = color.  Pass i = 0 .. iterations-1 has tap spacing s = 2^i and computes c_{i+1}
 * from c_i.  For pixel p = (x, y) the 25 taps q = (x + dx*s, y + dy*s) are visited with dy = -2..2 outer, dx = -2..2 inner; a tap outside
 * the image is skipped (nothing is added for it).  With h = {1/16, 1/4, 3/8, 1/4, 1/16} (exact in fp32):
 *   sig  = sigma_color / (float)(1 << i)
 *   dc   = c_i(p) - c_i(q)            e_c = (dc.x*dc.x + dc.y*dc.y + dc.z*dc.z) / (sig * sig)
 *   dn   = normal(p) - normal(q)      e_n = (dn.x*dn.x + dn.y*dn.y + dn.z*dn.z) / (sigma_normal * sigma_normal)
 *   da   = albedo(p) - albedo(q)      e_a = (da.x*da.x + da.y*da.y + da.z*da.z) / (sigma_albedo * sigma_albedo)
 *   m    = depth(p) > depth(q) ? depth(p) : depth(q)
 *   r    = (depth(p) - depth(q)) / (sigma_depth * m)      e_d = m > 0 ? r * r : 0      (relative depth; depth 0 = a miss)
 *   w    = (h[dy+2] * h[dx+2]) * exp(-(((e_c + e_n) + e_a) + e_d))                     (exp: det_expf of csrc/crt_detmath.h)
 *   num  = num + c_i(q) * w   (per channel)               den = den + w
 *   c_{i+1}(p) = num / den    (per channel)
 * num and den start at +0.0f; sums are left to right as written; every * + - / is one IEEE fp32 operation (no FMA, no reciprocal
 * multiply).  A guide pointer that is NULL makes its term +0.0f (color is required).  iterations is 1 .. 5.  Each sigma must be > 0 and
 * not NaN; +inf is allowed and switches its term off.  Non-finite inputs are not special-cased: the arithmetic above defines the result
 * (exp(NaN) is NaN, exp(x < -87) is exactly 0).  Outputs: c_iterations as out_mean (3 floats per pixel) and / or its RGB8 tone map
 * out_rgb (3 bytes per pixel: the bits crt_render writes for that mean); either may be NULL, not both.
 * crt_denoise_defaults fills iterations 3, sigma_color 4, sigma_normal 0.5, sigma_albedo 0.1, sigma_depth 0.05 (width and height 0):
 * the best of a small sweep on 160x120 spp 8 frames of the two shipped scenes and nothing larger.
 * A null pointer, a size of 0, iterations outside 1 .. 5, a sigma that is not > 0, two NULL outputs or a scratch buffer that is missing,
 * too small or not 16-byte aligned is CRT_ERR_INVALID_ARG, checked before any device call.  (A side longer than 2^24 pixels:
 * CRT_ERR_UNSUPPORTED.) */
typedef struct {
    uint32_t width, height;
    uint32_t iterations;
    float sigma_color, sigma_normal, sigma_albedo, sigma_depth;
} crt_denoise_params;
typedef struct { const float* color; const float* albedo; const float* normal; const float* depth; } crt_denoise_inputs;
typedef struct {
    float total_ms;    /* HIP-event time of the call's kernels on its stream */
    uint32_t passes;   /* filter passes that ran (= iterations) */
} crt_denoise_info;
int crt_denoise_defaults(crt_denoise_params* params);
/* bytes of device scratch crt_denoise_device needs for a width x height image: 64 B per pixel (the colour ping-pong pair and the two
 * packed guide planes, 16 B per pixel each) */
int crt_denoise_scratch_bytes(uint32_t width, uint32_t height, uint64_t* bytes);
/* host buffers; allocates and frees its own device memory on `device`; info optional */
int crt_denoise(int device, const crt_denoise_params* params, const crt_denoise_inputs* host_in, float* out_mean, uint8_t* out_rgb,
                crt_denoise_info* info);
/* Everything in device memory on `device`; enqueued on hip_stream (NULL = default stream) without synchronizing, unless info != NULL
 * (the call then synchronizes the stream to read the timer).  The caller owns d_scratch (scratch_bytes >= crt_denoise_scratch_bytes),
 * so frames can be pipelined without allocation.  Outputs must not overlap inputs or scratch. */
int crt_denoise_device(int device, const crt_denoise_params* params, const crt_denoise_inputs* dev_in, void* d_out_mean, void* d_out_rgb,
                       void* d_scratch, uint64_t scratch_bytes, void* hip_stream, crt_denoise_info* info);

/* Variance-guided form of the filter (the spatial half of SVGF, Schied et al. 2017): the colour tolerance of a pixel is set by how noisy
 * the renderer says its neighbourhood is, not by one sigma_color for the whole frame, and the variance is filtered along with the colour
 * so that later passes see what noise is left.  `variance` is what crt_variance returns (3 floats per pixel) and is required; albedo,
 * normal and depth may be NULL as in crt_denoise.  c_0 = color, v_0(p) = (variance(p).x + variance(p).y) + variance(p).z.  Pass
 * i = 0 .. iterations-1, tap spacing s = 2^i:
 *   g(p):  3x3 taps t = (x + dx, y + dy) at spacing 1 in EVERY pass, dy = -1..1 outer, dx = -1..1 inner, k = {1/4, 1/2, 1/4}, a tap
 *          outside the image is skipped:   gn = gn + (k[dy+1] * k[dx+1]) * v_i(t);   gd = gd + (k[dy+1] * k[dx+1]);   g = gn / gd
 *   n_c  = (sigma_color * sigma_color) * g(p) + 1e-10f                 (no halving of sigma_color per pass: v_i shrinks instead)
 *   e_c  = (dc.x*dc.x + dc.y*dc.y + dc.z*dc.z) / n_c                   dc = c_i(p) - c_i(q)
 *   e_n, e_a, e_d, h, the 25 taps q, their order and the border rule: exactly as crt_denoise
 *   w    = (h[dy+2] * h[dx+2]) * exp(-(((e_c + e_n) + e_a) + e_d))     (det_expf)
 *   num  = num + c_i(q) * w      den = den + w      vnum = vnum + v_i(q) * (w * w)
 *   c_{i+1}(p) = num / den       v_{i+1}(p) = vnum / (den * den)
 * all sums from +0.0f, left to right as written, one IEEE fp32 operation per * + - /, no FMA.  Outputs: c_iterations as out_mean and /
 * or its tone map out_rgb (not both NULL), and optionally v_iterations as out_variance (1 float per pixel: the filter's own estimate of
 * the noise that is left).  Scratch: the same 64 B per pixel (crt_denoise_scratch_bytes); the scalar variance rides in the .w of the
 * colour planes.  Argument checks as crt_denoise, plus: a null `variance` and a sigma_color of +inf are CRT_ERR_INVALID_ARG (inf x 0
 * would make every weight NaN; to drop the colour term use crt_denoise).  Non-finite or negative variance values are not special-cased.
 * crt_denoise_var_defaults fills iterations 3, sigma_color 6, sigma_normal 0.5, sigma_albedo 0.1, sigma_depth 0.05: on the 160x120 spp 8
 * frames crt_denoise's defaults were chosen on, the error against a converged frame falls from 169.3 to 159.9 (cornell-box) and from
 * 149.6 to 112.1 (veach-mis) (docs/experiments.md, "The variance-guided filter"). */
typedef struct { const float* color; const float* variance; const float* albedo; const float* normal; const float* depth; } crt_denoise_var_inputs;
int crt_denoise_var_defaults(crt_denoise_params* params);
int crt_denoise_var(int device, const crt_denoise_params* params, const crt_denoise_var_inputs* host_in, float* out_mean, uint8_t* out_rgb,
                    float* out_variance, crt_denoise_info* info);
int crt_denoise_var_device(int device, const crt_denoise_params* params, const crt_denoise_var_inputs* dev_in, void* d_out_mean,
                           void* d_out_rgb, void* d_out_variance, void* d_scratch, uint64_t scratch_bytes, void* hip_stream,
                           crt_denoise_info* info);

/* Non-local means with variance-normalised patch distances (Rousselle et al. 2012), joint with the guides (Rousselle et al. 2013): one
 * pass whose weight between two pixels comes from how much the patches around them differ beyond what their variances explain, so the
 * filter follows the sample count by itself and keeps structure that the guides do not see.  Inputs and outputs are crt_denoise_var's:
 * color and variance required, albedo / normal / depth optional (a NULL guide makes its term +0.0f); out_mean and / or out_rgb (the
 * frame's tone map of the mean), not both NULL, and optionally out_variance (1 float per pixel).  An image operation: row-major, no
 * scene handle.  info->passes is 1.
 *   v(p)  = (variance(p).x + variance(p).y) + variance(p).z
 *   g(p)  = the 3x3 Gaussian of v around p: exactly crt_denoise_var's g of pass 0 (k = {1/4, 1/2, 1/4}, dy outer, dx inner, taps outside
 *           the image skipped, gn / gd)
 *   k2    = k * k
 * For pixel p and window offset o = (ox, oy), oy = -radius..radius outer, ox = -radius..radius inner, q = p + o; a q outside the image
 * is skipped:
 *   D = +0, n = 0
 *   for py = -patch..patch (outer):  row = +0
 *     for px = -patch..patch (inner):  t = p + (px, py), u = t + o;  t or u outside the image: skipped (nothing added, n unchanged)
 *       dc  = c(t) - c(u)                          s = dc.x*dc.x + dc.y*dc.y + dc.z*dc.z
 *       mn  = g(u) < g(t) ? g(u) : g(t)
 *       d   = (s - alpha * (g(t) + mn)) / (1e-10f + k2 * (g(t) + g(u)))
 *       row = row + d;  n = n + 1
 *     D = D + row                                  (after every py, also when the row had no tap)
 *   Dm  = D / (float)n                             (n >= 1: the patch centre is always inside)
 *   e_p = Dm < 0 ? 0 : Dm                          (a NaN passes through)
 *   e_n, e_a, e_d between p and q: exactly crt_denoise's, with sigma_normal, sigma_albedo, sigma_depth
 *   w   = exp(-(((e_p + e_n) + e_a) + e_d))        (det_expf)
 *   num = num + c(q) * w (per channel)    den = den + w    vnum = vnum + v(q) * (w * w)
 *   out_mean(p) = num / den (per channel)          out_variance(p) = vnum / (den * den)
 * All arithmetic is fp32 with one IEEE operation per symbol (no FMA, no reciprocal multiply); sums start at +0.0f and run left to right
 * as written.  Non-finite inputs are not special-cased.
 * The pair term d depends on (t, o) only, not on p, and so does whether a tap is skipped.  A row sum row(x, y + py, o) is therefore the
 * same number for every pixel of column x that reaches that row: an implementation may compute each d once per (t, o) and each row sum
 * once per (x, row, o), and still match a per-pixel evaluation bit for bit.  The library has both forms (csrc/crt_nlm.hip: k_nlm_shared
 * shares them through LDS, k_nlm_direct does not); the environment variable CRT_NLM_FORM=direct|shared, read per call, selects one
 * (for tests; any other value is CRT_ERR_INVALID_ARG), and both give the same bits.
 * radius is 1 .. 8 (a search window of (2 radius + 1)^2), patch 0 .. 3 (patches of (2 patch + 1)^2), k > 0 and finite (the damping of
 * the patch distance), alpha >= 0 and finite (how much of the variance is taken off a squared difference); each sigma > 0 and not NaN,
 * +inf switches its term off.  A null params, inputs, color or variance, a size of 0, a setting outside these ranges, two NULL outputs,
 * a negative device or a scratch buffer that is missing, too small or not 16-byte aligned is CRT_ERR_INVALID_ARG, checked before any
 * device call.  (A side longer than 2^24 pixels: CRT_ERR_UNSUPPORTED.)  Scratch: 48 B per pixel (crt_denoise_nlm_scratch_bytes: three
 * float4 planes -- (colour, g), (normal, depth), (albedo, v)).
 * crt_denoise_nlm_defaults fills radius 5, patch 1, k 0.7, alpha 1, sigma_normal 0.5, sigma_albedo 0.1, sigma_depth 0.05: the set with the
 * smallest summed error relative to crt_denoise_var's defaults on the 160x120 spp 8 and spp 32 frames of the two shipped scenes
 * (docs/experiments.md, "The non-local-means filter"). */
typedef struct {
    uint32_t width, height;
    uint32_t radius;      /* search window (2 radius + 1)^2: 1 .. 8 */
    uint32_t patch;       /* patches of (2 patch + 1)^2: 0 .. 3 */
    float k;              /* damping of the patch distance: > 0, finite */
    float alpha;          /* how much of the variance is taken off a squared difference: >= 0, finite */
    float sigma_normal, sigma_albedo, sigma_depth;   /* as crt_denoise: > 0, not NaN, +inf switches the term off */
} crt_nlm_params;
int crt_denoise_nlm_defaults(crt_nlm_params* params);
int crt_denoise_nlm_scratch_bytes(uint32_t width, uint32_t height, uint64_t* bytes);
int crt_denoise_nlm(int device, const crt_nlm_params* params, const crt_denoise_var_inputs* host_in, float* out_mean, uint8_t* out_rgb,
                    float* out_variance, crt_denoise_info* info);
int crt_denoise_nlm_device(int device, const crt_nlm_params* params, const crt_denoise_var_inputs* dev_in, void* d_out_mean, void* d_out_rgb,
                           void* d_out_variance, void* d_scratch, uint64_t scratch_bytes, void* hip_stream, crt_denoise_info* info);

/* First-order feature regression with non-local-means weights (Moon et al. 2014; Bitterli et al. 2016, "NFOR"): in the window around a
 * pixel the colour is fitted as a linear function of the guides -- weighted least squares, the weight of a tap crt_denoise_nlm's patch
 * term -- and the output is the fit's value at the pixel.  Where the three filters above take a weighted mean, which cannot follow a
 * gradient, this one follows whatever is linear in the enabled features.  The weights may come from another image than the one that is
 * fitted (weight_color / weight_variance: with the half frames of crt_half_buffers, half B for half A and the reverse, weight and noise
 * are independent).  An image operation: row-major, no scene handle; buffers as crt_denoise_var's (3 floats per pixel, depth 1).
 * Inputs: color and variance required; weight_color NULL = color, weight_variance NULL = variance (with both given `variance` itself is
 * not read); albedo / normal / depth are read only where `features` enables them.  Outputs: out_mean and / or out_rgb (the frame's tone
 * map of the mean), not both NULL.  There is no out_variance (see below).
 *   wc, wv = weight_color, weight_variance;  k2 = k * k;  F = the regressors enabled in `features`, M = F + 1
 * For pixel p and window offset o = (ox, oy), oy = -radius..radius outer, ox = -radius..radius inner, q = p + o; a q outside the image
 * is skipped:
 *   e_p = crt_denoise_nlm's e_p of (p, o), to the bit: its v, g (the 3x3 Gaussian of the summed wv), pair term d, row sums in its order,
 *         its skipping rule, n, Dm = D / (float)n and the clamp Dm < 0 ? 0 : Dm -- evaluated on wc and wv with this call's patch, k, alpha
 *   w   = exp(-e_p)                                  (det_expf; crt_denoise_nlm's guide terms e_n, e_a, e_d are NOT in the weight)
 *   x(q): M entries, the enabled ones of the following in this order, then the constant 1 LAST:
 *     CRT_REGRESS_NORMAL    (normal(q).c - normal(p).c) / sigma_normal                    c = x, y, z
 *     CRT_REGRESS_ALBEDO    (albedo(q).c - albedo(p).c) / sigma_albedo                    c = x, y, z
 *     CRT_REGRESS_DEPTH     m = depth(p) > depth(q) ? depth(p) : depth(q);   m > 0 ? (depth(q) - depth(p)) / (sigma_depth * m) : 0
 *     CRT_REGRESS_POSITION  (float)ox / (sigma_position * (float)radius),   (float)oy / (sigma_position * (float)radius)
 *   for i = 0..F:   wx = w * x_i;   A[i][j] = A[i][j] + wx * x_j  for j = i..F;   B[i][c] = B[i][c] + wx * color(q).c  for c = r, g, b
 * Every entry of x is centred on p, so the fit's value at p is the coefficient of the constant.  After the window:
 *   S = A[F][F] (the sum of the weights),  Z_c = B[F][c]
 *   A[i][i] = A[i][i] + ridge * S                    for i < F
 *   for k = 0..F-1:  d = A[k][k];  !(d > 0): fall back
 *     for i = k+1..F:  f = A[k][i] / d;   A[i][j] = A[i][j] - f * A[k][j]  for j = i..F;   B[i][c] = B[i][c] - f * B[k][c]
 *   d = A[F][F];  !(d > 0): fall back;   out_mean(p).c = B[F][c] / d
 *   fall back:  out_mean(p).c = Z_c / S              (the zero-order result: the weighted mean of the window)
 * Gaussian elimination of the symmetric system on its upper triangle, without pivoting and without back-substitution: only the last
 * unknown is wanted.  All sums start at +0.0f and run in window order; fp32 with one IEEE operation per symbol (no FMA, no reciprocal
 * multiply).  A NaN pivot falls back by the !(d > 0) test; non-finite inputs are otherwise not special-cased.  info->fallback_pixels
 * counts the pixels that fell back.  With features = 0 the filter is the zero-order one (M = 1: B[0] / A[0][0] = Z / S) and no pixel
 * falls back unless S is not > 0.
 * A disabled feature has no row and no column: the library instantiates its kernel per mask (csrc/crt_regress.hip), so a smaller mask
 * runs the smaller system and a disabled feature's buffer may be NULL or not, with the same bits.  An enabled feature with a NULL buffer
 * is CRT_ERR_INVALID_ARG.  The sigmas here scale the features (and with them what `ridge` means): each > 0 and not NaN; sigma_position is
 * in units of radius.  ridge >= 0 and finite; radius 1 .. 8, patch 0 .. 3, k > 0 and finite, alpha >= 0 and finite as crt_denoise_nlm;
 * a null params, inputs, color or variance, a size of 0, unknown mask bits, two NULL outputs, a negative device or a scratch buffer that
 * is missing, too small or not 16-byte aligned is CRT_ERR_INVALID_ARG, checked before any device call.  (A side longer than 2^24
 * pixels: CRT_ERR_UNSUPPORTED.)  Scratch: 64 B per pixel (crt_denoise_regress_scratch_bytes: four float4 planes -- (weight colour, g),
 * (normal, depth), (albedo, -), (colour, 0)).  The kernel has one form, the shared one (k_nlm_shared's staging and phases).
 * Not done: the variance left after the fit (it needs the fit's equivalent kernel, a second pass), second-order fits, iterating the
 * filter or pre-filtering the features, specular guides as regressors, temporal inputs, per-channel variances.
 * crt_denoise_regress_defaults fills radius 5, patch 1, k 0.6, alpha 1, sigma_normal 0.5, sigma_albedo 0.1, sigma_depth 0.05,
 * sigma_position 2, ridge 0.4 and every feature: the set with the smallest summed error relative to crt_denoise_var's defaults on the
 * 160x120 spp 8 and spp 32 frames of cornell-box, veach-mis and the textured cornell-box (docs/experiments.md, "The feature-regression
 * filter"). */
#define CRT_REGRESS_NORMAL 1u
#define CRT_REGRESS_ALBEDO 2u
#define CRT_REGRESS_DEPTH 4u
#define CRT_REGRESS_POSITION 8u
typedef struct {
    uint32_t width, height;
    uint32_t radius;      /* window (2 radius + 1)^2: 1 .. 8 */
    uint32_t patch;       /* patches of (2 patch + 1)^2: 0 .. 3 */
    float k, alpha;       /* as crt_nlm_params */
    float sigma_normal, sigma_albedo, sigma_depth;   /* the scales of the features: > 0, not NaN */
    float sigma_position; /* in units of radius: > 0, not NaN */
    float ridge;          /* >= 0, finite: added to the features' diagonal, times the sum of the weights */
    uint32_t features;    /* CRT_REGRESS_* bits; 0: the zero-order filter */
} crt_regress_params;
typedef struct {
    const float* color; const float* variance;
    const float* weight_color;      /* NULL: color */
    const float* weight_variance;   /* NULL: variance */
    const float* albedo; const float* normal; const float* depth;
} crt_regress_inputs;
typedef struct {
    float total_ms;
    uint64_t fallback_pixels;  /* pixels that took Z / S */
} crt_regress_info;
int crt_denoise_regress_defaults(crt_regress_params* params);
int crt_denoise_regress_scratch_bytes(uint32_t width, uint32_t height, uint64_t* bytes);
int crt_denoise_regress(int device, const crt_regress_params* params, const crt_regress_inputs* host_in, float* out_mean, uint8_t* out_rgb,
                        crt_regress_info* info);
int crt_denoise_regress_device(int device, const crt_regress_params* params, const crt_regress_inputs* dev_in, void* d_out_mean, void* d_out_rgb,
                               void* d_scratch, uint64_t scratch_bytes, void* hip_stream, crt_regress_info* info);

/* Albedo demodulation: filter irradiance, not radiance.  crt_demodulate takes the emission off a frame and divides it by the albedo,
 * crt_modulate puts both back, so that crt_denoise* and crt_temporal* in between see neither the surfaces' colour nor the lights
 * (SVGF, Schied et al. 2017, section 4).  With emission and diffuse_albedo of crt_render_aov_shading the factorisation is exact for this
 * renderer: frame = emission + sum_k kd(m_k) * I_k / S.  Image operations: no scene handle, no scratch.  Row-major images of width x
 * height, 3 floats per pixel every one (out_rgb: 3 bytes).  Per pixel and channel, in fp32, one IEEE operation per symbol (no FMA, no
 * reciprocal multiply):
 *   use = albedo > albedo_floor                                   (false for a NaN albedo)
 *   crt_demodulate:  d = color - emission                         (emission NULL: d = color)
 *                    irradiance   = use ? d / albedo : d
 *                    out_variance = use ? variance / (albedo * albedo) : variance      (variance, out_variance: both or neither)
 *   crt_modulate:    m = use ? irradiance * albedo : irradiance
 *                    c = m + emission                             (emission NULL: c = m)
 *                    out_mean = c;  out_rgb = the frame's tone map of c (the bits crt_render writes for that mean); either may be
 *                    NULL, not both
 * Where the albedo is not above the floor the value passes through both ways, so the pair is the identity there (a pixel without a hit,
 * a channel the surface absorbs: its radiance is +0 anyway).  Non-finite inputs are not special-cased: the arithmetic defines the
 * result.  albedo_floor must be >= 0 and not NaN; crt_modulate_defaults fills 0 (width and height 0).
 * A null params, image, albedo or output pointer, a size of 0, a bad floor, variance without out_variance or the reverse, or two NULL
 * outputs of crt_modulate is CRT_ERR_INVALID_ARG, checked before any device call.  (A side longer than 2^24 pixels:
 * CRT_ERR_UNSUPPORTED.)  An output may be the input image itself; otherwise buffers must not overlap. */
typedef struct {
    uint32_t width, height;
    float albedo_floor;
} crt_modulate_params;
typedef struct {
    float total_ms;    /* HIP-event time of the call's kernel on its stream */
} crt_modulate_info;
int crt_modulate_defaults(crt_modulate_params* params);
/* host buffers; allocates and frees its own device memory on `device`; info optional */
int crt_demodulate(int device, const crt_modulate_params* params, const float* color, const float* albedo, const float* emission /* may be NULL */,
                   const float* variance /* may be NULL */, float* out_irradiance, float* out_variance /* with variance */, crt_modulate_info* info);
int crt_modulate(int device, const crt_modulate_params* params, const float* irradiance, const float* albedo, const float* emission /* may be NULL */,
                 float* out_mean, uint8_t* out_rgb, crt_modulate_info* info);
/* Everything in device memory on `device`; enqueued on hip_stream (NULL = default stream) without synchronizing, unless info != NULL
 * (the call then synchronizes the stream to read the timer).  Buffers that are all 16-byte aligned (out_rgb: 4-byte) take 16-byte
 * accesses; any other alignment of whole floats works, component by component. */
int crt_demodulate_device(int device, const crt_modulate_params* params, const void* d_color, const void* d_albedo, const void* d_emission,
                          const void* d_variance, void* d_out_irradiance, void* d_out_variance, void* hip_stream, crt_modulate_info* info);
int crt_modulate_device(int device, const crt_modulate_params* params, const void* d_irradiance, const void* d_albedo, const void* d_emission,
                        void* d_out_mean, void* d_out_rgb, void* hip_stream, crt_modulate_info* info);

/* Temporal accumulation with reprojection (the temporal half of SVGF, Schied et al. 2017): the frame of the current camera is blended
 * with the accumulated frame of the previous camera, fetched where the surface point of each pixel was seen then, so that a moving
 * camera keeps most of the samples it has already paid for.  An image operation: no scene handle, no scratch buffer.  Row-major images
 * of width x height; color, variance, normal 3 floats per pixel; depth, history 1 float per pixel; id 1 int32 per pixel: what crt_render
 * (out_mean), crt_variance and crt_render_aov (depth, normal, material or tri) return, as they are.  `history` is the number of frames
 * accumulated in a pixel.  The caller keeps out_color, out_variance, out_history and the current frame's depth, normal and id as the next
 * call's crt_temporal_history (with prev = this call's cur) and ping-pongs the buffers: outputs must not overlap any input.
 * With scale = det_tanf(cur.fov_y / 2), scale' = det_tanf(prev.fov_y / 2), ar = (float)W / (float)H (host, as the camera rays take
 * them), iv = cur.inv_view, iv' = prev.inv_view, eye = cur.eye, eye' = prev.eye, per pixel p = (x, y):
 *   sx = (((2 * ((float)x + 0.5f)) / W - 1) * scale) * ar          sy = (1 - (2 * ((float)y + 0.5f)) / H) * scale
 *   cd = unit3(-sx, sy, 1)                       unit3(a): z = a.x*a.x + (a.y*a.y + a.z*a.z); z > 0 ? a / sqrt(z) : a
 *   wd = (iv[0]*cd.x + (iv[3]*cd.y + iv[6]*cd.z), iv[1]*cd.x + (iv[4]*cd.y + iv[7]*cd.z), iv[2]*cd.x + (iv[5]*cd.y + iv[8]*cd.z))
 *   d  = unit3(wd)                               the pixel-centre camera ray
 *   P  = eye + d * depth(p)                      per component: one multiply, one add
 *   v  = P - eye'
 *   cx = iv'[0]*v.x + (iv'[1]*v.y + iv'[2]*v.z)   cy = iv'[3]*v.x + (iv'[4]*v.y + iv'[5]*v.z)   cz = iv'[6]*v.x + (iv'[7]*v.y + iv'[8]*v.z)
 *   tp = sqrt(v.x*v.x + (v.y*v.y + v.z*v.z))     the depth the previous frame would have stored for P
 *   fx = (((((-cx) / cz) / (scale' * ar)) + 1) * W) / 2 - 0.5f     fy = (((1 - (cy / cz) / scale') * H) / 2) - 0.5f
 *   ok = depth(p) > 0 && cz > 0 && fx > -1 && fx < W && fy > -1 && fy < H                  (a NaN anywhere: false)
 *   x0 = floor(fx); wx = fx - x0; y0 = floor(fy); wy = fy - y0
 *   taps q = (x0 + i, y0 + j), j = 0, 1 outer, i = 0, 1 inner; a tap counts iff it is inside the image
 *        && prev.depth(q) > 0 && |prev.depth(q) - tp| <= depth_tolerance * tp
 *        && (normals given: dn = normal(p) - prev.normal(q); dn.x*dn.x + dn.y*dn.y + dn.z*dn.z <= normal_tolerance * normal_tolerance)
 *        && (ids given: id(p) == prev.id(q));  for a tap that counts
 *      b  = (i ? wx : 1 - wx) * (j ? wy : 1 - wy)
 *      hc = hc + prev.color(q) * b;  hv = hv + prev.variance(q) * b;  hn = hn + prev.history(q) * b;  ws = ws + b
 *   if ok && ws > 0.015625f:
 *      hc = hc / ws; hv = hv / ws; hn = hn / ws;   n = hn + 1;   a = 1 / n;   a = a < alpha_min ? alpha_min : a;   k = 1 - a
 *      out_color = hc * k + color(p) * a;   out_variance = hv * (k * k) + variance(p) * (a * a);   out_history = n
 *   else (reset):  out_color = color(p);  out_variance = variance(p);  out_history = 1
 * hc, hv (per channel), hn and ws start at +0.0f; sums run left to right as written; every * + - / and sqrt is one IEEE fp32 operation
 * (no FMA, no reciprocal multiply).  Non-finite colours or variances in a tap that counts are not special-cased.  With alpha_min = 0 this
 * would be the running mean of the frames; alpha_min bounds how long a stale sample lives.
 * The pixel-centre ray and the MEAN hit distance of the pixel's jittered samples only approximate the surface point the pixel shows (at
 * a silhouette the mean depth lies between two surfaces): the tolerances absorb that error, and a pixel they reject is reset.
 * The variance line treats the two frames as independent estimates: render consecutive frames with DIFFERENT seeds, or the accumulated
 * variance understates the noise (the same seed and camera would add the same frame to itself).
 * Required: cur.color, cur.depth, out_color, out_history; with a history also prev.color, prev.history, prev.depth.  normal and id: in
 * both frames or in neither.  cur.variance and out_variance: both or neither; prev.variance is then required too.  out_rgb (optional) is
 * the frame's tone map of out_color, the bits crt_render writes for that mean.  host_prev / dev_prev == NULL: no history, every pixel
 * resets.  crt_temporal_defaults fills depth_tolerance 0.05, normal_tolerance 0.5, alpha_min 0.05 (sizes and cameras zero); the two
 * tolerances are the denoiser's sigma_depth and sigma_normal and were tuned on nothing; alpha_min was compared with 0.1 and 0.2 on two
 * scenes and nothing more (docs/experiments.md, "Temporal accumulation").
 * CRT_ERR_INVALID_ARG, checked before any device call: a null required pointer, a size of 0, a tolerance that is not > 0 (NaN included;
 * +inf is allowed and switches its test off), alpha_min outside (0, 1], a half-given pair.  A side longer than 2^24 pixels or more than
 * 2^31 thread blocks of 64 x 4 pixels: CRT_ERR_UNSUPPORTED.
 * Not done here: a wider search when the four taps fail, moving geometry, tiled shards.  Clamping the history to the colours around p
 * (view-dependent highlights lag behind the camera) is crt_temporal_clamped, below. */
typedef struct {
    uint32_t width, height;
    crt_camera cur, prev;          /* camera of the current frame / of the frame the history was made with */
    float depth_tolerance;         /* relative; > 0, not NaN, +inf allowed */
    float normal_tolerance;        /* > 0, not NaN, +inf allowed */
    float alpha_min;               /* 0 < alpha_min <= 1 */
} crt_temporal_params;
typedef struct { const float* color; const float* variance; const float* depth; const float* normal; const int32_t* id; } crt_temporal_frame;   /* current frame */
typedef struct { const float* color; const float* variance; const float* history; const float* depth; const float* normal; const int32_t* id; } crt_temporal_history;
typedef struct {
    float total_ms;        /* HIP-event time of the call's kernel on its stream */
    uint64_t reprojected;  /* pixels that took the history */
} crt_temporal_info;
int crt_temporal_defaults(crt_temporal_params* params);
/* host buffers; allocates and frees its own device memory on `device`; info optional */
int crt_temporal(int device, const crt_temporal_params* params, const crt_temporal_frame* host_cur, const crt_temporal_history* host_prev /* may be NULL */,
                 float* out_color, float* out_variance, float* out_history, uint8_t* out_rgb, crt_temporal_info* info);
/* Everything in device memory on `device`; enqueued on hip_stream (NULL = default stream) without synchronizing, unless info != NULL
 * (the call then counts the reprojected pixels and synchronizes the stream to read them and the timer). */
int crt_temporal_device(int device, const crt_temporal_params* params, const crt_temporal_frame* dev_cur, const crt_temporal_history* dev_prev,
                        void* d_out_color, void* d_out_variance, void* d_out_history, void* d_out_rgb, void* hip_stream, crt_temporal_info* info);

/* crt_temporal with the history clamped to its neighbourhood (the variance clamp of temporal anti-aliasing, Salvi 2016): before the
 * blend, the interpolated history colour of a pixel is clamped, per channel, to mean +- gamma standard deviations of the CURRENT frame's
 * colour over the (2 * radius + 1)^2 pixels around it, so that a history that no longer resembles what the pixel shows now (a
 * view-dependent highlight that has moved on, a surface the tolerances let through) is pulled to the present instead of blended in.
 * Everything of crt_temporal's definition up to and including `hc = hc / ws; ... k = 1 - a` is unchanged.  For a pixel p = (x, y) that
 * takes the history (ok && ws > 0.015625f), with H = hc / ws per channel and r = radius:
 *   s1 = s2 = +0.0f per channel; cnt = +0.0f
 *   taps t = (x + dx, y + dy), dy = -r .. r outer, dx = -r .. r inner; a tap outside the image is skipped (p itself always counts)
 *        s1 = s1 + color(t);   s2 = s2 + color(t) * color(t);   cnt = cnt + 1
 *   mu = s1 / cnt;   e = s2 / cnt - mu * mu;   e = e < 0 ? 0 : e;   sd = sqrt(e);   w = gamma * sd
 *   lo = mu - w;     hi = mu + w
 *   Hc = H < lo ? lo : H;    Hc = Hc > hi ? hi : Hc
 *   out_color = Hc * k + color(p) * a
 *   clamped(p) = one of the six comparisons (two per channel) was true
 * Every * + - / and sqrt is one IEEE fp32 operation (no FMA, no reciprocal multiply); sums run left to right as written.  A NaN in H, lo
 * or hi makes both comparisons false and H passes through; with gamma = +inf, w is +inf or (sd = 0) NaN and nothing is ever clamped:
 * the call then writes crt_temporal's bits.  The neighbourhood takes every tap inside the image whatever its depth or ID: a box that
 * spans two surfaces is wider and clamps less, the safe side.
 * out_variance and out_history are crt_temporal's, from the UNclamped hv and hn: the carried variance therefore understates the noise of
 * a clamped pixel (its history was replaced by a statistic of one frame), and its history length overstates what it has accumulated.
 * Reset pixels and calls without a history are crt_temporal's.  clamp == NULL: the call is crt_temporal / crt_temporal_device (the same
 * kernel, the same bits; clamped = 0).  crt_temporal_clamp_defaults fills radius 1, gamma 1 (docs/experiments.md, "The neighbourhood
 * clamp": the setting with the smallest summed error ratio over four sequences; what it does and does not repair is stated there).
 * CRT_ERR_INVALID_ARG, checked before any device call: everything crt_temporal refuses, a radius outside 1 .. 3, a gamma that is
 * negative or NaN.
 * Not done here: cutting the history length or inflating the variance of clamped pixels, clamping in another colour space (YCoCg), a
 * neighbourhood restricted to the pixel's surface, the 3x3 fallback search, tiled shards and crt_multi. */
typedef struct {
    uint32_t radius;   /* neighbourhood is (2*radius+1)^2 pixels of the CURRENT frame's colour; 1 .. 3 */
    float    gamma;    /* half-width of the box in standard deviations; >= 0, not NaN, +inf allowed (never clamps) */
} crt_temporal_clamp;
typedef struct {
    float total_ms;        /* as crt_temporal_info */
    uint64_t reprojected;  /* as crt_temporal_info */
    uint64_t clamped;      /* of those: pixels where at least one channel of the history was moved by the clamp */
} crt_temporal_clamp_info;
int crt_temporal_clamp_defaults(crt_temporal_clamp* clamp);
/* host buffers, as crt_temporal; clamp may be NULL; info optional */
int crt_temporal_clamped(int device, const crt_temporal_params* params, const crt_temporal_clamp* clamp, const crt_temporal_frame* host_cur,
                         const crt_temporal_history* host_prev /* may be NULL */, float* out_color, float* out_variance, float* out_history,
                         uint8_t* out_rgb, crt_temporal_clamp_info* info);
/* device buffers on hip_stream, as crt_temporal_device (info != NULL: counts both, synchronizes the stream) */
int crt_temporal_clamped_device(int device, const crt_temporal_params* params, const crt_temporal_clamp* clamp, const crt_temporal_frame* dev_cur,
                                const crt_temporal_history* dev_prev, void* d_out_color, void* d_out_variance, void* d_out_history, void* d_out_rgb,
                                void* hip_stream, crt_temporal_clamp_info* info);

/* crt_temporal_clamped that also carries the first two moments of what each pixel was seen to show over its history, so that the
 * variance handed to crt_denoise_var can be measured (crt_variance_estimate, below) instead of carried: two more history planes in
 * (prev_moments: m1, m2, 3 floats per pixel each, row-major) and two more out (out_m1, out_m2), kept by the caller with the rest of the
 * history.  Everything of crt_temporal_clamped's definition stands unchanged -- taps, tolerances, ws > 0.015625f, n, a, k, the clamp,
 * out_color, out_variance, out_history, both counts -- and clamp may be NULL (then crt_temporal's).  In addition, per channel, with
 * c = color(p):
 *   for a tap that counts, with the same b:    h1 = h1 + prev.m1(q) * b;   h2 = h2 + prev.m2(q) * b          (both from +0.0f)
 *   a pixel that takes the history:            h1 = h1 / ws;   h2 = h2 / ws
 *                                              out_m1 = h1 * k + c * a;    out_m2 = h2 * k + (c * c) * a
 *   a reset pixel, or no history:              out_m1 = c;                 out_m2 = c * c
 * Every * + / is one IEEE fp32 operation (no FMA), left to right as written.  The moments are never clamped: m1 is the UNclamped running
 * mean, so with clamp == NULL the bits of out_m1 are the bits of out_color, and with a clamp they differ on the pixels it moved -- which
 * is why m1 is carried at all (m2 - out_color^2 would measure the distance to the clamped mean, not the pixel's own noise).
 * cur.variance / out_variance stay optional, both or neither: at one sample per pixel, where crt_variance has nothing to return, the
 * caller gives neither.  Non-finite values are not special-cased.
 * CRT_ERR_INVALID_ARG, checked before any device call: everything crt_temporal_clamped refuses, a NULL out_m1 or out_m2, moment planes
 * without a history or a history without moment planes, a NULL plane inside a given struct.
 * Not done here: moments of the luminance alone, of the demodulated colour, a shorter history for clamped pixels. */
typedef struct { const float* m1; const float* m2; } crt_temporal_moment_planes;  /* 3 floats per pixel each, row-major */
/* host buffers, as crt_temporal_clamped; clamp may be NULL; host_prev_moments is NULL iff host_prev is NULL; info optional */
int crt_temporal_moments(int device, const crt_temporal_params* params, const crt_temporal_clamp* clamp, const crt_temporal_frame* host_cur,
                         const crt_temporal_history* host_prev /* may be NULL */, const crt_temporal_moment_planes* host_prev_moments,
                         float* out_color, float* out_variance, float* out_history, float* out_m1, float* out_m2, uint8_t* out_rgb,
                         crt_temporal_clamp_info* info);
/* device buffers on hip_stream, as crt_temporal_clamped_device (info != NULL: counts both, synchronizes the stream) */
int crt_temporal_moments_device(int device, const crt_temporal_params* params, const crt_temporal_clamp* clamp, const crt_temporal_frame* dev_cur,
                                const crt_temporal_history* dev_prev, const crt_temporal_moment_planes* dev_prev_moments, void* d_out_color,
                                void* d_out_variance, void* d_out_history, void* d_out_m1, void* d_out_m2, void* d_out_rgb, void* hip_stream,
                                crt_temporal_clamp_info* info);

/* crt_temporal_clamped with two reprojections per mirror pixel (the "virtual motion" of real-time denoisers).  A pixel of a planar mirror
 * shows two things at once: its own diffuse shading, which moves with the surface, and the mirrored scene, which moves rigidly with its
 * VIRTUAL IMAGE -- the point at path_depth along the pixel's camera ray (crt_render_aov_specular: the length of the mirror chain).
 * crt_temporal reprojects through the first hit alone, so a reflection that moves across a still plate is accumulated as if it stood
 * still.  This call fetches a history through each point and blends the one that agrees with what the pixel shows now.
 * Two more planes per frame, three with last_normal (cur_spec, prev_spec: crt_render_aov_specular's path_depth, bounces and last_normal as
 * they are, row-major; path_depth, bounces 1 float per pixel, last_normal 3); the caller keeps the current frame's with the rest of the
 * history, as it keeps depth, normal and id.  Everything is IEEE fp32, every * + - / and sqrt one operation (no FMA, no reciprocal
 * multiply), sums left to right as written.  Per pixel p = (x, y) of a call with a history:
 * 1. Surface candidate S: crt_temporal's definition, unchanged, up to and including the tap loop: hc_S, hv_S, hn_S, ws_S;
 *      valid_S = ok && ws_S > 0.015625f
 * 2. Virtual candidate V, tried iff  cur.bounces(p) >= min_bounces  (a NaN: false)  &&  cur.path_depth(p) > 0:
 *      Pv = eye + d * cur.path_depth(p)           d: crt_temporal's pixel-centre ray
 *      v, cx, cy, cz, tp, fx, fy, x0, wx, y0, wy: exactly as crt_temporal computes them from P, here from Pv
 *      ok_V = cur.path_depth(p) > 0 && cz > 0 && fx > -1 && fx < W && fy > -1 && fy < H           (a NaN anywhere: false)
 *      taps q = (x0 + i, y0 + j), j outer, i inner; a tap counts iff it is inside the image
 *           && prev.bounces(q) >= min_bounces && prev.path_depth(q) > 0
 *           && |prev.path_depth(q) - tp| <= depth_tolerance * tp
 *           && (last normals given: crt_temporal's normal test on cur.last_normal(p) and prev.last_normal(q))
 *           && (ids given: id(p) == prev.id(q)             -- the FIRST-hit id: the same mirror)
 *      for a tap that counts, with the same b:  hc_V, hv_V, hn_V, ws_V as in crt_temporal
 *      valid_V = ok_V && ws_V > 0.015625f
 * 3. Choice, made only when valid_V; r = dual.radius:
 *      s1 = +0.0f per channel; cnt = +0.0f;  taps t = (x + dx, y + dy), dy = -r .. r outer, dx = -r .. r inner, a tap outside the image
 *      is skipped:  s1 = s1 + color(t);  cnt = cnt + 1            (crt_temporal_clamped's loop)        mu = s1 / cnt
 *      for each valid candidate:  H = hc / ws per channel;  dx = H.x - mu.x, dy = H.y - mu.y, dz = H.z - mu.z;  e = dx*dx + (dy*dy + dz*dz)
 *      V is taken iff  !valid_S || e_V < e_S        a tie keeps S; a NaN in either e makes the comparison false and keeps S; with S
 *      invalid V is taken whatever e_V is
 * 4. Blend: the chosen candidate's hc, hv, hn, ws go on through crt_temporal_clamped's text from `hc = hc / ws` to the end, the clamp (if
 *    any: clamp may be NULL) on the chosen H with the clamp's own radius.  Neither candidate valid: the pixel resets.
 * 5. Counts (info): virtual_tried = pixels for which V was tried (step 2's condition, whatever became of it), virtual_taken = pixels
 *    that took V; reprojected (pixels that took either history) and clamped as in crt_temporal_clamped.
 * Without a history every pixel resets, nothing is tried and no specular plane is read.  Two consequences:
 *   - with min_bounces = +inf (finite bounces), or with cur.bounces zero everywhere, no pixel tries V and the call writes
 *     crt_temporal_clamped's bits and counts (crt_temporal's with clamp == NULL);
 *   - crt_temporal, crt_temporal_clamped and crt_temporal_moments are what they were: their kernels are not the ones of this call.
 * The choice compares single interpolated colours with a mean of (2r+1)^2 noisy ones: at low sample counts it is itself noisy, and where
 * both histories lie equally far from the mean it keeps S.  crt_temporal_dual_defaults (into a crt_temporal_dual_params) fills radius 1, min_bounces 0.5: tuned on
 * nothing (docs/experiments.md, "Dual reprojection", has a small sweep; the defaults were set before it and stayed).
 * CRT_ERR_INVALID_ARG, checked before any device call: everything crt_temporal_clamped refuses, a NULL dual, a radius outside 1 .. 3, a
 * min_bounces that is not > 0 (NaN included; +inf is allowed), a NULL cur_spec, a missing path_depth or bounces, last_normal given in
 * one frame only, prev_spec without prev or prev without prev_spec.
 * Not done here: curved mirrors (the virtual point is then only an approximation: the reflection does not move rigidly), rough plates
 * (path_depth follows mirror bounces only), refraction, the moments form (crt_temporal_moments with two candidates), splitting the
 * radiance into a surface layer and a reflected layer with a history each, blending the two histories, tiled shards and crt_multi. */
typedef struct {
    uint32_t radius;       /* neighbourhood of the choice: (2*radius+1)^2 pixels of the CURRENT frame's colour; 1 .. 3 */
    float    min_bounces;  /* share of reflected samples from which a pixel (and a tap) counts as a mirror; > 0, not NaN, +inf allowed (never tries) */
} crt_temporal_dual_params;
typedef struct { const float* path_depth; const float* bounces; const float* last_normal; } crt_temporal_specular_planes;
    /* path_depth, bounces: 1 float per pixel, required; last_normal: 3 floats per pixel, in both frames or in neither */
typedef struct {
    float total_ms;          /* as crt_temporal_info */
    uint64_t reprojected;    /* pixels that took a history, S or V */
    uint64_t clamped;        /* as crt_temporal_clamp_info */
    uint64_t virtual_tried;  /* pixels for which the virtual candidate was tried */
    uint64_t virtual_taken;  /* pixels that took it */
} crt_temporal_dual_info;
int crt_temporal_dual_defaults(crt_temporal_dual_params* dual);
/* host buffers, as crt_temporal_clamped; clamp may be NULL; host_prev_spec is NULL iff host_prev is NULL; info optional */
int crt_temporal_dual(int device, const crt_temporal_params* params, const crt_temporal_clamp* clamp, const crt_temporal_dual_params* dual,
                      const crt_temporal_frame* host_cur, const crt_temporal_specular_planes* host_cur_spec,
                      const crt_temporal_history* host_prev /* may be NULL */, const crt_temporal_specular_planes* host_prev_spec,
                      float* out_color, float* out_variance, float* out_history, uint8_t* out_rgb, crt_temporal_dual_info* info);
/* device buffers on hip_stream, as crt_temporal_clamped_device (info != NULL: counts all four, synchronizes the stream) */
int crt_temporal_dual_device(int device, const crt_temporal_params* params, const crt_temporal_clamp* clamp, const crt_temporal_dual_params* dual,
                             const crt_temporal_frame* dev_cur, const crt_temporal_specular_planes* dev_cur_spec,
                             const crt_temporal_history* dev_prev, const crt_temporal_specular_planes* dev_prev_spec, void* d_out_color,
                             void* d_out_variance, void* d_out_history, void* d_out_rgb, void* hip_stream, crt_temporal_dual_info* info);

/* Variance from temporal moments (SVGF, Schied et al. 2017, section 4.2): what crt_denoise_var takes as `variance`, estimated from what
 * each pixel was actually seen to do over its history instead of carried along with it.  An image operation: no scene handle, no scratch.
 * m1, m2, history: what crt_temporal_moments wrote (required); normal, depth: the current frame's AOVs (either may be NULL: its term is
 * +0.0f).  Output: 3 floats per pixel.  Per pixel p = (x, y) and per channel, with n = history(p), fm = (float)min_history, r = radius:
 *   temporal branch, n >= fm:
 *      e = m2(p) - m1(p) * m1(p);   e = e < 0 ? 0 : e   (NaN stays NaN);   var = e
 *   spatial branch, otherwise (a NaN n lands here): the pixel has not seen enough frames, so its neighbours stand in for them
 *      taps q = (x + dx, y + dy), dy = -r .. r outer, dx = -r .. r inner; a tap outside the image is skipped
 *        e_n, e_d: exactly crt_denoise's lines (e_d on the relative depth, m > 0 ? r * r : 0)
 *        w  = exp(-(e_n + e_d))                                                                  (det_expf)
 *        s1 = s1 + m1(q) * w;   s2 = s2 + m2(q) * w;   sw = sw + w                               (all from +0.0f)
 *      mu = s1 / sw;   e = s2 / sw - mu * mu;   e = e < 0 ? 0 : e;   var = e * (fm / n)          (the boost SVGF gives a short history)
 *   of_mean != 0:   ne = n > history_cap ? history_cap : n;   var = var / ne
 * Every * + - / is one IEEE fp32 operation (no FMA, no reciprocal multiply), left to right as written.  Non-finite inputs are not
 * special-cased: the arithmetic defines the result.  of_mean = 0 is SVGF's choice, the variance of ONE frame's sample of the pixel;
 * of_mean = 1 divides by the number of frames the blend can hold (history_cap = 2 / alpha_min - 1 for crt_temporal's defaults), an
 * estimate of the variance of the accumulated mean itself.  docs/experiments.md, "Variance from temporal moments", has both measured.
 * crt_variance_estimate_defaults fills min_history 4, radius 3, sigma_normal 0.5, sigma_depth 0.05, of_mean 0, history_cap 39.
 * CRT_ERR_INVALID_ARG, checked before any device call: a null required pointer, a size of 0, min_history 0, a radius outside 1 .. 3, a
 * sigma that is not > 0, a history_cap that is < 1 or NaN.  A side longer than 2^24 pixels or more than 2^31 thread blocks of 64 x 4
 * pixels: CRT_ERR_UNSUPPORTED. */
typedef struct {
    uint32_t width, height;
    uint32_t min_history;     /* below this history length the spatial estimate is used; >= 1 */
    uint32_t radius;          /* spatial window (2 radius + 1)^2; 1 .. 3 */
    float sigma_normal, sigma_depth;   /* as crt_denoise's; > 0, not NaN, +inf switches the term off */
    uint32_t of_mean;         /* 0: variance of one frame's sample (SVGF); 1: divided by the capped history length */
    float history_cap;        /* of_mean only: n_e = history > cap ? cap : history; >= 1, +inf allowed */
} crt_variance_estimate_params;
typedef struct { const float* m1; const float* m2; const float* history; const float* normal; const float* depth; } crt_variance_estimate_inputs;
typedef struct {
    float total_ms;        /* HIP-event time of the call's kernel on its stream */
    uint64_t spatial;      /* pixels that took the spatial branch */
} crt_variance_estimate_info;
int crt_variance_estimate_defaults(crt_variance_estimate_params* params);
/* host buffers; allocates and frees its own device memory on `device`; info optional */
int crt_variance_estimate(int device, const crt_variance_estimate_params* params, const crt_variance_estimate_inputs* host_in,
                          float* out_variance, crt_variance_estimate_info* info);
/* Everything in device memory on `device`; enqueued on hip_stream (NULL = default stream) without synchronizing, unless info != NULL
 * (the call then counts the pixels of the spatial branch and synchronizes the stream to read them and the timer). */
int crt_variance_estimate_device(int device, const crt_variance_estimate_params* params, const crt_variance_estimate_inputs* dev_in,
                                 void* d_out_variance, void* hip_stream, crt_variance_estimate_info* info);

/* Guide-driven upsampling: an image rendered at low_width x low_height brought to width x height along guides that exist at BOTH sizes
 * (joint bilateral upsampling, Kopf et al. 2007).  Meant for irradiance (crt_demodulate of a low-resolution frame): the first-hit passes
 * that produce albedo, normal and depth are cheap at full size, paths are not, and irradiance is smooth between geometric edges.  An
 * image operation: no scene handle, no scratch; the taps come straight from the caller's buffers.  Row-major images; color, variance,
 * albedo and normal 3 floats per pixel, depth 1.  `low` holds the low-resolution image and its guides, `guides` the output-resolution
 * guides.  Per output pixel p = (x, y), all in fp32:
 *   sx = (float)low_width / (float)width                      sy = (float)low_height / (float)height
 *   u  = ((float)x + 0.5f) * sx - 0.5f                        v  = ((float)y + 0.5f) * sy - 0.5f
 *   x0 = (int)floorf(u)                                       y0 = (int)floorf(v)
 *        (low pixel X covers the part [X / sx, (X + 1) / sx) of the output's columns: the camera ray divides pixel + jitter by the width)
 *   taps q = (tx, ty): ty = y0 - radius + 1 .. y0 + radius outer, tx = x0 - radius + 1 .. x0 + radius inner; a tap outside the low image
 *   is skipped (nothing is added for it)
 *     wx = 1.0f - fabsf(u - (float)tx) / (float)radius        wy = 1.0f - fabsf(v - (float)ty) / (float)radius        hw = wy * wx
 *     e_n, e_a, e_d: exactly crt_denoise's lines, between guides(p) (output resolution) and low(q) (low resolution), p's value first
 *     w    = hw * exp(-((e_n + e_a) + e_d))                                                     (exp: det_expf)
 *     num  = num + color(q) * w        den  = den + w        vnum  = vnum + variance(q) * (w * w)           (per channel)
 *     snum = snum + color(q) * hw      sden = sden + hw      svnum = svnum + variance(q) * (hw * hw)
 *   guided       = den > min_weight * sden                                                      (false for NaN)
 *   out_color    = guided ? num / den : snum / sden                                             (per channel)
 *   out_variance = guided ? vnum / (den * den) : svnum / (sden * sden)
 *   out_rgb      = the frame's tone map of out_color (the bits crt_render writes for that mean)
 * Every sum starts at +0.0f and runs left to right as written; every * + - / is one IEEE fp32 operation (no FMA, no reciprocal
 * multiply).  A pixel none of whose taps agrees with its guides (a feature thinner than a low-resolution pixel) falls back to the plain
 * tent interpolation instead of amplifying rounding noise; info->fallback_pixels counts the pixels with `guided` false.
 * A guide term is used only when both of its buffers are given (low->normal and guides->normal, ...); one of a pair without the other
 * is CRT_ERR_INVALID_ARG; a term without buffers is +0.0f.  guides == NULL: all three terms are off, whatever `low` holds, and the result
 * is the tent interpolation.  Non-finite inputs are not special-cased: the arithmetic defines the result.  With equal sizes, radius 1
 * and no guides the output has the input's bits.  For 1 <= low_width <= width every pixel has a tap inside the low image.
 * crt_upsample_defaults fills radius 1, min_weight 1/64 (the share at which crt_temporal gives up its taps), sigma_normal 0.5,
 * sigma_albedo 0.1, sigma_depth 0.05 (the denoiser's; sizes 0).  Nobody has tuned them for this operation on anything but the frames of
 * docs/experiments.md, "Guide-driven upsampling".
 * CRT_ERR_INVALID_ARG, checked before any device call: a null params, low or low->color; a size of 0; a low side longer than the
 * output's; a radius outside 1 .. 4; a min_weight that is negative, infinite or NaN; a sigma that is not > 0; low->variance and
 * out_variance not given together; neither out_color nor out_rgb.  A side longer than 2^24 pixels or more than 2^31 thread blocks of
 * 64 x 4 pixels: CRT_ERR_UNSUPPORTED. */
typedef struct {
    uint32_t width, height;          /* the output */
    uint32_t low_width, low_height;  /* the input: 1 <= low_width <= width, 1 <= low_height <= height */
    uint32_t radius;                 /* 1 .. 4: (2 radius)^2 low-resolution taps per output pixel; 1 = the bilinear footprint */
    float min_weight;                /* >= 0, finite: below this share of the spatial weight the guides are dropped for the pixel */
    float sigma_normal, sigma_albedo, sigma_depth;  /* as crt_denoise: > 0, not NaN, +inf switches the term off */
} crt_upsample_params;
typedef struct { const float* color; const float* variance; const float* albedo; const float* normal; const float* depth; } crt_upsample_low;  /* low_width x low_height */
typedef struct { const float* albedo; const float* normal; const float* depth; } crt_upsample_guides;                                         /* width x height */
typedef struct {
    float total_ms;            /* HIP-event time of the call's kernel on its stream */
    uint64_t fallback_pixels;  /* pixels with `guided` false */
} crt_upsample_info;
int crt_upsample_defaults(crt_upsample_params* params);
/* host buffers; allocates and frees its own device memory on `device`; info optional */
int crt_upsample(int device, const crt_upsample_params* params, const crt_upsample_low* host_low, const crt_upsample_guides* host_guides /* may be NULL */,
                 float* out_color, float* out_variance /* with low->variance */, uint8_t* out_rgb, crt_upsample_info* info);
/* Everything in device memory on `device`; enqueued on hip_stream (NULL = default stream) without synchronizing, unless info != NULL
 * (the call then counts the fallback pixels and synchronizes the stream to read them and the timer).  Outputs must not overlap inputs. */
int crt_upsample_device(int device, const crt_upsample_params* params, const crt_upsample_low* dev_low, const crt_upsample_guides* dev_guides,
                        void* d_out_color, void* d_out_variance, void* d_out_rgb, void* hip_stream, crt_upsample_info* info);

/* Multi-scale denoising: the two image operations of a Laplacian pyramid over crt_denoise_var, crt_denoise_nlm and crt_denoise_regress
 * (Rousselle et al. 2012; Delbracio et al. 2014; the last stage of NFOR).  A single-scale filter sees one window, so noise coarser than
 * the window stays; the pyramid filters the frame at every scale and replaces the low frequencies of a finer result with the coarser
 * scale's result.  crt_pyramid_down halves a frame and its guides, crt_pyramid_merge puts a finished coarser result into a filtered
 * finer one.  Image operations: no scene handle, no scratch; row-major images; color, variance, albedo and normal 3 floats per pixel,
 * depth 1.  The fine image is width x height, the coarse one low_width x low_height with
 *   low_width = (width + 1) / 2        low_height = (height + 1) / 2                            (crt_pyramid_size; a scale may be 1 x 1)
 * crt_pyramid_down, per coarse pixel (X, Y): the taps are the fine pixels (2X, 2Y), (2X + 1, 2Y), (2X, 2Y + 1), (2X + 1, 2Y + 1), in that
 * order; a tap outside the fine image is skipped; n = the number of taps taken, as a float (4, 2 or 1).  Every sum starts at +0.0f and
 * runs in that order:
 *   color, albedo, normal (per channel):   out = sum / n
 *   variance (per channel):                out = sum / (n * n)                 (the variance of the mean of n independent pixels)
 *   depth:  sum and the count nd run over the taps with depth > 0 only (false for NaN);  out = nd > 0 ? sum / nd : 0.0f
 *           (a miss does not pull a surface's depth towards the eye)
 * color is required; every other plane is optional, as an input / output pair.
 * crt_pyramid_merge, with `fine` the filtered fine scale and `coarse` the finished result of the coarser scale:
 *   d(Q)   = coarse(Q) - D(fine)(Q)       per channel and coarse pixel Q; D: exactly crt_pyramid_down's colour line
 *   out(p) = fine(p) + U(d)(p)            per channel and fine pixel p
 * U is crt_upsample's interpolation without guides at radius 1 from low_width x low_height: its sx, sy, u, v, x0, y0, wx, wy, hw lines, its
 * taps in its order (ty = y0, y0 + 1 outer, tx = x0, x0 + 1 inner, a tap outside the coarse image skipped),
 *   snum = snum + d(q) * hw      sden = sden + hw      U(d)(p) = snum / sden
 * out_rgb = the frame's tone map of out (the bits crt_render writes for that mean).  With coarse = D(fine) every d is +-0 and out has
 * fine's values.  There is NO variance output: the fine and the coarse result come from the same samples and are correlated, so the
 * variance of their combination is not the sum the filters' own estimates would give.
 * In both operations every * + - / is one IEEE fp32 operation (no FMA, no reciprocal multiply); non-finite inputs are not special-cased:
 * the arithmetic defines the result.  The library has two forms of the merge kernel (csrc/crt_pyramid.h: `staged` computes each d once
 * per workgroup into LDS, `direct` once per tap); the environment variable CRT_PYRAMID_FORM=direct|staged, read per call, selects one (for
 * tests; any other value is CRT_ERR_INVALID_ARG), and both give the same bits.
 * CRT_ERR_INVALID_ARG, checked before any device call: a null params (down: inputs, outputs, either colour buffer; merge: fine or coarse);
 * a size of 0; low sizes that are not ((width + 1) / 2, (height + 1) / 2); down: one of a plane's input / output pair without the other;
 * merge: neither out_color nor out_rgb; a negative device index.  A side longer than 2^24 pixels or more than 2^31 thread blocks
 * (down: 64 x 4 coarse pixels, merge: 32 x 8 pixels): CRT_ERR_UNSUPPORTED.
 * Not done: a guide-aware U, a variance of the merged result, per-scale filter settings. */
typedef struct {
    uint32_t width, height;          /* the fine image */
    uint32_t low_width, low_height;  /* the coarse image: ((width + 1) / 2, (height + 1) / 2) */
} crt_pyramid_params;
typedef struct { const float* color; const float* variance; const float* albedo; const float* normal; const float* depth; } crt_pyramid_planes;  /* width x height */
typedef struct { float* color; float* variance; float* albedo; float* normal; float* depth; } crt_pyramid_out_planes;                            /* low_width x low_height */
typedef struct {
    float total_ms;            /* HIP-event time of the call's kernel on its stream */
} crt_pyramid_info;
int crt_pyramid_size(uint32_t width, uint32_t height, uint32_t* low_width, uint32_t* low_height);
/* host buffers; allocates and frees its own device memory on `device`; info optional */
int crt_pyramid_down(int device, const crt_pyramid_params* params, const crt_pyramid_planes* host_in, const crt_pyramid_out_planes* host_out,
                     crt_pyramid_info* info);
int crt_pyramid_merge(int device, const crt_pyramid_params* params, const float* fine, const float* coarse, float* out_color, uint8_t* out_rgb,
                      crt_pyramid_info* info);
/* Everything in device memory on `device`; enqueued on hip_stream (NULL = default stream) without synchronizing, unless info != NULL
 * (the call then synchronizes the stream to read the timer).  Outputs must not overlap inputs. */
int crt_pyramid_down_device(int device, const crt_pyramid_params* params, const crt_pyramid_planes* dev_in, const crt_pyramid_out_planes* dev_out,
                            void* hip_stream, crt_pyramid_info* info);
int crt_pyramid_merge_device(int device, const crt_pyramid_params* params, const void* d_fine, const void* d_coarse, void* d_out_color, void* d_out_rgb,
                             void* hip_stream, crt_pyramid_info* info);

/* Error-estimated filter selection: per pixel, the one of K filtered candidates whose error, estimated against an independent half
 * frame, is smallest (Rousselle et al. 2012).  The caller renders with CRT_FLAG_HALF_BUFFERS, applies every candidate filter k to half
 * A and to half B (crt_half_buffers), and passes the halves, the variance of ONE half's mean (2 x crt_variance) and the 2 K filtered
 * images.  An image operation like the denoisers: no scene handle, row-major images, 3 floats per pixel.  With a = half_a, b = half_b,
 * v = half_variance, fa_k = filtered_a[k], fb_k = filtered_b[k], all in fp32, every * + - / one IEEE operation, no FMA:
 *  1 per pixel and candidate, per channel:
 *      da = fa_k - b;  db = fb_k - a;  t = (da * da - v) + (db * db - v)
 *    then  e_k = ((t_x + t_y) + t_z) / 6.0f;  an e_k that is not finite (NaN, +-inf) becomes +inf.
 *    (fa_k - b is the half filter's error plus b's noise, which is independent of fa_k: the square overstates the squared error by v.)
 *  2 smoothing, separable, in-image taps only, r = error_radius:
 *      H_k(x, y) = sum over dx = -r .. r ascending of e_k(x + dx, y), from +0.0f
 *      E_k(x, y) = (sum over dy = -r .. r ascending of H_k(x, y + dy), from +0.0f) / (float)(nx * ny)
 *    nx, ny: the taps inside the image along each axis.
 *  3 choice:  best = 0;  for k = 1 .. K - 1:  if (E_k < E_best) best = k.  Ties, NaN and all +inf stay with the lower index.
 *    out_choice = best;  out_error = E_best.
 *  4 blend, s = blend_radius: over the in-image pixels of the (2 s + 1)^2 window, m_k = the number that chose k, m = their total;
 *      o = +0.0f;  for ascending k with m_k > 0:  o = o + ((float)m_k / (float)m) * ((fa_k + fb_k) * 0.5f)      (per channel)
 *    a candidate nobody in the window chose contributes nothing (not 0 x its value).  out_mean = o; out_rgb = the frame's tone map of o.
 * info->chosen[k]: the pixels with out_choice = k.  crt_filter_select_defaults fills error_radius 3, blend_radius 1, n_candidates 2
 * (sizes 0); the radii are untuned beyond docs/experiments.md, "Half buffers and filter selection".
 * Scratch (the _device form): crt_filter_select_scratch_bytes(width, height) bytes, 16-byte aligned: the choice map between the two
 * kernels.
 * CRT_ERR_INVALID_ARG, checked before any device call: a null params or inputs; a size of 0; n_candidates outside 1 .. 4; error_radius
 * above 8; blend_radius above 4; a null half_a, half_b, half_variance or filtered image below n_candidates; neither out_mean nor
 * out_rgb; a null, small or misaligned scratch buffer.  A side longer than 2^24 pixels or more than 2^31 thread blocks of 32 x 8
 * pixels: CRT_ERR_UNSUPPORTED. */
#define CRT_SELECT_MAX_CANDIDATES 4
typedef struct {
    uint32_t width, height;
    uint32_t n_candidates;   /* K: 1 .. 4 */
    uint32_t error_radius;   /* r: 0 .. 8 */
    uint32_t blend_radius;   /* s: 0 .. 4 */
} crt_filter_select_params;
typedef struct {
    const float* half_a; const float* half_b;     /* crt_half_buffers */
    const float* half_variance;                   /* the variance of one half's mean: 2 x crt_variance */
    const float* filtered_a[CRT_SELECT_MAX_CANDIDATES]; /* filter k applied to half_a ... */
    const float* filtered_b[CRT_SELECT_MAX_CANDIDATES]; /* ... and to half_b; entries k >= n_candidates are not read */
} crt_filter_select_inputs;
typedef struct {
    float total_ms;                               /* HIP-event time of the call's two kernels on its stream */
    uint64_t chosen[CRT_SELECT_MAX_CANDIDATES];   /* pixels per candidate */
} crt_filter_select_info;
int crt_filter_select_defaults(crt_filter_select_params* params);
int crt_filter_select_scratch_bytes(uint32_t width, uint32_t height, uint64_t* bytes);
/* host buffers; allocates and frees its own device memory on `device`; out_choice (W x H bytes), out_error (W x H floats) and info are
 * optional, one of out_mean and out_rgb is required */
int crt_filter_select(int device, const crt_filter_select_params* params, const crt_filter_select_inputs* host_in, float* out_mean, uint8_t* out_rgb,
                      uint8_t* out_choice, float* out_error, crt_filter_select_info* info);
/* Everything in device memory on `device`; enqueued on hip_stream (NULL = default stream) without synchronizing, unless info != NULL
 * (the call then counts the choices and synchronizes the stream to read them and the timer).  Outputs must not overlap inputs. */
int crt_filter_select_device(int device, const crt_filter_select_params* params, const crt_filter_select_inputs* dev_in, void* d_out_mean,
                             void* d_out_rgb, void* d_out_choice, void* d_out_error, void* d_scratch, uint64_t scratch_bytes, void* hip_stream,
                             crt_filter_select_info* info);

/* ------------------------------------------------------------------------
 * Multi-device rendering in ONE process.  The reference picks device 0 and stops there
 * (config_CUDA, src/main.cu:92-105); a crt_multi holds one device replica of the scene per entry of
 * `devices` (= rank), renders the interleaved 8x8-tile shards concurrently (one host thread and one HIP
 * stream per device), exchanges the compact tile buffers with ONE ncclAllGather over RCCL / xGMI and
 * de-interleaves them into the row-major frame on rank 0 -- the frame is identical to crt_render's on
 * one device, whatever the number of ranks.
 * ---------------------------------------------------------------------- */
typedef struct crt_multi crt_multi;
enum {
    CRT_GATHER_AUTO = 0,  /* RCCL when there are two or more DISTINCT devices, peer copies otherwise */
    CRT_GATHER_RCCL = 1,  /* ncclCommInitAll + one ncclAllGather per frame (librccl.so.1 is bound at run time; its absence is CRT_ERR_UNSUPPORTED) */
    CRT_GATHER_COPY = 2   /* every rank copies its block into rank 0's buffer (hipMemcpyPeerAsync); also the only mode that accepts
                             several ranks on ONE device (test configuration: RCCL refuses duplicate devices) */
};
typedef struct {
    uint32_t n_ranks;        /* device replicas that rendered */
    uint32_t gather;         /* CRT_GATHER_* that ran */
    uint32_t rccl_ranks;     /* ncclCommCount of the communicator the gather ran on; 0 with CRT_GATHER_COPY */
    int32_t rccl_version;    /* ncclGetVersion; 0 if RCCL was not used */
    float render_ms;         /* host clock: until the slowest rank's shard is complete */
    float gather_ms;         /* host clock: exchange + de-interleave + copy to the host */
    float frame_ms;          /* host clock: the whole call */
    float max_kernel_ms;     /* largest crt_stats.kernel_ms over the ranks */
    uint64_t bytes_per_rank; /* size of one rank's block in the exchange */
    uint64_t rays, paths, rays_untraced; /* sums over the ranks */
    char fallback_reason[160]; /* (ABI 5) CRT_GATHER_AUTO only: why the gather runs on peer copies although the devices are distinct -- librccl.so.1 not
                                  found, ncclCommInitAll refused ...; empty when no fallback happened.  An explicit CRT_GATHER_RCCL fails instead. */
} crt_multi_info;
/* gather: CRT_GATHER_*.  Uploads the scene to every device (crt_scene_create per rank). */
int crt_multi_create(const crt_scene_desc* desc, const int* devices, uint32_t n_devices, uint32_t gather, crt_multi** out);
int crt_multi_destroy(crt_multi* multi);
/* = Render::run_view over all ranks.  params->rank / world are ignored (rank r renders tiles t % n == r).  out_rgb: W*H*3 bytes,
 * row-major, row 0 = image top, may be NULL (the frame then stays on rank 0's device, crt_multi_frame_device); out_mean optional
 * (needs out_rgb); stats: NULL or n_devices entries, one per rank; info optional. */
int crt_multi_render(crt_multi* multi, const crt_camera* cam, const crt_params* params, uint8_t* out_rgb, float* out_mean,
                     crt_stats* stats, crt_multi_info* info);
/* device pointers of the last frame on rank 0's device (d_mean: NULL unless the last call asked for the mean; d_rgb: NULL after a
 * crt_multi_render_buffers that did not ask for RGB) */
int crt_multi_frame_device(crt_multi* multi, void** d_rgb, void** d_mean, int* device);

/* The buffers of a multi-device frame: what the image operations of this header (crt_denoise*, crt_demodulate / crt_modulate,
 * crt_filter_select, crt_pyramid_*, crt_temporal*, crt_upsample) take, gathered row-major on rank 0's device.  One bit per plane; the
 * bits' order is the order of the planes in a rank's block and of crt_multi_buffers' members. */
enum {
    CRT_MULTI_RGB = 1u,              /* 3 x u8   crt_render's out_rgb */
    CRT_MULTI_MEAN = 2u,             /* 3 x f32  crt_render's out_mean */
    CRT_MULTI_VARIANCE = 4u,         /* 3 x f32  crt_variance */
    CRT_MULTI_HALF_A = 8u,           /* 3 x f32  crt_half_buffers' out_a */
    CRT_MULTI_HALF_B = 16u,          /* 3 x f32  crt_half_buffers' out_b */
    CRT_MULTI_ALBEDO = 32u,          /* 3 x f32  crt_render_aov */
    CRT_MULTI_NORMAL = 64u,          /* 3 x f32 */
    CRT_MULTI_DEPTH = 128u,          /* f32 */
    CRT_MULTI_COVERAGE = 256u,       /* f32 */
    CRT_MULTI_TRI = 512u,            /* i32 */
    CRT_MULTI_MATERIAL = 1024u,      /* i32 */
    CRT_MULTI_EMISSION = 2048u,      /* 3 x f32  crt_render_aov_shading */
    CRT_MULTI_DIFFUSE_ALBEDO = 4096u,/* 3 x f32 */
    CRT_MULTI_ALL = 8191u
};
typedef struct {
    uint8_t* rgb;
    float* mean; float* variance; float* half_a; float* half_b;
    float* albedo; float* normal; float* depth; float* coverage;
    int32_t* tri; int32_t* material;
    float* emission; float* diffuse_albedo;
} crt_multi_buffers;
/* Renders the frame over all ranks as crt_multi_render does and gathers every plane of `want` (CRT_MULTI_* bits): afterwards each is
 * row-major (W x H pixels, row 0 = image top) on rank 0's device, and is copied to the matching pointer of host_out where that is not
 * NULL (host_out itself may be NULL; pointers of planes that are not wanted are ignored).  Every plane has the bits of the
 * single-device call named beside its bit above, on the same scene, camera and params, whatever the number of ranks.
 * Per rank, on the rank's own thread and stream, in this order: crt_render_device with CRT_FLAG_TILED_OUTPUT -- CRT_FLAG_VARIANCE set
 * exactly when VARIANCE is wanted, CRT_FLAG_HALF_BUFFERS exactly when a half is, both cleared otherwise whatever params->flags says --;
 * crt_variance_device / crt_half_buffers_device into the rank's block; then at most ONE trace of the frame's camera rays:
 * crt_render_aov_shading_device when EMISSION or DIFFUSE_ALBEDO is wanted (its `first` names the wanted first-hit planes, NULL when
 * there is none), crt_render_aov_device when only first-hit planes are, nothing when no AOV plane is.
 * A rank's block is its wanted planes one after the other in the bits' order, each from a 16-byte boundary, of `slots` pixels each
 * (crt_shard_slots; padding slots as the calls above define them), with 64-bit byte offsets.  The blocks travel in ONE ncclAllGather
 * (or the peer copies of CRT_GATHER_COPY), crt_multi_info.bytes_per_rank is a block's size, and ONE kernel launch on rank 0
 * de-interleaves all planes (csrc/crt_untile.h).  An all-gather delivers every plane to every rank although only rank 0 uses them.
 * render_ms ends when every rank's passes are complete; gather_ms is the exchange, the de-interleave and the copies to the host.
 * CRT_ERR_INVALID_ARG, checked before any device call: a null handle, camera or params; want == 0 or a bit outside CRT_MULTI_ALL;
 * VARIANCE, HALF_A or HALF_B with params->spp < 2; a width or height of 0.  A refused or failed call leaves the handle usable.
 * crt_multi_render IS this call with RGB (and MEAN when out_mean is given): one implementation, the same results, info and
 * bytes_per_rank as before.  stats, info: as crt_multi_render's. */
int crt_multi_render_buffers(crt_multi* multi, const crt_camera* cam, const crt_params* params, uint32_t want,
                             const crt_multi_buffers* host_out /* may be NULL */, crt_stats* stats, crt_multi_info* info);
/* The device pointers, on rank 0's device (*device, optional), of the planes the last render on the handle made -- crt_multi_render
 * makes RGB and, asked for, MEAN --; a plane that call did not make is NULL, as is every plane after a call that failed on a device (a refused call leaves them as they were).  Valid until the
 * next render on the handle.  For the *_device forms of the image operations: no host round trip. */
int crt_multi_buffers_device(crt_multi* multi, crt_multi_buffers* dev, int* device);
/* Measurement hook (tools/gather_probe.py): launches the de-interleave of the last frame on the handle again, `calls` times, each
 * between two HIP events on rank 0's stream; ms[c] receives the time of launch c.  The gathered blocks are still in place, so the
 * planes are rewritten with their own values.  CRT_ERR_INVALID_ARG: a null argument, calls == 0, no frame on the handle. */
int crt_multi_untile_time(crt_multi* multi, uint32_t calls, float* ms);

/* Closest-hit query for n rays (device-side DeviceBVH::intersect,
 * DeviceBVH.cuh:128-170), host buffers. dirs are normalised as Ray's
 * constructor does (Ray.cuh:12-15). out_tri: BVH-order triangle index or -1. */
#define CRT_INTERSECT_RAW_DIRECTIONS 0x100u /* OR into `traversal`: take dirs as they are (already a Ray's direction), do not normalise again */
#define CRT_INTERSECT_FORCE_EXACT 0x200u     /* OR into `traversal`: as CRT_FLAG_FORCE_EXACT for the queries (test hook) */
/* OR into `traversal`: the rays are visibility rays -- blocked() of Render.cuh:19-27.  out_t[i] holds t_to_light on entry; on return
 * out_t[i] = 1.0f if the ray is blocked (t_to_light - closest.t > EPSILON) else 0.0f and out_tri[i] = a blocking triangle or -1
 * (REFERENCE: the closest hit; FAST: the first one the any-hit traversal met). */
#define CRT_INTERSECT_VISIBILITY 0x400u
int crt_intersect(crt_scene* scene, uint32_t n, const float* origins, const float* dirs, uint32_t traversal,
                  int32_t* out_tri, float* out_t);

/* Device-side evaluation of the deterministic math / RNG helpers, for parity
 * tests against the oracle.  fn in {"sin","cos","tan","acos","atan2","exp","log10","pow","uniform"}. */
int crt_device_math(int device, const char* fn, uint32_t n, const float* a, const float* b, float* out);
int crt_device_philox(int device, uint32_t n, const uint32_t* ctr4, const uint32_t* key2, uint32_t* out4);
/* One named device function per element, as the render kernels call it, for value-level parity tests.  A record is a fixed number of
 * 32-bit words, floats and integers alike, passed as bits: element i reads in[i * in_words ..] and writes out[i * out_words ..].
 * Element i is computed by thread i of a launch with 256-thread blocks, so it is lane i % 64 of wave i / 64: the elements
 * [64 w, 64 w + 64) meet the wave-uniform branches (the guard of unit3 / div3) together.  Draws go in as raw words and become uniforms
 * through the kernels' own mapping.  name (input words -> output words):
 *   sin cos tan asin acos atan exp log log10 uniform (1 -> 1), sincos (1 -> 2: sin, cos), atan2 (y, x) pow (x, y) (2 -> 1);
 *   dot3 (a, b: 6 -> 1), cross3 (a, b: 6 -> 3), norm3 (3 -> 1), unit3 (3 -> 3), div3 (a, s: 4 -> 3), make_ray (d: 3 -> 6 = unit3(d), 1 / each);
 *   to_world (a, N: 6 -> 3), sample_hemisphere (N, word1, word2: 5 -> 3), sample_lobe (out, delta_theta, delta_phi, word1, word2: 7 -> 3),
 *   bounce_dir (N, rb.y, rb.z: 5 -> 3);
 *   cos_to_next (from, to, n: 9 -> 1), roulette (seed lo, seed hi, pixel, k, depth, p_rr: 6 -> 5 = stop, rb.xyzw),
 *   probe_dir (seed lo, seed hi, pixel, k, depth, ns, arrived, n: 12 -> 3), probe_term (n, kd, ke, o, d, t, ns: 17 -> 3),
 *   indirect_step (L, f_r, cos, p_rr, L_dir: 11 -> 3), seed_direct (L_dir: 3 -> 3), seed_emitter (deepest, ke: 4 -> 3);
 *   tonemap (1 -> 1: the byte of one channel).
 * An unknown name, a null pointer, word counts other than the function's or a negative device are CRT_ERR_INVALID_ARG, reported before
 * any device call; n == 0 is CRT_OK. */
int crt_device_fn(int device, const char* name, uint32_t n, const uint32_t* in, uint32_t in_words, uint32_t* out, uint32_t out_words);
/* Exhaustive self-check of the short reciprocal the kernels use in place of the division 1.0f / x (Ray.cuh:14,
 * DeviceTriangle.cuh:47): evaluates both for all 2^32 bit patterns of x on the device and returns, in *mismatches, the
 * number of inputs INSIDE the guarded range (2^-126 <= |x| < 2^126) whose bits differ (must be 0), and in *outside the
 * number of inputs outside the range that differ (those take the division itself).  A few milliseconds. */
int crt_device_rcp_check(int device, uint64_t* mismatches, uint64_t* outside);
/* Test-only export of the traversal trees a scene handle holds, copied from DEVICE memory (what the kernels read; layouts:
 * csrc/crt_device.h, csrc/crt_scene_layout.h).  `name` is one of the arrays "nodes", "nodes3", "nodes4", "nodes4i", "leaf_geo",
 * "leaf_geo_i", "rec_map", "tri_geo", "leaf_count", "tri_nm", "ltri", or "scalars" (one crt_tree_scalars).  *bytes receives the array's
 * size (0 for an array the scene does not have: "nodes" / "nodes3" when the tree is one leaf, the nodes4i set when layout_caps
 * bit 3 is clear); dst == NULL asks for the size only.  An unknown name, a null `bytes`, a null scene or a capacity below the size
 * is CRT_ERR_INVALID_ARG (the name and `bytes` are checked first, so a null scene reports those). */
typedef struct {
    int32_t root_fast, root_exact, root3_fast, root3_exact, root4, root4i;
    uint32_t n_mixed4i, empty4_off, empty4i_off; /* empty*_off: byte offsets of the node of four empty slots */
    float coord_max;
    uint32_t stack_cap;                          /* traversal stack entries per ray the scene was sized for */
    uint32_t node4i_f4;                          /* float4 per node of nodes4i (NODE4I_F4) */
} crt_tree_scalars;
int crt_scene_export(crt_scene* scene, const char* name, void* dst, size_t capacity, size_t* bytes);
/* "ltri": the light triangles' rows (four float4 each: v1, v2, v3, normal, ke, area_of_obj), 0 bytes for a scene without lights. */

/* Refit: new coordinates for the triangles of a scene handle, without rebuilding it.  `tris` are in the handle's BVH order and
 * `light_tris` in its shape order -- the arrays and the layout of crt_scene_desc -- and the counts must equal the handle's.  Materials,
 * lights, the leaves' triangle ranges [it, it + n) and every topology the handle holds stay: the reference tree and the SAH tree in
 * `nodes` / `nodes3`, the collapsed tree in `nodes4`, its copy without refs `nodes4i`, the leaf records and `rec_map`.  Only
 * coordinates are rewritten, and afterwards the handle renders, bit for bit, what a fresh handle renders from the description with the
 * same topology and the refitted boxes (a frame depends on the triangles, the leaves' own boxes and on inner boxes being supersets:
 * DESIGN.md 4).  Operation by operation (names: crt_scene_export; csrc/crt_scene_layout.h builds the same rows at crt_scene_create):
 *   1. Rows.  e1 = v2 - v1, e2 = v3 - v1 in fp32.  tri_geo row 3 i .. 3 i + 2 = (v1.xyz, e1.x) (e1.yz, e2.xy) (e2.z, normal.xyz);
 *      tri_nm[i] = (normal.xyz, the word it had: material and flags stay); both lanes of the dense leaf_geo records (the second lane
 *      of an odd tail repeats the first) and their copies in leaf_geo_i at rec_map[record]; ltri row 4 j .. 4 j + 3 =
 *      (v1.xyz, v2.x) (v2.yz, v3.xy) (v3.z, normal.xyz) (ke as it was, area_of_obj).  `area` is not stored anywhere.
 *   2. Leaf boxes.  Per axis lo = the minimum and hi = the maximum of the nine vertex coordinates of each of the leaf's triangles, in
 *      the order x < y, or x == y with x = -0 and y = +0: the bits do not depend on the order of evaluation.
 *   3. Inner boxes.  Each is the union of its children's boxes under the same order, in every tree; every stored plane of nodes (both
 *      ranges), nodes3, nodes4 and nodes4i is the plane of the child's box.  Empty slots and the empty nodes stay.
 *   4. In nodes4i the six planes of child 0 of a mixed node (an inner child) keep their low 12 mantissa bits: each is the nearest value
 *      outwards of the refitted plane that has the bits the plane had.  Leaf planes are exact.
 *   5. Scalars.  crt_tree_scalars.coord_max = the largest |plane| of the used children of nodes4 and nodes4i (0 when the scene is one
 *      leaf); the root box crt_aov_ao_defaults reads = the box of the reference tree's root.  Every other field of crt_tree_scalars,
 *      crt_accel_info (layout_caps, depths) and the stack capacity are unchanged.
 * Refusals, each CRT_ERR_INVALID_ARG, and each leaves the handle byte for byte as it was: a NULL scene or triangle array (light_tris
 * may be NULL only when the handle has none), counts other than the handle's, any vertex coordinate that is not finite or has
 * |x| > 2^126 (so step 4 cannot leave the finite floats and layout_caps cannot change; the check of ALL coordinates completes on the
 * device before the first array is written), and -- host form only -- a triangle whose `material` differs from the handle's.  The
 * device form does not read `material` or `area`.  `normal` and `area_of_obj` are taken as given: they are stored as they come and are
 * not checked, in either form.
 * A refit ends the frame in flight: the sums of crt_render_range, CRT_FLAG_VARIANCE, CRT_FLAG_HALF_BUFFERS and CRT_FLAG_PIXEL_FILTER
 * are as after a new frame's start (a range with sample_begin > 0, crt_variance, ... are refused until a frame starts at sample 0).
 * The order of the work items (crt_item_order) stays: the scene is not in it.
 * crt_scene_refit_device reads two device arrays of crt_triangle on `hip_stream`, enqueues everything there and synchronizes that
 * stream ONCE, to read one 32-byte result (the count of refused coordinates, coord_max, the root box) through pinned memory;
 * crt_scene_refit uploads the two arrays and calls it on the null stream.  The tables the kernels walk (one entry per leaf and per
 * inner node of every tree) are made at the handle's FIRST refit from the arrays the handle holds -- crt_scene_create does nothing
 * for a refit -- and the time is reported in prepare_ms (0 on later calls).
 * The inner boxes have two forms with the same bytes: CRT_REFIT_FORM=levels (one launch per node height) | walk (one launch: the
 * last thread to arrive at a node computes it); read per call -- the calls of one handle may take either form in any order --
 * another value is CRT_ERR_INVALID_ARG; unset: the faster one
 * (docs/experiments.md, "Refitting a scene"). */
typedef struct {
    uint32_t n_tris, n_light_tris;
    uint32_t leaves;           /* leaf boxes computed */
    uint32_t boxes_written;    /* child boxes stored in nodes, nodes3, nodes4 and nodes4i together */
    uint32_t launches;         /* kernel launches of the call */
    uint32_t form;             /* 0: levels, 1: walk */
    float root_aa[3], root_bb[3], coord_max;   /* the scalars of step 5 as the handle now holds them */
    float prepare_ms;          /* host clock: the tables (the first refit of a handle; 0 afterwards) */
    float device_ms;           /* HIP events around the call's launches */
} crt_refit_info;
int crt_scene_refit(crt_scene* scene, const crt_triangle* tris, uint32_t n_tris, const crt_triangle* light_tris, uint32_t n_light_tris,
                    crt_refit_info* info /* may be NULL */);
int crt_scene_refit_device(crt_scene* scene, const void* d_tris, uint32_t n_tris, const void* d_light_tris, uint32_t n_light_tris,
                           void* hip_stream, crt_refit_info* info /* may be NULL */);

/* ------------------------------------------------------------------------
 * Host layer: scene ingestion and BVH build on the CPU (north star: "C++ host
 * code builds the BVH and triangle/material/light arrays as today").
 * Mirrors Scene / Loader / Object / BVH / Camera of the reference.
 * ---------------------------------------------------------------------- */
typedef struct crt_host_scene crt_host_scene;

/* Scene(width, height)  (Scene.h:28-31) */
int crt_host_scene_create(uint32_t width, uint32_t height, crt_host_scene** out);
int crt_host_scene_destroy(crt_host_scene* scene); /* Scene::free */
/* Loader::read_OBJ + load_object for every shape + Scene::add_normal_obj/add_light_obj
 * in shape order (src/main.cu:122-145) */
int crt_host_scene_add_obj(crt_host_scene* scene, const char* obj_path, const char* mtl_dir);
/* Scene::set_BVH(thresh_n) (Scene.h:50-54 -> BVH.h:30-84) */
int crt_host_scene_set_bvh(crt_host_scene* scene, uint32_t thresh_n);
/* The same BVH built on the GPU (csrc/crt_bvh_build.hip): level-synchronous median split; per level the
 * device replays the quicksort phase of libstdc++'s std::sort on every range (equal centroid coordinates are the norm on real
 * meshes, and an unstable sort's order of equal keys is its own) and finishes with one stable radix sort of the whole triangle
 * order.  Node and triangle arrays are BYTE-IDENTICAL to crt_host_scene_set_bvh's.  A range whose quicksort phase hits std::sort's
 * depth limit is sorted by the host between two levels (info->host_sorts); scenes with -0.0 or non-finite coordinates are built on
 * the host entirely (info->host_triangles = all). */
typedef struct {
    uint32_t n_triangles, n_nodes, levels;
    uint32_t host_ranges;      /* subtrees finished by the host builder (none unless a range's extents are NaN) */
    uint32_t host_triangles;   /* triangles in them */
    uint32_t host_sorts;       /* single range sorts done by the host's std::sort between two levels: ranges whose quicksort phase ran into
                                  std::sort's depth limit (heapsort), e.g. already-sorted keys full of ties */
    uint64_t host_sort_elements;
    float device_ms;           /* HIP events around the level loop */
    float total_ms;            /* host clock: uploads, level loop, downloads, host subtrees */
    float host_build_ms;       /* host clock: the host builder's part (host ranges, or everything on a fallback) */
} crt_bvh_build_info;
int crt_host_scene_set_bvh_device(crt_host_scene* scene, uint32_t thresh_n, int device, crt_bvh_build_info* info);
/* Flat view of the built scene; pointers stay valid until the host scene is
 * destroyed or modified. */
int crt_host_scene_desc(const crt_host_scene* scene, crt_scene_desc* out);
int crt_host_scene_num_objects(const crt_host_scene* scene, uint32_t* n);
/* Object area as printed by the reference (Object.h:25) and whether it is a light */
int crt_host_scene_object(const crt_host_scene* scene, uint32_t index, float* area, int32_t* is_light,
                          uint32_t* n_tris);

/* Moves one object of a scene whose BVH is built: the 3 x 4 affine map m (row-major: x' = m[0] x + m[1] y + m[2] z + m[3], ...; fp32,
 * terms in that order, a term whose coefficient is 0 left out, so the identity keeps every bit) on the vertices of object `index`
 * (crt_host_scene_object's order), in its triangles and, for a light, in its light triangles.  normal, area and area_of_obj are
 * recomputed with the loader's formulas (Triangle.h:27,39; Object.h:15-23).  The BVH keeps its topology and its triangle order; its
 * boxes are refitted by crt_scene_refit's rule (leaf: minimum and maximum of its triangles' vertices, inner: the union of its
 * children, -0 < +0), so crt_host_scene_desc then returns the moved description, whose triangle arrays crt_scene_refit takes.
 * crt_host_scene_set_bvh afterwards builds a new tree as before.  A bad index, a matrix entry that is not finite or a scene
 * without a BVH is CRT_ERR_INVALID_ARG. */
int crt_host_scene_transform_object(crt_host_scene* scene, uint32_t index, const float m[12]);

/* get_inverse_view_matrix (Camera.h:9-36); out = 9 floats column-major */
int crt_inverse_view(const float eye[3], const float lookat[3], const float up[3], float out[9]);

/* Task / config.json (src/main.cu:40-90) */
typedef struct {
    uint32_t n_objs;           /* entries of OBJ_paths in the file -- any number, as src/main.cu:74-78 loops over them.  The two arrays of this struct
                                  hold the first 8 only: a client that walks obj_path[i] / mtl_dir[i] must stop at min(n_objs, 8) and take the rest
                                  from crt_task_obj */
    char obj_path[8][512];     /* the first eight; crt_task_obj() returns any of them */
    char mtl_dir[8][512];
    float lookat[3], up[3], eye_pos[3];
    float fov_y;        /* degrees, as in the file */
    uint32_t width, height, bvh_thresh_n, light_sample_n, spp;
    float p_rr;
} crt_task;
int crt_task_load(const char* config_json_path, crt_task* out);
/* Entry `index` (< n_objs) of the file's OBJ_paths: the two strings, NUL-terminated, into buffers of `cap` bytes each
 * (CRT_ERR_INVALID_ARG if one does not fit or the index is out of range).  For configurations of more than eight OBJ files. */
int crt_task_obj(const char* config_json_path, uint32_t index, char* obj_path, char* mtl_dir, uint32_t cap);

/* What the reference's texture decoder returns for a map_Kd file -- stbi_load(path, &x, &y, &comp, 0) of Loader.h:58: 8-bit
 * samples, row 0 = top, the file's own channel count.  Decodes every format that decoder reads -- PNG (plain and Adam7), JPEG
 * (baseline and progressive), BMP, TGA, GIF (first frame), PSD, Softimage PIC, binary PNM and Radiance HDR (csrc/crt_image.h,
 * crt_png.h, crt_jpeg.h, crt_formats.h) -- with that decoder's own conventions, pinned sample for sample against the reference's
 * vendored stb_image by tests/golden/stb_decode.json.  A file that is none of these, or damaged beyond what the reference's
 * decoder accepts, returns CRT_ERR_UNSUPPORTED.  out may be NULL (size query); cap = bytes available at out (x * y * comp needed). */
int crt_image_load(const char* path, int32_t* x, int32_t* y, int32_t* comp, uint8_t* out, uint64_t cap);

/* stb-free PNG writer used by Render::save_frame_buffer's replacement (Render.cuh:489-493) */
int crt_write_png(const char* path, uint32_t width, uint32_t height, const uint8_t* rgb);
/* Portable Float Map of width x height pixels of `channels` (1: "Pf", 3: "PF") floats, row 0 of `data` = image top: header
 * "P?\n<width> <height>\n-1.0\n" (scale -1.0 = little-endian), then the rows bottom to top, as the format stores them.  The AOV
 * buffers' depth / coverage (1 channel) or albedo / normal (3 channels). */
int crt_write_pfm(const char* path, uint32_t width, uint32_t height, uint32_t channels, const float* data);

/* Sample maps: one frame in which pixel p receives samples sample_begin .. n_p - 1 of its S = params->spp samples, n_p GIVEN per pixel
 * by the caller (an importance or foveation map, a mask of a region to refine, a plan made from an earlier frame's variance) -- where
 * crt_render_adaptive finds n_p itself, one launch of the render kernel per step.  Here all the samples a pixel still needs go into ONE
 * launch per chunk (below).  Sample k of pixel p is the path it is in crt_render's frame (same seed, same draws), S is the cap AND the
 * divisor of every sample, exactly as in crt_render_adaptive.  Operation by operation:
 *   count      sample_map holds one uint32 per pixel of the WHOLE width x height image, row-major, also for a rank / world shard (which
 *              reads the entries of its own pixels).  n_p = min(max(map[p], max(sample_begin, 1)), S): a pixel cannot take fewer samples than
 *              it has, nor none at all, nor more than the cap; a map value of 0 or above S is legal and is clamped.
 *   sums       c = c + x_k, q = q + x_k * x_k with x_k = L_k / (float)S for k = sample_begin .. n_p - 1 in sample order (the sums of
 *              crt_variance; from +0.0f if sample_begin = 0), every * + / one IEEE fp32 operation, no FMA.
 *   outputs    exactly crt_render_adaptive's, made by the same kernel, in the layout of crt_render's buffers (row-major, or the shard's
 *              compact tiles with CRT_FLAG_TILED_OUTPUT; padding slots 0 / +0.0f): out_samples = n_p; out_mean = c * ((float)S / (float)n_p)
 *              per channel; out_rgb = the frame's tone map of out_mean; out_variance = crt_variance's formula with fn = (float)n_p.  For
 *              n_p = 1 the variance is what IEEE arithmetic gives that formula: (rr * d) / (1.0f - 1.0f), i.e. NaN for d = 0 and +inf
 *              otherwise -- one sample has no variance, and the call does not hide it.  out_samples and out_variance may be NULL; out_rgb
 *              and out_mean not both.
 * sample_begin = 0 starts a frame.  sample_begin > 0 continues the frame in flight on the handle, which must hold exactly samples
 * [0, sample_begin) of every pixel with valid variance sums -- the state after crt_render_range(0, sample_begin) with CRT_FLAG_VARIANCE
 * (in one range or several) -- and have the same spp, width, height, rank, world and CRT_FLAG_TILED_OUTPUT.  Anything else is
 * CRT_ERR_INVALID_ARG before any device call, and the handle stays as it was: the frame in flight can still be previewed and continued.
 * Flags: CRT_FLAG_VARIANCE is implied; CRT_FLAG_STATS and CRT_FLAG_BOUNDED_RADIANCE are ignored.  Afterwards NO frame is in flight on
 * the handle, as after crt_render_adaptive: crt_preview, crt_variance, crt_sample_plan and a range or map with sample_begin > 0 are
 * refused, and a later crt_render is unaffected.
 * How it runs: a prepare kernel computes n_p per pixel slot and a histogram of n_p over 0 .. S; the host reads the S + 1 words of the
 * histogram once, through pinned memory -- ONE synchronization of the stream per call, in both forms, however many chunks follow -- and
 * from count_s = pixels with n_p > s sizes every chunk of samples [s0, s0 + ns): its number of work items and where each sample's
 * entries start in its item list.  Per chunk a list kernel writes the list (sample-major, the pixel slots of a wave side by side), the
 * render kernel runs once over it, and a fold kernel adds min(n_p, s0 + ns) - s0 samples to each pixel's sums.  Chunks beyond the largest
 * n_p are not launched (max n_p = sample_begin: no launch at all).
 * Limits: the per-path radiance buffer stays dense per chunk, (samples of the chunk) x (pixel slots) x 12 B, whatever the map holds,
 * and a chunk holds as many whole samples as 2^30 paths allow, as crt_render's; the list costs 4 B per work item of a chunk beside it;
 * a chunk's number of work items and every item number stay below 2^32 (the chunk is capped at 2^30 paths).  spp above 2^24 (the
 * histogram and the cursors cost 8 B per sample of the cap) or more than 2^30 pixel slots in a shard: CRT_ERR_UNSUPPORTED.
 * CRT_ERR_INVALID_ARG, before any device call: a null scene, camera, params or map; both image outputs NULL; sample_begin >= spp;
 * anything crt_render refuses; a sample_begin > 0 that does not continue the frame in flight.  CRT_ERR_UNSUPPORTED: the fallback
 * pipeline (CRT_PIPELINE=2, or a scene beyond the render kernel's limits).  crt_multi has no map form. */
typedef struct {
    uint64_t paths;         /* paths this call traced: sum over the shard's pixels of n_p - sample_begin (crt_render_planned: of n_p, the warm-up included) */
    uint64_t paths_uniform; /* pixels x spp: what crt_render would have traced */
    uint32_t launches;      /* launches of the render kernel (crt_render_planned: the warm-up's included) */
    uint32_t max_samples;   /* the largest n_p of the shard */
    float kernel_ms, total_ms; /* the render kernel's launches (first launch's start to last launch's end; crt_render_planned: plus the
                                  warm-up's) / the whole device pipeline of the call, HIP events on its stream */
} crt_map_info;
/* host buffers: sample_map width x height uint32; the outputs as crt_render_adaptive's; info optional */
int crt_render_map(crt_scene* scene, const crt_camera* cam, const crt_params* params, const uint32_t* sample_map, uint32_t sample_begin,
                   uint8_t* out_rgb, float* out_mean, uint32_t* out_samples, float* out_variance, crt_map_info* info);
/* Device buffers on the scene's device (d_sample_map: width x height uint32, written before the call in stream order), work enqueued on
 * hip_stream (NULL = default stream).  SYNCHRONIZES hip_stream once, after the prepare kernel, to read the histogram; the launches and
 * the outputs are enqueued after it without a further synchronization, unless info != NULL (once more, to read the timers). */
int crt_render_map_device(crt_scene* scene, const crt_camera* cam, const crt_params* params, const void* d_sample_map, uint32_t sample_begin,
                          void* d_rgb, void* d_mean, void* d_samples, void* d_variance, void* hip_stream, crt_map_info* info);

/* The sample count each pixel needs, from the sums of the frame in flight: crt_render_adaptive's stop criterion solved for n (the
 * variance of the mean falls as 1 / n).  Reads the handle's sums only; writes one uint32 per pixel in the layout of the frame's out_mean
 * (row-major, or the shard's compact tiles, padding slots 0).  With n = samples accumulated, S = the frame's spp, fn = (float)n,
 * fs = (float)S, every operation one IEEE fp32 operation, no FMA:
 *   r = fs / fn;  rr = r * r;  per channel var = crt_variance's formula, p = c * r
 *   v = (var.x + var.y) + var.z;   m = (p.x + p.y) + p.z
 *   t = threshold * (m + mean_floor);   tt = t * t;   w = (fn * v) / tt
 *   n_p = (w < fs) ? max(n, (uint32_t)ceilf(w)) : S
 * so NaN, +inf and w >= S all give the cap; threshold 0 sends every pixel to the cap, threshold +inf every pixel to n.  A row-major map
 * of a whole frame is what crt_render_map takes with sample_begin = n.
 * CRT_ERR_INVALID_ARG, before any device call: a null scene or map; a threshold that is negative or NaN; a mean_floor that is negative
 * or not finite; what crt_variance refuses (no valid variance sums on the handle; n < 2). */
typedef struct {
    uint32_t samples;       /* n: the samples in the sums the plan was made from */
    uint32_t spp;           /* S: the cap */
} crt_plan_info;
int crt_sample_plan(crt_scene* scene, float threshold, float mean_floor, uint32_t* out_map, crt_plan_info* info);
/* d_map: a device buffer on the scene's device; enqueued on hip_stream (NULL = default stream) without synchronizing */
int crt_sample_plan_device(crt_scene* scene, float threshold, float mean_floor, void* d_map, void* hip_stream, crt_plan_info* info);

/* The adaptive frame in two launches: the warm-up crt_render_range(0, min_samples) with the variance sums, crt_sample_plan at
 * n = min_samples with adaptive->threshold and mean_floor, and crt_render_map of that plan with sample_begin = min_samples -- composed on
 * the device, the plan never visits the host.  adaptive->step_samples is ignored; the other fields are checked as crt_render_adaptive
 * checks them.  Outputs, handle state, limits and the one synchronization are crt_render_map's.  Unlike crt_render_adaptive, which looks
 * again after every step, the plan trusts the variance estimate of the first min_samples samples: a pixel whose early samples happen to
 * agree stops at min_samples whatever comes later, and one with an early outlier is sent further than the iterative call would send it
 * (docs/experiments.md, "Sample maps and planned adaptive frames"). */
int crt_render_planned(crt_scene* scene, const crt_camera* cam, const crt_params* params, const crt_adaptive_params* adaptive,
                       uint8_t* out_rgb, float* out_mean, uint32_t* out_samples, float* out_variance, crt_map_info* info);
int crt_render_planned_device(crt_scene* scene, const crt_camera* cam, const crt_params* params, const crt_adaptive_params* adaptive,
                              void* d_rgb, void* d_mean, void* d_samples, void* d_variance, void* hip_stream, crt_map_info* info);

/* The error of the frame in flight in one small struct: the sums c and q of the crt_variance contract, reduced on the device over the
 * shard's VALID pixel slots (padding slots of a tiled shard count for nothing).  Accepts the state crt_variance accepts -- a frame in
 * flight or the last finished frame, rendered with CRT_FLAG_VARIANCE, n >= 2 samples in the sums -- and changes nothing on the handle:
 * a call between two ranges changes no later bit.  With S = the frame's spp, fn = (float)n, fs = (float)S, per valid slot, every
 * operation one IEEE fp32 operation, no FMA (crt_render_adaptive's criterion):
 *   r = fs / fn;  rr = r * r
 *   per channel  d = fn * q - c * c;  d = d < 0.0f ? 0.0f : d;  var = (rr * d) / (fn - 1.0f);   p = c * r
 *   v = (var.x + var.y) + var.z;   m = (p.x + p.y) + p.z;   t = threshold * (m + mean_floor);   tt = t * t
 *   nan_pixels  slots where v or tt is NaN
 *   above       slots with !(v <= tt): the pixels crt_render_adaptive would send on, NaN slots included
 *   hist[b]     the other slots by b = the number of j in 0 .. 14 with v > tt * e_j, e_j = 4^(j - 7) (an exact fp32 constant, the product
 *               one fp32 multiply).  e_7 = 1, so above == hist[8] + ... + hist[15] + nan_pixels, and the sum of hist + nan_pixels ==
 *               pixels.  Bin b <= 7 holds the pixels whose v is within 4^(b - 7) times the target, bin 8 + k those beyond it by up to 4^(k + 1).
 *   sum_variance, sum_mean   fp64 sums of (double)v and (double)m over the valid slots that are not NaN slots; every other slot
 *               contributes +0.0.  Every add is one IEEE fp64 add and their order is part of the contract, so that the bits do not
 *               depend on how the reduction is launched:
 *     1. slots are taken in blocks of 256 consecutive slot indices (the last block filled up with +0.0), in a block in groups of 64
 *     2. in a group, for s = 32, 16, 8, 4, 2, 1:  x[t] += x[t + s] for every t < s; the group's sum is x[0]: w0 .. w3 of the block
 *     3. the block's partial is ((w0 + w1) + w2) + w3
 *     4. with P[0 .. nb) the blocks' partials: lane l of ONE group of 64 adds P[l], P[l + 64], ... in ascending order to +0.0
 *     5. the 64 lane sums are folded by the tree of step 2
 * The counts are integers: exact in any order.
 * CRT_ERR_INVALID_ARG, before any device call, the handle untouched: what crt_variance refuses (a null scene; no valid variance sums
 * on the handle; n < 2); a null output; a threshold that is negative or NaN; a mean_floor that is negative or not finite.
 * crt_frame_error_defaults gives threshold 0.05 and mean_floor 0.01, crt_adaptive_defaults' values (untuned). */
typedef struct {
    uint32_t samples_done;  /* n: the samples in the sums */
    uint32_t spp;           /* S */
    uint64_t pixels;        /* the shard's valid pixel slots */
    uint64_t nan_pixels;
    uint64_t above;
    uint64_t hist[16];
    double sum_variance;
    double sum_mean;
} crt_frame_error_info;
int crt_frame_error_defaults(float* threshold, float* mean_floor);
/* returns the struct; synchronizes once */
int crt_frame_error(crt_scene* scene, float threshold, float mean_floor, crt_frame_error_info* out);
/* d_out: sizeof(crt_frame_error_info) bytes on the scene's device, 8-byte aligned; enqueued on hip_stream (NULL = default stream)
 * without synchronizing.  The partial sums live in a scratch buffer on the handle: one summary of a handle at a time. */
int crt_frame_error_device(crt_scene* scene, float threshold, float mean_floor, void* d_out, void* hip_stream);

/* A uniform frame rendered until it is clean enough, and left in flight.  CRT_FLAG_VARIANCE is implied; every other flag means what it
 * means to crt_render_range.  In terms of the calls above, S = params->spp:
 *   1. sample_begin == 0: crt_render_range(0, min_samples); n = min_samples.
 *      sample_begin > 0: the frame in flight must hold exactly samples [0, sample_begin) of every pixel with CRT_FLAG_VARIANCE from
 *      sample 0 on, at the same spp, size, shard and layout.  sample_begin < min_samples: crt_render_range(sample_begin, min_samples -
 *      sample_begin), n = min_samples; else n = sample_begin and nothing is rendered yet.
 *   2. E = crt_frame_error(threshold, mean_floor) at n; E.above is recorded.  E.above <= max_above or n == S: stop.
 *   3. ns = min(step_samples, S - n); crt_render_range(n, ns); n += ns; step 2.
 * n == S: the last range wrote the frame: out_rgb / out_mean are crt_render's bits, out_variance crt_variance's, the frame is finished.
 * n < S: out_rgb / out_mean are crt_preview's bits at n, out_variance crt_variance's at n, and THE FRAME STAYS IN FLIGHT at n: a later
 * crt_render_range(n, ...) or crt_render_until(sample_begin = n) with a stricter target continues it, and run to S it ends with
 * crt_render's bits.  out_rgb is required; out_mean, out_variance and info are optional.
 * CRT_ERR_INVALID_ARG, before any device call, the handle as it was: a null scene, camera, params, until params or out_rgb;
 * min_samples < 2 or > spp; step_samples == 0; threshold / mean_floor as crt_frame_error; a sample_begin that does not continue the
 * frame in flight; whatever crt_render_range with CRT_FLAG_VARIANCE refuses, refused as it refuses it.  crt_multi has no such call.
 * crt_until_defaults fills min_samples 16, step_samples 64 (crt_adaptive_defaults' values: every range is a launch of the render
 * kernel with its tail), threshold 0.05, mean_floor 0.01, max_above 0. */
typedef struct {
    uint32_t min_samples;   /* the first check is made at max(min_samples, sample_begin) samples; >= 2, <= spp */
    uint32_t step_samples;  /* samples per range after it; >= 1 */
    float threshold;
    float mean_floor;
    uint64_t max_above;     /* pixels that may stay above the target */
} crt_until_params;
#define CRT_UNTIL_CHECKS_REPORTED 64
typedef struct {
    uint32_t passes;        /* ranges this call rendered */
    uint32_t checks;        /* summaries it read */
    uint32_t samples_done;  /* n at the end */
    uint32_t reserved_;
    uint64_t above[CRT_UNTIL_CHECKS_REPORTED]; /* E.above of check 0, 1, ... (checks beyond 64 are not recorded) */
    uint64_t paths;         /* pixels x samples this call rendered */
    float kernel_ms;        /* the render kernel's launches (0 on the fallback pipeline) */
    float total_ms;
    crt_frame_error_info last; /* the summary of the last check */
} crt_until_info;
int crt_until_defaults(crt_until_params* params);
int crt_render_until(crt_scene* scene, const crt_camera* cam, const crt_params* params, const crt_until_params* until, uint32_t sample_begin,
                     uint8_t* out_rgb, float* out_mean, float* out_variance, crt_until_info* info);
/* d_rgb / d_mean / d_variance: device buffers in the layout of crt_render_device's, enqueued on hip_stream (NULL = default stream).
 * SYNCHRONIZES hip_stream once per check, as crt_render_adaptive_device per pass, to read E.above: one 8-byte copy into pinned memory;
 * once more at the end when info != NULL (the last summary and the timers). */
int crt_render_until_device(crt_scene* scene, const crt_camera* cam, const crt_params* params, const crt_until_params* until, uint32_t sample_begin,
                            void* d_rgb, void* d_mean, void* d_variance, void* hip_stream, crt_until_info* info);

/* The order in which the render kernel hands out the last work items of a launch (the paths the roulette draws will let run longest
 * first: it shortens the end of a launch, where every wave runs its pool dry, and cannot change a result).  The order is a list on the
 * handle that depends on the seed, the sample range, the size and shard of the frame, p_rr and the stream -- not on the camera or the
 * scene -- and is built again only when one of these changes between two launches.  For the handle: the launches of the render kernel
 * that built the list and that found it built, and of the last launch the number of length classes and the work items per cursor shard
 * that were ordered (both 0: cursor order -- CRT_ITEM_ORDER=0, the fallback pipeline -- or the list of a sparse frame). */
typedef struct {
    uint64_t lists_built, lists_reused;
    uint32_t classes, window;
} crt_item_order_info;
int crt_item_order(crt_scene* scene, crt_item_order_info* info);

#ifdef __cplusplus
}
#endif
#endif /* CRT_H */
