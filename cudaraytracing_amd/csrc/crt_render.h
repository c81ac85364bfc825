// cudaraytracing_amd/csrc/crt_render.h -- what crt_sparse.hip (the sparse frames: crt_render_adaptive, crt_render_map, crt_sample_plan,
// crt_render_planned) and crt_aov_pass.hip (the AOV passes: crt_render_aov*) take from crt_render.hip, and nothing else of it.
#ifndef CRT_RENDER_H
#define CRT_RENDER_H
#include "crt_scene.h"

namespace crtk {

// Where the work items of a range come from when not every pixel slot takes every sample.  A Frame may carry one; without, every chunk
// is the uniform hand-out: samples x pixel slots.  With one, the whole cursor range of a launch goes through an item list that names the
// frame's own work item (sample of the chunk x nslots + slot) of every position: k_mega3 decodes it and writes L[item] as ever.
struct ItemSource {
    SumsParams sums; // the frame's sums and its count plane, which says how far into the range each slot's samples reach
    // work items of chunk k (0, 1, ... of the range), which holds ns samples
    virtual uint32_t items(uint32_t k, uint32_t ns) const = 0;
    // the list of the chunk of samples [s0, s0 + ns): n_items entries, enqueued on st
    virtual void fill(uint32_t* item_list, uint32_t s0, uint32_t ns, uint32_t n_items, hipStream_t st) const = 0;
    // the chunk's radiance (A.L) into the sums, enqueued on st: every slot takes as many of the chunk's samples as its count reaches into it
    void fold(const AParams& A, uint32_t s0, uint32_t ns, hipStream_t st) const { launch_map_fold(SumsParams{A, sums.qacc, sums.nsamp}, s0, ns, st); }
};

const uint64_t kMaxChunkItems = 1ull << 30; // paths per chunk (12.9 GB of per-path radiance: sized for 288 GB of HBM, every launch ends with a 2 ms tail)
uint32_t chunk_samples(uint32_t nslots, uint32_t s_count);
uint32_t choose_pipeline(const crt_scene* sc);
int params_check(const char* who, const crt_params* prm, bool camera_rays_only = false);
bool continues_frame(const FrameMark& f, const crt_params* prm, uint32_t s_begin, bool tiled);
AParams frame_aparams(const crt_scene* sc, const FrameMark& f, const Shard& sh);
void ensure_events(crt_scene* sc);
void camera_scale_ar(const crt_camera* cam, const crt_params* prm, float& scale, float& ar);
// 1 / n for n a power of two (exactly representable), else 0: LParams::inv_lsn_pow2 of a frame and of the direct-light AOV pass
inline float inv_if_pow2(int32_t n) { return (n > 0 && (n & (n - 1)) == 0) ? 1.0f / (float)n : 0.0f; }
// The n query rays in the handle's query pool, from `first` on, traced on st: the answers stay on the device, `stride` floats apart
const float* trace_queries(crt_scene* sc, uint32_t n, uint32_t traversal, bool force_exact, hipStream_t st, uint32_t& stride, size_t first = 0);
// src: the range's item source.  open: the range belongs to a frame its caller resolves (every range of a sparse frame, its uniform
// warm-up and the ranges with a source alike): the range that ends at spp tone-maps nothing, d_rgb / d_mean are not used.
int render_impl(crt_scene* sc, const crt_camera* cam, const crt_params* prm, void* d_rgb, void* d_mean, hipStream_t st, crt_stats* stats, uint32_t s_begin = 0,
                uint32_t s_count = 0xffffffffu, const ItemSource* src = nullptr, bool open = false);

// Pixels (or, tiled, pixel slots) of the frame buffers a shard writes
inline uint64_t out_pixels(uint32_t w, uint32_t h, uint32_t world, bool tiled) { return tiled ? make_shard(w, h, world).nslots : (uint64_t)w * h; }

// The host-buffer form of an entry that writes an rgb8 frame and / or three float planes: device buffers for the device form (null
// where not asked for), then the copies back
struct Staging {
    uint64_t npix;
    DevBuf<uint8_t> rgb;
    DevBuf<float> f32;
    Staging(uint64_t npix_, bool want_rgb, bool want_f32) : npix(npix_)
    {
        if (want_rgb) rgb.alloc(npix * 3);
        if (want_f32) f32.alloc(npix * 3);
    }
    void download(uint8_t* out_rgb, float* out_f32)
    {
        HIP_CHECK(hipDeviceSynchronize()); // Render.cuh:440
        rgb.download(out_rgb, npix * 3); // Render.cuh:464
        f32.download(out_f32, npix * 3);
    }
};

} // namespace crtk
#endif
