// cudaraytracing_amd/csrc/crt_internal.h -- between the translation units of libcrt.so's device layer: error plumbing, device
// buffers (with the copies of the host-buffer forms), the stages the image-space kernels share (slot map, three-plane sums, sample fold,
// output write), and the launch entry points each kernel file exports to the host code in crt_render.hip (crt_scene.h: the scene handle).
#ifndef CRT_INTERNAL_H
#define CRT_INTERNAL_H
#include <cstdlib>
#include "crt_mega3.h"

#include <cstddef>
#include <string>
#include <vector>

extern "C" void crt_set_last_error_(const char* msg);

namespace crtk {

struct HipFail {
    hipError_t e;
    const char* what;
};
#define HIP_CHECK(call)                                          \
    do {                                                         \
        hipError_t e_ = (call);                                  \
        if (e_ != hipSuccess) throw HipFail{e_, #call};          \
    } while (0)

// an entry point's error return: the message goes to crt_last_error
inline int fail(int status, const std::string& msg)
{
    crt_set_last_error_(msg.c_str());
    return status;
}
inline int fail_hip(const HipFail& f) { return fail(CRT_ERR_HIP, std::string(f.what) + ": " + hipGetErrorString(f.e)); }

template <typename T> struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    void alloc(size_t count)
    {
        release();
        if (count == 0) count = 1;
        HIP_CHECK(hipMalloc((void**)&p, count * sizeof(T)));
        n = count;
        debug_fill();
    }
    // CRT_DEBUG_FILL=<byte>: every new allocation is filled with that byte (tests: a read of memory nobody wrote shows up whatever the
    // allocator hands out)
    void debug_fill()
    {
        static const char* e = std::getenv("CRT_DEBUG_FILL");
        if (!e || !*e) return;
        if (e[0] == 's') { HIP_CHECK(hipDeviceSynchronize()); return; }       // synchronise only
        if (e[0] == 'u' && !uncached) return;                                  // u<byte>: uncached allocations only
        if (e[0] == 'c' && uncached) return;                                   // c<byte>: cached allocations only
        const char* v = (e[0] == 'u' || e[0] == 'c') ? e + 1 : e;
        HIP_CHECK(hipMemset(p, std::atoi(v) & 0xff, n * sizeof(T)));
    }
    void ensure(size_t count)
    {
        if (n < count) alloc(count);
    }
    // Uncached device memory: every access goes to memory, past the L2 caches of the XCDs, which are not coherent with one another
    // inside a launch (the commit ring's buffers: written by one wave, read by another during the same launch).
    void ensure_uncached(size_t count)
    {
        if (n >= count && uncached) return;
        release();
        if (count == 0) count = 1;
        HIP_CHECK(hipExtMallocWithFlags((void**)&p, count * sizeof(T), hipDeviceMallocUncached));
        n = count;
        uncached = true;
        debug_fill();
    }
    bool uncached = false;
    template <typename Row> T* upload(const std::vector<Row>& v) // (Row: T, or the plain-C++ row type of crt_scene_layout.h with T's layout)
    {
        static_assert(sizeof(Row) == sizeof(T) && alignof(T) % alignof(Row) == 0, "upload is a byte copy");
        alloc(v.size());
        if (!v.empty()) HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return p;
    }
    // the host-buffer forms of the entry points: a buffer the size of the host array (null: none, and nothing to copy back)
    T* upload(const T* h, size_t count)
    {
        if (!h) return nullptr;
        alloc(count);
        HIP_CHECK(hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice));
        return p;
    }
    void download(T* h, size_t count) const
    {
        if (h) HIP_CHECK(hipMemcpy(h, p, count * sizeof(T), hipMemcpyDeviceToHost));
    }
    void release()
    {
        if (p) { (void)hipFree(p); p = nullptr; n = 0; uncached = false; }
    }
    ~DevBuf() { release(); }
};

const int kMaxBatch = 64;

// the frame's tone map (write_color)
__device__ __forceinline__ uint8_t to_u8(float v)
{
    if (!(v == v)) return 0;
    if (v <= 0.0f) return 0;
    if (v >= 255.0f) return 255;
    return (uint8_t)v; // truncation (Render.cuh:350)
}
// reference: Global.h:121-124 then Render.cuh:350
__device__ __forceinline__ uint8_t tonemap(float c)
{
    float cl = maxf_ref(0.0f, minf_ref(1.0f, c));
    return to_u8(255 * det_powf(cl, 0.6f));
}

// ---- the image-space kernels' shared stages (crt_frame.hip, crt_adaptive.hip, crt_aov.hip; the denoiser takes write_color) ----
// Which pixel slots a shard has and where each one's pixel lies in the output: the arguments of slot_to_pixel (crt_path.h) and the
// output layout.  Filled on the host by fill_slot_map (crt_scene.h).
struct SlotMap {
    uint32_t width, height, rank, world, tiles_x, n_tiles, nslots, tiled_output;
    FastDiv tiles_x_div;
};
// A slot of the map: `valid` = it is a pixel, (i, j); `out` = it has an entry in the output (every slot of a tiled output, padding
// included; the pixels of a row-major one), at index o
struct SlotPixel {
    bool valid, out;
    uint32_t i, j;
    uint64_t o;
};
__device__ __forceinline__ SlotPixel slot_pixel(const SlotMap& m, const uint32_t slot)
{
    SlotPixel p;
    p.i = 0; p.j = 0;
    p.valid = slot_to_pixel(slot, m.rank, m.world, m.n_tiles, m.tiles_x, m.tiles_x_div, m.width, m.height, p.i, p.j);
    p.out = p.valid || m.tiled_output;
    p.o = m.tiled_output ? (uint64_t)slot : (uint64_t)p.j * m.width + p.i;
    return p;
}

// the frame kernels (k_accumulate, k_preview, k_variance) and, inside AdaptiveParams, the adaptive ones
struct AParams : SlotMap {
    uint32_t spp;
    uint32_t chunk_samples;
    uint32_t first_chunk, last_chunk;
    const Rad3* L;     // the chunk's radiance, 12 bytes per work item: L[sample of the chunk * nslots + slot]
    float* accum;      // 3 planes of nslots (running sum across chunks)
    uint8_t* out_rgb;
    float* out_mean;   // may be null
};

// The sums c and q: three planes of nslots floats in uncached memory that commit-ring launches read and write with agent-scope atomics --
// the same accesses here
__device__ __forceinline__ float acc_load(const float* p) { return __uint_as_float(__hip_atomic_load((const unsigned int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); }
__device__ __forceinline__ void acc_store(float* p, const float v) { __hip_atomic_store((unsigned int*)p, __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ F3 acc_load3(const float* planes, const uint32_t nslots, const uint32_t slot)
{
    return f3(acc_load(planes + slot), acc_load(planes + nslots + slot), acc_load(planes + 2ull * nslots + slot));
}
__device__ __forceinline__ void acc_store3(float* planes, const uint32_t nslots, const uint32_t slot, const F3 v)
{
    acc_store(planes + slot, v.x); acc_store(planes + nslots + slot, v.y); acc_store(planes + 2ull * nslots + slot, v.z);
}

// The chunk's samples of a slot into its sums, in sample order: c = c + L / spp (Render.cuh:348); VAR (CRT_FLAG_VARIANCE, adaptive
// passes): also the sum of squares q = q + x * x of the same quotients x.  Without VAR q is not touched.
// The radiance is read with ONE plain 12-byte load per sample: the launch that wrote it has ended, and a kernel boundary makes its stores
// visible (docs/experiments.md 6.14; the three 4-byte agent-scope loads per sample that stood here since round 5 cost more than a quarter
// of k_accumulate).  The sums keep their agent scope: launches with the commit ring write them from inside the launch.
// fold_samples_n: the first `count` samples of the chunk.
template <bool VAR> __device__ __forceinline__ void fold_samples_n(const AParams& A, const uint32_t slot, const uint32_t count, F3& c, F3& q)
{
    const float fspp = (float)A.spp;
    const Rad3* lp = A.L + slot;
#pragma unroll 4
    for (uint32_t s = 0; s < count; s++, lp += A.nslots) {
        const Rad3 l = load_radiance(lp);
        if (VAR) {
            const float xx = l.x / fspp, xy = l.y / fspp, xz = l.z / fspp;
            c.x = c.x + xx; c.y = c.y + xy; c.z = c.z + xz;
            q.x = q.x + xx * xx; q.y = q.y + xy * xy; q.z = q.z + xz * xz;
        } else {
            c.x = c.x + l.x / fspp;
            c.y = c.y + l.y / fspp;
            c.z = c.z + l.z / fspp;
        }
    }
}
// every slot takes the whole chunk (the frame kernels, an adaptive pass); fold_samples_n with a count of its own per slot: a sample map
template <bool VAR> __device__ __forceinline__ void fold_samples(const AParams& A, const uint32_t slot, F3& c, F3& q) { fold_samples_n<VAR>(A, slot, A.chunk_samples, c, q); }

// the variance of the mean from the sums c and q (contract: crt_variance, include/crt.h); rr = (fs / fn)^2
__device__ __forceinline__ float variance_of(const float c, const float q, const float fn, const float rr)
{
    float d = fn * q - c * c;
    d = d < 0.0f ? 0.0f : d;
    return (rr * d) / (fn - 1.0f);
}
__device__ __forceinline__ F3 variance_of3(const F3 c, const F3 q, const float fn, const float rr)
{
    return f3(variance_of(c.x, q.x, fn, rr), variance_of(c.y, q.y, fn, rr), variance_of(c.z, q.z, fn, rr));
}

// Colour c of a pixel into entry o of the outputs of parameter block P (P.out_mean and P.out_rgb, either may be null): the mean as it
// is and its tone map; a padding slot of a tiled output (!valid) gets 0 and c, which its kernel left +0
template <class PB> __device__ __forceinline__ void write_color(const PB& P, const uint64_t o, const bool valid, const F3 c)
{
    if (P.out_mean) { P.out_mean[o * 3 + 0] = c.x; P.out_mean[o * 3 + 1] = c.y; P.out_mean[o * 3 + 2] = c.z; }
    if (P.out_rgb) {
        P.out_rgb[o * 3 + 0] = valid ? tonemap(c.x) : 0;
        P.out_rgb[o * 3 + 1] = valid ? tonemap(c.y) : 0;
        P.out_rgb[o * 3 + 2] = valid ? tonemap(c.z) : 0;
    }
}


// wavefront pipeline (crt_wavefront.hip)
#define REFILL_MIN 32
#define LEAF_MIN 24
#define SLOT_SHARDS 64
#define SLOT_STRIDE 32
void launch_pool_init(uint32_t blocks, hipStream_t st, const Pool& pool);
void launch_logic(bool lds_tables, uint32_t blocks, hipStream_t st, const LParams& P);
int trace_blocks_per_cu(int mode_id, size_t lds);
void launch_trace(int mode_id, const TParams& T, uint32_t blocks, size_t lds, hipStream_t st);
// frame and test kernels (crt_frame.hip)
void launch_accumulate(const AParams& A, hipStream_t st);
void launch_accumulate_var(const AParams& A, float* qacc, hipStream_t st); // CRT_FLAG_VARIANCE: c and the sum of squares q (3 planes of nslots)
void launch_variance(const AParams& A, const float* qacc, float fn, float fs, hipStream_t st); // crt_variance: A.accum, qacc -> A.out_mean
void launch_preview(const AParams& A, float scale, hipStream_t st);
void launch_fill_rays(const Pool& pool, uint32_t n, const float* o, const float* d, bool raw_dir, const float* limits);
void launch_math(int fn, uint32_t n, const float* a, const float* b, float* out);
void launch_philox(uint32_t n, const uint32_t* ctr, const uint32_t* key, uint32_t* out);
void launch_rcp_check(unsigned long long* counts);

// first-hit AOV pass (crt_aov.hip; host side: crt_render_aov in crt_render.hip).  One chunk = samples [sample_begin, sample_begin + n_samples)
// of every pixel slot of the shard; query ray / result item = sample offset in the chunk x nslots + slot.
struct AovParams : SlotMap {
    // the camera, as LParams holds it (camera_dir; width and height: the slot map's)
    float eye[3];
    float inv_view[9];
    float scale, ar;
    uint64_t seed;
    uint32_t spp, sample_begin, n_samples;
    uint32_t first_chunk, last_chunk;
    Pool pool;               // k_aov_rays: the query pool (ro, rd, res)
    const float* res;        // k_aov_resolve: (t, bits(triangle or -1)) of item i at res[i * res_stride]
    uint32_t res_stride;     // floats per item: 4 (k_mega3 query form, its float4 answers) or 2 (k_trace, the pool's res plane)
    const float4* tri_nm;    // scene: normal.xyz, bits(material word) per triangle
    const float4* mats;      // scene: 3 rows per material, row 1 = kd.xyz
    float4* acc;             // [nslots][3] running sums across chunks: (albedo.xyz, depth), (normal.xyz, bits(hits)), (bits(tri_0), bits(m_0), -, -)
    float* albedo;           // outputs (any may be null): row-major W x H, or nslots with tiled_output
    float* normal;
    float* depth;
    float* coverage;
    int32_t* tri;
    int32_t* material;
};
void launch_aov_rays(const AovParams& A, hipStream_t st);
void launch_aov_resolve(const AovParams& A, hipStream_t st);

// adaptive sampling (crt_adaptive.hip; host side: crt_render_adaptive in crt_render.hip; contract: include/crt.h).  Beside the frame's
// sums c (A.accum) and q (qacc) the handle keeps, per pixel slot, whether the pixel still takes samples and how many it has; a pass
// renders the slots of `list`.  All of these live in uncached memory and are accessed with agent-scope atomics only, as the sums are.
struct AdaptiveParams {
    AParams A;               // the frame's layout and sums; L, chunk_samples: the chunk k_adaptive_accumulate folds in
    float* qacc;
    uint32_t* active;        // [nslots] 1 = the pixel takes the next pass's samples (padding slots: 0)
    uint32_t* nsamp;         // [nslots] n_p so far
    uint32_t* list;          // [count] the active slots, in any order (k_adaptive_select)
    unsigned int* count;
    uint32_t n;              // samples every active pixel has (k_adaptive_accumulate: after its chunk)
    float threshold, mean_floor;
    uint32_t* out_samples;   // k_adaptive_resolve: beside A.out_rgb / A.out_mean (any may be null)
    float* out_variance;
};
void launch_adaptive_init(const AdaptiveParams& D, hipStream_t st);       // after the warm-up: every pixel active, n_p = D.n
void launch_adaptive_select(const AdaptiveParams& D, hipStream_t st);     // the stop criterion at n = D.n; compacts the active slots into list / count
// item_list[pos] = the frame's work item (sample s of the chunk, slot list[a]) of cursor position pos = s * n_active + a
void launch_adaptive_items(uint32_t* item_list, const uint32_t* list, uint32_t n_active, uint32_t n_items, uint32_t nslots, hipStream_t st);
void launch_adaptive_accumulate(const AdaptiveParams& D, hipStream_t st); // the chunk's samples into c and q of the active slots
void launch_adaptive_resolve(const AdaptiveParams& D, hipStream_t st);    // mean, RGB, samples, variance in the output layout

// sample maps (crt_sample_map.hip; host side: crt_render_map, crt_sample_plan and crt_render_planned in crt_render.hip; contract:
// include/crt.h).  The count plane n_p is the adaptive frame's (AdaptiveParams::nsamp: k_adaptive_resolve makes the frame from it); the
// histogram and the cursors live in uncached memory and are accessed with agent-scope atomics only, as the planes are.
struct MapParams {
    AParams A;               // the frame's layout and sums; L, first_chunk: the chunk k_map_fold folds in
    float* qacc;
    uint32_t* nsamp;         // [nslots] n_p (padding slots: 0)
    const uint32_t* map;     // k_map_prepare: the caller's counts, one per pixel of the W x H image (row-major) or, map_per_slot, per pixel slot
    uint32_t map_per_slot;
    uint32_t sample_begin;   // k_map_prepare: the samples every pixel has already
    unsigned int* hist;      // k_map_prepare: [spp + 1] slots per value of n_p, zeroed before the launch
    unsigned int* cursor;    // k_map_items: [spp] where the next entry of sample s goes in its chunk's list
    uint32_t* item_list;     // k_map_items: n_items entries
    uint32_t n_items;
    uint32_t s0, ns;         // k_map_items, k_map_fold: the chunk's samples [s0, s0 + ns)
    uint32_t n;              // k_sample_plan: samples in the sums
    float threshold, mean_floor;
    uint32_t* out_map;       // k_sample_plan: in the frame's output layout
};
void launch_map_prepare(const MapParams& D, hipStream_t st);
void launch_map_items(const MapParams& D, hipStream_t st);
void launch_map_fold(const MapParams& D, hipStream_t st);
void launch_sample_plan(const MapParams& D, hipStream_t st);

} // namespace crtk
#endif
