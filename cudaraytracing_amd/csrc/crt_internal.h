// cudaraytracing_amd/csrc/crt_internal.h -- between the translation units of libcrt.so's device layer: error plumbing, device
// buffers, and the launch entry points each kernel file exports to the host code in crt_render.hip (crt_scene.h: the scene handle).
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
    void release()
    {
        if (p) { (void)hipFree(p); p = nullptr; n = 0; uncached = false; }
    }
    ~DevBuf() { release(); }
};

const int kMaxBatch = 64;

// the frame's tone map, shared by k_accumulate / k_preview (crt_frame.hip) and the denoiser's last pass (crt_denoise.hip)
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

// shared by the per-pixel-slot kernels of crt_frame.hip and crt_adaptive.hip
__device__ __forceinline__ FastDiv make_fastdiv_dev(uint32_t d)
{
    // k_accumulate runs once per pixel: derive the magic on the fly (same formula as make_fastdiv)
    uint32_t l = d > 1 ? 32u - (uint32_t)__clz((int)(d - 1)) : 0u;
    FastDiv f;
    f.m = (uint32_t)((((1ull << l) - d) << 32) / d + 1);
    f.sh = (l < 1 ? l : 1u) | ((l > 0 ? l - 1 : 0u) << 8);
    return f;
}

__device__ __forceinline__ float acc_load(const float* p) { return __uint_as_float(__hip_atomic_load((const unsigned int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); }
__device__ __forceinline__ void acc_store(float* p, const float v) { __hip_atomic_store((unsigned int*)p, __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the variance of the mean from the sums c and q (contract: crt_variance, include/crt.h); rr = (fs / fn)^2
__device__ __forceinline__ float variance_of(const float c, const float q, const float fn, const float rr)
{
    float d = fn * q - c * c;
    d = d < 0.0f ? 0.0f : d;
    return (rr * d) / (fn - 1.0f);
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
struct AovParams {
    // the camera, as LParams holds it (camera_dir)
    float eye[3];
    float inv_view[9];
    float scale, ar;
    uint32_t width, height;
    uint64_t seed;
    // the shard's pixel slots (slot_to_pixel)
    uint32_t rank, world, tiles_x, n_tiles, nslots;
    FastDiv tiles_x_div;
    uint32_t spp, sample_begin, n_samples;
    uint32_t first_chunk, last_chunk, tiled_output;
    Pool pool;               // k_aov_rays: the query pool (ro, rd, res)
    const float* res;        // k_aov_resolve: (t, bits(triangle or -1)) of item i at res[i * res_stride]
    uint32_t res_stride;     // floats per item: 4 (k_mega3 query form, L) or 2 (k_trace, the pool's res plane)
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

} // namespace crtk
#endif
