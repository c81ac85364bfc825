// cudaraytracing_amd/csrc/crt_internal.h -- between the translation units of libcrt.so's device layer: error plumbing, device
// buffers (with the copies of the host-buffer forms), the stages the image-space kernels share (crt_stages.h: slot map, three-plane sums,
// sample fold, output write), and the launch entry points each kernel file exports to the host code in crt_render.hip and crt_sparse.hip
// (crt_scene.h: the scene handle).
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
// The device calls of an entry point: body() returns the entry's status; a HIP error that HIP_CHECK throws inside it becomes CRT_ERR_HIP
template <class Body> int hip_guard(Body body)
{
    try { return body(); } catch (const HipFail& f) { return fail_hip(f); }
}

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

} // namespace crtk

#include "crt_stages.h" // the image-space kernels' shared stages

namespace crtk {

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
void launch_accumulate_half(const AParams& A, float* qacc, float* hacc, uint32_t parity, hipStream_t st); // CRT_FLAG_HALF_BUFFERS: c, q and the half sums (6 planes); parity of the chunk's first sample
void launch_half_buffers(const AParams& A, const float* hacc, float* out_a, float* out_b, float scale_a, float scale_b, hipStream_t st); // crt_half_buffers
void launch_variance(const AParams& A, const float* qacc, float fn, float fs, hipStream_t st); // crt_variance: A.accum, qacc -> A.out_mean
void launch_preview(const AParams& A, float scale, hipStream_t st);
// pixel reconstruction filters (crt_pixel_filter.hip): the chunk A describes into the four planes of filter pf's sums; s0: the chunk's first sample in the frame
void launch_pixel_filter(const AParams& A, const crt_pixel_filter& pf, float* planes, uint64_t seed, uint32_t s0, hipStream_t st);
void launch_fill_rays(const Pool& pool, uint32_t n, const float* o, const float* d, bool raw_dir, const float* limits);
void launch_math(int fn, uint32_t n, const float* a, const float* b, float* out);
void launch_philox(uint32_t n, const uint32_t* ctr, const uint32_t* key, uint32_t* out);
void launch_rcp_check(unsigned long long* counts);

// first-hit AOV pass (crt_aov.hip; host side: crt_render_aov in crt_aov_pass.hip).  One chunk = samples [sample_begin, sample_begin + n_samples)
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
                             // the shading form: [nslots][4], row 2 = (bits(tri_0), bits(m_0), emission.xy), row 3 = (emission.z, diffuse_albedo.xyz)
    float* albedo;           // outputs (any may be null): row-major W x H, or nslots with tiled_output
    float* normal;
    float* depth;
    float* coverage;
    int32_t* tri;
    int32_t* material;
};
void launch_aov_rays(const AovParams& A, hipStream_t st);
void launch_aov_resolve(const AovParams& A, hipStream_t st);
// crt_render_aov_shading: the outputs the shading form of the resolve writes beside AovParams' (either may be null), same layout
struct AovShadingOut {
    float* emission;
    float* diffuse_albedo;
};
void launch_aov_resolve_shading(const AovParams& A, const AovShadingOut& H, hipStream_t st);

// AOV pass that follows mirror bounces (crt_aov.hip; host side: crt_render_aov_specular in crt_aov_pass.hip).  Items as above.  A stage
// reads the answers of the n_in rays traced last (stage 0: the camera rays, ray i = item i; later: the reflected rays, ray i of item
// in_item[i]), advances the chain state of their items and compacts the rays that go on into the other half of the query pool.
struct AovSpecParams : SlotMap {
    uint32_t spp, n_samples;
    uint32_t first_chunk, last_chunk;
    uint32_t max_bounces;
    // k_aov_bounce
    uint32_t n_in, stage0;
    const float4* in_ro;     // the rays traced (xyz)
    const float4* in_rd;
    const uint32_t* in_item;
    const float* res;        // their answers, as AovParams::res
    uint32_t res_stride;
    float4* out_ro;          // the rays that go on, primed as k_aov_rays primes them: at most n_in
    float4* out_rd;
    float2* out_res;
    uint32_t* out_item;
    unsigned int* count;     // how many (zeroed by the host)
    float4* state;           // per item: thr.xyz, len
    int2* aux;               // per item: (last triangle hit, or -1 after a miss), B; a sample whose camera ray missed: (-1, 0)
    const float4* tri_nm;
    const float4* mats;      // 3 rows per material, row 1 = kd.xyz, row 2 = ke.xyz
    // k_aov_spec_resolve
    float4* acc;             // [nslots][3] running sums across chunks: (guide.xyz, sum D), (normal.xyz, bits(hits)), (sum B, bits(tri_L of sample 0), -, -)
    float* guide_albedo;     // outputs (any may be null), layout as AovParams
    float* last_normal;
    float* path_depth;
    float* bounces;
    int32_t* last_tri;
};
void launch_aov_bounce(const AovSpecParams& S, hipStream_t st);
void launch_aov_spec_resolve(const AovSpecParams& S, hipStream_t st);

// sparse frames (parameter blocks: crt_stages.h; host side: crt_sparse.hip)
// crt_adaptive.hip
void launch_adaptive_init(const AdaptiveParams& D, hipStream_t st);       // after the warm-up: n_p = D.n at every pixel, 0 at padding slots
void launch_adaptive_select(const AdaptiveParams& D, hipStream_t st);     // the stop criterion at the slots with n_p == D.n; those that go on: into list / count, n_p = D.n + D.ns_pass
// item_list[pos] = the frame's work item (sample s of the chunk, slot list[a]) of cursor position pos = s * n_active + a
void launch_adaptive_items(uint32_t* item_list, const uint32_t* list, uint32_t n_active, uint32_t n_items, uint32_t nslots, hipStream_t st);
void launch_adaptive_resolve(const SumsParams& D, uint32_t* out_samples, float* out_variance, hipStream_t st); // mean, RGB (D.A.out_*), samples, variance in the output layout; any may be null
// crt_sample_map.hip
void launch_map_prepare(const MapParams& D, hipStream_t st);
void launch_map_items(const MapParams& D, hipStream_t st);
void launch_map_fold(const SumsParams& D, uint32_t s0, uint32_t ns, hipStream_t st); // samples [s0, s0 + ns) into c and q: slot p takes those below n_p
void launch_sample_plan(const MapParams& D, hipStream_t st);

} // namespace crtk
#endif
