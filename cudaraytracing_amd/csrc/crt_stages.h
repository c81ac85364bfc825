// cudaraytracing_amd/csrc/crt_stages.h -- the stages the image-space kernels share (crt_frame.hip, crt_adaptive.hip, crt_sample_map.hip,
// crt_aov.hip; the denoiser takes write_color): the slot map, the frame kernels' parameters, the accessors of the sums and of the word
// planes, the sample fold, the variance formula, the adaptive stop criterion, the output write with its tone map, and the parameter
// blocks of the sparse-frame kernels.  crt_internal.h includes it after crt_mega3.h; it includes nothing itself, so that
// tools/sample_map_host_check.cpp can compile this very text for the host behind stand-ins for what it takes from outside:
// F3 / f3, maxf_ref / minf_ref (crt_device.h), FastDiv (crt_fastdiv.h), det_powf (crt_detmath.h), Rad3, load_radiance, slot_to_pixel
// (crt_path.h), dim3, the __hip_atomic_* builtins and __uint_as_float / __float_as_uint.
#ifndef CRT_STAGES_H
#define CRT_STAGES_H

namespace crtk {

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

// the grid of a kernel with one thread per pixel slot, in blocks of 256
inline dim3 slot_grid(const SlotMap& m) { return dim3((m.nslots + 255) / 256); }

// the frame kernels (k_accumulate, k_preview, k_variance) and, inside SumsParams, the sparse-frame ones
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
// the word planes of a sparse frame (per-slot counts, the list of active slots): uncached memory, the same accesses
__device__ __forceinline__ uint32_t word_load(const uint32_t* p) { return __hip_atomic_load((const unsigned int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void word_store(uint32_t* p, const uint32_t v) { __hip_atomic_store((unsigned int*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The chunk's samples of a slot into its sums, in sample order: c = c + L / spp (Render.cuh:348); VAR (CRT_FLAG_VARIANCE, sparse
// frames): also the sum of squares q = q + x * x of the same quotients x.  Without VAR q is not touched.
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
// every slot takes the whole chunk (the frame kernels); fold_samples_n with a count of its own per slot: a sparse frame
template <bool VAR> __device__ __forceinline__ void fold_samples(const AParams& A, const uint32_t slot, F3& c, F3& q) { fold_samples_n<VAR>(A, slot, A.chunk_samples, c, q); }
// fold_samples_n<true>'s sibling for CRT_FLAG_HALF_BUFFERS (contract: crt_half_buffers, include/crt.h): c and q exactly as there, and the
// same quotients x into h0 (even k) or h1 (odd k), k = the sample's index in the FRAME: `parity` is that of the chunk's first sample
// (AParams does not carry the chunk's start; the launch passes it).  A sibling and not a third template parameter of fold_samples_n, so
// that the kernels built from that one keep their instructions.
__device__ __forceinline__ void fold_samples_half(const AParams& A, const uint32_t slot, const uint32_t count, const uint32_t parity, F3& c, F3& q, F3& h0, F3& h1)
{
    const float fspp = (float)A.spp;
    const Rad3* lp = A.L + slot;
#pragma unroll 4
    for (uint32_t s = 0; s < count; s++, lp += A.nslots) {
        const Rad3 l = load_radiance(lp);
        const float xx = l.x / fspp, xy = l.y / fspp, xz = l.z / fspp;
        c.x = c.x + xx; c.y = c.y + xy; c.z = c.z + xz;
        q.x = q.x + xx * xx; q.y = q.y + xy * xy; q.z = q.z + xz * xz;
        if (((s + parity) & 1u) == 0u) { h0.x = h0.x + xx; h0.y = h0.y + xy; h0.z = h0.z + xz; }
        else { h1.x = h1.x + xx; h1.y = h1.y + xy; h1.z = h1.z + xz; }
    }
}

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

// The adaptive stop criterion of include/crt.h at a slot whose sums hold n samples: v = the variance of the mean summed over the
// channels, tt = (threshold * (mean summed over the channels + mean_floor))^2.  The pixel stops when v <= tt (k_adaptive_select);
// n * v / tt samples would bring it there (k_sample_plan).
struct StopCriterion {
    float v, tt;
};
__device__ __forceinline__ StopCriterion stop_criterion(const AParams& A, const float* qacc, const uint32_t slot, const uint32_t n, const float threshold,
                                                        const float mean_floor)
{
    const float fn = (float)n, fs = (float)A.spp;
    const float r = fs / fn, rr = r * r;
    const F3 c = acc_load3(A.accum, A.nslots, slot);
    const F3 var = variance_of3(c, acc_load3(qacc, A.nslots, slot), fn, rr);
    const F3 p = f3(c.x * r, c.y * r, c.z * r);
    const float v = (var.x + var.y) + var.z, m = (p.x + p.y) + p.z;
    const float t = threshold * (m + mean_floor);
    StopCriterion k;
    k.v = v; k.tt = t * t;
    return k;
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

// ---- sparse frames: not every pixel takes every sample (kernels: crt_adaptive.hip, crt_sample_map.hip; host side: crt_sparse.hip;
// contract: include/crt.h) ----
// What every such frame keeps beside the sum c (A.accum): the sum of squares q and the count plane n_p.  k_map_fold adds a chunk to the
// sums of the slots whose count reaches into it, k_adaptive_resolve makes the frame from the three.  The planes live in uncached memory
// and are accessed with agent-scope atomics only, as the sums are.
struct SumsParams {
    AParams A;               // the frame's layout and sums; L, first_chunk: the chunk k_map_fold folds in
    float* qacc;
    uint32_t* nsamp;         // [nslots] n_p: the samples the slot's sums hold once the range under way is folded (padding slots: 0)
};
// crt_render_adaptive: a pass renders the slots of `list`
struct AdaptiveParams {
    SumsParams sums;
    uint32_t* list;          // [count] the slots that go on, in any order (k_adaptive_select)
    unsigned int* count;
    uint32_t n;              // the samples a slot that is still active has: nsamp[slot] == n
    uint32_t ns_pass;        // k_adaptive_select: the samples of the pass that follows, min(step_samples, spp - n)
    float threshold, mean_floor;
};
// crt_render_map, crt_sample_plan, crt_render_planned.  The histogram and the cursors live in uncached memory too.
struct MapParams {
    SumsParams sums;
    const uint32_t* map;     // k_map_prepare: the caller's counts, one per pixel of the W x H image (row-major) or, map_per_slot, per pixel slot
    uint32_t map_per_slot;
    uint32_t sample_begin;   // k_map_prepare: the samples every pixel has already
    unsigned int* hist;      // k_map_prepare: [spp + 1] slots per value of n_p, zeroed before the launch
    unsigned int* cursor;    // k_map_items: [spp] where the next entry of sample s goes in its chunk's list
    uint32_t* item_list;     // k_map_items: n_items entries
    uint32_t n_items;
    uint32_t s0, ns;         // k_map_items: the chunk's samples [s0, s0 + ns)
    uint32_t n;              // k_sample_plan: samples in the sums
    float threshold, mean_floor;
    uint32_t* out_map;       // k_sample_plan: in the frame's output layout
};

} // namespace crtk
#endif
