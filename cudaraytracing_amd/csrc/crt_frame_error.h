// cudaraytracing_amd/csrc/crt_frame_error.h -- the device text of crt_frame_error (contract: include/crt.h; kernels, scratch, entry
// points and the loop of crt_render_until: crt_frame_error.hip): the error of the frame in flight, reduced over the shard's valid
// pixel slots into one crt_frame_error_info.  Two launches and nothing between them but the kernel boundary -- no atomic, no zeroing
// pass, no fence between blocks:
//   blocks   one thread per slot in slot_grid's blocks of 256: the slot's criterion (frame_error_slot), the fp64 tree over each wave
//            (steps 1 and 2 of the contract's summation order) and a ballot and popcount per count; the waves' partials meet in LDS
//            and the block's last wave writes the block's partials (step 3) to the scratch planes, with plain vector stores
//   finish   one wave per quantity (kFeQuantities blocks of 64): lane l adds the blocks' partials l, l + 64, ... in ascending order
//            (step 4), the tree folds the 64 lane sums (step 5), lane 0 writes the quantity's field of the struct
// Like crt_aov_ao.h this file includes nothing, so that tools/frame_error_host_check.cpp can compile this very text for the host behind
// tools/host_device.h's stand-ins for what it takes from outside: AParams, slot_pixel, acc_load3, variance_of3 (crt_stages.h), F3
// (crt_device.h), crt_frame_error_info (include/crt.h), __shfl_down on 8-byte values, __ballot, __popcll, __shared__, __syncthreads.
#ifndef CRT_FRAME_ERROR_H
#define CRT_FRAME_ERROR_H

namespace crtk {

// The quantities a block leaves a partial of: counts 0 .. 15 = hist[], then nan_pixels, pixels and above; sums 0 and 1 = v and m
const uint32_t kFeCounts = 19, kFeNan = 16, kFePixels = 17, kFeAbove = 18, kFeSums = 2, kFeQuantities = kFeCounts + kFeSums;
const uint32_t kFeNotAPixel = 17; // frame_error_slot's bin of a slot that counts for nothing (kFeNan: a NaN slot)

struct FrameErrorParams {
    AParams A;               // the frame's layout and the sum c (A.accum)
    const float* qacc;       // the sum of squares q
    uint32_t n;              // the samples the sums hold
    float threshold, mean_floor;
    uint32_t n_blocks;       // slot_grid(A).x
    double* part_sum;        // [kFeSums][n_blocks] the blocks' partials of v and m
    uint32_t* part_cnt;      // [kFeCounts][n_blocks] and of the counts (at most 256 each)
    crt_frame_error_info* out;
};

// stop_criterion's sibling (crt_stages.h: that one stays as it is, so that k_adaptive_select and k_sample_plan keep their listings):
// the same operations in the same order, and the channel-summed mean m beside (v, tt)
struct StopCriterionM {
    float v, tt, m;
};
__device__ __forceinline__ StopCriterionM stop_criterion_m(const AParams& A, const float* qacc, const uint32_t slot, const uint32_t n, const float threshold,
                                                           const float mean_floor)
{
    const float fn = (float)n, fs = (float)A.spp;
    const float r = fs / fn, rr = r * r;
    const F3 c = acc_load3(A.accum, A.nslots, slot);
    const F3 var = variance_of3(c, acc_load3(qacc, A.nslots, slot), fn, rr);
    const F3 p = f3(c.x * r, c.y * r, c.z * r);
    const float v = (var.x + var.y) + var.z, m = (p.x + p.y) + p.z;
    const float t = threshold * (m + mean_floor);
    StopCriterionM k;
    k.v = v; k.tt = t * t; k.m = m;
    return k;
}

// What a slot adds: its bin (0 .. 15: hist; kFeNan; kFeNotAPixel: padding, or beyond the shard's slots) and (double)v, (double)m --
// +0.0 both unless the bin is one of hist's
struct FrameErrorSlot {
    uint32_t bin;
    double v, m;
};
__device__ __forceinline__ FrameErrorSlot frame_error_slot(const FrameErrorParams& D, const uint32_t slot)
{
    FrameErrorSlot s;
    s.bin = kFeNotAPixel; s.v = 0.0; s.m = 0.0;
    if (slot >= D.A.nslots || !slot_pixel(D.A, slot).valid) return s;
    const StopCriterionM k = stop_criterion_m(D.A, D.qacc, slot, D.n, D.threshold, D.mean_floor);
    if (!(k.v == k.v) || !(k.tt == k.tt)) { s.bin = kFeNan; return s; }
    uint32_t b = 0;
#pragma unroll
    for (uint32_t j = 0; j < 15u; j++) b += k.v > k.tt * __uint_as_float((113u + 2u * j) << 23) ? 1u : 0u; // 4^(j - 7) = 2^(2 j - 14)
    s.bin = b; s.v = (double)k.v; s.m = (double)k.m;
    return s;
}

// Step 2 of the summation order over the 64 lanes of a wave: lane 0 returns the group's sum (lane t < s holds the contract's x[t]
// after step s: what it takes from lane t + s < 2 s is that lane's value after the step before).  T: double, or unsigned long long
// for the counts, whose order does not matter.
template <class T> __device__ __forceinline__ T frame_error_tree(T x)
{
#pragma unroll
    for (uint32_t s = 32u; s >= 1u; s >>= 1) x += __shfl_down(x, s);
    return x;
}

// ---- blocks: 256 threads, every one of them takes part in the cross-lane operations ----
__device__ __forceinline__ void frame_error_block(const FrameErrorParams& D)
{
    __shared__ double w_sum[kFeSums][4];
    __shared__ uint32_t w_cnt[kFeCounts][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const FrameErrorSlot s = frame_error_slot(D, blockIdx.x * 256u + threadIdx.x);
    const double wv = frame_error_tree(s.v), wm = frame_error_tree(s.m);
    if (lane == 0u) { w_sum[0][wave] = wv; w_sum[1][wave] = wm; }
#pragma unroll
    for (uint32_t k = 0; k < kFeCounts; k++) {
        const bool in = k < 16u ? s.bin == k : k == kFeNan ? s.bin == kFeNan : k == kFePixels ? s.bin != kFeNotAPixel : (s.bin >= 8u && s.bin <= kFeNan);
        const uint32_t c = (uint32_t)__popcll(__ballot(in));
        if (lane == 0u) w_cnt[k][wave] = c;
    }
    __syncthreads();
    // the block's last wave: one lane per quantity (on the host a block's waves run one after another, so the last one finds the others' partials too)
    if (wave != 3u) return;
    if (lane < kFeCounts) D.part_cnt[(size_t)lane * D.n_blocks + blockIdx.x] = (w_cnt[lane][0] + w_cnt[lane][1]) + (w_cnt[lane][2] + w_cnt[lane][3]);
    else if (lane < kFeQuantities) {
        const uint32_t q = lane - kFeCounts;
        D.part_sum[(size_t)q * D.n_blocks + blockIdx.x] = ((w_sum[q][0] + w_sum[q][1]) + w_sum[q][2]) + w_sum[q][3]; // step 3
    }
}

// ---- finish: one wave of 64 per quantity; blockIdx.x names it ----
__device__ __forceinline__ void frame_error_finish(const FrameErrorParams& D)
{
    const uint32_t lane = threadIdx.x & 63u, k = blockIdx.x;
    crt_frame_error_info* const o = D.out;
    if (k >= kFeCounts) {
        const double* P = D.part_sum + (size_t)(k - kFeCounts) * D.n_blocks;
        double a = 0.0;
#pragma unroll 32
        for (uint32_t i = lane; i < D.n_blocks; i += 64u) a += P[i]; // step 4
        a = frame_error_tree(a);                                     // step 5
        if (lane == 0u) { if (k == kFeCounts) o->sum_variance = a; else o->sum_mean = a; }
        return;
    }
    const uint32_t* P = D.part_cnt + (size_t)k * D.n_blocks;
    unsigned long long a = 0ull;
#pragma unroll 32
    for (uint32_t i = lane; i < D.n_blocks; i += 64u) a += P[i];
    a = frame_error_tree(a);
    if (lane != 0u) return;
    if (k < 16u) o->hist[k] = a;
    else if (k == kFeNan) o->nan_pixels = a;
    else if (k == kFeAbove) o->above = a;
    else { o->pixels = a; o->samples_done = D.n; o->spp = D.A.spp; }
}

// crt_frame_error.hip (the host check states its own two kernels around the same bodies)
void launch_frame_error(const FrameErrorParams& D, hipStream_t st);

} // namespace crtk
#endif
