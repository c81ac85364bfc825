// cudaraytracing_amd/csrc/crt_frame.hip -- the kernels around the render kernels: k_accumulate (per pixel c += L_k / spp in sample order, tone map:
// include/Render.cuh:348-350; k_accumulate_var: also the sum of squares behind crt_variance, read out by k_variance; k_accumulate_half: also the half sums behind crt_half_buffers, read out by k_half_buffers), k_preview, and the kernels behind crt_intersect's ray upload and the crt_device_* self-tests.
// The stages these share with crt_adaptive.hip -- slot to pixel to output index, the three-plane sums, the sample fold, the output write -- are in crt_stages.h.
#include "crt_internal.h"

namespace crtk {

// VAR (CRT_FLAG_VARIANCE): beside c, the sum of squares q of the same quotients (fold_samples), carried across chunks in the planes of
// `qacc` as c is in A.accum; the last chunk then leaves c and q on the handle for crt_variance.  Without VAR the code is what it was
// before the flag existed.
template <bool VAR> __device__ __forceinline__ void accumulate(const AParams& A, float* qacc)
{
    uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= A.nslots) return;
    const SlotPixel px = slot_pixel(A, slot);
    F3 c = f3(0.0f, 0.0f, 0.0f);
    F3 q = f3(0.0f, 0.0f, 0.0f);
    if (px.valid) {
        if (!A.first_chunk) c = acc_load3(A.accum, A.nslots, slot);
        if (VAR && !A.first_chunk) q = acc_load3(qacc, A.nslots, slot);
        fold_samples<VAR>(A, slot, c, q);
        if (VAR) acc_store3(qacc, A.nslots, slot, q);
        if (VAR || !A.last_chunk) {
            acc_store3(A.accum, A.nslots, slot, c);
            if (!A.last_chunk) return;
        }
    } else if (!px.out || !A.last_chunk) {
        return;
    }
    write_color(A, px.o, px.valid, c);
}

__global__ __launch_bounds__(256) void k_accumulate(const AParams A) { accumulate<false>(A, nullptr); }
__global__ __launch_bounds__(256) void k_accumulate_var(const AParams A, float* const qacc) { accumulate<true>(A, qacc); }

// CRT_FLAG_HALF_BUFFERS: k_accumulate_var, and the sums of the even and of the odd samples (fold_samples_half) carried in the six planes
// of `hacc` -- h0 in planes 0 .. 2, h1 in 3 .. 5 -- as q is in qacc.  parity: of the chunk's first sample in the frame.
__global__ __launch_bounds__(256) void k_accumulate_half(const AParams A, float* const qacc, float* const hacc, const uint32_t parity)
{
    uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= A.nslots) return;
    const SlotPixel px = slot_pixel(A, slot);
    F3 c = f3(0.0f, 0.0f, 0.0f);
    if (px.valid) {
        F3 q = f3(0.0f, 0.0f, 0.0f), h0 = f3(0.0f, 0.0f, 0.0f), h1 = f3(0.0f, 0.0f, 0.0f);
        float* const hacc1 = hacc + 3ull * A.nslots;
        if (!A.first_chunk) {
            c = acc_load3(A.accum, A.nslots, slot); q = acc_load3(qacc, A.nslots, slot);
            h0 = acc_load3(hacc, A.nslots, slot); h1 = acc_load3(hacc1, A.nslots, slot);
        }
        fold_samples_half(A, slot, A.chunk_samples, parity, c, q, h0, h1);
        acc_store3(qacc, A.nslots, slot, q);
        acc_store3(hacc, A.nslots, slot, h0); acc_store3(hacc1, A.nslots, slot, h1);
        acc_store3(A.accum, A.nslots, slot, c);
        if (!A.last_chunk) return;
    } else if (!px.out || !A.last_chunk) {
        return;
    }
    write_color(A, px.o, px.valid, c);
}

// crt_half_buffers (contract: include/crt.h): the two half means from the handle's sums h0 and h1, scale_a = S / n_a, scale_b = S / n_b,
// in the frame's layout (padding slots of a tiled shard +0).  Reads the sums only; either output may be null.
__global__ __launch_bounds__(256) void k_half_buffers(const AParams A, const float* const hacc, float* const out_a, float* const out_b, const float scale_a,
                                                      const float scale_b)
{
    uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= A.nslots) return;
    const SlotPixel px = slot_pixel(A, slot);
    if (!px.out) return;
    F3 a = f3(0.0f, 0.0f, 0.0f), b = f3(0.0f, 0.0f, 0.0f);
    if (px.valid) {
        const F3 h0 = acc_load3(hacc, A.nslots, slot), h1 = acc_load3(hacc + 3ull * A.nslots, A.nslots, slot);
        a = f3(h0.x * scale_a, h0.y * scale_a, h0.z * scale_a);
        b = f3(h1.x * scale_b, h1.y * scale_b, h1.z * scale_b);
    }
    if (out_a) { out_a[px.o * 3 + 0] = a.x; out_a[px.o * 3 + 1] = a.y; out_a[px.o * 3 + 2] = a.z; }
    if (out_b) { out_b[px.o * 3 + 0] = b.x; out_b[px.o * 3 + 1] = b.y; out_b[px.o * 3 + 2] = b.z; }
}

// crt_variance (contract: include/crt.h): the variance of the mean from the handle's sums c (A.accum) and q, n = samples so far, written
// to A.out_mean in the frame's layout (padding slots of a tiled shard +0).  Reads the sums only.
__global__ __launch_bounds__(256) void k_variance(const AParams A, const float* const qacc, const float fn, const float fs)
{
    uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= A.nslots) return;
    const SlotPixel px = slot_pixel(A, slot);
    if (!px.out) return;
    F3 v = f3(0.0f, 0.0f, 0.0f);
    if (px.valid) {
        const float r = fs / fn;
        v = variance_of3(acc_load3(A.accum, A.nslots, slot), acc_load3(qacc, A.nslots, slot), fn, r * r);
    }
    A.out_mean[px.o * 3 + 0] = v.x; A.out_mean[px.o * 3 + 1] = v.y; A.out_mean[px.o * 3 + 2] = v.z;
}

// crt_preview: the frame a progressive render would show now.  The accumulator holds sum_{k < done} L_k / spp (Render.cuh:348
// with the samples so far); its estimate of the mean is that sum * spp / done.  Reads the accumulator only, with plain loads.
__global__ __launch_bounds__(256) void k_preview(const AParams A, const float scale)
{
    uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= A.nslots) return;
    const SlotPixel px = slot_pixel(A, slot);
    if (!px.out) return;
    F3 c = f3(0.0f, 0.0f, 0.0f);
    if (px.valid) c = f3(A.accum[slot] * scale, A.accum[A.nslots + slot] * scale, A.accum[2ull * A.nslots + slot] * scale);
    write_color(A, px.o, px.valid, c);
}

// ------------------------------------------------------------ test kernels --
// crt_intersect: loads n host rays into the first n pool slots (direction normalised as Ray's
// constructor does, Ray.cuh:12-13) so that the production trace kernel answers them.
// limits != nullptr: the rays are visibility rays (blocked(), Render.cuh:19-27) with these t_to_light values.
__global__ __launch_bounds__(256) void k_fill_rays(Pool pl, uint32_t n, const float* o, const float* d, const bool raw_dir, const float* limits)
{
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    F3 dir = f3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    if (!raw_dir) dir = unit3(dir);
    pl.ro[i] = make_float4(o[3 * i], o[3 * i + 1], o[3 * i + 2], limits ? limits[i] : 0.0f);
    pl.rd[i] = make_float4(dir.x, dir.y, dir.z, __uint_as_float((uint32_t)(limits ? RAY_SHADOW : RAY_CLOSEST)));
    pl.res[i] = make_float2(FLT_MAX, __int_as_float(-1));
}

__global__ void k_math(int fn, uint32_t n, const float* a, const float* b, float* out)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x = a[i], y = b ? b[i] : 0.0f, r;
    switch (fn) {
    case 0: r = det_sinf(x); break;
    case 1: r = det_cosf(x); break;
    case 2: r = det_tanf(x); break;
    case 3: r = det_acosf(x); break;
    case 4: r = det_atan2f(x, y); break;
    case 5: r = det_expf(x); break;
    case 6: r = det_log10f(x); break;
    case 7: r = det_powf(x, y); break;
    case 8: r = rng_uniform(__float_as_uint(x)); break;
    case 9: { float s, c; det_sincosf(x, &s, &c); r = s; break; }
    case 10: { float s, c; det_sincosf(x, &s, &c); r = c; break; }
    case 11: r = quot3_exact(f3(x, x, x), y, false).y; break;              // the short exact division against x / y (tests)
    case 12: r = quot3_exact(f3(x, 0.0f, -0.0f), y, true).x; break;        // ... in the form unit3 uses
    default: r = qnan();
    }
    out[i] = r;
}
// crt_device_rcp_check: every fp32 bit pattern through rcp_short and through the division
__global__ void k_rcp_check(unsigned long long* counts)
{
    const unsigned long long tid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    unsigned int bad_in = 0, bad_out = 0;
    for (unsigned long long b = tid; b < (1ull << 32); b += stride) {
        const float x = __uint_as_float((uint32_t)b);
        const float ref = 1.0f / x, got = rcp_short(x);
        const bool same = __float_as_uint(ref) == __float_as_uint(got) || (ref != ref && got != got);
        if (!same) { if (rcp_short_ok(x)) bad_in++; else bad_out++; }
    }
    bad_in = wave_sum(bad_in); bad_out = wave_sum(bad_out);
    if ((threadIdx.x & 63) == 0 && (bad_in | bad_out)) { atomicAdd(&counts[0], (unsigned long long)bad_in); atomicAdd(&counts[1], (unsigned long long)bad_out); }
}

__global__ void k_philox(uint32_t n, const uint32_t* ctr, const uint32_t* key, uint32_t* out)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    U4 c;
    c.x = ctr[4 * i]; c.y = ctr[4 * i + 1]; c.z = ctr[4 * i + 2]; c.w = ctr[4 * i + 3];
    U4 r = philox4x32_10(c, key[2 * i], key[2 * i + 1]);
    out[4 * i] = r.x; out[4 * i + 1] = r.y; out[4 * i + 2] = r.z; out[4 * i + 3] = r.w;
}


// ---- exported to crt_render.hip ----
void launch_accumulate(const AParams& A, hipStream_t st) { hipLaunchKernelGGL(k_accumulate, dim3((A.nslots + 255) / 256), dim3(256), 0, st, A); }
void launch_accumulate_var(const AParams& A, float* qacc, hipStream_t st) { hipLaunchKernelGGL(k_accumulate_var, dim3((A.nslots + 255) / 256), dim3(256), 0, st, A, qacc); }
void launch_accumulate_half(const AParams& A, float* qacc, float* hacc, uint32_t parity, hipStream_t st)
{
    hipLaunchKernelGGL(k_accumulate_half, dim3((A.nslots + 255) / 256), dim3(256), 0, st, A, qacc, hacc, parity);
}
void launch_half_buffers(const AParams& A, const float* hacc, float* out_a, float* out_b, float scale_a, float scale_b, hipStream_t st)
{
    hipLaunchKernelGGL(k_half_buffers, dim3((A.nslots + 255) / 256), dim3(256), 0, st, A, hacc, out_a, out_b, scale_a, scale_b);
}
void launch_variance(const AParams& A, const float* qacc, float fn, float fs, hipStream_t st)
{
    hipLaunchKernelGGL(k_variance, dim3((A.nslots + 255) / 256), dim3(256), 0, st, A, qacc, fn, fs);
}
void launch_preview(const AParams& A, float scale, hipStream_t st) { hipLaunchKernelGGL(k_preview, dim3((A.nslots + 255) / 256), dim3(256), 0, st, A, scale); }
void launch_fill_rays(const Pool& pool, uint32_t n, const float* o, const float* d, bool raw_dir, const float* limits)
{
    hipLaunchKernelGGL(k_fill_rays, dim3((n + 255) / 256), dim3(256), 0, 0, pool, n, o, d, raw_dir, limits);
}
void launch_math(int fn, uint32_t n, const float* a, const float* b, float* out) { hipLaunchKernelGGL(k_math, dim3((n + 255) / 256), dim3(256), 0, 0, fn, n, a, b, out); }
void launch_philox(uint32_t n, const uint32_t* ctr, const uint32_t* key, uint32_t* out) { hipLaunchKernelGGL(k_philox, dim3((n + 255) / 256), dim3(256), 0, 0, n, ctr, key, out); }
void launch_rcp_check(unsigned long long* counts) { hipLaunchKernelGGL(k_rcp_check, dim3(256 * 32), dim3(256), 0, 0, counts); }

} // namespace crtk
