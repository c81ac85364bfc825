// cudaraytracing_amd/csrc/crt_filter_host.h -- what the host side of every image-space filter does around its own checks and launches
// (crt_denoise.hip, crt_nlm.hip, crt_modulate.hip, crt_temporal.hip, crt_variance_estimate.hip): the size and scratch checks, the launch
// between two events with its optional counters, and the host-buffer form's device copies.  Host code only: no kernel, and no device
// header includes it.
#ifndef CRT_FILTER_HOST_H
#define CRT_FILTER_HOST_H
#include "crt_internal.h"

#include <cstring>
#include <deque>
#include <string>
#include <vector>

namespace crtk {

const uint32_t kMaxSide = 1u << 24;
inline bool sigma_ok(float s) { return s > 0.0f; } // (false for NaN)

// The checks below return CRT_OK or the entry point's error return (w: the entry point's name); a filter's check function calls each
// where its test stands among the filter's own, since the order decides which message a call with several faults gets.
inline int size_positive(const std::string& w, uint32_t width, uint32_t height)
{
    if (width == 0 || height == 0) return fail(CRT_ERR_INVALID_ARG, w + ": width and height must be positive");
    return CRT_OK;
}
inline int sides_supported(const std::string& w, uint32_t width, uint32_t height)
{
    if (width > kMaxSide || height > kMaxSide) return fail(CRT_ERR_UNSUPPORTED, w + ": a side longer than 2^24 pixels");
    return CRT_OK;
}
// (tile_w x tile_h: the pixels of a thread block of the filter's launch)
inline int size_supported(const std::string& w, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h)
{
    const int rc = sides_supported(w, width, height);
    if (rc != CRT_OK) return rc;
    if ((uint64_t)((width + tile_w - 1) / tile_w) * ((height + tile_h - 1) / tile_h) > 0x7fffffffull)
        return fail(CRT_ERR_UNSUPPORTED, w + ": more than 2^31 thread blocks");
    return CRT_OK;
}
// The caller's scratch buffer (sizing_call: the entry point that tells its size)
inline int scratch_ok(const std::string& w, const void* d_scratch, uint64_t scratch_bytes, uint64_t needed, const char* sizing_call)
{
    if (!d_scratch) return fail(CRT_ERR_INVALID_ARG, w + ": null scratch buffer");
    if (scratch_bytes < needed) return fail(CRT_ERR_INVALID_ARG, w + ": scratch buffer too small (" + sizing_call + ")");
    if ((uintptr_t)d_scratch % sizeof(float4) != 0) return fail(CRT_ERR_INVALID_ARG, w + ": scratch buffer not 16-byte aligned");
    return CRT_OK;
}

struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~EventPair()
    {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// A filter's launches on the stream: enqueue(d_count) launches them (and may HIP_CHECK).  With an `info`, between two events: *info is
// zeroed and its total_ms filled once the stream has run dry (the filter's own fields: the caller's, after CRT_OK).  n_counts > 0: that
// many device counters, zeroed on the stream before the first event, in `counts` after the second; d_count is null without an info.
template <class Info, class Enqueue>
int timed_launch(const std::string& who, int device, hipStream_t st, Info* info, unsigned long long* counts, size_t n_counts, Enqueue enqueue)
{
    if (device < 0) return fail(CRT_ERR_INVALID_ARG, who + ": device index out of range");
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(device));
        DevBuf<unsigned long long> d_count;
        EventPair ev;
        if (info) {
            if (n_counts) {
                d_count.alloc(n_counts);
                HIP_CHECK(hipMemsetAsync(d_count.p, 0, n_counts * sizeof(unsigned long long), st));
            }
            HIP_CHECK(hipEventCreate(&ev.e0));
            HIP_CHECK(hipEventCreate(&ev.e1));
            HIP_CHECK(hipEventRecord(ev.e0, st));
        }
        enqueue(d_count.p);
        HIP_CHECK(hipGetLastError());
        if (info) {
            HIP_CHECK(hipEventRecord(ev.e1, st));
            if (n_counts) HIP_CHECK(hipMemcpyAsync(counts, d_count.p, n_counts * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            std::memset(info, 0, sizeof(*info));
            HIP_CHECK(hipEventElapsedTime(&info->total_ms, ev.e0, ev.e1));
        }
        return CRT_OK;
    });
}
template <class Info, class Enqueue> int timed_launch(const std::string& who, int device, hipStream_t st, Info* info, Enqueue enqueue)
{
    return timed_launch(who, device, st, info, nullptr, 0, [&](unsigned long long*) { enqueue(); });
}

// The device copies of a host-buffer form.  A null host pointer gives a null device pointer and allocates nothing.
class HostCopies {
    struct Out { DevBuf<char>* dev; void* host; size_t bytes; };
    std::deque<DevBuf<char>> bufs_; // (a deque: the buffers stay where they are)
    std::vector<Out> outs_;
    template <typename T> T* fresh(size_t count)
    {
        bufs_.emplace_back();
        bufs_.back().alloc(count * sizeof(T));
        return (T*)bufs_.back().p;
    }

public:
    template <typename T> T* in(const T* h, size_t count)
    {
        if (!h) return nullptr;
        bufs_.emplace_back();
        return (T*)bufs_.back().upload((const char*)h, count * sizeof(T));
    }
    template <typename T> T* out(T* h, size_t count) // copied to h by download()
    {
        if (!h) return nullptr;
        T* d = fresh<T>(count);
        outs_.push_back({&bufs_.back(), h, count * sizeof(T)});
        return d;
    }
    template <typename T> T* scratch(size_t count) { return fresh<T>(count); }
    void download() const
    {
        for (const Out& o : outs_) o.dev->download((char*)o.host, o.bytes);
    }
};

// A host-buffer form (the caller has checked its arguments): body(copies) makes the device copies and runs the device implementation
// on the null stream; after CRT_OK from it, the device is drained and the outputs are copied back.
template <class Body> int host_form(const std::string& who, int device, Body body)
{
    if (device < 0) return fail(CRT_ERR_INVALID_ARG, who + ": device index out of range");
    return hip_guard([&]() -> int {
        HIP_CHECK(hipSetDevice(device));
        HostCopies copies;
        const int rc = body(copies);
        if (rc != CRT_OK) return rc;
        HIP_CHECK(hipDeviceSynchronize());
        copies.download();
        return CRT_OK;
    });
}

} // namespace crtk
#endif
