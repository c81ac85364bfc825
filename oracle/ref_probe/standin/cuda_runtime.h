/*
 * oracle/ref_probe/standin/cuda_runtime.h -- TEST INFRASTRUCTURE.
 *
 * A host-only stand-in for the slice of the CUDA runtime interface the
 * reference's headers use, written from CUDA's documented interface, so that
 * plain g++ can compile those headers from where they lie and run them on the
 * CPU (oracle/ref_probe/path_probe.cpp).  "Device" memory is the heap, the
 * execution-space qualifiers are empty, and the built-in index variables are
 * ordinary globals the probe sets per pixel.
 */
#ifndef REF_PROBE_STANDIN_CUDA_RUNTIME_H
#define REF_PROBE_STANDIN_CUDA_RUNTIME_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>

#define __host__
#define __device__
#define __global__

typedef int cudaError_t;
enum { cudaSuccess = 0, cudaErrorMemoryAllocation = 2 };
enum cudaMemcpyKind { cudaMemcpyHostToHost = 0, cudaMemcpyHostToDevice = 1, cudaMemcpyDeviceToHost = 2, cudaMemcpyDeviceToDevice = 3 };

inline cudaError_t cudaMalloc(void** p, size_t n)
{
    *p = std::malloc(n ? n : 1);
    return *p ? cudaSuccess : cudaErrorMemoryAllocation;
}
inline cudaError_t cudaMemcpy(void* dst, const void* src, size_t n, cudaMemcpyKind)
{
    std::memcpy(dst, src, n);
    return cudaSuccess;
}
inline cudaError_t cudaFree(void* p)
{
    std::free(p);
    return cudaSuccess;
}
inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
inline cudaError_t cudaGetLastError() { return cudaSuccess; }
inline const char* cudaGetErrorString(cudaError_t e) { return e == cudaSuccess ? "no error" : "stand-in allocation failure"; }

struct uchar3 { unsigned char x, y, z; };
inline uchar3 make_uchar3(unsigned char x, unsigned char y, unsigned char z) { return uchar3{x, y, z}; }

struct uint3 { unsigned int x, y, z; };
struct dim3 {
    unsigned int x, y, z;
    dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};
/* one definition each, in the probe's translation unit */
extern uint3 blockIdx, threadIdx;
extern dim3 blockDim, gridDim;

/* Two spellings the reference takes from MSVC's <cmath>, which libstdc++ does not offer in namespace std. */
namespace std {
inline float atan2f(float y, float x) { return ::atan2f(y, x); }
inline float modff(float x, float* ip) { return ::modff(x, ip); }
}

#endif
