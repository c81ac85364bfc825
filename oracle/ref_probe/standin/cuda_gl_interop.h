/*
 * oracle/ref_probe/standin/cuda_gl_interop.h -- TEST INFRASTRUCTURE.
 *
 * The part of the reference the probe compiles (everything before its Render
 * class) names nothing of the OpenGL interoperability interface; the include
 * only has to resolve.
 */
#ifndef REF_PROBE_STANDIN_CUDA_GL_INTEROP_H
#define REF_PROBE_STANDIN_CUDA_GL_INTEROP_H
#include "cuda_runtime.h"
struct cudaGraphicsResource;
#endif
