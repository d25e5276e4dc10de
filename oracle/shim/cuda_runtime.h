/*
 * cuda_runtime.h — TEST INFRASTRUCTURE.  Our own name-only stand-in for the vendor SDK header of that name, found through
 * -Ishim by oracle/ref_shade.cpp alone, so that the reference's camera.cuh and src/camera.cu compile host-only
 * (`hipcc -x hip --cuda-host-only`).  It defines no behaviour: every line is an alias of a CUDA runtime name to ROCm's name
 * for the same thing, or the #include of a header this image has.  The harness never calls any of the aliased functions (it
 * runs the reference's CPU path only); the hip symbols are linked and never reached.
 *
 * <math.h> is here because the vendor's header includes it too (through its crt/math_functions.h), and the reference depends
 * on that: with the C++ library's <math.h> the float overloads of std:: are visible in the global namespace, so the
 * reference's unqualified `exp(-absorbance.x() * distance)` (include/materials.h:117) and `tan(theta / 2)`
 * (src/camera.cu:174) are expf and tanf, as they are in the reference's own build.  With <cmath> alone they would bind to the
 * C library's double functions and differ from that build in the last bit now and then (docs/LOG.md).
 */
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

using cudaTextureObject_t = hipTextureObject_t;
using cudaError_t = hipError_t;
using cudaEvent_t = hipEvent_t;
#define cudaSuccess hipSuccess
#define cudaMemcpyHostToDevice hipMemcpyHostToDevice
#define cudaMemcpyDeviceToHost hipMemcpyDeviceToHost
#define cudaDeviceReset hipDeviceReset
#define cudaDeviceSynchronize hipDeviceSynchronize
#define cudaGetLastError hipGetLastError
#define cudaMalloc hipMalloc
#define cudaFree hipFree
#define cudaMemcpy hipMemcpy
#define cudaMemcpyToSymbol(symbol, ...) hipMemcpyToSymbol(HIP_SYMBOL(symbol), __VA_ARGS__)
#define cudaGetSymbolAddress(pointer, symbol) hipGetSymbolAddress((pointer), HIP_SYMBOL(symbol))
#define cudaEventCreate hipEventCreate
#define cudaEventRecord hipEventRecord
#define cudaEventSynchronize hipEventSynchronize
#define cudaEventElapsedTime hipEventElapsedTime
#define cudaEventDestroy hipEventDestroy
