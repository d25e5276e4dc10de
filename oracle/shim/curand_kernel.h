/*
 * curand_kernel.h — TEST INFRASTRUCTURE.  Our own name-only stand-in for the vendor SDK header of that name, found through
 * -Ishim by oracle/ref_shade.cpp alone.  The reference's random_utils.h and materials.h include it but use nothing of cuRAND;
 * all they need is the CUDA dialect (__host__ __device__) and the type name of a texture handle.  This file defines no
 * behaviour: it includes ROCm's runtime header and the sibling alias header, which names that type.
 */
#pragma once
#include <hip/hip_runtime.h>
#include "cuda_runtime.h"
