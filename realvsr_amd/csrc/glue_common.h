// glue_common.h -- what the memory-bound ("glue") translation units share: misc_kernels.hip, train_kernels.hip, gan_kernels.hip,
// ca_kernels.hip and conv3d_kernels.hip.  Macros and __device__ __forceinline__ helpers only; no kernel lives here.
#pragma once
#include "rvsr_common.h"

// one thread per element, 256 threads per workgroup, at most 4096 workgroups that stride over the rest
#define GRID_FOR(n) dim3((unsigned)(((n) + 255) / 256 > 4096 ? 4096 : ((n) + 255) / 256))
#define LOOP(i, n) for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (size_t)gridDim.x * blockDim.x)

// after a launch: CHECK_LAUNCH fails the entry point on a launch error and otherwise goes on (more launches follow);
// RETURN_LAUNCH is the last statement of an entry point
#define CHECK_LAUNCH(name)                                                                        \
    do {                                                                                          \
        hipError_t e_ = hipGetLastError();                                                        \
        if (e_ != hipSuccess) FAIL(RVSR_ERR_LAUNCH, name " launch: %s", hipGetErrorString(e_));   \
    } while (0)
#define RETURN_LAUNCH(name)  \
    do {                     \
        CHECK_LAUNCH(name);  \
        return RVSR_OK;      \
    } while (0)

__device__ __forceinline__ float wave_sum(float v) {   // butterfly: every lane ends with the same sum, in one fixed order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// dst[0] = the sum of v over a workgroup of 256 threads (four waves): butterfly inside a wave, then LDS across the waves, in one
// fixed order.  Thread 0 stores.
__device__ __forceinline__ void block_sum4_to(float v, float* dst) {
    __shared__ float red[4];
    const float w = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) dst[0] = (red[0] + red[1]) + (red[2] + red[3]);
}
