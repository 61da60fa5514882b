// timeline.h -- s_memtime stamps of developer variant builds: the one timeline mechanism of the library.
//
// A kernel marks a point with RVSR_STAMP(cond, index): the threads for which `cond` holds write the shader clock into slot `index` of one
// __device__ buffer.  Without -DRVSR_TIMELINE the macro is empty and the product carries neither the buffer nor the reader.  A variant build
// compiles ONE source file with the flag and links it with the product's other objects,
//     tools/build_variant.sh tl conv2_kernels.hip -DRVSR_TIMELINE          ->  realvsr_amd/csrc/librealvsr_tl.so
// so the buffer and its reader exist once per library; the tool of that file (tools/*_timeline.py) loads the variant through RVSR_SO, runs
// the kernel and reads the slots back with rvsr_timeline_read.  The slot numbers of a kernel are an enum next to it; its tool repeats them.
// `cond` picks one workgroup and one thread (or lane 0 of each wave): every slot has one writer.
#pragma once

#ifdef RVSR_TIMELINE
#include <hip/hip_runtime.h>
#define RVSR_TIMELINE_SLOTS 512
__device__ unsigned long long rvsr_timeline[RVSR_TIMELINE_SLOTS];
// the first min(capacity, RVSR_TIMELINE_SLOTS) slots into `out` (host memory); returns the hipError_t of the copy (0: fine).  A developer
// symbol of variant builds: not part of include/realvsr_hip.h.
extern "C" int rvsr_timeline_read(unsigned long long* out, int capacity) {
    const int n = capacity < RVSR_TIMELINE_SLOTS ? capacity : RVSR_TIMELINE_SLOTS;
    if (!out || n <= 0) return (int)hipErrorInvalidValue;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(rvsr_timeline), sizeof(unsigned long long) * (size_t)n);
}
#define RVSR_STAMP(cond, index) do { if (cond) rvsr_timeline[(index)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define RVSR_STAMP(cond, index) do { (void)sizeof((cond) && (index)); } while (0)
#endif
