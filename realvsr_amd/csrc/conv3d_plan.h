// conv3d_plan.h -- which channel counts the temporal convolution (conv3d_kernels.hip, tconv3) takes, how its work is cut and which access
// width it and the PReLU kernels may use.
//
// In the spirit of conv_plan.h and ca_plan.h: every eligibility and slicing rule of the FSTRN kernels is written here and nowhere else,
// as pure host code -- no HIP call, no pointer dereferenced (addresses are only tested for alignment), no side effect.  rvsr_tconv3_plan
// and rvsr_prelu_plan export it.
#pragma once
#include "rvsr_common.h"

#define TC_MAX_C 64        // channels in and out: the weight image (3 x Co x Ci as hi | lo bf16, or as f32) stays in LDS: 48 KB at 64 x 64
#define TC_WG 256          // 4 waves
#define TC_WAVE_PIX 32     // one 32-column MFMA tile of pixels per wave
#define TC_TILE 128        // pixels of a work item: 4 waves x 32
#define TC_SLOTS 1024      // workgroups launched at most (256 CUs x 2 resident x 2); a workgroup walks several items with one weight image

struct TcPlan {
    int rc;            // RVSR_OK, or what the entry returns without launching anything
    const char* msg;   // text of a refusal
    int ks, mt;        // k-steps of 16 input channels, m-tiles of 32 output channels
    int tiles;         // work items per (batch element): ceil(H * W / TC_TILE)
    long items;        // B * tiles; every item walks the T frames
    int grid;          // workgroups
    int vec;           // 1: 16-byte loads and stores, 0: scalar
};

// s, res, out, pout: the streamed tensors of the call (res and pout may be NULL).
static inline TcPlan tc_plan(int T, int B, int Ci, int Co, int H, int W, const void* s, const void* res, const void* out, const void* pout) {
    TcPlan p = {};
    p.rc = RVSR_ERR_UNSUPPORTED;
    if (T <= 0 || B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0) {
        p.rc = RVSR_ERR_BAD_ARG;
        p.msg = "tconv3: empty shape";
        return p;
    }
    if (Ci > TC_MAX_C || Co > TC_MAX_C) {
        p.msg = "tconv3: more than 64 channels in or out (the weight image of all three taps stays in LDS)";
        return p;
    }
    const long HW = (long)H * W;
    if (HW * TC_MAX_C * 4 >= ((long)1 << 31)) {   // (a frame of a batch element is addressed with 32-bit byte offsets inside a 2 GB view)
        p.msg = "tconv3: a plane of 2^23 elements or more";
        return p;
    }
    p.ks = (Ci + 15) / 16;
    p.mt = (Co + 31) / 32;
    p.tiles = (int)((HW + TC_TILE - 1) / TC_TILE);
    p.items = (long)B * p.tiles;
    p.grid = (int)(p.items < TC_SLOTS ? p.items : TC_SLOTS);
    p.vec = HW % 4 == 0 && ((((uintptr_t)s) | ((uintptr_t)res) | ((uintptr_t)out) | ((uintptr_t)pout)) & 15) == 0;
    p.rc = RVSR_OK;
    return p;
}

// ---------------------------------------------------------------------------------------------
// PReLU (forward, backward, slope gradient): element-wise streams over n floats.
#define PR_WG 256
#define PR_MAX_BLOCKS 2048   // also the number of partial sums of the slope gradient
#define PR_BLOCK_ELEMS 4096  // elements a workgroup takes per trip: one 16-byte access of every thread, four times

struct PrPlan {
    int rc;
    const char* msg;
    int blocks;   // workgroups; a function of n alone, so the order of the slope gradient's sum is fixed by the shape
    int vec;      // 1: 16-byte accesses (4-byte ones of the keep mask), 0: scalar
};

// f0 .. f4: the f32 tensors of the call (forward: a, b, y; backward: g, a, b, gres, gx; NULL where the call has none); keep: the byte
// mask or NULL.
static inline PrPlan pr_plan(size_t n, const void* f0, const void* f1, const void* f2, const void* f3, const void* f4, const void* keep) {
    PrPlan p = {};
    if (n == 0) {
        p.rc = RVSR_ERR_BAD_ARG;
        p.msg = "prelu: empty tensor";
        return p;
    }
    const size_t nb = (n + PR_BLOCK_ELEMS - 1) / PR_BLOCK_ELEMS;
    p.blocks = (int)(nb < PR_MAX_BLOCKS ? nb : PR_MAX_BLOCKS);
    p.vec = n % 4 == 0 && ((((uintptr_t)f0) | ((uintptr_t)f1) | ((uintptr_t)f2) | ((uintptr_t)f3) | ((uintptr_t)f4)) & 15) == 0 &&
            (((uintptr_t)keep) & 3) == 0;
    p.rc = RVSR_OK;
    return p;
}

static inline size_t pr_workspace_bytes() { return sizeof(float) * PR_MAX_BLOCKS; }
