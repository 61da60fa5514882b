// ca_plan.h -- how a channel-attention call (ca_kernels.hip) is sliced and which load width it may use.
//
// In the spirit of conv_plan.h: every slicing and eligibility rule of the channel-attention kernels is written here and nowhere else, as
// pure host code -- no HIP call, no pointer dereferenced (addresses are only tested for alignment), no side effect.
// rvsr_channel_attention_plan exports it.
#pragma once
#include "rvsr_common.h"

#define CA_MAX_C 4096          // the scale kernel keeps the C pooled values (+ C / r hidden ones) of a batch element in LDS: 16 KB + 16 KB
#define CA_WG 256              // threads of the streaming kernels
#define CA_SLOTS 1024          // workgroups that fill the chip: 256 CUs x 4
#define CA_MIN_SLICE 4096      // elements: one 16-byte load of every thread, four times -- below this a slice is all prologue
#define CA_MAX_SLICES 64

struct CaPlan {
    int rc;            // RVSR_OK, or what the entry returns without launching anything
    const char* msg;   // text of a refusal
    int slices;        // S: workgroups (and partial sums) per (b, c) plane
    int chunk;         // elements per slice, a multiple of 4; slice q covers [q * chunk, min((q + 1) * chunk, H * W))
    int vec;           // 1: 16-byte loads and stores, 0: scalar
};

// S = 1 wherever the B * C planes fill the chip by themselves (32 x 64 planes of a training batch); a few planes of a large frame
// (inference, B = 1) are cut so that about CA_SLOTS workgroups exist, never into slices below CA_MIN_SLICE elements.  No slice is empty.
static inline void ca_slicing(long planes, long HW, int& slices, int& chunk) {
    long S = 1;
    if (planes < CA_SLOTS) {
        S = (CA_SLOTS + planes - 1) / planes;
        const long by_size = (HW + CA_MIN_SLICE - 1) / CA_MIN_SLICE;
        if (S > by_size) S = by_size;
        if (S > CA_MAX_SLICES) S = CA_MAX_SLICES;
        if (S < 1) S = 1;
    }
    long ch = ((HW + 3) / 4 + S - 1) / S * 4;
    if (ch < 4) ch = 4;
    S = (HW + ch - 1) / ch;   // (rounding the chunk up to whole float4s can leave the last slices empty: drop them)
    slices = (int)S;
    chunk = (int)ch;
}

// a, b, c: the three streamed tensors of the call (forward: u, x or NULL, out; backward: gout, u, gu).
static inline CaPlan ca_plan(int B, int C, int H, int W, const void* a, const void* b, const void* c) {
    CaPlan p = {};
    p.rc = RVSR_ERR_UNSUPPORTED;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) {
        p.rc = RVSR_ERR_BAD_ARG;
        p.msg = "channel_attention: empty shape";
        return p;
    }
    if (C > CA_MAX_C) {
        p.msg = "channel_attention: more channels than the LDS scratch of the scale kernel holds (4096)";
        return p;
    }
    const long HW = (long)H * W, planes = (long)B * C;
    if (HW >= ((long)1 << 31) - 4 * CA_WG * 4) {   // (indices inside a plane are 32-bit, the unrolled loops look 4 strides ahead)
        p.msg = "channel_attention: a plane of 2^31 elements or more";
        return p;
    }
    ca_slicing(planes, HW, p.slices, p.chunk);
    if (planes * p.slices >= ((long)1 << 31)) {
        p.msg = "channel_attention: more than 2^31 workgroups";
        return p;
    }
    p.vec = HW % 4 == 0 && ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15) == 0;
    p.rc = RVSR_OK;
    return p;
}

// Workspace, in floats: [B * C * S] partial plane sums | [B * C] gs, the broadcast term of gu | [B * C] gp2 | [B * C] gz (B * Cr used).
static inline size_t ca_workspace_bytes(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    int S, chunk;
    ca_slicing((long)B * C, (long)H * W, S, chunk);
    return sizeof(float) * (size_t)B * C * ((size_t)S + 3) + 64;
}
