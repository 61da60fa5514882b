// conv_plan.h -- which kernel a convolution call runs, and with what grid.
//
// The entries of conv_kernels.hip validate a call, ask one of the two plan functions below, and hand the plan to the launcher of the
// chosen family; the launchers (conv_kernels.hip, conv2_kernels.hip, conv_thin_kernels.hip) map the plan's template coordinates to a
// kernel and launch it.  Every eligibility rule, tile rule and slicing rule of the conv kernels is written here and nowhere else.  The
// plan functions are pure host code: no HIP call, no pointer dereferenced (addresses are only tested for alignment), no side effect --
// rvsr_conv2d_forward_plan exports the forward one, so the Python glue asks instead of restating a rule.
#pragma once
#include "conv_common.h"

static inline bool conv_al16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0;
}
// The buffer-addressed kernels reach one batch element of a tensor through 32-bit byte offsets in a 2 GB view.
static inline bool conv_span_ok(size_t H, size_t W, size_t C) { return sizeof(float) * H * W * C < ((size_t)1 << 31); }

// ------------------------------------------------------------------------------------------
// forward and data gradient (rvsr_conv2d_forward)

enum ConvFwdFamily {
    CONV_FWD_THIN = 0,   // conv_fwd_thin_kernel: 3x3 / stride 1 with <= 4 output channels on the vector ALU, exact f32
    CONV_FWD5 = 1,       // conv_fwd5_kernel<MT, ACT_IN, VEC, WIDE, NT>: 3x3 / stride 1 on the bf16 matrix cores
    CONV_FWD2 = 2,       // conv_fwd2_kernel<KS, STRIDE, MT, CCG, ACT_IN>: 3x3 / stride 2, 5x5, 1x1 on the bf16 matrix cores
    CONV_FWD_F32 = 3,    // conv_fwd_kernel<KS, STRIDE, MT, CC>: exact-f32 MFMA, takes everything
};

struct ConvFwdPlan {
    int rc;            // RVSR_OK, or what the entry returns without launching anything
    const char* msg;   // text of a refusal; nullptr: none (act 3 -- the caller has a plan B)
    int family;        // ConvFwdFamily
    int mt;            // 32-row M tiles per workgroup
    int vec;           // conv_fwd5: staging view, 0 scalar, 1 plain, 2 pixel-unshuffle, 3 zero-insert (16-byte loads)
    int wide;          // conv_fwd5: the 8 x 64 tile (else 16 x 32)
    int nt;            // terms of a product: 3, 2 / 1 in GEMM modes 2 / 3 where the kernel has them, 4 = the f16 + fp8 format
    int act_in;        // act' fused into the input load
    int cc;            // conv_fwd2: CCG (16-channel groups per chunk); conv_fwd: CC (channels per chunk)
    int vec4;          // ConvFwdParams.vec4: the 16-byte-store epilogue is usable
    int th, tw;        // output tile of a workgroup
    unsigned gx, gy, gz;
    size_t lds;
};

// Geometry of the packed weight image (conv_fwd5 / conv_fwd2, pack_weights_kernel): MT, CCG, chunks of 16 * CCG input channels,
// m-blocks of MT * 32 output channels.
static inline void conv_fwd2_geom(int ksize, int Co, int Ctot, int& mt, int& ccg, int& nchunks, int& nmb) {
    // never more than 2 M tiles per workgroup: the MT = 4 instantiation keeps 128 accumulator registers live and
    // spills (130-190 VGPRs to scratch); two 64-row m-blocks re-stage the input tile but run spill-free
    mt = (Co <= 32 || ksize == 5) ? 1 : 2;   // (5x5: 32-row m-blocks keep the 25-tap weight slice at 78 / 133 KB of LDS, stride 1 / 2)
    ccg = ksize == 1 ? 2 : 1;
    nchunks = (Ctot + 16 * ccg - 1) / (16 * ccg);
    nmb = (Co + mt * 32 - 1) / (mt * 32);
}
// The f16 + fp8 product format (ConvFwdParams.fmt) exists in the 3x3 / stride-1 kernels with 64-row m-blocks, forward weights only
static inline bool conv_f16fp8_ok(int ksize, int stride, int mt, int w_mode) { return ksize == 3 && stride == 1 && mt == 2 && w_mode == 0; }

// conv_fwd_thin_kernel: 3x3 / stride 1 / plain view / single input and output / no act' / f32 weights in the reference layout
#define THIN_FW 136          // staged columns per row: image columns x0-4 .. x0+131
#define THIN_FPL (10 * THIN_FW)
static inline bool conv_fwd_thin_ok(const ConvFwdParams& p, int ksize, int stride) {
    const TView& va = p.in.a;
    return ksize == 3 && stride == 1 && p.Co <= 4 && p.in.b.C == 0 && va.C % 8 == 0 && va.mode == 0 && va.act == nullptr &&
           p.out2 == nullptr && !p.ps && p.w_mode == 0 && p.Wout % 4 == 0 && va.Ws == p.Wout && va.Hs == p.Hout &&
           conv_al16(va.p, p.out1, p.res) && conv_span_ok(p.Hout, p.Wout, va.C) && va.C <= 256;
}

static inline ConvFwdPlan conv_fwd_refusal(const char* msg) {
    ConvFwdPlan r = {};
    r.rc = RVSR_ERR_UNSUPPORTED;
    r.msg = msg;
    r.family = -1;
    return r;
}

// `p`: the filled parameter block (views, pointers, sizes, w_mode / fmt, act); gemm_mode: the calling thread's (rvsr_gemm_mode_now).
static inline ConvFwdPlan conv_fwd_plan(const ConvFwdParams& p, int ksize, int stride, int gemm_mode) {
    const TView& va = p.in.a;
    const TView& vb = p.in.b;
    const int Ctot = va.C + vb.C, T = ksize * ksize;
    // act 3, out = (conv + bias) * (residual > 0 ? 1 : slope): an epilogue of the 8 x 64-tile conv_fwd5 kernel only
    if (p.act == 3 && (!p.res || ksize != 3 || stride != 1 || p.ps || p.out2 || gemm_mode == 1)) return conv_fwd_refusal(nullptr);
    // a periodic addend in front of the activation, out = act((conv + bias) + res[b % res_period]): an epilogue of that kernel only, too
    // (refused like the mask: the caller adds the broadcast partial in a pass of its own, rvsr_bcast_add_act)
    if (p.res_period > 0 && (p.act == 3 || ksize != 3 || stride != 1 || p.ps || p.out2 || gemm_mode == 1)) return conv_fwd_refusal(nullptr);
    ConvFwdPlan q = {};
    q.act_in = va.act != nullptr;
    q.nt = 3;
    q.th = 8;
    q.tw = 32;
    int ccg, nchunks, nmb;
    conv_fwd2_geom(ksize, p.Co, Ctot, q.mt, ccg, nchunks, nmb);
    const int ntx = (p.Wout + 31) / 32, nty8 = (p.Hout + 7) / 8;

    // ---- family
    bool split = p.act == 3 || p.res_period > 0;   // the bf16-split kernels, conv_fwd5 / conv_fwd2
    const bool thin = !split && conv_fwd_thin_ok(p, ksize, stride);
    if (!split && !thin) {
        // GEMM mode 1 is exact f32 everywhere; 5x5 through the zero-insert view of a stride-2 data gradient (in_mode 1) is staged by
        // the 3x3 kernels only; conv_fwd5's scalar staging wants a second input behind a multiple of 8 channels
        // (7x7, SpyNet's blocks: no bf16-split kernel exists for it, the exact-f32 family in every GEMM mode)
        split = gemm_mode != 1 && ksize != 7 && (va.mode != 1 || ksize == 3) && (vb.C == 0 || va.C % 8 == 0);
        // conv_fwd2 stages a plain view through raw buffer loads: 32-bit byte offsets inside one batch element (< 2 GB), and a second
        // input only behind a whole chunk, a multiple of 16 (1x1: 32) channels
        if (split && (ksize != 3 || stride == 2) && va.mode == 0 &&
            (!conv_span_ok(va.Hs, va.Ws, va.C > vb.C ? va.C : vb.C) || (vb.C != 0 && va.C % (16 * ccg) != 0)))
            split = false;
    }
    if (p.fmt && !(split && conv_f16fp8_ok(ksize, stride, q.mt, p.w_mode)))
        return conv_fwd_refusal("conv2d: the f16 + fp8 format (w_mode | 4) is for forward 3x3 / stride-1 convs with more than 32 output channels");

    if (thin) {
        q.family = CONV_FWD_THIN;
        q.mt = 1;
        q.tw = 128;
        q.gx = (unsigned)p.B * nty8 * ((p.Wout + 127) / 128);
        q.gy = q.gz = 1;
        q.lds = sizeof(float) * (8 * THIN_FPL + (size_t)va.C * 36);
        return q;
    }
    if (!split) {
        q.family = CONV_FWD_F32;
        q.mt = p.Co <= 32 ? 1 : (p.Co <= 64 ? 2 : 4);
        const int wide_m = q.mt == 4;   // (chunk sizes: LDS of 5x5 stride 1 66 / 58 KB, 2 workgroups per CU; stride 2 34 / 46 / 72 KB)
        q.cc = ksize == 1 ? 32 : ksize == 3 ? (stride == 1 ? (wide_m ? 8 : 16) : (wide_m ? 4 : 8)) : (stride == 1 ? (wide_m ? 4 : 8) : 4);
        if (ksize == 7) q.cc = wide_m ? 2 : 4;   // (14 x 38 halo, 49-tap weight slice: 59.5 / 54.8 KB at MT <= 2 / 4, 2 workgroups per CU; CC even)
        const int IH = 7 * stride + ksize, IW = 31 * stride + ksize;
        q.lds = sizeof(float) * ((size_t)q.cc * IH * IW + (size_t)T * q.cc * (q.mt * 32 + 1));
        q.gx = (unsigned)(ntx * nty8);
        q.gy = (unsigned)((p.Co + q.mt * 32 - 1) / (q.mt * 32));
        q.gz = (unsigned)p.B;
        return q;
    }
    // (the 16-byte-store epilogues address one batch element of the output / residual with 32-bit byte offsets in a 2 GB buffer view)
    q.vec4 = (p.Wout % 4 == 0) && conv_al16(p.out1, p.res) && !p.ps && p.out2 == nullptr && conv_span_ok(p.Hout, p.Wout, p.Co);
    q.cc = ccg;
    q.gy = q.gz = 1;
    long items = (long)nmb * p.B;   // (x tiles, below): persistent workgroups walk them
    if (ksize != 3 || stride != 1) {
        q.family = CONV_FWD2;
        const int IH = 7 * stride + ksize, IW = 31 * stride + ksize;   // 4 waves: 8 rows x 32 px
        q.lds = (size_t)16 * (2 * (2 * ccg) * IH * IW + 2 * T * (2 * ccg) * (q.mt * 32)) + sizeof(float) * q.mt * 32;
        items *= (long)ntx * nty8;
        const int slots = 256 * (q.lds > 80 * 1024 ? 1 : 2);   // 2 workgroups per CU when LDS allows
        q.gx = (unsigned)(items < slots ? items : slots);
        return q;
    }
    q.family = CONV_FWD5;
    // VEC staging addresses one batch element of an input with 32-bit byte offsets (raw buffers) and selects the input per
    // 16-channel chunk: planes of one element < 2 GB, a second input only behind a multiple of 16 channels
    const bool al = conv_al16(va.p, va.act, vb.p);
    if (va.mode == 0 && va.Ws % 4 == 0 && va.Wv == va.Ws && al && conv_span_ok(va.Hs, va.Ws, va.C > vb.C ? va.C : vb.C) &&
        (vb.C == 0 || va.C % 16 == 0))
        q.vec = 1;
    else if (va.mode == 2 && vb.C == 0 && va.C % 16 == 0 && va.Wv % 4 == 0 && va.Ws == 2 * va.Wv && va.Hs == 2 * va.Hv && al &&
             conv_span_ok(va.Hs, va.Ws, va.C >> 2))
        q.vec = 2;
    else if (va.mode == 1 && vb.C == 0 && va.Wv % 4 == 0 && va.Wv == 2 * va.Ws && va.Hv <= 2 * va.Hs && va.Ws % 2 == 0 && al &&
             conv_span_ok(va.Hs, va.Ws, va.C))
        q.vec = 3;
    if (p.fmt && (q.vec != 1 || q.act_in))   // f16 + fp8 images: only the plain vector-staged kernels without act' read them
        return conv_fwd_refusal("conv2d: the f16 + fp8 format needs a plain 16-byte-aligned input view with W % 4 == 0 and no act' tensor");
    // tile shape: 8 x 64 (256-byte output runs, 16-byte stores, plain vector-staged view, 64-row m-blocks) wherever it wastes no more
    // pixels than 16 x 32
    const long px_n = (long)((p.Hout + 15) / 16 * 16) * ((p.Wout + 31) / 32 * 32), px_w = (long)((p.Hout + 7) / 8 * 8) * ((p.Wout + 63) / 64 * 64);
    q.wide = q.mt == 2 && q.vec == 1 && q.vec4 && px_w <= px_n;
    if ((p.act == 3 || p.res_period > 0) && !q.wide) return conv_fwd_refusal(nullptr);   // (mask and addend epilogues: 8 x 64 tile only)
    // reduced-term products (GEMM modes 2 / 3): the 64-row m-block kernels on the vector-staged views; everything else keeps three terms
    if (p.fmt) q.nt = 4;
    else if (q.mt == 2 && q.vec != 0) q.nt = gemm_mode == 2 ? 2 : (gemm_mode == 3 ? 1 : 3);
    q.th = q.wide ? 8 : 16;
    q.tw = q.wide ? 64 : 32;
    const int NX = q.wide ? 2 * 10 * 66 : 2 * 18 * 34, WVEC = 9 * 2 * q.mt * 32;
    q.lds = (size_t)16 * (2 * 2 * NX + 2 * 2 * WVEC) + sizeof(float) * 4 * q.mt * 32 + 16;
    items *= (long)((p.Wout + q.tw - 1) / q.tw) * ((p.Hout + q.th - 1) / q.th);
    q.gx = (unsigned)(items < 256 ? items : 256);
    return q;
}

// ------------------------------------------------------------------------------------------
// weight gradient (rvsr_conv2d_backward_weight): partial sums [P][Co][Ctot][taps] (+ [P][Co] for the bias) on a (P, gy, gz) grid,
// reduced in a fixed order afterwards.  The families in the order in which they are asked:
enum ConvWgradFamily {
    CONV_WGRAD_THIN = 0,   // conv_wgrad_thin_kernel: 3x3 / stride 1, <= 4 output channels, vector ALU, exact f32 in every GEMM mode
    CONV_WGRAD2,           // conv_wgrad2_kernel: 3x3 / stride 1 on the bf16 matrix cores
    CONV_WGRAD5,           // conv_wgrad5_kernel: 5x5 on the bf16 matrix cores
    CONV_WGRAD_F32_5,      // conv_wgrad_kernel<5, S, 16>: GEMM mode 1
    CONV_WGRAD_1X1S,       // conv_wgrad1x1s_kernel: a plain GEMM on the bf16 matrix cores, LDS-staged and pipelined, 64 x 320 blocks of gW
    CONV_WGRAD_1X1,        // conv_wgrad1x1_kernel: the same GEMM straight from global memory, 64 x 64 blocks
    CONV_WGRAD_F32_3S1,    // conv_wgrad_kernel<3, 1, 64>
    CONV_WGRAD_S2,         // conv_wgrad_s2_kernel: 3x3 / stride 2 on the bf16 matrix cores
    CONV_WGRAD_F32_3S2,    // conv_wgrad_kernel<3, 2, 32>
    CONV_WGRAD_F32_1,      // conv_wgrad_kernel<1, 1, 64>
    CONV_WGRAD_F32_7,      // conv_wgrad_kernel<7, 1, 8>: 7x7 / stride 1 in every GEMM mode (SpyNet's blocks)
    CONV_WGRAD_FAMILIES
};
struct ConvWgradPlan {
    int family, P, gy, gz;
};

// Whether a family exists for this geometry at all -- what rvsr_conv2d_wgrad_workspace_bytes, which sees neither pointers nor modes, can know.
static inline bool conv_wgrad_can(int family, int ksize, int stride, int Co) {
    switch (family) {
        case CONV_WGRAD_THIN: return ksize == 3 && stride == 1 && Co <= 4;
        case CONV_WGRAD2: case CONV_WGRAD_F32_3S1: return ksize == 3 && stride == 1;
        case CONV_WGRAD5: case CONV_WGRAD_F32_5: return ksize == 5;
        case CONV_WGRAD_S2: case CONV_WGRAD_F32_3S2: return ksize == 3 && stride == 2;
        case CONV_WGRAD_F32_7: return ksize == 7 && stride == 1;
        default: return ksize == 1;   // CONV_WGRAD_1X1S, CONV_WGRAD_1X1, CONV_WGRAD_F32_1
    }
}
// How a family slices the pixels into P partial sums, and its grid.
static inline ConvWgradPlan conv_wgrad_slicing(int family, int B, int Hout, int Wout, int Co, int Ctot) {
    const long ntiles = (long)B * ((Hout + 3) / 4) * ((Wout + 31) / 32);   // 4 x 32-pixel tiles
    long units = ntiles, slots = 256;
    int gy = (Co + 63) / 64, gz = (Ctot + 63) / 64;
    switch (family) {
        case CONV_WGRAD_THIN:   // one partial per workgroup of its own grid of 4 x 64 tiles: 3 workgroups of 4 waves per CU
            units = (long)B * ((Hout + 3) / 4) * ((Wout + 63) / 64);
            slots = 768;
            gy = gz = 1;
            break;
        case CONV_WGRAD5:       // 32 x 32 blocks of the weight gradient
            gy = (Co + 31) / 32;
            gz = (Ctot + 31) / 32;
            break;
        case CONV_WGRAD_F32_5:  // 16 input channels per workgroup = 400 GEMM columns, 7 accumulator tiles per wave (64 would need 25)
            gz = (Ctot + 15) / 16;
            break;
        case CONV_WGRAD_F32_7:  // 8 input channels per workgroup = 392 GEMM columns, 13 tiles, 7 per wave: the registers of <5, S, 16>
            gz = (Ctot + 7) / 8;
            break;
        case CONV_WGRAD_S2:     // 2 workgroups of 4 waves per CU, pixels cut into 16-pixel units
            units = (long)B * Hout * ((Wout + 15) / 16);
            slots = 512;
            break;
        case CONV_WGRAD_F32_3S2:
            gz = (Ctot + 31) / 32;
            break;
        case CONV_WGRAD_1X1S: {   // one workgroup of 8 waves per CU and 64 x 320 block, pixels cut into 64-pixel tiles inside an image; never
            // more partial sums than CONV_WGRAD_1X1 would write for the geometry, so the workspace query is what it was
            const long P1 = 1024 / ((long)gy * gz);
            gz = (Ctot + 319) / 320;
            units = (long)B * ((Hout * Wout + 63) / 64);
            if (units > ntiles) units = ntiles;
            slots = 256;
            if (P1 < slots / ((long)gy * gz)) slots = P1 * gy * gz;
            break;
        }
        case CONV_WGRAD_1X1: case CONV_WGRAD_F32_1:   // the GEMM kernel runs 4 small workgroups per CU and hides its load latency with occupancy
            slots = 1024;
            break;
        default:
            break;
    }
    long P = slots / ((long)gy * gz);
    if (P < 1) P = 1;
    if (P > units) P = units;
    return {family, (int)P, gy, gz};
}
// The largest P any family might use for this geometry: sizes the workspace.
static inline int conv_wgrad_max_P(int ksize, int stride, int B, int Hout, int Wout, int Co, int Ctot) {
    int P = 0;
    for (int f = 0; f < CONV_WGRAD_FAMILIES; ++f)
        if (conv_wgrad_can(f, ksize, stride, Co)) {
            const int Pf = conv_wgrad_slicing(f, B, Hout, Wout, Co, Ctot).P;
            if (Pf > P) P = Pf;
        }
    return P;
}

// `p`: views and sizes filled (x.a / x.b = the conv's input, g = the output gradient); gemm_mode: the calling thread's.
static inline ConvWgradPlan conv_wgrad_plan(const ConvWgradParams& p, int ksize, int stride, int gemm_mode) {
    const int C1 = p.x.a.C, C2 = p.x.b.C, Ctot = C1 + C2;
    const bool al = conv_al16(p.x.a.p, p.x.b.p, p.g.p, p.g.act), split = gemm_mode != 1, plain_g = p.g.mode == 0;
    const auto takes = [&](int family) {
        switch (family) {
            case CONV_WGRAD_THIN:
                return C2 == 0 && C1 % 16 == 0 && plain_g && p.Wout % 4 == 0 && al && conv_span_ok(p.Hout, p.Wout, C1);
            case CONV_WGRAD2:
                // one image of each tensor behind 32-bit byte offsets (raw buffers, < 2 GB); the input is picked per 64-channel block: a
                // second input has to start on a multiple of 64 channels
                return split && p.Wout % 4 == 0 && al && conv_span_ok(p.Hout, p.Wout, p.Co > Ctot ? p.Co : Ctot) && (C2 == 0 || C1 % 64 == 0);
            case CONV_WGRAD5: return split;   // (the mode's terms, deterministic partials like the others)
            case CONV_WGRAD_1X1S:
                // 16-byte loads of 8-pixel items: whole float4s inside an image; one image of each tensor behind 32-bit byte offsets
                // (raw buffers, < 2 GB); the input is picked per 64-channel block
                return split && plain_g && (p.Hout * p.Wout) % 4 == 0 && al && (C2 == 0 || C1 % 64 == 0) &&
                       conv_span_ok(p.Hout, p.Wout, p.Co > (C1 > C2 ? C1 : C2) ? p.Co : (C1 > C2 ? C1 : C2));
            case CONV_WGRAD_1X1: return split && plain_g && (p.Hout * p.Wout) % 8 == 0 && al;
            case CONV_WGRAD_S2: return split && C2 == 0 && plain_g && p.Wout % 8 == 0 && p.x.a.Ws % 4 == 0 && al;
            default: return true;   // the exact-f32 kernels take what is left
        }
    };
    for (int f = 0; f < CONV_WGRAD_FAMILIES; ++f)
        if (conv_wgrad_can(f, ksize, stride, p.Co) && takes(f)) return conv_wgrad_slicing(f, p.B, p.Hout, p.Wout, p.Co, Ctot);
    return {-1, 0, 0, 0};   // (not reached: every validated (ksize, stride) has an exact-f32 family)
}
