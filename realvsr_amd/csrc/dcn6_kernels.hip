// dcn6_kernels.hip -- backward of the modulated DCN, sixth generation (gfx950): dcn_bwdin6 (input / offset / mask gradient) and, further
// down, dcn_bwdw6 (weight / bias gradient).
//
// dcn_bwdin6 replaces the reference's modulated_deformable_col2im + col2im_coord pair (kernel.cu:636-767) together with the
// `columns = W^T gOut` GEMM of deform_conv_cuda.cpp:623-626 in front of them, where 8 divides the channels per deformable group; every other
// call takes the first-generation dcn_bwd_input_kernel (dcn_kernels.hip).  Workgroup = 8 waves = 8 rows x 32 pixels, K chunk = 8 input channels.
//
// The scatter window (from the fifth generation, dcn_bwdin5; micro-benchmarks of the LDS on the MI355X: tools/micro/, profiles/r03_notes.md),
// cycles per wave instruction per CU with 8 waves issuing:
//     ds_add_u32 3.7    ds_add_u64 5.6    ds_add_f64 7.3    ds_add_f32 169 (!)    128-bit read-modify-write pair 15-23,
//     the same whether 16 or 64 lanes are active; with the address pattern of this scatter at sub-pixel offsets of random sign
//     (neighbouring lanes land on the same or the neighbouring cell): ds_add_u32 5.9, ds_add_u64 11.3, ds_add_f64 19.7.
//   * The grad_input tile of a workgroup is ONE shared window of 32-bit FIXED-POINT cells that every lane updates with ds_add_u32: no
//     ownership, no parity passes, no claims, no merge, any offset pattern.  Integer addition is associative: the in-tile sum is
//     bit-reproducible whatever the order.
//     Scale: a contribution is w_corner * mask * col_grad with w, mask in [0, 1] and |col_grad[t, c, px]| = |<W[:, c, t], gOut[:, px]>|
//     <= ||W[:, c, t]||_2 * ||gOut[:, px]||_2 (Cauchy-Schwarz); with Wn = the largest column norm of the chunk (dcn_bwd5_wnorm_kernel) and
//     Gn = the largest pixel norm of the tile (prologue) -- of the operands the products see: in the reduced-term GEMM modes the bf16-rounded
//     weights and, with one term, the bf16-rounded output gradient --, S = 2^31 / (2304 * Wn * Gn) maps every contribution to |q| <= 2^19.8 and a cell
//     can receive at most 8 * 32 * 9 = 2304 of them per chunk (each (pixel, tap) at most once): NO overflow for any input.
//     One unit is ~1e-6 of the bound, round-to-nearest (magic-number add), so the quantisation noise of a cell (~6 units at 36
//     contributions) stays below the bf16x3 error of col_grad itself; measured against the f64 oracle in tests/test_gpu_dcn*.py.
//   * 4 B per (cell, channel): the halo R is a template parameter, R = 2 / 4 / 5 / 8 / 12 px around the 8 x 32 pixel tile, selected on the
//     device from the offsets (dcn_offset_probe2_kernel).  Samples beyond the window keep the global gather / atomic path.
//   * Co > 64 runs in ONE pass: the K loop of col_grad = W^T gOut covers all output channels (NK = 8 k-steps: 64 VGPRs of gOut fragments, a
//     48 KB weight block per chunk), so sampling, scatter, flush and the offset / mask stores are done once.
//
// What the sixth generation changed (profiles/r04_*, r05_notes.md): dcn_bwdin5 executed 1.06 G vector wave-instructions per L1 launch against
// the forward's 0.24 G -- 200 per (wave, tap) -- and half of them were forced by its lane layout: the accumulator registers of lane
// (pixel, half) held 4 channels of FOUR taps, so both halves of a wave computed every sampling geometry, every tap needed three partner-lane
// sums (v_permlane32_swap + nops) for grad_offset / grad_mask, and each lane carried four channels through scalar f32 arithmetic.  Here
//   * the M rows of col_grad = W^T gOut are PERMUTED in the packed weight image so that lane (pixel, half) holds all 8 channels of TWO
//     taps: a lane owns a whole (pixel, tap) -- one geometry per lane, no partner-lane sums, every lane stores its own grad_offset /
//     grad_mask -- and the halves of a wave work on different taps: 5 lane iterations per chunk instead of 9 taps;
//   * the per-channel arithmetic runs on channel PAIRS (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 with op_sel broadcasts);
//   * the main path of a lane iteration is branch-free (dead lanes add 0 to spread cells and store beyond the buffer view); samples
//     beyond the window take the global gather / atomics with the reference's rule set.
//
// (A fully fused backward -- this kernel plus the weight gradient from the same sampling pass, column values transposed by the matrix
// core -- is numerically right and kept as experiments/dcn_bwd6_fused.hip; it needs ~400 live registers per wave and ran 16 ms per L1
// launch against 7.3 for the pair: profiles/r05_notes.md.)
#include "dcn_tile.h"
#include "dcn_plan.h"

#include "timeline.h"

// Timeline slots (timeline.h), read by tools/dcn6_timeline.py: lane 0 of wave 3 (thread 192) of one workgroup of each kernel
#define BI6_TL (blockIdx.x == 77 && blockIdx.z == 1 && threadIdx.x == 192)
#define BW6_TL (blockIdx.x == 77 && threadIdx.x == 192)
enum Bwdin6Stamp {       // dcn_bwdin6_kernel, workgroup 77 of batch element 1
    BI6_PROLOGUE = 0,    // gOut fragments, gOut^T emitted, window zeroed, chunk 0 requested
    BI6_END = 9,
    BI6_CHUNK = 10,      // + 8 * chunk (< 4) + {0: top, 1: x tile committed, 2: vmcnt(0), 3: barrier passed, 4: lane iterations done, 5: barrier passed,
                         //                      6: next requests issued, 7: flush done}
    BI6_C1_ITER = 50,    // + 4 * it + {0: start, 1: reads + math + atomics issued}, chunk 1, lane iteration it = 0..4
    BI6_C1_MTILE = 90,   // + mt: chunk 1, MFMAs of M tile mt issued
};
enum Bwdw6Stamp {        // dcn_bwdw6_kernel, workgroup 77, the third tile of its stream
    BW6_TILE = 128,      // + {0: top, 1: vmcnt(0): operands + x landed, 2: x committed + barrier, 3: next requests set up, 4: iterations done, 5: end barrier passed}
    BW6_ITER = 138,      // + 4 * it + {0: start, 1: column values blended, 2: split + transposer issued}, lane iteration it = 0..4
};

// Lane iteration `it` (0..4) of lane half h works on tap (half 0, half 1): (0, 3), (1, 6), (4, 7), (2, 5), (8, none).  The two taps of an
// iteration sit in DIFFERENT kernel rows: the halves' cells of one ds_add_u32 are then a window row (+-) apart and never the same cell.
// (First version: (0, 2), (1, 3), (4, 6), (5, 7) -- same row, two columns apart: lane (px + 2, half 0) and lane (px, half 1) hit the same
// cell in the same instruction whenever their floor()s agree, and the LDS serialises same-address atomics; the kernel was no faster than
// dcn_bwdin5 although it executes half the vector instructions.)
__host__ __device__ __forceinline__ int bwd6_tap(int it, int h) {
    return h == 0 ? (it == 0 ? 0 : it == 1 ? 1 : it == 2 ? 4 : it == 3 ? 2 : it == 4 ? 8 : -1)
                  : (it == 0 ? 3 : it == 1 ? 6 : it == 2 ? 7 : it == 3 ? 5 : -1);
}

// Wn[chunk] for the fixed-point scale: one block per chunk, 576 threads = 72 (tap, channel) columns x 8 slices of the output
// channels; slice sums combined through LDS, then the maximum over the columns.
// hi_only (the reduced-term GEMM modes): the norms of the bf16-rounded weights, the operand those products see -- the scale, and with it
// every fixed-point contribution, is then the one the three-term kernel derives from pre-rounded weights: a speed mode differs from mode 0
// on the rounded operands by the summation order of the scatter alone (tests/test_gpu_modes_definition.py).
__global__ __launch_bounds__(576) void dcn_bwd5_wnorm_kernel(const float* __restrict__ w, float* __restrict__ wn, int Co, int C, int hi_only) {
    __shared__ float red[576];
    const int chunk = blockIdx.x, t = threadIdx.x, col = t % 72, sl = t / 72;
    const int tap = col >> 3, c = 8 * chunk + (col & 7);
    float s = 0.f;
    if (c < C)
        for (int o = sl; o < Co; o += 8) {
            float v = w[((size_t)o * C + c) * 9 + tap];
            if (hi_only) v = (float)(__bf16)v;   // (round to nearest even: split8's hi part)
            s += v * v;
        }
    red[t] = s;
    __syncthreads();
    if (t < 72) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) a += red[t + 72 * k];
        red[t] = a;
    }
    __syncthreads();
    if (t < 64) red[t] = fmaxf(red[t], t + 64 < 72 ? red[t + 64] : 0.f);
    __syncthreads();
    for (int k = 32; k > 0; k >>= 1) {
        if (t < k) red[t] = fmaxf(red[t], red[t + k]);
        __syncthreads();
    }
    if (t == 0) wn[chunk] = sqrtf(red[0]);
}

// packed[chunk][mt (3)][part (hi, lo)][o-octet (2 NK)][row (32)][8 o].  Row i of M tile mt lands in accumulator register
// r = (i & 3) + 4 (i >> 3) of lane half h = (i >> 2) & 1 (D layout of the 32x32 MFMA); that register is to hold channel r & 7 of the tap of
// lane iteration it = 2 mt + (r >> 3).
template <int NK>
__global__ void pack_weights_bwd6_kernel(const float* __restrict__ w, bf16x8* __restrict__ packed, int Co, int C, int nchunks) {
    const size_t total = (size_t)nchunks * 3 * (2 * NK) * 32;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(idx & 31);
        size_t r = idx >> 5;
        const int ooct = (int)(r % (2 * NK));
        r /= (2 * NK);
        const int mt = (int)(r % 3), chunk = (int)(r / 3);
        const int h = (row >> 2) & 1, reg = (row & 3) + 4 * (row >> 3);
        const int tap = bwd6_tap(2 * mt + (reg >> 3), h), c = 8 * chunk + (reg & 7);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int o = 8 * ooct + j;
            v[j] = (tap >= 0 && c < C && o < Co) ? w[((size_t)o * C + c) * 9 + tap] : 0.f;
        }
        bf16x8 hi, lo;
        split8(v, hi, lo);
        const size_t blk = ((size_t)chunk * 3 + mt) * 2, per = (size_t)(2 * NK) * 32;
        packed[blk * per + ooct * 32 + row] = hi;
        packed[(blk + 1) * per + ooct * 32 + row] = lo;
    }
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) {
    f32x2 r;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) {
    f32x2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// s.x * b + c  /  s.y * b + c  (op_sel picks the half of s that both result lanes read)
__device__ __forceinline__ f32x2 pk_fma_x(f32x2 s, f32x2 b, f32x2 c) {
    f32x2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(r) : "v"(s), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ f32x2 pk_fma_y(f32x2 s, f32x2 b, f32x2 c) {
    f32x2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0]" : "=v"(r) : "v"(s), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ f32x2 pk_mul_x(f32x2 s, f32x2 b) {
    f32x2 r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(r) : "v"(s), "v"(b));
    return r;
}
__device__ __forceinline__ f32x2 pk_mul_y(f32x2 s, f32x2 b) {
    f32x2 r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0]" : "=v"(r) : "v"(s), "v"(b));
    return r;
}
__device__ __forceinline__ void lds_add_i32_6(int* p, int v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // ds_add_u32
}
// a + b of the two lane halves in every lane: v_permlane32_swap a, b exchanges lanes 32..63 of a with lanes 0..31 of b; with a = b = v every
// lane then holds both halves' values (VALU, no LDS queue).  Inline assembly: this hipcc lowers the second result of
// __builtin_amdgcn_permlane32_swap to a copy of the first; the s_nop covers the VALU-write -> permlane-read distance by hand.
__device__ __forceinline__ float half_sum6(float v) {
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 0" : "+v"(a), "+v"(b));
    return a + b;
}
// 8 f32 registers holding exact bf16 values -> one bf16x8 MFMA operand
__device__ __forceinline__ bf16x8 pack8_exact(const f32x16& d, int r0) {
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (__bf16)d[r0 + e];
    return o;
}


struct DcnBwdIn6Params {
    DcnGeom d;
    TView g;            // grad_output view (Co, Ho, Wo), optional fused act'
    float* gx;          // (B, C, H, W): accumulated into (zero or a partial gradient on entry)
    float* goff;
    float* gmask;
    size_t goff_bs, gmask_bs;
    DcnHaloSel sel;     // kernel selection on the device (dcn_common.h): every candidate halo is launched, one runs
    const float* wnorm; // [chunk]: max over the chunk's 72 (tap, channel) columns of ||W[:, c, tap]||_2  (dcn_bwd5_wnorm_kernel)
    bf16x8* agt;        // optional side output for dcn_bwdw6 (nullptr: none): gOut x act' of every pixel row as the A operands of the weight-gradient
    int agt_nmb32;      // GEMM, [b][row][x tile][mb32 (agt_nmb32)][ks (2)][hi, lo][lane (64)] bf16x8 -- see bwd6_emit_agt
    int agt_rows;       // rows per batch element in that buffer (a multiple of the tile height >= Ho)
};

// gOut^T by the matrix core.  The fragments gh / gl of a wave hold gOut[o = 16 ks + 8 h + e][pixel = lane & 31] (lane = pixel, K = output channel:
// the B operand of col_grad = W^T gOut).  The weight gradient gW = gOut col^T needs gOut with PIXELS along K: D = A x [I16 | 0] + A' x [0 | I16] with
// 0/1 selectors as B operands moves A[i = pixel][k = o] to D[i = pixel][j = o], whose register layout is (lane = j = o, register = i = pixel) --
// exact (one non-zero product per output, f32 accumulate).  Registers 0..7 / 8..15 of D are the two k-steps of the consumer; the pixel order along
// K is whatever the D layout makes it, the same for the column operand dcn_bwdw6 builds the same way.
template <int NK>
__device__ __forceinline__ void bwd6_emit_agt(bf16x8* dst, int nmb32, const bf16x8 (&gh)[NK], const bf16x8 (&gl)[NK], int lane) {
    const int lo = lane & 31, hi = lane >> 5;
    bf16x8 sel_e, sel_o;   // lane (j = lo, h = hi) supplies B[k = 8 h + e][j]:  even: (j == k), j < 16;  odd: (j == k + 16)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        sel_e[e] = (__bf16)((lo == 8 * hi + e) ? 1.f : 0.f);
        sel_o[e] = (__bf16)((lo == 8 * hi + e + 16) ? 1.f : 0.f);
    }
#pragma unroll
    for (int m = 0; m < (NK + 1) / 2; ++m) {
        f32x16 th = mfma_bf16_first(gh[2 * m], sel_e), tl = mfma_bf16_first(gl[2 * m], sel_e);
        if (2 * m + 1 < NK) {
            th = mfma_bf16(gh[2 * m + 1], sel_o, th);
            tl = mfma_bf16(gl[2 * m + 1], sel_o, tl);
        }
        bf16x8* q = dst + (size_t)(m * 4) * 64 + lane;
        q[0 * 64] = pack8_exact(th, 0);
        q[1 * 64] = pack8_exact(tl, 0);
        q[2 * 64] = pack8_exact(th, 8);
        q[3 * 64] = pack8_exact(tl, 8);
    }
    const bf16x8 z = {};
    for (int m = (NK + 1) / 2; m < nmb32; ++m) {   // (Co <= 32 inside a unit of 64 output channels: the second half reads as zero)
        bf16x8* q = dst + (size_t)(m * 4) * 64 + lane;
        q[0 * 64] = z; q[1 * 64] = z; q[2 * 64] = z; q[3 * 64] = z;
    }
}

// TERMS: terms of the bf16 product W^T * gOut (rvsr_common.h: gemm modes): 3 = hi*hi + hi*lo + lo*hi; 2 = without the weights' lo part;
// 1 = hi*hi.  WPS: waves per SIMD the launch bounds promise (2 = one 8-wave workgroup per CU).
// W2: two weight buffers in LDS (the DMA of chunk c + 1 is issued at the top of chunk c's iterations instead of after them).
// G2: two grad_input windows in LDS: chunk c scatters into one while the other -- chunk c - 1's -- is flushed a few rows per lane iteration
// of chunk c, inside the iterations' own stalls, instead of as a phase of its own between two barriers (round 6).
// (the second argument of __launch_bounds__ is waves per SIMD, not workgroups per CU)
template <int NK, int R, int TERMS, int WPS, bool W2, bool G2>
__global__ __launch_bounds__(512, WPS) void dcn_bwdin6_kernel(const DcnBwdIn6Params p, const bf16x8* __restrict__ wpack) {
    constexpr int TH = 8, NT = TH * 64;
    constexpr int TR = TH + 2 * R + 3, TC = 32 + 2 * R + 3, NPOS = TR * TC;
    constexpr int WBLK = 2 * (2 * NK) * 32;                        // vectors per (chunk, M tile): hi + lo
    constexpr int NXI = (2 * NPOS + NT - 1) / NT;                  // x-tile items (float4 of one position and quad) per thread
    constexpr int NWV = (3 * WBLK + NT - 1) / NT;                  // weight vectors per thread
    static_assert((3 * WBLK) % 64 == 0, "whole waves of weight vectors");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float4* xt = reinterpret_cast<float4*>(smem_raw);              // [2 quads][NPOS], zero outside the image
    int* gwin0 = reinterpret_cast<int*>(xt + 2 * NPOS);            // [G2 ? 2 : 1][8 channels][NPOS]: the grad_input tile of a chunk, fixed point
    bf16x8* wsb = reinterpret_cast<bf16x8*>(gwin0 + (G2 ? 2 : 1) * 8 * NPOS);   // [W2 ? 2 : 1][3][WBLK]
    float* gn_red = reinterpret_cast<float*>(wsb + (W2 ? 2 : 1) * 3 * WBLK);   // [8 waves]: largest ||gOut[:, px]||^2 of the wave's row
    if (dcn_halo_not_selected(p.sel)) return;   // (uniform) not the halo the offsets of this call ask for
    const DcnGeom& d = p.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 31, hi = lane >> 5;
    unsigned sbx, sby, sbz;
    swizzled_block(sbx, sby, sbz, d.swz);
    const int tx = __builtin_amdgcn_readfirstlane((int)(sbx % d.ntx)), ty = __builtin_amdgcn_readfirstlane((int)(sbx / d.ntx));
    const int x0 = tx * 32, y0 = ty * TH, b = __builtin_amdgcn_readfirstlane((int)sbz);
    const int ty0 = y0 - d.pad - R, tx0 = x0 - d.pad - R;         // image coordinates of tile cell (0, 0); stride 1
    const int nchunks = (d.C + 7) / 8;
    const unsigned HW = (unsigned)(d.H * d.W);
    const size_t hw = (size_t)d.Ho * d.Wo;
    const int oy = y0 + wave, ox = x0 + lo;
    const bool px_ok = oy < d.Ho && ox < d.Wo;
    const size_t pix = (size_t)oy * d.Wo + ox;
    // raw buffer views of this batch element (32-bit byte offsets: the launcher checks that each spans < 2 GB)
    const __amdgpu_buffer_rsrc_t x_rs = buf_view_2g(d.x + (size_t)b * d.C * HW), gx_rs = buf_view(p.gx + (size_t)b * d.C * HW);
    const __amdgpu_buffer_rsrc_t off_rs = buf_view(d.offset + (size_t)b * d.off_bs), msk_rs = buf_view(d.mask + (size_t)b * d.mask_bs);
    const __amdgpu_buffer_rsrc_t goff_rs = buf_view(p.goff + (size_t)b * p.goff_bs), gmsk_rs = buf_view(p.gmask + (size_t)b * p.gmask_bs);
    const unsigned pl4 = 4u * (unsigned)hw, HW4 = 4u * HW;        // bytes per offset / mask plane, per x plane
    const unsigned pix4 = px_ok ? 4u * (unsigned)pix : 0u;
    const float by = (float)(oy - d.pad), bx = (float)(ox - d.pad);   // image coordinates of tap (0, 0) at zero offset

    // x-tile items of this thread, once per tile: item = (quad, row, col); a position outside the image (or no item) gets a
    // lane offset beyond the 2 GB view, for which the buffer load returns 0 -- the zero padding costs no clamp and no select
    unsigned xoff[NXI];
#pragma unroll
    for (int k = 0; k < NXI; ++k) {
        const int it = tid + k * NT;
        const int quad = it >= NPOS ? 1 : 0, pos = it - quad * NPOS;
        const int rr = pos / TC, ss = pos - rr * TC;
        const int gy = ty0 + rr, gx = tx0 + ss;
        const bool ok = it < 2 * NPOS && gy >= 0 && gy < d.H && gx >= 0 && gx < d.W;
        xoff[k] = ok ? 4u * ((unsigned)(gy * d.W + gx) + (unsigned)(4 * quad) * HW) : 0x80000000u;
    }

    // gOut (x act') of this lane's pixel as bf16 hi / lo MFMA fragments: K = output channels, NK k-steps of 16
    bf16x8 gh[NK], gl[NK];
    float gsq = 0.f;
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
        const int ol0 = 8 * (2 * ks + hi);
        float v[8];
        if (p.g.mode == 0) {  // (uniform)
            tview_get_plain<8>(p.g, b, ol0, oy, ox, v);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = tview_get(p.g, b, ol0 + j, oy, ox);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (px_ok && ol0 + j < d.Co) ? v[j] : 0.f;
        split8(v, gh[ks], gl[ks]);
        // (one term: the products see the rounded output gradient, and so does the scale -- see dcn_bwd5_wnorm_kernel)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float u = TERMS == 1 ? (float)gh[ks][j] : v[j];
            gsq = __builtin_fmaf(u, u, gsq);
        }
    }
    {   // Gn^2 = the largest squared pixel norm of the tile (read back after the first barrier)
        gsq = half_sum6(gsq);
#pragma unroll
        for (int sft = 16; sft > 0; sft >>= 1) gsq = fmaxf(gsq, __shfl_xor(gsq, sft));
        if (lane == 0) gn_red[wave] = gsq;
    }
    for (int e = tid; e < (G2 ? 2 : 1) * 8 * NPOS; e += NT) gwin0[e] = 0;
    if (p.agt != nullptr)   // (uniform) this row's gOut as the weight-gradient kernel wants it (rows beyond Ho: zeros, the buffer covers the tile)
        bwd6_emit_agt<NK>(p.agt + (((size_t)b * p.agt_rows + oy) * d.ntx + tx) * (size_t)(p.agt_nmb32 * 4 * 64), p.agt_nmb32, gh, gl, lane);

    unsigned mg0 = 0x4B400000u;          // 1.5 * 2^23: the magic number of the fixed-point rounding, kept out of the literal encoder
    asm volatile("" : "+s"(mg0));
    const f32x2 MAGIC = {__builtin_bit_cast(float, mg0), __builtin_bit_cast(float, mg0)};

    float o_dy[5], o_dx[5], o_m[5];
    float xv[NXI][4];
    // requests of a chunk: (dy, dx, mask) of this lane's pixel at its five taps (15 loads), the weight blocks (LDS-DMA: lane l of a wave
    // lands at M0 + 16 l, no registers), the x tile (registers; committed to LDS at the top of the chunk).  Round 6: after the first chunk
    // they are issued a slice per lane iteration of the PREVIOUS chunk -- the triple of iteration `it` into the registers that iteration has
    // just read, x item `it` into the registers the chunk's commit has freed -- instead of as one burst between the iterations and the flush:
    // 34 vector-memory instructions in a row took 3 K of a chunk's 31 K cycles to issue (timeline in profiles/r06_notes.md).
    auto request_offsets = [&](int it, int chunk) {
        const int g = (chunk * 8) / d.cpg;
        const unsigned ob = (unsigned)(g * 18) * pl4, mb_ = (unsigned)(g * 9) * pl4;
        const int t0 = bwd6_tap(it, 0), t1 = it < 4 ? bwd6_tap(it, 1) : t0;   // (it == 4, half 1: no tap; reads tap 8, unused)
        const unsigned tp = (unsigned)(hi ? t1 : t0) * pl4;
        o_dy[it] = buf_load(off_rs, pix4 + 2u * tp, ob);
        o_dx[it] = buf_load(off_rs, pix4 + 2u * tp, ob + pl4);
        o_m[it] = buf_load(msk_rs, pix4 + tp, mb_);
    };
    auto request_weights = [&](int chunk, bf16x8* dst) {
        const bf16x8* src = wpack + (size_t)chunk * 3 * WBLK;
#pragma unroll
        for (int i = 0; i < NWV; ++i) {
            const int e = tid + i * NT;
            if (e - lane + 63 < 3 * WBLK)   // (wave-uniform)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + e),
                                                 (__attribute__((address_space(3))) void*)(dst + e), 16, 0, 0);
        }
    };
    auto request_x_item = [&](int k, int chunk) {
#pragma unroll
        for (int e = 0; e < 4; ++e) xv[k][e] = buf_load(x_rs, xoff[k], (unsigned)(chunk * 8 + e) * HW4);   // (C % 8 == 0)
    };
#pragma unroll
    for (int it = 0; it < 5; ++it) request_offsets(it, 0);
    request_weights(0, wsb);
#pragma unroll
    for (int k = 0; k < NXI; ++k) request_x_item(k, 0);
    RVSR_STAMP(BI6_TL, BI6_PROLOGUE);

    // ---- flush of window rows [r0, r1) of the chunk at channel cf0: wave w owns channel cf0 + w; one global atomic per touched cell inside the
    // image (the halos of neighbouring workgroups overlap), cell back to zero for its next use.  Round 6: a lane owns a window COLUMN and walks
    // the rows four at a time -- no division per cell, the row test is scalar, the column test and the image offset are per-kernel constants
    // (the round-5 form, four consecutive cells per lane, spent ~12 vector instructions per cell: a third of the kernel's vector work).
    static_assert(TC <= 64, "one lane per window column");
    const int fl_xx = tx0 + lane;
    const bool fl_col_ok = lane < TC && fl_xx >= 0 && fl_xx < d.W;
    const unsigned fl_col4 = 4u * (unsigned)(ty0 * d.W + fl_xx);   // (wraps for rows above the image: only used where the row test passed)
    auto flush_rows = [&](int* win, int cf0, float inv_s, int r0, int r1) {
        const unsigned cpl = (unsigned)(cf0 + wave) * HW4;
        int* gc = win + wave * NPOS + lane;
        const bool ok = fl_col_ok && cf0 + wave < d.C;
        if (lane < TC) {
#pragma unroll 1
            for (int r = r0; r < r1; r += 4) {
                int v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = r + j < r1 ? gc[(r + j) * TC] : 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int yy = ty0 + r + j;   // (uniform)
                    if (v[j] != 0) {
                        gc[(r + j) * TC] = 0;
                        if (ok && yy >= 0 && yy < d.H)
                            buf_atomic_add(gx_rs, fl_col4 + 4u * (unsigned)((r + j) * d.W), cpl, (float)v[j] * inv_s);
                    }
                }
            }
        }
    };
    constexpr int FRB = (TR + 4) / 5;   // window rows flushed per lane iteration (G2)
    float invS_prev = 0.f;
    // G2: the rows of one lane iteration in two halves -- the LDS reads at the top of the iteration (in front of its own atomics: read behind them
    // they waited for the whole burst to drain), the atomics / re-zeroing at its end
    auto flush_read = [&](const int* win, int r0, int (&v)[FRB]) {
        const int* gc = win + wave * NPOS + (lane < TC ? lane : 0);
#pragma unroll
        for (int j = 0; j < FRB; ++j) v[j] = r0 + j < TR ? gc[(r0 + j) * TC] : 0;
    };
    auto flush_commit = [&](int* win, int cf0, float inv_s, int r0, const int (&v)[FRB]) {
        const unsigned cpl = (unsigned)(cf0 + wave) * HW4;
        int* gc = win + wave * NPOS + lane;
        const bool ok = fl_col_ok && cf0 + wave < d.C;
#pragma unroll
        for (int j = 0; j < FRB; ++j) {
            const int yy = ty0 + r0 + j;   // (uniform)
            if (lane < TC && v[j] != 0) {
                gc[(r0 + j) * TC] = 0;
                if (ok && yy >= 0 && yy < d.H)
                    buf_atomic_add(gx_rs, fl_col4 + 4u * (unsigned)((r0 + j) * d.W), cpl, (float)v[j] * inv_s);
            }
        }
    };

    for (int chunk = 0; chunk < nchunks; ++chunk) {
        const int c0 = chunk * 8;
        const int g = c0 / d.cpg;
        int* const gwin = gwin0 + (G2 ? (chunk & 1) * 8 * NPOS : 0);
        int* const gwin_prev = gwin0 + (G2 ? ((chunk + 1) & 1) * 8 * NPOS : 0);
        RVSR_STAMP(BI6_TL && chunk < 4, BI6_CHUNK + 8 * chunk + 0);
#pragma unroll
        for (int k = 0; k < NXI; ++k) {
            const int it = tid + k * NT;
            if (it < 2 * NPOS) xt[it] = make_float4(xv[k][0], xv[k][1], xv[k][2], xv[k][3]);
        }
        RVSR_STAMP(BI6_TL && chunk < 4, BI6_CHUNK + 8 * chunk + 1);
        if (!W2 || chunk == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of the weight DMA has landed (W2: waited for below)
        RVSR_STAMP(BI6_TL && chunk < 4, BI6_CHUNK + 8 * chunk + 2);
        __syncthreads();
        RVSR_STAMP(BI6_TL && chunk < 4, BI6_CHUNK + 8 * chunk + 3);
        const int cn = chunk + 1 < nchunks ? chunk + 1 : chunk;   // (uniform) the chunk whose requests ride on this one's iterations; the last asks for itself
        bf16x8* const wcur = wsb + (W2 ? (chunk & 1) * 3 * WBLK : 0);
        if (W2) request_weights(cn, wsb + ((chunk + 1) & 1) * 3 * WBLK);   // (the other buffer: read by chunk - 1, whose iterations are behind the barrier)

        // fixed-point scale of this chunk (file header): |contribution| * S <= 0.995 * 2^31 / 2304
        float S, invS;
        {
            float g2 = gn_red[0];
#pragma unroll
            for (int k = 1; k < TH; ++k) g2 = fmaxf(g2, gn_red[k]);
            const float bound = 1.002f * p.wnorm[chunk] * sqrtf(g2);
            S = bound > 0.f ? 927407.f / bound : 0.f;
            invS = bound > 0.f ? bound * (1.f / 927407.f) : 0.f;
        }
        const bool first_of_group = c0 % d.cpg == 0;   // (uniform) later chunks of a deformable group (cpg > 8) add to its planes
        // col_grad of M tile mt (two lane iterations' worth): issued one M tile AHEAD of its iterations (round 6), so that the matrix pipe works
        // under the previous tile's scatter instead of in front of its own (12 MFMAs + their fragment reads stood 1.2-1.6 K cycles per tile)
        auto col_grad_tile = [&](int mt) {
            f32x16 a = zero16();
            const bf16x8* wb_hi = wcur + mt * WBLK;
            const bf16x8* wb_lo = wb_hi + (2 * NK) * 32;
#pragma unroll
            for (int ks = 0; ks < NK; ++ks) {
                const bf16x8 ah = wb_hi[(2 * ks + hi) * 32 + lo];
                a = ks == 0 ? mfma_bf16_first(ah, gh[0]) : mfma_bf16(ah, gh[ks], a);
                if (TERMS >= 2) a = mfma_bf16(ah, gl[ks], a);
                if (TERMS >= 3) a = mfma_bf16(wb_lo[(2 * ks + hi) * 32 + lo], gh[ks], a);
            }
            return a;
        };
        // AHEAD: M tile 0 at the top of the chunk; the MFMAs of tile mt + 1 INSIDE the two lane iterations of tile mt, a k-step behind each of their
        // first channel pairs, with the weight fragments read at the top of the iteration (in front of its atomics).  As a block between the
        // iterations a tile's 12 MFMAs stood 1.4-2.3 K cycles (fragment reads queued behind 32 LDS atomics, then both waves of the SIMD on the
        // matrix pipe): a quarter of a chunk (timeline in profiles/r06_notes.md).
        constexpr bool AHEAD = NK <= 4 && R <= 5;   // (NK = 8 holds 64 registers of gOut fragments, R >= 8 24 of x-tile items: a second accumulator tile would spill)
        constexpr int KH = (NK + 1) / 2;  // k-steps of the next tile per lane iteration
        f32x16 acc_next = zero16();
        if (AHEAD) acc_next = col_grad_tile(0);
#pragma unroll
        for (int mt = 0; mt < 3; ++mt) {
            f32x16 acc;
            if (AHEAD) {
                acc = acc_next;
            } else {
                acc = col_grad_tile(mt);
            }
            RVSR_STAMP(BI6_TL && chunk == 1, BI6_C1_MTILE + mt);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int it = 2 * mt + s;
                if (it >= 5) continue;   // (compile time)
                RVSR_STAMP(BI6_TL && chunk == 1, BI6_C1_ITER + 4 * it + 0);
                int fv[FRB];
                if (G2 && chunk > 0) flush_read(gwin_prev, it * FRB, fv);   // (uniform) the previous chunk's window: this iteration's share of rows
                // weight fragments of this iteration's share of the NEXT M tile (k-steps ks0 .. ks0 + KH - 1)
                const bool pre = AHEAD && mt < 2;      // (constant after unrolling)
                const int ks0 = s * KH;
                bf16x8 fh[KH], fl[KH];
                if (pre) {
                    const bf16x8* nb_hi = wcur + (mt + 1) * WBLK;
                    const bf16x8* nb_lo = nb_hi + (2 * NK) * 32;
#pragma unroll
                    for (int j = 0; j < KH; ++j) {
                        if (ks0 + j < NK) {
                            fh[j] = nb_hi[(2 * (ks0 + j) + hi) * 32 + lo];
                            if (TERMS >= 3) fl[j] = nb_lo[(2 * (ks0 + j) + hi) * 32 + lo];
                        }
                    }
                }
                const int t0 = bwd6_tap(it, 0), t1 = it < 4 ? bwd6_tap(it, 1) : 0;
                const bool has_tap = it < 4 || hi == 0;
                const int tap = hi ? t1 : t0;
                const bool act_lane = px_ok && has_tap;
                // lanes without a pixel / a tap: zero offset, zero mask (their col_grad is 0 or belongs to zero weight rows)
                const float dy = act_lane ? o_dy[it] : 0.f, dx = act_lane ? o_dx[it] : 0.f;
                float m = o_m[it];
                request_offsets(it, cn);   // (the registers just read: the next chunk's triple of this iteration)
#pragma unroll
                for (int k = it; k < NXI; k += 5) request_x_item(k, cn);   // (xv is free: committed to LDS at the top of this chunk)
                if (d.mask_logit) m = __builtin_amdgcn_rcpf(1.f + __expf(-m));
                const float kyf = hi ? (float)(t1 / 3) : (float)(t0 / 3), kxf = hi ? (float)(t1 % 3) : (float)(t0 % 3);
                // sample position in IMAGE coordinates exactly as the reference forms it (kernel.cu:594-616, 722-737)
                const float y = (by + kyf) + dy, x = (bx + kxf) + dx;
                const float fy = floorf(y), fx = floorf(x);
                const int yi = (int)fy, xi = (int)fx;
                const float ly = y - fy, lx = x - fx, hy = 1.f - ly, hx = 1.f - lx;
                const int r0 = yi - ty0, s0 = xi - tx0;   // tile coordinates of the top-left corner
                const bool in_tile = act_lane && (unsigned)r0 < (unsigned)(TR - 1) && (unsigned)s0 < (unsigned)(TC - 1);
                const bool inside = y > -1.f && x > -1.f && y < (float)d.H && x < (float)d.W;
                const bool far = !in_tile && inside && act_lane;   // beyond the halo: global gather / atomics with the full rule set
                const int pos0 = in_tile ? r0 * TC + s0 : lo;      // (dead lanes: distinct cells of the first row; they add 0)
                const float ml = in_tile ? m : 0.f;               // dead and far lanes contribute nothing on the main path
                const f32x2 L2 = {ly, lx}, MS = {ml, ml * S};
                const f32x2 W01 = {hy * hx, hy * lx}, W23 = {ly * hx, ly * lx};
                f32x2 gm2 = {0.f, 0.f}, gy2 = {0.f, 0.f}, gx2 = {0.f, 0.f};
                int* wq = gwin + pos0;
                float4 cr[2][4];   // both quads' corners up front: read inside the loop, the second quad's waited for the first quad's 16 atomics
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const float4* xq = xt + q * NPOS + pos0;
                    cr[q][0] = xq[0]; cr[q][1] = xq[1]; cr[q][2] = xq[TC]; cr[q][3] = xq[TC + 1];
                }
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const float4 a00 = cr[q][0], a01 = cr[q][1], a10 = cr[q][2], a11 = cr[q][3];
#pragma unroll
                    for (int ph = 0; ph < 2; ++ph) {       // channel pairs (2 pr, 2 pr + 1), pr = 2 q + ph
                        const int pr = 2 * q + ph;
                        const f32x2 c00 = ph ? f32x2{a00.z, a00.w} : f32x2{a00.x, a00.y};
                        const f32x2 c01 = ph ? f32x2{a01.z, a01.w} : f32x2{a01.x, a01.y};
                        const f32x2 c10 = ph ? f32x2{a10.z, a10.w} : f32x2{a10.x, a10.y};
                        const f32x2 c11 = ph ? f32x2{a11.z, a11.w} : f32x2{a11.x, a11.y};
                        const f32x2 cg = {acc[8 * s + 2 * pr], acc[8 * s + 2 * pr + 1]};
                        const f32x2 Bv = pk_sub(c01, c00), Cv = pk_sub(c10, c00), Dv = pk_sub(pk_sub(c11, c01), Cv);
                        const f32x2 dxv = pk_fma_x(L2, Dv, Bv), dyv = pk_fma_y(L2, Dv, Cv);   // d val / d x, d val / d y
                        const f32x2 val = pk_fma_y(L2, dxv, pk_fma_x(L2, Cv, c00));          // bilinear(x)
                        gm2 = pk_fma(cg, val, gm2);
                        const f32x2 tv = pk_mul_x(MS, cg);                                    // col_grad * mask
                        gy2 = pk_fma(dyv, tv, gy2);
                        gx2 = pk_fma(dxv, tv, gx2);
                        // ---- scatter: 8 LDS integer atomics per channel pair into the shared window (unconditional: dead lanes add 0)
                        const f32x2 ts = pk_mul_y(MS, cg);                                    // col_grad * mask * S
                        const f32x2 u00 = pk_fma_x(W01, ts, MAGIC), u01 = pk_fma_y(W01, ts, MAGIC);
                        const f32x2 u10 = pk_fma_x(W23, ts, MAGIC), u11 = pk_fma_y(W23, ts, MAGIC);
                        // (__float_as_uint, not __builtin_bit_cast(unsigned, u00.y): this hipcc compiles the bit_cast of a vector ELEMENT to element 0 -- /tmp test, r05_notes.md)
                        int* q0 = wq + (2 * pr) * NPOS;
                        int* q1 = q0 + NPOS;
                        lds_add_i32_6(q0, (int)(__float_as_uint(u00.x) - 0x4B400000u));
                        lds_add_i32_6(q0 + 1, (int)(__float_as_uint(u01.x) - 0x4B400000u));
                        lds_add_i32_6(q0 + TC, (int)(__float_as_uint(u10.x) - 0x4B400000u));
                        lds_add_i32_6(q0 + TC + 1, (int)(__float_as_uint(u11.x) - 0x4B400000u));
                        lds_add_i32_6(q1, (int)(__float_as_uint(u00.y) - 0x4B400000u));
                        lds_add_i32_6(q1 + 1, (int)(__float_as_uint(u01.y) - 0x4B400000u));
                        lds_add_i32_6(q1 + TC, (int)(__float_as_uint(u10.y) - 0x4B400000u));
                        lds_add_i32_6(q1 + TC + 1, (int)(__float_as_uint(u11.y) - 0x4B400000u));
                        if (pre && pr < KH && ks0 + pr < NK) {   // (compile time) one k-step of the next M tile
                            const int ks = ks0 + (pr < KH ? pr : 0);
                            acc_next = ks == 0 ? mfma_bf16_first(fh[pr < KH ? pr : 0], gh[0]) : mfma_bf16(fh[pr < KH ? pr : 0], gh[ks < NK ? ks : 0], acc_next);
                            if (TERMS >= 2) acc_next = mfma_bf16(fh[pr < KH ? pr : 0], gl[ks < NK ? ks : 0], acc_next);
                            if (TERMS >= 3) acc_next = mfma_bf16(fl[pr < KH ? pr : 0], gh[ks < NK ? ks : 0], acc_next);
                        }
                    }
                }
                float gm_s = gm2.x + gm2.y, gy_s = gy2.x + gy2.y, gx_s = gx2.x + gx2.y;
                gm_s = in_tile ? gm_s : 0.f;
                RVSR_STAMP(BI6_TL && chunk == 1, BI6_C1_ITER + 4 * it + 1);
                if (far) {   // ---- rare: the whole (pixel, tap) from global memory with the reference's rule set, plain arithmetic
                    const bool vy0 = yi >= 0, vy1 = yi + 1 <= d.H - 1, vx0 = xi >= 0, vx1 = xi + 1 <= d.W - 1;
                    const int cy0 = vy0 ? yi : 0, cy1 = vy1 ? yi + 1 : d.H - 1, cx0 = vx0 ? xi : 0, cx1 = vx1 ? xi + 1 : d.W - 1;
                    const int i00 = cy0 * d.W + cx0, i01 = cy0 * d.W + cx1, i10 = cy1 * d.W + cx0, i11 = cy1 * d.W + cx1;
                    const float z00 = (vy0 && vx0) ? 1.f : 0.f, z01 = (vy0 && vx1) ? 1.f : 0.f;
                    const float z10 = (vy1 && vx0) ? 1.f : 0.f, z11 = (vy1 && vx1) ? 1.f : 0.f;
                    const float w00 = hy * hx, w01 = hy * lx, w10 = ly * hx, w11 = ly * lx;
                    const float* pl = d.x + ((size_t)b * d.C + c0) * HW;
                    float* gp = p.gx + ((size_t)b * d.C + c0) * HW;
                    gm_s = gy_s = gx_s = 0.f;
                    // (all 32 loads in flight, no loop over the channels: a rolled `#pragma unroll 1` loop inside this divergent branch made dcn_bwdw6's
                    // results differ from run to run as soon as two waves shared a SIMD -- hipcc keeps its counter in a VGPR; profiles/r05_notes.md)
                    float u[8][4];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float* qp = pl + (size_t)e * HW;
                        u[e][0] = qp[i00]; u[e][1] = qp[i01]; u[e][2] = qp[i10]; u[e][3] = qp[i11];
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float c00 = u[e][0] * z00, c01 = u[e][1] * z01, c10 = u[e][2] * z10, c11 = u[e][3] * z11;
                        const float Bq = c01 - c00, Cq = c10 - c00, Dq = (c11 - c01) - Cq;
                        const float dxq = Bq + ly * Dq, dyq = Cq + lx * Dq, vq = (c00 + ly * Cq) + lx * dxq;
                        const float cgq = acc[8 * s + e], tq = cgq * m;
                        gm_s += cgq * vq;
                        gy_s += dyq * tq;
                        gx_s += dxq * tq;
                        float* gq = gp + (size_t)e * HW;
                        if (z00 * w00 != 0.f) atomicAdd(gq + i00, w00 * tq);
                        if (z01 * w01 != 0.f) atomicAdd(gq + i01, w01 * tq);
                        if (z10 * w10 != 0.f) atomicAdd(gq + i10, w10 * tq);
                        if (z11 * w11 != 0.f) atomicAdd(gq + i11, w11 * tq);
                    }
                }
                {   // grad_offset / grad_mask of (pixel, tap): this lane holds the sum over the chunk's 8 channels; dead lanes store beyond the view
                    if (d.mask_logit) gm_s *= m * (1.f - m);
                    const unsigned tp = (unsigned)tap * pl4;
                    const unsigned so = act_lane ? pix4 + 2u * tp : 0xfffffffcu, sm = act_lane ? pix4 + tp : 0xfffffffcu;
                    const unsigned go_ = (unsigned)(g * 18) * pl4, gk = (unsigned)(g * 9) * pl4;
                    if (first_of_group) {
                        buf_store(goff_rs, so, go_, gy_s);
                        buf_store(goff_rs, so, go_ + pl4, gx_s);
                        buf_store(gmsk_rs, sm, gk, gm_s);
                    } else if (act_lane) {   // a later chunk of the same deformable group (cpg > 8)
                        buf_store(goff_rs, so, go_, buf_load(goff_rs, so, go_) + gy_s);
                        buf_store(goff_rs, so, go_ + pl4, buf_load(goff_rs, so, go_ + pl4) + gx_s);
                        buf_store(gmsk_rs, sm, gk, buf_load(gmsk_rs, sm, gk) + gm_s);
                    }
                }
                if (G2 && chunk > 0) flush_commit(gwin_prev, c0 - 8, invS_prev, it * FRB, fv);
            }
        }
        RVSR_STAMP(BI6_TL && chunk < 4, BI6_CHUNK + 8 * chunk + 4);
        __syncthreads();
        RVSR_STAMP(BI6_TL && chunk < 4, BI6_CHUNK + 8 * chunk + 5);
        if (!W2) request_weights(cn, wsb);   // (one weight buffer: free now; in flight while the window is flushed, waited for at the top)
        if (W2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the DMA issued at the top of the iterations (hipcc does not count it); the loads behind it are a barrier old
        RVSR_STAMP(BI6_TL && chunk < 4, BI6_CHUNK + 8 * chunk + 6);
        if (!G2) flush_rows(gwin, c0, invS, 0, TR);   // (G2: during the next chunk's iterations / after the loop)
        invS_prev = invS;
        // (the barrier after the next commit orders this flush before the next chunk's atomics)
        RVSR_STAMP(BI6_TL && chunk < 4, BI6_CHUNK + 8 * chunk + 7);
    }
    if (G2) flush_rows(gwin0 + ((nchunks - 1) & 1) * 8 * NPOS, (nchunks - 1) * 8, invS_prev, 0, TR);   // (behind the last chunk's barrier)
    RVSR_STAMP(BI6_TL, BI6_END);
}

// Sampled statistic behind the halo selection of both DCN directions: every 16th row of every offset plane;
// cnt[0..5] = components with |v| > 2.5 / 3.5 / 5.5 / 7.5 / 8.5 / 11.5 px (DcnHaloSel).
__global__ void dcn_offset_probe2_kernel(const float* __restrict__ off, size_t off_bs, int B, int planes, int Ho, int Wo,
                                         unsigned* __restrict__ cnt) {
    const int nrow = (Ho + 15) / 16;
    const size_t total = (size_t)B * planes * nrow * Wo;
    const float lim[DCN_PROBE_COUNTERS] = {2.5f, 3.5f, 5.5f, 7.5f, 8.5f, 11.5f};
    unsigned n[DCN_PROBE_COUNTERS] = {0, 0, 0, 0, 0, 0};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wo);
        size_t r = i / Wo;
        const int row = (int)(r % nrow);
        r /= nrow;
        const int pl = (int)(r % planes), b = (int)(r / planes);
        const int y = row * 16 + 8 < Ho ? row * 16 + 8 : Ho - 1;
        const float v = fabsf(off[(size_t)b * off_bs + ((size_t)pl * Ho + y) * Wo + x]);
#pragma unroll
        for (int k = 0; k < DCN_PROBE_COUNTERS; ++k) n[k] += v > lim[k] ? 1u : 0u;
    }
#pragma unroll
    for (int k = 0; k < DCN_PROBE_COUNTERS; ++k)
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) n[k] += __shfl_xor(n[k], s);
    // one atomic per counter and BLOCK (per wave, 2 K blocks x 4 waves on the same few addresses took 226 us at 3 px offsets)
    __shared__ unsigned part[DCN_PROBE_COUNTERS][4];
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < DCN_PROBE_COUNTERS; ++k) part[k][wv] = n[k];
    }
    __syncthreads();
    if (threadIdx.x < DCN_PROBE_COUNTERS) {
        const unsigned t = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
        if (t) atomicAdd(cnt + threadIdx.x, t);
    }
}

// memset-free: the caller zeroes the counters (a fresh torch.zeros in the Python layer, hipMemsetAsync in the backward's own path)
void rvsr_launch_dcn_offset_probe(const DcnGeom& d, unsigned* cnt, hipStream_t st) {
    const int oplanes = (d.C / d.cpg) * 18;
    const size_t nprobe = dcn_probe_samples(d.B, d.C / d.cpg, d.Ho, d.Wo);
    const unsigned nb = (unsigned)((nprobe + 2047) / 2048 < 2048 ? (nprobe + 2047) / 2048 : 2048);
    hipLaunchKernelGGL(dcn_offset_probe2_kernel, dim3(nb ? nb : 1), dim3(256), 0, st, d.offset, d.off_bs, d.B, oplanes, d.Ho, d.Wo, cnt);
}

template <int NK, int R>
static int launch_bwdin6(const DcnBwdIn6Params& p, int nt, const bf16x8* wpack, hipStream_t st) {
    constexpr int TH = 8, TR = TH + 2 * R + 3, TC = 32 + 2 * R + 3, NPOS = TR * TC;
    constexpr size_t wbytes = (size_t)3 * 2 * (2 * NK) * 32 * 16;
    constexpr size_t lds1 = (size_t)NPOS * (2 * 16 + 8 * 4) + wbytes + 8 * sizeof(float);
    // 160 KB of LDS for ONE workgroup per CU: a second grad_input window first (the flush moves into the next chunk's iterations), then a
    // second weight buffer (the DMA moves to the top of the iterations) where they fit
    constexpr size_t gbytes = (size_t)NPOS * 8 * 4;
    // (NK = 8, the nf128 packs: the 48 KB weight block first -- measured at R = 5, where only one of the two fits: 4.01 against 4.21 ms)
    constexpr bool W2_FIRST = NK >= 8;
    constexpr bool G2 = lds1 + gbytes + (W2_FIRST && lds1 + wbytes <= 160 * 1024 ? wbytes : 0) <= 160 * 1024;
    constexpr bool W2 = lds1 + (G2 ? gbytes : 0) + wbytes <= 160 * 1024;
    constexpr size_t lds = lds1 + (G2 ? gbytes : 0) + (W2 ? wbytes : 0);
    constexpr int WPS = 2;   // waves per SIMD the launch bounds name: ONE 8-wave workgroup per CU (~220 registers per lane)
    auto k = dcn_bwdin6_kernel<NK, R, 3, WPS, W2, G2>;
    if constexpr (NK >= 4) {   // reduced-term products (gemm modes 2 / 3): the kernels of the nf64 / nf128 packs
        if (nt == 2) k = dcn_bwdin6_kernel<NK, R, 2, WPS, W2, G2>;
        if (nt == 1) k = dcn_bwdin6_kernel<NK, R, 1, WPS, W2, G2>;
    }
    if (set_lds(k, lds)) FAIL(RVSR_ERR_LAUNCH, "dcn_bwdin6: cannot reserve %zu B of LDS", lds);
    const DcnGeom& d = p.d;
    dim3 grid(d.ntx * ((d.Ho + TH - 1) / TH), 1, d.B);
    hipLaunchKernelGGL(k, grid, dim3(TH * 64), lds, st, p, wpack);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) FAIL(RVSR_ERR_LAUNCH, "dcn_bwdin6 launch: %s", hipGetErrorString(e));
    return RVSR_OK;
}

// The column norms and the packed weight image into the workspace, then one launch per candidate window of the plan; with more than one, each
// reads the offset counters (the caller's `probe`, else its own probe pass into the workspace) and returns at once unless it is the selected one.
int rvsr_launch_dcn_bwdin6(const DcnGeom& d, const DcnBwdPlan& q, const float* weight, const TView& g, float* gx, float* goff, size_t goff_bs,
                           float* gmask, size_t gmask_bs, void* workspace, const unsigned* probe, hipStream_t st) {
    const Bwdin6Workspace lay = bwdin6_workspace(d.Co, d.C);
    const int nchunks = (d.C + 7) / 8;
    bf16x8* wpack = (bf16x8*)workspace;
    float* wnorm = (float*)((unsigned char*)workspace + lay.wnorm);
    hipLaunchKernelGGL(dcn_bwd5_wnorm_kernel, dim3(nchunks), dim3(576), 0, st, weight, wnorm, d.Co, d.C, q.in_nt < 3 ? 1 : 0);
    const size_t total = (size_t)nchunks * 3 * (2 * q.nk) * 32;
    const dim3 pg((unsigned)((total + 255) / 256)), pb(256);
    switch (q.nk) {
        case 1: hipLaunchKernelGGL(pack_weights_bwd6_kernel<1>, pg, pb, 0, st, weight, wpack, d.Co, d.C, nchunks); break;
        case 2: hipLaunchKernelGGL(pack_weights_bwd6_kernel<2>, pg, pb, 0, st, weight, wpack, d.Co, d.C, nchunks); break;
        case 4: hipLaunchKernelGGL(pack_weights_bwd6_kernel<4>, pg, pb, 0, st, weight, wpack, d.Co, d.C, nchunks); break;
        default: hipLaunchKernelGGL(pack_weights_bwd6_kernel<8>, pg, pb, 0, st, weight, wpack, d.Co, d.C, nchunks); break;
    }
    DcnBwdIn6Params p;
    p.d = d; p.g = g; p.gx = gx; p.goff = goff; p.gmask = gmask; p.goff_bs = goff_bs; p.gmask_bs = gmask_bs;
    p.wnorm = wnorm;
    p.agt = q.handoff ? (bf16x8*)((unsigned char*)workspace + q.handoff_off) : nullptr;
    p.agt_nmb32 = 2 * ((d.Co + 63) / 64); p.agt_rows = ((d.Ho + 7) / 8) * 8;
    if (q.own_probe) {
        unsigned* cnt = (unsigned*)((unsigned char*)workspace + lay.probe);
        if (hipMemsetAsync(cnt, 0, DCN_PROBE_COUNTERS * sizeof(unsigned), st) != hipSuccess) FAIL(RVSR_ERR_LAUNCH, "dcn backward: memset of the probe counters failed");
        rvsr_launch_dcn_offset_probe(d, cnt, st);
        probe = cnt;
    }   // (else: the forward of this layer already counted these offsets, rvsr_dcn_pack_forward's probe)
    for (int k = 0; k < q.ncand; ++k) {
        p.sel = dcn_cand_sel(q.cand[k], probe);
        int rc = RVSR_ERR_LAUNCH;
#define BWDIN6(NK, R) case NK * 100 + R: rc = launch_bwdin6<NK, R>(p, q.in_nt, wpack, st); break
#define BWDIN6_TO8(NK) BWDIN6(NK, 2); BWDIN6(NK, 4); BWDIN6(NK, 5); BWDIN6(NK, 8)
        switch (q.nk * 100 + q.cand[k].halo) {   // the kernels that are built
            BWDIN6_TO8(1); BWDIN6(1, 12);
            BWDIN6_TO8(2); BWDIN6(2, 12);
            BWDIN6_TO8(4); BWDIN6(4, 12);
            BWDIN6_TO8(8);
            default: FAIL(RVSR_ERR_LAUNCH, "dcn_bwdin6: no kernel <%d, %d>", q.nk, q.cand[k].halo);
        }
#undef BWDIN6_TO8
#undef BWDIN6
        if (rc != RVSR_OK) return rc;
    }
    return RVSR_OK;
}

// ==========================================================================================================================================
// dcn_bwdw6: weight / bias gradient of the modulated DCN (the reference's im2col recompute + `gW += gOut col^T` GEMM + bias GEMV,
// deform_conv_cuda.cpp:647-671, kernel.cu:571-633), sixth generation.
//
// dcn_bwdw4 (dcn_bwdw4.inc) rebuilt the 72 x 128 column tile of a chunk in LDS through 2-byte stores, three barriers per tile, one
// workgroup per CU: 2.7 ms per L1 launch for the GEMM the forward does in 1.2 ms together with everything else.  Here
//   * lane (pixel, half) samples one (pixel, tap) for the chunk's 8 channels per lane iteration (the tap pairing of dcn_bwdin6), mask
//     folded into the four corner weights, packed f32 blend;
//   * the GEMM needs PIXELS along the MFMA's K (register) dimension for both operands, the sampling produces them along the LANE
//     dimension: the matrix core transposes.  D = A x [I16 | 0] (+ A' x [0 | I16]) with a 0/1 selector as B operand moves
//     A[i = pixel][k = column] into D[i = pixel][j = column], whose register layout is (lane = j, register = i) -- exact (one non-zero
//     product per output, f32 accumulate), no LDS tile, no 2-byte stores.  The pixel order along K is whatever the D layout makes it -- the
//     same for both operands, which is all a dot product needs;
//   * the other operand, gOut (x act') with pixels along K, comes pre-transposed from dcn_bwdin6 (bwd6_emit_agt: the same two instructions
//     on the gOut fragments that kernel holds anyway; one 16-byte vector per (row, x tile, 32 output channels, k-step, hi / lo, lane) in the
//     backward's workspace).  The two kernels run as a pair; a call that wants the weight gradient alone takes dcn_bwdw4.  The vectors of the
//     NEXT tile travel by LDS-DMA (no registers) into the wave's own slots as soon as its last MFMA of this tile has read them;
//   * chunk-major persistent schedule: a workgroup owns one (8-channel chunk, 64 output channels) unit and walks a contiguous range of
//     8 x 32 pixel tiles with the unit's 64 x 96 accumulator block in registers (96 per wave, a wave's own row of pixels as K); the units of a
//     tile stream sit on one XCD (they read the same operand vectors); deterministic partials at the end (rvsr_reduce_partials_kernel);
//   * ONE workgroup of 8 waves per CU.  Measured per L1 launch (B = 40, 64 -> 64 channels, 180 x 320): 1.90 ms against dcn_bwdw4's 2.80.
// Three things this kernel taught (profiles/r05_notes.md): the untied first MFMA of an accumulator must keep its operands alive
// (bf16x3.h: mfma_bf16_first); no rolled loop inside a divergent branch (the far path is unrolled: 32 loads in flight); two workgroups of four
// waves per CU gave run-to-run different weight gradients for a reason that was not found -- one workgroup per CU does not.
struct DcnBwdW6Params {
    DcnGeom d;
    const bf16x8* agt;  // gOut x act' as A operands, written by dcn_bwdin6 (bwd6_emit_agt): [b][row][x tile][mb32][ks][hi, lo][lane]
    int agt_nmb32, agt_rows;
    float* part;        // [ns][Co][C * 9] weight-gradient partials
    float* bpart;       // [ns][Co] bias-gradient partials (nullptr: not wanted)
    int ns;             // tile streams (= partials)
    int nty;            // tile rows of 8 output rows
    int ntiles;         // B * nty * ntx
    int nmb;            // units of 64 output channels
    int xcd_map;        // 1: units of a stream on one XCD (32 % (nchunks * nmb) == 0)
};

template <int R, int TERMS, int TH>
__global__ __launch_bounds__(TH * 64, 2) void dcn_bwdw6_kernel(const DcnBwdW6Params p) {
    constexpr int NT = TH * 64;
    constexpr int TR = TH + 2 * R + 3, TC = 32 + 2 * R + 3, NPOS = TR * TC;
    constexpr int NXI = (2 * NPOS + NT - 1) / NT;                  // x-tile items (float4 of one position and quad) per thread
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float4* xt = reinterpret_cast<float4*>(smem_raw);              // [2 quads][NPOS], zero outside the image
    bf16x8* agt = reinterpret_cast<bf16x8*>(xt + 2 * NPOS);        // [2][TH waves][8 vectors][64 lanes]: the wave's transposed gOut operands of this
                                                                   // and the next tile (kept out of the register file: the kernel sits at the
                                                                   // 256-register budget)
    const DcnGeom& d = p.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 31, hi = lane >> 5;
    const int nchunks = d.C >> 3, U = nchunks * p.nmb;
    // workgroup -> (tile stream, unit).  (Integer divisions run on the vector ALU; readfirstlane brings the uniform results back to SGPRs --
    // left in VGPRs they make every buffer descriptor "divergent": a waterfall loop around each buffer instruction.)
    const int L = blockIdx.x;
    const int unit = __builtin_amdgcn_readfirstlane(p.xcd_map ? (L >> 3) % U : L % U);
    const int stream = __builtin_amdgcn_readfirstlane(p.xcd_map ? (L & 7) + 8 * ((L >> 3) / U) : L / U);
    if (stream >= p.ns) return;   // (uniform)
    const int chunk = __builtin_amdgcn_readfirstlane(unit % nchunks), mbw = __builtin_amdgcn_readfirstlane(unit / nchunks);
    const int c0 = chunk * 8, g = c0 / d.cpg, o0 = 64 * mbw;
    const int t_begin = __builtin_amdgcn_readfirstlane((int)((long long)p.ntiles * stream / p.ns));
    const int t_end = __builtin_amdgcn_readfirstlane((int)((long long)p.ntiles * (stream + 1) / p.ns));
    const int per_b = p.nty * d.ntx;
    const unsigned HW = (unsigned)(d.H * d.W);
    const unsigned hw = (unsigned)(d.Ho * d.Wo);
    const unsigned pl4 = 4u * hw, HW4 = 4u * HW;

    // 0/1 selectors of the transposing MFMAs as B operands: lane (j = lo, h = hi) supplies B[k = 8 h + e][j], e < 8
    //   even: B[k][j] = (j == k), j < 16        odd: B[k][j] = (j == k + 16)
    bf16x8 sel_e, sel_o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        sel_e[e] = (__bf16)((lo == 8 * hi + e) ? 1.f : 0.f);
        sel_o[e] = (__bf16)((lo == 8 * hi + e + 16) ? 1.f : 0.f);
    }
    f32x16 gw_acc[2][3];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 3; ++nb) gw_acc[mb][nb] = zero16();

    float o_dy[5], o_dx[5], o_m[5];
    float xv[NXI][4];
    auto tile_coords = [&](int t, int& b, int& y0, int& x0) {
        b = __builtin_amdgcn_readfirstlane(t / per_b);
        const int rem = t - b * per_b, ty = __builtin_amdgcn_readfirstlane(rem / d.ntx);
        y0 = ty * TH;
        x0 = (rem - ty * d.ntx) * 32;
    };
    // Everything a tile reads from global memory is requested ONE TILE AHEAD (a tile is ~2 us of work for the workgroup, a round trip under
    // load about as much): the x tile into registers right after the previous one was committed to LDS, the operand vectors by LDS-DMA into
    // the other slot set, and the (dy, dx, mask) triple of lane iteration `it` into the registers iteration `it` of this tile has just
    // consumed.  (First version: all requests at the end of the tile, consumed at the top of the next: 1.90 ms per L1 launch.)
    const unsigned ob = (unsigned)(g * 18) * pl4, mb_ = (unsigned)(g * 9) * pl4;
    auto request_offsets = [&](int it, const __amdgpu_buffer_rsrc_t& off_rs, const __amdgpu_buffer_rsrc_t& msk_rs, unsigned pv) {
        const int t0 = bwd6_tap(it, 0), t1 = it < 4 ? bwd6_tap(it, 1) : t0;   // (it == 4, half 1: no tap; reads tap 8, unused)
        const unsigned tp = (unsigned)(hi ? t1 : t0) * pl4;
        o_dy[it] = buf_load(off_rs, pv + 2u * tp, ob);
        o_dx[it] = buf_load(off_rs, pv + 2u * tp, ob + pl4);
        o_m[it] = buf_load(msk_rs, pv + tp, mb_);
    };
    auto pixel_offset = [&](int y0, int x0) {   // (lanes without a pixel read the tile's first pixel: masked when used)
        const int oy = y0 + wave, ox = x0 + lo;
        return 4u * (unsigned)((oy < d.Ho && ox < d.Wo) ? oy * d.Wo + ox : y0 * d.Wo + x0);
    };
    // x-tile item k of this thread for the tile at (b, y0, x0): item = (quad, row, col), recomputed per tile (division by a constant: a handful of
    // instructions); a position outside the image (or no item) gets a lane offset beyond the 2 GB view, for which the buffer load returns 0
    auto request_x_item = [&](int k, int b, int y0, int x0) {
        const __amdgpu_buffer_rsrc_t x_rs = buf_view_2g(d.x + (size_t)b * d.C * HW);
        const int ty0 = y0 - d.pad - R, tx0 = x0 - d.pad - R;
        const int it = tid + k * NT;
        const int quad = it >= NPOS ? 1 : 0, pos = it - quad * NPOS;
        const int rr_ = pos / TC;
        const int gy = ty0 + rr_, gx = tx0 + (pos - rr_ * TC);
        const bool ok = it < 2 * NPOS && gy >= 0 && gy < d.H && gx >= 0 && gx < d.W;
        const unsigned xo = ok ? 4u * ((unsigned)(gy * d.W + gx) + (unsigned)(4 * quad) * HW) : 0x80000000u;
#pragma unroll
        for (int e = 0; e < 4; ++e) xv[k][e] = buf_load(x_rs, xo, (unsigned)(c0 + e) * HW4);
    };
    // operand vectors v0 .. v1 - 1 (of 8) of the wave for a tile by LDS-DMA (16 B per lane, no registers): lane l of the wave lands at its slot + 16 l
    auto fetch_ag = [&](int b, int y0, int x0, int set, int v0, int v1) {
        const bf16x8* src = p.agt + ((((size_t)b * p.agt_rows + (y0 + wave)) * d.ntx + (x0 >> 5)) * p.agt_nmb32 + 2 * mbw) * (size_t)(4 * 64) + lane;
        bf16x8* dst = agt + ((set * TH + wave) * 8) * 64 + lane;
#pragma unroll
        for (int v = v0; v < v1; ++v)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + v * 64),
                                             (__attribute__((address_space(3))) void*)(dst + v * 64), 16, 0, 0);
    };
    if (t_begin < t_end) {
        int b, y0, x0;
        tile_coords(t_begin, b, y0, x0);
        fetch_ag(b, y0, x0, 0, 0, 8);
#pragma unroll
        for (int k = 0; k < NXI; ++k) request_x_item(k, b, y0, x0);
        const __amdgpu_buffer_rsrc_t off_rs = buf_view(d.offset + (size_t)b * d.off_bs), msk_rs = buf_view(d.mask + (size_t)b * d.mask_bs);
        const unsigned pv = pixel_offset(y0, x0);
#pragma unroll
        for (int it = 0; it < 5; ++it) request_offsets(it, off_rs, msk_rs, pv);
    }

    for (int t = t_begin; t < t_end; ++t) {
        int b, y0, x0;
        tile_coords(t, b, y0, x0);
        const int ty0 = y0 - d.pad - R, tx0 = x0 - d.pad - R;
        const int oy = y0 + wave, ox = x0 + lo;
        const bool px_ok = oy < d.Ho && ox < d.Wo;
        const float by = (float)(oy - d.pad), bx = (float)(ox - d.pad);
        const int set = (t - t_begin) & 1;
        bf16x8* my_ag = agt + ((set * TH + wave) * 8) * 64 + lane;   // vector (mb, ks, part) at [(mb * 4 + ks * 2 + part) * 64]
        const bool tl = t == t_begin + 2;   // (timeline.h: the tile that is stamped)
        RVSR_STAMP(BW6_TL && tl, BW6_TILE + 0);
        // ---- this tile's operand vectors have landed (requested a tile ago; hipcc does not count LDS-DMA); commit the x tile
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        RVSR_STAMP(BW6_TL && tl, BW6_TILE + 1);
#pragma unroll
        for (int k = 0; k < NXI; ++k) {
            const int it = tid + k * NT;
            if (it < 2 * NPOS) xt[it] = make_float4(xv[k][0], xv[k][1], xv[k][2], xv[k][3]);
        }
        __syncthreads();
        RVSR_STAMP(BW6_TL && tl, BW6_TILE + 2);
        // ---- the next tile's requests (the last tile asks for itself again: unconditional loads keep hipcc's s_waitcnt bookkeeping simple).
        // They are issued a slice per lane iteration below, not as one burst here: 39 vector-memory instructions per wave in a row took 3.6 K of a
        // tile's 14 K cycles to ISSUE (the texture path takes ~100 cycles per instruction with eight waves asking at once) and the first iteration
        // then waited another 1.5 K behind them (profiles/r06_notes.md: timeline)
        int bn, y0n, x0n;
        tile_coords(t + 1 < t_end ? t + 1 : t, bn, y0n, x0n);
        const __amdgpu_buffer_rsrc_t off_rs_n = buf_view(d.offset + (size_t)bn * d.off_bs), msk_rs_n = buf_view(d.mask + (size_t)bn * d.mask_bs);
        const unsigned pv_n = pixel_offset(y0n, x0n);

        RVSR_STAMP(BW6_TL && tl, BW6_TILE + 3);
        f32x16 dt_h, dt_l;   // column values of two lane iterations, transposed: D[i = pixel][j = 16 (it & 1) + 8 h + ch]
#pragma unroll
        for (int it = 0; it < 5; ++it) {
            const int t0 = bwd6_tap(it, 0), t1 = it < 4 ? bwd6_tap(it, 1) : 0;
            const bool has_tap = it < 4 || hi == 0;
            const bool act_lane = px_ok && has_tap;
            RVSR_STAMP(BW6_TL && tl, BW6_ITER + 4 * it + 0);
            const float dy = act_lane ? o_dy[it] : 0.f, dx = act_lane ? o_dx[it] : 0.f;
            float m = o_m[it];
            request_offsets(it, off_rs_n, msk_rs_n, pv_n);   // (the registers just read: the next tile's triple of this iteration)
            if (it < 4) fetch_ag(bn, y0n, x0n, set ^ 1, 2 * it, 2 * it + 2);
#pragma unroll
            for (int k = it; k < NXI; k += 5) request_x_item(k, bn, y0n, x0n);   // (xv is free: committed to LDS above)
            if (d.mask_logit) m = __builtin_amdgcn_rcpf(1.f + __expf(-m));
            const float kyf = hi ? (float)(t1 / 3) : (float)(t0 / 3), kxf = hi ? (float)(t1 % 3) : (float)(t0 % 3);
            // sample position in IMAGE coordinates exactly as the reference forms it (kernel.cu:594-616)
            const float y = (by + kyf) + dy, x = (bx + kxf) + dx;
            const float fy = floorf(y), fx = floorf(x);
            const int yi = (int)fy, xi = (int)fx;
            const float ly = y - fy, lx = x - fx;
            const int r0 = yi - ty0, s0 = xi - tx0;
            const bool in_tile = act_lane && (unsigned)r0 < (unsigned)(TR - 1) && (unsigned)s0 < (unsigned)(TC - 1);
            const bool inside = y > -1.f && x > -1.f && y < (float)d.H && x < (float)d.W;
            const bool far = !in_tile && inside && act_lane;   // beyond the tile: global gather with the reference's rule set
            const int pos0 = in_tile ? r0 * TC + s0 : 0;
            const float ml = in_tile ? m : 0.f;               // dead and far lanes: zero column values on the main path
            // mask folded into the corner weights (the x tile is zero outside the image: no validity rules inside the tile)
            const float wy1 = ly * ml, wy0 = ml - wy1;
            const float w01 = wy0 * lx, w00 = wy0 - w01, w11 = wy1 * lx, w10 = wy1 - w11;
            const f32x2 W01 = {w00, w01}, W23 = {w10, w11};
            float colv[8];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float4* xq = xt + q * NPOS + pos0;
                const float4 a00 = xq[0], a01 = xq[1], a10 = xq[TC], a11 = xq[TC + 1];
#pragma unroll
                for (int ph = 0; ph < 2; ++ph) {
                    const f32x2 c00 = ph ? f32x2{a00.z, a00.w} : f32x2{a00.x, a00.y};
                    const f32x2 c01 = ph ? f32x2{a01.z, a01.w} : f32x2{a01.x, a01.y};
                    const f32x2 c10 = ph ? f32x2{a10.z, a10.w} : f32x2{a10.x, a10.y};
                    const f32x2 c11 = ph ? f32x2{a11.z, a11.w} : f32x2{a11.x, a11.y};
                    f32x2 r = pk_mul_x(W01, c00);
                    r = pk_fma_y(W01, c01, r);
                    r = pk_fma_x(W23, c10, r);
                    r = pk_fma_y(W23, c11, r);
                    colv[4 * q + 2 * ph] = r.x;
                    colv[4 * q + 2 * ph + 1] = r.y;
                }
            }
            if (far) {   // ---- rare: from global memory with the reference's rule set (kernel.cu:467-497)
                const bool vy0 = yi >= 0, vy1 = yi + 1 <= d.H - 1, vx0 = xi >= 0, vx1 = xi + 1 <= d.W - 1;
                const int cy0 = vy0 ? yi : 0, cy1 = vy1 ? yi + 1 : d.H - 1, cx0 = vx0 ? xi : 0, cx1 = vx1 ? xi + 1 : d.W - 1;
                const int i00 = cy0 * d.W + cx0, i01 = cy0 * d.W + cx1, i10 = cy1 * d.W + cx0, i11 = cy1 * d.W + cx1;
                const float hy = 1.f - ly, hx = 1.f - lx;
                const float u00 = (vy0 && vx0) ? hy * hx * m : 0.f, u01 = (vy0 && vx1) ? hy * lx * m : 0.f;
                const float u10 = (vy1 && vx0) ? ly * hx * m : 0.f, u11 = (vy1 && vx1) ? ly * lx * m : 0.f;
                const float* pl = d.x + ((size_t)b * d.C + c0) * HW;
                float q00[8], q01[8], q10[8], q11[8];   // (all 32 loads in flight; no loop over the channels: see profiles/r05_notes.md)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float* qp = pl + (size_t)e * HW;
                    q00[e] = qp[i00]; q01[e] = qp[i01]; q10[e] = qp[i10]; q11[e] = qp[i11];
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) colv[e] = u00 * q00[e] + u01 * q01[e] + u10 * q10[e] + u11 * q11[e];
            }
            RVSR_STAMP(BW6_TL && tl, BW6_ITER + 4 * it + 1);
            // (spare slot of iteration 4, half 1: the ones column of the bias gradient)
            if (it == 4) colv[0] = hi ? (px_ok ? 1.f : 0.f) : colv[0];
            bf16x8 ch_, cl_;
            split8(colv, ch_, cl_);
            if ((it & 1) == 0) {
                dt_h = mfma_bf16_first(ch_, sel_e);
                if (TERMS >= 2) dt_l = mfma_bf16_first(cl_, sel_e);
            } else {
                dt_h = mfma_bf16(ch_, sel_o, dt_h);
                if (TERMS >= 2) dt_l = mfma_bf16(cl_, sel_o, dt_l);
            }
            RVSR_STAMP(BW6_TL && tl, BW6_ITER + 4 * it + 2);
            if ((it & 1) || it == 4) {   // ---- n-block nb = it / 2 complete: gw_acc[mb][nb] += gOut^T[mb] x col, K = this row's 32 pixels
                const int nb = it >> 1;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const bf16x8 bh = pack8_exact(dt_h, 8 * ks);
                    bf16x8 bl = bh;
                    if (TERMS >= 2) bl = pack8_exact(dt_l, 8 * ks);
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb) {
                        const bf16x8 ah = my_ag[(mb * 4 + ks * 2) * 64];
                        gw_acc[mb][nb] = mfma_bf16(ah, bh, gw_acc[mb][nb]);
                        if (TERMS >= 2) gw_acc[mb][nb] = mfma_bf16(ah, bl, gw_acc[mb][nb]);
                        if (TERMS >= 3) gw_acc[mb][nb] = mfma_bf16(my_ag[(mb * 4 + ks * 2 + 1) * 64], bh, gw_acc[mb][nb]);
                    }
                }
            }
        }
        RVSR_STAMP(BW6_TL && tl, BW6_TILE + 4);
        __syncthreads();   // (every wave is done with the x tile)
        RVSR_STAMP(BW6_TL && tl, BW6_TILE + 5);
    }

    // ---- partial of this (stream, unit): sum of the waves (rows), fixed order, through LDS.  The last tile asked for itself again: that
    // LDS-DMA (and the x / offset loads) may still be in flight, hipcc does not count LDS-DMA, a barrier does not drain VMEM -- and `red` below
    // aliases the operand slots (rows of waves 6-7 overlap wave 0's set-0 slot at TH = 8): drain before the barrier (round-5 advisor finding).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    {
        float* red = reinterpret_cast<float*>(smem_raw);   // [TH waves][16 registers][64 lanes] = 16 / 32 KB (x tile + operand slots: free now)
        const int K = d.C * 9;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
            for (int nb = 0; nb < 3; ++nb) {
#pragma unroll
                for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * 64 + lane] = gw_acc[mb][nb][r];
                __syncthreads();
#pragma unroll
                for (int rq = 0; rq < 16 / TH; ++rq) {
                    const int r = wave + TH * rq;     // thread (wave, lane) sums register r of lane `lane` over the waves
                    float sum = 0.f;
#pragma unroll
                    for (int w4 = 0; w4 < TH; ++w4) sum += red[(w4 * 16 + r) * 64 + lane];
                    const int o = o0 + 32 * mb + drow(r, hi);
                    const int it = 2 * nb + (lo >> 4), h2 = (lo >> 3) & 1, ch = lo & 7;
                    const int tap = bwd6_tap(it, h2);
                    if (o < d.Co) {
                        if (tap >= 0) p.part[((size_t)stream * d.Co + o) * K + (size_t)(c0 + ch) * 9 + tap] = sum;
                        else if (it == 4 && h2 == 1 && ch == 0 && chunk == 0 && p.bpart != nullptr) p.bpart[(size_t)stream * d.Co + o] = sum;
                    }
                }
                __syncthreads();
            }
        }
    }
}

template <int R, int TH>
static int launch_bwdw6(const DcnGeom& d, const DcnBwdPlan& q, const void* agt, float* part, float* bpart, hipStream_t st) {
    DcnBwdW6Params p;
    p.d = d; p.agt = (const bf16x8*)agt; p.agt_nmb32 = 2 * q.nmb; p.agt_rows = ((d.Ho + 7) / 8) * 8;
    p.part = part; p.bpart = bpart;
    p.ns = q.ns; p.nty = (d.Ho + TH - 1) / TH; p.ntiles = d.B * p.nty * d.ntx; p.nmb = q.nmb; p.xcd_map = q.xcd;
    auto k = q.w_nt == 2 ? dcn_bwdw6_kernel<R, 2, TH> : (q.w_nt == 1 ? dcn_bwdw6_kernel<R, 1, TH> : dcn_bwdw6_kernel<R, 3, TH>);
    if (set_lds(k, q.w_lds)) FAIL(RVSR_ERR_LAUNCH, "dcn_bwdw6: cannot reserve %zu B of LDS", q.w_lds);
    hipLaunchKernelGGL(k, dim3(q.P * q.gy), dim3(TH * 64), q.w_lds, st, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) FAIL(RVSR_ERR_LAUNCH, "dcn_bwdw6 launch: %s", hipGetErrorString(e));
    return RVSR_OK;
}
int rvsr_launch_dcn_bwdw6(const DcnGeom& d, const DcnBwdPlan& q, const void* agt, float* part, float* bpart, hipStream_t st) {
    if (q.w_th == 4) return launch_bwdw6<2, 4>(d, q, agt, part, bpart, st);
    return launch_bwdw6<4, 8>(d, q, agt, part, bpart, st);
}
