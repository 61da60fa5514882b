// batch_kernels.hip -- the input side of a training step on the device (gfx950): packed uint8 frame crops -> the f32 [B, N, C, H, W] batch.
// One kernel does what the reference's data package does per sample on the host (codes/data/util.py:95 read_img's astype / 255,
// util.py:261-276 augment, RealVSR_dataset.py:333-341 stack + [2, 1, 0] + HWC -> CHW + ascontiguousarray):
//   src u8 [image][Hs][Ws][C] (image = sample * frames + frame), ANY byte alignment  ->  dst f32 [image][C][Ho][Wo]
//   a[y][x]   = s[vflip ? Hs-1-y : y][hflip ? Ws-1-x : x]          flags[sample] bit 0 hflip, bit 1 vflip
//   out[y][x] = rot90 ? a[x][y] : a[y][x]                           bit 2 rot90 (square crops only)
//   value     = float(u8) / 255.f, correctly rounded: a 256-entry table the workgroup builds with IEEE divisions (x * (1 / 255.f) differs
//               from numpy's x.astype(np.float32) / 255. on some of the 256 values)
//   RVSR_ASM_TO_YCBCR: the bytes are raw colour; planes (Y, Cb, Cr) = round-half-even((M . rgb + offset) / 255000) in exact integers,
//               the uint8 image scripts/prepare_data.py:42-45 stores, then the table.
// A workgroup owns one 64 x 64 tile of one output image.  Its source rectangle (<= 64 rows of <= 64 pixels, found from the flags) is
// staged in LDS as bytes with 16-byte loads ALIGNED DOWN: row r of the rectangle starts at byte address A_r, the loads cover the aligned
// blocks floor(A_r / 16) .. floor((A_r + len - 1) / 16), and segment byte j sits at LDS offset r * PITCH + (A_r & 15) + j.
// RULE (do not relax): no load is issued from an aligned 16-byte block that holds no byte of the rectangle.  A block that holds one is
// inside the same page as that byte, so reading its other bytes (neighbouring rows, the bytes before / after `src` in a larger
// allocation) cannot fault; those bytes reach LDS and are never read back.  Every store goes to an element of `dst` the tile owns.
// The read-out walks the OUTPUT row-major (four consecutive x per thread, 16-byte stores where Wo % 4 == 0), so both global sides are
// coalesced whatever the flags say; the transposition of rot90 happens in the LDS byte reads.
// rvsr_gather_clips is the same tile read from where the crop still sits in its whole frame: a data set decoded once into a resident
// store u8 [store_frames][H][W][C], and per sample a table row of store slots, crop origin and flags (gather_kernel below).
#include "glue_common.h"

// (a native vector type: an array of HIP's uint4 struct is not promoted to registers and leaves dead stores to scratch behind)
typedef unsigned asm_u32x4 __attribute__((ext_vector_type(4)));

#define ASM_T 64                  // tile edge in pixels
#define ASM_BLK 13                // 16-byte blocks per staged row: 64 px * 3 B = 192 B + up to 15 B of head
#define ASM_PITCH (16 * ASM_BLK)  // LDS bytes per staged row
#define ASM_LOADS ((ASM_T * ASM_BLK + 255) / 256)

// round-half-even(v / 255000) for v >= 0
__device__ __forceinline__ int div255000_rhe(int v) {
    int q = v / 255000;
    const int r = v - q * 255000;
    q += (r > 127500 || (r == 127500 && (q & 1))) ? 1 : 0;
    return q;
}

// The body both kernels share: one 64 x 64 tile of one Hs x Ws output image.  `origin` is the byte of source pixel (0, 0) of the image's
// Hs x Ws source rectangle and `row_bytes` the distance between two of its rows -- Ws * C for packed crops, the FRAME's W * C for a crop
// that still sits in its frame (gather_kernel).  Nothing else knows where the source is; the RULE above holds for any pitch, because the
// blocks a row loads are found from that row's own first and last byte.
template <int C, bool VEC>
__device__ __forceinline__ void assemble_tile(const unsigned char* __restrict__ origin, size_t row_bytes, float* __restrict__ out, int f,
                                              int Hs, int Ws, int mode, unsigned tile, unsigned tiles_x) {
    __shared__ asm_u32x4 stage4[ASM_T * ASM_BLK];
    __shared__ float tab[256];
    const unsigned char* stage = (const unsigned char*)stage4;
    const int tid = threadIdx.x;
    const bool hf = f & 1, vf = f & 2, rot = f & 4;
    const int Ho = Hs, Wo = Ws;   // (rot90 needs Hs == Ws: checked by the entry point)
    const int Y0 = (int)(tile / tiles_x) * ASM_T, X0 = (int)(tile % tiles_x) * ASM_T;
    const int Y1 = min(Y0 + ASM_T, Ho), X1 = min(X0 + ASM_T, Wo);
    // the tile in `a`, then in the source
    const int AY0 = rot ? X0 : Y0, AY1 = rot ? X1 : Y1, AX0 = rot ? Y0 : X0, AX1 = rot ? Y1 : X1;
    const int SY0 = vf ? Hs - AY1 : AY0, SX0 = hf ? Ws - AX1 : AX0;
    const int nr = AY1 - AY0, len = (AX1 - AX0) * C;   // rows of the rectangle, bytes per row: 1 .. 64, 1 .. 192
    const unsigned char* rect = origin + (size_t)SY0 * row_bytes + (size_t)SX0 * C;

    tab[tid] = __fdiv_rn((float)tid, 255.f);

    // stage: all loads first (branch-free: a slot beyond the rectangle repeats its last block, the one of a row its last block)
    asm_u32x4 v[ASM_LOADS];
    int at[ASM_LOADS];
#pragma unroll
    for (int i = 0; i < ASM_LOADS; ++i) {
        int idx = tid + 256 * i;
        idx = min(idx, nr * ASM_BLK - 1);
        const int r = idx / ASM_BLK;
        int k = idx - r * ASM_BLK;
        const uintptr_t A = (uintptr_t)(rect + (size_t)r * row_bytes);
        const uintptr_t first = A & ~(uintptr_t)15, last = (A + (uintptr_t)len - 1) & ~(uintptr_t)15;
        k = min(k, (int)((last - first) >> 4));
        v[i] = *(const asm_u32x4*)(first + 16 * (uintptr_t)k);
        at[i] = r * ASM_BLK + k;
    }
#pragma unroll
    for (int i = 0; i < ASM_LOADS; ++i) stage4[at[i]] = v[i];
    __syncthreads();

    const unsigned head0 = (unsigned)((uintptr_t)rect & 15), head_step = (unsigned)(row_bytes & 15);
    const size_t plane = (size_t)Ho * Wo;
    const bool rev = mode & 1, ycc = C == 3 && (mode & 2);
#pragma unroll
    for (int it = 0; it < ASM_T * ASM_T / 4 / 256; ++it) {
        const int q = tid + 256 * it;
        const int Y = Y0 + q / (ASM_T / 4), Xq = X0 + (q % (ASM_T / 4)) * 4;
        if (Y >= Y1 || Xq >= X1) continue;
        float val[C][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int X = min(Xq + j, X1 - 1);   // (a quad that crosses the right edge repeats the last pixel; not stored)
            const int ay = rot ? X : Y, ax = rot ? Y : X;
            const int r = (vf ? Hs - 1 - ay : ay) - SY0, cpx = (hf ? Ws - 1 - ax : ax) - SX0;
            const unsigned char* px = stage + r * ASM_PITCH + ((head0 + (unsigned)r * head_step) & 15) + cpx * C;
            if (ycc) {
                const int c0 = px[0], G = px[1], c2 = px[2];
                const int R = rev ? c2 : c0, B = rev ? c0 : c2;
                val[0][j] = tab[div255000_rhe(65481 * R + 128553 * G + 24966 * B + 16 * 255000)];
                val[C > 1 ? 1 : 0][j] = tab[div255000_rhe(-37797 * R - 74203 * G + 112000 * B + 128 * 255000)];
                val[C > 2 ? 2 : 0][j] = tab[div255000_rhe(112000 * R - 93786 * G - 18214 * B + 128 * 255000)];
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) val[c][j] = tab[px[rev ? C - 1 - c : c]];
            }
        }
        float* o = out + (size_t)Y * Wo + Xq;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (VEC) {   // Wo % 4 == 0: the quad is inside the row and 16-byte aligned
                *(float4*)(o + c * plane) = make_float4(val[c][0], val[c][1], val[c][2], val[c][3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (Xq + j < X1) o[c * plane + j] = val[c][j];
            }
        }
    }
}

template <int C, bool VEC>
__global__ void __launch_bounds__(256) assemble_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst,
                                                       const int* __restrict__ flags, int frames, int Hs, int Ws, int mode,
                                                       unsigned tiles_x, unsigned tiles) {
    const size_t image = blockIdx.x / tiles;
    const unsigned tile = blockIdx.x - (unsigned)image * tiles;
    const int f = flags ? flags[image / (size_t)frames] : 0;   // (uniform)
    const size_t row_bytes = (size_t)Ws * C;
    assemble_tile<C, VEC>(src + image * (size_t)Hs * row_bytes, row_bytes, dst + image * C * ((size_t)Hs * Ws), f, Hs, Ws, mode, tile,
                          tiles_x);
}

// The same tiles read out of a resident store u8 [store_frames][H][W][C]: row b of `table` (frames + 3 ints) names the store slot of
// every frame of sample b, then the crop's row, its column and the flags.  Slot and origin are CLAMPED into the store, so a wrong table
// gives wrong pixels, never a read outside it; every byte offset is a size_t (a store is tens of gigabytes).
template <int C, bool VEC>
__global__ void __launch_bounds__(256) gather_kernel(const unsigned char* __restrict__ store, float* __restrict__ dst,
                                                     const int* __restrict__ table, int frames, int store_frames, int H, int W, int S,
                                                     int mode, unsigned tiles_x, unsigned tiles) {
    const size_t image = blockIdx.x / tiles;
    const unsigned tile = blockIdx.x - (unsigned)image * tiles;
    const size_t b = image / (size_t)frames;
    const int* row = table + b * (size_t)(frames + 3);   // (uniform)
    const int slot = min(max(row[image - b * (size_t)frames], 0), store_frames - 1);
    const int y0 = min(max(row[frames], 0), H - S), x0 = min(max(row[frames + 1], 0), W - S);
    const size_t row_bytes = (size_t)W * C;
    const unsigned char* origin = store + ((size_t)slot * (size_t)H + (size_t)y0) * row_bytes + (size_t)x0 * C;
    assemble_tile<C, VEC>(origin, row_bytes, dst + image * C * ((size_t)S * S), row[frames + 2] & 7, S, S, mode, tile, tiles_x);
}

// ---------------------------------------------------------------- host side
// the one place that chooses the kernel: 1 = 16-byte stores (every output row starts on a 16-byte boundary), 0 = scalar stores
static int assemble_variant(const float* dst, int Wo) { return (Wo % 4 == 0 && ((uintptr_t)dst & 15) == 0) ? 1 : 0; }

static int assemble_args(const void* src, const void* dst, const void* flags, size_t samples, int frames, int C, int Hs, int Ws,
                         int mode, size_t* blocks) {
    if (!src || !dst) FAIL(RVSR_ERR_BAD_ARG, "assemble_clips: null argument");
    if (samples == 0 || frames <= 0 || Hs <= 0 || Ws <= 0)
        FAIL(RVSR_ERR_BAD_ARG, "assemble_clips: empty shape (%zu samples, %d frames, %d x %d)", samples, frames, Hs, Ws);
    if (((uintptr_t)dst & 3) != 0) FAIL(RVSR_ERR_BAD_ARG, "assemble_clips: dst is not aligned to its float32 elements");
    if (C != 1 && C != 3) FAIL(RVSR_ERR_UNSUPPORTED, "assemble_clips: %d channels (1 or 3)", C);
    if (mode & ~(RVSR_ASM_REVERSE | RVSR_ASM_TO_YCBCR)) FAIL(RVSR_ERR_UNSUPPORTED, "assemble_clips: mode %d", mode);
    if ((mode & RVSR_ASM_TO_YCBCR) && C != 3) FAIL(RVSR_ERR_UNSUPPORTED, "assemble_clips: the YCbCr conversion needs 3 channels");
    if (flags && Hs != Ws)
        FAIL(RVSR_ERR_UNSUPPORTED, "assemble_clips: flips / rot90 need square crops, got %d x %d (pass flags = NULL)", Hs, Ws);
    const size_t tiles = (size_t)((Hs + ASM_T - 1) / ASM_T) * (size_t)((Ws + ASM_T - 1) / ASM_T);
    if (tiles > 0x7fffffffu || samples * (size_t)frames > 0x7fffffffu / tiles)
        FAIL(RVSR_ERR_UNSUPPORTED, "assemble_clips: %zu images of %zu tiles exceed one launch", samples * (size_t)frames, tiles);
    *blocks = samples * (size_t)frames * tiles;
    return RVSR_OK;
}

extern "C" int rvsr_assemble_plan(const float* dst, size_t samples, int frames, int C, int Hs, int Ws, int* variant, int* blocks) {
    size_t nb = 0;
    const int rc = assemble_args(dst, dst, NULL, samples, frames, C, Hs, Ws, 0, &nb);
    if (rc != RVSR_OK) return rc;
    if (variant) *variant = assemble_variant(dst, Ws);
    if (blocks) *blocks = (int)nb;
    return RVSR_OK;
}

extern "C" int rvsr_assemble_clips(const unsigned char* src, float* dst, const int* flags, size_t samples, int frames, int C, int Hs,
                                   int Ws, int mode, void* stream) {
    size_t nb = 0;
    const int rc = assemble_args(src, dst, flags, samples, frames, C, Hs, Ws, mode, &nb);
    if (rc != RVSR_OK) return rc;
    const unsigned tiles_x = (unsigned)((Ws + ASM_T - 1) / ASM_T), tiles = tiles_x * (unsigned)((Hs + ASM_T - 1) / ASM_T);
    const int variant = assemble_variant(dst, Ws);
#define ASM_LAUNCH(CC, VV)                                                                                                         \
    hipLaunchKernelGGL((assemble_kernel<CC, VV>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, src, dst, flags, frames, Hs, \
                       Ws, mode, tiles_x, tiles)
    if (C == 3 && variant) ASM_LAUNCH(3, true);
    else if (C == 3) ASM_LAUNCH(3, false);
    else if (variant) ASM_LAUNCH(1, true);
    else ASM_LAUNCH(1, false);
#undef ASM_LAUNCH
    RETURN_LAUNCH("assemble_clips");
}

// (the plan has neither store nor table and passes dst in their place, as rvsr_assemble_plan does for src)
static int gather_args(const void* store, const void* table, const void* dst, size_t store_frames, int H, int W, size_t samples,
                       int frames, int C, int S, int mode, size_t* blocks) {
    if (!store || !table || !dst) FAIL(RVSR_ERR_BAD_ARG, "gather_clips: null argument");
    if (samples == 0 || frames <= 0 || store_frames == 0 || H <= 0 || W <= 0)
        FAIL(RVSR_ERR_BAD_ARG, "gather_clips: empty shape (%zu samples, %d frames, a store of %zu frames of %d x %d)", samples, frames,
             store_frames, H, W);
    if (store_frames > 0x7fffffffu) FAIL(RVSR_ERR_UNSUPPORTED, "gather_clips: %zu store frames (a slot is an int32)", store_frames);
    if (((uintptr_t)dst & 3) != 0) FAIL(RVSR_ERR_BAD_ARG, "gather_clips: dst is not aligned to its float32 elements");
    if (((uintptr_t)table & 3) != 0) FAIL(RVSR_ERR_BAD_ARG, "gather_clips: the table is not aligned to its int32 elements");
    if (C != 1 && C != 3) FAIL(RVSR_ERR_UNSUPPORTED, "gather_clips: %d channels (1 or 3)", C);
    if (S < 1 || S > H || S > W) FAIL(RVSR_ERR_BAD_ARG, "gather_clips: a crop of %d leaves the %d x %d frame", S, H, W);
    if (mode & ~(RVSR_ASM_REVERSE | RVSR_ASM_TO_YCBCR)) FAIL(RVSR_ERR_UNSUPPORTED, "gather_clips: mode %d", mode);
    if ((mode & RVSR_ASM_TO_YCBCR) && C != 3) FAIL(RVSR_ERR_UNSUPPORTED, "gather_clips: the YCbCr conversion needs 3 channels");
    const size_t tiles = (size_t)((S + ASM_T - 1) / ASM_T) * (size_t)((S + ASM_T - 1) / ASM_T);
    if (tiles > 0x7fffffffu || samples * (size_t)frames > 0x7fffffffu / tiles)
        FAIL(RVSR_ERR_UNSUPPORTED, "gather_clips: %zu images of %zu tiles exceed one launch", samples * (size_t)frames, tiles);
    *blocks = samples * (size_t)frames * tiles;
    return RVSR_OK;
}

extern "C" int rvsr_gather_plan(const float* dst, size_t samples, int frames, int C, int S, int* variant, int* blocks) {
    size_t nb = 0;
    const int rc = gather_args(dst, dst, dst, 1, S, S, samples, frames, C, S, 0, &nb);
    if (rc != RVSR_OK) return rc;
    if (variant) *variant = assemble_variant(dst, S);
    if (blocks) *blocks = (int)nb;
    return RVSR_OK;
}

extern "C" int rvsr_gather_clips(const unsigned char* store, size_t store_frames, int H, int W, const int* table, float* dst,
                                 size_t samples, int frames, int C, int S, int mode, void* stream) {
    size_t nb = 0;
    const int rc = gather_args(store, table, dst, store_frames, H, W, samples, frames, C, S, mode, &nb);
    if (rc != RVSR_OK) return rc;
    const unsigned tiles_x = (unsigned)((S + ASM_T - 1) / ASM_T), tiles = tiles_x * tiles_x;
    const int variant = assemble_variant(dst, S);
#define GAT_LAUNCH(CC, VV)                                                                                                          \
    hipLaunchKernelGGL((gather_kernel<CC, VV>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, store, dst, table, frames, \
                       (int)store_frames, H, W, S, mode, tiles_x, tiles)
    if (C == 3 && variant) GAT_LAUNCH(3, true);
    else if (C == 3) GAT_LAUNCH(3, false);
    else if (variant) GAT_LAUNCH(1, true);
    else GAT_LAUNCH(1, false);
#undef GAT_LAUNCH
    RETURN_LAUNCH("gather_clips");
}
