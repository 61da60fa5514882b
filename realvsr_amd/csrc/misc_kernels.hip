// misc_kernels.hip -- the HBM-bound pieces of the EDVR hot path (gfx950), one fused pass each:
//   * bilinear x2 / x4 upsampling (align_corners=False) with fused scale   EDVR_arch.py:111-124,194,200,316
//   * MaxPool2d(3,2,1) + AvgPool2d(3,2,1) written as one concatenated tensor   EDVR_arch.py:188-194
//   * TSA temporal attention: correlation + sigmoid + modulation              EDVR_arch.py:171-181
//   * TSA output: fea * sigmoid(att) * 2 + att_add                            EDVR_arch.py:204-207
//   * every reflect-padded 5x5 binomial stencil of the Laplacian pyramid: blur + ::2 select, zero-insert upsample + diff, and
//     conv_gauss / upsample as stand-alone operators                          utils/util.py:503-554
//   * YCbCr -> BGR uint8 for the inference path, the MFMA rate aid of bench.py, and the library's error string (rvsr_last_error)
// The scalar losses live in train_kernels.hip.
// All kernels: one thread per output element (the *_v4 kernels: 4 adjacent elements of a row, 16-byte accesses), lanes along W
// (coalesced), grid-stride loops.
// Backward kernels are gathers that re-evaluate the forward index map over a conservative
// candidate window (no atomics -> deterministic).
#define RVSR_DEFINE_REDUCE
#include "glue_common.h"

// ---------------------------------------------------------------- bilinear upsample
struct Lerp {
    int i0, i1;
    float l0, l1;
};
// source taps of destination index d for integer scale factor S (PyTorch area_pixel_compute_source_index)
__device__ __forceinline__ Lerp up_src(int d, int S, int n) {
    float s = ((float)d + 0.5f) / (float)S - 0.5f;
    if (s < 0.f) s = 0.f;
    Lerp r;
    r.i0 = (int)s;
    r.i1 = r.i0 + (r.i0 < n - 1 ? 1 : 0);
    r.l1 = s - (float)r.i0;
    r.l0 = 1.f - r.l1;
    return r;
}

__global__ void upsample_fwd_kernel(const float* __restrict__ in, float* __restrict__ out, size_t planes, int H, int W,
                                    int S, float scale) {
    const int Ho = H * S, Wo = W * S;
    const size_t n = planes * Ho * Wo;
    LOOP(i, n) {
        const int ox = (int)(i % Wo);
        const int oy = (int)((i / Wo) % Ho);
        const size_t pl = i / ((size_t)Wo * Ho);
        const Lerp ly = up_src(oy, S, H), lx = up_src(ox, S, W);
        const float* p = in + pl * H * W;
        const float v = ly.l0 * (lx.l0 * p[ly.i0 * W + lx.i0] + lx.l1 * p[ly.i0 * W + lx.i1]) +
                        ly.l1 * (lx.l0 * p[ly.i1 * W + lx.i0] + lx.l1 * p[ly.i1 * W + lx.i1]);
        out[i] = v * scale;
    }
}

__global__ void upsample_bwd_kernel(const float* __restrict__ gout, float* __restrict__ gin, size_t planes, int H,
                                    int W, int S, float scale) {
    const int Ho = H * S, Wo = W * S;
    const size_t n = planes * H * W;
    LOOP(i, n) {
        const int ix = (int)(i % W);
        const int iy = (int)((i / W) % H);
        const size_t pl = i / ((size_t)W * H);
        const float* g = gout + pl * Ho * Wo;
        // outputs that can read input row iy: for S = 2 exactly rows 2iy-1 .. 2iy+2 (source coordinate oy/2 - 1/4);
        // other factors use a conservative window, rows outside get weight 0 below
        const int e_lo = S == 2 ? 1 : 2 * S, e_hi = S == 2 ? 2 : 2 * S;
        const int oy_lo = max(0, S * iy - e_lo), oy_hi = min(Ho - 1, S * iy + e_hi);
        const int ox_lo = max(0, S * ix - e_lo), ox_hi = min(Wo - 1, S * ix + e_hi);
        float acc = 0.f;
        for (int oy = oy_lo; oy <= oy_hi; ++oy) {
            const Lerp ly = up_src(oy, S, H);
            const float wy = (ly.i0 == iy ? ly.l0 : 0.f) + (ly.i1 == iy ? ly.l1 : 0.f);
            if (wy == 0.f) continue;
            float rowacc = 0.f;
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                const Lerp lx = up_src(ox, S, W);
                const float wx = (lx.i0 == ix ? lx.l0 : 0.f) + (lx.i1 == ix ? lx.l1 : 0.f);
                rowacc += wx * g[(size_t)oy * Wo + ox];
            }
            acc += wy * rowacc;
        }
        gin[i] = acc * scale;
    }
}

// x2 specialisations (every upsample of the alignment stage: EDVR_arch.py:111-124): one thread per INPUT pixel, 32-bit index
// math, constant weights.  Output rows 2y / 2y+1 read input rows (y-1, y) / (y, y+1) with weights (1/4, 3/4) / (3/4, 1/4); at
// the borders the clamped source index folds the outer weight onto the edge row.  The generic kernels above (64-bit div/mod per
// output element, per-element float divisions, 4x4 candidate scan) ran at 0.5 / 0.7 ms on the 40 x 64 x 90 x 160 -> 180 x 320
// tensors against a 0.14 ms HBM floor.
__global__ void upsample2_fwd_kernel(const float* __restrict__ in, float* __restrict__ out, unsigned planes, int H, int W, float scale) {
    const unsigned n = planes * (unsigned)(H * W);
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned pl = i / (unsigned)(H * W), rem = i - pl * (unsigned)(H * W);
        const int y = (int)(rem / (unsigned)W), x = (int)(rem - (unsigned)y * W);
        const float* p = in + (size_t)pl * H * W;
        const int ym = y > 0 ? y - 1 : 0, yp = y < H - 1 ? y + 1 : H - 1;
        const int xm = x > 0 ? x - 1 : 0, xp = x < W - 1 ? x + 1 : W - 1;
        const float a00 = p[ym * W + xm], a01 = p[ym * W + x], a02 = p[ym * W + xp];
        const float a10 = p[y * W + xm], a11 = p[y * W + x], a12 = p[y * W + xp];
        const float a20 = p[yp * W + xm], a21 = p[yp * W + x], a22 = p[yp * W + xp];
        // same association as the generic kernel: ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11)
        const float wA0 = y > 0 ? 0.25f : 0.f, wA1 = y > 0 ? 0.75f : 1.f;           // output row 2y: rows (y-1, y)
        const float wB0 = 0.75f, wB1 = 0.25f;                                           // output row 2y+1: rows (y, y+1 clamped)
        const float uA0 = x > 0 ? 0.25f : 0.f, uA1 = x > 0 ? 0.75f : 1.f;            // output col 2x: cols (x-1, x)
        const float uB0 = 0.75f, uB1 = 0.25f;                                           // output col 2x+1: cols (x, x+1 clamped)
        float2 r0, r1;
        r0.x = (wA0 * (uA0 * a00 + uA1 * a01) + wA1 * (uA0 * a10 + uA1 * a11)) * scale;
        r0.y = (wA0 * (uB0 * a01 + uB1 * a02) + wA1 * (uB0 * a11 + uB1 * a12)) * scale;
        r1.x = (wB0 * (uA0 * a10 + uA1 * a11) + wB1 * (uA0 * a20 + uA1 * a21)) * scale;
        r1.y = (wB0 * (uB0 * a11 + uB1 * a12) + wB1 * (uB0 * a21 + uB1 * a22)) * scale;
        float* o = out + (size_t)pl * 4 * H * W + (size_t)(2 * y) * (2 * W) + 2 * x;
        *reinterpret_cast<float2*>(o) = r0;
        *reinterpret_cast<float2*>(o + 2 * W) = r1;
    }
}
// adjoint: input pixel (y, x) collects output rows 2y-1 .. 2y+2 with weights (1/4, 3/4, 3/4, 1/4), edge rows folded as above
__global__ void upsample2_bwd_kernel(const float* __restrict__ gout, float* __restrict__ gin, unsigned planes, int H, int W, float scale) {
    const unsigned n = planes * (unsigned)(H * W);
    const int Wo = 2 * W;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned pl = i / (unsigned)(H * W), rem = i - pl * (unsigned)(H * W);
        const int y = (int)(rem / (unsigned)W), x = (int)(rem - (unsigned)y * W);
        const float* g = gout + (size_t)pl * 4 * H * W;
        const float wy[4] = {y > 0 ? 0.25f : 0.f, y > 0 ? 0.75f : 1.f, y < H - 1 ? 0.75f : 1.f, y < H - 1 ? 0.25f : 0.f};
        const float wx[4] = {x > 0 ? 0.25f : 0.f, x > 0 ? 0.75f : 1.f, x < W - 1 ? 0.75f : 1.f, x < W - 1 ? 0.25f : 0.f};
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            int oy = 2 * y - 1 + a;
            oy = oy < 0 ? 0 : (oy > 2 * H - 1 ? 2 * H - 1 : oy);    // clamped rows carry weight 0
            const float* row = g + (size_t)oy * Wo;
            const float2 mid = *reinterpret_cast<const float2*>(row + 2 * x);        // cols 2x, 2x+1 (8-byte aligned)
            const float l = row[x > 0 ? 2 * x - 1 : 0], r = row[x < W - 1 ? 2 * x + 2 : Wo - 1];
            acc += wy[a] * (wx[0] * l + wx[1] * mid.x + wx[2] * mid.y + wx[3] * r);
        }
        gin[i] = acc * scale;
    }
}

// Backward with W % 4 == 0 and 16-byte aligned pointers: one thread per FOUR adjacent input pixels of a row, the four output rows as
// two 16-byte loads plus the two neighbours each, one 16-byte store, two 32-bit divisions per thread instead of two per pixel:
// 0.255 against 0.309 ms on 40 x 64 x 180 x 320 -> 90 x 160.  (The forward stays on the float2 kernel.  Two 16-byte forms of it were
// built and measured against its 0.216 ms on 40 x 64 x 90 x 160: four pixels per thread, 2 x 8 outputs as four 16-byte stores, 0.224 ms
// -- a lane then owns 32 bytes of a row and a store instruction fills every other 16 bytes of its span; two pixels per thread, two
// contiguous 16-byte stores, 0.214 ms there but 6 % slower over the step's 48 launches.  profiles/r12_notes.md section 5.)
// ARITHMETIC: the float2 kernel above leaves it to the compiler which product of a sum a * b + c * d is fused into the add and which
// is rounded first, and what it chose (read from its gfx950 code) is not uniform over the terms.  The results of that kernel are
// the library's results, so the v4 kernel spells that choice out -- fmaf where the float2 code fuses, a rounded product where it
// does not, contraction off -- and gives the same bits on any input (tests/test_gpu_glue_vector.py compares the two on random values).
__global__ void upsample2_bwd_v4_kernel(const float* __restrict__ gout, float* __restrict__ gin, unsigned planes, int H, int W, float scale) {
#pragma clang fp contract(off)
    const unsigned W4 = (unsigned)W >> 2, n = planes * (unsigned)H * W4;
    const int Wo = 2 * W;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned row = i / W4, pl = row / (unsigned)H;
        const int x0 = (int)((i - row * W4) << 2), y = (int)(row - pl * (unsigned)H);
        const float* g = gout + (size_t)pl * 4 * H * W;
        const float wy[4] = {y > 0 ? 0.25f : 0.f, y > 0 ? 0.75f : 1.f, y < H - 1 ? 0.75f : 1.f, y < H - 1 ? 0.25f : 0.f};
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            int oy = 2 * y - 1 + a;
            oy = oy < 0 ? 0 : (oy > 2 * H - 1 ? 2 * H - 1 : oy);    // clamped rows carry weight 0
            const float* q = g + (size_t)oy * Wo + 2 * x0;
            const float4 m0 = reinterpret_cast<const float4*>(q)[0], m1 = reinterpret_cast<const float4*>(q)[1];
            // cols 2 x0 - 1 .. 2 x0 + 8; the two outer ones clamp onto the row's ends, where their weight is 0
            const float c[10] = {q[x0 > 0 ? -1 : 0], m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, q[x0 + 4 < W ? 8 : 7]};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = x0 + k;
                const float wx0 = x > 0 ? 0.25f : 0.f, wx1 = x > 0 ? 0.75f : 1.f, wx2 = x < W - 1 ? 0.75f : 1.f, wx3 = x < W - 1 ? 0.25f : 0.f;
                // the float2 kernel's row sum: rows 2y - 1 .. 2y + 1 round wx2 * c before adding it, row 2y + 2 fuses it
                const float s01 = fmaf(wx1, c[2 * k + 1], wx0 * c[2 * k]);
                const float s012 = a < 3 ? wx2 * c[2 * k + 2] + s01 : fmaf(wx2, c[2 * k + 2], s01);
                acc[k] = fmaf(wy[a], fmaf(wx3, c[2 * k + 3], s012), acc[k]);
            }
        }
        *reinterpret_cast<float4*>(gin + (size_t)row * W + x0) = make_float4(acc[0] * scale, acc[1] * scale, acc[2] * scale, acc[3] * scale);
    }
}

// ---------------------------------------------------------------- max+avg pool 3/2/1 -> cat
__global__ void pool_fwd_kernel(const float* __restrict__ in, float* __restrict__ out, unsigned char* __restrict__ arg,
                                int B, int C, int H, int W, int Ho, int Wo) {
    const size_t n = (size_t)B * C * Ho * Wo;
    LOOP(i, n) {
        const int ox = (int)(i % Wo);
        const int oy = (int)((i / Wo) % Ho);
        const int c = (int)((i / ((size_t)Wo * Ho)) % C);
        const int b = (int)(i / ((size_t)Wo * Ho * C));
        const float* p = in + ((size_t)b * C + c) * H * W;
        float mx = -INFINITY, sum = 0.f;
        int am = 0;
        bool first = true;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int y = 2 * oy - 1 + t / 3, x = 2 * ox - 1 + t % 3;
            if (y < 0 || y >= H || x < 0 || x >= W) continue;
            const float v = p[(size_t)y * W + x];
            sum += v;
            if (first || v > mx || v != v) {
                mx = v;
                am = t;
                first = false;
            }
        }
        const size_t hw = (size_t)Ho * Wo;
        const size_t pix = (size_t)oy * Wo + ox;
        out[((size_t)b * 2 * C + c) * hw + pix] = mx;
        out[((size_t)b * 2 * C + C + c) * hw + pix] = sum * (1.f / 9.f);  // count_include_pad=True
        arg[i] = (unsigned char)am;
    }
}

__global__ void pool_bwd_kernel(const float* __restrict__ gout, const unsigned char* __restrict__ arg,
                                float* __restrict__ gin, int B, int C, int H, int W, int Ho, int Wo) {
    const size_t n = (size_t)B * C * H * W;
    LOOP(i, n) {
        const int x = (int)(i % W);
        const int y = (int)((i / W) % H);
        const int c = (int)((i / ((size_t)W * H)) % C);
        const int b = (int)(i / ((size_t)W * H * C));
        const size_t hw = (size_t)Ho * Wo;
        const float* gm = gout + ((size_t)b * 2 * C + c) * hw;
        const float* ga = gout + ((size_t)b * 2 * C + C + c) * hw;
        const unsigned char* a = arg + ((size_t)b * C + c) * hw;
        float acc = 0.f;
        for (int oy = y / 2; oy <= (y + 1) / 2; ++oy) {
            if (oy >= Ho) continue;
            for (int ox = x / 2; ox <= (x + 1) / 2; ++ox) {
                if (ox >= Wo) continue;
                const int t = (y - (2 * oy - 1)) * 3 + (x - (2 * ox - 1));
                const size_t pix = (size_t)oy * Wo + ox;
                acc += ga[pix] * (1.f / 9.f);
                if (a[pix] == t) acc += gm[pix];
            }
        }
        gin[i] = acc;
    }
}

// W % 8 == 0 (forward) / W % 4 == 0 (backward) and 16-byte aligned pointers, fewer than 2^31 elements: one thread per FOUR adjacent
// outputs (forward) or inputs (backward) of a row, 32-bit indices.  Forward: the three source rows as two 16-byte loads plus the left
// neighbour, both halves and the argmax written as 16- / 4-byte stores.  Taps are visited in the scan order of the kernels above
// (first maximum wins, a NaN wins, the sum adds in that order), so the results are theirs bit for bit.
__global__ void pool_fwd_v4_kernel(const float* __restrict__ in, float* __restrict__ out, unsigned char* __restrict__ arg,
                                   int B, int C, int H, int W, int Ho, int Wo) {
    const unsigned Wq = (unsigned)Wo >> 2, n = (unsigned)B * C * Ho * Wq;
    const unsigned hw = (unsigned)Ho * Wo;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned row = i / Wq, pl = row / (unsigned)Ho, b = pl / (unsigned)C;
        const int ox0 = (int)((i - row * Wq) << 2), oy = (int)(row - pl * (unsigned)Ho), c = (int)(pl - b * (unsigned)C);
        const float* p = in + (size_t)pl * H * W;
        float v[3][9];      // rows 2 oy - 1 .. 2 oy + 1, cols 2 ox0 - 1 .. 2 ox0 + 7 (all inside the row but col -1)
        bool rowok[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int y = 2 * oy - 1 + r;
            rowok[r] = y >= 0 && y < H;
            const float* q = p + (size_t)(rowok[r] ? y : 2 * oy) * W + 2 * ox0;
            const float4 m0 = reinterpret_cast<const float4*>(q)[0], m1 = reinterpret_cast<const float4*>(q)[1];
            v[r][0] = q[ox0 > 0 ? -1 : 0];
            v[r][1] = m0.x, v[r][2] = m0.y, v[r][3] = m0.z, v[r][4] = m0.w;
            v[r][5] = m1.x, v[r][6] = m1.y, v[r][7] = m1.z, v[r][8] = m1.w;
        }
        float mxs[4], avs[4];
        unsigned ams = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float mx = -INFINITY, sum = 0.f;
            int am = 0;
            bool first = true;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                if (!rowok[t / 3] || (t % 3 == 0 && ox0 + k == 0)) continue;
                const float u = v[t / 3][2 * k + t % 3];
                sum += u;
                if (first || u > mx || u != u) {
                    mx = u;
                    am = t;
                    first = false;
                }
            }
            mxs[k] = mx;
            avs[k] = sum * (1.f / 9.f);  // count_include_pad=True
            ams |= (unsigned)am << (8 * k);
        }
        const unsigned pix = (unsigned)oy * Wo + ox0;
        *reinterpret_cast<float4*>(out + ((size_t)b * 2 * C + c) * hw + pix) = make_float4(mxs[0], mxs[1], mxs[2], mxs[3]);
        *reinterpret_cast<float4*>(out + ((size_t)b * 2 * C + C + c) * hw + pix) = make_float4(avs[0], avs[1], avs[2], avs[3]);
        *reinterpret_cast<unsigned*>(arg + (size_t)pl * hw + pix) = ams;
    }
}
// inputs x0 .. x0 + 3 of row y read the outputs x0 / 2 .. x0 / 2 + 2 of rows y / 2 .. (y + 1) / 2
__global__ void pool_bwd_v4_kernel(const float* __restrict__ gout, const unsigned char* __restrict__ arg,
                                   float* __restrict__ gin, int B, int C, int H, int W, int Ho, int Wo) {
#pragma clang fp contract(off)
    const unsigned W4 = (unsigned)W >> 2, n = (unsigned)B * C * H * W4;
    const unsigned hw = (unsigned)Ho * Wo;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned row = i / W4, pl = row / (unsigned)H, b = pl / (unsigned)C;
        const int x0 = (int)((i - row * W4) << 2), y = (int)(row - pl * (unsigned)H), c = (int)(pl - b * (unsigned)C);
        const float* gm = gout + ((size_t)b * 2 * C + c) * hw;
        const float* ga = gout + ((size_t)b * 2 * C + C + c) * hw;
        const unsigned char* a = arg + (size_t)pl * hw;
        const int o0 = x0 >> 1;
        const bool third = o0 + 2 < Wo;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int oy = y / 2; oy <= (y + 1) / 2; ++oy) {
            if (oy >= Ho) continue;
            const unsigned pix = (unsigned)oy * Wo + o0;
            const float2 m2 = *reinterpret_cast<const float2*>(gm + pix), a2 = *reinterpret_cast<const float2*>(ga + pix);
            const unsigned short t2 = *reinterpret_cast<const unsigned short*>(a + pix);
            const float m[3] = {m2.x, m2.y, third ? gm[pix + 2] : 0.f}, av[3] = {a2.x, a2.y, third ? ga[pix + 2] : 0.f};
            const int ts[3] = {t2 & 255, t2 >> 8, third ? a[pix + 2] : 255};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = x0 + k;
#pragma unroll
                for (int j = k / 2; j <= (k + 1) / 2; ++j) {       // ox = o0 + j, ascending as above
                    if (j == 2 && !third) continue;
                    const int t = (y - (2 * oy - 1)) * 3 + (x - (2 * (o0 + j) - 1));
                    acc[k] = fmaf(av[j], 1.f / 9.f, acc[k]);      // (fused, as pool_bwd_kernel's `acc += ga * (1 / 9)` is)
                    if (ts[j] == t) acc[k] += m[j];
                }
            }
        }
        *reinterpret_cast<float4*>(gin + (size_t)row * W + x0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
}

// ---------------------------------------------------------------- TSA temporal attention
__global__ void tsa_corr_fwd_kernel(const float* __restrict__ emb, const float* __restrict__ emb_ref,
                                    const float* __restrict__ aligned, float* __restrict__ mod,
                                    float* __restrict__ prob, int B, int N, int C, size_t HW, int frame_major) {
    const size_t n = (size_t)B * N * HW;
    LOOP(i, n) {
        const size_t px = i % HW;
        const int f = (int)((i / HW) % N);
        const int b = (int)(i / (HW * N));
        // emb / aligned: [B][N] (the reference's stack(dim=1)) or frame-major [N][B] (the PCD batch as it is); mod / prob: [B][N]
        const size_t fb = frame_major ? (size_t)f * B + b : (size_t)b * N + f;
        const float* e = emb + (fb * C) * HW + px;
        const float* r = emb_ref + ((size_t)b * C) * HW + px;
        float cor = 0.f;
        for (int c = 0; c < C; ++c) cor += e[(size_t)c * HW] * r[(size_t)c * HW];
        const float pr = 1.f / (1.f + __expf(-cor));
        prob[i] = pr;
        const float* a = aligned + (fb * C) * HW + px;
        float* m = mod + (((size_t)b * N + f) * C) * HW + px;
        for (int c = 0; c < C; ++c) m[(size_t)c * HW] = a[(size_t)c * HW] * pr;
    }
}

#define TSA_MAXN 8
__global__ void tsa_corr_bwd_kernel(const float* __restrict__ gmod, const float* __restrict__ emb,
                                    const float* __restrict__ emb_ref, const float* __restrict__ aligned,
                                    const float* __restrict__ prob, float* __restrict__ galigned,
                                    float* __restrict__ gemb, float* __restrict__ gemb_ref, int B, int N, int C,
                                    size_t HW, int frame_major) {
    const size_t n = (size_t)B * HW;
    LOOP(i, n) {
        const size_t px = i % HW;
        const int b = (int)(i / HW);
        float gcor[TSA_MAXN];
        for (int f = 0; f < N; ++f) {
            const size_t base = (((size_t)b * N + f) * C) * HW + px;                                      // gmod: [B][N]
            const size_t bin = ((frame_major ? (size_t)f * B + b : (size_t)b * N + f) * C) * HW + px;     // aligned / galigned
            const float pr = prob[((size_t)b * N + f) * HW + px];
            float gp = 0.f;
            for (int c = 0; c < C; ++c) {
                const float g = gmod[base + (size_t)c * HW];
                gp += g * aligned[bin + (size_t)c * HW];
                galigned[bin + (size_t)c * HW] = g * pr;
            }
            gcor[f] = gp * pr * (1.f - pr);
        }
        const float* r = emb_ref + ((size_t)b * C) * HW + px;
        for (int c = 0; c < C; ++c) {
            const float rv = r[(size_t)c * HW];
            float s = 0.f;
            for (int f = 0; f < N; ++f) {
                const size_t idx = ((frame_major ? (size_t)f * B + b : (size_t)b * N + f) * C + c) * HW + px;
                s += gcor[f] * emb[idx];
                gemb[idx] = gcor[f] * rv;
            }
            gemb_ref[((size_t)b * C + c) * HW + px] = s;
        }
    }
}

__global__ void tsa_final_fwd_kernel(const float* __restrict__ fea, const float* __restrict__ att,
                                     const float* __restrict__ add, float* __restrict__ out, size_t n) {
    LOOP(i, n) {
        const float s = 1.f / (1.f + __expf(-att[i]));
        out[i] = fea[i] * s * 2.f + add[i];
    }
}
__global__ void tsa_final_bwd_kernel(const float* __restrict__ g, const float* __restrict__ fea,
                                     const float* __restrict__ att, float* __restrict__ gfea,
                                     float* __restrict__ gatt, size_t n) {
    LOOP(i, n) {
        const float s = 1.f / (1.f + __expf(-att[i]));
        const float gi = g[i];
        gfea[i] = gi * s * 2.f;
        gatt[i] = gi * fea[i] * 2.f * s * (1.f - s);
    }
}

// ---------------------------------------------------------------- Laplacian pyramid
__device__ __forceinline__ int reflect(int q, int n) { return q < 0 ? -q : (q >= n ? 2 * (n - 1) - q : q); }
__device__ __forceinline__ float binom(int i) { return i == 0 || i == 4 ? 1.f : (i == 2 ? 6.f : 4.f); }

// idx -> (plane, y, x) of a planes x H x W tensor: two 32-bit divisions while the tensor has fewer than 2^32 elements (every launch
// of the training step), the 64-bit ones beyond
__device__ __forceinline__ size_t pyr_split(size_t idx, bool small, int H, int W, int& y, int& x) {
    if (small) {
        const unsigned row = (unsigned)idx / (unsigned)W, pl = row / (unsigned)H;
        x = (int)((unsigned)idx - row * (unsigned)W);
        y = (int)(row - pl * (unsigned)H);
        return pl;
    }
    x = (int)(idx % W);
    y = (int)((idx / W) % H);
    return idx / ((size_t)W * H);
}

// The four pyramid stencils below have two paths each.  Away from the border no tap reflects: the forward kernels index their taps
// directly, and the adjoints enumerate the few outputs that read an input -- by parity (1, 6, 1) or (4, 4) for the ::2 select, always
// (1, 4, 6, 4, 1) for the zero-insert upsample -- instead of testing every tap of a 7- or 9-wide candidate window.  Border rows and
// columns keep the reflect() / candidate-scan code.  Both paths add the same terms in the same ascending order with the same
// rowacc / acc grouping, so which path a pixel takes does not show in the bits.

// The 25-tap sum of gauss_down_fwd, v[5 i + j] = in[row i][col j] of the window: taps 0 .. 12 are fused multiply-adds onto the running
// sum, taps 13 .. 24 are rounded products added to it.  That split is what the compiler made of `acc += w * in[..]` in this kernel
// since it was written (it packs the later products in pairs) and so defines the operator's bits; written out, it no longer depends
// on how the taps are addressed.
__device__ __forceinline__ float gauss_down_sum(const float (&v)[25]) {
#pragma clang fp contract(off)
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < 25; ++t) {
        const float w = binom(t / 5) * binom(t % 5) * (1.f / 256.f);
        acc = t < 13 ? fmaf(w, v[t], acc) : acc + w * v[t];
    }
    return acc;
}

// out[y][x] = sum_{i,j} k[i]k[j]/256 * in[reflect(2y+i-2)][reflect(2x+j-2)]     (conv_gauss + ::2)
__global__ void gauss_down_fwd_kernel(const float* __restrict__ in, float* __restrict__ out, size_t planes, int H,
                                      int W, int Hd, int Wd) {
    const size_t n = planes * Hd * Wd;
    const bool small = n < (1ull << 32);
    LOOP(idx, n) {
        int x, y;
        const float* p = in + pyr_split(idx, small, Hd, Wd, y, x) * H * W;
        float v[25];
        if (y >= 1 && 2 * y + 2 < H && x >= 1 && 2 * x + 2 < W) {      // interior: rows 2y-2 .. 2y+2, cols 2x-2 .. 2x+2 as they are
            const float* q = p + (size_t)(2 * y - 2) * W + (2 * x - 2);
#pragma unroll
            for (int t = 0; t < 25; ++t) v[t] = q[(t / 5) * W + t % 5];
        } else {
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int r = reflect(2 * y + i - 2, H);
#pragma unroll
                for (int j = 0; j < 5; ++j) v[5 * i + j] = p[(size_t)r * W + reflect(2 * x + j - 2, W)];
            }
        }
        out[idx] = gauss_down_sum(v);
    }
}

__global__ void gauss_down_bwd_kernel(const float* __restrict__ gout, float* __restrict__ gin, size_t planes, int H,
                                      int W, int Hd, int Wd) {
    const size_t n = planes * H * W;
    const bool small = n < (1ull << 32);
    LOOP(idx, n) {
        int s, r;
        const float* g = gout + pyr_split(idx, small, H, W, r, s) * Hd * Wd;
        if (r >= 3 && r <= H - 4 && s >= 3 && s <= W - 4) {
            // interior: an even row is read by outputs r/2 - 1, r/2, r/2 + 1 through taps 4, 2, 0 (weights 1, 6, 1), an odd row by
            // r/2, r/2 + 1 through taps 3, 1 (4, 4); no reflected tap lands on rows 3 .. H - 4
            const int oddr = r & 1, odds = s & 1;
            const int y0 = r / 2 - 1 + oddr, x0 = s / 2 - 1 + odds;
            const float wy0 = oddr ? 4.f : 1.f, wy1 = oddr ? 4.f : 6.f, wx0 = odds ? 4.f : 1.f, wx1 = odds ? 4.f : 6.f;
            float acc = 0.f;
#pragma unroll
            for (int ty = 0; ty < 3; ++ty) {      // (every `+= w * g` of this kernel is one fused multiply-add)
                if (ty == 2 && oddr) continue;
                const float* q = g + (size_t)(y0 + ty) * Wd + x0;
                float rowacc = fmaf(wx0, q[0], 0.f);
                rowacc = fmaf(wx1, q[1], rowacc);
                if (!odds) rowacc = fmaf(1.f, q[2], rowacc);
                acc = fmaf(ty == 0 ? wy0 : (ty == 1 ? wy1 : 1.f), rowacc, acc);
            }
            gin[idx] = acc * (1.f / 256.f);
            continue;
        }
        float wy[7], wx[7];
        const int yb = r / 2 - 3, xb = s / 2 - 3;
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            const int y = yb + t, x = xb + t;
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                if (y >= 0 && y < Hd && reflect(2 * y + i - 2, H) == r) a += binom(i);
                if (x >= 0 && x < Wd && reflect(2 * x + i - 2, W) == s) b += binom(i);
            }
            wy[t] = a;
            wx[t] = b;
        }
        float acc = 0.f;
#pragma unroll
        for (int ty = 0; ty < 7; ++ty) {
            if (wy[ty] == 0.f) continue;
            float rowacc = 0.f;
#pragma unroll
            for (int tx = 0; tx < 7; ++tx)
                if (wx[tx] != 0.f) rowacc += wx[tx] * g[(size_t)(yb + ty) * Wd + xb + tx];
            acc += wy[ty] * rowacc;
        }
        gin[idx] = acc * (1.f / 256.f);
    }
}

// out = cur - conv_gauss(zero_insert(down), 4*kernel)                      (upsample + diff)
__global__ void lap_updiff_fwd_kernel(const float* __restrict__ cur, const float* __restrict__ down,
                                      float* __restrict__ out, size_t planes, int H, int W) {
    const int Hd = H / 2, Wd = W / 2;
    const size_t n = planes * H * W;
    const bool small = n < (1ull << 32);
    LOOP(idx, n) {
        int x, y;
        const float* d = down + pyr_split(idx, small, H, W, y, x) * Hd * Wd;
        float acc = 0.f;
        if (y >= 2 && y <= H - 3 && x >= 2 && x <= W - 3) {
            // interior: the even rows among y-2 .. y+2 are taps 0, 2, 4 (y even) or 1, 3 (y odd), the same along x
            const int i0 = y & 1, j0 = x & 1;
            const float* q = d + (size_t)((y + i0 - 2) >> 1) * Wd + ((x + j0 - 2) >> 1);
#pragma unroll
            for (int ii = 0; ii < 3; ++ii) {
                if (ii == 2 && i0) continue;
                const float bi = i0 ? 4.f : (ii == 1 ? 6.f : 1.f);
#pragma unroll
                for (int jj = 0; jj < 3; ++jj) {
                    if (jj == 2 && j0) continue;
                    const float bj = j0 ? 4.f : (jj == 1 ? 6.f : 1.f);
                    acc = fmaf(bi * bj * (4.f / 256.f), q[ii * Wd + jj], acc);      // (fused, as every tap of the border path is)
                }
            }
            out[idx] = cur[idx] - acc;
            continue;
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int r = reflect(y + i - 2, H);
            if (r & 1) continue;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int s = reflect(x + j - 2, W);
                if (s & 1) continue;
                acc += (binom(i) * binom(j) * (4.f / 256.f)) * d[(size_t)(r >> 1) * Wd + (s >> 1)];
            }
        }
        out[idx] = cur[idx] - acc;
    }
}

// gdown[a][b] = -sum_{y,x} gout[y][x] * 4 k[i]k[j]/256 over taps with reflect(y+i-2)=2a, reflect(x+j-2)=2b
__global__ void lap_updiff_bwd_kernel(const float* __restrict__ gout, float* __restrict__ gdown, size_t planes, int H,
                                      int W) {
    const int Hd = H / 2, Wd = W / 2;
    const size_t n = planes * Hd * Wd;
    const bool small = n < (1ull << 32);
    LOOP(idx, n) {
        int a, b;
        const float* g = gout + pyr_split(idx, small, Hd, Wd, a, b) * H * W;
        if (a >= 2 && a <= Hd - 2 && b >= 2 && b <= Wd - 2) {
            // interior: rows 2a-2 .. 2a+2 reach row 2a through taps 4 .. 0 (weights 1, 4, 6, 4, 1); no reflected tap lands on it
            const float* q = g + (size_t)(2 * a - 2) * W + (2 * b - 2);
            float acc = 0.f;
#pragma unroll
            for (int ty = 0; ty < 5; ++ty) {
                float rowacc = 0.f;      // (every `+= w * g` of this kernel is one fused multiply-add)
#pragma unroll
                for (int tx = 0; tx < 5; ++tx) rowacc = fmaf(binom(tx), q[ty * W + tx], rowacc);
                acc = fmaf(binom(ty), rowacc, acc);
            }
            gdown[idx] = -acc * (4.f / 256.f);
            continue;
        }
        float wy[9], wx[9];
        const int yb = 2 * a - 4, xb = 2 * b - 4;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int y = yb + t, x = xb + t;
            float u = 0.f, v = 0.f;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                if (y >= 0 && y < H && reflect(y + i - 2, H) == 2 * a) u += binom(i);
                if (x >= 0 && x < W && reflect(x + i - 2, W) == 2 * b) v += binom(i);
            }
            wy[t] = u;
            wx[t] = v;
        }
        float acc = 0.f;
#pragma unroll
        for (int ty = 0; ty < 9; ++ty) {
            if (wy[ty] == 0.f) continue;
            float rowacc = 0.f;
#pragma unroll
            for (int tx = 0; tx < 9; ++tx)
                if (wx[tx] != 0.f) rowacc += wx[tx] * g[(size_t)(yb + ty) * W + xb + tx];
            acc += wy[ty] * rowacc;
        }
        gdown[idx] = -acc * (4.f / 256.f);
    }
}

// conv_gauss / upsample of the pyramid helpers as stand-alone operators (utils/util.py:503-516)
// out[y][x] = gain/256 * sum k[i]k[j] Z[reflect(y+i-2)][reflect(x+j-2)];  up == 0: Z = in (H x W);
// up == 1: Z = zero-insert of in (H/2 x W/2) at the even positions of an H x W grid
__global__ void gauss_full_fwd_kernel(const float* __restrict__ in, float* __restrict__ out, size_t planes, int H, int W,
                                      int up, float gain) {
    const int Hs = up ? H / 2 : H, Ws = up ? W / 2 : W;
    const size_t n = planes * H * W;
    LOOP(idx, n) {
        const int x = (int)(idx % W);
        const int y = (int)((idx / W) % H);
        const float* p = in + (idx / ((size_t)W * H)) * Hs * Ws;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int r = reflect(y + i - 2, H);
            if (up && (r & 1)) continue;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int s = reflect(x + j - 2, W);
                if (up && (s & 1)) continue;
                acc += (binom(i) * binom(j)) * p[(size_t)(up ? r >> 1 : r) * Ws + (up ? s >> 1 : s)];
            }
        }
        out[idx] = acc * (gain * (1.f / 256.f));
    }
}
// adjoint: gin[a][b] = gain/256 * sum over outputs (y, x) in a 5x5 neighbourhood of the taps that land on Z[r][s],
// (r, s) = (a, b) (up == 0) or (2a, 2b) (up == 1).  Reflection keeps |y - r| <= 2.
__global__ void gauss_full_bwd_kernel(const float* __restrict__ gout, float* __restrict__ gin, size_t planes, int H, int W,
                                      int up, float gain) {
    const int Hs = up ? H / 2 : H, Ws = up ? W / 2 : W;
    const size_t n = planes * Hs * Ws;
    LOOP(idx, n) {
        const int b = (int)(idx % Ws);
        const int a = (int)((idx / Ws) % Hs);
        const float* g = gout + (idx / ((size_t)Ws * Hs)) * H * W;
        const int r = up ? 2 * a : a, s = up ? 2 * b : b;
        float wy[5], wx[5];
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int y = r - 2 + t, x = s - 2 + t;
            float u = 0.f, v = 0.f;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                if (y >= 0 && y < H && reflect(y + i - 2, H) == r) u += binom(i);
                if (x >= 0 && x < W && reflect(x + i - 2, W) == s) v += binom(i);
            }
            wy[t] = u;
            wx[t] = v;
        }
        float acc = 0.f;
#pragma unroll
        for (int ty = 0; ty < 5; ++ty) {
            if (wy[ty] == 0.f) continue;
            float rowacc = 0.f;
#pragma unroll
            for (int tx = 0; tx < 5; ++tx)
                if (wx[tx] != 0.f) rowacc += wx[tx] * g[(size_t)(r - 2 + ty) * W + s - 2 + tx];
            acc += wy[ty] * rowacc;
        }
        gin[idx] = acc * (gain * (1.f / 256.f));
    }
}

// ---------------------------------------------------------------- host side
thread_local char rvsr_g_err[256] = "";
extern "C" const char* rvsr_last_error() { return rvsr_g_err; }

extern "C" int rvsr_upsample_bilinear_forward(const float* in, float* out, size_t planes, int H, int W, int factor,
                                              float scale, void* stream) {
    if (!in || !out || (factor != 2 && factor != 4)) FAIL(RVSR_ERR_BAD_ARG, "upsample: bad argument (factor %d)", factor);
    const size_t n = planes * H * factor * W * factor;
    if (factor == 2 && n < (1ull << 32) && (((uintptr_t)out) & 7) == 0) {
        hipLaunchKernelGGL(upsample2_fwd_kernel, GRID_FOR(n / 4), dim3(256), 0, (hipStream_t)stream, in, out, (unsigned)planes, H, W, scale);
        RETURN_LAUNCH("upsample2_fwd");
    }
    hipLaunchKernelGGL(upsample_fwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, in, out, planes, H, W, factor, scale);
    RETURN_LAUNCH("upsample_fwd");
}
extern "C" int rvsr_upsample_bilinear_backward(const float* gout, float* gin, size_t planes, int H, int W, int factor,
                                               float scale, void* stream) {
    if (!gout || !gin || (factor != 2 && factor != 4)) FAIL(RVSR_ERR_BAD_ARG, "upsample backward: bad argument");
    const size_t n = planes * H * W;
    if (factor == 2 && n * 4 < (1ull << 32) && W % 4 == 0 && ((((uintptr_t)gout) | ((uintptr_t)gin)) & 15) == 0) {
        hipLaunchKernelGGL(upsample2_bwd_v4_kernel, GRID_FOR(n / 4), dim3(256), 0, (hipStream_t)stream, gout, gin, (unsigned)planes, H, W, scale);
        RETURN_LAUNCH("upsample2_bwd_v4");
    }
    if (factor == 2 && n * 4 < (1ull << 32) && (((uintptr_t)gout) & 7) == 0) {
        hipLaunchKernelGGL(upsample2_bwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, gout, gin, (unsigned)planes, H, W, scale);
        RETURN_LAUNCH("upsample2_bwd");
    }
    hipLaunchKernelGGL(upsample_bwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, gout, gin, planes, H, W, factor, scale);
    RETURN_LAUNCH("upsample_bwd");
}
extern "C" int rvsr_maxavgpool_forward(const float* in, float* out, unsigned char* argmax, int B, int C, int H, int W,
                                       void* stream) {
    if (!in || !out || !argmax) FAIL(RVSR_ERR_BAD_ARG, "pool: null argument");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const size_t n = (size_t)B * C * Ho * Wo;
    if (W % 8 == 0 && (size_t)B * C * H * W < (1ull << 31) && ((((uintptr_t)in) | ((uintptr_t)out) | ((uintptr_t)argmax)) & 15) == 0) {
        hipLaunchKernelGGL(pool_fwd_v4_kernel, GRID_FOR(n / 4), dim3(256), 0, (hipStream_t)stream, in, out, argmax, B, C, H, W, Ho, Wo);
        RETURN_LAUNCH("pool_fwd_v4");
    }
    hipLaunchKernelGGL(pool_fwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, in, out, argmax, B, C, H, W, Ho, Wo);
    RETURN_LAUNCH("pool_fwd");
}
extern "C" int rvsr_maxavgpool_backward(const float* gout, const unsigned char* argmax, float* gin, int B, int C, int H,
                                        int W, void* stream) {
    if (!gout || !gin || !argmax) FAIL(RVSR_ERR_BAD_ARG, "pool backward: null argument");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const size_t n = (size_t)B * C * H * W;
    if (W % 4 == 0 && n < (1ull << 31) && ((((uintptr_t)gout) | ((uintptr_t)gin) | ((uintptr_t)argmax)) & 15) == 0) {
        hipLaunchKernelGGL(pool_bwd_v4_kernel, GRID_FOR(n / 4), dim3(256), 0, (hipStream_t)stream, gout, argmax, gin, B, C, H, W, Ho, Wo);
        RETURN_LAUNCH("pool_bwd_v4");
    }
    hipLaunchKernelGGL(pool_bwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, gout, argmax, gin, B, C, H, W, Ho, Wo);
    RETURN_LAUNCH("pool_bwd");
}
extern "C" int rvsr_tsa_temporal_forward(const float* emb, const float* emb_ref, const float* aligned, float* mod,
                                         float* prob, int B, int N, int C, int H, int W, int frame_major, void* stream) {
    if (!emb || !emb_ref || !aligned || !mod || !prob) FAIL(RVSR_ERR_BAD_ARG, "tsa_temporal: null argument");
    const size_t n = (size_t)B * N * H * W;
    hipLaunchKernelGGL(tsa_corr_fwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, emb, emb_ref, aligned, mod, prob, B, N,
                       C, (size_t)H * W, frame_major);
    RETURN_LAUNCH("tsa_corr_fwd");
}
extern "C" int rvsr_tsa_temporal_backward(const float* gmod, const float* emb, const float* emb_ref, const float* aligned,
                                          const float* prob, float* galigned, float* gemb, float* gemb_ref, int B, int N,
                                          int C, int H, int W, int frame_major, void* stream) {
    if (!gmod || !emb || !emb_ref || !aligned || !prob || !galigned || !gemb || !gemb_ref)
        FAIL(RVSR_ERR_BAD_ARG, "tsa_temporal backward: null argument");
    if (N > TSA_MAXN) FAIL(RVSR_ERR_UNSUPPORTED, "tsa_temporal backward: nframes %d > %d", N, TSA_MAXN);
    const size_t n = (size_t)B * H * W;
    hipLaunchKernelGGL(tsa_corr_bwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, gmod, emb, emb_ref, aligned, prob,
                       galigned, gemb, gemb_ref, B, N, C, (size_t)H * W, frame_major);
    RETURN_LAUNCH("tsa_corr_bwd");
}
extern "C" int rvsr_tsa_output_forward(const float* fea, const float* att, const float* att_add, float* out, size_t n,
                                       void* stream) {
    if (!fea || !att || !att_add || !out) FAIL(RVSR_ERR_BAD_ARG, "tsa_output: null argument");
    hipLaunchKernelGGL(tsa_final_fwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, fea, att, att_add, out, n);
    RETURN_LAUNCH("tsa_final_fwd");
}
extern "C" int rvsr_tsa_output_backward(const float* g, const float* fea, const float* att, float* gfea, float* gatt,
                                        size_t n, void* stream) {
    if (!g || !fea || !att || !gfea || !gatt) FAIL(RVSR_ERR_BAD_ARG, "tsa_output backward: null argument");
    hipLaunchKernelGGL(tsa_final_bwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, g, fea, att, gfea, gatt, n);
    RETURN_LAUNCH("tsa_final_bwd");
}
extern "C" int rvsr_pyr_down_forward(const float* in, float* out, size_t planes, int H, int W, void* stream) {
    if (!in || !out || H < 3 || W < 3) FAIL(RVSR_ERR_BAD_ARG, "pyr_down: bad argument (reflect pad 2 needs H,W >= 3)");
    const int Hd = (H + 1) / 2, Wd = (W + 1) / 2;
    const size_t n = planes * Hd * Wd;
    hipLaunchKernelGGL(gauss_down_fwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, in, out, planes, H, W, Hd, Wd);
    RETURN_LAUNCH("gauss_down_fwd");
}
extern "C" int rvsr_pyr_down_backward(const float* gout, float* gin, size_t planes, int H, int W, void* stream) {
    if (!gout || !gin || H < 3 || W < 3) FAIL(RVSR_ERR_BAD_ARG, "pyr_down backward: bad argument");
    const int Hd = (H + 1) / 2, Wd = (W + 1) / 2;
    const size_t n = planes * H * W;
    hipLaunchKernelGGL(gauss_down_bwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, gout, gin, planes, H, W, Hd, Wd);
    RETURN_LAUNCH("gauss_down_bwd");
}
extern "C" int rvsr_pyr_updiff_forward(const float* cur, const float* down, float* out, size_t planes, int H, int W,
                                       void* stream) {
    if (!cur || !down || !out || (H & 1) || (W & 1) || H < 4 || W < 4)
        FAIL(RVSR_ERR_BAD_ARG, "pyr_updiff: H, W must be even and >= 4 (got %dx%d)", H, W);
    const size_t n = planes * H * W;
    hipLaunchKernelGGL(lap_updiff_fwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, cur, down, out, planes, H, W);
    RETURN_LAUNCH("lap_updiff_fwd");
}
extern "C" int rvsr_pyr_updiff_backward(const float* gout, float* gdown, size_t planes, int H, int W, void* stream) {
    if (!gout || !gdown || (H & 1) || (W & 1) || H < 4 || W < 4) FAIL(RVSR_ERR_BAD_ARG, "pyr_updiff backward: bad argument");
    const size_t n = planes * (H / 2) * (W / 2);
    hipLaunchKernelGGL(lap_updiff_bwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, gout, gdown, planes, H, W);
    RETURN_LAUNCH("lap_updiff_bwd");
}
extern "C" int rvsr_conv_gauss_forward(const float* in, float* out, size_t planes, int H, int W, float gain, void* stream) {
    if (!in || !out || H < 3 || W < 3) FAIL(RVSR_ERR_BAD_ARG, "conv_gauss: bad argument (reflect padding 2 needs H, W >= 3)");
    const size_t n = planes * (size_t)H * W;
    hipLaunchKernelGGL(gauss_full_fwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, in, out, planes, H, W, 0, gain);
    RETURN_LAUNCH("conv_gauss_fwd");
}
extern "C" int rvsr_conv_gauss_backward(const float* gout, float* gin, size_t planes, int H, int W, float gain, void* stream) {
    if (!gout || !gin || H < 3 || W < 3) FAIL(RVSR_ERR_BAD_ARG, "conv_gauss backward: bad argument");
    const size_t n = planes * (size_t)H * W;
    hipLaunchKernelGGL(gauss_full_bwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, gout, gin, planes, H, W, 0, gain);
    RETURN_LAUNCH("conv_gauss_bwd");
}
// in: planes x H x W  ->  out: planes x 2H x 2W
extern "C" int rvsr_pyr_upsample_forward(const float* in, float* out, size_t planes, int H, int W, void* stream) {
    if (!in || !out || H < 2 || W < 2) FAIL(RVSR_ERR_BAD_ARG, "pyr_upsample: bad argument");
    const size_t n = planes * (size_t)H * W * 4;
    hipLaunchKernelGGL(gauss_full_fwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, in, out, planes, 2 * H, 2 * W, 1, 4.f);
    RETURN_LAUNCH("pyr_upsample_fwd");
}
extern "C" int rvsr_pyr_upsample_backward(const float* gout, float* gin, size_t planes, int H, int W, void* stream) {
    if (!gout || !gin || H < 2 || W < 2) FAIL(RVSR_ERR_BAD_ARG, "pyr_upsample backward: bad argument");
    const size_t n = planes * (size_t)H * W;
    hipLaunchKernelGGL(gauss_full_bwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, gout, gin, planes, 2 * H, 2 * W, 1, 4.f);
    RETURN_LAUNCH("pyr_upsample_bwd");
}

// ---------------------------------------------------------------- YCbCr (planar f32) -> BGR uint8 (HWC)
// Restates, operation for operation, what the reference's test script does on the host with numpy
// (test_RealVSR_wi_GT.py:122-123): tensor2img(out_type=float32, reverse_channel=False) = clamp to [0, 1];
// data/util.py:397-416 ycbcr2bgr on a float32 image: `img *= 255` in f32, matmul with the f64 matrix (f64
// accumulation), `* 255.0 + offset`, `/ 255.` in f64, cast to f32; then clip, `* 255.` in f32, round half to even,
// uint8.  Done on the GPU so a frame leaves as 3 bytes per pixel instead of 12.
__global__ void ycbcr2bgr_u8_kernel(const float* __restrict__ ycc, unsigned char* __restrict__ bgr, size_t hw) {
    const double M[3][3] = {{0.00456621, 0.00456621, 0.00456621}, {0.00791071, -0.00153632, 0.0}, {0.0, -0.00318811, 0.00625893}};
    const double off[3] = {-276.836, 135.576, -222.921};
    LOOP(i, hw) {
        float s[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = ycc[(size_t)c * hw + i];
            v = fminf(fmaxf(v, 0.f), 1.f);
            s[c] = __fmul_rn(v, 255.f);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double d = __dmul_rn((double)s[0], M[0][j]);
            d = __dadd_rn(d, __dmul_rn((double)s[1], M[1][j]));
            d = __dadd_rn(d, __dmul_rn((double)s[2], M[2][j]));
            d = __dadd_rn(__dmul_rn(d, 255.0), off[j]);
            float r = (float)(d / 255.0);
            r = fminf(fmaxf(r, 0.f), 1.f);
            bgr[i * 3 + j] = (unsigned char)rintf(__fmul_rn(r, 255.f));
        }
    }
}
extern "C" int rvsr_ycbcr_to_bgr_u8(const float* ycc, unsigned char* bgr, int H, int W, void* stream) {
    if (!ycc || !bgr || H <= 0 || W <= 0) FAIL(RVSR_ERR_BAD_ARG, "ycbcr_to_bgr_u8: null/empty argument");
    const size_t hw = (size_t)H * W;
    hipLaunchKernelGGL(ycbcr2bgr_u8_kernel, GRID_FOR(hw), dim3(256), 0, (hipStream_t)stream, ycc, bgr, hw);
    RETURN_LAUNCH("ycbcr_to_bgr_u8");
}

// ------------------------------------------------------------------------------------------
// Measurement aid (bench.py: roofline_conv.sustained_peak): the rate this device SUSTAINS on v_mfma_f32_32x32x16_bf16 with operands
// that carry data.  One 8-wave workgroup per CU, every wave loops over 8 MFMAs on 8 accumulator sets with 4 + 4 operand registers taken
// from `ops` (8 x 512 x 16 B): nothing but the matrix pipe runs.  Constant operands reach the nominal 2.5 PFLOP/s; N(0,1)-like values or
// the three-term hi / lo pattern run into the package power limit at ~0.67 of it (profiles/r05_mfma_power_micro.txt).
typedef __bf16 dbg_bf16x8 __attribute__((ext_vector_type(8)));
__global__ __launch_bounds__(512) void mfma_rate_kernel(const dbg_bf16x8* __restrict__ ops, float* out, int iters) {
    f32x16 a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = zero16();
    dbg_bf16x8 x[4], y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { x[i] = ops[(i * 2) * 512 + threadIdx.x]; y[i] = ops[(i * 2 + 1) * 512 + threadIdx.x]; }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[i & 3], y[(i + (i >> 2)) & 3], a[i], 0, 0, 0);
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) s += a[i][j];
    out[(size_t)blockIdx.x * 512 + threadIdx.x] = s;
}
extern "C" int rvsr_debug_mfma_rate(const void* ops, float* out, int workgroups, int iters, void* stream) {
    if (!ops || !out || workgroups <= 0 || iters <= 0) FAIL(RVSR_ERR_BAD_ARG, "debug_mfma_rate: null/empty argument");
    hipLaunchKernelGGL(mfma_rate_kernel, dim3((unsigned)workgroups), dim3(512), 0, (hipStream_t)stream, (const dbg_bf16x8*)ops, out, iters);
    RETURN_LAUNCH("debug_mfma_rate");
}
