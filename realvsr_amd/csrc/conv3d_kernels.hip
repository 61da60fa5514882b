// conv3d_kernels.hip -- the kernels FSTRN needs beyond the 2-D convolutions (codes/models/archs/FSTRN_arch.py), on frame-major f32
// activations [T, B, C, H, W]:
//
//   tconv3   the (3,1,1) temporal convolution of an FRB (:17, :21-22) with bias, the block's residual add and the next block's PReLU:
//              out[t,b,co,p]  = bias[co] + sum_{dt < 3, 0 <= t+dt-1 < T} sum_ci w[co,ci,dt] * s[t+dt-1,b,ci,p]  [+ residual[t,b,co,p]]
//              pout[t,b,co,p] = out > 0 ? out : slope * out                                                      (optional)
//            transposed: w is read as [ci, co, 2 - dt], which makes the same kernel the data gradient.
//   prelu    y = prelu(a [+ b]) [* keep * scale] (:15, :42-43, :60-62), its backward, and the slope gradient as a two-stage sum.
//
// tconv3 is a GEMM with M = Co <= 64, K = 3 * Ci <= 192 and N = pixels, memory-bound by a wide margin (72 matrix instructions per 32
// pixels and frame against 24 KB moved).  A wave owns 32 consecutive pixels of one batch element and walks t = 0 .. T-1 holding the
// operand fragments of frames t-1, t, t+1 in REGISTERS (a pixel's three taps are the same pixel one frame apart, so nothing is shared
// between lanes and the rotation needs no LDS): every element of s is loaded from memory once.  The weight image of all three taps stays
// in LDS, built by the workgroup itself from the f32 weights (no separate pack launch) and reused for every work item the workgroup walks.
// Products: three-term bf16 split (bf16x3.h) or, in GEMM mode f32, the exact-f32 MFMA; the reduced-term speed modes keep three terms.
// The accumulators start from the bias, so no MFMA has a constant-zero SrcC (see mfma_bf16_first in bf16x3.h).
// On the vector path (conv3d_plan.h) loads and stores are 16 bytes per lane: a lane loads 4 pixels of one channel and a 4 x 4 transpose
// inside the lane quad turns that into the MFMA's "one pixel, consecutive channels"; the epilogue does the reverse.
#include "conv3d_plan.h"

#include "bf16x3.h"
#include "glue_common.h"

struct TcParams {
    const float* s;
    const float* w;
    const float* bias;    // NULL: none
    const float* res;     // NULL: none; may be `out` itself (every element is read and written by the same lane)
    const float* slope;   // device scalar, read when pout != NULL
    float* out;
    float* pout;          // NULL: none
    int T, B, Ci, Co, HW, tiles, vec, transposed;
    long items;
};

// Operand fragments of one frame for one wave: lane (lo = lane & 31, hi = lane >> 5) holds channels 16 ks + 8 hi + 0..7 of pixel lo.
template <int KS, bool F32>
struct TcFrame;
template <int KS>
struct TcFrame<KS, true> {
    float v[KS][8];
};
template <int KS>
struct TcFrame<KS, false> {
    bf16x8 hi[KS], lo[KS];
};

template <int KS>
__device__ __forceinline__ void tc_convert(const float (&raw)[KS][8], TcFrame<KS, true>& f) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) f.v[ks][e] = raw[ks][e];
}
template <int KS>
__device__ __forceinline__ void tc_convert(const float (&raw)[KS][8], TcFrame<KS, false>& f) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) split8(raw[ks], f.hi[ks], f.lo[ks]);
}

// Byte offsets of a lane's loads inside one frame of one batch element ([Ci][HW] floats, addressed through a 2 GB buffer view): the same
// for every frame of the walk.  A channel >= Ci or a pixel >= HW gets an offset beyond the view: its load returns 0 and needs no branch.
// VEC: one offset per 16-byte load, [ks][g] -- lane j of a quad loads channel 16 ks + 8 hi + 4 g + j at the quad's 4 pixels.  Scalar: the
// offset of channel 8 hi at the lane's own pixel; the 8 KS channel offsets are added per load (kept out of registers: they spilled).
#define TC_OOB 0x80000000u
template <int KS, bool VEC>
__device__ __forceinline__ void tc_offsets(const TcParams& p, int pix0, int lo, int hi, unsigned (&off)[VEC ? 2 * KS : 1]) {
    const unsigned HW = (unsigned)p.HW;
    if (VEC) {
        const int px = pix0 + (lo & ~3);
#pragma unroll
        for (int i = 0; i < 2 * KS; ++i) {
            const int c = (i >> 1) * 16 + 8 * hi + 4 * (i & 1) + (lo & 3);
            off[VEC ? i : 0] = (px < p.HW && c < p.Ci) ? 4u * ((unsigned)c * HW + (unsigned)px) : TC_OOB;
        }
    } else {
        const int px = pix0 + lo;
        off[0] = px < p.HW ? 4u * ((unsigned)(8 * hi) * HW + (unsigned)px) : TC_OOB;
    }
}

// The wave's 32 pixels of one frame: all loads are issued before any value is used.
template <int KS, bool VEC>
__device__ __forceinline__ void tc_load(const TcParams& p, __amdgpu_buffer_rsrc_t rs, const unsigned (&off)[VEC ? 2 * KS : 1], int lo, int hi,
                                        float (&v)[KS][8]) {
    if (VEC) {
        typedef float f32x4v __attribute__((ext_vector_type(4)));
        f32x4v q[2 * KS];
#pragma unroll
        for (int i = 0; i < 2 * KS; ++i) q[i] = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off[VEC ? i : 0], 0, 0));
#pragma unroll
        for (int i = 0; i < 2 * KS; ++i) {
            float r0 = q[i].x, r1 = q[i].y, r2 = q[i].z, r3 = q[i].w;
            quad_transpose4(r0, r1, r2, r3, lo);   // lane j: channel j of the group at 4 pixels -> pixel j at the group's 4 channels
            v[i >> 1][4 * (i & 1) + 0] = r0; v[i >> 1][4 * (i & 1) + 1] = r1; v[i >> 1][4 * (i & 1) + 2] = r2; v[i >> 1][4 * (i & 1) + 3] = r3;
        }
    } else {
        const unsigned HW4 = 4u * (unsigned)p.HW;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = ks * 16 + 8 * hi + e;
                v[ks][e] = buf_load(rs, (off[0] != TC_OOB && c < p.Ci) ? off[0] + (unsigned)(ks * 16 + e) * HW4 : TC_OOB, 0u);
            }
    }
}

// acc[m] += W_dt[32 m .. 32 m + 31][:] * frame.  img: the LDS weight image, [dt][ks][m][part][lane] x 16 bytes.
template <int KS, int MT>
__device__ __forceinline__ void tc_gemm(f32x16 (&acc)[MT], const TcFrame<KS, false>& f, const uint4* img, int dt, int lane) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const uint4* a = img + (size_t)(((dt * KS + ks) * MT + m) * 2) * 64 + lane;
            const bf16x8 ahi = __builtin_bit_cast(bf16x8, a[0]), alo = __builtin_bit_cast(bf16x8, a[64]);
            acc[m] = mfma_bf16(ahi, f.hi[ks], acc[m]);
            acc[m] = mfma_bf16(ahi, f.lo[ks], acc[m]);
            acc[m] = mfma_bf16(alo, f.hi[ks], acc[m]);
        }
}
template <int KS, int MT>
__device__ __forceinline__ void tc_gemm(f32x16 (&acc)[MT], const TcFrame<KS, true>& f, const uint4* img, int dt, int lane) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const uint4* a = img + (size_t)(((dt * KS + ks) * MT + m) * 2) * 64 + lane;
            const uint4 a0 = a[0], a1 = a[64];
            const unsigned u[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            // k-step e of the exact-f32 MFMA (32x32x2): lane half hi supplies channel 16 ks + 8 hi + e on both sides
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[m] = mfma32(__builtin_bit_cast(float, u[e]), f.v[ks][e], acc[m]);
            __builtin_amdgcn_sched_barrier(0);   // (keeps the LDS reads of later fragments from being hoisted above this chain: they spilled)
        }
}

// One output frame of one batch element ([Co][HW] floats behind 2 GB buffer views; res / pout views are only used where the call has them).
// Stores beyond the view (channel >= Co, pixel >= HW) are dropped by the hardware: no divergent branch.
template <int MT, bool VEC>
__device__ __forceinline__ void tc_epilogue(f32x16 (&acc)[MT], const TcParams& p, __amdgpu_buffer_rsrc_t out_rs, __amdgpu_buffer_rsrc_t res_rs,
                                            __amdgpu_buffer_rsrc_t pout_rs, int pix0, int lo, int hi, float sl) {
    const unsigned HW = (unsigned)p.HW;
    const bool has_res = p.res != nullptr, has_pout = p.pout != nullptr;   // (uniform)
    if (VEC) {
        typedef float f32x4v __attribute__((ext_vector_type(4)));
        const int j = lo & 3, px4 = pix0 + (lo & ~3);
        const bool pok = px4 < p.HW;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            f32x4v rv[4];
            unsigned off[4];
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int co = m * 32 + 8 * rg + 4 * hi + j;
                off[rg] = (pok && co < p.Co) ? 4u * ((unsigned)co * HW + (unsigned)px4) : TC_OOB;
                if (has_res) rv[rg] = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(res_rs, (int)off[rg], 0, 0));
            }
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                float r0 = acc[m][4 * rg + 0], r1 = acc[m][4 * rg + 1], r2 = acc[m][4 * rg + 2], r3 = acc[m][4 * rg + 3];
                quad_transpose4(r0, r1, r2, r3, lo);   // lane j: pixel j at 4 channels -> channel j of the group at 4 pixels
                float4 v = make_float4(r0, r1, r2, r3);
                if (has_res) { v.x += rv[rg].x; v.y += rv[rg].y; v.z += rv[rg].z; v.w += rv[rg].w; }
                buf_store4(out_rs, off[rg], 0u, v);
                if (has_pout)
                    buf_store4(pout_rs, off[rg], 0u, make_float4(v.x > 0.f ? v.x : sl * v.x, v.y > 0.f ? v.y : sl * v.y, v.z > 0.f ? v.z : sl * v.z,
                                                                 v.w > 0.f ? v.w : sl * v.w));
            }
        }
    } else {
        const int px = pix0 + lo;
        const bool pok = px < p.HW;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                float rv[4];
                unsigned off[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int co = m * 32 + 8 * rg + 4 * hi + i;   // (= 32 m + drow(4 rg + i, hi))
                    off[i] = (pok && co < p.Co) ? 4u * ((unsigned)co * HW + (unsigned)px) : TC_OOB;
                    if (has_res) rv[i] = buf_load(res_rs, off[i], 0u);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float v = acc[m][4 * rg + i];
                    if (has_res) v += rv[i];
                    buf_store(out_rs, off[i], 0u, v);
                    if (has_pout) buf_store(pout_rs, off[i], 0u, v > 0.f ? v : sl * v);
                }
            }
        }
    }
}

template <int KS, int MT, bool F32, bool VEC>
__global__ __launch_bounds__(TC_WG, 2) void tconv3_kernel(const TcParams p) {
    __shared__ uint4 img[3 * KS * MT * 2 * 64];
    __shared__ float bias_s[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 31, hi = lane >> 5;
    // the weight image: fragment (dt, ks, m), lane l holds row co = 32 m + (l & 31), channels 16 ks + 8 (l >> 5) + 0..7
    for (int idx = tid; idx < 3 * KS * MT * 64; idx += TC_WG) {
        const int l = idx & 63, frag = idx >> 6, m = frag % MT, ks = (frag / MT) % KS, dt = frag / (MT * KS);
        const int co = m * 32 + (l & 31);
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ci = ks * 16 + 8 * (l >> 5) + e;
            const bool ok = co < p.Co && ci < p.Ci;
            const size_t wi = p.transposed ? ((size_t)ci * p.Co + co) * 3 + (2 - dt) : ((size_t)co * p.Ci + ci) * 3 + dt;
            const float x = p.w[ok ? wi : 0];
            v[e] = ok ? x : 0.f;
        }
        uint4 a0, a1;
        if (F32) {
            a0 = make_uint4(__builtin_bit_cast(unsigned, v[0]), __builtin_bit_cast(unsigned, v[1]), __builtin_bit_cast(unsigned, v[2]),
                            __builtin_bit_cast(unsigned, v[3]));
            a1 = make_uint4(__builtin_bit_cast(unsigned, v[4]), __builtin_bit_cast(unsigned, v[5]), __builtin_bit_cast(unsigned, v[6]),
                            __builtin_bit_cast(unsigned, v[7]));
        } else {
            bf16x8 h, l8;
            split8(v, h, l8);
            a0 = __builtin_bit_cast(uint4, h);
            a1 = __builtin_bit_cast(uint4, l8);
        }
        img[(size_t)frag * 128 + l] = a0;
        img[(size_t)frag * 128 + 64 + l] = a1;
    }
    if (tid < 64) bias_s[tid] = (p.bias && tid < p.Co) ? p.bias[tid] : 0.f;
    __syncthreads();
    const float sl = p.pout ? p.slope[0] : 0.f;
    const size_t HW = (size_t)p.HW, in_frame = (size_t)p.B * p.Ci * HW;

    for (long item = blockIdx.x; item < p.items; item += gridDim.x) {
        const int b = (int)(item / p.tiles), tile = (int)(item - (long)b * p.tiles);
        const int pix0 = tile * TC_TILE + wave * TC_WAVE_PIX;
        if (pix0 >= p.HW) continue;   // (wave-uniform; no barrier inside the walk)
        const float* sb = p.s + (size_t)b * p.Ci * HW;
        unsigned off[VEC ? 2 * KS : 1];
        tc_offsets<KS, VEC>(p, pix0, lo, hi, off);
        TcFrame<KS, F32> prev, cur, next;
        float raw[KS][8];
        tc_load<KS, VEC>(p, buf_view_2g(sb), off, lo, hi, raw);
        tc_convert<KS>(raw, cur);
        prev = cur;   // (never read at t = 0; keeps the registers defined)
        next = cur;
        if (p.T > 1) {
            tc_load<KS, VEC>(p, buf_view_2g(sb + in_frame), off, lo, hi, raw);
            tc_convert<KS>(raw, next);
        }
        for (int t = 0; t < p.T; ++t) {
            const bool more = t + 2 < p.T;   // (uniform) frame t + 2 travels while frame t is computed
            if (more) tc_load<KS, VEC>(p, buf_view_2g(sb + (size_t)(t + 2) * in_frame), off, lo, hi, raw);
            f32x16 acc[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][r] = bias_s[m * 32 + drow(r, hi)];
            if (t > 0) tc_gemm<KS, MT>(acc, prev, img, 0, lane);
            tc_gemm<KS, MT>(acc, cur, img, 1, lane);
            if (t + 1 < p.T) tc_gemm<KS, MT>(acc, next, img, 2, lane);
            const size_t o = ((size_t)t * p.B + b) * p.Co * HW;
            tc_epilogue<MT, VEC>(acc, p, buf_view_2g(p.out + o), buf_view_2g(p.res ? p.res + o : p.out + o),
                                 buf_view_2g(p.pout ? p.pout + o : p.out + o), pix0, lo, hi, sl);
            prev = cur;
            cur = next;
            if (more) tc_convert<KS>(raw, next);
        }
    }
}

template <int KS, int MT>
static int tc_launch(const TcParams& p, int grid, int f32, hipStream_t st) {
    auto k = f32 ? (p.vec ? tconv3_kernel<KS, MT, true, true> : tconv3_kernel<KS, MT, true, false>)
                 : (p.vec ? tconv3_kernel<KS, MT, false, true> : tconv3_kernel<KS, MT, false, false>);
    hipLaunchKernelGGL(k, dim3(grid), dim3(TC_WG), 0, st, p);
    RETURN_LAUNCH("tconv3");
}

extern "C" int rvsr_tconv3_plan(int T, int B, int Ci, int Co, int H, int W, const void* s, const void* residual, const void* out,
                                const void* pout, int* vec, int* grid) {
    const TcPlan q = tc_plan(T, B, Ci, Co, H, W, s, residual, out, pout);
    if (q.rc != RVSR_OK) FAIL(q.rc, "%s", q.msg);
    if (vec) *vec = q.vec;
    if (grid) *grid = q.grid;
    return RVSR_OK;
}

extern "C" int rvsr_tconv3_forward(const float* s, const float* w, const float* bias, const float* residual, const float* slope, float* out,
                                   float* pout, int T, int B, int Ci, int Co, int H, int W, int transposed, void* stream) {
    const TcPlan q = tc_plan(T, B, Ci, Co, H, W, s, residual, out, pout);
    if (q.rc != RVSR_OK) FAIL(q.rc, "%s", q.msg);
    if (!s || !w || !out) FAIL(RVSR_ERR_BAD_ARG, "tconv3: null argument (only bias, residual, slope and pout may be NULL)");
    if (pout && !slope) FAIL(RVSR_ERR_BAD_ARG, "tconv3: pout needs the slope");
    if (s == out || s == pout) FAIL(RVSR_ERR_BAD_ARG, "tconv3: the input cannot be an output (frames t - 1 and t + 1 are read after frame t is written)");
    TcParams p;
    p.s = s; p.w = w; p.bias = bias; p.res = residual; p.slope = slope; p.out = out; p.pout = pout;
    p.T = T; p.B = B; p.Ci = Ci; p.Co = Co; p.HW = H * W; p.tiles = q.tiles; p.vec = q.vec; p.transposed = transposed ? 1 : 0;
    p.items = q.items;
    hipStream_t st = (hipStream_t)stream;
    const int f32 = rvsr_gemm_mode_now() == 1;
    switch (q.ks * 2 + q.mt - 1) {
        case 2: return tc_launch<1, 1>(p, q.grid, f32, st);
        case 3: return tc_launch<1, 2>(p, q.grid, f32, st);
        case 4: return tc_launch<2, 1>(p, q.grid, f32, st);
        case 5: return tc_launch<2, 2>(p, q.grid, f32, st);
        case 6: return tc_launch<3, 1>(p, q.grid, f32, st);
        case 7: return tc_launch<3, 2>(p, q.grid, f32, st);
        case 8: return tc_launch<4, 1>(p, q.grid, f32, st);
        default: return tc_launch<4, 2>(p, q.grid, f32, st);
    }
}

// ---------------------------------------------------------------------------------------------
// PReLU.  One slope for the whole tensor (nn.PReLU()), always read from device memory.
// y = prelu(a [+ b]) [* keep * scale]
template <int VEC>
__global__ __launch_bounds__(PR_WG) void prelu_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ slope,
                                                          const unsigned char* __restrict__ keep, float scale, float* __restrict__ y, size_t n) {
    const float sl = slope[0];
    const size_t first = (size_t)blockIdx.x * PR_WG + threadIdx.x, step = (size_t)gridDim.x * PR_WG;
    if (VEC) {
        const float4* a4 = reinterpret_cast<const float4*>(a);
        const float4* b4 = reinterpret_cast<const float4*>(b);
        const uchar4* k4 = reinterpret_cast<const uchar4*>(keep);
        float4* y4 = reinterpret_cast<float4*>(y);
        const size_t n4 = n >> 2;
#pragma unroll 4
        for (size_t i = first; i < n4; i += step) {
            float4 x = a4[i];
            if (b) { const float4 r = b4[i]; x.x += r.x; x.y += r.y; x.z += r.z; x.w += r.w; }
            float4 v = make_float4(x.x > 0.f ? x.x : sl * x.x, x.y > 0.f ? x.y : sl * x.y, x.z > 0.f ? x.z : sl * x.z, x.w > 0.f ? x.w : sl * x.w);
            if (keep) {
                const uchar4 k = k4[i];
                v.x *= k.x ? scale : 0.f; v.y *= k.y ? scale : 0.f; v.z *= k.z ? scale : 0.f; v.w *= k.w ? scale : 0.f;
            }
            y4[i] = v;
        }
    } else {
#pragma unroll 4
        for (size_t i = first; i < n; i += step) {
            float x = a[i];
            if (b) x += b[i];
            float v = x > 0.f ? x : sl * x;
            if (keep) v *= keep[i] ? scale : 0.f;
            y[i] = v;
        }
    }
}

// gx = g * [keep * scale] * (x > 0 ? 1 : slope) [+ gres], x = a [+ b];  part[block] = sum g * [keep * scale] * x * (x <= 0)
template <int VEC>
__global__ __launch_bounds__(PR_WG) void prelu_bwd_kernel(const float* __restrict__ g, const float* __restrict__ a, const float* __restrict__ b,
                                                          const float* __restrict__ slope, const unsigned char* __restrict__ keep, float scale,
                                                          const float* gres, float* gx, float* __restrict__ part, size_t n) {
    const float sl = slope[0];
    const size_t first = (size_t)blockIdx.x * PR_WG + threadIdx.x, step = (size_t)gridDim.x * PR_WG;
    float acc = 0.f;
    if (VEC) {
        const float4* g4 = reinterpret_cast<const float4*>(g);
        const float4* a4 = reinterpret_cast<const float4*>(a);
        const float4* b4 = reinterpret_cast<const float4*>(b);
        const float4* r4 = reinterpret_cast<const float4*>(gres);
        const uchar4* k4 = reinterpret_cast<const uchar4*>(keep);
        float4* o4 = reinterpret_cast<float4*>(gx);
        const size_t n4 = n >> 2;
#pragma unroll 2
        for (size_t i = first; i < n4; i += step) {
            float4 gg = g4[i], x = a4[i];
            if (b) { const float4 r = b4[i]; x.x += r.x; x.y += r.y; x.z += r.z; x.w += r.w; }
            if (keep) {
                const uchar4 k = k4[i];
                gg.x *= k.x ? scale : 0.f; gg.y *= k.y ? scale : 0.f; gg.z *= k.z ? scale : 0.f; gg.w *= k.w ? scale : 0.f;
            }
            float4 o = make_float4(gg.x * (x.x > 0.f ? 1.f : sl), gg.y * (x.y > 0.f ? 1.f : sl), gg.z * (x.z > 0.f ? 1.f : sl),
                                   gg.w * (x.w > 0.f ? 1.f : sl));
            if (gres) { const float4 r = r4[i]; o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w; }
            if (gx) o4[i] = o;
            acc += (gg.x * (x.x > 0.f ? 0.f : x.x) + gg.y * (x.y > 0.f ? 0.f : x.y)) + (gg.z * (x.z > 0.f ? 0.f : x.z) + gg.w * (x.w > 0.f ? 0.f : x.w));
        }
    } else {
#pragma unroll 2
        for (size_t i = first; i < n; i += step) {
            float gg = g[i], x = a[i];
            if (b) x += b[i];
            if (keep) gg *= keep[i] ? scale : 0.f;
            float o = gg * (x > 0.f ? 1.f : sl);
            if (gres) o += gres[i];
            if (gx) gx[i] = o;
            acc += gg * (x > 0.f ? 0.f : x);
        }
    }
    block_sum4_to(acc, part + blockIdx.x);
}

// gslope[0] = sum of the `blocks` partials: one workgroup, an order fixed by `blocks` alone
__global__ __launch_bounds__(PR_WG) void prelu_slope_kernel(const float* __restrict__ part, int blocks, float* __restrict__ gslope) {
    float acc = 0.f;
    for (int i = threadIdx.x; i < blocks; i += PR_WG) acc += part[i];
    block_sum4_to(acc, gslope);
}

extern "C" size_t rvsr_prelu_workspace_bytes(void) { return pr_workspace_bytes(); }

extern "C" int rvsr_prelu_plan(size_t n, const void* f0, const void* f1, const void* f2, const void* f3, const void* f4, const void* keep,
                               int* vec, int* blocks) {
    const PrPlan q = pr_plan(n, f0, f1, f2, f3, f4, keep);
    if (q.rc != RVSR_OK) FAIL(q.rc, "%s", q.msg);
    if (vec) *vec = q.vec;
    if (blocks) *blocks = q.blocks;
    return RVSR_OK;
}

extern "C" int rvsr_prelu_forward(const float* a, const float* b, const float* slope, const unsigned char* keep, float scale, float* y, size_t n,
                                  void* stream) {
    const PrPlan q = pr_plan(n, a, b, y, nullptr, nullptr, keep);
    if (q.rc != RVSR_OK) FAIL(q.rc, "%s", q.msg);
    if (!a || !slope || !y) FAIL(RVSR_ERR_BAD_ARG, "prelu: null argument (only b and keep may be NULL)");
    hipStream_t st = (hipStream_t)stream;
    if (q.vec)
        hipLaunchKernelGGL(prelu_fwd_kernel<1>, dim3(q.blocks), dim3(PR_WG), 0, st, a, b, slope, keep, scale, y, n);
    else
        hipLaunchKernelGGL(prelu_fwd_kernel<0>, dim3(q.blocks), dim3(PR_WG), 0, st, a, b, slope, keep, scale, y, n);
    RETURN_LAUNCH("prelu_forward");
}

extern "C" int rvsr_prelu_backward(const float* g, const float* a, const float* b, const float* slope, const unsigned char* keep, float scale,
                                   const float* gres, float* gx, float* gslope, size_t n, void* ws, size_t ws_bytes, void* stream) {
    const PrPlan q = pr_plan(n, g, a, b, gres, gx, keep);
    if (q.rc != RVSR_OK) FAIL(q.rc, "%s", q.msg);
    if (!g || !a || !slope || (!gx && !gslope)) FAIL(RVSR_ERR_BAD_ARG, "prelu backward: null argument (b, keep, gres and one of gx / gslope may be NULL)");
    if (!ws || ws_bytes < pr_workspace_bytes()) FAIL(RVSR_ERR_WORKSPACE, "prelu backward: workspace %zu B < %zu B", ws_bytes, pr_workspace_bytes());
    if (((uintptr_t)ws) & 3) FAIL(RVSR_ERR_BAD_ARG, "prelu backward: workspace is not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)ws;
    if (q.vec)
        hipLaunchKernelGGL(prelu_bwd_kernel<1>, dim3(q.blocks), dim3(PR_WG), 0, st, g, a, b, slope, keep, scale, gres, gx, part, n);
    else
        hipLaunchKernelGGL(prelu_bwd_kernel<0>, dim3(q.blocks), dim3(PR_WG), 0, st, g, a, b, slope, keep, scale, gres, gx, part, n);
    CHECK_LAUNCH("prelu_backward");
    if (gslope) {
        hipLaunchKernelGGL(prelu_slope_kernel, dim3(1), dim3(PR_WG), 0, st, part, q.blocks, gslope);
        CHECK_LAUNCH("prelu_slope");
    }
    return RVSR_OK;
}
