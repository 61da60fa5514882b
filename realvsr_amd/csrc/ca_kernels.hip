// ca_kernels.hip -- channel attention of RCAN (codes/models/archs/RCAN_arch.py:30-70) as one fused operator on f32 NCHW tensors:
//
//   s[b,c] = mean_hw u[b,c]      z[b,j] = relu(W1[j,:] . s[b,:] + b1[j])      a[b,c] = sigmoid(W2[c,:] . z[b,:] + b2[c])
//   out = (x ? x : 0) + res_scale * u * a
//
// Memory-bound throughout (the matrices are C x C/r, 64 x 4 in the reference's option files): no matrix cores, no atomics.  Bytes moved
// per call, in passes over one B x C x H x W tensor:
//   forward   ca_pool_kernel        reads u                                  1      (writes B * C * S partial sums)
//             ca_scale_kernel       reads u and x, writes out                3      (2 without x)
//   backward  ca_bwd_dot_kernel     reads gout and u                         2
//             ca_bwd_gate_kernel    the small-matrix backward                0      (one workgroup, B * C values)
//             ca_bwd_scale_kernel   reads gout, writes gu                    2
// Every sum runs in an order fixed by the launch geometry alone: results are bit-identical from run to run.  Slicing and load width come
// from ca_plan.h.
#include "ca_plan.h"

#include "glue_common.h"

// ---------------------------------------------------------------------------------------------
// Plane sums: workgroup (plane, q) sums slice q of plane `plane` of u (DOT: of g * u) into part[plane * S + q].
// Four independent 16-byte loads per thread and tensor in flight, wave reduction, then LDS across the four waves.
template <int DOT>
__global__ __launch_bounds__(CA_WG) void ca_pool_kernel(const float* __restrict__ u, const float* __restrict__ g, float* __restrict__ part,
                                                        int HW, int S, int chunk, int vec) {
    const unsigned plane = blockIdx.x / (unsigned)S, q = blockIdx.x - plane * (unsigned)S;
    const int lo = (int)q * chunk, hi = lo + chunk < HW ? lo + chunk : HW, tid = threadIdx.x;
    const float* pu = u + (size_t)plane * HW + lo;
    const float* pg = DOT ? g + (size_t)plane * HW + lo : nullptr;
    const int n = hi > lo ? hi - lo : 0;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (vec) {   // (uniform) H * W % 4 == 0 and 16-byte-aligned bases: plane starts and slice starts are whole float4s
        const float4* u4 = reinterpret_cast<const float4*>(pu);
        const float4* g4 = reinterpret_cast<const float4*>(pg);
        const int n4 = n >> 2;
        int i = tid;
        for (; i + 3 * CA_WG < n4; i += 4 * CA_WG) {
            float4 a0 = u4[i], a1 = u4[i + CA_WG], a2 = u4[i + 2 * CA_WG], a3 = u4[i + 3 * CA_WG];
            if (DOT) {
                const float4 b0 = g4[i], b1 = g4[i + CA_WG], b2 = g4[i + 2 * CA_WG], b3 = g4[i + 3 * CA_WG];
                s0 += (a0.x * b0.x + a0.y * b0.y) + (a0.z * b0.z + a0.w * b0.w);
                s1 += (a1.x * b1.x + a1.y * b1.y) + (a1.z * b1.z + a1.w * b1.w);
                s2 += (a2.x * b2.x + a2.y * b2.y) + (a2.z * b2.z + a2.w * b2.w);
                s3 += (a3.x * b3.x + a3.y * b3.y) + (a3.z * b3.z + a3.w * b3.w);
            } else {
                s0 += (a0.x + a0.y) + (a0.z + a0.w);
                s1 += (a1.x + a1.y) + (a1.z + a1.w);
                s2 += (a2.x + a2.y) + (a2.z + a2.w);
                s3 += (a3.x + a3.y) + (a3.z + a3.w);
            }
        }
        for (; i < n4; i += CA_WG) {
            const float4 a0 = u4[i];
            if (DOT) {
                const float4 b0 = g4[i];
                s0 += (a0.x * b0.x + a0.y * b0.y) + (a0.z * b0.z + a0.w * b0.w);
            } else {
                s0 += (a0.x + a0.y) + (a0.z + a0.w);
            }
        }
    } else {     // odd planes / unaligned views: scalar loads, the same unrolling, a strided tail
        int i = tid;
        for (; i + 3 * CA_WG < n; i += 4 * CA_WG) {
            const float a0 = pu[i], a1 = pu[i + CA_WG], a2 = pu[i + 2 * CA_WG], a3 = pu[i + 3 * CA_WG];
            if (DOT) {
                s0 += a0 * pg[i];
                s1 += a1 * pg[i + CA_WG];
                s2 += a2 * pg[i + 2 * CA_WG];
                s3 += a3 * pg[i + 3 * CA_WG];
            } else {
                s0 += a0; s1 += a1; s2 += a2; s3 += a3;
            }
        }
        for (; i < n; i += CA_WG) s0 += DOT ? pu[i] * pg[i] : pu[i];
    }
    block_sum4_to((s0 + s1) + (s2 + s3), part + blockIdx.x);
}

// dst = (X ? x : 0) + k * src + add over one slice of one plane
template <int X>
__device__ __forceinline__ void ca_stream(const float* __restrict__ src, const float* __restrict__ x, float* __restrict__ dst, int n, int vec,
                                          float k, float add) {
    const int tid = threadIdx.x;
    if (vec) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        const float4* x4 = reinterpret_cast<const float4*>(x);
        float4* d4 = reinterpret_cast<float4*>(dst);
        const int n4 = n >> 2;
        int i = tid;
        for (; i + 3 * CA_WG < n4; i += 4 * CA_WG) {
            float4 v[4], r[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = s4[i + j * CA_WG];
            if (X) {
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] = x4[i + j * CA_WG];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float4 o;
                o.x = fmaf(k, v[j].x, X ? r[j].x : add);
                o.y = fmaf(k, v[j].y, X ? r[j].y : add);
                o.z = fmaf(k, v[j].z, X ? r[j].z : add);
                o.w = fmaf(k, v[j].w, X ? r[j].w : add);
                d4[i + j * CA_WG] = o;
            }
        }
        for (; i < n4; i += CA_WG) {
            const float4 v = s4[i];
            float4 r = {add, add, add, add};
            if (X) r = x4[i];
            float4 o;
            o.x = fmaf(k, v.x, r.x);
            o.y = fmaf(k, v.y, r.y);
            o.z = fmaf(k, v.z, r.z);
            o.w = fmaf(k, v.w, r.w);
            d4[i] = o;
        }
    } else {
        int i = tid;
        for (; i + 3 * CA_WG < n; i += 4 * CA_WG) {
            float v[4], r[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = src[i + j * CA_WG];
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = X ? x[i + j * CA_WG] : add;
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[i + j * CA_WG] = fmaf(k, v[j], r[j]);
        }
        for (; i < n; i += CA_WG) dst[i] = fmaf(k, src[i], X ? x[i] : add);
    }
}

// ---------------------------------------------------------------------------------------------
// Workgroup (plane = (b, c), q): finishes the C x S partial sums of batch element b into LDS, computes the Cr hidden values and the gate
// of its own channel -- C * Cr + Cr FMAs, redundant per workgroup and free next to the stream -- then streams slice q of `out`.  The
// q == 0 workgroup of a plane writes pooled / gate, that of channel 0 also the hidden values of b.
template <int X>
__global__ __launch_bounds__(CA_WG) void ca_scale_kernel(const float* __restrict__ u, const float* __restrict__ x, const float* __restrict__ part,
                                                         const float* __restrict__ w1, const float* __restrict__ b1,
                                                         const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ out,
                                                         float* __restrict__ pooled, float* __restrict__ hidden, float* __restrict__ gate,
                                                         int C, int Cr, int HW, int S, int chunk, int vec, float res_scale, float inv_hw) {
    extern __shared__ float ca_lds[];   // [C] pooled | [Cr] hidden | [1] gate
    float* sS = ca_lds;
    float* sZ = ca_lds + C;
    float* sA = sZ + Cr;
    const unsigned plane = blockIdx.x / (unsigned)S, q = blockIdx.x - plane * (unsigned)S;
    const unsigned b = plane / (unsigned)C, c = plane - b * (unsigned)C;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int cc = tid; cc < C; cc += CA_WG) {
        const float* pp = part + ((size_t)b * C + cc) * S;
        float s = 0.f;
        for (int k = 0; k < S; ++k) s += pp[k];
        sS[cc] = s * inv_hw;
    }
    __syncthreads();
    for (int j = wave; j < Cr; j += CA_WG / 64) {
        float acc = 0.f;
        for (int cc = lane; cc < C; cc += 64) acc = fmaf(w1[(size_t)j * C + cc], sS[cc], acc);
        acc = wave_sum(acc);
        if (lane == 0) sZ[j] = fmaxf(acc + b1[j], 0.f);
    }
    __syncthreads();
    if (wave == 0) {
        float acc = 0.f;
        for (int j = lane; j < Cr; j += 64) acc = fmaf(w2[(size_t)c * Cr + j], sZ[j], acc);
        acc = wave_sum(acc);
        if (lane == 0) sA[0] = 1.f / (1.f + expf(-(acc + b2[c])));
    }
    __syncthreads();
    const float a = sA[0];
    if (q == 0) {
        if (tid == 0) {
            gate[plane] = a;
            pooled[plane] = sS[c];
        }
        if (c == 0)
            for (int j = tid; j < Cr; j += CA_WG) hidden[(size_t)b * Cr + j] = sZ[j];
    }
    const int lo = (int)q * chunk, hi = lo + chunk < HW ? lo + chunk : HW;
    const size_t off = (size_t)plane * HW + lo;
    ca_stream<X>(u + off, X ? x + off : nullptr, out + off, hi > lo ? hi - lo : 0, vec, res_scale * a, 0.f);
}

// ---------------------------------------------------------------------------------------------
// The small-matrix backward, one workgroup.  d[b,c] = sum_q part;  gp2 = res_scale * d * a * (1 - a);  gz = (W2^T gp2) * [z > 0];
// gs = W1^T gz / (H * W) (the broadcast term of gu, left in the workspace for ca_bwd_scale_kernel);  gW2 = sum_b gp2 (x) z, gb2 = sum_b gp2,
// gW1 = sum_b gz (x) s, gb1 = sum_b gz: one thread per output element, b in ascending order, WRITTEN (not accumulated).
#define CA_GATE_WG 1024
__global__ __launch_bounds__(CA_GATE_WG) void ca_bwd_gate_kernel(const float* __restrict__ part, const float* __restrict__ w1,
                                                                const float* __restrict__ w2, const float* __restrict__ pooled,
                                                                const float* __restrict__ hidden, const float* __restrict__ gate,
                                                                float* gs, float* gp2, float* gz, float* __restrict__ gw1,
                                                                float* __restrict__ gb1, float* __restrict__ gw2, float* __restrict__ gb2,
                                                                int B, int C, int Cr, int S, float res_scale, float inv_hw) {
    const int tid = threadIdx.x;
    const long BC = (long)B * C, BR = (long)B * Cr;
    for (long i = tid; i < BC; i += CA_GATE_WG) {
        const float* pp = part + (size_t)i * S;
        float d = 0.f;
        for (int k = 0; k < S; ++k) d += pp[k];
        const float a = gate[i];
        gp2[i] = res_scale * d * a * (1.f - a);
    }
    __syncthreads();   // (workgroup-scope: the values above are read back through this CU's cache)
    for (long i = tid; i < BR; i += CA_GATE_WG) {
        const long b = i / Cr;
        const int j = (int)(i - b * Cr);
        float acc = 0.f;
        for (int c = 0; c < C; ++c) acc = fmaf(w2[(size_t)c * Cr + j], gp2[b * C + c], acc);
        gz[i] = hidden[i] > 0.f ? acc : 0.f;
    }
    __syncthreads();
    const long CR = (long)C * Cr;
    const long n_gs = BC, n_w2 = gw2 ? CR : 0, n_b2 = gb2 ? C : 0, n_w1 = gw1 ? CR : 0, n_b1 = gb1 ? Cr : 0;
    const long total = n_gs + n_w2 + n_b2 + n_w1 + n_b1;
    for (long i = tid; i < total; i += CA_GATE_WG) {
        long e = i;
        if (e < n_gs) {
            const long b = e / C;
            const int c = (int)(e - b * C);
            float acc = 0.f;
            for (int j = 0; j < Cr; ++j) acc = fmaf(w1[(size_t)j * C + c], gz[b * Cr + j], acc);
            gs[e] = acc * inv_hw;
            continue;
        }
        e -= n_gs;
        if (e < n_w2) {          // gW2[c][j]
            const int c = (int)(e / Cr), j = (int)(e - (long)c * Cr);
            float acc = 0.f;
            for (int b = 0; b < B; ++b) acc = fmaf(gp2[(size_t)b * C + c], hidden[(size_t)b * Cr + j], acc);
            gw2[e] = acc;
            continue;
        }
        e -= n_w2;
        if (e < n_b2) {
            float acc = 0.f;
            for (int b = 0; b < B; ++b) acc += gp2[(size_t)b * C + e];
            gb2[e] = acc;
            continue;
        }
        e -= n_b2;
        if (e < n_w1) {          // gW1[j][c]
            const int j = (int)(e / C), c = (int)(e - (long)j * C);
            float acc = 0.f;
            for (int b = 0; b < B; ++b) acc = fmaf(gz[(size_t)b * Cr + j], pooled[(size_t)b * C + c], acc);
            gw1[e] = acc;
            continue;
        }
        e -= n_w1;
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += gz[(size_t)b * Cr + e];
        gb1[e] = acc;
    }
}

// gu = res_scale * a[b,c] * g + gs[b,c]
__global__ __launch_bounds__(CA_WG) void ca_bwd_scale_kernel(const float* __restrict__ g, const float* __restrict__ gate,
                                                             const float* __restrict__ gs, float* __restrict__ gu, int HW, int S, int chunk,
                                                             int vec, float res_scale) {
    const unsigned plane = blockIdx.x / (unsigned)S, q = blockIdx.x - plane * (unsigned)S;
    const int lo = (int)q * chunk, hi = lo + chunk < HW ? lo + chunk : HW;
    const size_t off = (size_t)plane * HW + lo;
    ca_stream<0>(g + off, nullptr, gu + off, hi > lo ? hi - lo : 0, vec, res_scale * gate[plane], gs[plane]);
}

// ---------------------------------------------------------------------------------------------
extern "C" size_t rvsr_channel_attention_workspace_bytes(int B, int C, int H, int W) { return ca_workspace_bytes(B, C, H, W); }

extern "C" int rvsr_channel_attention_plan(int B, int C, int H, int W, const void* u, const void* x, const void* out, int* slices, int* vec) {
    const CaPlan p = ca_plan(B, C, H, W, u, x, out);
    if (p.rc != RVSR_OK) FAIL(p.rc, "%s", p.msg);
    if (slices) *slices = p.slices;
    if (vec) *vec = p.vec;
    return RVSR_OK;
}

static int ca_check(const CaPlan& p, int B, int C, int Cr, int H, int W, void* ws, size_t wsb) {
    if (p.rc != RVSR_OK) FAIL(p.rc, "%s", p.msg);
    if (Cr < 1 || Cr > C) FAIL(RVSR_ERR_UNSUPPORTED, "channel_attention: %d hidden channels for %d channels (need 1 <= Cr <= C)", Cr, C);
    if (!ws || wsb < ca_workspace_bytes(B, C, H, W))
        FAIL(RVSR_ERR_WORKSPACE, "channel_attention: workspace %zu B < %zu B", wsb, ca_workspace_bytes(B, C, H, W));
    if (((uintptr_t)ws) & 3) FAIL(RVSR_ERR_BAD_ARG, "channel_attention: workspace is not 4-byte aligned");
    return RVSR_OK;
}

extern "C" int rvsr_channel_attention_forward(const float* u, const float* x, const float* w1, const float* b1, const float* w2,
                                              const float* b2, float* out, float* pooled, float* hidden, float* gate, int B, int C, int Cr,
                                              int H, int W, float res_scale, void* ws, size_t ws_bytes, void* stream) {
    if (!u || !w1 || !b1 || !w2 || !b2 || !out || !pooled || !hidden || !gate)
        FAIL(RVSR_ERR_UNSUPPORTED, "channel_attention: null argument (only x may be NULL)");
    const CaPlan p = ca_plan(B, C, H, W, u, x, out);
    if (int rc = ca_check(p, B, C, Cr, H, W, ws, ws_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W;
    float* part = (float*)ws;
    const dim3 grid((unsigned)((long)B * C * p.slices));
    const size_t lds = sizeof(float) * ((size_t)C + Cr + 4);
    hipLaunchKernelGGL(ca_pool_kernel<0>, grid, dim3(CA_WG), 0, st, u, (const float*)nullptr, part, HW, p.slices, p.chunk, p.vec);
    CHECK_LAUNCH("ca_pool");
    if (x)
        hipLaunchKernelGGL(ca_scale_kernel<1>, grid, dim3(CA_WG), lds, st, u, x, part, w1, b1, w2, b2, out, pooled, hidden, gate, C, Cr, HW,
                           p.slices, p.chunk, p.vec, res_scale, 1.f / (float)HW);
    else
        hipLaunchKernelGGL(ca_scale_kernel<0>, grid, dim3(CA_WG), lds, st, u, x, part, w1, b1, w2, b2, out, pooled, hidden, gate, C, Cr, HW,
                           p.slices, p.chunk, p.vec, res_scale, 1.f / (float)HW);
    RETURN_LAUNCH("ca_scale");
}

extern "C" int rvsr_channel_attention_backward(const float* gout, const float* u, const float* w1, const float* w2, const float* pooled,
                                               const float* hidden, const float* gate, float* gu, float* gw1, float* gb1, float* gw2,
                                               float* gb2, int B, int C, int Cr, int H, int W, float res_scale, void* ws, size_t ws_bytes,
                                               void* stream) {
    if (!gout || !u || !w1 || !w2 || !pooled || !hidden || !gate || !gu)
        FAIL(RVSR_ERR_UNSUPPORTED, "channel_attention backward: null argument (only the parameter gradients may be NULL)");
    const CaPlan p = ca_plan(B, C, H, W, gout, u, gu);
    if (int rc = ca_check(p, B, C, Cr, H, W, ws, ws_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W;
    const size_t BC = (size_t)B * C;
    float* part = (float*)ws;
    float* gs = part + BC * p.slices;
    float* gp2 = gs + BC;
    float* gz = gp2 + BC;
    const dim3 grid((unsigned)((long)B * C * p.slices));
    hipLaunchKernelGGL(ca_pool_kernel<1>, grid, dim3(CA_WG), 0, st, u, gout, part, HW, p.slices, p.chunk, p.vec);
    CHECK_LAUNCH("ca_bwd_dot");
    hipLaunchKernelGGL(ca_bwd_gate_kernel, dim3(1), dim3(CA_GATE_WG), 0, st, part, w1, w2, pooled, hidden, gate, gs, gp2, gz, gw1, gb1, gw2,
                       gb2, B, C, Cr, p.slices, res_scale, 1.f / (float)HW);
    CHECK_LAUNCH("ca_bwd_gate");
    hipLaunchKernelGGL(ca_bwd_scale_kernel, grid, dim3(CA_WG), 0, st, gout, gate, gs, gu, HW, p.slices, p.chunk, p.vec, res_scale);
    RETURN_LAUNCH("ca_bwd_scale");
}
