// conv_kernels.hip -- 3x3 / 1x1 convolution blocks of the EDVR hot path as implicit GEMMs on the
// gfx950 f32 matrix cores (v_mfma_f32_32x32x2_f32: exact f32, see rvsr_common.h).
//
// Replaces, on the hot path, the reference's nn.Conv2d calls + the elementwise ops around them
// (codes/models/archs/EDVR_arch.py:96-132,166-208,256-319; arch_util.py:121-139):
//   * bias + ReLU / LeakyReLU(0.1) + residual add fused in the epilogue,
//   * torch.cat([a, b], 1) never materialised (two input pointers),
//   * nn.PixelShuffle(2) fused into the store (forward) / the load (backward),
//   * activation derivative fused into the gradient load (TView.act),
//   * data gradient = the same kernel with transposed+flipped weight addressing (w_mode 1),
//     stride-2 data gradient through a zero-inserted view (TView mode 1),
//   * weight gradient: persistent workgroups accumulate gW tiles in registers over many pixel
//     tiles, write deterministic partials, a second kernel reduces them (no atomics).
//
// Tiling (forward): one workgroup = 4 waves = 8 x 32 output pixels x (MT * 32) output channels;
// wave w owns rows 2w, 2w+1 (two 32-pixel N tiles) x MT M tiles.  K is walked in chunks of CC
// input channels: the input tile (+halo) and the weight slice [tap][c][o] live in LDS; the B
// operand is read straight out of the input tile at the tap's shifted address, so no im2col
// buffer exists anywhere.
#include "rvsr_common.h"

#include "conv_plan.h"

template <int KS, int STRIDE, int MT, int CC>
__global__ __launch_bounds__(RVSR_WG, 2) void conv_fwd_kernel(const ConvFwdParams p) {
    constexpr int T = KS * KS, PAD = KS / 2, TH = 8, TW = 32;
    constexpr int IH = (TH - 1) * STRIDE + KS, IW = (TW - 1) * STRIDE + KS;
    constexpr int MP = MT * 32, MPP = MP + 1;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* xs = smem;                  // [CC][IH][IW]
    float* ws = smem + CC * IH * IW;   // [T][CC][MPP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 31, hi = lane >> 5;
    const int tx = blockIdx.x % p.ntx, ty = blockIdx.x / p.ntx;
    const int x0 = tx * TW, y0 = ty * TH, mb = blockIdx.y, b = blockIdx.z;
    const int Ctot = p.in.a.C + p.in.b.C;

    f32x16 acc[MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        acc[m][0] = zero16();
        acc[m][1] = zero16();
    }

    for (int c0 = 0; c0 < Ctot; c0 += CC) {
#pragma unroll 2
        for (int e = tid; e < CC * IH * IW; e += RVSR_WG) {
            const int cc = e / (IH * IW);
            const int rem = e - cc * (IH * IW);
            const int r = rem / IW, s = rem - r * IW;
            const int c = c0 + cc;
            float v = 0.f;
            if (c < Ctot) v = tcat_get(p.in, b, c, y0 * STRIDE - PAD + r, x0 * STRIDE - PAD + s);
            xs[e] = v;
        }
        if (p.w_mode == 0) {  // A[o][(tap, c)] = w[o][c][tap]
#pragma unroll 4
            for (int e = tid; e < MP * CC * T; e += RVSR_WG) {
                const int m = e / (CC * T);
                const int rem = e - m * (CC * T);
                const int cc = rem / T, tap = rem - cc * T;
                const int o = mb * MP + m, c = c0 + cc;
                float v = 0.f;
                if (o < p.Co && c < Ctot) v = p.w[((size_t)o * Ctot + c) * T + tap];
                ws[(tap * CC + cc) * MPP + m] = v;
            }
        } else {  // data gradient: A[i][(tap, k)] = w[k][i][T-1-tap], w stored [Ctot][Co][T]
#pragma unroll 4
            for (int e = tid; e < CC * MP * T; e += RVSR_WG) {
                const int cc = e / (MP * T);
                const int rem = e - cc * (MP * T);
                const int m = rem / T, tap = rem - m * T;
                const int i = mb * MP + m, k = c0 + cc;
                float v = 0.f;
                if (i < p.Co && k < Ctot) v = p.w[((size_t)k * p.Co + i) * T + (T - 1 - tap)];
                ws[(tap * CC + cc) * MPP + m] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < T; ++tap) {
            const int dy = tap / KS, dx = tap % KS;
#pragma unroll 4
            for (int cp = 0; cp < CC / 2; ++cp) {
                const int cc = 2 * cp + hi;
                float a[MT], bv[2];
#pragma unroll
                for (int m = 0; m < MT; ++m) a[m] = ws[(tap * CC + cc) * MPP + m * 32 + lo];
#pragma unroll
                for (int n = 0; n < 2; ++n)
                    bv[n] = xs[cc * (IH * IW) + ((wave * 2 + n) * STRIDE + dy) * IW + lo * STRIDE + dx];
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    acc[m][0] = mfma32(a[m], bv[0], acc[m][0]);
                    acc[m][1] = mfma32(a[m], bv[1], acc[m][1]);
                }
            }
        }
        __syncthreads();
    }

    // epilogue: bias + activation (+ residual | pixel-shuffle | channel split), 128-B row segments
    if (p.ps)
        conv_epilogue<MT, 3>(acc, p, b, mb * (MT * 32), y0 + wave * 2, x0 + lo, hi);
    else if (p.out2 != nullptr)
        conv_epilogue<MT, 2>(acc, p, b, mb * (MT * 32), y0 + wave * 2, x0 + lo, hi);
    else if (p.res != nullptr)
        conv_epilogue<MT, 1>(acc, p, b, mb * (MT * 32), y0 + wave * 2, x0 + lo, hi);
    else
        conv_epilogue<MT, 0>(acc, p, b, mb * (MT * 32), y0 + wave * 2, x0 + lo, hi);
}

// ------------------------------------------------------------------------------------------
template <int KS, int STRIDE, int CCW>
__global__ __launch_bounds__(RVSR_WG) void conv_wgrad_kernel(const ConvWgradParams p) {
    constexpr int T = KS * KS, PAD = KS / 2, TH = 4, TW = 32, NPX = TH * TW;
    constexpr int IH = (TH - 1) * STRIDE + KS, IW = (TW - 1) * STRIDE + KS;
    constexpr int CS = (IH * IW) | 1;  // odd channel stride: lanes walk channels conflict-free
    constexpr int NTOT = T * CCW, NT = (NTOT + 31) / 32, TPW = (2 * NT + 3) / 4;
    constexpr int GP = 65;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* gT = smem;             // [NPX][GP]   gradient tile, pixel-major
    float* xs = smem + NPX * GP;  // [CCW][CS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 31, hi = lane >> 5;
    const int mb = blockIdx.y, c0 = blockIdx.z * CCW;
    const int Ctot = p.x.a.C + p.x.b.C;
    const int m = wave & 1;
    const bool m_live = (mb * 64 + m * 32) < p.Co;

    int boff[TPW];
    bool bval[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int nt = (wave >> 1) + 2 * i;
        const int n = nt * 32 + lo;
        bval[i] = (nt < NT) && (n < NTOT);
        const int tap = n / CCW, cc = n - tap * CCW;
        boff[i] = bval[i] ? cc * CS + (tap / KS) * IW + (tap % KS) : 0;
    }
    f32x16 acc[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) acc[i] = zero16();
    float bsum = 0.f;

    const int ntiles = p.B * p.nty * p.ntx;
    for (int tile = blockIdx.x; tile < ntiles; tile += p.P) {
        const int b = tile / (p.nty * p.ntx);
        const int trem = tile - b * (p.nty * p.ntx);
        const int ty = trem / p.ntx, tx = trem - ty * p.ntx;
        const int y0 = ty * TH, x0 = tx * TW;
        // plain views (the common case) are staged four elements per batch of loads, see tview_get_batch
        if (p.g.mode == 0) {  // (uniform)
            for (int e0 = tid; e0 < 64 * NPX; e0 += 4 * RVSR_WG) {
                int cc[4], yy[4], xx[4];
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = e0 + j * RVSR_WG;
                    const int ol = e / NPX, px = e - ol * NPX;
                    cc[j] = e < 64 * NPX ? mb * 64 + ol : -1;
                    yy[j] = y0 + (px >> 5);
                    xx[j] = x0 + (px & 31);
                }
                tview_get_batch<4>(p.g, b, cc, yy, xx, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = e0 + j * RVSR_WG;
                    const int ol = e / NPX, px = e - ol * NPX;
                    if (e < 64 * NPX) gT[px * GP + ol] = v[j];
                }
            }
        } else {
#pragma unroll 2
            for (int e = tid; e < 64 * NPX; e += RVSR_WG) {
                const int ol = e / NPX, px = e - ol * NPX;
                const int o = mb * 64 + ol;
                float v = 0.f;
                if (o < p.Co) v = tview_get(p.g, b, o, y0 + (px >> 5), x0 + (px & 31));
                gT[px * GP + ol] = v;
            }
        }
        if (p.x.b.p == nullptr && p.x.a.mode == 0) {  // (uniform)
            for (int e0 = tid; e0 < CCW * IH * IW; e0 += 4 * RVSR_WG) {
                int cc[4], yy[4], xx[4];
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = e0 + j * RVSR_WG;
                    const int ci = e / (IH * IW), rem = e - ci * (IH * IW);
                    const int r = rem / IW, s = rem - r * IW;
                    cc[j] = e < CCW * IH * IW ? c0 + ci : -1;
                    yy[j] = y0 * STRIDE - PAD + r;
                    xx[j] = x0 * STRIDE - PAD + s;
                }
                tview_get_batch<4>(p.x.a, b, cc, yy, xx, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = e0 + j * RVSR_WG;
                    const int ci = e / (IH * IW), rem = e - ci * (IH * IW);
                    const int r = rem / IW, s = rem - r * IW;
                    if (e < CCW * IH * IW) xs[ci * CS + r * IW + s] = v[j];
                }
            }
        } else {
#pragma unroll 2
            for (int e = tid; e < CCW * IH * IW; e += RVSR_WG) {
                const int cc = e / (IH * IW);
                const int rem = e - cc * (IH * IW);
                const int r = rem / IW, s = rem - r * IW;
                const int c = c0 + cc;
                float v = 0.f;
                if (c < Ctot) v = tcat_get(p.x, b, c, y0 * STRIDE - PAD + r, x0 * STRIDE - PAD + s);
                xs[cc * CS + r * IW + s] = v;
            }
        }
        __syncthreads();
        if (p.bpart != nullptr && blockIdx.z == 0 && tid < 64) {
            float s = 0.f;
            for (int px = 0; px < NPX; ++px) s += gT[px * GP + tid];
            bsum += s;
        }
        if (m_live) {
#pragma unroll 2
            for (int ks = 0; ks < NPX / 2; ++ks) {
                const int row = ks >> 4, colp = 2 * (ks & 15) + hi;
                const float a = gT[(row * 32 + colp) * GP + m * 32 + lo];
                const int poff = row * STRIDE * IW + colp * STRIDE;
#pragma unroll
                for (int i = 0; i < TPW; ++i) {
                    if ((wave >> 1) + 2 * i < NT) {
                        const float bv = bval[i] ? xs[boff[i] + poff] : 0.f;
                        acc[i] = mfma32(a, bv, acc[i]);
                    }
                }
            }
        }
        __syncthreads();
    }

    if (m_live) {
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int nt = (wave >> 1) + 2 * i;
            const int n = nt * 32 + lo;
            if (nt >= NT || n >= NTOT) continue;
            const int tap = n / CCW, c = c0 + (n - tap * CCW);
            if (c >= Ctot) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = mb * 64 + m * 32 + drow(r, hi);
                if (o < p.Co) p.part[(((size_t)blockIdx.x * p.Co + o) * Ctot + c) * T + tap] = acc[i][r];
            }
        }
    }
    if (p.bpart != nullptr && blockIdx.z == 0 && tid < 64) {
        const int o = mb * 64 + tid;
        if (o < p.Co) p.bpart[(size_t)blockIdx.x * p.Co + o] = bsum;
    }
}

// ------------------------------------------------------------------------------------------
// host side


// exact-f32 forward: the plan's (MT, CC) per geometry
static int launch_fwd(const ConvFwdParams& p, const ConvFwdPlan& q, int ksize, int stride, hipStream_t st) {
    void (*k)(const ConvFwdParams) = nullptr;
#define ROW(KS, STRIDE, CC12, CC4)                                                 \
    if (ksize == KS && stride == STRIDE)                                           \
        k = q.mt == 1 ? conv_fwd_kernel<KS, STRIDE, 1, CC12> : q.mt == 2 ? conv_fwd_kernel<KS, STRIDE, 2, CC12> : conv_fwd_kernel<KS, STRIDE, 4, CC4>
    ROW(3, 1, 16, 8);
    ROW(3, 2, 8, 4);
    ROW(5, 1, 8, 4);
    ROW(5, 2, 4, 4);
    ROW(1, 1, 32, 32);
    ROW(7, 1, 4, 2);
#undef ROW
    return rvsr_conv_launch("conv_fwd", k, dim3(q.gx, q.gy, q.gz), RVSR_WG, q.lds, st, p);
}

static int make_view(TView& v, const float* p, const float* act, float slope, int C, int Hs, int Ws, int mode,
                     int Hv, int Wv) {
    v.p = p;
    v.act = act;
    v.slope = slope;
    v.C = C;
    v.Hs = Hs;
    v.Ws = Ws;
    v.mode = mode;
    if (mode == 0) {
        v.Hv = Hs;
        v.Wv = Ws;
    } else if (mode == 1) {
        v.Hv = Hv;
        v.Wv = Wv;
    } else if (mode == 2) {
        if ((Hs | Ws) & 1 || C % 4) return 1;
        v.Hv = Hs / 2;
        v.Wv = Ws / 2;
    } else {
        return 1;
    }
    return 0;
}

// Validates a rvsr_conv2d_forward call and fills its parameter block (wpack and vec4: rvsr_launch_conv_fwd2, from the plan).
static int conv_fwd_params(ConvFwdParams& p, const float* x1, int C1, const float* x2, int C2, const float* xact, float xact_slope,
                           int in_mode, int Hs, int Ws, const float* weight, const float* bias, const float* residual, float* out1,
                           int Co1, float* out2, int Co2, int B, int ksize, int stride, int w_mode, int act, float slope,
                           int pixel_shuffle, int Hout, int Wout, int addend_period) {
    if (!x1 || !weight || !out1 || B <= 0 || C1 <= 0 || Co1 <= 0) FAIL(RVSR_ERR_BAD_ARG, "conv2d: null/empty argument");
    if (addend_period < 0 || (addend_period > 0 && !residual)) FAIL(RVSR_ERR_BAD_ARG, "conv2d: addend period %d without an addend", addend_period);
    if ((x2 == nullptr) != (C2 == 0) || (out2 == nullptr) != (Co2 == 0))
        FAIL(RVSR_ERR_BAD_ARG, "conv2d: second input/output pointer and channel count disagree");
    if (ksize != 1 && ksize != 3 && ksize != 5 && ksize != 7) FAIL(RVSR_ERR_UNSUPPORTED, "conv2d: kernel size %d (1, 3, 5 or 7 supported)", ksize);
    if (stride != 1 && !(stride == 2 && ksize != 1 && ksize != 7)) FAIL(RVSR_ERR_UNSUPPORTED, "conv2d: stride %d", stride);
    if (in_mode != 0 && (x2 != nullptr || stride != 1)) FAIL(RVSR_ERR_UNSUPPORTED, "conv2d: view mode with concat/stride");
    if (xact && x2) FAIL(RVSR_ERR_UNSUPPORTED, "conv2d: act' fusion with concat input");
    // (an addend with a split or pixel-shuffled output is the plan's to refuse, silently: the caller has a plan B)
    if ((residual || pixel_shuffle) && out2 && !addend_period) FAIL(RVSR_ERR_UNSUPPORTED, "conv2d: residual/pixel-shuffle with split output");
    if (residual && pixel_shuffle && !addend_period) FAIL(RVSR_ERR_UNSUPPORTED, "conv2d: residual with pixel-shuffle");
    if (make_view(p.in.a, x1, xact, xact_slope, C1, Hs, Ws, in_mode, Hout, Wout))
        FAIL(RVSR_ERR_BAD_ARG, "conv2d: bad input view (mode %d, C %d, %dx%d)", in_mode, C1, Hs, Ws);
    make_view(p.in.b, x2, nullptr, 0.f, C2, Hs, Ws, 0, 0, 0);
    const int pad = ksize / 2;
    const int He = (p.in.a.Hv + 2 * pad - ksize) / stride + 1, We = (p.in.a.Wv + 2 * pad - ksize) / stride + 1;
    if (He != Hout || We != Wout) FAIL(RVSR_ERR_BAD_ARG, "conv2d: output size %dx%d, expected %dx%d", Hout, Wout, He, We);
    p.w = weight;
    p.wpack = nullptr;
    p.swz = rvsr_swizzle_enabled();
    p.vec4 = 0;
    p.bias = bias;
    p.res = residual;
    p.res_period = addend_period;
    p.out1 = out1;
    p.out2 = out2;
    p.Co1 = Co1;
    p.Co = Co1 + Co2;
    if (pixel_shuffle && (p.Co % 4)) FAIL(RVSR_ERR_BAD_ARG, "conv2d: pixel-shuffle needs Co %% 4 == 0");
    p.B = B;
    p.Hout = Hout;
    p.Wout = Wout;
    p.w_mode = w_mode & 1;
    p.prepacked = (w_mode >> 1) & 1;
    p.fmt = (w_mode >> 2) & 1;
    p.act = act;
    p.slope = slope;
    p.ps = pixel_shuffle;
    p.ntx = (Wout + 31) / 32;
    return RVSR_OK;
}
// A refusal of the plan: nothing is launched.  (No message for act 3 -- the caller has a plan B -- and no stale one either.)
static int conv_fwd_refuse(const ConvFwdPlan& q) {
    snprintf(rvsr_g_err, sizeof(rvsr_g_err), "%s", q.msg ? q.msg : "");
    return q.rc;
}

// Fused conv block.  See include/realvsr_hip.h for the contract: validate, plan (conv_plan.h), refuse or launch.  One body behind
// rvsr_conv2d_forward (addend_period 0) and rvsr_conv2d_forward_addend.
static int conv2d_forward_call(const float* x1, int C1, const float* x2, int C2, const float* xact, float xact_slope, int in_mode, int Hs,
                               int Ws, const float* weight, const float* bias, const float* residual, float* out1, int Co1, float* out2,
                               int Co2, int B, int ksize, int stride, int w_mode, int act, float slope, int pixel_shuffle, int Hout,
                               int Wout, int addend_period, void* workspace, size_t workspace_bytes, void* stream) {
    ConvFwdParams p;
    const int rc = conv_fwd_params(p, x1, C1, x2, C2, xact, xact_slope, in_mode, Hs, Ws, weight, bias, residual, out1, Co1, out2, Co2, B,
                                   ksize, stride, w_mode, act, slope, pixel_shuffle, Hout, Wout, addend_period);
    if (rc) return rc;
    const ConvFwdPlan q = conv_fwd_plan(p, ksize, stride, rvsr_gemm_mode_now());
    if (q.rc) return conv_fwd_refuse(q);
    hipStream_t st = (hipStream_t)stream;
    switch (q.family) {
        case CONV_FWD_THIN: return rvsr_launch_conv_fwd_thin(p, q, st);
        case CONV_FWD_F32: return launch_fwd(p, q, ksize, stride, st);
        default: return rvsr_launch_conv_fwd2(p, q, ksize, stride, workspace, workspace_bytes, st);   // conv_fwd5 / conv_fwd2
    }
}
// The plan of that call, without a GPU: same arguments, same return code (and rvsr_last_error), nothing launched.
static int conv2d_forward_plan_of(const float* x1, int C1, const float* x2, int C2, const float* xact, float xact_slope, int in_mode, int Hs,
                                  int Ws, const float* weight, const float* bias, const float* residual, float* out1, int Co1, float* out2,
                                  int Co2, int B, int ksize, int stride, int w_mode, int act, float slope, int pixel_shuffle, int Hout,
                                  int Wout, int addend_period, int* plan) {
    ConvFwdParams p;
    const int rc = conv_fwd_params(p, x1, C1, x2, C2, xact, xact_slope, in_mode, Hs, Ws, weight, bias, residual, out1, Co1, out2, Co2, B,
                                   ksize, stride, w_mode, act, slope, pixel_shuffle, Hout, Wout, addend_period);
    if (rc) return rc;
    const ConvFwdPlan q = conv_fwd_plan(p, ksize, stride, rvsr_gemm_mode_now());
    const int row[14] = {q.family, q.mt, q.vec, q.wide, q.nt, q.act_in, q.cc, q.vec4, q.th, q.tw, (int)q.gx, (int)q.gy, (int)q.gz, (int)q.lds};
    for (int i = 0; plan && i < 14; ++i) plan[i] = row[i];
    return q.rc ? conv_fwd_refuse(q) : RVSR_OK;
}
extern "C" int rvsr_conv2d_forward(const float* x1, int C1, const float* x2, int C2, const float* xact,
                                   float xact_slope, int in_mode, int Hs, int Ws, const float* weight,
                                   const float* bias, const float* residual, float* out1, int Co1, float* out2,
                                   int Co2, int B, int ksize, int stride, int w_mode, int act, float slope,
                                   int pixel_shuffle, int Hout, int Wout, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    return conv2d_forward_call(x1, C1, x2, C2, xact, xact_slope, in_mode, Hs, Ws, weight, bias, residual, out1, Co1, out2, Co2, B, ksize,
                               stride, w_mode, act, slope, pixel_shuffle, Hout, Wout, 0, workspace, workspace_bytes, stream);
}
extern "C" int rvsr_conv2d_forward_plan(const float* x1, int C1, const float* x2, int C2, const float* xact,
                                        float xact_slope, int in_mode, int Hs, int Ws, const float* weight,
                                        const float* bias, const float* residual, float* out1, int Co1, float* out2,
                                        int Co2, int B, int ksize, int stride, int w_mode, int act, float slope,
                                        int pixel_shuffle, int Hout, int Wout, int* plan) {
    return conv2d_forward_plan_of(x1, C1, x2, C2, xact, xact_slope, in_mode, Hs, Ws, weight, bias, residual, out1, Co1, out2, Co2, B, ksize,
                                  stride, w_mode, act, slope, pixel_shuffle, Hout, Wout, 0, plan);
}
// out = act((conv + bias) + addend[b % addend_period]): `addend` (addend_period, Co1, Hout, Wout) takes the place of the residual
extern "C" int rvsr_conv2d_forward_addend(const float* x1, int C1, const float* x2, int C2, const float* xact,
                                          float xact_slope, int in_mode, int Hs, int Ws, const float* weight,
                                          const float* bias, const float* addend, float* out1, int Co1, float* out2,
                                          int Co2, int B, int ksize, int stride, int w_mode, int act, float slope,
                                          int pixel_shuffle, int Hout, int Wout, int addend_period, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    return conv2d_forward_call(x1, C1, x2, C2, xact, xact_slope, in_mode, Hs, Ws, weight, bias, addend, out1, Co1, out2, Co2, B, ksize,
                               stride, w_mode, act, slope, pixel_shuffle, Hout, Wout, addend_period, workspace, workspace_bytes, stream);
}
extern "C" int rvsr_conv2d_forward_addend_plan(const float* x1, int C1, const float* x2, int C2, const float* xact,
                                               float xact_slope, int in_mode, int Hs, int Ws, const float* weight,
                                               const float* bias, const float* addend, float* out1, int Co1, float* out2,
                                               int Co2, int B, int ksize, int stride, int w_mode, int act, float slope,
                                               int pixel_shuffle, int Hout, int Wout, int addend_period, int* plan) {
    return conv2d_forward_plan_of(x1, C1, x2, C2, xact, xact_slope, in_mode, Hs, Ws, weight, bias, addend, out1, Co1, out2, Co2, B, ksize,
                                  stride, w_mode, act, slope, pixel_shuffle, Hout, Wout, addend_period, plan);
}

int rvsr_g_gemm_mode = 0;                  // process-wide default
thread_local int rvsr_t_gemm_mode = -1;    // the calling host thread's own choice (-1: follow the default)
extern "C" void rvsr_set_gemm_mode(int mode) { rvsr_g_gemm_mode = (mode >= 0 && mode <= 3) ? mode : 0; }
extern "C" void rvsr_set_gemm_mode_thread(int mode) { rvsr_t_gemm_mode = (mode >= 0 && mode <= 3) ? mode : -1; }
extern "C" int rvsr_get_gemm_mode() { return rvsr_gemm_mode_now(); }
extern "C" size_t rvsr_conv2d_forward_workspace_bytes(int C1, int C2, int Co, int ksize) {
    if (ksize == 7) return 0;   // (exact-f32 family only: it reads the weights where they are, no packed image)
    return rvsr_conv_fwd2_workspace_bytes(ksize, Co, C1 + C2);
}

extern "C" size_t rvsr_conv2d_wgrad_workspace_bytes(int C1, int C2, int Co, int B, int ksize, int stride, int Hout,
                                                    int Wout) {
    const size_t P = conv_wgrad_max_P(ksize, stride, B, Hout, Wout, Co, C1 + C2);
    return sizeof(float) * P * ((size_t)Co * (C1 + C2) * ksize * ksize + Co);
}

template <int KS, int STRIDE, int CCW>
static int launch_wgrad(const ConvWgradParams& p, int gy, int gz, hipStream_t st) {
    constexpr int IH = 3 * STRIDE + KS, IW = 31 * STRIDE + KS, CS = (IH * IW) | 1;
    return rvsr_conv_launch("conv_wgrad", conv_wgrad_kernel<KS, STRIDE, CCW>, dim3(p.P, gy, gz), RVSR_WG, sizeof(float) * (128 * 65 + CCW * CS), st, p);
}

// Validates a weight-gradient call and fills its parameter block (without the slicing: P, part, bpart).
static int conv_wgrad_params(ConvWgradParams& p, const float* x1, int C1, const float* x2, int C2, int Hin, int Win, const float* gout,
                             const float* gact, float gact_slope, int g_mode, int Gs_h, int Gs_w, float* grad_weight, int Co, int B,
                             int ksize, int stride, int Hout, int Wout) {
    if (!x1 || !gout || !grad_weight || B <= 0) FAIL(RVSR_ERR_BAD_ARG, "conv2d_backward_weight: null/empty argument");
    if ((x2 == nullptr) != (C2 == 0)) FAIL(RVSR_ERR_BAD_ARG, "conv2d_backward_weight: x2/C2 disagree");
    if (ksize != 1 && ksize != 3 && ksize != 5 && ksize != 7) FAIL(RVSR_ERR_UNSUPPORTED, "conv2d_backward_weight: kernel size %d", ksize);
    if (stride != 1 && !(stride == 2 && ksize != 1 && ksize != 7)) FAIL(RVSR_ERR_UNSUPPORTED, "conv2d_backward_weight: stride %d", stride);
    if (g_mode != 0 && g_mode != 2) FAIL(RVSR_ERR_UNSUPPORTED, "conv2d_backward_weight: gradient view mode %d", g_mode);
    make_view(p.x.a, x1, nullptr, 0.f, C1, Hin, Win, 0, 0, 0);
    make_view(p.x.b, x2, nullptr, 0.f, C2, Hin, Win, 0, 0, 0);
    if (make_view(p.g, gout, gact, gact_slope, Co, Gs_h, Gs_w, g_mode, 0, 0) || p.g.Hv != Hout || p.g.Wv != Wout)
        FAIL(RVSR_ERR_BAD_ARG, "conv2d_backward_weight: gradient view %dx%d (mode %d) vs output %dx%d", Gs_h, Gs_w, g_mode,
             Hout, Wout);
    const int pad = ksize / 2;
    if ((Hin + 2 * pad - ksize) / stride + 1 != Hout || (Win + 2 * pad - ksize) / stride + 1 != Wout)
        FAIL(RVSR_ERR_BAD_ARG, "conv2d_backward_weight: input %dx%d does not give output %dx%d", Hin, Win, Hout, Wout);
    p.part = p.bpart = nullptr;
    p.B = B;
    p.Co = Co;
    p.Hout = Hout;
    p.Wout = Wout;
    p.ntx = (Wout + 31) / 32;
    p.nty = (Hout + 3) / 4;
    p.P = 0;
    return RVSR_OK;
}

// The plan of a weight-gradient call, without a GPU: the arguments of rvsr_conv2d_backward_weight that the plan looks at, same
// validation and return code, nothing launched.  plan[4] = {family (ConvWgradFamily), P, grid y, grid z}.
extern "C" int rvsr_conv2d_backward_weight_plan(const float* x1, int C1, const float* x2, int C2, int Hin, int Win,
                                                const float* gout, const float* gact, float gact_slope, int g_mode,
                                                int Gs_h, int Gs_w, float* grad_weight, int Co, int B, int ksize, int stride,
                                                int Hout, int Wout, int* plan) {
    ConvWgradParams p;
    const int rc = conv_wgrad_params(p, x1, C1, x2, C2, Hin, Win, gout, gact, gact_slope, g_mode, Gs_h, Gs_w, grad_weight, Co, B, ksize,
                                     stride, Hout, Wout);
    if (rc) return rc;
    const ConvWgradPlan q = conv_wgrad_plan(p, ksize, stride, rvsr_gemm_mode_now());
    const int row[4] = {q.family, q.P, q.gy, q.gz};
    for (int i = 0; plan && i < 4; ++i) plan[i] = row[i];
    return RVSR_OK;
}

extern "C" int rvsr_conv2d_backward_weight(const float* x1, int C1, const float* x2, int C2, int Hin, int Win,
                                           const float* gout, const float* gact, float gact_slope, int g_mode,
                                           int Gs_h, int Gs_w, float* grad_weight, float* grad_bias, int Co, int B,
                                           int ksize, int stride, int Hout, int Wout, int accumulate, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    ConvWgradParams p;
    const int prc = conv_wgrad_params(p, x1, C1, x2, C2, Hin, Win, gout, gact, gact_slope, g_mode, Gs_h, Gs_w, grad_weight, Co, B, ksize,
                                      stride, Hout, Wout);
    if (prc) return prc;
    const size_t need = rvsr_conv2d_wgrad_workspace_bytes(C1, C2, Co, B, ksize, stride, Hout, Wout);
    if (!workspace || workspace_bytes < need)
        FAIL(RVSR_ERR_WORKSPACE, "conv2d_backward_weight: workspace %zu B < %zu B", workspace_bytes, need);
    const ConvWgradPlan q = conv_wgrad_plan(p, ksize, stride, rvsr_gemm_mode_now());
    const size_t nw = (size_t)Co * (C1 + C2) * ksize * ksize;
    p.P = q.P;
    p.part = (float*)workspace;
    p.bpart = grad_bias ? p.part + (size_t)p.P * nw : nullptr;
    hipStream_t st = (hipStream_t)stream;
    int rc = RVSR_ERR_UNSUPPORTED;
    switch (q.family) {
        case CONV_WGRAD_THIN: rc = rvsr_launch_conv_wgrad_thin(p, st); break;
        case CONV_WGRAD2: rc = rvsr_launch_conv_wgrad2(p, q.gy, q.gz, st); break;
        case CONV_WGRAD5: rc = rvsr_launch_conv_wgrad5(p, stride, q.gy, q.gz, st); break;
        case CONV_WGRAD_F32_5: rc = stride == 1 ? launch_wgrad<5, 1, 16>(p, q.gy, q.gz, st) : launch_wgrad<5, 2, 16>(p, q.gy, q.gz, st); break;
        case CONV_WGRAD_1X1S: rc = rvsr_launch_conv_wgrad1x1s(p, q.gy, q.gz, st); break;
        case CONV_WGRAD_1X1: rc = rvsr_launch_conv_wgrad1x1(p, q.gy, q.gz, st); break;
        case CONV_WGRAD_F32_3S1: rc = launch_wgrad<3, 1, 64>(p, q.gy, q.gz, st); break;
        case CONV_WGRAD_S2: rc = rvsr_launch_conv_wgrad_s2(p, q.gy, q.gz, st); break;
        case CONV_WGRAD_F32_3S2: rc = launch_wgrad<3, 2, 32>(p, q.gy, q.gz, st); break;
        case CONV_WGRAD_F32_1: rc = launch_wgrad<1, 1, 64>(p, q.gy, q.gz, st); break;
        case CONV_WGRAD_F32_7: rc = launch_wgrad<7, 1, 8>(p, q.gy, q.gz, st); break;
    }
    if (rc) return rc;
    rvsr_launch_reduce(p.part, p.P, nw, grad_weight, accumulate, st, p.bpart, (size_t)Co, grad_bias);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) FAIL(RVSR_ERR_LAUNCH, "conv_wgrad reduce launch: %s", hipGetErrorString(e));
    return RVSR_OK;
}
