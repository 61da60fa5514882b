// flow_kernels.hip -- the resampling operators of SpyNet (TOF's alignment; codes/models/archs/TOF_arch.py:54-88), one pass each, f32 on
// contiguous tensors:
//   * flow warp = arch_util.flow_warp (arch_util.py:47-80): F.grid_sample(align_corners=True) at pixel + flow, bilinear / nearest,
//     zeros / border padding, with the gradients of the image (scatter, float atomics) and of the flow (gather, no atomics)
//   * F.avg_pool2d(x, 2, 2) of the image pyramids                                               TOF_arch.py:66-76
//   * scale * F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True) of the flow  TOF_arch.py:81-82
// One thread per pixel (warp) or element (pool, upsample), lanes along W, grid-stride loops.  Every tensor index is checked against the
// frame before it is used: frames down to 1 x 1 and flows of any size (infinite or NaN included) read and write inside the tensors only.
#include "glue_common.h"

// ---------------------------------------------------------------- flow warp
// Sampling coordinate of pixel `i` of an axis of `n` pixels displaced by `f`.  The reference normalises, g = 2 (i + f) / max(n - 1, 1) - 1
// (arch_util.py:68-69), and grid_sample (align_corners=True) un-normalises, (g + 1) / 2 * (n - 1): that round trip is i + f, which is what
// is computed here -- without the two or three ulps the round trip loses wherever n - 1 is no power of two, so that a zero flow is the
// identity and an integer flow a shift, bit for bit.  n == 1: the round trip multiplies by n - 1 = 0, the coordinate is 0 whatever the flow.
// border: clipped to [0, n - 1]; *dflow = d coordinate / d flow: 1 strictly inside (0, n - 1), 0 on and beyond the edges (or n == 1).
__device__ __forceinline__ float warp_coord(int i, float f, int n, int border, float* dflow) {
    if (n == 1) {
        *dflow = 0.f;
        return 0.f;
    }
    float c = (float)i + f;
    float d = 1.f;
    if (border) {   // (grid_sample's clip_coordinates_set_grad: the edges themselves count as clipped, c <= 0 and c >= n - 1 get gradient 0)
        if (c <= 0.f) {
            d = 0.f;
            c = 0.f;
        } else if (c >= (float)(n - 1)) {
            d = 0.f;
            c = (float)(n - 1);
        } else if (!(c == c)) {   // NaN: the clip of the reference leaves it; no tap below is in the frame either way
            d = 0.f;
        }
    }
    *dflow = d;
    return c;
}
// floor / round-half-even of a coordinate as a tap index; anything the frame cannot hold (huge, infinite, NaN) -> -2, out of every frame
__device__ __forceinline__ int warp_tap(float r) { return (r >= -1.f && r <= 2147483000.f) ? (int)r : -2; }

struct WarpTaps {
    int x0, y0;              // north-west tap; the others are +1
    float wx0, wx1, wy0, wy1;   // bilinear weights of the columns x0, x0 + 1 and the rows y0, y0 + 1
    float dx, dy;            // d coordinate / d flow
};
__device__ __forceinline__ WarpTaps warp_taps(const float* __restrict__ flow, size_t pix, int y, int x, int H, int W, int nearest, int border) {
    WarpTaps t;
    const float cx = warp_coord(x, flow[2 * pix], W, border, &t.dx), cy = warp_coord(y, flow[2 * pix + 1], H, border, &t.dy);
    if (nearest) {
        t.x0 = warp_tap(rintf(cx));
        t.y0 = warp_tap(rintf(cy));
        t.wx0 = t.wy0 = 1.f;
        t.wx1 = t.wy1 = 0.f;
    } else {
        const float fx = floorf(cx), fy = floorf(cy);
        t.x0 = warp_tap(fx);
        t.y0 = warp_tap(fy);
        t.wx1 = cx - fx;
        t.wx0 = (fx + 1.f) - cx;
        t.wy1 = cy - fy;
        t.wy0 = (fy + 1.f) - cy;
    }
    return t;
}

__global__ void flow_warp_fwd_kernel(const float* __restrict__ x, const float* __restrict__ flow, float* __restrict__ out, int B, int C,
                                     int H, int W, int nearest, int border) {
    const size_t hw = (size_t)H * W, n = (size_t)B * hw;
    LOOP(i, n) {
        const int px = (int)(i % W), py = (int)((i / W) % H);
        const size_t b = i / hw;
        const WarpTaps t = warp_taps(flow, i, py, px, H, W, nearest, border);
        const bool okx0 = t.x0 >= 0 && t.x0 < W, okx1 = !nearest && t.x0 >= -1 && t.x0 < W - 1;
        const bool oky0 = t.y0 >= 0 && t.y0 < H, oky1 = !nearest && t.y0 >= -1 && t.y0 < H - 1;
        const size_t o00 = (size_t)(oky0 ? t.y0 : 0) * W + (okx0 ? t.x0 : 0), o01 = (size_t)(oky0 ? t.y0 : 0) * W + (okx1 ? t.x0 + 1 : 0);
        const size_t o10 = (size_t)(oky1 ? t.y0 + 1 : 0) * W + (okx0 ? t.x0 : 0), o11 = (size_t)(oky1 ? t.y0 + 1 : 0) * W + (okx1 ? t.x0 + 1 : 0);
        for (int c = 0; c < C; ++c) {
            const float* p = x + (b * C + c) * hw;
            const float v00 = p[o00], v01 = p[o01], v10 = p[o10], v11 = p[o11];   // (always inside the plane; validity by select)
            float v = 0.f;
            if (oky0 && okx0) v += v00 * (t.wx0 * t.wy0);
            if (oky0 && okx1) v += v01 * (t.wx1 * t.wy0);
            if (oky1 && okx0) v += v10 * (t.wx0 * t.wy1);
            if (oky1 && okx1) v += v11 * (t.wx1 * t.wy1);
            out[(b * C + c) * hw + (size_t)py * W + px] = v;
        }
    }
}

// gflow (NULL: skipped): one thread gathers its own pixel over the channels, no atomics.  gx (NULL: skipped; zero-filled by the caller):
// every thread adds its four taps, float atomics.
__global__ void flow_warp_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ x, const float* __restrict__ flow,
                                     float* __restrict__ gx, float* __restrict__ gflow, int B, int C, int H, int W, int nearest, int border) {
    const size_t hw = (size_t)H * W, n = (size_t)B * hw;
    LOOP(i, n) {
        const int px = (int)(i % W), py = (int)((i / W) % H);
        const size_t b = i / hw;
        const WarpTaps t = warp_taps(flow, i, py, px, H, W, nearest, border);
        const bool okx0 = t.x0 >= 0 && t.x0 < W, okx1 = !nearest && t.x0 >= -1 && t.x0 < W - 1;
        const bool oky0 = t.y0 >= 0 && t.y0 < H, oky1 = !nearest && t.y0 >= -1 && t.y0 < H - 1;
        const size_t o00 = (size_t)(oky0 ? t.y0 : 0) * W + (okx0 ? t.x0 : 0), o01 = (size_t)(oky0 ? t.y0 : 0) * W + (okx1 ? t.x0 + 1 : 0);
        const size_t o10 = (size_t)(oky1 ? t.y0 + 1 : 0) * W + (okx0 ? t.x0 : 0), o11 = (size_t)(oky1 ? t.y0 + 1 : 0) * W + (okx1 ? t.x0 + 1 : 0);
        float gcx = 0.f, gcy = 0.f;
        for (int c = 0; c < C; ++c) {
            const size_t plane = (b * C + c) * hw;
            const float g = gout[plane + (size_t)py * W + px];
            if (gflow != nullptr && !nearest) {
                const float* p = x + plane;
                const float v00 = (oky0 && okx0) ? p[o00] : 0.f, v01 = (oky0 && okx1) ? p[o01] : 0.f;
                const float v10 = (oky1 && okx0) ? p[o10] : 0.f, v11 = (oky1 && okx1) ? p[o11] : 0.f;
                gcx += g * ((v01 - v00) * t.wy0 + (v11 - v10) * t.wy1);
                gcy += g * ((v10 - v00) * t.wx0 + (v11 - v01) * t.wx1);
            }
            if (gx != nullptr) {
                float* q = gx + plane;
                if (oky0 && okx0) atomicAdd(q + o00, g * (t.wx0 * t.wy0));
                if (oky0 && okx1) atomicAdd(q + o01, g * (t.wx1 * t.wy0));
                if (oky1 && okx0) atomicAdd(q + o10, g * (t.wx0 * t.wy1));
                if (oky1 && okx1) atomicAdd(q + o11, g * (t.wx1 * t.wy1));
            }
        }
        if (gflow != nullptr) {
            gflow[2 * i] = gcx * t.dx;
            gflow[2 * i + 1] = gcy * t.dy;
        }
    }
}

// ---------------------------------------------------------------- 2 x 2 average pool
__global__ void avgpool2_fwd_kernel(const float* __restrict__ in, float* __restrict__ out, size_t planes, int H, int W) {
    const int Ho = H / 2, Wo = W / 2;
    const size_t n = planes * Ho * Wo;
    LOOP(i, n) {
        const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho);
        const float* p = in + (i / ((size_t)Wo * Ho)) * H * W + (size_t)(2 * oy) * W + 2 * ox;   // (2 oy + 1 < H, 2 ox + 1 < W by the floor)
        out[i] = (((p[0] + p[1]) + p[W]) + p[W + 1]) * 0.25f;
    }
}
__global__ void avgpool2_bwd_kernel(const float* __restrict__ gout, float* __restrict__ gin, size_t planes, int H, int W) {
    const int Ho = H / 2, Wo = W / 2;
    const size_t n = planes * H * W;
    LOOP(i, n) {
        const int ix = (int)(i % W), iy = (int)((i / W) % H);
        const bool in = (iy >> 1) < Ho && (ix >> 1) < Wo;   // an odd last row / column took no part
        gin[i] = in ? 0.25f * gout[(i / ((size_t)W * H)) * Ho * Wo + (size_t)(iy >> 1) * Wo + (ix >> 1)] : 0.f;
    }
}

// ---------------------------------------------------------------- x2 bilinear upsample, align_corners=True
struct LerpAC {
    int i0, i1;
    float l0, l1;
};
// source taps of destination index d: source coordinate d * (n - 1) / (2n - 1), 0 for n == 1 (PyTorch area_pixel_compute_scale).  Tap and
// weight come from the integer quotient and remainder, one rounding each -- the float product (n - 1) / (2n - 1) * d loses 2e-5 of a pixel
// at d = 500, more than the 1e-5 the resampling kernels are held to.
__device__ __forceinline__ LerpAC up_ac_src(int d, int n) {
    const int num = d * (n - 1), den = 2 * n - 1;   // (d < 2n, n < 2^15 by the entry's check: no overflow)
    LerpAC r;
    r.i0 = min(num / den, n - 1);
    r.i1 = r.i0 + (r.i0 < n - 1 ? 1 : 0);
    r.l1 = (float)(num - r.i0 * den) / (float)den;
    r.l0 = 1.f - r.l1;
    return r;
}
__global__ void upsample2_ac_fwd_kernel(const float* __restrict__ in, float* __restrict__ out, size_t planes, int H, int W, float scale) {
    const int Ho = 2 * H, Wo = 2 * W;
    const size_t n = planes * Ho * Wo;
    LOOP(i, n) {
        const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho);
        const LerpAC ly = up_ac_src(oy, H), lx = up_ac_src(ox, W);
        const float* p = in + (i / ((size_t)Wo * Ho)) * H * W;
        const float v = ly.l0 * (lx.l0 * p[(size_t)ly.i0 * W + lx.i0] + lx.l1 * p[(size_t)ly.i0 * W + lx.i1]) +
                        ly.l1 * (lx.l0 * p[(size_t)ly.i1 * W + lx.i0] + lx.l1 * p[(size_t)ly.i1 * W + lx.i1]);
        out[i] = v * scale;
    }
}
// Gather: input (iy, ix) is a tap of the outputs whose source coordinate lies within one pixel of it; the source of output 2i + k is
// i + (k (n - 1) - i) / (2n - 1), so rows 2 iy - 3 .. 2 iy + 4 hold them all.  The forward's index map is evaluated again for each
// candidate, rows and columns apart (8 + 8 weights), and the sum runs in one fixed order.
#define UP_AC_LO 3
#define UP_AC_N 8
__global__ void upsample2_ac_bwd_kernel(const float* __restrict__ gout, float* __restrict__ gin, size_t planes, int H, int W, float scale) {
    const int Ho = 2 * H, Wo = 2 * W;
    const size_t n = planes * H * W;
    LOOP(i, n) {
        const int ix = (int)(i % W), iy = (int)((i / W) % H);
        const float* g = gout + (i / ((size_t)W * H)) * Ho * Wo;
        float wx[UP_AC_N];
#pragma unroll
        for (int k = 0; k < UP_AC_N; ++k) {
            const int ox = 2 * ix - UP_AC_LO + k;
            wx[k] = 0.f;
            if (ox >= 0 && ox < Wo) {
                const LerpAC lx = up_ac_src(ox, W);
                wx[k] = (lx.i0 == ix ? lx.l0 : 0.f) + (lx.i1 == ix ? lx.l1 : 0.f);
            }
        }
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < UP_AC_N; ++j) {
            const int oy = 2 * iy - UP_AC_LO + j;
            if (oy < 0 || oy >= Ho) continue;
            const LerpAC ly = up_ac_src(oy, H);
            const float wy = (ly.i0 == iy ? ly.l0 : 0.f) + (ly.i1 == iy ? ly.l1 : 0.f);
            if (wy == 0.f) continue;
            float rowacc = 0.f;
#pragma unroll
            for (int k = 0; k < UP_AC_N; ++k) {
                const int ox = 2 * ix - UP_AC_LO + k;
                if (ox >= 0 && ox < Wo) rowacc += wx[k] * g[(size_t)oy * Wo + ox];
            }
            acc += wy * rowacc;
        }
        gin[i] = acc * scale;
    }
}

// ---------------------------------------------------------------- host side
static int flow_warp_check(const char* what, int B, int C, int H, int W, int interp, int padding) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) FAIL(RVSR_ERR_BAD_ARG, "%s: empty shape (%d, %d, %d, %d)", what, B, C, H, W);
    if (interp != 0 && interp != 1) FAIL(RVSR_ERR_UNSUPPORTED, "%s: interpolation %d (0 bilinear, 1 nearest)", what, interp);
    if (padding != 0 && padding != 1) FAIL(RVSR_ERR_UNSUPPORTED, "%s: padding %d (0 zeros, 1 border; reflection is not built)", what, padding);
    return RVSR_OK;
}
extern "C" int rvsr_flow_warp_forward(const float* x, const float* flow, float* out, int B, int C, int H, int W, int interp, int padding,
                                      void* stream) {
    if (!x || !flow || !out) FAIL(RVSR_ERR_BAD_ARG, "flow_warp: null argument");
    const int rc = flow_warp_check("flow_warp", B, C, H, W, interp, padding);
    if (rc) return rc;
    const size_t n = (size_t)B * H * W;
    hipLaunchKernelGGL(flow_warp_fwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, x, flow, out, B, C, H, W, interp, padding);
    RETURN_LAUNCH("flow_warp_fwd");
}
extern "C" int rvsr_flow_warp_backward(const float* gout, const float* x, const float* flow, float* gx, float* gflow, int B, int C, int H,
                                       int W, int interp, int padding, void* stream) {
    if (!gout || !flow || (gflow && !x)) FAIL(RVSR_ERR_BAD_ARG, "flow_warp backward: null argument");
    const int rc = flow_warp_check("flow_warp backward", B, C, H, W, interp, padding);
    if (rc) return rc;
    if (!gx && !gflow) return RVSR_OK;
    const size_t n = (size_t)B * H * W;
    hipLaunchKernelGGL(flow_warp_bwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, gout, x, flow, gx, gflow, B, C, H, W, interp,
                       padding);
    RETURN_LAUNCH("flow_warp_bwd");
}

extern "C" int rvsr_avgpool2_forward(const float* in, float* out, size_t planes, int H, int W, void* stream) {
    if (!in || planes == 0 || H <= 0 || W <= 0) FAIL(RVSR_ERR_BAD_ARG, "avgpool2: null/empty argument");
    const size_t n = planes * (H / 2) * (W / 2);
    if (n == 0) return RVSR_OK;   // (a frame of one row or column pools to nothing)
    if (!out) FAIL(RVSR_ERR_BAD_ARG, "avgpool2: null output");
    hipLaunchKernelGGL(avgpool2_fwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, in, out, planes, H, W);
    RETURN_LAUNCH("avgpool2_fwd");
}
extern "C" int rvsr_avgpool2_backward(const float* gout, float* gin, size_t planes, int H, int W, void* stream) {
    if (!gin || planes == 0 || H <= 0 || W <= 0) FAIL(RVSR_ERR_BAD_ARG, "avgpool2 backward: null/empty argument");
    if (!gout && (H / 2) * (W / 2) != 0) FAIL(RVSR_ERR_BAD_ARG, "avgpool2 backward: null gradient");
    const size_t n = planes * H * W;
    hipLaunchKernelGGL(avgpool2_bwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, gout, gin, planes, H, W);
    RETURN_LAUNCH("avgpool2_bwd");
}

extern "C" int rvsr_upsample2_ac_forward(const float* in, float* out, size_t planes, int H, int W, float scale, void* stream) {
    if (!in || !out || planes == 0 || H <= 0 || W <= 0) FAIL(RVSR_ERR_BAD_ARG, "upsample2_ac: null/empty argument");
    if (H >= (1 << 15) || W >= (1 << 15)) FAIL(RVSR_ERR_UNSUPPORTED, "upsample2_ac: a %d x %d frame (sides below 32768)", H, W);
    const size_t n = planes * H * W * 4;
    hipLaunchKernelGGL(upsample2_ac_fwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, in, out, planes, H, W, scale);
    RETURN_LAUNCH("upsample2_ac_fwd");
}
extern "C" int rvsr_upsample2_ac_backward(const float* gout, float* gin, size_t planes, int H, int W, float scale, void* stream) {
    if (!gout || !gin || planes == 0 || H <= 0 || W <= 0) FAIL(RVSR_ERR_BAD_ARG, "upsample2_ac backward: null/empty argument");
    if (H >= (1 << 15) || W >= (1 << 15)) FAIL(RVSR_ERR_UNSUPPORTED, "upsample2_ac backward: a %d x %d frame (sides below 32768)", H, W);
    const size_t n = planes * H * W;
    hipLaunchKernelGGL(upsample2_ac_bwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, gout, gin, planes, H, W, scale);
    RETURN_LAUNCH("upsample2_ac_bwd");
}
