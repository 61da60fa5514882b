// metric_kernels.hip -- the validation metrics of the reference's entry points on the device (gfx950):
//   * the uint8 quantisation in front of both metrics (codes/train.py:301-302: (x * 255.0).round().astype(np.uint8) on the clamped
//     float32 image of utils/util.py:157 tensor2img)
//   * calculate_psnr (utils/util.py:283-290) as an exact 64-bit integer sum of squared differences per plane
//   * ssim / calculate_ssim (utils/util.py:293-334): 11x11 Gaussian window, sigma 1.5, 'valid' region, accumulated in double
//   * crop_border (utils/util.py, called at codes/test_RealVSR_wi_GT.py:139) as an offset into the plane, not a copy
// A plane is H x W float32 with contiguous rows; plane p of an input starts p * plane_stride elements behind its pointer, so channel 0 of
// a [B, 3, H, W] tensor is scored in place.  Only scalars leave a call: one long long (PSNR) or one double (SSIM) per plane.
// No atomics; every sum runs in an order fixed by the shape alone, so results are bit-identical from run to run.  Nothing here may be
// built with fast-math flags: the quantisation is float32 IEEE arithmetic, the SSIM map float64 IEEE arithmetic.
#include "glue_common.h"
#include <math.h>

// q(x) = rint(clamp(x, 0, 1) * 255) in float32, round-half-even: bit for bit numpy's (np.clip(x, 0, 1) * 255.0).round() on a float32
// array.  The clamp is written as two selects so that NaN (for which numpy's cast to uint8 is undefined) maps to 0, like -0.0 and
// every negative number.  The product feeds rintf alone: nothing for the compiler to contract it with, and contraction is off anyway.
__device__ __forceinline__ float quant255(float x) {
#pragma clang fp contract(off)
    x = x > 0.f ? x : 0.f;
    x = x < 1.f ? x : 1.f;
    return rintf(x * 255.0f);
}

// the sum of v over the 256 threads of a workgroup, in every thread, in one fixed order (the tree of train_kernels.hip's block_sum);
// `red` holds 256 values and is free again on return
template <typename T>
__device__ __forceinline__ T block_sum256(T v, T* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const T r = red[0];
    __syncthreads();
    return r;
}

// out[p] = sum of partial[p][0 .. nb) for every plane, one workgroup
template <typename T>
__global__ void metric_finish_kernel(const T* __restrict__ partial, size_t nb, size_t planes, T* __restrict__ out) {
    __shared__ T red[256];
    for (size_t p = 0; p < planes; ++p) {
        T acc = 0;
        for (size_t i = threadIdx.x; i < nb; i += 256) acc += partial[p * nb + i];
        const T s = block_sum256(acc, red);
        if (threadIdx.x == 0) out[p] = s;
    }
}

// ---------------------------------------------------------------- quantisation on its own
__global__ void quantize_u8_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, size_t n) {
    LOOP(i, n) out[i] = (unsigned char)(int)quant255(x[i]);
}

// ---------------------------------------------------------------- PSNR: sum of squared differences of the quantised values
// Work item = 1024 consecutive columns of one row of the cropped plane (four loads per thread in flight); the host flattens an uncropped
// plane into one row of H * W columns.  Workgroup (x, plane) strides over the items and leaves one partial sum.
#define PSNR_BLOCKS 1024
#define PSNR_CHUNK 1024
__global__ void psnr_sse_kernel(const float* __restrict__ a, size_t stride_a, const float* __restrict__ b, size_t stride_b, size_t rows,
                                size_t cols, size_t pitch, size_t origin, size_t nchunks, long long* __restrict__ partial) {
    __shared__ long long red[256];
    const float* pa = a + blockIdx.y * stride_a + origin;
    const float* pb = b + blockIdx.y * stride_b + origin;
    const size_t items = rows * nchunks;
    long long acc = 0;
    for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
        const size_t y = it / nchunks, x0 = (it - y * nchunks) * PSNR_CHUNK + threadIdx.x;
        float va[4], vb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t x = x0 + 256 * k;
            const size_t o = x < cols ? y * pitch + x : 0;   // (element 0 of the cropped plane always exists)
            va[k] = pa[o];
            vb[k] = pb[o];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int d = (int)quant255(va[k]) - (int)quant255(vb[k]);
            acc += x0 + 256 * k < cols ? (long long)(d * d) : 0;
        }
    }
    const long long s = block_sum256(acc, red);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// ---------------------------------------------------------------- SSIM
// One workgroup per METRIC_TH x METRIC_TW tile of the 'valid' map of one plane:
//   1. the (TH + 10) x (TW + 10) patch of both images is loaded once, quantised, and kept in LDS as bytes (every load guarded at the
//      cropped plane's edge: outside it the patch holds 0 and no address is formed);
//   2. horizontal 11-tap pass of the five maps (x, y, x^2, y^2, xy) into LDS as double, [map][patch row][column]: a half-wave reads or
//      writes 32 consecutive doubles = all 64 banks once;
//   3. vertical 11-tap pass from LDS and the per-pixel formula, METRIC_TH / 8 rows per thread, lanes along W;
//   4. one double per tile (positions beyond the map contribute 0), summed per plane by metric_finish_kernel in tile order.
// LDS: 5 * 34 * 32 * 8 + 2 * 34 * 44 + 256 * 8 = 48560 bytes, so three workgroups share a CU's 160 KB.  (Measured on a 2160 x 3840
// plane: tile heights 16 / 24 / 32, i.e. four / three / two workgroups per CU, took 0.175 / 0.166 / 0.185 ms -- the kernel is bound by
// its f64 instruction stream, not by occupancy; a lower tile repeats more of the horizontal pass, 26 / 16 against 34 / 24 rows.)
#define METRIC_TH 24
#define METRIC_TW 32
#define METRIC_PH (METRIC_TH + 10)
#define METRIC_PW (METRIC_TW + 10)
#define METRIC_PITCH 44   // bytes per patch row (42 rounded up to a multiple of 4)

struct MetricWin {
    double w[11];   // cv2.getGaussianKernel(11, 1.5): exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, built by the host in double
};

// util.ssim()'s map value from the five filtered values, operation for operation in IEEE double (no contraction: with identical inputs
// numerator and denominator are then formed from the same values by the same roundings, and the quotient is exactly 1)
__device__ __forceinline__ double ssim_pixel(double mu1, double mu2, double e11, double e22, double e12, double C1, double C2) {
#pragma clang fp contract(off)
    const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
    const double sigma1_sq = e11 - mu1_sq, sigma2_sq = e22 - mu2_sq, sigma12 = e12 - mu1_mu2;
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2));
}

__global__ void __launch_bounds__(256) ssim_tile_kernel(const float* __restrict__ a, size_t stride_a, const float* __restrict__ b,
                                                        size_t stride_b, int Hc, int Wc, size_t pitch, size_t origin, int tiles_x,
                                                        MetricWin win, double C1, double C2, double* __restrict__ partial) {
    __shared__ double hbuf[5][METRIC_PH][METRIC_TW];
    __shared__ unsigned char qa[METRIC_PH][METRIC_PITCH], qb[METRIC_PH][METRIC_PITCH];
    __shared__ double red[256];
    const float* pa = a + blockIdx.y * stride_a + origin;
    const float* pb = b + blockIdx.y * stride_b + origin;
    const int oy = (int)(blockIdx.x / tiles_x) * METRIC_TH, ox = (int)(blockIdx.x % tiles_x) * METRIC_TW;
    const int tid = threadIdx.x;

    for (int idx = tid; idx < METRIC_PH * METRIC_PW; idx += 256) {
        const int r = idx / METRIC_PW, c = idx - r * METRIC_PW;
        const int gy = oy + r, gx = ox + c;
        const bool in = gy < Hc && gx < Wc;
        const size_t o = in ? (size_t)gy * pitch + gx : 0;   // branch-free: the load is always issued, from inside the plane
        const float va = pa[o], vb = pb[o];
        qa[r][c] = in ? (unsigned char)(int)quant255(va) : 0;
        qb[r][c] = in ? (unsigned char)(int)quant255(vb) : 0;
    }
    __syncthreads();

    for (int idx = tid; idx < METRIC_PH * METRIC_TW; idx += 256) {
        const int r = idx / METRIC_TW, c = idx % METRIC_TW;
        double m1 = 0.0, m2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
        for (int j = 0; j < 11; ++j) {
            const double w = win.w[j], x = (double)qa[r][c + j], y = (double)qb[r][c + j];
            m1 = fma(w, x, m1);
            m2 = fma(w, y, m2);
            e11 = fma(w, x * x, e11);   // (products of two bytes: exact)
            e22 = fma(w, y * y, e22);
            e12 = fma(w, x * y, e12);
        }
        hbuf[0][r][c] = m1;
        hbuf[1][r][c] = m2;
        hbuf[2][r][c] = e11;
        hbuf[3][r][c] = e22;
        hbuf[4][r][c] = e12;
    }
    __syncthreads();

    const int Ho = Hc - 10, Wo = Wc - 10;
    const int c = tid % METRIC_TW;
    double acc = 0.0;
    for (int r = tid / METRIC_TW; r < METRIC_TH; r += 256 / METRIC_TW) {
        double m1 = 0.0, m2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
        for (int i = 0; i < 11; ++i) {
            const double w = win.w[i];
            m1 = fma(w, hbuf[0][r + i][c], m1);
            m2 = fma(w, hbuf[1][r + i][c], m2);
            e11 = fma(w, hbuf[2][r + i][c], e11);
            e22 = fma(w, hbuf[3][r + i][c], e22);
            e12 = fma(w, hbuf[4][r + i][c], e12);
        }
        const double v = ssim_pixel(m1, m2, e11, e22, e12, C1, C2);
        acc += (oy + r < Ho && ox + c < Wo) ? v : 0.0;
    }
    const double s = block_sum256(acc, red);
    if (tid == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// ---------------------------------------------------------------- host side
static size_t ssim_tiles(int Hc, int Wc) {
    return (size_t)((Hc - 10 + METRIC_TH - 1) / METRIC_TH) * (size_t)((Wc - 10 + METRIC_TW - 1) / METRIC_TW);
}
// work items of the PSNR kernel for a cropped plane: an uncropped one is a single row of H * W columns
static void psnr_shape(int H, int W, int crop, size_t* rows, size_t* cols, size_t* nchunks, unsigned* nb) {
    *rows = crop == 0 ? 1 : (size_t)(H - 2 * crop);
    *cols = crop == 0 ? (size_t)H * W : (size_t)(W - 2 * crop);
    *nchunks = (*cols + PSNR_CHUNK - 1) / PSNR_CHUNK;
    const size_t items = *rows * *nchunks;
    *nb = (unsigned)(items < PSNR_BLOCKS ? items : PSNR_BLOCKS);
}
static int metric_args(const char* what, const void* a, const void* b, const void* out, const void* workspace, size_t planes, int H,
                       int W, int crop) {
    if (!a || !b || !out || !workspace) FAIL(RVSR_ERR_BAD_ARG, "%s: null argument", what);
    if (planes == 0 || planes > 65535) FAIL(RVSR_ERR_BAD_ARG, "%s: %zu planes (1 .. 65535)", what, planes);
    if (H <= 0 || W <= 0 || crop < 0 || H <= 2 * (long long)crop || W <= 2 * (long long)crop)
        FAIL(RVSR_ERR_BAD_ARG, "%s: a %d x %d plane with crop_border %d is empty", what, H, W, crop);
    return RVSR_OK;
}

extern "C" int rvsr_metric_tile(int* th, int* tw) {
    if (th) *th = METRIC_TH;
    if (tw) *tw = METRIC_TW;
    return RVSR_OK;
}

extern "C" size_t rvsr_metric_workspace_bytes(size_t planes, int H, int W, int crop) {
    if (planes == 0 || H <= 0 || W <= 0 || crop < 0 || H <= 2 * (long long)crop || W <= 2 * (long long)crop) return 0;
    const int Hc = H - 2 * crop, Wc = W - 2 * crop;
    size_t per_plane = PSNR_BLOCKS;
    if (Hc >= 11 && Wc >= 11 && ssim_tiles(Hc, Wc) > per_plane) per_plane = ssim_tiles(Hc, Wc);
    return planes * per_plane * 8;
}

extern "C" int rvsr_quantize_u8(const float* x, unsigned char* out, size_t n, void* stream) {
    if (!x || !out) FAIL(RVSR_ERR_BAD_ARG, "quantize_u8: null argument");
    if (n == 0) return RVSR_OK;
    hipLaunchKernelGGL(quantize_u8_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, x, out, n);
    RETURN_LAUNCH("quantize_u8");
}

extern "C" int rvsr_psnr_sse(const float* a, size_t a_plane_stride, const float* b, size_t b_plane_stride, size_t planes, int H, int W,
                             int crop, long long* sse, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = metric_args("psnr_sse", a, b, sse, workspace, planes, H, W, crop);
    if (rc != RVSR_OK) return rc;
    size_t rows, cols, nchunks;
    unsigned nb;
    psnr_shape(H, W, crop, &rows, &cols, &nchunks, &nb);
    if (workspace_bytes < planes * nb * sizeof(long long))
        FAIL(RVSR_ERR_WORKSPACE, "psnr_sse: workspace of %zu bytes, %zu needed", workspace_bytes, planes * nb * sizeof(long long));
    const size_t origin = (size_t)crop * W + crop;
    hipLaunchKernelGGL(psnr_sse_kernel, dim3(nb, (unsigned)planes), dim3(256), 0, (hipStream_t)stream, a, a_plane_stride, b,
                       b_plane_stride, rows, cols, (size_t)W, origin, nchunks, (long long*)workspace);
    CHECK_LAUNCH("psnr_sse");
    hipLaunchKernelGGL(metric_finish_kernel<long long>, dim3(1), dim3(256), 0, (hipStream_t)stream, (const long long*)workspace,
                       (size_t)nb, planes, sse);
    RETURN_LAUNCH("psnr_sse finish");
}

extern "C" int rvsr_ssim_sum(const float* a, size_t a_plane_stride, const float* b, size_t b_plane_stride, size_t planes, int H, int W,
                             int crop, double* sum, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = metric_args("ssim_sum", a, b, sum, workspace, planes, H, W, crop);
    if (rc != RVSR_OK) return rc;
    const int Hc = H - 2 * crop, Wc = W - 2 * crop;
    if (Hc < 11 || Wc < 11)
        FAIL(RVSR_ERR_BAD_ARG, "ssim_sum: the cropped plane %d x %d is smaller than the 11 x 11 window", Hc, Wc);
    const size_t tiles = ssim_tiles(Hc, Wc);
    if (tiles > 0x7fffffffu) FAIL(RVSR_ERR_BAD_ARG, "ssim_sum: %zu tiles per plane", tiles);
    if (workspace_bytes < planes * tiles * sizeof(double))
        FAIL(RVSR_ERR_WORKSPACE, "ssim_sum: workspace of %zu bytes, %zu needed", workspace_bytes, planes * tiles * sizeof(double));
    MetricWin win;
    double total = 0.0;
    for (int i = 0; i < 11; ++i) {
        win.w[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        total += win.w[i];
    }
    for (int i = 0; i < 11; ++i) win.w[i] /= total;
    const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
    const size_t origin = (size_t)crop * W + crop;
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)tiles, (unsigned)planes), dim3(256), 0, (hipStream_t)stream, a, a_plane_stride, b,
                       b_plane_stride, Hc, Wc, (size_t)W, origin, (int)((Wc - 10 + METRIC_TW - 1) / METRIC_TW), win, C1, C2,
                       (double*)workspace);
    CHECK_LAUNCH("ssim_sum");
    hipLaunchKernelGGL(metric_finish_kernel<double>, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, tiles, planes,
                       sum);
    RETURN_LAUNCH("ssim_sum finish");
}
