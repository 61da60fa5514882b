// gan_kernels.hip -- the non-convolution operators of the GAN discriminator and its criterion
// (codes/models/archs/discriminator_arch.py:46-92 PatchDiscriminator, codes/models/loss.py:102-133 GANLoss):
//   * nn.BatchNorm2d (train and eval) fused with the LeakyReLU(0.2) that follows every BN of the patch discriminator,
//   * BCEWithLogitsLoss against a constant label, optionally relativistic (a - mean(b), RaGAN).
//
// Reductions follow the project's convention: double accumulators, a fixed split of the work over workgroups, a fixed
// LDS tree inside a workgroup and a fixed-order sum over the partials -> bit-identical results from run to run.
#include "glue_common.h"

// ---------------------------------------------------------------- BatchNorm2d + LeakyReLU
// Per channel the B*HW elements are cut into NP equal slices (NP from the size alone); workgroup (q, c) reduces slice q of
// channel c into part[c][q][0..1].
static int bn_parts(long n) {
    long np = (n + 8191) / 8192;
    if (np > 64) np = 64;
    if (np < 1) np = 1;
    return (int)np;
}

__device__ __forceinline__ void block_sum2(double& s1, double& s2, double (*red)[256]) {
    const int t = threadIdx.x;
    red[0][t] = s1;
    red[1][t] = s2;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
            red[0][t] += red[0][t + w];
            red[1][t] += red[1][t + w];
        }
        __syncthreads();
    }
    s1 = red[0][0];
    s2 = red[1][0];
}

// MODE 0: (sum x, sum x^2).  MODE 1: (sum gz, sum gz * xhat), gz = gy * lrelu'(y).
template <int MODE>
__global__ __launch_bounds__(256) void bn_partial_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                         const float* __restrict__ y, const float* __restrict__ mean,
                                                         const float* __restrict__ invstd, int C, int HW, long n, int NP,
                                                         float slope, double* __restrict__ part) {
    __shared__ double red[2][256];
    const int q = blockIdx.x, c = blockIdx.y;
    const long beg = n * q / NP, end = n * (q + 1) / NP;
    double s1 = 0.0, s2 = 0.0;
    const float m = MODE ? mean[c] : 0.f, is = MODE ? invstd[c] : 0.f;
    for (long i = beg + threadIdx.x; i < end; i += 256) {
        const long b = i / HW, s = i - b * HW;
        const size_t idx = ((size_t)b * C + c) * HW + s;
        const float v = x[idx];
        if (MODE == 0) {
            s1 += (double)v;
            s2 += (double)v * (double)v;
        } else {
            const float g = gy[idx] * (y[idx] > 0.f ? 1.f : slope);
            const float xh = (v - m) * is;
            s1 += (double)g;
            s2 += (double)g * (double)xh;
        }
    }
    block_sum2(s1, s2, red);
    if (threadIdx.x == 0) {
        part[((size_t)c * NP + q) * 2 + 0] = s1;
        part[((size_t)c * NP + q) * 2 + 1] = s2;
    }
}

// one thread per channel: statistics, running-statistics update, the per-channel affine of the apply pass (coef[c] = scale,
// coef[C + c] = shift)
__global__ void bn_stats_kernel(const double* __restrict__ part, int NP, int C, long n, int train, const float* __restrict__ gamma,
                                const float* __restrict__ beta, float* running_mean, float* running_var, long long* nbt,
                                float momentum, float eps, float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                float* __restrict__ coef) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && train && nbt != nullptr) nbt[0] += 1;
    if (c >= C) return;
    float mean, invstd;
    if (train) {
        double s1 = 0.0, s2 = 0.0;
        for (int q = 0; q < NP; ++q) {
            s1 += part[((size_t)c * NP + q) * 2 + 0];
            s2 += part[((size_t)c * NP + q) * 2 + 1];
        }
        const double md = s1 / (double)n;
        double var = s2 / (double)n - md * md;
        if (var < 0.0) var = 0.0;
        mean = (float)md;
        invstd = (float)(1.0 / sqrt(var + (double)eps));
        if (running_mean != nullptr) {
            running_mean[c] = momentum * (float)md + (1.f - momentum) * running_mean[c];
            running_var[c] = momentum * (float)(var * (double)n / (double)(n - 1)) + (1.f - momentum) * running_var[c];
        }
    } else {
        mean = running_mean[c];
        invstd = (float)(1.0 / sqrt((double)running_var[c] + (double)eps));
    }
    save_mean[c] = mean;
    save_invstd[c] = invstd;
    const float sc = invstd * (gamma ? gamma[c] : 1.f);
    coef[c] = sc;
    coef[C + c] = (beta ? beta[c] : 0.f) - mean * sc;
}

__global__ void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ coef, float* __restrict__ y, int C, int HW,
                                size_t total, float slope) {
    LOOP(i, total) {
        const int c = (int)((i / HW) % C);
        const float v = x[i] * coef[c] + coef[C + c];
        y[i] = v > 0.f ? v : v * slope;
    }
}

// one thread per channel: gamma / beta gradients and the coefficients of gx = k1 * (gz - k2 - xhat * k3)
__global__ void bn_bwd_stats_kernel(const double* __restrict__ part, int NP, int C, long n, int train, const float* __restrict__ gamma,
                                    const float* __restrict__ invstd, float* __restrict__ ggamma, float* __restrict__ gbeta,
                                    float* __restrict__ coef) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int q = 0; q < NP; ++q) {
        s1 += part[((size_t)c * NP + q) * 2 + 0];
        s2 += part[((size_t)c * NP + q) * 2 + 1];
    }
    if (gbeta) gbeta[c] = (float)s1;
    if (ggamma) ggamma[c] = (float)s2;
    coef[c] = (gamma ? gamma[c] : 1.f) * invstd[c];
    coef[C + c] = train ? (float)(s1 / (double)n) : 0.f;
    coef[2 * C + c] = train ? (float)(s2 / (double)n) : 0.f;
}

__global__ void bn_bwd_apply_kernel(const float* __restrict__ gy, const float* __restrict__ y, const float* __restrict__ x,
                                    const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ coef,
                                    float* __restrict__ gx, int C, int HW, size_t total, float slope) {
    LOOP(i, total) {
        const int c = (int)((i / HW) % C);
        const float g = gy[i] * (y[i] > 0.f ? 1.f : slope);
        const float xh = (x[i] - mean[c]) * invstd[c];
        gx[i] = coef[c] * (g - coef[C + c] - xh * coef[2 * C + c]);
    }
}

static size_t bn_part_bytes(int B, int C, int HW) { return (size_t)C * bn_parts((long)B * HW) * 2 * sizeof(double); }
extern "C" size_t rvsr_bn_workspace_bytes(int B, int C, int HW) {
    return bn_part_bytes(B, C, HW) + (size_t)3 * C * sizeof(float) + 16;
}

static int bn_check(int B, int C, int HW, void* ws, size_t wsb) {
    if (B <= 0 || C <= 0 || HW <= 0) FAIL(RVSR_ERR_BAD_ARG, "bn_lrelu: empty shape (%d, %d, %d)", B, C, HW);
    if (!ws || wsb < rvsr_bn_workspace_bytes(B, C, HW))
        FAIL(RVSR_ERR_WORKSPACE, "bn_lrelu: workspace %zu B < %zu B", wsb, rvsr_bn_workspace_bytes(B, C, HW));
    return RVSR_OK;
}

extern "C" int rvsr_bn_lrelu_forward(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                     long long* num_batches_tracked, float* y, float* save_mean, float* save_invstd, int B, int C,
                                     int HW, int train, float momentum, float eps, float slope, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    if (!x || !y || !save_mean || !save_invstd) FAIL(RVSR_ERR_BAD_ARG, "bn_lrelu: null argument");
    if ((running_mean == nullptr) != (running_var == nullptr)) FAIL(RVSR_ERR_BAD_ARG, "bn_lrelu: running_mean / running_var disagree");
    if (!train && !running_mean) FAIL(RVSR_ERR_BAD_ARG, "bn_lrelu: eval mode needs the running statistics");
    const long n = (long)B * HW;
    if (train && n < 2) FAIL(RVSR_ERR_BAD_ARG, "bn_lrelu: train mode needs more than one value per channel");
    if (int rc = bn_check(B, C, HW, workspace, workspace_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int NP = bn_parts(n);
    double* part = (double*)workspace;
    float* coef = (float*)((char*)workspace + bn_part_bytes(B, C, HW));
    if (train)
        hipLaunchKernelGGL(bn_partial_kernel<0>, dim3(NP, C), dim3(256), 0, st, x, nullptr, nullptr, nullptr, nullptr, C, HW, n, NP, 0.f,
                           part);
    hipLaunchKernelGGL(bn_stats_kernel, dim3((C + 63) / 64), dim3(64), 0, st, part, NP, C, n, train, gamma, beta, running_mean,
                       running_var, num_batches_tracked, momentum, eps, save_mean, save_invstd, coef);
    const size_t total = (size_t)n * C;
    hipLaunchKernelGGL(bn_apply_kernel, GRID_FOR(total), dim3(256), 0, st, x, coef, y, C, HW, total, slope);
    RETURN_LAUNCH("bn_lrelu_forward");
}

extern "C" int rvsr_bn_lrelu_backward(const float* gy, const float* y, const float* x, const float* gamma, const float* save_mean,
                                      const float* save_invstd, float* gx, float* ggamma, float* gbeta, int B, int C, int HW, int train,
                                      float slope, void* workspace, size_t workspace_bytes, void* stream) {
    if (!gy || !y || !x || !save_mean || !save_invstd) FAIL(RVSR_ERR_BAD_ARG, "bn_lrelu backward: null argument");
    if (int rc = bn_check(B, C, HW, workspace, workspace_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long n = (long)B * HW;
    const int NP = bn_parts(n);
    double* part = (double*)workspace;
    float* coef = (float*)((char*)workspace + bn_part_bytes(B, C, HW));
    if (!(train || ggamma || gbeta) && !gx) return RVSR_OK;
    hipLaunchKernelGGL(bn_partial_kernel<1>, dim3(NP, C), dim3(256), 0, st, x, gy, y, save_mean, save_invstd, C, HW, n, NP, slope,
                       part);
    hipLaunchKernelGGL(bn_bwd_stats_kernel, dim3((C + 63) / 64), dim3(64), 0, st, part, NP, C, n, train, gamma, save_invstd, ggamma,
                       gbeta, coef);
    if (gx) {
        const size_t total = (size_t)n * C;
        hipLaunchKernelGGL(bn_bwd_apply_kernel, GRID_FOR(total), dim3(256), 0, st, gy, y, x, save_mean, save_invstd, coef, gx, C, HW,
                           total, slope);
    }
    RETURN_LAUNCH("bn_lrelu_backward");
}

// ---------------------------------------------------------------- BCE-with-logits GAN criterion
__device__ __forceinline__ float sigmoid_stable(float z) {
    if (z >= 0.f) return 1.f / (1.f + expf(-z));
    const float e = expf(z);
    return e / (1.f + e);
}

__device__ __forceinline__ double block_sum1024(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int w = 512; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// one workgroup of 1024 threads: the discriminator maps are small (B x 1 x H/4 x W/4)
__global__ __launch_bounds__(1024) void gan_loss_fwd_kernel(const float* __restrict__ a, size_t na, const float* __restrict__ b,
                                                            size_t nb, float t, double scale, float* __restrict__ out,
                                                            float* __restrict__ saved) {
    __shared__ double red[1024];
    float shift = 0.f;
    if (b != nullptr) {
        double s = 0.0;
        for (size_t i = threadIdx.x; i < nb; i += 1024) s += (double)b[i];
        shift = (float)(block_sum1024(s, red) / (double)nb);
    }
    double sl = 0.0, sd = 0.0;
    for (size_t i = threadIdx.x; i < na; i += 1024) {
        const float z = a[i] - shift;
        sl += (double)(fmaxf(z, 0.f) - z * t + log1pf(expf(-fabsf(z))));
        sd += (double)(sigmoid_stable(z) - t);
    }
    sl = block_sum1024(sl, red);
    sd = block_sum1024(sd, red);
    if (threadIdx.x == 0) {
        out[0] = (float)(sl * scale);
        saved[0] = shift;
        saved[1] = (float)sd;
    }
}

__global__ void gan_loss_bwd_kernel(const float* __restrict__ a, size_t na, size_t nb, const float* __restrict__ saved,
                                    const float* __restrict__ gscalar, float t, float scale, float* __restrict__ ga,
                                    float* __restrict__ gb) {
    const float g = gscalar[0] * scale, shift = saved[0];
    if (ga != nullptr) {
        LOOP(i, na) ga[i] = g * (sigmoid_stable(a[i] - shift) - t);
    }
    if (gb != nullptr) {
        const float v = -g * saved[1] / (float)nb;
        LOOP(j, nb) gb[j] = v;
    }
}

extern "C" int rvsr_gan_loss_forward(const float* a, size_t na, const float* b, size_t nb, float target, double scale, float* out,
                                     float* saved, void* stream) {
    if (!a || !out || !saved || na == 0) FAIL(RVSR_ERR_BAD_ARG, "gan_loss: null / empty argument");
    if (b != nullptr && nb == 0) FAIL(RVSR_ERR_BAD_ARG, "gan_loss: empty relativistic operand");
    hipLaunchKernelGGL(gan_loss_fwd_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a, na, b, nb, target, scale, out, saved);
    RETURN_LAUNCH("gan_loss_forward");
}

extern "C" int rvsr_gan_loss_backward(const float* a, size_t na, size_t nb, const float* saved, const float* gscalar, float target,
                                      float scale, float* ga, float* gb, void* stream) {
    if (!a || !saved || !gscalar || na == 0) FAIL(RVSR_ERR_BAD_ARG, "gan_loss backward: null / empty argument");
    if (gb != nullptr && nb == 0) FAIL(RVSR_ERR_BAD_ARG, "gan_loss backward: gradient of an empty relativistic operand");
    const size_t n = na > nb ? na : nb;
    hipLaunchKernelGGL(gan_loss_bwd_kernel, GRID_FOR(n), dim3(256), 0, (hipStream_t)stream, a, na, nb, saved, gscalar, target, scale, ga,
                       gb);
    RETURN_LAUNCH("gan_loss_backward");
}
