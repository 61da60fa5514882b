/*
 * realvsr_hip.h -- C ABI of librealvsr_hip.so: the MI355X (gfx950) implementation of RealVSR's
 * EDVR alignment / fusion / reconstruction / pyramid-loss hot path.
 *
 * Conventions (all entry points):
 *   - plain device pointers (float32, NCHW, contiguous unless a batch stride is stated) + sizes;
 *     no torch / ATen types.  The caller owns every buffer; the library allocates nothing
 *     (temporaries come in through `workspace`) and keeps no state between calls EXCEPT one
 *     setting, the GEMM arithmetic: a process-wide default (rvsr_set_gemm_mode below; set it once
 *     before the first call) and a per-host-thread override (rvsr_set_gemm_mode_thread), both read
 *     by every conv / DCN entry point at call time on the calling thread -- so the reference's
 *     nn.DataParallel threads (VideoSR_AllPair_model_YCbCr_Split.py:35-36), which all CALL
 *     concurrently, each on its own device / stream, can each choose without racing
 *     (tests/test_gpu_misc.py::test_two_host_threads_two_streams, ::test_gemm_mode_per_thread).  The host
 *     mirror realvsr_amd.functional keeps two per-process caches on top (bf16 weight images keyed
 *     on the parameter object, per-layer DCN offset statistics); both are keyed per parameter
 *     object + device, so DataParallel replicas (distinct parameter objects) get their own entries.
 *   - `stream` is a hipStream_t (NULL = default stream).  Launches are asynchronous; the call is
 *     re-entrant across devices/streams (the caller sets the current device, as
 *     at::DeviceGuard does in the reference: deform_conv_cuda.cpp:499,581).
 *   - return value: 0 = ok, RVSR_ERR_* otherwise; rvsr_last_error() gives the message for the
 *     calling thread.  (The reference only printf()s launch errors, kernel.cu:794-798; shape
 *     errors there are c10::Error -> RuntimeError, deform_conv_cuda.cpp:497-516.)
 *
 * Section 1 is the drop-in for the reference's pybind module `deform_conv_cuda`
 * (codes/models/archs/dcn/src/deform_conv_cuda.cpp:687-701).  Sections 2-4 replace the ATen /
 * cuDNN calls the reference's Python makes on the same path (nn.Conv2d, F.interpolate, pooling,
 * pixel_shuffle, the TSA element-wise chain, utils/util.py pyramids, Charbonnier loss).
 */
#ifndef REALVSR_HIP_H
#define REALVSR_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define RVSR_OK 0
#define RVSR_ERR_UNSUPPORTED 1 /* valid request, not implemented on the HIP path (e.g. 5x5 DCN) */
#define RVSR_ERR_BAD_ARG 2     /* null pointer / inconsistent shapes                              */
#define RVSR_ERR_LAUNCH 3      /* HIP launch error                                                */
#define RVSR_ERR_WORKSPACE 4   /* workspace missing or too small                                  */

/* In front of a parameter: a pointer into HOST memory that the call writes through.  Every unmarked pointer is device memory, or a
 * buffer whose comment says where it lives.  (realvsr_amd/_lib.py reads its ctypes signatures from this file: a marked int* / long long*
 * is a typed POINTER there, every other pointer a void*.) */
#define RVSR_HOST

const char* rvsr_last_error(void);

/* GEMM arithmetic of the conv blocks: 0 (default) = 3-term bf16 split on the bf16 matrix cores
 * (a = a_hi + a_lo; a_hi*b_hi + a_hi*b_lo + a_lo*b_hi accumulated in f32; ~2^-17 relative error
 * per product), 1 = exact f32 MFMA (an fmaf chain; ~5x slower GEMMs).  Opt-in speed modes:
 * 2 = two terms (the weights -- in a weight gradient: the output gradient -- rounded to bf16, the
 * other operand hi + lo: exactly the result of mode 0 on bf16-rounded weights), 3 = one term (both
 * operands rounded to bf16); accumulation stays f32, ~2^-9 per product.  Modes 2 / 3 act in the
 * kernels that dominate a training step and ONLY there:
 *   conv_fwd5   3x3 stride-1 forward and data gradient, where the plan (below) says 64-row m-blocks on a
 *               vector-staged input view: rvsr_conv2d_forward_plan reports the term count of a call;
 *   conv_wgrad2 / conv_wgrad5   the 3x3 stride-1 and the 5x5 weight gradient on the matrix cores;
 *   dcn_fwd3    fused DCN forward with C_out > 32;
 *   dcn_bwdin6               fused DCN input / offset / mask gradient with C_out > 32;
 *   dcn_bwdw4 / dcn_bwdw6    fused DCN weight gradient
 *   (which DCN calls these kernels take: dcn_fwd_plan / dcn_bwd_plan, csrc/dcn_plan.h; rvsr_dcn_pack_*_plan report the term count of a call).
 * Every other kernel (1x1 and strided forward convs and their weight gradients, narrow m-blocks such as the 3-channel output conv,
 * scalar-staged views, the generic DCN path of section 1c) computes three terms in modes 2 / 3, so a network off those shapes gets
 * mode 0's result and speed.  A gradient is a call of its own and its own plan decides: the data gradient of a stride-2 conv or of a
 * conv with few output channels is a stride-1 conv_fwd5 call with the conv's INPUT channels as rows (64-row m-blocks from 33 input
 * channels on: reduced), and conv_wgrad2 takes the weight gradient of every 3x3 stride-1 conv with more than 4 output channels (16-byte aligned, W % 4 == 0).
 * The definition holds bit for bit for every output but the DCN's grad_input, an atomic scatter: there mode 2 / 3 differs from mode 0 on
 * the rounded operands by the summation order alone, as two runs of mode 0 do (the fixed-point scale of dcn_bwdin6's window is taken
 * from the rounded operands in these modes).  The DCN weight-gradient kernels form grad_bias as a product with a ones column, so it
 * follows the rounded output gradient; the conv weight-gradient kernels sum the f32 output gradient and give mode 0's grad_bias.
 * tests/test_gpu_modes_definition.py pins all of this per kernel.  Other values select 0.  Process-wide switch. */
void rvsr_set_gemm_mode(int mode);
int rvsr_get_gemm_mode(void);   /* the mode the CALLING thread's next call computes in */
/* The same choice for the calling host thread only (every entry point reads the mode at call time on the calling thread): mode 0-3
 * overrides the process-wide setting for this thread's calls, any other value (-1) returns the thread to the process-wide setting.
 * This is the race-free way to select the arithmetic per call -- set it, call, set it back -- when several host threads drive the
 * library at once (the reference's nn.DataParallel replicas); rvsr_set_gemm_mode stays the default for threads that never ask. */
void rvsr_set_gemm_mode_thread(int mode);

/* ---------------------------------------------------------------------------------------------
 * 1. Modulated deformable convolution (DCNv2)
 * --------------------------------------------------------------------------------------------- */

/* Replaces modulated_deform_conv_cuda_forward (deform_conv_cuda.cpp:490-569) +
 * modulated_deformable_im2col_cuda (deform_conv_cuda_kernel.cu:571-633, 769-799).
 *   input (B,C,H,W)  weight (Co,C,kh,kw)  bias (Co) or NULL  offset (B,2*dg*kh*kw,Ho,Wo)
 *   mask (B,dg*kh*kw,Ho,Wo)  output (B,Co,Ho,Wo) -- fully overwritten.
 * The reference's `ones` / `columns` temporaries do not exist here (the column tile lives in LDS).
 * HIP path: kh = kw = 3, group = 1, isotropic stride/pad/dilation, C/dg dividing or a multiple of 8.
 * workspace: rvsr_modulated_deform_conv_forward_workspace_bytes(channels, channels_out) bytes for
 * the bf16 hi/lo re-packed weights of the bf16x3 kernels; NULL selects the exact-f32 kernel.
 * Which kernels a DCN call runs -- forward: dcn_fwd3 (stride 1, dilation 1; tile halo 3 / 7 / 11 px, selected on the device among up to
 * three launches, or fixed by the caller's hint), dcn_fwd2 (other strides / dilations, frames beyond 4 GB per batch element) or the
 * exact-f32 dcn_fwd_kernel (GEMM mode 1, no workspace, fewer than 8 channels per deformable group); backward: dcn_bwdin6 + dcn_bwdw6 as
 * a pair, dcn_bwdw4 / dcn_bwdw2 for a weight gradient alone or a view the pair does not take, the first-generation kernels for the
 * rest -- with their tiles, term counts, candidates, grids, whether the probe pass and the weight pack run, and the layout of the
 * backward's workspace, is decided by dcn_fwd_plan / dcn_bwd_plan / dcn_bwd_workspace (csrc/dcn_plan.h), which state every rule once.
 * Entries validate, plan, refuse or launch in order; a refused call (RVSR_ERR_WORKSPACE included) launches nothing, the probe pass
 * included.  All kernels of a direction compute the same function. */
size_t rvsr_modulated_deform_conv_forward_workspace_bytes(int channels, int channels_out);
int rvsr_modulated_deform_conv_forward(const float* input, const float* weight, const float* bias,
                                       const float* offset, const float* mask, float* output,
                                       int batch, int channels, int height, int width, int channels_out,
                                       int kernel_h, int kernel_w, int stride_h, int stride_w,
                                       int pad_h, int pad_w, int dilation_h, int dilation_w,
                                       int group, int deformable_group, int with_bias,
                                       void* workspace, size_t workspace_bytes, void* stream);

/* Replaces modulated_deform_conv_cuda_backward (deform_conv_cuda.cpp:571-685) + the col2im /
 * col2im_coord / im2col kernels (deform_conv_cuda_kernel.cu:571-767).
 *   grad_input (B,C,H,W): must be zero on entry (scatter-add, as the reference: deform_conv.py:127)
 *   grad_offset, grad_mask: overwritten.   grad_weight, grad_bias: accumulated into (+=), the
 *   caller zeroes them (deform_conv.py:130-131, cpp:659-671).
 *   grad_input/grad_offset/grad_mask may be NULL together (skip), grad_weight may be NULL (skip).
 *   workspace: rvsr_modulated_deform_conv_backward_workspace_bytes() bytes, needed iff grad_weight.
 *   SIZE: for stride 1 / dilation 1 / channels % 8 == 0 / channels_out <= 128 (what EDVR and TDAN instantiate) the workspace also holds the
 *   hand-off between the input-gradient and the weight-gradient kernel -- a bf16 hi + lo copy of grad_output in matrix-core operand order,
 *   batch x ceil8(Ho) x ceil32(Wo) x ceil64(channels_out) x 4 bytes (~575 MiB at 40 x 64 x 180 x 320) -- on top of the weight image and the
 *   weight-gradient partials (tens of MB).  Other geometries: partials only.
 *   The kernel for grad_input/grad_offset/grad_mask is chosen ON THE DEVICE from a sampled statistic of `offset` (no host
 *   synchronisation): one shared fixed-point LDS window per 8-channel chunk with a halo of 2 / 4 / 5 / 8 / 12 px; samples beyond the halo
 *   go through global gathers / atomics with the reference's rule set; all candidates give the same result up to the summation order of
 *   the scatter.  grad_weight / grad_bias / grad_offset / grad_mask are bit-reproducible run to run, grad_input is not (atomics, as the
 *   reference's col2im, kernel.cu:688). */
size_t rvsr_modulated_deform_conv_backward_workspace_bytes(int batch, int channels, int height, int width,
                                                           int channels_out, int stride, int pad, int dil);
int rvsr_modulated_deform_conv_backward(const float* input, const float* weight, const float* bias,
                                        const float* offset, const float* mask, float* grad_input,
                                        float* grad_weight, float* grad_bias, float* grad_offset,
                                        float* grad_mask, const float* grad_output,
                                        int batch, int channels, int height, int width, int channels_out,
                                        int kernel_h, int kernel_w, int stride_h, int stride_w,
                                        int pad_h, int pad_w, int dilation_h, int dilation_w,
                                        int group, int deformable_group, int with_bias,
                                        void* workspace, size_t workspace_bytes, void* stream);

/* 1b. DCNv1 -- the other three functions of the reference's pybind module (deform_conv_cuda.cpp:152-260 deform_conv_forward_cuda,
 * :262-374 deform_conv_backward_input_cuda, :376-488 deform_conv_backward_parameters_cuda; registration :687-701), same argument order
 * (kW, kH, dW, dH, padW, padH, dilationW, dilationH, group, deformable_group[, scale], im2col_step) with the tensors as plain pointers:
 *   input (B,C,H,W), offset (B, 2*dg*kH*kW, Ho, Wo), weight (Co, C, kH, kW), output / grad_output (B,Co,Ho,Wo); no bias, no mask.
 * The reference's `columns` / `ones` temporaries do not exist here (no column matrix); `im2col_step` has to divide the batch
 * (deform_conv.py:41) and is otherwise unused.  Same geometry limits as section 1 (3x3, group 1, isotropic stride / pad / dilation).
 * backward_input accumulates into the caller-zeroed grad_input and writes grad_offset; backward_parameters accumulates scale * gradient
 * into the caller-zeroed grad_weight (scale must be 1, what deform_conv.py:76 passes).
 * workspace: rvsr_deform_conv_workspace_bytes(...) bytes for all three. */
size_t rvsr_deform_conv_workspace_bytes(int batch, int channels, int height, int width, int channels_out, int kW, int kH, int dW,
                                        int padW, int dilationW, int deformable_group);
int rvsr_deform_conv_forward(const float* input, const float* weight, const float* offset, float* output, int batch, int channels,
                             int height, int width, int channels_out, int kW, int kH, int dW, int dH, int padW, int padH,
                             int dilationW, int dilationH, int group, int deformable_group, int im2col_step, void* workspace,
                             size_t workspace_bytes, void* stream);
int rvsr_deform_conv_backward_input(const float* input, const float* offset, const float* grad_output, float* grad_input,
                                    float* grad_offset, const float* weight, int batch, int channels, int height, int width,
                                    int channels_out, int kW, int kH, int dW, int dH, int padW, int padH, int dilationW,
                                    int dilationH, int group, int deformable_group, int im2col_step, void* workspace,
                                    size_t workspace_bytes, void* stream);
int rvsr_deform_conv_backward_parameters(const float* input, const float* offset, const float* grad_output, float* grad_weight,
                                         int batch, int channels, int height, int width, int channels_out, int kW, int kH, int dW,
                                         int dH, int padW, int padH, int dilationW, int dilationH, int group, int deformable_group,
                                         float scale, int im2col_step, void* workspace, size_t workspace_bytes, void* stream);

/* Fused core of ModulatedDeformConvPack.forward (deform_conv.py:274-292): `om` is the raw
 * (B,3*dg*9,Ho,Wo) output of conv_offset_mask; torch.chunk/torch.cat become addressing (channels
 * [0,2*dg*9) are the offsets, the rest mask logits) and torch.sigmoid runs in-kernel.
 * act: 0 none, 1 ReLU, 2 LeakyReLU(slope) applied to the output (EDVR_arch.py:107,130); act | 0x100: `workspace`
 * already holds this layer's packed weight image (rvsr_dcn_pack_weights / rvsr_pack_weights_batched), skip the per-call pack.
 * probe (NULL or 8 zeroed uint32 on the device): receives the sampled offset statistic (components beyond 2.5 .. 11.5 px) from
 * which the forward picks the halo of its LDS tile on the device (3 / 7 / 11 px, no host round trip); hand the same buffer to
 * rvsr_dcn_pack_backward, which then skips its own probe pass.  NULL: the halo in act bits 10..13 (3 / 7 / 11, chosen by the caller
 * from an earlier statistic, rvsr_dcn_offset_probe), else 3 px; out-of-tile samples gather from global memory in every case. */
int rvsr_dcn_offset_probe(const float* om, int batch, int height_out, int width_out, int deformable_group, void* probe, void* stream);
size_t rvsr_dcn_pack_weights(const float* weight, int channels, int channels_out, void* out, size_t out_bytes,
                             RVSR_HOST long long* desc, void* stream);
int rvsr_dcn_pack_forward(const float* input, const float* weight, const float* bias, const float* om,
                          float* output, int batch, int channels, int height, int width, int channels_out,
                          int stride, int pad, int dilation, int deformable_group, int act, float slope,
                          void* probe, void* workspace, size_t workspace_bytes, void* stream);
/* act_out (NULL or the saved activation output) fuses the activation derivative into the
 * grad_output load.  grad_om (B,3*dg*9,Ho,Wo) is overwritten (d/d logit for the mask part);
 * grad_input zero on entry; grad_weight/grad_bias accumulated.
 * probe: NULL, or the counters rvsr_dcn_pack_forward filled for the same `om`. */
int rvsr_dcn_pack_backward(const float* input, const float* weight, const float* om, const float* grad_output,
                           const float* act_out, float act_slope, float* grad_input, float* grad_weight,
                           float* grad_bias, float* grad_om, int batch, int channels, int height, int width,
                           int channels_out, int stride, int pad, int dilation, int deformable_group,
                           const void* probe, void* workspace, size_t workspace_bytes, void* stream);
/* The plans of these two calls, without running them (no GPU needed, nothing launched, no pointer dereferenced): the arguments of the
 * call without the stream; return what the call itself would return before launching (rvsr_last_error set alike) and fill
 *   forward  plan[36] = {family (0 dcn_fwd3, 1 dcn_fwd2<8, MT>, 2 dcn_fwd_kernel<MT, CHS>; -1 refused), MT, CHS, terms of a product,
 *            weight pack runs, probe pass runs, its samples, launches (1-3), 3 x {halo, ge, lt, ge2, thr_ge, thr_lt, thr_ge2, LDS bytes}
 *            (the DcnHaloSel of each launch: counter indices, -1 = condition absent; unused slots 0), grid x, y, z, LDS bytes};
 *   backward plan[41] = {input-gradient family (0 none, 1 dcn_bwdin6<NK>, 2 dcn_bwd_input_kernel<CHS>; -1 refused), NK, terms, CHS,
 *            LDS bytes of dcn_bwd_input_kernel, dcn_bwdin6 runs its own probe pass, launches (1-5), 5 x {window, ge, lt, threshold},
 *            hand-off written, its byte offset in the workspace, weight-gradient family (0 none, 1 dcn_bwdw6<R, TH>, 2 dcn_bwdw4<NT>,
 *            3 dcn_bwdw2_kernel, 4 dcn_bwd_weight_kernel<0>), R, TH, terms, ns, nmb, xcd, P, Q (partials), gy, gz, LDS bytes}.
 * The developer switches (RVSR_DCN_BWD, RVSR_DCN5_HALO, RVSR_DCN3_HALO, RVSR_BWDW6_WG; read once per process) enter as in the call. */
int rvsr_dcn_pack_forward_plan(const float* input, const float* weight, const float* bias, const float* om,
                               float* output, int batch, int channels, int height, int width, int channels_out,
                               int stride, int pad, int dilation, int deformable_group, int act, float slope,
                               void* probe, void* workspace, size_t workspace_bytes, RVSR_HOST long long* plan);
int rvsr_dcn_pack_backward_plan(const float* input, const float* weight, const float* om, const float* grad_output,
                                const float* act_out, float act_slope, float* grad_input, float* grad_weight,
                                float* grad_bias, float* grad_om, int batch, int channels, int height, int width,
                                int channels_out, int stride, int pad, int dilation, int deformable_group,
                                const void* probe, void* workspace, size_t workspace_bytes, RVSR_HOST long long* plan);
/* Three rules of csrc/dcn_plan.h for the host glue (no GPU needed): the code with which the fused entries of sections 1 / 1b answer a
 * geometry (RVSR_OK: taken); the number of samples behind the counters of rvsr_dcn_offset_probe; and the tile halo (3 / 7 / 11; 0: no
 * samples) that a forward with channels_out output channels selects on the device from such counters -- `counters`: 6 uint32 in HOST
 * memory, read only and therefore unmarked (RVSR_HOST) -- so that a caller who kept them can pass the same choice as the hint of a later step. */
int rvsr_dcn_fused_takes(int batch, int channels, int height, int width, int channels_out, int kernel_h, int kernel_w, int stride_h,
                         int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w, int group, int deformable_group);
size_t rvsr_dcn_probe_samples(int batch, int deformable_group, int height_out, int width_out);
int rvsr_dcn_forward_halo(const unsigned* counters, size_t nsamples, int channels_out);

/* 1c. The operator over its whole argument space: any kernel_h x kernel_w, anisotropic stride / padding / dilation, group >= 1, any
 * number of channels per deformable group, DCNv1 (mask == NULL) and DCNv2, element types f32 / f64 / f16 (dtype 0 / 1 / 2) -- what
 * modulated_deform_conv_cuda_forward / _backward and the three deform_conv_*_cuda functions accept (deform_conv_cuda.cpp:490-685,
 * 152-488; AT_DISPATCH_FLOATING_TYPES_AND_HALF, deform_conv_cuda_kernel.cu:781).  Sections 1 / 1b above are the fused f32 kernels for
 * the geometries the reference's architectures instantiate (3 x 3, isotropic); this is the general path behind the same Python
 * operator, organised as the reference organises it (per batch element: columns in the workspace + one GEMM per group).  All tensors
 * of a call have the element type `dtype`; arithmetic is f32 for f16 / f32 tensors and f64 for f64.
 *   backward: grad_input (zero on entry: scatter-add) and grad_offset are given together or both NULL; grad_mask NULL for DCNv1;
 *   grad_weight / grad_bias are accumulated into, NULL = skip. */
size_t rvsr_deform_conv_generic_workspace_bytes(int dtype, int channels, int height, int width, int kernel_h, int kernel_w,
                                                int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w);
/* what the forward alone needs (one column buffer instead of two + the f16 scatter planes) */
size_t rvsr_deform_conv_generic_forward_workspace_bytes(int dtype, int channels, int height, int width, int kernel_h, int kernel_w,
                                                        int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h,
                                                        int dilation_w);
int rvsr_deform_conv_generic_forward(int dtype, const void* input, const void* weight, const void* bias, const void* offset,
                                     const void* mask, void* output, int batch, int channels, int height, int width,
                                     int channels_out, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                                     int dilation_h, int dilation_w, int group, int deformable_group, void* workspace,
                                     size_t workspace_bytes, void* stream);
int rvsr_deform_conv_generic_backward(int dtype, const void* input, const void* weight, const void* offset, const void* mask,
                                      const void* grad_output, void* grad_input, void* grad_offset, void* grad_mask,
                                      void* grad_weight, void* grad_bias, int batch, int channels, int height, int width,
                                      int channels_out, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                                      int dilation_h, int dilation_w, int group, int deformable_group, void* workspace,
                                      size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 2. Convolution blocks (nn.Conv2d 3x3 / 1x1, padding = ksize/2) with fused neighbours
 *    (EDVR_arch.py:96-132, 166-208, 256-319; arch_util.py:121-139)
 * --------------------------------------------------------------------------------------------- */

/* out = act(conv(cat(x1, x2)) + bias) [+ residual]
 *   x1 (B,C1,..), x2 (B,C2,..) or NULL/0: torch.cat([x1,x2],1) without materialising it.
 *   in_mode 0: x1 is (B,C1,Hs,Ws).
 *   in_mode 1: x1 is read through a zero-inserted x2 view of virtual size (Hout,Wout)
 *              (data gradient of a stride-2 conv).
 *   in_mode 2: x1 is stored (B,C1/4,Hs,Ws) and read pixel-unshuffled as (B,C1,Hs/2,Ws/2)
 *              (gradient arriving through nn.PixelShuffle(2), EDVR_arch.py:311-312).
 *   xact (NULL or a tensor stored like x1): value *= (xact > 0 ? 1 : xact_slope), i.e. the
 *              ReLU / LeakyReLU derivative taken from the saved activation output.
 *   weight: w_mode 0 -> (Co, C1+C2, k, k) used as is;
 *           w_mode 1 -> (C1+C2, Co, k, k) used transposed + spatially flipped (data gradient);
 *           w_mode | 2: `workspace` already holds the packed image of these weights (section 2b), the per-call pack is skipped.
 *           w_mode | 4 (opt-in): this forward conv forms its products in the f16 + fp8 format -- a1*b1 on v_mfma_f32_32x32x16_f16 plus
 *               the cross terms a1*b2 + a2*b1 on v_mfma_scale_f32_32x32x64_f8f6f4 (a1 = f16(a), a2 = a - a1, fp8 e4m3 with the 2^12 in the
 *               block scales): 56 instead of 108 matrix instructions per 16-channel stage, ~1.2e-5 instead of ~4.6e-6 relative l2 error
 *               per convolution (f32: 3e-7).  Only the plain vector-staged conv_fwd5 kernels with 64-row m-blocks read such an image
 *               (the rule: conv_fwd_plan, csrc/conv_plan.h); for any other call the flag is refused with RVSR_ERR_UNSUPPORTED and a
 *               message, nothing is launched, and rvsr_conv2d_forward_plan gives the same answer beforehand.
 *               Activations must lie inside f16's range (|x| < 65504; below 6e-8 they round to zero).  A packed image (w_mode | 2) must
 *               have been written with the same flag.  realvsr_amd.set_gemm_mode('f16fp8') sets it on every eligible forward conv.
 *   out1 (B,Co1,Hout,Wout) [+ out2 (B,Co2,Hout,Wout): rows split, for the gradient of a cat].
 *   residual (NULL or shaped like out1, out2 must be NULL): added after the activation.  It may be out1 itself (in-place accumulation):
 *        every element is read before it is stored, by the lane that stores it; act 3 reads `residual` as a mask and must not alias.
 *   act: 0 none, 1 ReLU, 2 LeakyReLU(slope); 3 (with `residual`, ksize 3, stride 1, one output): out = (conv + bias) * (residual > 0 ? 1 : slope),
 *        i.e. a data gradient multiplied by the derivative of the activation whose saved OUTPUT `residual` is -- the consumers of that
 *        gradient then need no mask.  An epilogue of the 8 x 64-tile kernel only: for calls that kernel does not take the plan refuses
 *        with RVSR_ERR_UNSUPPORTED and an empty message, nothing is launched, and the caller applies the mask on the consumer side
 *        (xact / gout_act) instead.
 *   pixel_shuffle 1: out1 is (B,Co/4,2*Hout,2*Wout), written through PixelShuffle(2).
 *   stride 2 only with ksize 3 or 5 and in_mode 0.
 *   ksize 5 (pad 2; the patch discriminator, discriminator_arch.py:46-92): stride-2 data gradients through in_mode 1 as for 3x3.
 *   ksize 7 (pad 3; SpyNet's blocks, TOF_arch.py:18-27): stride 1 only, on the exact-f32 kernel in every GEMM mode (no packed image:
 *   the workspace query is 0); w_mode | 4 is refused as for every other ineligible call.
 *   workspace: rvsr_conv2d_forward_workspace_bytes(C1, C2, Co1+Co2, ksize) bytes (holds the weights re-packed as bf16 hi/lo for the
 *   matrix cores; needed by the matrix-core kernels only).
 *   Which kernel a call runs -- the vector-ALU kernel for <= 4 output channels, conv_fwd5 (3x3 stride 1) or conv_fwd2 (3x3 stride 2,
 *   5x5, 1x1) on the bf16 matrix cores, or the exact-f32 kernel that takes everything else (GEMM mode 1, 5x5 through in_mode 1, inputs of
 *   2 GB per batch element, a second input behind a channel count the chunked staging cannot split at) -- and its tile, staging view,
 *   term count and grid are decided by ONE function, conv_fwd_plan (csrc/conv_plan.h), which states every rule once; all kernels
 *   compute the same convolution. */
size_t rvsr_conv2d_forward_workspace_bytes(int C1, int C2, int Co, int ksize);
int rvsr_conv2d_forward(const float* x1, int C1, const float* x2, int C2, const float* xact, float xact_slope,
                        int in_mode, int Hs, int Ws, const float* weight, const float* bias,
                        const float* residual, float* out1, int Co1, float* out2, int Co2, int B, int ksize,
                        int stride, int w_mode, int act, float slope, int pixel_shuffle, int Hout, int Wout,
                        void* workspace, size_t workspace_bytes, void* stream);
/* That function's answer for a call, without running it (no GPU needed, nothing launched, no pointer dereferenced): the arguments of
 * rvsr_conv2d_forward without workspace and stream; returns what the call itself would return before launching (RVSR_OK, a refusal or
 * a bad-argument code, rvsr_last_error set alike) and fills plan[14] = {family (0 vector ALU, 1 conv_fwd5, 2 conv_fwd2, 3 exact f32;
 * -1 refused), MT (32-row M tiles per workgroup), conv_fwd5's staging view (0 scalar, 1 plain, 2 pixel-unshuffle, 3 zero-insert),
 * 8 x 64 tile, terms of a product (3, 2, 1; 4 = f16 + fp8), act' on the input, CCG / CC, 16-byte-store epilogue, tile h, tile w,
 * grid x, y, z, LDS bytes}.  The host glue asks it where it has to know (realvsr_amd.functional: the w_mode | 4 gate, grad_mask_fusable). */
int rvsr_conv2d_forward_plan(const float* x1, int C1, const float* x2, int C2, const float* xact, float xact_slope,
                             int in_mode, int Hs, int Ws, const float* weight, const float* bias,
                             const float* residual, float* out1, int Co1, float* out2, int Co2, int B, int ksize,
                             int stride, int w_mode, int act, float slope, int pixel_shuffle, int Hout, int Wout,
                             RVSR_HOST int* plan);
/* The same call with a periodic addend in front of the activation (the PCD stage's conv(cat(x, ref.repeat(N))) = conv_a(x) + conv_b(ref),
 * realvsr_amd.functional.conv_cat_bcast):
 *     out1[b] = act((conv(x)[b] + bias) + addend[b % addend_period])
 *   addend: (addend_period, Co1, Hout, Wout), in the place of `residual`; frame-major x [N * B] with addend_period = B adds partial b to
 *   the N frames of window b.  conv + bias is rounded to f32 before the addend joins: the result is bit for bit what rvsr_conv2d_forward
 *   (act 0) followed by rvsr_bcast_add_act stores, without that pass's read and write of the output.
 *   addend_period 0: rvsr_conv2d_forward, argument for argument (`addend` is then its residual, added after the activation) -- one body
 *   serves both entries.  addend_period > 0 is an epilogue of the 8 x 64-tile conv_fwd5 kernel only: 3x3, stride 1, more than 32 output
 *   channels, a 16-byte-aligned plain input view and output with W % 4 == 0, one output, no pixel shuffle, not GEMM mode 1, not act 3.
 *   Every other call is refused by the plan with RVSR_ERR_UNSUPPORTED and an empty message, nothing is launched, and the caller runs the
 *   conv and rvsr_bcast_add_act instead.  rvsr_conv2d_forward_addend_plan is to it what rvsr_conv2d_forward_plan is to
 *   rvsr_conv2d_forward. */
int rvsr_conv2d_forward_addend(const float* x1, int C1, const float* x2, int C2, const float* xact, float xact_slope,
                               int in_mode, int Hs, int Ws, const float* weight, const float* bias,
                               const float* addend, float* out1, int Co1, float* out2, int Co2, int B, int ksize,
                               int stride, int w_mode, int act, float slope, int pixel_shuffle, int Hout, int Wout,
                               int addend_period, void* workspace, size_t workspace_bytes, void* stream);
int rvsr_conv2d_forward_addend_plan(const float* x1, int C1, const float* x2, int C2, const float* xact, float xact_slope,
                                    int in_mode, int Hs, int Ws, const float* weight, const float* bias,
                                    const float* addend, float* out1, int Co1, float* out2, int Co2, int B, int ksize,
                                    int stride, int w_mode, int act, float slope, int pixel_shuffle, int Hout, int Wout,
                                    int addend_period, RVSR_HOST int* plan);

/* 2b. Packed weight images, once per optimizer step.  The matrix-core kernels stage weights as bf16 hi/lo images
 *   ([m-block][chunk][hi|lo][tap][octet][row][8]); rvsr_conv2d_forward builds that image in its workspace on every call.
 *   rvsr_conv2d_pack_weights / rvsr_dcn_pack_weights write the image of one layer (forward: w_mode 0, data gradient: w_mode 1; w_mode 4:
 *   the forward image in the f16 + fp8 format of rvsr_conv2d_forward's w_mode | 4, for the layers that call grants it and for stride-1
 *   use only, 0 otherwise) to
 *   caller-owned memory of rvsr_conv2d_forward_workspace_bytes(C_in, 0, Co, ksize) /
 *   rvsr_modulated_deform_conv_forward_workspace_bytes(channels, channels_out) bytes and return that size (0 = bad argument);
 *   `desc` (NULL or 10 x long long, host; 20 x long long for rvsr_dcn_pack_weights) receives {weight, out, Co, C_in, taps, MP, CCG,
 *   nchunks, nmb, mode}.  The DCN forward keeps ONE image in that buffer, the tap-major one of its kernels (mode 0, desc[0..9]);
 *   rvsr_dcn_pack_weights still WRITES 20 values: desc[10..19] was the descriptor of a second, k-step-major image whose kernel has
 *   left the library, and is always all zero -- the caller's array must hold 20, only the first 10 mean anything.
 *   rvsr_pack_weights_batched re-packs n images in ONE launch from a DEVICE table of 48-byte records
 *   {const float* w; void* out; int Co, C_in, taps, MP, CCG, nchunks, nmb, mode;} built from those descriptors: the host
 *   (realvsr_amd.caches.PackedWeights) calls it once after the optimizer has updated the parameters in place. */
size_t rvsr_conv2d_pack_weights(const float* weight, int C_in, int Co, int ksize, int w_mode, void* out, size_t out_bytes,
                                RVSR_HOST long long* desc, void* stream);
int rvsr_pack_weights_batched(const void* descs, int n, void* stream);

/* grad_weight (Co,C1+C2,k,k) and grad_bias (Co) (NULL = skip) of the conv above.
 *   gout: gradient w.r.t. the conv output.  g_mode 0: stored (B,Co,Gs_h,Gs_w) = (.., Hout, Wout);
 *         g_mode 2: stored (B,Co/4,Gs_h,Gs_w) pixel-shuffled (2*Hout, 2*Wout).
 *   gact/gact_slope: fused activation derivative (stored like gout), or NULL.
 *   accumulate 0: overwrite, 1: += .  Deterministic (fixed-order reduction of partials).
 *   Eleven kernel families (vector ALU for <= 4 output channels; conv_wgrad2 / conv_wgrad5 / conv_wgrad1x1s / conv_wgrad1x1 /
 *   conv_wgrad_s2 on the bf16 matrix cores; an exact-f32 kernel per geometry, which also serves GEMM mode 1 and is the only one 7x7 has): conv_wgrad_plan
 *   (csrc/conv_plan.h) picks one and its slicing into partial sums; the workspace query sizes for the largest slicing any family of
 *   the geometry can ask for.  A 1x1 weight gradient runs the LDS-staged conv_wgrad1x1s when gout is plain (g_mode 0), Hout * Wout is
 *   a multiple of 4, all pointers are 16-byte aligned, one batch element of every tensor is below 2 GB and a second input starts on a
 *   multiple of 64 channels; otherwise conv_wgrad1x1 (Hout * Wout a multiple of 8, aligned) or the exact-f32 kernel. */
size_t rvsr_conv2d_wgrad_workspace_bytes(int C1, int C2, int Co, int B, int ksize, int stride, int Hout, int Wout);
int rvsr_conv2d_backward_weight(const float* x1, int C1, const float* x2, int C2, int Hin, int Win,
                                const float* gout, const float* gact, float gact_slope, int g_mode,
                                int Gs_h, int Gs_w, float* grad_weight, float* grad_bias, int Co, int B,
                                int ksize, int stride, int Hout, int Wout, int accumulate,
                                void* workspace, size_t workspace_bytes, void* stream);
/* conv_wgrad_plan's answer for that call, without running it (no GPU needed, nothing launched, no pointer dereferenced): the arguments
 * of rvsr_conv2d_backward_weight that the plan looks at, the same validation and return code, and plan[4] = {family in the order of
 * ConvWgradFamily (0 vector ALU, 1 conv_wgrad2, 2 conv_wgrad5, 3 exact f32 5x5, 4 conv_wgrad1x1s, 5 conv_wgrad1x1, 6 exact f32 3x3,
 * 7 conv_wgrad_s2, 8 exact f32 3x3 stride 2, 9 exact f32 1x1, 10 exact f32 7x7), partial sums P, grid y, grid z}.  The workspace the call needs is
 * rvsr_conv2d_wgrad_workspace_bytes >= 4 * P * (Co * (C1 + C2) * k * k + Co) bytes. */
int rvsr_conv2d_backward_weight_plan(const float* x1, int C1, const float* x2, int C2, int Hin, int Win,
                                     const float* gout, const float* gact, float gact_slope, int g_mode,
                                     int Gs_h, int Gs_w, float* grad_weight, int Co, int B, int ksize, int stride,
                                     int Hout, int Wout, RVSR_HOST int* plan);

/* ---------------------------------------------------------------------------------------------
 * 3. Fusion / resampling element-wise chain
 * --------------------------------------------------------------------------------------------- */

/* scale * F.interpolate(x, scale_factor=factor, mode='bilinear', align_corners=False), factor 2|4
 * (EDVR_arch.py:111-112,115,120-121,124,194,200,316).  in: `planes` images of HxW. */
int rvsr_upsample_bilinear_forward(const float* in, float* out, size_t planes, int H, int W, int factor,
                                   float scale, void* stream);
int rvsr_upsample_bilinear_backward(const float* gout, float* gin, size_t planes, int H, int W, int factor,
                                    float scale, void* stream);

/* cat([MaxPool2d(3,2,1)(x), AvgPool2d(3,2,1)(x)], 1) (EDVR_arch.py:154-155,188-194):
 * in (B,C,H,W) -> out (B,2C,Ho,Wo), argmax (B,C,Ho,Wo) uint8 saved for the backward. */
int rvsr_maxavgpool_forward(const float* in, float* out, unsigned char* argmax, int B, int C, int H, int W,
                            void* stream);
int rvsr_maxavgpool_backward(const float* gout, const unsigned char* argmax, float* gin, int B, int C, int H,
                             int W, void* stream);

/* TSA temporal attention (EDVR_arch.py:171-181): prob[b,n] = sigmoid(sum_c emb[b,n,c]*emb_ref[b,c]);
 * mod[b,n,c] = aligned[b,n,c] * prob[b,n].  mod (B,N,C,H,W), emb_ref (B,C,H,W), prob (B,N,H,W);
 * emb / aligned (and galigned / gemb): (B,N,C,H,W) as the reference stacks them (frame_major 0), or (N,B,C,H,W) =
 * the frame-major batch the alignment stage works on (frame_major 1: no transposing copy between the two stages). */
int rvsr_tsa_temporal_forward(const float* emb, const float* emb_ref, const float* aligned, float* mod,
                              float* prob, int B, int N, int C, int H, int W, int frame_major, void* stream);
int rvsr_tsa_temporal_backward(const float* gmod, const float* emb, const float* emb_ref, const float* aligned,
                               const float* prob, float* galigned, float* gemb, float* gemb_ref, int B, int N,
                               int C, int H, int W, int frame_major, void* stream);

/* out = fea * sigmoid(att) * 2 + att_add (EDVR_arch.py:204-207); grad w.r.t. att_add is g itself. */
int rvsr_tsa_output_forward(const float* fea, const float* att, const float* att_add, float* out, size_t n,
                            void* stream);
int rvsr_tsa_output_backward(const float* g, const float* fea, const float* att, float* gfea, float* gatt,
                             size_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 4. Laplacian pyramid decomposition + Charbonnier loss (utils/util.py:491-554, loss.py:10-23)
 * --------------------------------------------------------------------------------------------- */

/* downsample(conv_gauss(x)): reflect-pad 2, 5x5 binomial /256, keep even rows/cols.
 * in: `planes` images HxW -> out ceil(H/2) x ceil(W/2).  (utils/util.py:503-510) */
int rvsr_pyr_down_forward(const float* in, float* out, size_t planes, int H, int W, void* stream);
int rvsr_pyr_down_backward(const float* gout, float* gin, size_t planes, int H, int W, void* stream);
/* out = cur - upsample(down): zero-insert at even positions, reflect-pad 2, 5x5 binomial * 4/256
 * (utils/util.py:513-516, 548-551).  H, W even; down is (H/2, W/2).
 * backward: grad_cur = gout (identity), grad_down computed here. */
int rvsr_pyr_updiff_forward(const float* cur, const float* down, float* out, size_t planes, int H, int W,
                            void* stream);
int rvsr_pyr_updiff_backward(const float* gout, float* gdown, size_t planes, int H, int W, void* stream);

/* out[0] = scale * sum(sqrt((x-y)^2 + eps))  (scale = 1/n for reduction='mean'). */
size_t rvsr_charbonnier_workspace_bytes(void);
int rvsr_charbonnier_forward(const float* x, const float* y, size_t n, float eps, double scale, float* out,
                             void* workspace, void* stream);
/* gx = gscalar[0] * scale * (x-y)/sqrt((x-y)^2+eps); gscalar is a device pointer (no host sync). */
int rvsr_charbonnier_backward(const float* x, const float* y, const float* gscalar, float scale, float eps,
                              float* gx, size_t n, void* stream);

/* GWLoss (codes/models/loss.py:54-80): out[0] = scale * sum (1 + w|Sx(d)|)(1 + w|Sy(d)|)|d|, d = x1 - x2, depthwise 3x3 Sobel
 * with zero padding.  fa/fbx/fby (NULL together, or three buffers shaped like x1) receive the per-pixel factors the
 * backward needs.  workspace: rvsr_charbonnier_workspace_bytes().  backward: gx1 = gscalar[0]*scale * dL/dx1 (dL/dx2 = -gx1). */
int rvsr_gwloss_forward(const float* x1, const float* x2, size_t planes, int H, int W, float w, double scale, float* out,
                        float* fa, float* fbx, float* fby, void* workspace, void* stream);
int rvsr_gwloss_backward(const float* fa, const float* fbx, const float* fby, const float* gscalar, float scale, float* gx,
                         size_t planes, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 5. Test-time output conversion
 * --------------------------------------------------------------------------------------------- */

/* ycc: planar f32 [3][H][W] network output (Y, Cb, Cr in [0, 1] nominal) -> bgr: uint8 [H][W][3].
 * Replaces the host-side numpy chain of codes/test_RealVSR_wi_GT.py:122-123
 * (utils/util.py:151-181 tensor2img(float32, reverse_channel=False) -> data/util.py:397-416 ycbcr2bgr ->
 * clip, *255, round, uint8), same arithmetic order and precisions: bit-exact. */
int rvsr_ycbcr_to_bgr_u8(const float* ycc, unsigned char* bgr, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 6. The rest of the reference's pixel criteria (codes/models/loss.py) and pyramid helpers
 * --------------------------------------------------------------------------------------------- */

/* Bytes of the partial-sum workspace the reductions below need. */
size_t rvsr_reduce_workspace_bytes(void);

/* out[0] = scale * sum f(x - y) over n elements; mode 0: |d| (nn.L1Loss, loss.py:167-168), 1: d^2 (nn.MSELoss, :169-170),
 * 2: Huber with delta = param (HuberLoss, loss.py:26-40), 3: sqrt(d^2 + param) (CharbonnierLoss, loss.py:10-23).
 * backward: gx = gscalar[0] * scale * f'(x - y)  (grad w.r.t. y is -gx); gscalar is a device pointer. */
int rvsr_pixel_loss_forward(const float* x, const float* y, size_t n, int mode, float param, double scale, float* out,
                            void* workspace, void* stream);
int rvsr_pixel_loss_backward(const float* x, const float* y, const float* gscalar, int mode, float param, float scale,
                             float* gx, size_t n, void* stream);

/* SSIM loss as LapPyrLoss(lf_mode='ssim') uses it (loss.py:203,209,222 -> IQA_pytorch.SSIM(channels=1)(x, y, as_loss=True);
 * third-party, un-vendored: algorithm restated in oracle/ssim_oracle.py, parity unpinned): 11x11 Gaussian window sigma 1.5,
 * 'valid' correlation, C1 = 0.01^2, C2 = 0.03^2, contrast-structure map clamped at 0, out[0] = 1 - scale * sum(ssim_map)
 * with scale = 1 / (planes (H-10) (W-10)).  ga/gb/gc (NULL together, or planes x (H-10) x (W-10) each) receive
 * dS/dmu_x, dS/dE[xx], dS/dE[xy] for the backward: gx = -gscalar[0] * scale * window-adjoint(ga + 2 x gb + y gc). */
int rvsr_ssim_forward(const float* x, const float* y, size_t planes, int H, int W, double scale, float* out, float* ga,
                      float* gb, float* gc, void* workspace, void* stream);
int rvsr_ssim_backward(const float* x, const float* y, const float* ga, const float* gb, const float* gc,
                       const float* gscalar, float scale, float* gx, size_t planes, int H, int W, void* stream);

/* conv_gauss(img, gain * gauss_kernel) (utils/util.py:503-506): reflect-pad 2 + depthwise 5x5 binomial /256, same size. */
int rvsr_conv_gauss_forward(const float* in, float* out, size_t planes, int H, int W, float gain, void* stream);
int rvsr_conv_gauss_backward(const float* gout, float* gin, size_t planes, int H, int W, float gain, void* stream);
/* upsample(x) (utils/util.py:513-516): zero-insert to 2H x 2W, conv_gauss with 4 * kernel.  in planes x H x W. */
int rvsr_pyr_upsample_forward(const float* in, float* out, size_t planes, int H, int W, void* stream);
int rvsr_pyr_upsample_backward(const float* gout, float* gin, size_t planes, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 7. The two steps either side of netG in optimize_parameters
 * --------------------------------------------------------------------------------------------- */

/* One torch.optim.Adam update (VideoSR_AllPair_model_YCbCr_Split.py:122-124,187) of n contiguous f32 parameters, in place:
 *   g' = grad + weight_decay * param; exp_avg += (g' - exp_avg)(1 - beta1); exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) g'^2;
 *   param -= step_size * exp_avg / (sqrt(exp_avg_sq) / bias_correction2_sqrt + eps)
 * with step_size = lr / (1 - beta1^t), bias_correction2_sqrt = sqrt(1 - beta2^t) computed by the caller. 16-byte aligned buffers. */
int rvsr_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float step_size, float beta1,
                   float beta2, float eps, float weight_decay, float bias_correction2_sqrt, void* stream);

/* CutBlur / rgb-permute / blend of a clip pair (data/augments_video_allpair.py:38-88) in one pass over `frames` x 3 x H x W:
 *   a = im1[f, perm[c]], b = im2[f, perm[c]];  out1 = a;  out2 = b            (box_mode 0)
 *                                              out2 = inside box ? a : b      (box_mode 1: im1's box pasted into im2)
 *                                              out2 = inside box ? b : a      (box_mode 2: im2's box pasted into a copy of im1)
 *   colour != NULL (frames x 3): out = v * out + (1 - v) * colour[f, c]        (blend)
 * The random decisions (which augmentation, box, permutation, v) are drawn by the caller in the reference's host-RNG order. */
int rvsr_augment_clips(const float* im1, const float* im2, float* out1, float* out2, const float* colour, size_t frames, int H,
                       int W, int perm0, int perm1, int perm2, int box_mode, int y0, int y1, int x0, int x1, float v,
                       void* stream);

/* The algebraic split of the PCD "concat with the repeated reference" convs (EDVR_arch.py:100-101,109,118,127: conv(cat([nbr, ref]))
 * with ref identical for the N frames of a window): conv(cat(x, repeat(ref))) = conv_a(x) + conv_b(ref).  These two kernels are the
 * elementwise glue: a[n][j] = act(a[n][j] + b[j]) in place (n < N repeats of `per` floats; act 0 none, 1 ReLU, 2 LeakyReLU(slope)),
 * and its adjoint gb[j] = sum_n gout[n][j] * act'(out[n][j]) (out NULL: no activation). */
int rvsr_bcast_add_act(float* a, const float* b, size_t per, int N, int act, float slope, void* stream);
int rvsr_bcast_reduce_act(const float* gout, const float* out, float* gb, size_t per, int N, float gslope, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 7. GAN discriminator (VideoSRGAN_AllPair_model_YCbCr_Split.py; discriminator_arch.py:46-92, loss.py:102-133)
 * --------------------------------------------------------------------------------------------- */

/* nn.BatchNorm2d followed by LeakyReLU(slope) on x (B,C,HW planes), one fused operator:
 *   train 1: batch statistics (biased variance) through fixed-order two-stage reductions in double; save_mean / save_invstd
 *            (C floats) receive mean and 1/sqrt(var + eps); running_mean / running_var (NULL together = not tracked) are updated
 *            on the device with `momentum` (running_var with the unbiased variance); *num_batches_tracked (int64, NULL = none) += 1.
 *   train 0: running statistics (save_mean / save_invstd are written from them).
 *   y = lrelu((x - mean) * invstd * gamma + beta); gamma / beta NULL = 1 / 0.  B*HW >= 2 in train mode.
 *   workspace: rvsr_bn_workspace_bytes(B, C, HW) bytes, forward and backward alike.  Bit-identical from run to run. */
size_t rvsr_bn_workspace_bytes(int B, int C, int HW);
int rvsr_bn_lrelu_forward(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                          long long* num_batches_tracked, float* y, float* save_mean, float* save_invstd, int B, int C, int HW,
                          int train, float momentum, float eps, float slope, void* workspace, size_t workspace_bytes, void* stream);
/* Backward of the above: gz = gy * (y > 0 ? 1 : slope) from the saved OUTPUT y, xhat = (x - save_mean) * save_invstd;
 *   ggamma = sum gz * xhat, gbeta = sum gz (per channel, fixed order, double; NULL = skip);
 *   gx (NULL = skip) = gamma * invstd * (gz - mean(gz) - xhat * mean(gz * xhat)) in train mode, gamma * invstd * gz in eval mode. */
int rvsr_bn_lrelu_backward(const float* gy, const float* y, const float* x, const float* gamma, const float* save_mean,
                           const float* save_invstd, float* gx, float* ggamma, float* gbeta, int B, int C, int HW, int train,
                           float slope, void* workspace, size_t workspace_bytes, void* stream);

/* GAN criterion (GANLoss 'gan' / 'ragan' = BCEWithLogitsLoss, mean): out[0] = scale * sum_i bce(a_i - shift, target),
 *   shift = mean(b) (b != NULL, nb elements: the relativistic form) or 0; bce(z, t) = max(z, 0) - z t + log1p(exp(-|z|)).
 *   saved (2 device floats): {shift, sum_i (sigmoid(a_i - shift) - target)} for the backward.  One workgroup, fixed order, double.
 * Backward: ga_i = g * scale * (sigmoid(a_i - shift) - target); gb_j (gb may be NULL) = -g * scale * saved[1] / nb; g = gscalar[0]
 *   (device pointer: no host sync). */
int rvsr_gan_loss_forward(const float* a, size_t na, const float* b, size_t nb, float target, double scale, float* out, float* saved,
                          void* stream);
int rvsr_gan_loss_backward(const float* a, size_t na, size_t nb, const float* saved, const float* gscalar, float target, float scale,
                           float* ga, float* gb, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 8. Channel attention of RCAN (codes/models/archs/RCAN_arch.py:30-70: ChannelAttention, and the scaled residual add of RCAB)
 * --------------------------------------------------------------------------------------------- */

/* One fused operator on f32 NCHW contiguous tensors, C channels squeezed to Cr = C / squeeze_factor >= 1:
 *   pooled[b,c] = mean_hw u[b,c]                                  (AdaptiveAvgPool2d(1))
 *   hidden[b,j] = relu(w1[j,:] . pooled[b,:] + b1[j])             (w1: Cr x C, the 1x1 squeeze conv)
 *   gate[b,c]   = sigmoid(w2[c,:] . hidden[b,:] + b2[c])          (w2: C x Cr, the 1x1 excite conv)
 *   out         = (x ? x : 0) + res_scale * u * gate              (x NULL: no residual)
 * pooled (B x C), hidden (B x Cr) and gate (B x C) are written out for the backward.  Two launches: plane sums (one read of u), then
 * gate + stream (reads u and x, writes out).  No matrix cores and no atomics: exact f32 in every GEMM mode, bit-identical from run to
 * run.  workspace: rvsr_channel_attention_workspace_bytes(B, C, H, W) bytes, forward and backward alike.
 * Refused with RVSR_ERR_UNSUPPORTED: C > 4096 (the LDS scratch of the gate), Cr < 1 or Cr > C, a plane of 2^31 elements, null pointers. */
size_t rvsr_channel_attention_workspace_bytes(int B, int C, int H, int W);
/* The plan of a call without running it (pure host code, no GPU needed, no pointer dereferenced: the three streamed tensors are only
 * tested for alignment): *slices = workgroups and partial sums per (b, c) plane -- 1 where B * C planes fill the chip, more for a few
 * planes of a large frame; *vec = 1 when the kernels use 16-byte loads and stores (H * W % 4 == 0 and all three addresses 16-byte
 * aligned; x may be NULL), else 0, the scalar path.  Either output pointer may be NULL. */
int rvsr_channel_attention_plan(int B, int C, int H, int W, const void* u, const void* x, const void* out,
                                RVSR_HOST int* slices, RVSR_HOST int* vec);
int rvsr_channel_attention_forward(const float* u, const float* x /*NULL ok*/, const float* w1, const float* b1, const float* w2,
                                   const float* b2, float* out, float* pooled, float* hidden, float* gate, int B, int C, int Cr, int H,
                                   int W, float res_scale, void* ws, size_t ws_bytes, void* stream);
/* Backward, given gout = dL/dout and the saved pooled / hidden / gate:
 *   d[b,c] = sum_hw gout * u;  gp2 = res_scale * d * gate * (1 - gate);  gw2 = sum_b gp2 (x) hidden, gb2 = sum_b gp2;
 *   gz = (w2^T gp2) * [hidden > 0];  gw1 = sum_b gz (x) pooled, gb1 = sum_b gz;  gs = w1^T gz / (H * W);
 *   gu = res_scale * gate * gout + gs   (gs broadcast over the plane).
 * The gradient of x is gout itself: the caller passes it on.  gw1 / gb1 / gw2 / gb2 are WRITTEN, not accumulated (sum over b in ascending
 * order); any of the four may be NULL.  Three launches: plane dot products (reads gout and u), the small-matrix backward in one
 * workgroup, the stream (reads gout, writes gu). */
int rvsr_channel_attention_backward(const float* gout, const float* u, const float* w1, const float* w2, const float* pooled,
                                    const float* hidden, const float* gate, float* gu, float* gw1, float* gb1, float* gw2, float* gb2,
                                    int B, int C, int Cr, int H, int W, float res_scale, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 9. FSTRN: the temporal convolution of an FRB, PReLU and Dropout (codes/models/archs/FSTRN_arch.py)
 * --------------------------------------------------------------------------------------------- */

/* tconv3: nn.Conv3d(Ci, Co, (3, 1, 1), padding (1, 0, 0)) (FSTRN_arch.py:17), with the FRB's `res + out` (:22) and the PReLU of the
 * NEXT block (:15, :21) fused, on FRAME-MAJOR f32 tensors [T, B, C, H, W], contiguous:
 *   out[t,b,co,y,x]  = bias[co] + sum_{dt < 3, 0 <= t+dt-1 < T} sum_ci w[co,ci,dt] * s[t+dt-1,b,ci,y,x]  [+ residual[t,b,co,y,x]]
 *   pout[t,b,co,y,x] = out > 0 ? out : slope[0] * out          (pout may be NULL; slope is a DEVICE pointer)
 * w is the Conv3d weight, [Co, Ci, 3] contiguous.  transposed != 0: w is [Ci, Co, 3] and read as w[ci, co, 2 - dt] -- the data gradient
 * of the convolution whose weight it is.  bias and residual may be NULL; residual may be `out` itself (in-place accumulation), s may be
 * neither output.  One launch: a wave owns 32 pixels of a batch element and walks the frames with the operands of three frames in
 * registers, so s is read once; the weights of all taps stay in LDS.  Products follow the calling thread's GEMM mode: three-term bf16 split,
 * exact f32 in mode 1; modes 2 and 3 keep three terms.  No atomics: bit-identical from run to run.
 * Refused with RVSR_ERR_UNSUPPORTED: Ci > 64 or Co > 64 (the caller composes the operator from 1x1 convolutions), a plane of 2^23
 * elements; RVSR_ERR_BAD_ARG: empty shapes, null pointers. */
int rvsr_tconv3_forward(const float* s, const float* w, const float* bias /*NULL ok*/, const float* residual /*NULL ok*/,
                        const float* slope /*NULL ok without pout*/, float* out, float* pout /*NULL ok*/, int T, int B, int Ci, int Co, int H,
                        int W, int transposed, void* stream);
/* The plan of a call without running it (pure host code, no GPU needed, no pointer dereferenced): *vec = 1 when the kernel uses 16-byte
 * loads and stores (H * W % 4 == 0 and s, residual, out and pout 16-byte aligned, NULL counting as aligned), else 0, the scalar path;
 * *grid = workgroups launched.  Returns what rvsr_tconv3_forward would return for the shape.  Either output pointer may be NULL. */
int rvsr_tconv3_plan(int T, int B, int Ci, int Co, int H, int W, const void* s, const void* residual, const void* out, const void* pout,
                     RVSR_HOST int* vec, RVSR_HOST int* grid);

/* nn.PReLU() with one learnable slope (FSTRN_arch.py:15, :42), the long skip `lr_res + out` (:60) and nn.Dropout (:43, :62) in one pass
 * over n contiguous floats:
 *   y = prelu(a [+ b]) [* keep * scale]        prelu(x) = x > 0 ? x : slope[0] * x;  keep: n bytes, 0 = dropped;  scale = 1 / (1 - p)
 * b and keep may be NULL.  slope is a DEVICE pointer.  16-byte accesses when n % 4 == 0, the f32 tensors are 16-byte and keep 4-byte
 * aligned; else scalar. */
int rvsr_prelu_forward(const float* a, const float* b /*NULL ok*/, const float* slope, const unsigned char* keep /*NULL ok*/, float scale,
                       float* y, size_t n, void* stream);
/* Backward, x = a [+ b]:
 *   gx     = g * [keep * scale] * (x > 0 ? 1 : slope[0]) [+ gres]      (gres: a gradient arriving over a skip connection; may be gx)
 *   gslope = sum g * [keep * scale] * x * (x <= 0)                     (WRITTEN; per-workgroup partials in ws, summed by one workgroup
 *                                                                       in an order fixed by n: bit-identical from run to run)
 * gx or gslope may be NULL.  ws: rvsr_prelu_workspace_bytes() bytes. */
size_t rvsr_prelu_workspace_bytes(void);
int rvsr_prelu_backward(const float* g, const float* a, const float* b /*NULL ok*/, const float* slope, const unsigned char* keep /*NULL ok*/,
                        float scale, const float* gres /*NULL ok*/, float* gx, float* gslope, size_t n, void* ws, size_t ws_bytes,
                        void* stream);
/* The plan of a PReLU call (pure host code): *vec as above for the f32 tensors of the call, f0 .. f4 (forward: a, b, y; backward: g, a, b,
 * gres, gx; NULL where the call has none), and the keep mask; *blocks = workgroups, which is also the number of partial sums of the slope
 * gradient.  n == 0 is RVSR_ERR_BAD_ARG. */
int rvsr_prelu_plan(size_t n, const void* f0, const void* f1, const void* f2, const void* f3, const void* f4, const void* keep,
                    RVSR_HOST int* vec, RVSR_HOST int* blocks);

/* ---------------------------------------------------------------------------------------------
 * 10. TOF: the resampling operators of SpyNet (codes/models/archs/TOF_arch.py:54-88, arch_util.py:47-80)
 * --------------------------------------------------------------------------------------------- */

/* arch_util.flow_warp (arch_util.py:47-80; called at TOF_arch.py:84 per pyramid level and :87 at full resolution):
 *   out[b,c,y,x] = grid_sample(x, align_corners=True) at (x + flow[b,y,x,0], y + flow[b,y,x,1])
 * x, out, gout, gx (B,C,H,W); flow, gflow (B,H,W,2) in pixels, x first; all f32, contiguous.
 * The sampling coordinate is w + fx (h + fy) in one float32 addition.  The reference normalises, g = 2 (w + fx) / max(W - 1, 1) - 1, and
 * grid_sample un-normalises, (g + 1) / 2 * (W - 1): that round trip is the same number up to two or three ulps and is left out on
 * purpose, so that a zero flow is the identity and an integer flow a shift, bit for bit.  An axis of one pixel samples coordinate 0
 * whatever the flow, with flow gradient 0 (what the round trip gives: it multiplies by W - 1 = 0).
 * interp 0: bilinear, 1: nearest (round half to even).  padding 0: zeros, 1: border.  Anything else (reflection) is RVSR_ERR_UNSUPPORTED.
 * Backward: gflow (NULL = skip) is gathered, one thread per pixel over the channels -- no atomics, bit-identical from run to run; it is
 * zero for nearest, and under border for a coordinate on or beyond the frame's edge (<= 0 or >= W - 1, as grid_sample clips).  gx (NULL = skip) is scattered with float atomic adds INTO what the
 * buffer holds (the caller zero-fills it): order-dependent in its last bits.  x may be NULL when gflow is. */
int rvsr_flow_warp_forward(const float* x, const float* flow, float* out, int B, int C, int H, int W, int interp, int padding,
                           void* stream);
int rvsr_flow_warp_backward(const float* gout, const float* x /*NULL ok without gflow*/, const float* flow, float* gx /*NULL ok*/,
                            float* gflow /*NULL ok*/, int B, int C, int H, int W, int interp, int padding, void* stream);

/* F.avg_pool2d(x, 2, 2) (the image pyramids, TOF_arch.py:66-76): in `planes` images of HxW -> out of (H/2)x(W/2), sizes floor; an odd
 * last row or column takes no part and gets zero gradient.  A frame of one row or column pools to nothing (no launch). */
int rvsr_avgpool2_forward(const float* in, float* out, size_t planes, int H, int W, void* stream);
int rvsr_avgpool2_backward(const float* gout, float* gin, size_t planes, int H, int W, void* stream);

/* scale * F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True) (the flow between pyramid levels, TOF_arch.py:81-82):
 * source coordinate dst * (H - 1) / (2H - 1), 0 for H == 1.  The backward is a gather in a fixed order (no atomics). */
int rvsr_upsample2_ac_forward(const float* in, float* out, size_t planes, int H, int W, float scale, void* stream);
int rvsr_upsample2_ac_backward(const float* gout, float* gin, size_t planes, int H, int W, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 11. Validation metrics (codes/train.py:274-320, codes/test_RealVSR_wi_GT.py:134-168, utils/util.py:283-334)
 * --------------------------------------------------------------------------------------------- */

/* All entries of this section score PLANES: H x W float32 images with contiguous rows, plane p of an input starting
 * p * plane_stride ELEMENTS behind its pointer (channel 0 of a [B, 3, H, W] tensor: planes = B, plane_stride = 3 * H * W, no copy);
 * the two inputs have their own strides.  crop >= 0 drops that many pixels on every side first (util.crop_border,
 * test_RealVSR_wi_GT.py:139) by offsetting into the plane.  Both metrics see the QUANTISED image
 *     q(x) = uint8(rint(clamp(x, 0, 1) * 255.0f))     float32, round-half-even
 * which is bit for bit tensor2img's clamp (utils/util.py:157) followed by train.py:301-302, (x * 255.0).round().astype(np.uint8);
 * NaN quantises to 0 (numpy leaves that cast undefined).  No atomics, fixed summation orders: bit-identical from run to run.
 * workspace: rvsr_metric_workspace_bytes(planes, H, W, crop) bytes serve either metric (0 for an empty shape); a smaller one is
 * RVSR_ERR_WORKSPACE.  RVSR_ERR_BAD_ARG: null pointers, no planes or more than 65535, an empty cropped plane. */
size_t rvsr_metric_workspace_bytes(size_t planes, int H, int W, int crop);
/* The output tile one workgroup of the SSIM kernel computes (tests build their edge shapes from it). */
int rvsr_metric_tile(RVSR_HOST int* th, RVSR_HOST int* tw);

/* out[i] = q(x[i]) for n contiguous floats: the quantisation on its own. */
int rvsr_quantize_u8(const float* x, unsigned char* out, size_t n, void* stream);

/* util.calculate_psnr (utils/util.py:283-290; called on channel 0 at train.py:305 and test_RealVSR_wi_GT.py:142), its device part:
 * sse[p] = sum (q(a) - q(b))^2 over the cropped plane p, an exact 64-bit integer (device pointer, `planes` values).  The caller
 * finishes in double: mse = sse / n, 20 log10(255 / sqrt(mse)), inf for sse == 0 -- every partial sum is an integer below 2^53, so this
 * equals the reference's np.mean path exactly. */
int rvsr_psnr_sse(const float* a, size_t a_plane_stride, const float* b, size_t b_plane_stride, size_t planes, int H, int W, int crop,
                  long long* sse, void* workspace, size_t workspace_bytes, void* stream);

/* util.ssim (utils/util.py:293-313; calculate_ssim :316-334, called at test_RealVSR_wi_GT.py:143), its device part: sum[p] = the sum of
 * the SSIM map of the cropped plane p in double (device pointer, `planes` values); the caller divides by (Hc - 10) (Wc - 10).
 * Window: the outer product of cv2.getGaussianKernel(11, 1.5) = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, evaluated separably (11 + 11 taps
 * for each of mu1, mu2, E[x^2], E[y^2], E[xy]) in double on the quantised values; 'valid' region; C1 = (0.01 * 255)^2,
 * C2 = (0.03 * 255)^2.  Identical inputs give exactly (Hc - 10) (Wc - 10).  A cropped plane below 11 x 11 is RVSR_ERR_BAD_ARG. */
int rvsr_ssim_sum(const float* a, size_t a_plane_stride, const float* b, size_t b_plane_stride, size_t planes, int H, int W, int crop,
                  double* sum, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 12. Batch assembly (codes/data/RealVSR_dataset.py:142-172, 309-341, codes/data/util.py:86-122, 261-276)
 * --------------------------------------------------------------------------------------------- */

/* Packed uint8 frame crops -> the float32 batch, in one launch: what the reference's data package computes per sample on the host
 * (read_img's astype(np.float32) / 255., util.augment, np.stack, [2, 1, 0], HWC -> CHW, ascontiguousarray).
 *   src   uint8 [samples][frames][Hs][Ws][C], contiguous, at ANY byte alignment (read with 16-byte loads aligned down; no load is
 *         issued from an aligned 16-byte block that holds no source byte)
 *   dst   float32 [samples][frames][C][Ho][Wo], fully overwritten, nothing outside it written; 16-byte aligned for the vector stores
 *         (rvsr_assemble_plan), 4-byte aligned at least
 *   flags one int per sample (device memory) or NULL: bit 0 hflip, bit 1 vflip, bit 2 rot90, applied in the order of util.augment,
 *             a[y][x] = s[vflip ? Hs-1-y : y][hflip ? Ws-1-x : x],   out[y][x] = rot90 ? a[x][y] : a[y][x]
 *         With flags, Hs == Ws is required (RVSR_ERR_UNSUPPORTED otherwise; the reference's np.stack needs the same).  NULL: no flips,
 *         any Hs x Ws (whole validation frames).  Ho = Hs, Wo = Ws.
 *   C     1 or 3 (else RVSR_ERR_UNSUPPORTED)
 *   mode  RVSR_ASM_REVERSE: output plane c reads source channel C-1-c (the [2, 1, 0] of RealVSR_dataset.py:337-339, util.py:120).
 *         RVSR_ASM_TO_YCBCR (C == 3 only): the source holds raw colour bytes, in the order B, G, R with RVSR_ASM_REVERSE (cv2) and
 *         R, G, B without (PIL); the output planes are (Y, Cb, Cr) of util.bgr2ycbcr(uint8, only_y=False) (util.py:351-373) ROUNDED TO
 *         uint8 as scripts/prepare_data.py:42-45 stores them, then normalised -- in exact integers:
 *             v = 65481 R + 128553 G + 24966 B + 16 * 255000   (Cb: -37797, -74203, 112000, 128 * 255000;  Cr: 112000, -93786, -18214,
 *             128 * 255000),   value = v / 255000 rounded half to even.
 * The value map is float(u8) / 255.f correctly rounded: numpy's x.astype(np.float32) / 255. for all 256 values. */
#define RVSR_ASM_REVERSE 1
#define RVSR_ASM_TO_YCBCR 2
int rvsr_assemble_clips(const unsigned char* src, float* dst, const int* flags, size_t samples, int frames, int C, int Hs, int Ws,
                        int mode, void* stream);
/* The plan of that call (pure host code; the same shape checks): *variant = 1 for 16-byte stores (Ws % 4 == 0 and dst 16-byte aligned),
 * 0 for scalar stores; *blocks = workgroups (one per 64 x 64 output tile of an image). */
int rvsr_assemble_plan(const float* dst, size_t samples, int frames, int C, int Hs, int Ws, RVSR_HOST int* variant, RVSR_HOST int* blocks);

/* ---------------------------------------------------------------------------------------------
 * 12b. Batch assembly from a resident frame store (codes/data/RealVSR_dataset.py:120-172, 283-341, codes/data/util.py:86-101, 261-276)
 * --------------------------------------------------------------------------------------------- */

/* The same float32 batch as rvsr_assemble_clips, gathered from whole decoded frames that stay on the device: what the reference does
 * per sample with read_img on every frame of the window (RealVSR_dataset.py:120-140, 283-307: cv2.imread of a 1024 x 512 file each), the
 * crop (:154-157, :321-324), util.augment (:160-163, :327-330) and the stack / [2, 1, 0] / CHW tail (:166-172, :333-341) -- with the
 * files decoded once, at start-up.
 *   store  uint8 [store_frames][H][W][C], contiguous, at ANY byte alignment; read like `src` above (16-byte loads aligned down, none
 *          from an aligned block that holds no byte of a crop); every byte offset into it is a size_t
 *   table  int32 [samples][frames + 3] (device memory): per sample `frames` store slots, then the crop's row, its column, and the flags
 *          of section 12 (bits 0-2; higher bits are ignored)
 *   dst    float32 [samples][frames][C][S][S], fully overwritten, nothing outside it written:
 *              dst[b][f] = assemble(store[slot[b][f]][row_b : row_b + S, col_b : col_b + S], flags_b, mode)
 *          bit for bit the values of rvsr_assemble_clips on those crops packed contiguously (the kernels share the tile body)
 *   C      1 or 3;  1 <= S <= min(H, W) (RVSR_ERR_BAD_ARG otherwise);  mode as in section 12
 * What the table holds is device data the entry point cannot see: the kernel clamps a slot into [0, store_frames) and the origin into
 * [0, H - S] x [0, W - S], so a wrong table gives wrong pixels, never an access outside the store. */
int rvsr_gather_clips(const unsigned char* store, size_t store_frames, int H, int W, const int* table, float* dst, size_t samples,
                      int frames, int C, int S, int mode, void* stream);
/* The plan of that call (pure host code; the same shape checks where it has the numbers): *variant = 1 for 16-byte stores (S % 4 == 0
 * and dst 16-byte aligned), 0 for scalar stores; *blocks = workgroups (one per 64 x 64 output tile of an image). */
int rvsr_gather_plan(const float* dst, size_t samples, int frames, int C, int S, RVSR_HOST int* variant, RVSR_HOST int* blocks);

/* ---------------------------------------------------------------------------------------------
 * 13. Bicubic degradation of uint8 frames (codes/scripts/generate_LR_BI_Vimeo90K.m:28, codes/data/util.py:511-710)
 * --------------------------------------------------------------------------------------------- */

/* MATLAB's antialiased bicubic imresize (cubic with a = -0.5, stretched by `scale` when shrinking; symmetric reflection at the
 * borders) at the factors 1 / scale and scale, scale = 2 or 4, on uint8 frames, in exact integers: the LQ frames the reference's
 * Vimeo-90K runs read from a second copy of the data set, computed from the GT bytes instead.  At these factors every normalised
 * weight is k / 2^n:
 *     x 1/2   [-3, -9, 29, 111, 111, 29, -9, -3] / 256                     at inputs 2 j - 3 .. 2 j + 4 of output j
 *     x 2     [-3, 29, 111, -9] / 128 at inputs m - 2 .. m + 1 of output 2 m,   [-9, 111, 29, -3] / 128 at m - 1 .. m + 2 of 2 m + 1
 *     x 1/4   [-7, -45, -75, -49, 93, 399, 745, 987, 987, 745, 399, 93, -49, -75, -45, -7] / 4096   at inputs 4 j - 6 .. 4 j + 9
 *     x 4     [-45, 399, 745, -75], [-7, 93, 987, -49] / 1024 at m - 2 .. m + 1 of outputs 4 m, 4 m + 1;
 *             [-49, 987, 93, -7], [-75, 745, 399, -45] / 1024 at m - 1 .. m + 2 of outputs 4 m + 2, 4 m + 3
 * so a value is N / 2^b with N an integer sum over the bytes (|N| < 2^53), and the byte stored is
 *     clamp(floor((N + 2^(b-1)) / 2^b), 0, 255),     b = 16 (x 1/2), 24 (x 1/4), 30 (x 1/2 then x 2), 44 (x 1/4 then x 4);
 * the intermediate image of a two-stage chain is NOT rounded (MATLAB's is a double).  tests/bicubic_reference.py is this definition
 * in numpy; the reference's float32 imresize_np can differ from it, by 1, only where N / 2^b lies next to a half-integer (tests: within 1e-3).
 *   Hf, Wf the frame: multiples of `scale` (the script's modcrop), every edge >= 2 * scale (RVSR_ERR_UNSUPPORTED otherwise: below
 *          that one reflection no longer suffices), at most 2^24
 *   src    uint8 [samples][frames][Hw][Ww][C], contiguous, at ANY byte alignment (byte loads): a WINDOW of each frame, rows
 *          wy .. wy + Hw - 1 and columns wx .. wx + Ww - 1; Hw <= Hf, Ww <= Wf
 *   S_h, S_w   the crop, at (y0, x0) of the frame; RVSR_BIC_DOWN: crop size and origin are multiples of `scale`
 *   geom   four ints per sample (device memory), {wy, wx, y0, x0}, or NULL = all zeros (whole frames, or their top-left part)
 *   dst    RVSR_BIC_SAME: uint8 [samples][frames][S_h][S_w][C], shrink by `scale`, then enlarge by `scale`, rounded once;
 *          RVSR_BIC_DOWN: uint8 [samples][frames][S_h / scale][S_w / scale][C].
 *          Either holds what the chain gives on the WHOLE frame at the crop's position: both stages reflect at the frame's borders
 *          (the enlarging stage at those of the Hf / scale x Wf / scale intermediate image), not at the window's, so a random crop
 *          taken through a window is bit-identical to the crop of the degraded frame.
 *   crop   optional (NULL: not written): uint8 [samples][frames][S_h][S_w][C], the window's own bytes at the crop -- the GT crop, from
 *          the tile the same launch has staged
 *   C      1 or 3;  scale 2 or 4;  mode RVSR_BIC_SAME or RVSR_BIC_DOWN   (else RVSR_ERR_UNSUPPORTED)
 * The window has to hold every frame pixel an output touches after reflection.  rvsr_bicubic_halo(scale, mode) is how far that is
 * beyond the crop (7 / 3 at scale 2 SAME / DOWN, 15 / 6 at scale 4; derived from the tables, -1 for an unknown scale or mode); the
 * host uploads rows [clamp(y0 - h, 0, Hf - (S_h + 2 h)), + S_h + 2 h), or the whole frame where that is smaller, and columns alike.
 * The entry point checks the sizes (RVSR_ERR_BAD_ARG: a window smaller than that; with geom == NULL smaller than S + h).  WHERE the
 * window and the crop sit is device data: the kernel clamps them into the frame and clamps every read into the window, so a wrong
 * geometry gives wrong bytes, never an access outside src.  dst and crop are fully overwritten, nothing outside them is written.
 * One workgroup per 32 x 32 (SAME) or 16 x 16 (DOWN) tile of dst of one image; one kernel variant per (scale, mode, C). */
#define RVSR_BIC_SAME 0
#define RVSR_BIC_DOWN 1
int rvsr_bicubic_u8(const unsigned char* src, unsigned char* dst, unsigned char* crop, const int* geom, size_t samples, int frames, int C,
                    int Hw, int Ww, int Hf, int Wf, int S_h, int S_w, int scale, int mode, void* stream);
int rvsr_bicubic_halo(int scale, int mode);   /* pure host code */

/* Measurement aid, not part of the reference's interface (bench.py: roofline_conv.sustained_peak): `workgroups` x 8 waves loop `iters`
 * times over 8 register-resident v_mfma_f32_32x32x16_bf16 whose operands come from `ops` (8 x 512 x 16 B of bf16: [operand][thread][8]);
 * out: workgroups x 512 floats (checksums).  MFMA work issued = workgroups * 8 waves * iters * 8 * 32768 FLOP. */
int rvsr_debug_mfma_rate(const void* ops, float* out, int workgroups, int iters, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* REALVSR_HIP_H */
