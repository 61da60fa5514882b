"""What the bit-for-bit pins of the reduced-term GEMM modes stand on (tests/test_gpu_modes_definition.py; plain CPU helper, its own facts
are shown in tests/test_modes_reference_host.py).

The kernels of the modes 'bf16x2' / 'bf16' accumulate hi*hi, then hi*lo, then lo*hi into one f32 accumulator.  An operand that already is
a bf16 value has lo == 0, the product of two bf16 values is exact in f32, and a matrix instruction on a zero operand adds exact zeros: so
the three-term kernel on PRE-ROUNDED operands produces the very bits of the reduced-term kernel on the original ones.  Pre-rounding is
`bf16_round`.  The deformable kernels form one operand themselves -- the sampled column mask * bilinear(x) -- and that one is a bf16
value whenever x is, if the sample positions are integers (one corner with weight exactly 1) and the mask a power of two:
`integer_offsets` and `pow2_masks` draw such fields."""
import torch

MASK_VALUES = (1.0, 0.5, 0.25)


def bf16_round(t):
    """Round to nearest even through torch.bfloat16 (what split8 of csrc/bf16x3.h keeps as the hi part); float32 out."""
    return t.to(torch.bfloat16).to(torch.float32)


def integer_offsets(B, dg, Ho, Wo, reach, generator, taps=9):
    """(B, dg * 2 * taps, Ho, Wo) float32 offsets, integer-valued and independent per (batch element, deformable group, tap, component,
    pixel), uniform in [-reach, reach]: channel g * 2 * taps + 2 k is dy, + 1 dx of tap k (deform_conv_cuda_kernel.cu:608-612).  Pixels near
    the border sample outside the frame for every reach >= 0 (tap 0 of pixel (0, 0) sits at (-1, -1) already), more of them the larger
    the reach; a reach beyond the frame puts whole taps outside."""
    reach = int(reach)
    return torch.randint(-reach, reach + 1, (B, dg * 2 * taps, Ho, Wo), generator=generator).to(torch.float32)


def pow2_masks(B, dg, Ho, Wo, generator, taps=9):
    """(B, dg * taps, Ho, Wo) float32 masks drawn from {1, 0.5, 0.25}: a product with one is an exponent shift."""
    idx = torch.randint(0, len(MASK_VALUES), (B, dg * taps, Ho, Wo), generator=generator)
    return torch.tensor(MASK_VALUES, dtype=torch.float32)[idx]


def sample_positions(offset, dg, pad=1, taps=9):
    """(y, x) int64 tensors (B, dg, taps, Ho, Wo): the image position tap k of deformable group g samples at each output pixel for
    INTEGER offsets, 3 x 3 / stride 1 / dilation 1: (h - pad + k // 3 + dy, w - pad + k % 3 + dx) (kernel.cu:594-616)."""
    B, _, Ho, Wo = offset.shape
    o = offset.view(B, dg, taps, 2, Ho, Wo)
    assert bool((o == o.round()).all()), 'integer offsets only'
    k = torch.arange(taps).view(1, 1, taps, 1, 1)
    h = torch.arange(Ho).view(1, 1, 1, Ho, 1)
    w = torch.arange(Wo).view(1, 1, 1, 1, Wo)
    return h - pad + k // 3 + o[:, :, :, 0].long(), w - pad + k % 3 + o[:, :, :, 1].long()


def gathered_columns(x, offset, mask, dg, pad=1, taps=9):
    """(B, C * taps, Ho * Wo) columns of the modulated DCN's im2col for INTEGER offsets, by plain gathers: row c * taps + k holds
    mask[b, g * taps + k] * x[b, c, y, x] at the sampled position inside the frame and 0 outside; also returns the (B, C * taps, Ho * Wo)
    bool of in-frame samples.  Same dtype as x."""
    B, C, H, W = x.shape
    cpg = C // dg
    y, xx = sample_positions(offset, dg, pad, taps)
    Ho, Wo = y.shape[-2:]
    inside = (y >= 0) & (y < H) & (xx >= 0) & (xx < W)
    flat = (y.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).view(B, dg, 1, taps, Ho * Wo).expand(B, dg, cpg, taps, Ho * Wo)
    src = x.reshape(B, dg, cpg, 1, H * W).expand(B, dg, cpg, taps, H * W)
    val = torch.gather(src, 4, flat)
    ins = inside.view(B, dg, 1, taps, Ho * Wo).expand(B, dg, cpg, taps, Ho * Wo)
    m = mask.view(B, dg, 1, taps, Ho * Wo).to(x.dtype)
    col = torch.where(ins, val * m, torch.zeros((), dtype=x.dtype))
    return col.reshape(B, C * taps, Ho * Wo), ins.reshape(B, C * taps, Ho * Wo)
