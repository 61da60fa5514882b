"""Case builders and the float64 reference for the two non-convolution operators of the GAN stage (csrc/gan_kernels.hip):
BatchNorm2d + LeakyReLU and the BCE-with-logits criterion.  Shared by test_gan_reference_host.py (which holds the case list to the
conditions it is named for) and test_gpu_gan_edges.py.

The reference is torch's own ``F.batch_norm`` -> ``F.leaky_relu`` and ``F.binary_cross_entropy_with_logits`` in float64 under autograd
-- what the reference project executes -- on inputs generated in float32.  The same functions run in float32 give the yardstick of the
ill-conditioned cases: how far a plain float32 evaluation of the operator is from float64 on the very same inputs.

Kink rule (as in the conv tests): the output gradient is zeroed where the float64 pre-activation has |v| <= KINK, the derivative of
the LeakyReLU there depends on the last bits of v."""
import functools

import torch
import torch.nn.functional as F

KINK = 1e-3

# ------------------------------------------------------------------------------------------ BatchNorm2d + LeakyReLU
# name: (B, C, H, W, NP the case is named for, x kind, gy kind).  n = B * H * W values per channel are cut into
# NP = min(64, ceil(n / 8192)) slices [n * q / NP, n * (q + 1) / NP); the statistics kernels run 64 channels per workgroup.
#   x kind:  'randn'  1.7 * randn + a per-channel offset 3 * randn
#            'const'  the same with channel 1 constant (variance clamps to 0, invstd = 1 / sqrt(eps))
#            'mean1e3' per-channel mean +-1e3 at unit spread;  'spread1e-4'  2 + 1e-4 * randn
#   gy kind: 'noise'  randn;  'stats'  randn + 0.5 + 0.5 * xhat per channel: mean(gz) and mean(gz * xhat) are O(1), the two statistics
#            terms of gx = k1 * (gz - mean(gz) - xhat * mean(gz * xhat)) are then as large as gx itself
BN_CASES = {
    'n2':                 (2, 3, 1, 1, 1, 'randn', 'noise'),
    'n6_stats':           (2, 4, 1, 3, 1, 'randn', 'stats'),
    'n8192':              (2, 2, 64, 64, 1, 'randn', 'noise'),
    'n8193':              (1, 2, 1, 8193, 2, 'randn', 'noise'),           # slices of 4096 and 4097
    'ragged_np2_stats':   (5, 3, 41, 41, 2, 'randn', 'stats'),            # n = 8405: the boundary 4202 lies inside plane 2 of 5
    'ragged_np3_stats':   (7, 2, 49, 49, 3, 'randn', 'stats'),            # n = 16807: boundaries 5602 and 11204
    'ragged_cap64_stats': (1, 2, 725, 725, 64, 'randn', 'stats'),         # n = 525625: ceil(n / 8192) = 65 -> 64, n % 64 = 57
    'c1':                 (3, 1, 5, 7, 1, 'randn', 'noise'),
    'c65_stats':          (2, 65, 3, 5, 1, 'randn', 'stats'),
    'c130':               (2, 130, 2, 3, 1, 'randn', 'noise'),
    'ill_const':          (2, 4, 5, 7, 1, 'const', 'noise'),
    'ill_mean1e3':        (2, 4, 5, 7, 1, 'mean1e3', 'noise'),
    'ill_spread1e-4':     (2, 4, 5, 7, 1, 'spread1e-4', 'noise'),
}
# seeds: chosen so that the kink rule zeroes at most 1 % of gy (test_gan_reference_host.py holds every case to that)
BN_SEEDS = {name: 2200 + i for i, name in enumerate(BN_CASES)}
ILL_CONDITIONED = ('ill_const', 'ill_mean1e3', 'ill_spread1e-4')     # every tensor by the yardstick rule; 'n2': gx alone
BN_DEFAULTS = dict(momentum=0.1, eps=1e-5, slope=0.2)


def bn_raw(B, C, H, W, seed, xkind='randn', gykind='noise', eps=1e-5):
    """Seeded float32 CPU inputs: x, gy, weight, bias, running_mean, running_var."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)    # noqa: E731
    if xkind in ('randn', 'const'):
        x = rn(B, C, H, W) * 1.7 + rn(1, C, 1, 1) * 3.0
        if xkind == 'const':
            x[:, 1] = 0.7
    elif xkind == 'mean1e3':
        sign = torch.tensor([1.0, -1.0] * C)[:C].view(1, C, 1, 1)
        x = rn(B, C, H, W) + 1e3 * sign * (1.0 + 0.1 * torch.rand(1, C, 1, 1, generator=g))
    elif xkind == 'spread1e-4':
        x = 2.0 + 1e-4 * rn(B, C, H, W)
    else:
        raise ValueError(xkind)
    weight = 1.0 + 0.3 * rn(C)
    bias = 0.2 * rn(C)
    bias = torch.where(bias.abs() < 0.05, torch.full_like(bias, 0.05), bias)    # (a constant channel's pre-activation IS its bias)
    running_mean = 0.1 * rn(C)
    running_var = 1.0 + 0.2 * torch.rand(C, generator=g)
    gy = rn(B, C, H, W)
    if gykind == 'stats':
        xd = x.double()
        m = xd.mean((0, 2, 3), keepdim=True)
        xhat = (xd - m) / torch.sqrt(xd.var((0, 2, 3), unbiased=False, keepdim=True) + eps)
        gy = (gy.double() + 0.5 + 0.5 * xhat).float()
    elif gykind != 'noise':
        raise ValueError(gykind)
    return dict(x=x, gy=gy, weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)


@functools.lru_cache(maxsize=None)
def bn_inputs(name):
    """The inputs of a named case, made once and never written."""
    B, C, H, W, _, xkind, gykind = BN_CASES[name]
    return bn_raw(B, C, H, W, BN_SEEDS[name], xkind, gykind)


def bn_reference(x, gy, weight, bias, running_mean, running_var, train=True, momentum=0.1, eps=1e-5, slope=0.2, dtype=torch.float64,
                 kink=True):
    """lrelu(batch_norm(x)) and its backward in `dtype` under autograd.  weight / bias None: affine=False.  running_* None: no buffers
    (track_running_stats=False: batch statistics in eval too).  Returns a dict:
      v, y, gx, ggamma, gbeta (None without affine), running_mean, running_var (the NEW values; None without buffers),
      gy     the float32 output gradient that was applied (zeroed by the kink rule if `kink`), share: the fraction zeroed,
      k1     gamma * invstd per channel, gz = gy * lrelu'(v), stat = gx - k1 * gz: the statistics part of gx (zero in eval mode)."""
    assert all(t is None or t.dtype == torch.float32 for t in (x, gy, weight, bias)), 'generate in float32'    # (buffers: as handed on)
    C = x.shape[1]
    xr = x.to(dtype).requires_grad_(True)
    w = None if weight is None else weight.to(dtype).requires_grad_(True)
    b = None if bias is None else bias.to(dtype).requires_grad_(True)
    rm = None if running_mean is None else running_mean.to(dtype).clone()
    rv = None if running_var is None else running_var.to(dtype).clone()
    use_batch = bool(train) or rm is None
    if use_batch:
        mean = xr.detach().mean((0, 2, 3))
        invstd = 1.0 / torch.sqrt(xr.detach().var((0, 2, 3), unbiased=False) + eps)
    else:
        mean, invstd = rm.clone(), 1.0 / torch.sqrt(rv + eps)
    v = F.batch_norm(xr, rm, rv, w, b, use_batch, momentum, eps)
    if kink:
        keep = v.detach().abs() > KINK
        gy, share = gy * keep.float(), 1.0 - keep.double().mean().item()
    else:
        share = 0.0
    y = F.leaky_relu(v, slope)
    y.backward(gy.to(dtype))
    k1 = (invstd if w is None else w.detach() * invstd).view(1, C, 1, 1)
    gz = gy.to(dtype) * torch.where(v.detach() > 0, torch.ones((), dtype=dtype), torch.full((), float(slope), dtype=dtype))
    return dict(v=v.detach(), y=y.detach(), gx=xr.grad, ggamma=None if w is None else w.grad, gbeta=None if b is None else b.grad,
                running_mean=rm, running_var=rv, gy=gy, share=share, k1=k1, gz=gz, stat=xr.grad - k1 * gz, mean=mean, invstd=invstd)


BN_TENSORS = ('y', 'gx', 'ggamma', 'gbeta', 'running_mean', 'running_var')


def bn_yardstick(ref, x, weight, bias, running_mean, running_var, **kw):
    """max |float32 - float64| per tensor of the same torch CPU computation on the same inputs (ref: the float64 result, whose
    kink-zeroed gy is reused as it is)."""
    f32 = bn_reference(x, ref['gy'], weight, bias, running_mean, running_var, dtype=torch.float32, kink=False, **kw)
    return {k: (f32[k].double() - ref[k]).abs().max().item() for k in BN_TENSORS if ref[k] is not None}


@functools.lru_cache(maxsize=None)
def bn_case_reference(name):
    """Train-mode float64 reference of a named case at the default momentum / eps / slope, computed once."""
    t = bn_inputs(name)
    return bn_reference(t['x'], t['gy'], t['weight'], t['bias'], t['running_mean'], t['running_var'], True, **BN_DEFAULTS)


@functools.lru_cache(maxsize=None)
def bn_case_yardstick(name):
    t = bn_inputs(name)
    return bn_yardstick(bn_case_reference(name), t['x'], t['weight'], t['bias'], t['running_mean'], t['running_var'], train=True,
                        **BN_DEFAULTS)


THREE = ((2, 6, 5, 7), (5, 6, 41, 41), (3, 6, 4, 4))      # one module, three inputs: n = 70, 8405 (two ragged slices), 48


@functools.lru_cache(maxsize=None)
def three_inputs_reference():
    """D(real) + D(fake) + one more in one graph: one set of parameters applied to three inputs in turn, the float64 running
    statistics handed from call to call (nothing is rounded in between).
    -> (parameters and starting buffers, [x], [reference of each call], running_mean, running_var after the three updates)."""
    first = bn_raw(*THREE[0], seed=2250, gykind='stats')
    rm, rv, refs, xs = first['running_mean'], first['running_var'], [], []
    for i, shape in enumerate(THREE):
        t = bn_raw(*shape, seed=2250 + i, gykind='stats')
        refs.append(bn_reference(t['x'], t['gy'], first['weight'], first['bias'], rm, rv, True, **BN_DEFAULTS))
        rm, rv = refs[-1]['running_mean'], refs[-1]['running_var']
        xs.append(t['x'])
    return first, xs, refs, rm, rv


def yardstick_bound(ref, yard_err, rel=2e-5, margin=8.0):
    """Bound on max |got - ref| where the operator itself is ill-conditioned in float32: the relative tolerance of the well-conditioned
    cases, or `margin` times what float32 torch errs on the same inputs -- the margin covers a different but equally valid
    summation order and nothing more (the rule of the SSIM edge test)."""
    return max(rel * ref.abs().max().item(), margin * yard_err)


# ------------------------------------------------------------------------------------------ BCE-with-logits criterion
# One 1024-thread workgroup strides over a (na values) and, relativistic, over b (nb values).
# name: (shape of a, shape of b or None, kind)
#   'plain'      a = 2 * randn, b = 3 * randn + 1
#   'saturated'  the same with logits +-30, +-200 and +-1e4 spread over a: float32 sigmoid is exactly 1 from about +17 and exactly 0
#                below about -104
#   'tail'       a in [-91, -89], b of mean 0: sigmoid(z) ~ 1e-39 is a float32 subnormal that only e^z / (1 + e^z) reaches
#                (exp(89) overflows float32)
CRIT_CASES = {
    'n1':            ((1, 1, 1, 1), None, 'plain'),
    'n1023':         ((1, 1, 33, 31), None, 'plain'),
    'n1024':         ((2, 1, 16, 32), None, 'plain'),
    'n1025':         ((1, 1, 25, 41), None, 'plain'),
    'n3079':         ((1, 1, 1, 3079), None, 'plain'),
    'rel_n1':        ((1, 1, 1, 1), (1, 1, 1, 1), 'plain'),
    'rel_n1023':     ((1, 1, 33, 31), (1, 1, 33, 31), 'plain'),
    'rel_n1024':     ((2, 1, 16, 32), (2, 1, 16, 32), 'plain'),
    'rel_n1025':     ((1, 1, 25, 41), (1, 1, 25, 41), 'plain'),
    'rel_n3079':     ((1, 1, 1, 3079), (1, 1, 1, 3079), 'plain'),
    'rel_nb1_na1025': ((1, 1, 25, 41), (1, 1, 1, 1), 'plain'),
    'rel_nb1025_na7': ((1, 1, 1, 7), (1, 1, 25, 41), 'plain'),
    'saturated':     ((1, 1, 25, 41), None, 'saturated'),
    'rel_saturated': ((1, 1, 25, 41), (1, 1, 7, 9), 'saturated'),
    'rel_tail':      ((1, 1, 1, 3), (1, 1, 1, 2), 'tail'),
}
CRIT_TARGETS = (1.0, 0.0, 0.9, 0.1)
SATURATED_LOGITS = (30.0, -30.0, 200.0, -200.0, 1e4, -1e4)


@functools.lru_cache(maxsize=None)
def crit_inputs(name):
    """(a, b or None), float32 CPU, made once and never written."""
    sa, sb, kind = CRIT_CASES[name]
    g = torch.Generator().manual_seed(2300 + list(CRIT_CASES).index(name))
    a = 2.0 * torch.randn(sa, generator=g)
    b = None if sb is None else 3.0 * torch.randn(sb, generator=g) + 1.0
    if kind == 'saturated':
        flat = a.view(-1)
        for k, v in enumerate(SATURATED_LOGITS):     # in the first stride of the workgroup and in its last, partial one
            flat[3 + 5 * k] = v
            flat[flat.numel() - 1 - 2 * k] = v
    elif kind == 'tail':
        a = torch.tensor([-89.0, -90.0, -91.0]).view(sa)
        b = torch.tensor([0.25, -0.25]).view(sb)
    elif kind != 'plain':
        raise ValueError(kind)
    return a, b


def crit_reference(a, b, target, g=1.0, dtype=torch.float64):
    """g * mean(BCEWithLogits(a - mean(b), target)) backward in `dtype`: dict(loss, ga, gb (None without b), z)."""
    ar = a.to(dtype).requires_grad_(True)
    br = None if b is None else b.to(dtype).requires_grad_(True)
    z = ar if br is None else ar - torch.mean(br)
    loss = F.binary_cross_entropy_with_logits(z, torch.full_like(z, target))
    loss.backward(torch.tensor(g, dtype=dtype))
    return dict(loss=loss.detach(), ga=ar.grad, gb=None if br is None else br.grad, z=z.detach())


def crit_yardstick(ref, a, b, target, g=1.0):
    f32 = crit_reference(a, b, target, g, torch.float32)
    return {k: (f32[k].double() - ref[k]).abs().max().item() for k in ('loss', 'ga', 'gb') if ref[k] is not None}


def saturation_masks(a, b):
    """(sigmoid exactly 0, sigmoid exactly 1) in float32 for z = a - mean(b), the mean taken in float64 and rounded once."""
    shift = torch.tensor(0.0) if b is None else b.double().mean().float()
    s = torch.sigmoid(a - shift)
    return s == 0, s == 1
