"""HIP conv blocks vs torch CPU float64 (exact-f32 MFMA => tight tolerance).  -m gpu"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from gpu_util import check, dev, gemm_modes

pytestmark = pytest.mark.gpu
# exact-f32 MFMA: an fmaf chain -> tight; bf16x3 split: ~2^-17 per product
TOLS = {'f32': 2e-5, 'bf16x3': 1e-4, 'bf16x2': 2e-2, 'bf16': 2e-2, 'f16fp8': 2.5e-4}   # (speed modes: tests/test_gpu_modes.py)

CASES = [
    # C1, C2, Co, k, stride, act, residual, pixel_shuffle, B, H, W
    (16, 0, 16, 3, 1, 'lrelu', False, False, 2, 12, 20),
    (64, 0, 64, 3, 1, 'relu', False, False, 1, 45, 80),
    (64, 0, 64, 3, 1, 'none', True, False, 2, 16, 40),
    (64, 64, 64, 3, 1, 'lrelu', False, False, 1, 23, 37),
    (3, 0, 64, 3, 1, 'lrelu', False, False, 2, 16, 24),
    (64, 0, 3, 3, 1, 'none', True, False, 1, 32, 48),
    (64, 0, 216, 3, 1, 'none', False, False, 1, 20, 36),
    (16, 0, 108, 3, 1, 'none', False, False, 2, 7, 9),
    (64, 0, 64, 3, 2, 'lrelu', False, False, 2, 24, 40),
    (16, 0, 16, 3, 2, 'lrelu', False, False, 1, 16, 24),
    (64, 0, 256, 3, 1, 'lrelu', False, True, 1, 12, 20),
    (16, 0, 64, 3, 1, 'lrelu', False, True, 2, 8, 12),
    (320, 0, 64, 1, 1, 'lrelu', False, False, 1, 16, 40),
    (48, 0, 16, 1, 1, 'none', False, False, 2, 12, 20),
    (32, 32, 16, 1, 1, 'lrelu', False, False, 1, 9, 33),
    (64, 64, 80, 1, 1, 'lrelu', False, False, 2, 10, 36),   # concat 1x1 on the GEMM weight-gradient path (HW % 8 == 0)
    (64, 0, 64, 3, 2, 'relu', False, False, 1, 23, 37),      # odd sizes through the zero-insert data gradient
    (64, 0, 64, 3, 2, 'lrelu', False, False, 2, 32, 48),     # stride-2 weight gradient on the bf16x3 direct-load kernel
    (16, 0, 24, 3, 2, 'none', False, False, 1, 18, 32),      # same, odd output height, Co/C not multiples of 32
    (128, 0, 128, 3, 1, 'relu', False, False, 1, 12, 36),
    (64, 0, 64, 3, 1, 'lrelu', True, False, 1, 16, 24),   # act + residual (sAtt_3 pattern)
    (32, 0, 4, 3, 1, 'lrelu', False, False, 2, 10, 72),    # thin layer (Co <= 4) on the vector-ALU weight-gradient kernel: act', ragged tile
    (16, 0, 1, 3, 1, 'none', False, False, 3, 7, 132),      # thin layer, one output channel, three column tiles
]


def _ref(x1, x2, w, b, res, stride, act, ps):
    x = x1 if x2 is None else torch.cat([x1, x2], 1)
    y = F.conv2d(x, w, b, stride=stride, padding=w.shape[-1] // 2)
    if ps:
        y = F.pixel_shuffle(y, 2)
    if act == 'relu':
        y = F.relu(y)
    elif act == 'lrelu':
        y = F.leaky_relu(y, 0.1)
    if res is not None:
        y = y + res
    return y


gemm_mode = gemm_modes()


def _at_offset(t, off, d, leaf=True):
    """`t` on the device, starting `off` floats behind a 16-byte boundary inside a larger flat buffer; leaf: it wants a gradient."""
    if t is None:
        return None
    if off:
        buf = torch.zeros(t.numel() + 8, device=d)
        assert buf.data_ptr() % 16 == 0
        v = buf[off:off + t.numel()].view(t.shape)
        v.copy_(t)
    else:
        v = t.to(d)
    return v.requires_grad_(True) if leaf else v


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_conv_block_forward_backward(case, gemm_mode, offsets=(0, 0, 0, 0)):
    """offsets: float offsets of x1, x2, the output gradient and the residual from a 16-byte boundary (tests/test_gpu_conv_ledger.py)."""
    from realvsr_amd import functional as RF
    TOL = TOLS[gemm_mode]
    C1, C2, Co, k, stride, act, use_res, ps, B, H, W = case
    g = torch.Generator().manual_seed(hash(case) % 2 ** 31)
    conv = nn.Conv2d(C1 + C2, Co, k, stride, k // 2)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (3.0 * (C1 + C2) ** 0.5))
        conv.bias.copy_(torch.randn(Co, generator=g) * 0.1)
    x1 = torch.randn(B, C1, H, W, generator=g)
    x2 = torch.randn(B, C2, H, W, generator=g) if C2 else None
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    oshape = (B, Co // 4, 2 * Ho, 2 * Wo) if ps else (B, Co, Ho, Wo)
    res = torch.randn(oshape, generator=g) if use_res else None
    gout = torch.randn(oshape, generator=g)
    if act != 'none':
        # keep the comparison away from the activation kink: where the exact pre-activation is within
        # 1e-3 of zero the derivative legitimately depends on the last bits of the GEMM
        with torch.no_grad():
            z = _ref(x1.double(), None if x2 is None else x2.double(), conv.weight.double(), conv.bias.double(), None,
                     stride, 'none', ps)
            gout = gout * (z.abs() > (1e-3 if gemm_mode in ('f32', 'bf16x3') else 5e-2)).float()   # (speed modes perturb z by ~2e-3 |z|)

    # float64 CPU reference
    r = [t.double().requires_grad_(True) if t is not None else None for t in (x1, x2, res)]
    wr, br = conv.weight.detach().double().requires_grad_(True), conv.bias.detach().double().requires_grad_(True)
    yr = _ref(r[0], r[1], wr, br, r[2], stride, act, ps)
    yr.backward(gout.double())

    d = dev()
    conv = conv.to(d)
    t = [_at_offset(v, off, d) for v, off in zip((x1, x2, res), (offsets[0], offsets[1], offsets[3]))]
    code = {'none': RF.ACT_NONE, 'relu': RF.ACT_RELU, 'lrelu': RF.ACT_LRELU}[act]
    y = RF.conv2d(t[0], conv, code, 0.1, x2=t[1], residual=t[2], pixel_shuffle=ps)
    y.backward(_at_offset(gout, offsets[2], d, leaf=False))
    torch.cuda.synchronize()
    check('out', y, yr, TOL)
    check('grad_x1', t[0].grad, r[0].grad, TOL)
    if C2:
        check('grad_x2', t[1].grad, r[1].grad, TOL)
    if use_res:
        check('grad_res', t[2].grad, r[2].grad, TOL)
    check('grad_weight', conv.weight.grad, wr.grad, TOL)
    check('grad_bias', conv.bias.grad, br.grad, TOL)


def _random_cases(n, seed):
    """Seeded sweep over the shapes the buffer-addressed staging has to get right: channel counts that leave partial octets /
    chunks, concat inputs on and off the 16 / 64-channel boundaries, widths on and off the vector path, ragged tiles."""
    import random
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        k = rnd.choice([3, 3, 3, 1])
        C1 = rnd.choice([3, 8, 9, 16, 24, 40, 64, 72])
        C2 = rnd.choice([0, 0, 0, 16, 64]) if C1 % 8 == 0 else 0
        Co = rnd.choice([1, 3, 4, 12, 32, 64, 80, 216]) if k == 3 else rnd.choice([16, 64])
        ps = k == 3 and Co % 4 == 0 and Co >= 32 and rnd.random() < 0.25
        act = rnd.choice(['none', 'relu', 'lrelu'])
        use_res = (not ps) and rnd.random() < 0.3
        H = rnd.choice([5, 8, 13, 16, 18, 33])
        W = rnd.choice([8, 12, 20, 36, 68, 30])   # 30: off the vector path
        out.append((C1, C2, Co, k, 1, act, use_res, ps, rnd.choice([1, 2, 3]), H, W))
    return out


@pytest.mark.parametrize('case', _random_cases(36, 20260928), ids=lambda c: '-'.join(str(v) for v in c))
def test_conv_random_shapes(case, gemm_mode):
    test_conv_block_forward_backward(case, gemm_mode)


def test_conv_refuses_cpu_tensors():
    from realvsr_amd import functional as RF
    conv = nn.Conv2d(4, 4, 3, 1, 1)
    with pytest.raises(NotImplementedError):
        RF.conv2d(torch.randn(1, 4, 8, 8), conv)


def test_conv_wgrad_is_deterministic():
    from realvsr_amd import functional as RF
    d = dev()
    torch.manual_seed(0)
    conv = nn.Conv2d(64, 64, 3, 1, 1).to(d)
    x = torch.randn(4, 64, 45, 80, device=d)
    grads = []
    for _ in range(2):
        conv.zero_grad()
        RF.conv2d(x, conv, RF.ACT_LRELU).square().sum().backward()
        grads.append(conv.weight.grad.clone())
    assert torch.equal(grads[0], grads[1])


# ---- refusals of the plan (csrc/conv_plan.h), straight through the C ABI: nothing may be launched
SENTINEL = -12345.0


def _raw_conv(x, w, bias, res, out, w_mode, act, slope=0.1):
    """rvsr_conv2d_forward on a single-input 3x3 / stride-1 conv; returns (code, message)."""
    from realvsr_amd import _lib
    from realvsr_amd._lib import _p, _stream
    L = _lib.lib()
    B, C, H, W = x.shape
    Co = out.shape[1]
    ws = torch.empty(L.rvsr_conv2d_forward_workspace_bytes(C, 0, Co, 3), dtype=torch.uint8, device=x.device)
    rc = L.rvsr_conv2d_forward(_p(x), C, None, 0, None, 0.0, 0, H, W, _p(w), _p(bias), _p(res), _p(out), Co, None, 0, B, 3, 1, w_mode, act,
                               slope, 0, H, W, _p(ws), ws.numel(), _stream())
    torch.cuda.synchronize()
    return rc, (L.rvsr_last_error() or b'').decode()


@pytest.fixture
def bf16x3_mode():
    from realvsr_amd import _lib
    old = _lib.get_gemm_mode()
    _lib.set_gemm_mode('bf16x3')
    yield
    _lib.set_gemm_mode(old)


def test_f16fp8_flag_on_an_ineligible_conv_is_refused(bf16x3_mode):
    """w_mode | 4 on a conv with 32 output channels: RVSR_ERR_UNSUPPORTED with a message that names the format, and no kernel runs
    (before the plan the call fell through to the exact-f32 kernel and returned RVSR_OK)."""
    d = dev()
    g = torch.Generator().manual_seed(5)
    x, w, b = (torch.randn(s, generator=g).to(d) for s in ((1, 16, 8, 8), (32, 16, 3, 3), (32,)))
    out = torch.full((1, 32, 8, 8), SENTINEL, device=d)
    rc, msg = _raw_conv(x, w, b, None, out, 4, 0)
    assert rc == 1 and 'f16 + fp8' in msg, (rc, msg)
    assert bool((out == SENTINEL).all())


def test_mask_epilogue_refused_or_exact(bf16x3_mode):
    """act 3 (out = (conv + bias) * (residual > 0 ? 1 : slope)): refused without a message and without touching the output on a frame the
    8 x 64 tile does not take (16 x 24); computed on one it takes (8 x 64)."""
    d = dev()
    g = torch.Generator().manual_seed(6)
    w, b = torch.randn(64, 64, 3, 3, generator=g) / 72.0, torch.randn(64, generator=g) * 0.1
    for H, W, taken in ((16, 24, False), (8, 64, True)):
        x, res = torch.randn(1, 64, H, W, generator=g), torch.randn(1, 64, H, W, generator=g)
        out = torch.full((1, 64, H, W), SENTINEL, device=d)
        rc, msg = _raw_conv(x.to(d), w.to(d), b.to(d), res.to(d), out, 0, 3, 0.1)
        if not taken:
            assert rc == 1 and msg == '', (rc, msg)
            assert bool((out == SENTINEL).all())
        else:
            assert rc == 0, (rc, msg)
            ref = F.conv2d(x.double(), w.double(), b.double(), padding=1) * torch.where(res.double() > 0, 1.0, 0.1)
            check('masked data gradient', out, ref, TOLS['bf16x3'])


# ---- what only the raw C ABI reaches: an output buffer off a 16-byte boundary, act' on a strided or 5x5 forward conv, the mask epilogue
# with act' in the speed modes.  Calls as tests/conv_ledger.py describes them (the coverage ledger, tests/test_conv_ledger_host.py,
# takes its raw-ABI keys from RAW_LEDGER_CALLS); every tensor sits inside a larger buffer of sentinels that must stay untouched.
def _raw_ledger_calls():
    from conv_ledger import fwd_call
    return [
        ('out+res off', fwd_call(64, 64, 8, 64, 8, 64, 1, res=True, res_off=1, out_off=1)),   # W % 4 == 0: element stores by alignment alone
        ('act s2 Co64', fwd_call(64, 64, 16, 32, 8, 16, 1, stride=2, xact=True)),
        ('act s2 Co16', fwd_call(16, 16, 9, 30, 5, 15, 2, stride=2, xact=True)),
        ('act 5x5', fwd_call(16, 16, 9, 30, 9, 30, 1, k=5, xact=True)),
        ('ps view, out off', fwd_call(64, 16, 16, 32, 8, 16, 1, in_mode=2, w_mode=1, xact=True, out_off=1)),
        ('zero-insert view, out off', fwd_call(64, 64, 8, 16, 16, 32, 1, in_mode=1, w_mode=1, out_off=1)),
    ]


RAW_LEDGER_CALLS = _raw_ledger_calls()
_PAD = 32   # floats of sentinel on either side (a multiple of 4: the tensor's own offset decides its alignment)


def _padded(t, off, d):
    """(buffer, view): `t` at `off` floats behind a 16-byte boundary, sentinels around it."""
    buf = torch.full((t.numel() + 2 * _PAD + 4,), SENTINEL, device=d)
    assert buf.data_ptr() % 16 == 0
    v = buf[_PAD + off:_PAD + off + t.numel()].view(t.shape)
    v.copy_(t)
    return buf, v


def _border_untouched(buf, off, n):
    return bool((buf[:_PAD + off] == SENTINEL).all()) and bool((buf[_PAD + off + n:] == SENTINEL).all())


def _raw_call(call, seed, slope=0.1):
    """Runs one single-input, single-output rvsr_conv2d_forward call on seeded tensors; returns (code, message, output, float64
    reference, borders untouched)."""
    from realvsr_amd import _lib
    from realvsr_amd._lib import _p, _stream
    c = call
    assert c['C2'] == 0 and c['Co2'] == 0 and not c['ps']
    L, d = _lib.lib(), dev()
    g = torch.Generator().manual_seed(seed)
    B, C, Co, k, T = c['B'], c['C1'], c['Co1'], c['k'], c['k'] ** 2
    x = torch.randn(B, C // 4 if c['in_mode'] == 2 else C, c['Hs'], c['Ws'], generator=g)
    xact = torch.randn(x.shape, generator=g) if c['xact'] else None
    w = torch.randn((C, Co, k, k) if c['w_mode'] & 1 else (Co, C, k, k), generator=g) / (T * C) ** 0.5
    bias = torch.randn(Co, generator=g) * 0.1
    res = torch.randn(B, Co, c['Hout'], c['Wout'], generator=g) if c['res'] else None

    xin = x.double() if xact is None else x.double() * torch.where(xact.double() > 0, 1.0, slope)
    if c['in_mode'] == 2:       # stored pixel-shuffled
        xin = F.pixel_unshuffle(xin, 2)
    elif c['in_mode'] == 1:     # the zero-insert view of a stride-2 data gradient
        z = torch.zeros(B, C, c['Hout'], c['Wout'], dtype=torch.float64)
        z[:, :, 0:2 * c['Hs']:2, 0:2 * c['Ws']:2] = xin
        xin = z
    weff = w.double().transpose(0, 1).flip(2, 3) if c['w_mode'] & 1 else w.double()
    ref = F.conv2d(xin, weff, bias.double(), stride=c['stride'], padding=k // 2)
    if c['act'] == 3:
        ref = ref * torch.where(res.double() > 0, 1.0, slope)
    else:
        ref = F.leaky_relu(ref, slope) if c['act'] == 2 else F.relu(ref) if c['act'] == 1 else ref
        ref = ref if res is None else ref + res.double()

    xb, xv = _padded(x, c['x_off'], d)
    ab, av = _padded(xact, c['xact_off'], d) if c['xact'] else (None, None)
    rb, rv = _padded(res, c['res_off'], d) if c['res'] else (None, None)
    ob, ov = _padded(torch.full(tuple(ref.shape), SENTINEL), c['out_off'], d)
    wd, bd = w.to(d), bias.to(d)
    ws = torch.empty(L.rvsr_conv2d_forward_workspace_bytes(C, 0, Co, k), dtype=torch.uint8, device=d)
    rc = L.rvsr_conv2d_forward(_p(xv), C, None, 0, _p(av), slope, c['in_mode'], c['Hs'], c['Ws'], _p(wd), _p(bd), _p(rv), _p(ov), Co, None, 0, B, k,
                               c['stride'], c['w_mode'], c['act'], slope, 0, c['Hout'], c['Wout'], _p(ws), ws.numel(), _stream())
    torch.cuda.synchronize()
    clean = _border_untouched(ob, c['out_off'], ov.numel()) and _border_untouched(xb, c['x_off'], xv.numel()) and \
        (rb is None or _border_untouched(rb, c['res_off'], rv.numel())) and (ab is None or _border_untouched(ab, c['xact_off'], av.numel()))
    return rc, (L.rvsr_last_error() or b'').decode(), ov, ref, clean


@pytest.mark.parametrize('name,call', RAW_LEDGER_CALLS, ids=[n.replace(' ', '_') for n, _ in RAW_LEDGER_CALLS])
def test_raw_abi_calls_vs_float64(name, call, gemm_mode):
    rc, msg, out, ref, clean = _raw_call(call, 11)
    assert rc == 0, (rc, msg)
    assert clean, 'a store outside the output (or into an input)'
    check(name, out, ref, TOLS[gemm_mode])


@pytest.mark.parametrize('mode', ['bf16x2', 'bf16'])
def test_mask_epilogue_with_act_in_in_the_speed_modes(mode):
    """act 3 with act' on the input, two terms and one term per product, on a frame the 8 x 64 tile takes with a ragged last row and a
    ragged last column tile (17 x 60)."""
    from conv_ledger import fwd_call, fwd_plan
    from realvsr_amd import _lib
    call = fwd_call(64, 64, 17, 60, 17, 60, 1, w_mode=1, act=3, res=True, xact=True)
    rc, row = fwd_plan(call, mode)
    assert rc == 0 and (row['wide'], row['NT'], row['act_in']) == (1, 2 if mode == 'bf16x2' else 1, 1), row
    old = _lib.get_gemm_mode()
    _lib.set_gemm_mode(mode)
    try:
        rc, msg, out, ref, clean = _raw_call(call, 12)
    finally:
        _lib.set_gemm_mode(old)
    assert rc == 0, (rc, msg)
    assert clean
    check('masked data gradient with act\', ' + mode, out, ref, TOLS[mode])
