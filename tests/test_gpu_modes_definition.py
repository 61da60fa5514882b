"""The reduced-term GEMM modes held to their DEFINITION, bit for bit, in every kernel they act in (include/realvsr_hip.h, the comment on
rvsr_set_gemm_mode: 'bf16x2' = mode 0 on bf16-rounded weights -- in a weight gradient the output gradient is the operand rounded --, 'bf16'
rounds both operands; conv_fwd5 forward and data gradient, conv_wgrad2, conv_wgrad5, dcn_fwd3, dcn_bwdin6, dcn_bwdw4, dcn_bwdw6; every
other kernel keeps three terms).  -m gpu

Every kernel accumulates hi*hi, then hi*lo, then lo*hi into one f32 accumulator (conv2_kernels.hip: conv_fwd5 1002-1015, wg2_row 1248-1255,
conv_wgrad5 2021-2023; dcn3_kernels.hip 297-301; dcn6_kernels.hip 457-459, 570-572, 1024-1026; dcn_bwdw4.inc 254-256).  A bf16 x bf16 product
is exact in f32 and an operand that already is a bf16 value has lo == 0 (tests/test_modes_reference_host.py), so

    speed mode on the original tensors  ==  'bf16x3' on the pre-rounded ones        (torch.equal, no tolerance)

and a single wrong, missing or stale product shows.  Each case also asks the exported plan for the term count of the kernel it runs
(rvsr_conv2d_forward_plan's NT, rvsr_dcn_pack_*_plan; a weight gradient's family comes from rvsr_conv2d_backward_weight_plan and its term
count is the mode's: rvsr_launch_conv_wgrad2 / rvsr_launch_conv_wgrad5 read rvsr_gemm_terms()) and asserts that the speed-mode result is
NOT the three-term result on the original tensors.  Where the plan says three terms (scalar-staged views, 32-row m-blocks, exact-f32
fallbacks, first-generation DCN kernels) the same case asserts the opposite: the default mode's bits.

Which operand is pre-rounded (second column: 'bf16x2'; third: additionally in 'bf16'):
    conv_fwd5 forward          weight              x, x2                out, with the case's activation / residual / PixelShuffle epilogue
    conv_fwd5 data gradient    weight              output gradient      grad_x, grad_x2
    conv_wgrad2 / conv_wgrad5  output gradient     x, x2                grad_weight
    dcn_fwd3                   weight              x (*)                out
    dcn_bwdin6                 weight              output gradient      grad_offset, grad_mask bit for bit; grad_input bounded (below)
    dcn_bwdw6 / dcn_bwdw4      output gradient     x (*)                grad_weight, grad_bias
(*) the kernel forms the operand itself, mask * bilinear(x): a bf16 value for bf16 x at integer sample positions and masks in {1, 1/2, 1/4}
(tests/modes_reference.py), so the 'bf16' rows of the DCN use those fields and the 'bf16x2' rows random fractional offsets.  The backward
of one call is compared against TWO reference runs, because its two gradient kernels drop the lo part of different operands; dcn_bwdin6
multiplies col_grad with values of the UNROUNDED x (dcn6_kernels.hip:545-552), so its 'bf16' reference keeps x as it is.  Gradients that
depend on forward state are taken with ACT_NONE (an activation mask from a forward on rounded weights is another mask); the ReLU case
through the raw ABI hands the same activation tensor to both runs.

Bias gradients.  conv_wgrad2 and conv_wgrad5 SUM the f32 output gradient (conv2_kernels.hip:1431 and 1999-2003): grad_bias is the default
mode's on the unrounded output gradient.  dcn_bwdw6 and dcn_bwdw4 get it as a PRODUCT with a ones column through the same matrix
instructions (dcn6_kernels.hip:1003 with 1023-1026; dcn_bwdw4.inc:37 with 254-256 and 281): grad_bias is the three-term kernel's on the
ROUNDED output gradient.

grad_input of the DCN is an atomic scatter and not reproducible run to run: it is compared with the reference run in relative L2 and in
max |a - b| / max |b|, bounded by four times the largest spread of the 'bf16x3' reference against ITSELF over five runs on the rounded
operands (GX_SPREAD below: measured per case on the MI355X; atomic-order noise is heavy-tailed, tests/test_gpu_dist.py uses the same
factor).  In dcn_bwdin6 the scatter passes a fixed-point window whose scale S = 927407 / (1.002 * Wn * Gn) (dcn6_kernels.hip, "fixed-point
scale of this chunk") comes from the column norms of the weights and the pixel norms of the output gradient.  This test found those taken
from the UNROUNDED tensors in the speed modes: the quantisation grid then differed from the reference run's by ~1e-3 of its step and
grad_input sat 2.5e-5 ('bf16x2') / 8e-6 ('bf16') in L2 from the three-term kernel on the rounded operands, a hundred times the run-to-run
spread.  The norms are now those of the operands the products see (dcn_bwd5_wnorm_kernel's hi_only, the kernel's gsq with one term), every
fixed-point contribution is the reference run's, and what is left is the summation order of the float atomics at the flush."""
import pytest
import torch
import torch.nn as nn

import conv_ledger as CL
import dcn_ledger as DL
import modes_reference as MR
from conftest import rel_err
from gpu_util import dev, l2_err

pytestmark = pytest.mark.gpu

TERMS = {'bf16x2': 2, 'bf16': 1}
R = MR.bf16_round

# grad_input: the largest distance between two of five 'bf16x3' runs on the rounded operands, (relative L2, max |a - b| / max |b|), measured
# on the MI355X over the cases of _dcn_cases() in both modes (the larger of two measurements) -- per kernel; cases of one workgroup tile
# per image measured 0:
#     dcn_bwdin6<4>: 2-64-64-8-20-36 9.6e-9 / 6.3e-8, 1-32-40-4-9-33 1.8e-9 / 3.1e-8, 1-64-64-8-24-40 (3 px) 1.5e-8 / 1.2e-7, (6 px) 3.4e-8 / 1.1e-7,
#                    1-64-64-8-9-33 3.9e-9 / 7.3e-8;   dcn_bwdin6<8>: 1-128-128-8-12-40 6.0e-9 / 5.4e-8, 1-128-128-8-17-40 1.8e-8 / 1.5e-7;
#     dcn_bwdin6<1>: 2-16-16-2-9-33 6.3e-9 / 3.4e-8;   dcn_bwd_input_kernel: 2-8-64-2-9-20 3.7e-8 / 9.1e-8, 2-32-128-8-6-20 6.8e-8 / 1.8e-7,
#                    2-32-64-8-6-33 5.2e-8 / 1.2e-7, 1-8-130-1-8-32 8.8e-8 / 1.5e-7, 2-16-130-2-9-36 6.2e-8 / 1.1e-7;
#     the generic path (5 x 5 kernel of the scope test): 1.96e-7 / 4.4e-7.
# The bounds are four times the largest of the fused kernels and of the generic path.  (The speed modes measured against the reference run:
# at most 6.6e-8 / 1.3e-7 on the fused kernels -- and 2.5e-5 / 2.4e-5 before dcn_bwdin6 took its scale from the rounded operands.)
GX_SPREAD = {'fused': (8.9e-8, 1.9e-7), 'generic': (1.96e-7, 4.5e-7)}
GX_BOUND = {k: (4 * v[0], 4 * v[1]) for k, v in GX_SPREAD.items()}


@pytest.fixture(params=['bf16x2', 'bf16'])
def speed_mode(request):
    from realvsr_amd import _lib
    old = _lib.get_gemm_mode()
    yield request.param
    _lib.set_gemm_mode(old)


class _mode:
    """The GEMM mode of the calls inside; the caller's mode comes back whatever happens."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from realvsr_amd import _lib
        self.old = _lib.get_gemm_mode()
        _lib.set_gemm_mode(self.mode)

    def __exit__(self, *exc):
        from realvsr_amd import _lib
        _lib.set_gemm_mode(self.old)


def _same(name, a, b):
    assert torch.equal(a, b), '%s: not bit-identical, %d of %d elements differ, max |a - b| %.3e' % (
        name, int((a != b).sum()), a.numel(), float((a - b).abs().max()))


def _differs(name, a, b):
    assert not torch.equal(a, b), '%s: the speed mode gave the three-term result on the original operands -- the reduced kernel did not run' % name


def _seed(*ints):
    return sum((i + 1) * int(v) for i, v in enumerate(ints)) % (2 ** 31)


# ------------------------------------------------------------------------------------------------------------------------------------
# conv_fwd5 (forward, data gradient) and conv_wgrad2 on the cases the speed-mode sweeps of tests/test_gpu_modes.py select
def _conv_cases():
    from test_gpu_modes import _speed_mode_conv_cases, _speed_mode_ledger_cases
    return [(c, (0, 0, 0, 0)) for c in _speed_mode_conv_cases()] + list(_speed_mode_ledger_cases())


def _conv_id(v):
    return '-'.join(str(x) for x in v[0]) + ('' if not any(v[1]) else '+' + ''.join(str(o) for o in v[1]))


def _conv_run(mode, case, offsets, act, w, b, x1, x2, res, gout=None):
    """One conv2d() node of the block `case` in `mode` on a FRESH module holding (w, b) -- no packed weight image of an earlier run can
    serve this one --, tensors at the case's pointer offsets; with `gout` also its backward.  Returns the outputs by name."""
    from realvsr_amd import functional as RF
    from test_gpu_conv import _at_offset
    C1, C2, Co, k, stride, _, _, ps, B, H, W = case
    d = dev()
    conv = nn.Conv2d(C1 + C2, Co, k, stride, k // 2).to(d)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    RF.invalidate_weight_cache()
    t = [_at_offset(v, off, d) for v, off in zip((x1, x2, res), (offsets[0], offsets[1], offsets[3]))]
    with _mode(mode):
        y = RF.conv2d(t[0], conv, CL.ACT[act], 0.1, x2=t[1], residual=t[2], pixel_shuffle=ps)
        if gout is not None:
            y.backward(_at_offset(gout, offsets[2], d, leaf=False))
        torch.cuda.synchronize()
    got = {'out': y.detach().clone()}
    if gout is not None:
        got.update(grad_x=t[0].grad, grad_x2=None if t[1] is None else t[1].grad, grad_weight=conv.weight.grad, grad_bias=conv.bias.grad)
    return got


def _conv_tensors(case):
    C1, C2, Co, k, stride, act, use_res, ps, B, H, W = case
    g = torch.Generator().manual_seed(_seed(C1, C2, Co, k, stride, B, H, W))
    w = torch.randn(Co, C1 + C2, k, k, generator=g) / (k * (C1 + C2) ** 0.5)
    b = torch.randn(Co, generator=g) * 0.1
    x1 = torch.randn(B, C1, H, W, generator=g)
    x2 = torch.randn(B, C2, H, W, generator=g) if C2 else None
    Ho, Wo = CL.out_size(H, W, k, stride)
    oshape = (B, Co // 4, 2 * Ho, 2 * Wo) if ps else (B, Co, Ho, Wo)
    res = torch.randn(oshape, generator=g) if use_res else None
    gout = torch.randn(oshape, generator=g)
    return w, b, x1, x2, res, gout


def _conv_plans(case, offsets, mode):
    """(forward NT, data-gradient NT, weight-gradient family) of the calls conv2d() issues for the block: the forward with the case's
    activation, the backward with ACT_NONE (tests/conv_ledger.py; its drift guard compares these calls with functional.py's)."""
    fwd = dict(CL.calls_of(case, offsets, mode))['forward']
    bwd = dict(CL.calls_of(case[:5] + ('none',) + case[6:], offsets, mode))
    rows = []
    for call in (fwd, bwd['dgrad']):
        rc, row = CL.fwd_plan(call, mode)
        assert rc == 0, (call, rc)
        rows.append(row['NT'] if CL.FWD_FAMILY[row['family']] == 'fwd5' else 3)
    rc, wrow = CL.wgrad_plan(bwd['wgrad'], mode)
    assert rc == 0, (bwd['wgrad'], rc)
    return rows[0], rows[1], CL.WGRAD_FAMILY[wrow['family']]


def _check_conv_block(case, offsets, mode, reduced_wgrad=('wgrad2', 'wgrad5')):
    """The identities of one block in one speed mode.  Returns what ran reduced: (forward, data gradient, weight gradient)."""
    nt = TERMS[mode]
    C1, C2, Co, k, stride, act, use_res, ps, B, H, W = case
    nt_f, nt_d, wfam = _conv_plans(case, offsets, mode)
    assert nt_f in (nt, 3) and nt_d in (nt, 3), (nt_f, nt_d)
    w, b, x1, x2, res, gout = _conv_tensors(case)
    both = mode == 'bf16'
    xr1, xr2 = (R(x1), None if x2 is None else R(x2)) if both else (x1, x2)
    tag = '%s %s ' % (mode, _conv_id((case, offsets)))

    # ---- forward, with every epilogue of the case
    with torch.no_grad():
        got = _conv_run(mode, case, offsets, act, w, b, x1, x2, res)['out']
        plain = _conv_run('bf16x3', case, offsets, act, w, b, x1, x2, res)['out']
        if nt_f == nt:
            ref = _conv_run('bf16x3', case, offsets, act, R(w), b, xr1, xr2, res)['out']
            _same(tag + 'out (NT %d)' % nt_f, got, ref)
            _differs(tag + 'out', got, plain)
        else:
            _same(tag + 'out (three terms by the plan)', got, plain)

    # ---- backward without an activation: the data gradient drops the weights' lo part, the weight gradient the output gradient's
    none = case[:5] + ('none',) + case[6:]
    got = _conv_run(mode, none, offsets, 'none', w, b, x1, x2, res, gout)
    plain = _conv_run('bf16x3', none, offsets, 'none', w, b, x1, x2, res, gout)
    names = ['grad_x'] + (['grad_x2'] if C2 else [])
    if nt_d == nt:
        ref = _conv_run('bf16x3', none, offsets, 'none', R(w), b, x1, x2, res, R(gout) if both else gout)
        for n in names:
            _same(tag + n + ' (NT %d)' % nt_d, got[n], ref[n])
        _differs(tag + 'grad_x', got['grad_x'], plain['grad_x'])
    else:
        for n in names:
            _same(tag + n + ' (three terms by the plan)', got[n], plain[n])
    if wfam in reduced_wgrad:
        ref = _conv_run('bf16x3', none, offsets, 'none', w, b, xr1, xr2, res, R(gout))
        _same(tag + 'grad_weight (%s)' % wfam, got['grad_weight'], ref['grad_weight'])
        _differs(tag + 'grad_weight', got['grad_weight'], plain['grad_weight'])
    else:
        assert wfam not in ('wgrad2', 'wgrad5'), wfam
        _same(tag + 'grad_weight (%s: every split mode alike)' % wfam, got['grad_weight'], plain['grad_weight'])
    # a sum of the f32 output gradient in conv_wgrad2 (conv2_kernels.hip:1431) and conv_wgrad5 (:1999-2003), not a product
    _same(tag + 'grad_bias', got['grad_bias'], plain['grad_bias'])
    return nt_f == nt, nt_d == nt, wfam in reduced_wgrad


@pytest.mark.parametrize('case', _conv_cases(), ids=_conv_id)
def test_conv_block_is_the_three_term_kernel_on_rounded_operands(case, speed_mode):
    _check_conv_block(case[0], case[1], speed_mode)


def test_the_conv_cases_reach_every_reduced_conv_kernel(speed_mode):
    """By the plans alone: the list above holds, per mode, reduced conv_fwd5 forwards on the 16 x 32 and the 8 x 64 tile with the residual,
    PixelShuffle and plain epilogues and a concatenated input, reduced data gradients through the plain and the pixel-unshuffle view and with
    a split output, and conv_wgrad2 with a concatenated input and a pixel-shuffled output gradient."""
    nt = TERMS[speed_mode]
    seen = set()
    for case, offsets in _conv_cases():
        fwd = dict(CL.calls_of(case, offsets, speed_mode))['forward']
        bwd = dict(CL.calls_of(case[:5] + ('none',) + case[6:], offsets, speed_mode))
        frow, drow = CL.fwd_plan(fwd, speed_mode)[1], CL.fwd_plan(bwd['dgrad'], speed_mode)[1]
        wfam = CL.WGRAD_FAMILY[CL.wgrad_plan(bwd['wgrad'], speed_mode)[1]['family']]
        if CL.FWD_FAMILY[frow['family']] == 'fwd5' and frow['NT'] == nt:
            seen |= {('fwd', 'wide', frow['wide']), ('fwd', CL.epilogue_of(fwd)), ('fwd', 'x2', fwd['C2'] > 0)}
        if CL.FWD_FAMILY[drow['family']] == 'fwd5' and drow['NT'] == nt:
            seen |= {('dgrad', 'vec', drow['vec']), ('dgrad', 'split', bwd['dgrad']['Co2'] > 0)}
        if wfam == 'wgrad2':
            seen |= {('wgrad2', 'x2', bwd['wgrad']['C2'] > 0), ('wgrad2', 'g_mode', bwd['wgrad']['g_mode'])}
    want = {('fwd', 'wide', 0), ('fwd', 'wide', 1), ('fwd', 'plain'), ('fwd', 'residual'), ('fwd', 'pixel-shuffle'), ('fwd', 'x2', True),
            ('dgrad', 'vec', 1), ('dgrad', 'vec', 2), ('dgrad', 'split', True), ('wgrad2', 'x2', True), ('wgrad2', 'g_mode', 2)}
    assert want <= seen, sorted(want - seen)


# ---- ReLU through the raw ABI: act' = 0 / 1 keeps the products exact, the SAME activation tensor goes to both runs
def _raw_dgrad(mode, gout, act_out, w):
    """rvsr_conv2d_forward as the data gradient of a 3x3 / stride-1 conv with weight w (Co, C, 3, 3): input gout x relu'(act_out)."""
    from realvsr_amd import _lib
    from realvsr_amd._lib import _p, _stream
    L, d = _lib.lib(), dev()
    B, Co, H, W = gout.shape
    C = w.shape[1]
    g, a, wd = gout.to(d), act_out.to(d), w.to(d)
    out = torch.full((B, C, H, W), -12345.0, device=d)
    ws = torch.empty(L.rvsr_conv2d_forward_workspace_bytes(Co, 0, C, 3), dtype=torch.uint8, device=d)
    with _mode(mode):
        rc = L.rvsr_conv2d_forward(_p(g), Co, None, 0, _p(a), 0.0, 0, H, W, _p(wd), None, None, _p(out), C, None, 0, B, 3, 1, 1, 0, 0.0, 0, H, W,
                                   _p(ws), ws.numel(), _stream())
        torch.cuda.synchronize()
    assert rc == 0, (rc, L.rvsr_last_error())
    return out


def _raw_wgrad(mode, x, gout, act_out):
    """rvsr_conv2d_backward_weight of that conv: (grad_weight, grad_bias) from x and gout x relu'(act_out)."""
    from realvsr_amd import _lib
    from realvsr_amd._lib import _p, _stream
    L, d = _lib.lib(), dev()
    B, C, H, W = x.shape
    Co = gout.shape[1]
    xd, g, a = x.to(d), gout.to(d), act_out.to(d)
    gw, gb = torch.full((Co, C, 3, 3), -12345.0, device=d), torch.full((Co,), -12345.0, device=d)
    ws = torch.empty(L.rvsr_conv2d_wgrad_workspace_bytes(C, 0, Co, B, 3, 1, H, W), dtype=torch.uint8, device=d)
    with _mode(mode):
        rc = L.rvsr_conv2d_backward_weight(_p(xd), C, None, 0, H, W, _p(g), _p(a), 0.0, 0, H, W, _p(gw), _p(gb), Co, B, 3, 1, H, W, 0,
                                           _p(ws), ws.numel(), _stream())
        torch.cuda.synchronize()
    assert rc == 0, (rc, L.rvsr_last_error())
    return gw, gb


def test_relu_gradients_through_the_raw_abi(speed_mode):
    """Data and weight gradient of a 64 -> 64 conv behind a ReLU on a 17 x 60 frame (ragged last row and last column tile, the 8 x 64
    tile): act' fused into the load of the output gradient in both kernels."""
    nt, both = TERMS[speed_mode], speed_mode == 'bf16'
    B, C, Co, H, W = 2, 64, 64, 17, 60
    rc, row = CL.fwd_plan(CL.fwd_call(Co, C, H, W, H, W, B, w_mode=1, xact=True), speed_mode)
    assert rc == 0 and (CL.FWD_FAMILY[row['family']], row['NT'], row['act_in']) == ('fwd5', nt, 1), row
    rc, wrow = CL.wgrad_plan(CL.wgrad_call(C, Co, H, W, H, W, B, gact=True), speed_mode)
    assert rc == 0 and CL.WGRAD_FAMILY[wrow['family']] == 'wgrad2', wrow
    g = torch.Generator().manual_seed(_seed(B, C, Co, H, W))
    w = torch.randn(Co, C, 3, 3, generator=g) / (3 * C ** 0.5)
    x, gout = torch.randn(B, C, H, W, generator=g), torch.randn(B, Co, H, W, generator=g)
    act_out = torch.relu(torch.randn(B, Co, H, W, generator=g))
    got = _raw_dgrad(speed_mode, gout, act_out, w)
    _same(speed_mode + ' raw grad_x', got, _raw_dgrad('bf16x3', R(gout) if both else gout, act_out, R(w)))
    _differs(speed_mode + ' raw grad_x', got, _raw_dgrad('bf16x3', gout, act_out, w))
    gw, gb = _raw_wgrad(speed_mode, x, gout, act_out)
    gw_r, _ = _raw_wgrad('bf16x3', R(x) if both else x, R(gout), act_out)
    gw_3, gb_3 = _raw_wgrad('bf16x3', x, gout, act_out)
    _same(speed_mode + ' raw grad_weight', gw, gw_r)
    _differs(speed_mode + ' raw grad_weight', gw, gw_3)
    _same(speed_mode + ' raw grad_bias (conv2_kernels.hip:1431: a sum of gout x act\', not a product)', gb, gb_3)


# ------------------------------------------------------------------------------------------------------------------------------------
# conv_wgrad5_kernel<STRIDE, NT>: the 5x5 weight gradient of the patch discriminator's layers (first, inner, last), strides 1 and 2.
# Frames: 5 x 9, 8 x 32 and 9 x 33 (one ragged 4 x 32 tile, whole tiles, ragged in both directions) as the input -- and at stride 2 also
# as the OUTPUT, the frame the kernel tiles.  The forward and the data gradient of these convs keep three terms.
WGRAD5_CASES = [(ci, co, stride, h, w) for ci, co in ((3, 64), (64, 64), (64, 1)) for stride, frames in
                ((1, ((5, 9), (8, 32), (9, 33))), (2, ((5, 9), (8, 32), (9, 33), (10, 18), (16, 64), (17, 65)))) for h, w in frames]


@pytest.mark.parametrize('case', WGRAD5_CASES, ids=lambda c: '%d-%d-s%d-%dx%d' % c)
def test_conv_wgrad5_is_the_three_term_kernel_on_rounded_operands(case, speed_mode):
    ci, co, stride, H, W = case
    block = (ci, 0, co, 5, stride, 'none', False, False, 2, H, W)
    assert _conv_plans(block, (0, 0, 0, 0), speed_mode) == (3, 3, 'wgrad5')
    assert _check_conv_block(block, (0, 0, 0, 0), speed_mode) == (False, False, True)


# ------------------------------------------------------------------------------------------------------------------------------------
# dcn_fwd3, dcn_bwdin6, dcn_bwdw6 / dcn_bwdw4 through modulated_deform_conv (the mask is an argument)
def _dcn_cases():
    from test_gpu_modes import _speed_mode_dcn_cases
    cases = [s[:6] + (s[9], s[10]) for s in _speed_mode_dcn_cases() if s[4] <= 24 and s[5] <= 40]
    return cases + [
        # B, C, Co, dg, H, W, offset std, bias
        (1, 64, 64, 8, 9, 33, 2.0, True),      # W = 33 at NK = 4 (the list above has 32 -> 40 at 9 x 33 and 64 -> 80, two output-channel passes)
        (2, 64, 80, 8, 9, 20, 6.0, True),      # 80 output channels, two batch elements, large offsets (NK = 8: the 8 px window)
        (2, 16, 16, 2, 9, 33, 2.0, True),      # C_out <= 32: forward and input gradient keep three terms, the weight gradient is reduced
        # 130 output channels: beyond dcn_bwdin6 (and with it dcn_bwdw6), the weight gradient is dcn_bwdw4 -- one chunk, then two chunks,
        # two batch elements and a ragged last tile row
        (1, 8, 130, 1, 8, 32, 1.0, True),
        (2, 16, 130, 2, 9, 36, 2.0, True),
    ]


def _dcn_id(c):
    return '-'.join(str(v) for v in c)


def _dcn_tensors(case, mode):
    """bf16x2: random fractional offsets at the case's scale and random masks; bf16: integer offsets up to the reach that lands in the same
    window of dcn_bwdin6's selection (2 / 5 / 12 px; 2 % of the components beyond 2.5 / 3.5 / 5.5 / 8.5 px switch up) and masks in
    {1, 1/2, 1/4}."""
    B, C, Co, dg, H, W, ostd, with_bias = case
    g = torch.Generator().manual_seed(_seed(B, C, Co, dg, H, W))
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) / (3 * C ** 0.5)
    b = torch.randn(Co, generator=g) if with_bias else None
    gout = torch.randn(B, Co, H, W, generator=g)
    if mode == 'bf16':
        off = MR.integer_offsets(B, dg, H, W, 2 if ostd <= 1.0 else (5 if ostd <= 3.0 else 12), g)
        m = MR.pow2_masks(B, dg, H, W, g)
    else:
        off = torch.randn(B, dg * 18, H, W, generator=g) * ostd
        m = torch.rand(B, dg * 9, H, W, generator=g)
    return x, off, m, w, b, gout


def _dcn_run(mode, x, off, m, w, b, gout, dg, pad=1):
    from realvsr_amd import functional as RF
    from realvsr_amd.archs.dcn import modulated_deform_conv
    d = dev()
    RF.invalidate_weight_cache()   # (the operator packs its weight image per call; nothing of an earlier run may serve this one)
    leaves = [None if t is None else t.to(d).requires_grad_(True) for t in (x, off, m, w, b)]
    with _mode(mode):
        out = modulated_deform_conv(*leaves, 1, pad, 1, 1, dg)
        out.backward(gout.to(d))
        torch.cuda.synchronize()
    names = ('grad_input', 'grad_offset', 'grad_mask', 'grad_weight', 'grad_bias')
    got = {n: (None if t is None else t.grad) for n, t in zip(names, leaves)}
    got['out'] = out.detach()
    return got


def _gx_distance(a, ref):
    return l2_err(a, ref), rel_err(a.cpu(), ref.cpu())


def _gx_bounded(name, a, ref, path='fused'):
    l2, mx = _gx_distance(a, ref)
    bound = GX_BOUND[path]
    print('%-60s grad_input l2 %.3e (bound %.1e), max %.3e (bound %.1e)' % (name, l2, bound[0], mx, bound[1]))
    assert l2 <= bound[0] and mx <= bound[1], (name, l2, mx, bound)


def _dcn_plans(case, mode):
    """(forward, input gradient, weight gradient) as (family name, terms) from rvsr_dcn_pack_forward_plan / rvsr_dcn_pack_backward_plan: the
    operator's entries ask the same two plan functions (csrc/dcn_plan.h) with the same geometry; probe, hint and prepacked flag move
    neither family nor term count."""
    B, C, Co, dg, H, W = case[:6]
    rc, f = DL.fwd_plan(DL.fwd_call(B, C, Co, dg, H, W), mode)
    assert rc == 0, rc
    rc, q = DL.bwd_plan(DL.bwd_call(B, C, Co, dg, H, W), mode)
    assert rc == 0, rc
    in_fam = DL.IN_FAMILY[q['in_family']]
    return ((DL.FWD_FAMILY[f['family']], f['NT']), (in_fam, q['in_NT'] if in_fam == 'dcn_bwdin6' else 3),
            (DL.W_FAMILY[q['w_family']], q['w_NT']), q['NK'])


def _dcn_reference_runs(case, mode):
    """The tensors of the reference runs in 'bf16x3': (forward, input / offset / mask gradient, weight / bias gradient)."""
    B, C, Co, dg = case[:4]
    x, off, m, w, b, gout = _dcn_tensors(case, mode)
    if mode == 'bf16x2':
        a = (x, off, m, R(w), b, gout, dg)
        return a, a, (x, off, m, w, b, R(gout), dg)
    # bf16: the forward and the weight gradient form their column operand from x; dcn_bwdin6 rounds W and gOut and keeps x
    return (R(x), off, m, R(w), b, gout, dg), (x, off, m, R(w), b, R(gout), dg), (R(x), off, m, w, b, R(gout), dg)


def _check_dcn_case(case, mode):
    nt = TERMS[mode]
    (ffam, fnt), (ifam, int_), (wfam, wnt), nk = _dcn_plans(case, mode)
    dg = case[3]
    tensors = _dcn_tensors(case, mode)
    tag = '%s %s ' % (mode, _dcn_id(case))
    got = _dcn_run(mode, *tensors, dg)
    plain = _dcn_run('bf16x3', *tensors, dg)
    ref_f, ref_i, ref_w = _dcn_reference_runs(case, mode)
    ran = []
    if (ffam, fnt) == ('dcn_fwd3', nt):
        ref = _dcn_run('bf16x3', *ref_f)
        _same(tag + 'out (dcn_fwd3, %d terms)' % fnt, got['out'], ref['out'])
        _differs(tag + 'out', got['out'], plain['out'])
        ran.append('dcn_fwd3')
    else:
        assert fnt == 3, (ffam, fnt)
        _same(tag + 'out (%s: three terms by the plan)' % ffam, got['out'], plain['out'])
    if (ifam, int_) == ('dcn_bwdin6', nt):
        ref = ref if ref_i is ref_f and ran else _dcn_run('bf16x3', *ref_i)
        _same(tag + 'grad_offset (dcn_bwdin6<%d>, %d terms)' % (nk, int_), got['grad_offset'], ref['grad_offset'])
        _same(tag + 'grad_mask', got['grad_mask'], ref['grad_mask'])
        _differs(tag + 'grad_offset', got['grad_offset'], plain['grad_offset'])
        _differs(tag + 'grad_mask', got['grad_mask'], plain['grad_mask'])
        # (an atomic scatter: the module docstring)
        _gx_bounded(tag + 'against the three-term kernel on the rounded operands', got['grad_input'], ref['grad_input'])
        ran.append('dcn_bwdin6<%d>' % nk)
    else:
        assert int_ == 3, (ifam, int_)
        _same(tag + 'grad_offset (%s: three terms by the plan)' % ifam, got['grad_offset'], plain['grad_offset'])
        _same(tag + 'grad_mask', got['grad_mask'], plain['grad_mask'])
        _gx_bounded(tag + 'against the default mode', got['grad_input'], plain['grad_input'])
    if wfam in ('dcn_bwdw6', 'dcn_bwdw4') and wnt == nt:
        ref = _dcn_run('bf16x3', *ref_w)
        _same(tag + 'grad_weight (%s, %d terms)' % (wfam, wnt), got['grad_weight'], ref['grad_weight'])
        _differs(tag + 'grad_weight', got['grad_weight'], plain['grad_weight'])
        if got['grad_bias'] is not None:
            # a product with a ones column (dcn6_kernels.hip:1003 and 1023-1026; dcn_bwdw4.inc:37, 254-256, 281): the rounded output gradient's
            _same(tag + 'grad_bias', got['grad_bias'], ref['grad_bias'])
            _differs(tag + 'grad_bias', got['grad_bias'], plain['grad_bias'])
        ran.append(wfam)
    else:
        assert wnt == 3, (wfam, wnt)
        _same(tag + 'grad_weight (%s: three terms by the plan)' % wfam, got['grad_weight'], plain['grad_weight'])
        if got['grad_bias'] is not None:
            _same(tag + 'grad_bias', got['grad_bias'], plain['grad_bias'])
    return ran


@pytest.mark.parametrize('case', _dcn_cases(), ids=_dcn_id)
def test_dcn_is_the_three_term_kernels_on_rounded_operands(case, speed_mode):
    _check_dcn_case(case, speed_mode)


def test_the_dcn_cases_reach_every_reduced_dcn_kernel(speed_mode):
    """By the plans alone: dcn_fwd3 with two and four M tiles, dcn_bwdin6 with NK = 4 and NK = 8, dcn_bwdw6 and dcn_bwdw4 run with the
    mode's term count in some case; the offset scales reach the 2, 5 and 12 px windows of dcn_bwdin6<4>."""
    nt = TERMS[speed_mode]
    seen = set()
    for case in _dcn_cases():
        (ffam, fnt), (ifam, int_), (wfam, wnt), nk = _dcn_plans(case, speed_mode)
        if fnt == nt:
            seen.add(ffam)
        if int_ == nt:
            seen.add((ifam, nk))
            if nk == 4:
                B, C, Co, dg, H, W = case[:6]
                off = _dcn_tensors(case, speed_mode)[1]
                q = DL.bwd_plan(DL.bwd_call(B, C, Co, dg, H, W), speed_mode)[1]
                seen.add(('window', DL.selected(DL.bwd_cands(q), DL.probe_counters(off.numpy()))))
        if wnt == nt:
            seen.add(wfam)
    want = {'dcn_fwd3', ('dcn_bwdin6', 4), ('dcn_bwdin6', 8), 'dcn_bwdw6', 'dcn_bwdw4', ('window', 2), ('window', 5), ('window', 12)}
    assert want <= seen, (sorted(map(str, want - seen)), sorted(map(str, seen)))


# ------------------------------------------------------------------------------------------------------------------------------------
# Scope: what the header says the modes do NOT touch gives the default mode's bits
SCOPE_CONVS = [
    # (C, Co, k, stride, H, W), (data gradient reduced, weight gradient reduced).  The FORWARD of every one keeps three terms.  Their
    # gradients are calls of their own and the plan of each decides: the data gradient of the stride-2, the 32- and the 3-channel conv is a
    # stride-1 conv with 64 output channels (on the zero-insert view for stride 2) -- conv_fwd5 with 64-row m-blocks, reduced --, and
    # conv_wgrad2 takes every 3x3 / stride-1 weight gradient with more than 4 output channels.
    ((64, 64, 1, 1, 9, 20), (False, False)),     # 1x1
    ((64, 64, 3, 2, 16, 24), (True, False)),     # 3x3 stride 2
    ((16, 16, 3, 2, 16, 24), (False, False)),    # 3x3 stride 2 with 32-row m-blocks in both directions
    ((16, 16, 7, 1, 9, 20), (False, False)),     # 7x7
    ((64, 32, 3, 1, 16, 24), (True, True)),      # 32-row m-blocks
    ((64, 3, 3, 1, 16, 24), (True, False)),      # the 3-channel output conv (vector-ALU forward and weight gradient)
    ((64, 64, 3, 1, 9, 30), (False, False)),     # W % 4 != 0: the scalar-staged view (and the exact-f32 weight gradient)
]


def test_scope_of_the_speed_modes(speed_mode):
    """A 1x1, a stride-2, a 7x7 conv, 32 and 3 output channels, a width off the vector path: the forward gives the default mode's bits,
    and so does every gradient whose own call the plan gives three terms (SCOPE_CONVS says which are not; those are the rounded operands').
    A 5x5 conv: forward and data gradient equal, the weight gradient (conv_wgrad5) differs and is the rounded operands'.  The generic DCN
    path (a 5 x 5 deformable kernel) and a fused DCN with 16 output channels (q.in_nt = nk >= 4 ? ... : 3, csrc/dcn_plan.h): forward,
    offset and mask gradient equal, grad_input within the run-to-run bound; the fused one's weight gradient is reduced."""
    nt = TERMS[speed_mode]
    for (C, Co, k, stride, H, W), (dgrad_reduced, wgrad_reduced) in SCOPE_CONVS:
        block = (C, 0, Co, k, stride, 'none', False, False, 2, H, W)
        assert _check_conv_block(block, (0, 0, 0, 0), speed_mode) == (False, dgrad_reduced, wgrad_reduced), block
    for stride in (1, 2):
        block = (64, 0, 64, 5, stride, 'none', False, False, 2, 9, 20)
        assert _check_conv_block(block, (0, 0, 0, 0), speed_mode) == (False, False, True)
    # the fused DCN with C_out <= 32
    case = (2, 16, 16, 2, 9, 33, 2.0, True)
    assert _dcn_plans(case, speed_mode)[:3] == (('dcn_fwd3', 3), ('dcn_bwdin6', 3), ('dcn_bwdw6', nt))
    assert _check_dcn_case(case, speed_mode) == ['dcn_bwdw6']
    # the generic path: a 5 x 5 deformable kernel
    g = torch.Generator().manual_seed(55)
    B, C, Co, dg, H, W = 1, 16, 16, 2, 8, 12
    t = (torch.randn(B, C, H, W, generator=g), torch.randn(B, dg * 50, H, W, generator=g) * 1.5, torch.rand(B, dg * 25, H, W, generator=g),
         torch.randn(Co, C, 5, 5, generator=g) / (5 * C ** 0.5), torch.randn(Co, generator=g), torch.randn(B, Co, H, W, generator=g))
    got, plain = _dcn_run(speed_mode, *t, dg, pad=2), _dcn_run('bf16x3', *t, dg, pad=2)
    for name in ('out', 'grad_offset', 'grad_mask', 'grad_weight', 'grad_bias'):
        _same('%s scope generic DCN %s' % (speed_mode, name), got[name], plain[name])
    _gx_bounded(speed_mode + ' scope generic DCN', got['grad_input'], plain['grad_input'], 'generic')
