"""Block cases that fill the coverage ledger of the conv kernels (tests/test_conv_ledger_host.py), vs torch CPU float64.  -m gpu

Same comparison, distance from the activation kink and tolerances as test_gpu_conv.test_conv_block_forward_backward (which it calls).
Each case is the smallest shape found for a kernel variant that no other list reaches: the ledger test names the key a case is there
for, and fails when a case is removed.  Offsets are floats from a 16-byte boundary of (x1, x2, the output gradient, the residual): the
plan's fallbacks for a misaligned pointer.

The drift guard at the end records what functional.py really passes to the library and compares it with what tests/conv_ledger.py
says it passes: the ledger is worked out from the latter."""
import pytest
import torch
import torch.nn as nn

import conv_ledger as CL
from gpu_util import dev, gemm_modes
from test_gpu_conv import test_conv_block_forward_backward as _block

pytestmark = pytest.mark.gpu

Z = (0, 0, 0, 0)
LEDGER_CASES = [
    # (C1, C2, Co, k, stride, act, residual, pixel_shuffle, B, H, W), offsets
    # PixelShuffle without an activation: the pixel-unshuffle staging (VEC 2) of the data gradient without act', 64- and 32-row m-blocks
    ((64, 0, 256, 3, 1, 'none', False, True, 1, 12, 20), Z),
    ((16, 0, 64, 3, 1, 'none', False, True, 2, 8, 12), Z),
    # stride 2 without an activation at 64 channels: the zero-insert staging (VEC 3) without act', 64-row m-blocks
    ((64, 0, 64, 3, 2, 'none', False, False, 1, 16, 24), Z),
    # the residual epilogue of conv_fwd2: stride 2 and 1x1, 16-byte and element stores
    ((16, 0, 16, 3, 2, 'none', True, False, 1, 16, 24), Z),
    ((64, 0, 64, 3, 2, 'none', True, False, 1, 9, 30), Z),
    ((48, 0, 16, 1, 1, 'none', True, False, 2, 8, 12), Z),
    ((64, 0, 64, 1, 1, 'none', True, False, 1, 9, 30), Z),
    # 1x1 concat off the chunk: exact-f32 forward, and a data gradient that is conv_fwd2 with a split output of a 32-row m-block
    ((16, 16, 16, 1, 1, 'lrelu', False, True, 1, 8, 12), Z),
    # stride-2 weight gradient with three m-blocks and two 64-channel blocks (8 x 16 output)
    ((128, 0, 136, 3, 2, 'lrelu', False, False, 1, 16, 32), Z),
    # conv_wgrad2 with a concat and act' together
    ((64, 64, 64, 3, 1, 'lrelu', False, False, 1, 8, 36), Z),
    # conv_wgrad1x1s with three m-blocks and no concat
    ((64, 0, 136, 1, 1, 'none', False, False, 1, 8, 12), Z),
    # calls that fall to the exact-f32 families in bf16x3 mode: a concat off the chunk (1x1: 32, 3x3 / stride 2: 16, 3x3: 8 channels), with
    # 32-, 64- and 128-row m-blocks, the PixelShuffle and residual epilogues, one weight-gradient tile (P = 1)
    ((16, 16, 80, 1, 1, 'none', False, False, 1, 8, 12), Z),
    ((3, 16, 12, 3, 1, 'none', True, False, 1, 4, 30), (1, 1, 0, 1)),
    ((3, 16, 64, 3, 1, 'lrelu', False, True, 1, 8, 12), Z),
    ((3, 16, 80, 3, 1, 'none', False, False, 1, 8, 12), Z),
    ((8, 16, 12, 3, 2, 'none', False, False, 1, 8, 36), Z),
    ((8, 16, 64, 3, 2, 'lrelu', False, False, 1, 9, 30), Z),
    ((8, 16, 80, 3, 2, 'none', True, False, 2, 16, 24), (1, 1, 0, 1)),
    # 1x1 with PixelShuffle: the epilogue of conv_fwd2, the exact-f32 weight gradient on a pixel-shuffled gradient view
    ((16, 0, 64, 1, 1, 'lrelu', False, True, 1, 8, 12), Z),
    # a pointer one float off a 16-byte boundary on frames with W % 4 == 0: scalar staging with 16-byte stores (x1 / the output
    # gradient off), 16-byte staging with element stores (the residual off), both; the weight gradient falls to the exact-f32 families
    ((64, 0, 64, 3, 1, 'lrelu', False, False, 1, 8, 64), (1, 0, 0, 0)),
    ((64, 0, 64, 3, 1, 'lrelu', False, False, 1, 8, 64), (0, 0, 1, 0)),
    ((64, 0, 64, 3, 1, 'none', True, False, 1, 8, 64), (0, 0, 0, 1)),
    ((16, 0, 16, 3, 1, 'none', True, False, 2, 8, 36), (1, 0, 0, 1)),
    ((64, 0, 64, 3, 2, 'lrelu', False, False, 1, 16, 32), (1, 0, 0, 0)),
    ((16, 0, 24, 3, 2, 'none', True, False, 1, 16, 24), (1, 0, 1, 1)),
    ((48, 0, 16, 1, 1, 'none', True, False, 2, 8, 12), (1, 0, 1, 1)),
    ((16, 16, 80, 1, 1, 'none', True, False, 1, 8, 12), (1, 1, 0, 1)),
]

# Cases whose keys another new case reaches too: a premask pair of test_gpu_conv_nodes.py (PixelShuffle without act'), a raw-ABI case, a
# case with offsets on the same kernel, or -- the ledger's coordinates are pairwise, not the full product -- the combination that the
# comment above the case names.  Every other case is the only one that reaches some key: test_conv_ledger_host.test_a_dropped_case_is_named.
NOT_SOLE = [
    ((64, 0, 256, 3, 1, 'none', False, True, 1, 12, 20), Z),
    ((16, 0, 64, 3, 1, 'none', False, True, 2, 8, 12), Z),
    ((64, 0, 64, 3, 2, 'none', False, False, 1, 16, 24), Z),
    ((64, 0, 64, 3, 2, 'none', True, False, 1, 9, 30), Z),
    ((64, 0, 64, 1, 1, 'none', True, False, 1, 9, 30), Z),
    ((16, 16, 16, 1, 1, 'lrelu', False, True, 1, 8, 12), Z),
    ((64, 64, 64, 3, 1, 'lrelu', False, False, 1, 8, 36), Z),
    ((64, 0, 136, 1, 1, 'none', False, False, 1, 8, 12), Z),
    ((64, 0, 64, 3, 1, 'lrelu', False, False, 1, 8, 64), (1, 0, 0, 0)),
    ((64, 0, 64, 3, 1, 'none', True, False, 1, 8, 64), (0, 0, 0, 1)),
]

gemm_mode = gemm_modes()


def _id(v):
    case, offsets = v
    return '-'.join(str(x) for x in case) + ('' if not any(offsets) else '+' + ''.join(str(o) for o in offsets))


@pytest.mark.parametrize('case', LEDGER_CASES, ids=_id)
def test_ledger_case_forward_backward(case, gemm_mode):
    _block(case[0], gemm_mode, offsets=case[1])


# ---- drift guard
class _Recorder:
    """Wraps functional._conv / functional._conv_wgrad: the calls that ran (a refused mask epilogue is the caller's question, not a call)."""

    def __enter__(self):
        from realvsr_amd import functional as RF
        self.RF, self.calls, self.orig = RF, [], (RF._conv, RF._conv_wgrad)

        def conv(*a, **kw):
            ran = self.orig[0](*a, **kw)
            if ran:
                self.calls.append(CL.fwd_call_of_args(*a, **kw))
            return ran

        def wgrad(*a, **kw):
            self.calls.append(CL.wgrad_call_of_args(*a, **kw))
            return self.orig[1](*a, **kw)
        RF._conv, RF._conv_wgrad = conv, wgrad
        return self

    def __exit__(self, *exc):
        self.RF._conv, self.RF._conv_wgrad = self.orig


def _same_calls(name, got, want):
    canon = lambda calls: sorted(repr(sorted(c.items())) for c in calls)   # noqa: E731  (a pair's backward order is autograd's)
    assert canon(got) == canon([c for _, c in want]), '%s: functional.py issues\n%s\nthe ledger expects\n%s' % (
        name, '\n'.join(canon(got)), '\n'.join(canon([c for _, c in want])))


def _run_block(case, offsets=Z, x_premask=None, grad_premasked=False, x=None):
    """Forward (+ backward when x is None) of one conv2d() node on random tensors; returns (output, what to call backward on)."""
    from test_gpu_conv import _at_offset
    from realvsr_amd import functional as RF
    C1, C2, Co, k, stride, act, use_res, ps, B, H, W = case
    d = dev()
    conv = nn.Conv2d(C1 + C2, Co, k, stride, k // 2).to(d)
    x1 = _at_offset(torch.randn(B, C1, H, W), offsets[0], d) if x is None else x
    x2 = _at_offset(torch.randn(B, C2, H, W), offsets[1], d) if C2 else None
    Ho, Wo = CL.out_size(H, W, k, stride)
    oshape = (B, Co // 4, 2 * Ho, 2 * Wo) if ps else (B, Co, Ho, Wo)
    res = _at_offset(torch.randn(oshape), offsets[3], d) if use_res else None
    y = RF.conv2d(x1, conv, CL.ACT[act], 0.1, x2=x2, residual=res, pixel_shuffle=ps,
                  x_premask=None if x_premask is None else (CL.ACT[x_premask], 0.1), grad_premasked=grad_premasked)
    return y, _at_offset(torch.randn(oshape), offsets[2], d, leaf=False)


def test_the_ledger_knows_the_calls_of_functional():
    """Plain, concat, PixelShuffle, stride 2, with and without an activation, fused and outside residual, pointers off the boundary,
    res_block on a frame the mask epilogue takes and one it does not, a premask pair, conv_cat_bcast with sinks: the arguments that
    reach the library equal conv_ledger's."""
    from realvsr_amd import _lib
    from realvsr_amd import functional as RF
    mode = _lib.get_gemm_mode()
    d = dev()
    torch.manual_seed(3)
    blocks = [((16, 0, 16, 3, 1, 'lrelu', False, False, 2, 12, 20), Z), ((64, 64, 64, 3, 1, 'none', False, False, 1, 8, 36), Z),
              ((16, 0, 64, 3, 1, 'lrelu', False, True, 1, 8, 12), Z), ((16, 0, 24, 3, 2, 'none', False, False, 1, 18, 32), Z),
              ((64, 0, 64, 3, 1, 'none', True, False, 1, 8, 64), (0, 0, 0, 1)), ((64, 0, 64, 3, 1, 'lrelu', True, False, 1, 16, 24), Z),
              ((48, 0, 16, 1, 1, 'none', True, False, 2, 8, 12), (1, 0, 1, 1)), ((8, 16, 80, 3, 2, 'none', True, False, 2, 16, 24), (1, 1, 0, 1))]
    for case, offsets in blocks:
        with _Recorder() as rec:
            y, gout = _run_block(case, offsets)
            y.backward(gout)
        _same_calls(str((case, offsets)), rec.calls, CL.calls_of(case, offsets, mode))
    for C, B, H, W in ((64, 1, 7, 64), (64, 1, 16, 24), (16, 1, 8, 64)):
        c1, c2 = nn.Conv2d(C, C, 3, 1, 1).to(d), nn.Conv2d(C, C, 3, 1, 1).to(d)
        x = torch.randn(B, C, H, W, device=d, requires_grad=True)
        with _Recorder() as rec:
            RF.res_block(x, c1, c2).backward(torch.randn(B, C, H, W, device=d))
        _same_calls('res_block %s' % ((C, B, H, W),), rec.calls, CL.res_block_calls(C, B, H, W, mode))
        assert any(c.get('act') == CL.ACT_MASK for c in rec.calls) == (C == 64 and RF.grad_mask_fusable(H, W))
    for pair in (((64, 0, 64, 3, 1, 'lrelu', False, False, 1, 8, 64), (64, 0, 64, 3, 1, 'lrelu', False, False, 1, 8, 64)),
                 ((16, 0, 64, 3, 1, 'lrelu', False, True, 1, 8, 12), (16, 0, 3, 3, 1, 'none', True, False, 1, 16, 24))):
        with _Recorder() as rec:
            p, _ = _run_block(pair[0], grad_premasked=True)
            y, gout = _run_block(pair[1], x_premask=pair[0][5], x=p)
            y.backward(gout)
        _same_calls('pair %s' % (pair,), rec.calls, CL.premask_pair_calls(pair, mode))
    for case in ((16, 16, 16, 'lrelu', 3, 2, 8, 12, None, None), (16, 16, 16, 'none', 3, 1, 9, 10, 'own', 1)):
        C1, C2, Co, act, N, B, H, W, x_sink, ref_sink = case
        conv = nn.Conv2d(C1 + C2, Co, 3, 1, 1).to(d)
        x = torch.randn(N * B, C1, H, W, device=d, requires_grad=True)
        ref = torch.randn(B, C2, H, W, device=d, requires_grad=True)
        xs = rs = None
        if x_sink:
            xs = RF.GradSink()
            xs.buf = torch.randn(N * B, C1, H, W, device=d)
        if ref_sink is not None:
            rs = RF.GradSink((N * B, C2, H, W))
        with _Recorder() as rec:
            y = RF.conv_cat_bcast(x, ref, conv, N, CL.ACT[act], 0.1, x_sink=xs, x_owner=x_sink == 'own', ref_sink=rs,
                                  ref_block=ref_sink or 0)
            y.backward(torch.randn_like(y))
        _same_calls('conv_cat_bcast %s' % (case,), rec.calls, CL.cat_bcast_calls(case))
    # the frame-major nodes: 105-float frames, so that the frame ranges and the centre block start off a 16-byte boundary
    for case in ((5, 1, 4, 1, 3, 16, 5, 7, 3, True, True), (2, 0, 2, 1, 16, 3, 5, 7, 3, True, False)):
        T, f0, f1, B, Ci, Co, H, W, k, _, use_res = case
        conv = nn.Conv3d(Ci, Co, (3, k, k), padding=(1, k // 2, k // 2)).to(d)
        x = torch.randn(T, B, Ci, H, W, device=d, requires_grad=True)
        res = torch.randn(f1 - f0, B, Co, H, W, device=d) if use_res else None
        with _Recorder() as rec:
            RF.conv3d_frames(x, conv, frames=(f0, f1), residual=res).backward(torch.randn(f1 - f0, B, Co, H, W, device=d))
        _same_calls('conv3d_frames %s' % (case,), rec.calls, CL.conv3d_frames_calls(case))
    case = (3, 1, 1, 3, 5, 7)
    N, center, B, C, H, W = case
    t1, t2 = nn.Conv2d(C, C, 3, 1, 1).to(d), nn.Conv2d(C, C, 3, 1, 1).to(d)
    aligned = torch.randn(N, B, C, H, W, device=d, requires_grad=True)
    with _Recorder() as rec:
        RF.tsa_temporal_block(aligned, center, t1, t2).backward(torch.randn(B, N * C, H, W, device=d))
    _same_calls('tsa_temporal_block %s' % (case,), rec.calls, CL.tsa_block_calls(case))
    case = (6, 16, 24, 5, 7)
    convt = nn.ConvTranspose3d(16, 24, 1).to(d)
    x = torch.randn(3, 2, 16, 5, 7, device=d, requires_grad=True)
    with _Recorder() as rec:
        RF.conv_transpose1x1(x, convt).backward(torch.randn(3, 2, 24, 5, 7, device=d))
    _same_calls('conv_transpose1x1 %s' % (case,), rec.calls, CL.conv_transpose1x1_calls(case))
    torch.cuda.synchronize()
