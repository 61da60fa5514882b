"""The fused DCN pack node (functional.dcn_pack: sigmoid of the mask logits, activation epilogue, act' from the saved output, GradSink
deposit) against its float64 reference (tests/dcn_pack_reference.py), one case per kernel variant.  -m gpu

Which variant a case runs is asserted from the exported plan rows (tests/dcn_ledger.py; the coverage ledger over these case lists is
tests/test_dcn_ledger_host.py); where the device selects a halo from the offset counters, the counters of rvsr_dcn_offset_probe are held
against the ledger's numpy restatement first, and the selection rule is applied to them on the host.  Any window is numerically correct
(samples beyond it take the global path), so values cannot tell which halo ran: that assertion rests on the plan and the probe.

Every tensor is compared three times through gpu_util.check (maximum and L2 error), each part relative to its own maximum: whole, the
outermost ring of pixels (samples in (-1, 0) and (H - 1, H) interpolate against zeros), and the last tile column and row (32 x 8 tiles:
ragged where the frame is no multiple).  Tolerances are those of test_gpu_dcn.py."""
import ctypes
import functools

import pytest
import torch

import dcn_ledger as DL
import dcn_pack_reference as DR
from gpu_util import check, dev, gemm_modes, l2_err

gemm_mode = gemm_modes()

pytestmark = pytest.mark.gpu
TOL = {'f32': 2e-5, 'bf16x3': 1e-4}
TOL_G = 1e-4
SLOPE = 0.1


def _tols(mode):
    return TOL[mode], max(TOL_G, TOL[mode])


# ---- the cases (plain data and CPU generators: the host ledger imports them)
HALO_SHAPE = (2, 16, 2, 20, 68)   # B, C, dg, H, W: 4 | W, two ragged tile edges
HALO_CO = (16, 32, 64, 128)       # NK 1 / 2 / 4 / 8, MT 1 / 1 / 2 / 4
# regime: offset components uniform in +-a px, 0.5 % of them replaced by +-(far + U[0, 1)) px -- below every selection threshold (1 % is
# the smallest), but the beyond-window gather and atomics run
REGIMES = {'A': (2.4, 6.0), 'B': (3.4, 8.0), 'C': (5.4, 10.0), 'D': (8.4, 13.0), 'E': (12.0, 17.0)}
# what the regimes select (asserted from the host rule on each case's own offsets): dcn_bwdin6's window, 12 px not built at NK 8;
# dcn_fwd3's tile under no_grad, 11 px not built at MT 4
HALO_BWD = {'A': 2, 'B': 4, 'C': 5, 'D': 8, 'E': 12}
HALO_FWD = {'A': 3, 'B': 3, 'C': 7, 'D': 11, 'E': 11}
HALO_CASES = [(co, r) for co in HALO_CO for r in REGIMES]


def halo_expected(Co, regime):
    return min(HALO_BWD[regime], 8 if Co > 64 else 12), min(HALO_FWD[regime], 7 if Co > 64 else 11)


def halo_case(Co):
    B, C, dg, H, W = HALO_SHAPE
    return (B, C, Co, dg, H, W)


def _inputs(case, g, with_bias=True):
    B, C, Co, dg, H, W = case[:6]
    stride, dil = (tuple(case[6:]) + (1, 1))[:2]
    Ho, Wo = DL.out_size(H, W, stride, dil, dil)
    x = torch.randn(B, C, H, W, generator=g)
    logits = torch.randn(B, 9 * dg, Ho, Wo, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) / (3 * C ** 0.5)
    b = torch.randn(Co, generator=g) if with_bias else None
    gout = torch.randn(B, Co, Ho, Wo, generator=g)
    return x, logits, w, b, gout


@functools.lru_cache(maxsize=None)
def halo_inputs(Co, regime):
    """x, om, w, b, gout (float32, CPU) of a halo-matrix case."""
    a, far = REGIMES[regime]
    g = torch.Generator().manual_seed(1000 + Co + ord(regime))
    case = halo_case(Co)
    B, _, _, dg, H, W = case
    off = (torch.rand(B, 18 * dg, H, W, generator=g) * 2 - 1) * a
    out = torch.rand(off.shape, generator=g) < 0.005
    sign = torch.where(torch.rand(off.shape, generator=g) < 0.5, -1.0, 1.0)
    off = torch.where(out, sign * (far + torch.rand(off.shape, generator=g)), off)
    x, logits, w, b, gout = _inputs(case, g)
    return x, torch.cat([off, logits], 1), w, b, gout


def halo_counters(Co, regime):
    dg = HALO_SHAPE[2]
    return DL.probe_counters(halo_inputs(Co, regime)[1][:, :18 * dg].numpy())


NODE_CASES = [
    # (B, C, Co, dg, H, W[, stride[, dilation]]), gout floats off a 16-byte boundary: forward / input-gradient / weight-gradient family in
    # bf16x3, 16-byte gOut staging (None: one staging)
    ((1, 16, 16, 2, 8, 32), 0, ('dcn_fwd3', 'dcn_bwdin6', 'dcn_bwdw6', None)),        # hand-off with act'
    ((1, 16, 128, 2, 8, 32), 0, ('dcn_fwd3', 'dcn_bwdin6', 'dcn_bwdw6', None)),       # NK 8, two 64-channel units
    ((2, 64, 72, 8, 16, 64), 0, ('dcn_fwd3', 'dcn_bwdin6', 'dcn_bwdw6', None)),       # gy 16
    ((1, 32, 16, 2, 8, 32), 0, ('dcn_fwd3', 'dcn_bwdin6', 'dcn_bwdw6', None)),        # 16 channels per deformable group
    ((1, 8, 130, 1, 8, 32), 0, ('dcn_fwd3', 'dcn_bwd_input', 'dcn_bwdw4', True)),     # dcn_fwd3<4>, dcn_bwd_input_kernel<8> at its LDS bound
    ((1, 8, 130, 1, 7, 30), 0, ('dcn_fwd3', 'dcn_bwd_input', 'dcn_bwdw2', False)),    # 4 does not divide Wo: scalar staging
    ((1, 8, 130, 1, 8, 32), 1, ('dcn_fwd3', 'dcn_bwd_input', 'dcn_bwdw2', False)),    # gout a contiguous view one float off: scalar staging
    ((1, 16, 16, 2, 15, 63, 2), 0, ('dcn_fwd2', 'dcn_bwd_input', 'dcn_bwdw2', True)),     # stride 2, Wo 32
    ((1, 16, 16, 2, 9, 33, 2), 0, ('dcn_fwd2', 'dcn_bwd_input', 'dcn_bwdw2', False)),     # stride 2, Wo 17
    ((1, 16, 16, 2, 10, 34, 1, 2), 0, ('dcn_fwd2', 'dcn_bwd_input', 'dcn_bwdw2', False)),  # dilation 2
    ((1, 16, 16, 4, 8, 32), 0, ('dcn_fwd1', 'dcn_bwd_input', 'dcn_bwd_weight', None)),    # 4 channels per deformable group: first generation
]
# Cases that are here for a key of the coverage ledger (tests/test_dcn_ledger_host.py) no case above reaches -- the grids of the
# weight-gradient kernels (gy = ceil(Co / 64), gz = C / 8, one partial where a stride-2 frame is one tile) with and without act', the
# wider m-blocks of dcn_fwd2 and dcn_fwd_kernel: (case, gout offset, activation), with a bias, in both GEMM modes.  Chosen greedily,
# smallest first, from the ledger's own sweep.
LEDGER_CASES = [
    ((1, 8, 8, 2, 7, 30, 2, 1), 0, 'none'),
    ((1, 8, 8, 1, 8, 32, 2, 1), 0, 'none'),
    ((1, 8, 8, 1, 8, 32, 2, 1), 0, 'lrelu'),
    ((2, 8, 8, 2, 7, 30, 2, 1), 0, 'lrelu'),
    ((2, 8, 8, 1, 7, 30, 2, 1), 0, 'none'),
    ((2, 8, 8, 1, 7, 30, 2, 1), 0, 'lrelu'),
    ((1, 16, 8, 4, 7, 30, 2, 1), 0, 'none'),
    ((1, 16, 8, 4, 7, 30, 2, 1), 0, 'lrelu'),
    ((1, 16, 8, 2, 7, 30, 2, 1), 0, 'none'),
    ((1, 16, 8, 2, 7, 30, 2, 1), 0, 'lrelu'),
    ((2, 8, 8, 1, 8, 32, 2, 1), 0, 'none'),
    ((2, 8, 8, 1, 8, 32, 2, 1), 0, 'lrelu'),
    ((1, 16, 8, 2, 8, 32, 2, 1), 0, 'none'),
    ((1, 16, 8, 2, 8, 32, 2, 1), 0, 'lrelu'),
    ((1, 8, 64, 2, 7, 30, 2, 1), 0, 'lrelu'),
    ((1, 8, 64, 1, 7, 30, 2, 1), 0, 'none'),
    ((1, 8, 64, 1, 7, 30, 2, 1), 0, 'lrelu'),
    ((1, 8, 72, 2, 7, 30, 2, 1), 0, 'none'),
    ((1, 8, 72, 2, 7, 30, 2, 1), 0, 'lrelu'),
    ((1, 8, 72, 1, 7, 30, 2, 1), 0, 'none'),
    ((1, 8, 72, 1, 7, 30, 2, 1), 0, 'lrelu'),
    ((1, 8, 72, 1, 8, 32, 2, 1), 0, 'none'),
    ((1, 8, 72, 1, 8, 32, 2, 1), 0, 'lrelu'),
    ((2, 8, 72, 2, 7, 30, 2, 1), 0, 'none'),
    ((2, 8, 72, 2, 7, 30, 2, 1), 0, 'lrelu'),
    ((1, 16, 72, 4, 7, 30, 2, 1), 0, 'none'),
    ((1, 16, 72, 4, 7, 30, 2, 1), 0, 'lrelu'),
    ((1, 16, 72, 2, 7, 30, 2, 1), 0, 'none'),
    ((1, 16, 72, 2, 7, 30, 2, 1), 0, 'lrelu'),
    ((2, 8, 72, 1, 8, 32, 2, 1), 0, 'none'),
    ((2, 8, 72, 1, 8, 32, 2, 1), 0, 'lrelu'),
    ((1, 16, 72, 2, 8, 32, 2, 1), 0, 'none'),
    ((1, 16, 72, 2, 8, 32, 2, 1), 0, 'lrelu'),
    ((2, 16, 72, 4, 7, 30, 2, 1), 0, 'lrelu'),
    ((2, 16, 72, 2, 7, 30, 2, 1), 0, 'none'),
    ((2, 16, 72, 2, 7, 30, 2, 1), 0, 'lrelu'),
    ((2, 16, 72, 2, 8, 32, 2, 1), 0, 'none'),
    ((2, 16, 72, 2, 8, 32, 2, 1), 0, 'lrelu'),
    ((1, 16, 130, 2, 8, 32, 1, 1), 0, 'none'),
    ((1, 16, 130, 2, 8, 32, 1, 1), 0, 'lrelu'),
    ((1, 8, 16, 1, 8, 32, 1, 1), 0, 'lrelu'),   # dcn_bwdw6 on one chunk, one unit, with act'
]
NODE_ACTS = DR.ACTS
SINK_CASES = [NODE_CASES[0][0], NODE_CASES[1][0], NODE_CASES[4][0], NODE_CASES[10][0]]   # dcn_bwdin6 NK 1 / NK 8, dcn_bwd_input_kernel<8> / <0>
RAW_CASE = NODE_CASES[4][0]


def _name(case):
    return '-'.join(str(v) for v in case)


def ledger_case_name(case, g_off, act):
    return 'ledger %s+%d %s' % (_name(case), g_off, act)


@functools.lru_cache(maxsize=None)
def node_inputs(case, with_bias):
    g = torch.Generator().manual_seed(sum(int(v) for v in case) + 7)
    x, logits, w, b, gout = _inputs(case, g, with_bias)
    dg = case[3]
    off = torch.randn(logits.shape[0], 18 * dg, *logits.shape[2:], generator=g) * 2.0
    return x, torch.cat([off, logits], 1), w, b, gout


def node_counters(case):
    return DL.probe_counters(node_inputs(case, True)[1][:, :18 * case[3]].numpy())


def _geom(case):
    stride, dil = (tuple(case[6:]) + (1, 1))[:2]
    return stride, dil, dil   # stride, pad, dilation


def ledger_calls(mode):
    """[(case name, call, counters of its offsets)] of every DCN call the tests of this file make in a GEMM mode (the halo matrix, the
    operator runs, the sink and raw-ABI cases: bf16x3 only) -- what tests/test_dcn_ledger_host.py counts as reached."""
    out = []
    add = lambda name, calls, cnt: out.extend((name, c, cnt) for _, c in calls)   # noqa: E731
    if mode == 'bf16x3':
        for Co, regime in HALO_CASES:
            case, cnt, tile = halo_case(Co), halo_counters(Co, regime), halo_expected(Co, regime)[1]
            calls = DL.node_calls(case, 'lrelu') + DL.node_calls(case, 'lrelu', hint=tile)[:1] + DL.node_calls(case, 'none', hint=tile)[:1] + \
                DL.node_calls(case, 'lrelu', no_grad=True) + DL.node_calls(case, 'none', no_grad=True) + \
                [('raw backward, own probe', DL.bwd_call(*case, act_out=True))] + DL.node_calls(case, 'none')[1:] + DL.operator_calls(case)[1:]
            add('halo Co%d %s' % (Co, regime), calls, cnt)
        for case in SINK_CASES:
            add('sink %s' % _name(case), DL.node_calls(case, 'lrelu'), node_counters(case))
        add('raw act_out+1', [('backward', DL.bwd_call(*RAW_CASE, act_out=True, act_off=1))], node_counters(RAW_CASE))
    for case, g_off, _ in NODE_CASES:
        for act in NODE_ACTS:
            add('node %s+%d %s' % (_name(case), g_off, act), DL.node_calls(case, act, g_off), node_counters(case))
    for case, g_off, act in LEDGER_CASES:
        add(ledger_case_name(case, g_off, act), DL.node_calls(case, act, g_off), node_counters(case))
    return out


# ---- references, computed once per (inputs, activation)
@functools.lru_cache(maxsize=None)
def _halo_reference(Co, regime, act):
    x, om, w, b, gout = halo_inputs(Co, regime)
    r = DR.reference(x, om, w, b, 1, 1, 1, HALO_SHAPE[2], act, SLOPE, gout)
    assert r['share'] <= DR.KINK_SHARE_MAX, 'kink share %.4f' % r['share']
    return r


@functools.lru_cache(maxsize=None)
def _node_reference(case, with_bias, act):
    x, om, w, b, gout = node_inputs(case, with_bias)
    r = DR.reference(x, om, w, b, *_geom(case), case[3], act, SLOPE, gout)
    assert r['share'] <= DR.KINK_SHARE_MAX, 'kink share %.4f' % r['share']
    return r


# ---- comparisons
def _parts(Hd, Wd):
    ring = torch.zeros(Hd, Wd, dtype=torch.bool)
    ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True
    last = torch.zeros(Hd, Wd, dtype=torch.bool)
    last[8 * ((Hd - 1) // 8):] = True
    last[:, 32 * ((Wd - 1) // 32):] = True
    return (('ring', ring), ('last tile', last))


def check3(name, got, ref, tol, spatial=True, key=None):
    """check() on the whole tensor, its outermost ring and its last tile column / row.  key = (mode, ledger, ledger key, tensor): prints
    the worst maximum and L2 error of the three under that key (the record behind profiles/r15_notes.md)."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    errs = [(check(name, got, ref, tol), l2_err(got, ref))]
    if spatial:
        for part, m in _parts(*ref.shape[-2:]):
            errs.append((check('%s, %s' % (name, part), got[..., m], ref[..., m], tol), l2_err(got[..., m], ref[..., m])))
    if key is not None:
        print('record | %s | %s | %s | %s | %.2e | %.2e' % (key + (max(e for e, _ in errs), max(e for _, e in errs))))


def _check_all(tag, r, out, grads, mode, keys=None):
    """keys: {ledger: key} of the calls that produced these tensors (the forward's for out, the backward's for the gradients)."""
    tol, tol_g = _tols(mode)
    rec = lambda ledger, tensor: None if not keys or ledger not in keys else (mode, ledger, keys[ledger], tensor)   # noqa: E731
    if out is not None:
        check3(tag + ' out', out, r['out'], tol, key=rec('forward', 'out'))
    if grads is not None:
        gx, gom, gw, gb = grads
        if gx is not None:
            check3(tag + ' grad_input', gx, r['gx'], tol_g, key=rec('input gradient', 'grad_input'))
        check3(tag + ' grad_om', gom, r['gom'], tol_g, key=rec('input gradient', 'grad_om'))
        check3(tag + ' grad_weight', gw, r['gw'], tol_g, spatial=False, key=rec('weight gradient', 'grad_weight'))
        assert (gb is None) == (r['gb'] is None)
        if gb is not None:
            check3(tag + ' grad_bias', gb, r['gb'], tol_g, spatial=False, key=rec('weight gradient', 'grad_bias'))


def _keys(calls, mode, counters):
    """{ledger: key} of a list of (what, call)."""
    return {ledger: key for _, call in calls for ledger, key in DL.keys_of(call, mode, counters)}


def _act_code(act):
    from realvsr_amd import functional as RF
    return {'none': RF.ACT_NONE, 'relu': RF.ACT_RELU, 'lrelu': RF.ACT_LRELU}[act]


def _off_by(t, floats):
    """A contiguous copy of `t` on the GPU whose first element sits `floats` floats past a 16-byte boundary (a view into a larger buffer)."""
    buf = torch.empty(t.numel() + 8, device=dev())
    assert buf.data_ptr() % 16 == 0
    v = buf[floats:floats + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * floats
    return v


def _run_node(inputs, case, act, gout, g_off=0, sink=None, leaves=None):
    """The node with gradients: out, (x.grad, om.grad, w.grad, b.grad), the leaves."""
    from realvsr_amd import functional as RF
    d = dev()
    x, om, w, b, _ = inputs
    if leaves is None:
        leaves = [None if t is None else t.to(d).requires_grad_(True) for t in (x, om, w, b)]
    for t in leaves:
        if t is not None:
            t.grad = None
    out = RF.dcn_pack(*leaves, *_geom(case), case[3], act=_act_code(act), slope=SLOPE, sink=sink)
    g = _off_by(gout, g_off) if g_off else gout.to(d)
    seen = []
    out.register_hook(lambda t: seen.append(t.data_ptr() % 16))
    out.backward(g)
    torch.cuda.synchronize()
    assert seen == [4 * g_off], 'the node saw its output gradient at another alignment: %s' % seen
    return out, [None if t is None else t.grad for t in leaves], leaves


def _run_no_grad(inputs, case, act):
    from realvsr_amd import functional as RF
    d = dev()
    x, om, w, b, _ = inputs
    with torch.no_grad():
        out = RF.dcn_pack(*[None if t is None else t.to(d) for t in (x, om, w, b)], *_geom(case), case[3], act=_act_code(act), slope=SLOPE)
    torch.cuda.synchronize()
    return out


@pytest.fixture
def bf16x3():
    from realvsr_amd import _lib
    old = _lib.get_gemm_mode()
    _lib.set_gemm_mode('bf16x3')
    yield 'bf16x3'
    _lib.set_gemm_mode(old)


def _gpu_counters(om, case):
    from realvsr_amd import _lib
    from realvsr_amd._lib import _p, _stream
    B, dg = case[0], case[3]
    probe = torch.zeros(8, dtype=torch.int32, device=om.device)
    _lib.check(_lib.lib().rvsr_dcn_offset_probe(_p(om), B, om.shape[2], om.shape[3], dg, _p(probe), _stream()), 'dcn_offset_probe')
    torch.cuda.synchronize()
    return probe.cpu().tolist()


def _raw_backward(case, tensors, gout, act_out):
    """One rvsr_dcn_pack_backward call (stride 1, no probe handed over) on GPU tensors x, om, w, b: the exported plan row of that very
    call, and grad_input / grad_om / grad_weight / grad_bias."""
    from realvsr_amd import _lib
    from realvsr_amd._lib import _p, _stream
    B, C, Co, dg, H, W = case
    x, om, w, b = tensors
    gx, gw, gb, gom = torch.zeros_like(x), torch.zeros_like(w), torch.zeros_like(b), torch.empty_like(om)
    L = _lib.lib()
    nbytes = L.rvsr_modulated_deform_conv_backward_workspace_bytes(B, C, H, W, Co, 1, 1, 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    args = (_p(x), _p(w), _p(om), _p(gout), _p(act_out), SLOPE, _p(gx), _p(gw), _p(gb), _p(gom), B, C, H, W, Co, 1, 1, 1, dg, None, _p(ws), nbytes)
    row = (ctypes.c_longlong * 41)()
    assert L.rvsr_dcn_pack_backward_plan(*args, row) == 0
    _lib.check(L.rvsr_dcn_pack_backward(*args, _stream()), 'dcn_pack_backward')
    torch.cuda.synchronize()
    return dict(zip(DL._BWD_ROW, row)), [gx, gom, gw, gb]


# ---- halo matrix
@pytest.mark.parametrize('Co,regime', HALO_CASES, ids=lambda v: str(v))
def test_halo_matrix(Co, regime, bf16x3):
    """Every dcn_bwdin6<NK, R> and dcn_fwd3<MT, R>, LeakyReLU 0.1 and a bias: the probe's counters against the host restatement, the node
    with gradients (3 px forward tile, backward window selected on the device from the handed-over probe), a second forward on the same
    weight (tile from the recorded counters, as a hint), and the node under no_grad (tile selected on the device)."""
    from realvsr_amd import functional as RF
    case, inputs = halo_case(Co), halo_inputs(Co, regime)
    want_bwd, want_fwd = halo_expected(Co, regime)
    counters = halo_counters(Co, regime)
    got_counters = _gpu_counters(inputs[1].to(dev()), case)
    assert got_counters[:6] == counters and got_counters[6:] == [0, 0], (got_counters, counters)
    # the variants, from the plan rows and the counters
    (_, fcall), (_, bcall) = DL.node_calls(case, 'lrelu')
    fkey = DL.keys_of(fcall, 'bf16x3')[0][1]
    ikey, wkey = [k for _, k in DL.keys_of(bcall, 'bf16x3', counters)]
    nkey = DL.keys_of(DL.node_calls(case, 'lrelu', no_grad=True)[0][1], 'bf16x3', counters)[0][1]
    hkey = DL.keys_of(DL.node_calls(case, 'lrelu', hint=want_fwd)[0][1], 'bf16x3')[0][1]
    print('forward %s\ninput gradient %s\nweight gradient %s\nforward (no_grad) %s\nforward (hint) %s' % (fkey, ikey, wkey, nkey, hkey))
    nk, mt = {16: (1, 1), 32: (2, 1), 64: (4, 2), 128: (8, 4)}[Co]
    assert fkey[:2] == ('dcn_fwd3', mt) and fkey[4:6] == (3, 'fixed')
    assert ikey[:2] == ('dcn_bwdin6', nk) and ikey[4] == want_bwd and ikey[5:] == (True, False, True)
    assert wkey[0] == 'dcn_bwdw6'
    assert nkey[:2] == ('dcn_fwd3', mt) and nkey[4:6] == (want_fwd, 'device')
    assert hkey[:2] == ('dcn_fwd3', mt) and hkey[4:6] == (want_fwd, 'hint')
    r = _halo_reference(Co, regime, 'lrelu')
    tag = 'halo Co%d %s' % (Co, regime)
    out, grads, leaves = _run_node(inputs, case, 'lrelu', r['gout'])
    _check_all(tag, r, out, grads, 'bf16x3', {'forward': fkey, 'input gradient': ikey, 'weight gradient': wkey})
    # the counters of that backward are this layer's record: the next forward on the same weight takes its tile from them
    assert RF.dcn_offset_stats.forward_halo(leaves[2], Co) == want_fwd
    out2 = RF.dcn_pack(*leaves, 1, 1, 1, case[3], act=RF.ACT_LRELU, slope=SLOPE)
    out3 = RF.dcn_pack(*leaves, 1, 1, 1, case[3], act=RF.ACT_NONE)
    torch.cuda.synchronize()
    _check_all(tag + ' hint', r, out2, None, 'bf16x3', {'forward': hkey})
    _check_all(tag + ' no_grad', r, _run_no_grad(inputs, case, 'lrelu'), None, 'bf16x3', {'forward': nkey})
    # (the same two tiles without the epilogue: the reference's pre-activation)
    plain = lambda k: ('bf16x3', 'forward', k[:-1] + ('none',), 'out')   # noqa: E731
    check3(tag + ' hint, no activation', out3, r['z'], TOL['bf16x3'], key=plain(hkey))
    check3(tag + ' no_grad, no activation', _run_no_grad(inputs, case, 'none'), r['z'], TOL['bf16x3'], key=plain(nkey))
    # the same backward through the raw ABI without a probe: dcn_bwdin6 counts the offsets itself, with act'
    row, raw = _raw_backward(case, [t.detach() for t in leaves], r['gout'].to(dev()), out.detach())
    assert (row['in_family'], row['own_probe'], row['ncand'], row['handoff'], row['w_family']) == (1, 1, 4 if nk == 8 else 5, 1, 1), row
    _check_all(tag + ' raw, own probe', r, None, raw, 'bf16x3', _keys([('raw', DL.bwd_call(*case, act_out=True))], 'bf16x3', counters))


@pytest.mark.parametrize('Co,regime', HALO_CASES, ids=lambda v: str(v))
def test_halo_matrix_without_activation(Co, regime, bf16x3):
    """The same windows without act': the node (probe handed over) and archs.dcn.modulated_deform_conv (no probe: dcn_bwdin6 counts the
    offsets itself) on the halo-matrix inputs."""
    from realvsr_amd.archs.dcn import modulated_deform_conv
    case, inputs = halo_case(Co), halo_inputs(Co, regime)
    x, om, w, b, gout = inputs
    dg = case[3]
    counters = halo_counters(Co, regime)
    want_bwd = halo_expected(Co, regime)[0]
    nkey = DL.keys_of(DL.node_calls(case, 'none')[1][1], 'bf16x3', counters)[0][1]
    ikey = DL.keys_of(DL.operator_calls(case)[1][1], 'bf16x3', counters)[0][1]
    print('input gradient: node %s, operator %s' % (nkey, ikey))
    assert nkey[0] == 'dcn_bwdin6' and nkey[4] == want_bwd and nkey[5:] == (True, False, False)
    assert ikey[0] == 'dcn_bwdin6' and ikey[4] == want_bwd and ikey[5:] == (True, True, False)
    r = _halo_reference(Co, regime, 'none')
    out, grads, _ = _run_node(inputs, case, 'none', r['gout'])
    _check_all('halo Co%d %s none' % (Co, regime), r, out, grads, 'bf16x3', _keys(DL.node_calls(case, 'none'), 'bf16x3', counters))
    d = dev()
    leaves = [t.to(d).requires_grad_(True) for t in (x, om, w, b)]
    out = modulated_deform_conv(leaves[0], leaves[1][:, :18 * dg].contiguous(), torch.sigmoid(leaves[1][:, 18 * dg:]), leaves[2], leaves[3],
                                1, 1, 1, 1, dg)
    out.backward(gout.to(d))
    torch.cuda.synchronize()
    _check_all('operator Co%d %s' % (Co, regime), r, out, [t.grad for t in leaves], 'bf16x3', _keys(DL.operator_calls(case), 'bf16x3', counters))


# ---- node matrix
@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('act', NODE_ACTS)
@pytest.mark.parametrize('entry', NODE_CASES, ids=lambda e: '%s+%d' % (_name(e[0]), e[1]))
def test_node_matrix(entry, act, with_bias, gemm_mode):
    """Forward and all gradients of the node per kernel family and gOut staging, with each activation, with and without a bias."""
    case, g_off, families = entry
    counters = node_counters(case)
    (_, fcall), (_, bcall) = DL.node_calls(case, act, g_off)
    fkey = DL.keys_of(fcall, gemm_mode, counters)[0][1]
    ikey, wkey = [k for _, k in DL.keys_of(bcall, gemm_mode, counters)]
    print('forward %s\ninput gradient %s\nweight gradient %s' % (fkey, ikey, wkey))
    if gemm_mode == 'bf16x3':
        assert (fkey[0], ikey[0], wkey[0], wkey[3]) == families, (fkey, ikey, wkey)
    else:   # exact f32: dcn_fwd_kernel<mt, 8 | 0>, dcn_bwd_input_kernel, dcn_bwdw2 / dcn_bwd_weight_kernel
        c8 = (case[1] // case[3]) % 8 == 0
        assert (fkey[0], fkey[2], ikey[0], wkey[0]) == ('dcn_fwd1', 8 if c8 else 0, 'dcn_bwd_input', 'dcn_bwdw2' if c8 else 'dcn_bwd_weight')
    assert ikey[-1] == wkey[4] == (act != 'none')
    r = _node_reference(case, with_bias, act)
    inputs = node_inputs(case, with_bias)
    out, grads, _ = _run_node(inputs, case, act, r['gout'], g_off)
    _check_all('node %s+%d %s' % (_name(case), g_off, act), r, out, grads, gemm_mode, {'forward': fkey, 'input gradient': ikey, 'weight gradient': wkey})


@pytest.mark.parametrize('entry', LEDGER_CASES, ids=lambda e: '%s+%d-%s' % (_name(e[0]), e[1], e[2]))
def test_ledger_cases(entry, gemm_mode):
    """The cases added for a ledger key: forward and all gradients, with a bias."""
    case, g_off, act = entry
    counters = node_counters(case)
    keys = _keys(DL.node_calls(case, act, g_off), gemm_mode, counters)
    print('\n'.join('%s %s' % lk for lk in keys.items()))
    r = _node_reference(case, True, act)
    out, grads, _ = _run_node(node_inputs(case, True), case, act, r['gout'], g_off)
    _check_all(ledger_case_name(case, g_off, act), r, out, grads, gemm_mode, keys)


# ---- sink
@pytest.mark.parametrize('case', SINK_CASES, ids=_name)
def test_sink_deposit(case, bf16x3):
    """grad_input is ADDED into what a GradSink already holds (dcn_bwdin6's flush and beyond-window atomics, dcn_bwd_input_kernel);
    x.grad is None, the other gradients are those of a run without a sink; a closed sink leaves the gradient to autograd."""
    from realvsr_amd import functional as RF
    inputs = node_inputs(case, True)
    r = _node_reference(case, True, 'lrelu')
    tag = 'sink %s' % _name(case)
    _, plain, _ = _run_node(inputs, case, 'lrelu', r['gout'])
    D = torch.randn(inputs[0].shape, generator=torch.Generator().manual_seed(77)) * r['gx'].std().float()
    leaves = [t.to(dev()).requires_grad_(True) for t in inputs[:4]]
    sink = RF.GradSink()
    sink.get(leaves[0]).copy_(D)
    buf = sink.buf
    out, grads, _ = _run_node(inputs, case, 'lrelu', r['gout'], sink=sink, leaves=leaves)
    assert grads[0] is None and sink.buf is buf and not sink.closed
    _, tol_g = _tols('bf16x3')
    check3(tag + ' deposit - D', buf.detach().cpu().double() - D.double(), r['gx'], tol_g)
    _check_all(tag, r, out, [None] + grads[1:], 'bf16x3')
    for name, a, p in zip(('grad_om', 'grad_weight', 'grad_bias'), grads[1:], plain[1:]):
        assert torch.equal(a, p), '%s %s changed with a sink: max |diff| %.3e' % (tag, name, (a - p).abs().max().item())
    closed = RF.GradSink()
    closed.close()
    out, grads, _ = _run_node(inputs, case, 'lrelu', r['gout'], sink=closed, leaves=leaves)
    assert grads[0] is not None and closed.buf is None
    _check_all(tag + ' closed', r, out, grads, 'bf16x3')


# ---- raw ABI
def test_raw_backward_with_act_out_off_a_16_byte_boundary(bf16x3):
    """The node allocates act_out aligned; through the raw ABI it sits 4 bytes off: the plan of that very call names dcn_bwdw2 (scalar
    staging of gOut and act'), and the gradients match."""
    case = RAW_CASE
    inputs = node_inputs(case, True)
    r = _node_reference(case, True, 'lrelu')
    d = dev()
    act_out = _off_by(_run_no_grad(inputs, case, 'lrelu'), 1)
    gout = r['gout'].to(d)
    assert gout.data_ptr() % 16 == 0
    row, grads = _raw_backward(case, [t.to(d) for t in inputs[:4]], gout, act_out)
    assert (DL.IN_FAMILY[row['in_family']], DL.W_FAMILY[row['w_family']]) == ('dcn_bwd_input', 'dcn_bwdw2'), row
    assert DL.keys_of(DL.bwd_call(*case, act_out=True, act_off=1), 'bf16x3')[1][1][:4] == ('dcn_bwdw2', 3, 0, False)
    _check_all('raw act_out+1', r, None, grads, 'bf16x3', _keys([('raw', DL.bwd_call(*case, act_out=True, act_off=1))], 'bf16x3', None))
