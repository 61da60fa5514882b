"""Which DCN kernel variant a test case runs: the C-ABI calls of the fused DCN pack node, worked out from a case without a GPU, and the
ledger keys of the plan (csrc/dcn_plan.h) for each call.  Plain helper of test_dcn_ledger_host.py and of the GPU case lists
(tests/test_gpu_dcn_pack_node.py), modelled on tests/conv_ledger.py.

A *call* is a dict of what rvsr_dcn_pack_forward / rvsr_dcn_pack_backward look at apart from the data: sizes, the float offsets of x,
gout and act_out from a 16-byte boundary, and whether act_out, a probe and a halo hint are given.  `fwd_plan` / `bwd_plan` ask the
library's exported plan queries with made-up addresses.  Where a plan launches several candidates and the DEVICE selects one from the
offset counters, the selection is worked out here: `probe_counters` restates dcn_offset_probe2_kernel in numpy (the GPU file holds it
against the kernel's own counters: the drift guard) and `selected` applies the rule of dcn_cand_selected to the candidates of the plan
row; exactly one must be selected."""
import ctypes

import numpy as np

ACT = {'none': 0, 'relu': 1, 'lrelu': 2}
GEMM = {'bf16x3': 0, 'f32': 1, 'bf16x2': 2, 'bf16': 3}   # (the speed modes: tests/test_gpu_modes_definition.py asks for their term counts)
FWD_FAMILY = ('dcn_fwd3', 'dcn_fwd2', 'dcn_fwd1')
IN_FAMILY = ('none', 'dcn_bwdin6', 'dcn_bwd_input')
W_FAMILY = ('none', 'dcn_bwdw6', 'dcn_bwdw4', 'dcn_bwdw2', 'dcn_bwd_weight')
PROBE_LIMITS = (2.5, 3.5, 5.5, 7.5, 8.5, 11.5)
_A = 0x10000000   # 16-byte aligned; the plans dereference nothing

_FWD_ROW = ('family', 'MT', 'CHS', 'NT', 'pack', 'probe', 'nprobe', 'ncand') + tuple(
    '%s%d' % (k, i) for i in range(3) for k in ('halo', 'ge', 'lt', 'ge2', 'thr_ge', 'thr_lt', 'thr_ge2', 'lds')) + ('gx', 'gy', 'gz', 'lds')
_BWD_ROW = ('in_family', 'NK', 'in_NT', 'CHS', 'in_lds', 'own_probe', 'ncand') + tuple(
    '%s%d' % (k, i) for i in range(5) for k in ('halo', 'ge', 'lt', 'thr')) + ('handoff', 'handoff_off', 'w_family', 'R', 'TH', 'w_NT', 'ns', 'nmb',
                                                                               'xcd', 'P', 'Q', 'gy', 'gz', 'w_lds')


def out_size(H, W, stride, pad, dil):
    return (H + 2 * pad - (2 * dil + 1)) // stride + 1, (W + 2 * pad - (2 * dil + 1)) // stride + 1


def fwd_call(B, C, Co, dg, H, W, *, stride=1, dil=1, pad=None, act='none', x_off=0, probe=False, hint=0):
    """One rvsr_dcn_pack_forward call.  pad: the dilation unless given (what every architecture uses)."""
    return dict(dir='fwd', B=B, C=C, Co=Co, dg=dg, H=H, W=W, stride=stride, dil=dil, pad=dil if pad is None else pad, act=act, x_off=x_off % 4,
                probe=bool(probe), hint=hint)


def bwd_call(B, C, Co, dg, H, W, *, stride=1, dil=1, pad=None, act_out=False, g_off=0, act_off=0, probe=False):
    """One rvsr_dcn_pack_backward call with every gradient wanted."""
    return dict(dir='bwd', B=B, C=C, Co=Co, dg=dg, H=H, W=W, stride=stride, dil=dil, pad=dil if pad is None else pad, act_out=bool(act_out),
                g_off=g_off % 4, act_off=act_off % 4 if act_out else 0, probe=bool(probe))


# ---- the plans
_plans = {}


def _ptr(slot, off=0, on=True):
    return ctypes.c_void_p(_A + slot * 0x1000000 + 4 * off) if on else None


def fwd_plan(call, mode='bf16x3'):
    """(rc, plan row) of a forward call in a GEMM mode."""
    key = (mode,) + tuple(call.values())
    if key not in _plans:
        from realvsr_amd import _lib
        L = _lib.lib()
        c = call
        row = (ctypes.c_longlong * 36)(*([-7] * 36))
        need = L.rvsr_modulated_deform_conv_forward_workspace_bytes(c['C'], c['Co'])
        L.rvsr_set_gemm_mode_thread(GEMM[mode])
        try:
            rc = L.rvsr_dcn_pack_forward_plan(_ptr(1, c['x_off']), _ptr(2), _ptr(3), _ptr(4), _ptr(5), c['B'], c['C'], c['H'], c['W'], c['Co'],
                                              c['stride'], c['pad'], c['dil'], c['dg'], ACT[c['act']] | (c['hint'] << 10), 0.1,
                                              _ptr(6, on=c['probe']), _ptr(7), need, row)
        finally:
            L.rvsr_set_gemm_mode_thread(-1)
        _plans[key] = (rc, dict(zip(_FWD_ROW, row)))
    return _plans[key]


def bwd_plan(call, mode='bf16x3'):
    """(rc, plan row) of a backward call in a GEMM mode."""
    key = (mode,) + tuple(call.values())
    if key not in _plans:
        from realvsr_amd import _lib
        L = _lib.lib()
        c = call
        row = (ctypes.c_longlong * 41)(*([-7] * 41))
        need = L.rvsr_modulated_deform_conv_backward_workspace_bytes(c['B'], c['C'], c['H'], c['W'], c['Co'], c['stride'], c['pad'], c['dil'])
        L.rvsr_set_gemm_mode_thread(GEMM[mode])
        try:
            rc = L.rvsr_dcn_pack_backward_plan(_ptr(1), _ptr(2), _ptr(4), _ptr(5, c['g_off']), _ptr(8, c['act_off'], c['act_out']), 0.1, _ptr(9),
                                               _ptr(10), _ptr(11), _ptr(12), c['B'], c['C'], c['H'], c['W'], c['Co'], c['stride'], c['pad'],
                                               c['dil'], c['dg'], _ptr(6, on=c['probe']), _ptr(7), need, row)
        finally:
            L.rvsr_set_gemm_mode_thread(-1)
        _plans[key] = (rc, dict(zip(_BWD_ROW, row)))
    return _plans[key]


# ---- the device's selection, on the host
def probe_counters(offsets):
    """dcn_offset_probe2_kernel in numpy: rows min(16 r + 8, Ho - 1), r < ceil(Ho / 16), of every offset plane of `offsets`
    (B, 18 dg, Ho, Wo) -- the offset part of om -- and the counts of |v| > 2.5 / 3.5 / 5.5 / 7.5 / 8.5 / 11.5 in float32."""
    off = np.asarray(offsets, dtype=np.float32)
    Ho = off.shape[2]
    rows = [min(16 * r + 8, Ho - 1) for r in range((Ho + 15) // 16)]
    v = np.abs(off[:, :, rows, :])
    return [int((v > np.float32(lim)).sum()) for lim in PROBE_LIMITS]


def fwd_cands(row):
    return [dict(halo=row['halo%d' % k], ge=row['ge%d' % k], lt=row['lt%d' % k], ge2=row['ge2%d' % k], thr_ge=row['thr_ge%d' % k],
                 thr_lt=row['thr_lt%d' % k], thr_ge2=row['thr_ge2%d' % k]) for k in range(row['ncand'])]


def bwd_cands(row):
    """(dcn_bwdin6's candidates share one threshold and have no second lower bound)"""
    return [dict(halo=row['halo%d' % k], ge=row['ge%d' % k], lt=row['lt%d' % k], ge2=-1, thr_ge=row['thr%d' % k], thr_lt=row['thr%d' % k],
                 thr_ge2=0) for k in range(row['ncand'])]


def cand_selected(c, cnt):
    """dcn_cand_selected (csrc/dcn_plan.h)."""
    return not (c['ge'] >= 0 and cnt[c['ge']] < c['thr_ge']) and not (c['ge2'] >= 0 and cnt[c['ge2']] < c['thr_ge2']) and \
        not (c['lt'] >= 0 and cnt[c['lt']] >= c['thr_lt'])


def selected(cands, counters):
    """The halo of the one candidate the device selects from these counters."""
    hit = [c['halo'] for c in cands if cand_selected(c, counters)]
    assert len(hit) == 1, 'the candidates %s select %s from the counters %s' % (cands, hit, counters)
    return hit[0]


def counters_selecting(cands, halo):
    """Some counter vector (monotone, as the probe's are) from which the device selects `halo`: the universe visits every candidate."""
    thr = max([1] + [c[k] for c in cands for k in ('thr_ge', 'thr_lt', 'thr_ge2')])
    for n in range(len(PROBE_LIMITS) + 1):     # the first n counters at the threshold, the rest zero
        cnt = [thr] * n + [0] * (len(PROBE_LIMITS) - n)
        if [c['halo'] for c in cands if cand_selected(c, cnt)] == [halo]:
            return cnt
    raise AssertionError('no monotone counter vector selects halo %d of %s' % (halo, cands))


# ---- ledger keys
LEDGERS = ('forward', 'input gradient', 'weight gradient')


def fwd_key(call, row, counters=None, mode='bf16x3'):
    """(family, mt, chs, nt, halo, how the halo was chosen: device / hint / fixed, activation)."""
    fam = FWD_FAMILY[row['family']]
    if fam != 'dcn_fwd3':
        return (fam, row['MT'], row['CHS'], row['NT'], 0, 'fixed', call['act'])
    if row['ncand'] > 1:
        assert counters is not None, 'a device-side selection needs the counters of the offsets'
        return (fam, row['MT'], row['CHS'], row['NT'], selected(fwd_cands(row), counters), 'device', call['act'])
    # the hint is honoured where two hints give two plans (the rule stays the plan's)
    how = 'hint' if call['hint'] and fwd_plan(dict(call, hint=3), mode)[1]['halo0'] != fwd_plan(dict(call, hint=11), mode)[1]['halo0'] else 'fixed'
    return (fam, row['MT'], row['CHS'], row['NT'], row['halo0'], how, call['act'])


def in_key(call, row, counters=None):
    """(family, nk, in_nt, chs, halo, hand-off written, own probe, act')."""
    fam = IN_FAMILY[row['in_family']]
    halo = 0
    if fam == 'dcn_bwdin6':
        assert row['ncand'] == 1 or counters is not None, 'a device-side selection needs the counters of the offsets'
        halo = row['halo0'] if row['ncand'] == 1 else selected(bwd_cands(row), counters)
    return (fam, row['NK'], row['in_NT'], row['CHS'], halo, bool(row['handoff']), bool(row['own_probe']), call['act_out'])


def w_key(call, row):
    """(family, w_nt, w_th, 16-byte gOut staging or not (None: the kernel has one staging), act', nmb > 1, gy > 1, gz > 1, P or ns > 1).
    The 16-byte staging of dcn_bwdw2_kernel also needs 4 | Wo (dcn2_kernels.hip); dcn_bwdw4 is only taken with it."""
    fam = W_FAMILY[row['w_family']]
    Wo = out_size(call['H'], call['W'], call['stride'], call['pad'], call['dil'])[1]
    al16 = not (call['g_off'] or call['act_off'])
    g16 = {'dcn_bwdw4': True, 'dcn_bwdw2': al16 and Wo % 4 == 0}.get(fam)
    return (fam, row['w_NT'], row['TH'], g16, call['act_out'], row['nmb'] > 1, row['gy'] > 1, row['gz'] > 1, max(row['P'], row['ns']) > 1)


def keys_of(call, mode, counters=None):
    """[(ledger name, key)] of one call.  counters: of the call's offsets, where the device selects."""
    if call['dir'] == 'fwd':
        rc, row = fwd_plan(call, mode)
        assert rc == 0, (call, rc)
        return [('forward', fwd_key(call, row, counters, mode))]
    rc, row = bwd_plan(call, mode)
    assert rc == 0, (call, rc)
    return [('input gradient', in_key(call, row, counters)), ('weight gradient', w_key(call, row))]


def universe_keys_of(call, mode):
    """The keys of one call under every selection its plan allows (every candidate halo)."""
    if call['dir'] == 'fwd':
        rc, row = fwd_plan(call, mode)
        assert rc == 0, (call, rc)
        cands = fwd_cands(row)
    else:
        rc, row = bwd_plan(call, mode)
        assert rc == 0, (call, rc)
        cands = bwd_cands(row) if row['in_family'] == 1 else []
    if len(cands) <= 1:
        return keys_of(call, mode)
    out = []
    for c in cands:
        out += keys_of(call, mode, counters_selecting(cands, c['halo']))
    return out


def collect(named, mode, into=None):
    """{ledger: {key: name of the first case that reaches it}} over (name, call, counters) triples."""
    into = {name: {} for name in LEDGERS} if into is None else into
    for name, call, counters in named:
        for ledger, key in keys_of(call, mode, counters):
            into[ledger].setdefault(key, name)
    return into


# ---- the calls of the node and of the operator
def node_calls(case, act='none', g_off=0, no_grad=False, hint=0):
    """[(what, call)] of functional.dcn_pack for case = (B, C, Co, dg, H, W[, stride[, dil]]): with gradients the forward takes a hint
    (DcnOffsetStats: 0 on a fresh weight) and the backward the counters of rvsr_dcn_offset_probe where 8 | channels per deformable
    group at stride 1 / dilation 1; under no_grad the forward gets a probe buffer at stride 1 / dilation 1."""
    B, C, Co, dg, H, W = case[:6]
    stride, dil = (tuple(case[6:]) + (1, 1))[:2]
    s1 = stride == 1 and dil == 1
    if no_grad:
        return [('forward (no_grad)', fwd_call(B, C, Co, dg, H, W, stride=stride, dil=dil, act=act, probe=s1))]
    return [('forward', fwd_call(B, C, Co, dg, H, W, stride=stride, dil=dil, act=act, hint=hint)),
            ('backward', bwd_call(B, C, Co, dg, H, W, stride=stride, dil=dil, act_out=act != 'none', g_off=g_off,
                                  probe=s1 and C % (8 * dg) == 0))]


def operator_calls(case):
    """[(what, call)] of archs.dcn.modulated_deform_conv: no activation, no probe (dcn_bwdin6 runs its own), no hint."""
    B, C, Co, dg, H, W = case[:6]
    stride, dil = (tuple(case[6:]) + (1, 1))[:2]
    return [('forward', fwd_call(B, C, Co, dg, H, W, stride=stride, dil=dil)), ('backward', bwd_call(B, C, Co, dg, H, W, stride=stride, dil=dil))]
