"""The coverage ledger of the DCN kernels: every kernel variant the plan (csrc/dcn_plan.h) can pick over a sweep of the call space is
reached by at least one case of the GPU suite.  No GPU: the calls of each case are worked out by tests/dcn_ledger.py, the library's plan
queries answer which kernels each would launch (needs the built library, like the other plan tests), and where the DEVICE selects among
several launches from the offset counters, the counters are computed from the case's own offsets (a numpy restatement of
dcn_offset_probe2_kernel, held against the kernel by tests/test_gpu_dcn_pack_node.py) and the rule of dcn_cand_selected is applied on the
host; exactly one candidate must be selected.

Three ledgers per GEMM mode (bf16x3, f32): forward (family, mt, chs, nt, halo, how the halo is chosen, activation), input gradient
(family, nk, in_nt, chs, halo, hand-off written, own probe, act') and weight gradient (family, w_nt, w_th, 16-byte gOut staging, act',
nmb > 1, gy > 1, gz > 1, P or ns > 1).  Each prints as a table, key -> first case that reaches it; a failure names the keys no case
reaches.  What the ledger does not see: rules that need a tensor of 2 GB or more, more than 256 dcn_bwdw6 units, the speed modes
(bf16x2, bf16, f16fp8) and the developer switches (tests/test_gpu_switches.py forces those in subprocesses)."""
import functools
import itertools

import pytest
import torch

import dcn_ledger as DL

MODES = ('bf16x3', 'f32')
_C = (8, 16, 64, 128)
_CO = (8, 16, 32, 64, 72, 128, 130)
_CPG = (4, 8, 16)
_FRAMES = ((8, 32), (7, 30), (20, 68))
_ACTS = ('none', 'lrelu')   # with and without act_out (ReLU differs from LeakyReLU in the slope value only)


def _universe(mode):
    """Every key the plans return over the sweep, under every selection a plan allows (every candidate halo)."""
    got = {name: {} for name in DL.LEDGERS}
    for C, Co, cpg, stride, dil, (H, W), B in itertools.product(_C, _CO, _CPG, (1, 2), (1, 2), _FRAMES, (1, 2)):
        if C % cpg:
            continue
        geom = dict(stride=stride, dil=dil)
        calls = [DL.fwd_call(B, C, Co, C // cpg, H, W, act=act, probe=probe, hint=hint, **geom)
                 for act, (probe, hint) in itertools.product(_ACTS, ((False, 0), (True, 0), (False, 3), (False, 7), (False, 11)))]
        calls += [DL.bwd_call(B, C, Co, C // cpg, H, W, act_out=act, g_off=g_off, probe=probe, **geom)
                  for act, g_off, probe in itertools.product((False, True), (0, 1), (False, True))]
        for call in calls:
            for ledger, key in DL.universe_keys_of(call, mode):
                got[ledger].setdefault(key, call)
    return got


def _name(case):
    return '-'.join(str(v) for v in case)


@functools.lru_cache(maxsize=None)
def _operator_lists():
    """(name, call, counters) of the operator cases of test_gpu_dcn.py (its inputs regenerated: x first, then the offsets)."""
    from test_gpu_dcn import FAMILY_CASES, SHAPES, _random_shapes
    out = []
    for test, shapes in (('test_gpu_dcn shape', SHAPES), ('test_gpu_dcn sweep', _random_shapes(14, 928))):
        for shape in shapes:
            B, C, Co, dg, H, W, stride, pad, dil, ostd, _ = shape
            g = torch.Generator().manual_seed(sum(int(v) for v in shape[:9]))
            Ho, Wo = DL.out_size(H, W, stride, pad, dil)
            torch.randn(B, C, H, W, generator=g)
            cnt = DL.probe_counters((torch.randn(B, dg * 18, Ho, Wo, generator=g) * ostd).numpy())
            out += [('%s %s' % (test, _name(shape)), c, cnt) for _, c in DL.operator_calls((B, C, Co, dg, H, W, stride, dil))]
    for (B, C, Co, dg, H, W, stride), _ in FAMILY_CASES:
        g = torch.Generator().manual_seed(B + C + Co + dg + H + W + stride)
        Ho, Wo = DL.out_size(H, W, stride, 1, 1)
        cnt = DL.probe_counters((torch.randn(B, 27 * dg, Ho, Wo, generator=g)[:, :18 * dg] * 2.0).numpy())
        out += [('test_gpu_dcn family %s' % _name((B, C, Co, dg, H, W, stride)), c, cnt) for _, c in DL.node_calls((B, C, Co, dg, H, W, stride))]
    return out


def _reached(mode, drop=None):
    """What the GPU case lists reach in one GEMM mode.  drop: the name(s) of cases to leave out (test_a_dropped_case_is_named)."""
    from test_gpu_dcn_pack_node import ledger_calls
    return DL.collect([t for t in ledger_calls(mode) + _operator_lists() if t[0] not in ((drop,) if isinstance(drop, str) else drop or ())], mode)


# key -> one line on why no small shape reaches it; at most 5 % of a ledger's keys
EXEMPT = {mode: {name: {} for name in DL.LEDGERS} for mode in MODES}


def _missing(mode, universe, reached):
    return {name: sorted((k for k in universe[name] if k not in reached[name] and k not in EXEMPT[mode][name]), key=repr) for name in DL.LEDGERS}


def _print_table(mode, universe, reached):
    for name in DL.LEDGERS:
        print('\n%s ledger, %s: %d keys' % (name, mode, len(universe[name])))
        for key in sorted(universe[name], key=repr):
            ex = EXEMPT[mode][name]
            print('  %-84s %s' % (key, reached[name].get(key, 'EXEMPT: ' + ex[key] if key in ex else '-- NOT REACHED --')))


@pytest.mark.parametrize('mode', MODES)
def test_every_dcn_kernel_variant_is_reached(mode):
    universe, reached = _universe(mode), _reached(mode)
    _print_table(mode, universe, reached)
    for name in DL.LEDGERS:
        assert len(EXEMPT[mode][name]) <= 0.05 * len(universe[name]), 'too many exemptions in the %s ledger' % name
        assert all(k in universe[name] for k in EXEMPT[mode][name]), 'an exemption of the %s ledger is no key of it' % name
    missing = _missing(mode, universe, reached)
    assert not any(missing.values()), 'no GPU case reaches: %s' % {k: v for k, v in missing.items() if v}


def test_the_halo_matrix_selects_every_built_kernel():
    """The 20 halo-matrix cases: one candidate selected each time, the windows and tiles the case list states, and together all 19
    dcn_bwdin6<NK, R> and all 8 dcn_fwd3<MT, R> (the tables of dcn6_kernels.hip / dcn3_kernels.hip)."""
    import test_gpu_dcn_pack_node as T
    bwd, fwd = set(), set()
    for Co, regime in T.HALO_CASES:
        case, cnt = T.halo_case(Co), T.halo_counters(Co, regime)
        (_, bcall), = DL.node_calls(case, 'lrelu')[1:]
        (_, ncall), = DL.node_calls(case, 'lrelu', no_grad=True)
        ikey = DL.keys_of(bcall, 'bf16x3', cnt)[0][1]
        nkey = DL.keys_of(ncall, 'bf16x3', cnt)[0][1]
        n = DL.fwd_plan(ncall)[1]['nprobe']
        print('Co %3d %s: counters %s of %d, window %2d (NK %d), tile %2d (MT %d)' % (Co, regime, cnt, n, ikey[4], ikey[1], nkey[4], nkey[1]))
        assert (ikey[4], nkey[4]) == T.halo_expected(Co, regime)
        bwd.add((ikey[1], ikey[4]))
        fwd.add((nkey[1], nkey[4]))
    assert bwd == {(nk, r) for nk in (1, 2, 4, 8) for r in (2, 4, 5, 8, 12) if (nk, r) != (8, 12)} and len(bwd) == 19
    assert fwd == {(mt, r) for mt in (1, 2, 4) for r in (3, 7, 11) if (mt, r) != (4, 11)} and len(fwd) == 8


def test_probe_restatement_and_selection_rule():
    """probe_counters on a hand-made field (the sampled rows, strict '>'), and the selection of both plans at the edges of their thresholds."""
    off = torch.zeros(1, 18, 20, 4)
    off[0, 0, 8, 0], off[0, 0, 19, 1], off[0, 3, 8, 2], off[0, 5, 19, 3] = 2.5, -2.6, 100.0, -8.5   # rows 8 and min(24, 19)
    off[0, 1, 7] = 50.0    # (not a sampled row)
    assert DL.probe_counters(off.numpy()) == [3, 2, 2, 2, 1, 1]
    assert DL.probe_counters(torch.full((1, 18, 7, 5), 3.6).numpy()) == [90, 90, 0, 0, 0, 0]   # one row: min(8, 6)
    frow = DL.fwd_plan(DL.fwd_call(2, 16, 16, 2, 20, 68, probe=True))[1]
    n, cands = frow['nprobe'], DL.fwd_cands(frow)
    assert n == 2 * 36 * 2 * 68 and [c['halo'] for c in cands] == [3, 7, 11]
    thr3, thr7 = n * 8 // 100 + 1, n // 100 + 1
    assert DL.selected(cands, [n, thr3 - 1, 0, 0, 0, 0]) == 3 and DL.selected(cands, [n, thr3, 0, thr7 - 1, 0, 0]) == 7
    assert DL.selected(cands, [n, thr3, thr3, thr7, 0, 0]) == 11
    brow = DL.bwd_plan(DL.bwd_call(2, 16, 16, 2, 20, 68, probe=True))[1]
    cands, thr = DL.bwd_cands(brow), n * 2 // 100 + 1
    assert [c['halo'] for c in cands] == [2, 4, 5, 8, 12]
    for cnt, want in (([thr - 1, 0, 0, 0, 0, 0], 2), ([thr, thr - 1, 0, 0, 0, 0], 4), ([n, thr, thr - 1, 0, 0, 0], 5),
                      ([n, n, thr, thr, thr - 1, 0], 8), ([n, n, n, n, thr, 0], 12)):
        assert DL.selected(cands, cnt) == want
    for c in cands:
        assert DL.selected(cands, DL.counters_selecting(cands, c['halo'])) == c['halo']


# the two cases that select the same kernels (NK 8 has no 12 px window, MT 4 no 11 px tile): named when both go
SHARED = (('halo Co128 D', 'halo Co128 E'),)


def test_a_dropped_case_is_named():
    """Leaving out any one halo-matrix case, or any one case added for a ledger key, loses a key in one of the two modes, and the ledger
    names it.  (The node-matrix, sink and raw-ABI cases are there for their values -- activations, bias, deposits -- and share keys.)"""
    import test_gpu_dcn_pack_node as T
    universe = {mode: _universe(mode) for mode in MODES}
    full = {mode: _reached(mode) for mode in MODES}
    assert all(not any(_missing(mode, universe[mode], full[mode]).values()) for mode in MODES)
    names = ['halo Co%d %s' % cr for cr in T.HALO_CASES] + [T.ledger_case_name(*c) for c in T.LEDGER_CASES]
    drops = [n for n in names if not any(n in pair for pair in SHARED)] + list(SHARED)
    for drop in drops:
        lost = {mode: _missing(mode, universe[mode], _reached(mode, drop=drop)) for mode in MODES}
        keys = [k for m in lost.values() for ks in m.values() for k in ks]
        print('%-60s %s' % (drop, keys[:2]))
        assert keys, 'no key is lost without %s' % (drop,)
