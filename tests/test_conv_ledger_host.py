"""The coverage ledger of the conv kernels: every kernel variant the plan (csrc/conv_plan.h) can pick over a sweep of the call space is
reached by at least one case of the GPU suite.  No GPU: the calls of each case are worked out by tests/conv_ledger.py and the library's
plan queries answer which kernel each would run (needs the built library, like the other plan tests).

Five ledgers per GEMM mode (bf16x3, f32) -- forward kernel, forward epilogue, conv_fwd5 staging, weight gradient, and the fallbacks
for a misaligned pointer -- and the forward-kernel ledger for the speed modes.  Each prints as a table, key -> first case that reaches
it; a failure names the keys no case reaches.  What the ledger does not see: rules that need a tensor of 2 GB or more (DESIGN.md,
oracle pinning)."""
import itertools

import pytest

import conv_ledger as CL

# ---- the call space.  A superset of: C1 3..128, C2 0/16/64, Co 1..136, k 1/3, stride 1/2, act, residual, PixelShuffle, H 8/9/16,
# W 30/36/64/68, inputs and outputs on / 4 bytes off a 16-byte boundary.
_C1 = (3, 8, 16, 24, 64, 72, 128)
_C2 = (0, 16, 64)
_CO = (1, 4, 12, 32, 64, 80, 136)
_H = (8, 9, 16)
_W = (30, 36, 64, 68)
_MASK_FRAMES = tuple(itertools.product(_H, _W)) + ((7, 64), (17, 60), (16, 40), (16, 24), (8, 62))


def _sweep_cases():
    for C1, C2, Co, k, stride, act, res, ps, H, W in itertools.product(_C1, _C2, _CO, (1, 3), (1, 2), ('none', 'lrelu'), (False, True),
                                                                       (False, True), _H, _W):
        if (k == 1 and stride == 2) or (ps and (stride == 2 or res or Co % 4)):
            continue   # (not calls: stride 2 is for 3x3 / 5x5, PixelShuffle takes 4 k channels, no residual, stride 1)
        yield (C1, C2, Co, k, stride, act, res, ps, 1, H, W)


def _raw_variants(calls):
    """What only the raw C ABI reaches: the output buffer itself 4 bytes off (the nodes allocate their outputs)."""
    for name, call in calls:
        if 'Gh' not in call:
            yield name + ' out+4', dict(call, out_off=1, out2_off=1 if call['Co2'] else 0)


def _mask_nodes():
    """res_block and premask pairs over the sweep's frames, B 1 / 2, 16 and 64 channels; conv_cat_bcast as producer."""
    for (H, W), B, C in itertools.product(_MASK_FRAMES, (1, 2), (16, 64)):
        yield ('res_block', C, B, H, W)
        for cact, cres in (('none', False), ('lrelu', False), ('none', True)):
            cons = (C, 0, C, 3, 1, cact, cres, False, B, H, W)
            yield ('pair', ((C, 0, C, 3, 1, 'lrelu', False, False, B, H, W), cons))
            yield ('pair', ((C, C, C, 3, 1, 'lrelu', False, False, B, H, W), cons))
            yield ('pair', (('bcast', C, C, C, 'lrelu', 3, B, H, W, None, None), cons))
        if H % 2 == 0 and W % 2 == 0:
            yield ('pair', ((C, 0, 4 * C, 3, 1, 'lrelu', False, True, B, H // 2, W // 2), (C, 0, C, 3, 1, 'lrelu', False, False, B, H, W)))


def _node_calls(node, mode):
    kind = node[0]
    if kind == 'res_block':
        return CL.res_block_calls(*node[1:], mode=mode)
    if kind == 'pair':
        return CL.premask_pair_calls(node[1], mode=mode)
    if kind == 'bcast':
        return CL.cat_bcast_calls(node[1:])
    raise ValueError(kind)


def _conv5():
    from test_gpu_gan_ops import CONV5
    return CONV5


def _universe(mode, only=None):
    """Every key the plan returns over the sweep, in one GEMM mode.  only: a filter on block cases (the speed modes)."""
    from test_gpu_conv import RAW_LEDGER_CALLS
    got = None
    for case in _sweep_cases():
        if only is not None and not only(case):
            continue
        for (x_off, g_off), out_off in itertools.product(((0, 0), (1, 0), (0, 1), (1, 1)), (0, 1)):
            # the residual travels with the output offset: it is what a block case can move; the output buffer itself only the raw ABI
            calls = CL.calls_of(case, (x_off, x_off, g_off, out_off), mode)
            got = CL.collect(calls, mode, got)
            if out_off:
                got = CL.collect(_raw_variants(calls), mode, got)
    if only is None:
        for node in _mask_nodes():
            got = CL.collect(_node_calls(node, mode), mode, got)
        for case in _conv5():
            got = CL.collect(CL.conv5_calls(case), mode, got)
        # (act' on a strided or 5x5 forward conv has no caller in functional.py: the raw-ABI cases are its call space)
        got = CL.collect(RAW_LEDGER_CALLS, mode, got)
        got = CL.collect(_frame_node_calls(), mode, got)
    return got


_frame_calls = []


def _frame_node_calls():
    """The distinct calls of the frame-major nodes built from plain conv calls -- conv3d_frames, tsa_temporal_block,
    conv_transpose1x1 -- over their call space: T 1..5 with every frame range, N 1..7 with the centre first, middle and last, the
    channel counts of FSTRN and EDVR, frames from 5 x 7 to 8 x 64.  (They add no key: a node that starts issuing another call shows up
    as an unreached one.)"""
    if _frame_calls:
        return _frame_calls
    seen = set()

    def add(node, case, calls):
        for name, call in calls:
            if tuple(call.values()) not in seen:
                seen.add(tuple(call.values()))
                _frame_calls.append(('%s %s %s' % (node, _name(case), name), call))
    frames = ((5, 7), (8, 12), (9, 33), (8, 64))
    for (H, W), B in itertools.product(frames, (1, 2)):
        for Ci, Co in itertools.product((3, 16, 24, 32, 64), repeat=2):
            for T in range(1, 6):
                for f0, f1 in ((a, b) for a in range(T) for b in range(a + 1, T + 1)):
                    case = (T, f0, f1, B, Ci, Co, H, W, 3, True, False)
                    add('conv3d_frames', case, CL.conv3d_frames_calls(case))
            case = (3, 0, 3, B, Ci, Co, H, W, 1, True, True)
            add('conv3d_frames', case, CL.conv3d_frames_calls(case))
            add('conv_transpose1x1', (3 * B, Ci, Co, H, W), CL.conv_transpose1x1_calls((3 * B, Ci, Co, H, W)))
        for C, N in itertools.product((3, 16, 64), range(1, 8)):
            for center in sorted({0, N // 2, N - 1}):
                add('tsa_temporal_block', (N, center, B, C, H, W), CL.tsa_block_calls((N, center, B, C, H, W)))
    return _frame_calls


def _name(case):
    return '-'.join(str(v) for v in case) if isinstance(case, tuple) else str(case)


def _block_lists():
    """(test, cases with offsets) of every GPU list of block cases."""
    from test_gpu_conv import CASES, _random_cases
    from test_gpu_conv_ledger import LEDGER_CASES
    from test_gpu_conv_smallk import CASES as SMALLK
    zero = (0, 0, 0, 0)
    return [('test_gpu_conv', [(c, zero) for c in CASES]), ('test_gpu_conv random', [(c, zero) for c in _random_cases(36, 20260928)]),
            ('test_gpu_conv_smallk', [(c, zero) for c in SMALLK]), ('test_gpu_conv_ledger', list(LEDGER_CASES))]


def _reached(mode, drop=None):
    """What the GPU case lists reach in one GEMM mode.  drop: the name(s) of cases to leave out (test_a_dropped_case_is_named)."""
    from test_gpu_conv import RAW_LEDGER_CALLS
    from test_gpu_conv_nodes import BCAST_CASES, PAIRS, RES_BLOCKS
    got = CL.collect([], mode)
    dropped = lambda name: name == drop if isinstance(drop, str) else name in (drop or ())   # noqa: E731
    for test, cases in _block_lists():
        for case, offsets in cases:
            name = '%s %s%s' % (test, _name(case), '' if not any(offsets) else ' +%s' % (offsets,))
            if not dropped(name):
                got = CL.collect([(name, c) for _, c in CL.calls_of(case, offsets, mode)], mode, got)
    for case in _conv5():
        name = 'test_gpu_gan_ops ' + _name(case)
        got = CL.collect([(name, c) for _, c in CL.conv5_calls(case)], mode, got)
    for node in [('res_block',) + tuple(c) for c in RES_BLOCKS] + [('pair', p) for p in PAIRS] + [('bcast',) + tuple(c) for c in BCAST_CASES]:
        name = 'test_gpu_conv_nodes %s %s' % (node[0], _name(node[1]) if node[0] == 'pair' else _name(node[1:]))
        if not dropped(name):
            got = CL.collect([(name, c) for _, c in _node_calls(node, mode)], mode, got)
    got = CL.collect([('test_gpu_conv raw ' + n, c) for n, c in RAW_LEDGER_CALLS if not dropped('test_gpu_conv raw ' + n)], mode, got)
    return got


# key -> one line on why no small shape reaches it; at most 5 % of a ledger's keys
EXEMPT = {name: {} for name in CL.LEDGERS}


def _missing(universe, reached, ledgers=CL.LEDGERS):
    return {name: sorted(k for k in universe[name] if k not in reached[name] and k not in EXEMPT[name]) for name in ledgers}


def _print_table(mode, universe, reached, ledgers=CL.LEDGERS):
    for name in ledgers:
        print('\n%s ledger, %s: %d keys' % (name, mode, len(universe[name])))
        for key in sorted(universe[name], key=repr):
            print('  %-60s %s' % (key, reached[name].get(key, 'EXEMPT: ' + EXEMPT[name][key] if key in EXEMPT[name] else '-- NOT REACHED --')))


@pytest.mark.parametrize('mode', ['bf16x3', 'f32'])
def test_every_conv_kernel_variant_is_reached(mode):
    universe, reached = _universe(mode), _reached(mode)
    _print_table(mode, universe, reached)
    for name in CL.LEDGERS:
        assert len(EXEMPT[name]) <= 0.05 * len(universe[name]), 'too many exemptions in the %s ledger' % name
        assert all(k in universe[name] for k in EXEMPT[name]), 'an exemption of the %s ledger is no key of it' % name
    missing = _missing(universe, reached)
    assert not any(missing.values()), 'no GPU case reaches: %s' % {k: v for k, v in missing.items() if v}


def _speed_filter(c):
    return c[3] == 3 and c[4] == 1 and c[2] > 32


@pytest.mark.parametrize('mode', ['bf16x2', 'bf16', 'f16fp8'])
def test_every_forward_kernel_is_reached_in_the_speed_modes(mode):
    """The 3x3 / stride-1 blocks with more than 32 output channels (the kernels the speed modes act in): the forward-kernel ledger over
    the cases tests/test_gpu_modes.py runs in those modes."""
    from test_gpu_modes import _speed_mode_conv_cases, _speed_mode_ledger_cases
    universe = _universe(mode, only=_speed_filter)
    reached = None
    for case, offsets in [(c, (0, 0, 0, 0)) for c in _speed_mode_conv_cases()] + _speed_mode_ledger_cases():
        name = 'test_gpu_modes %s%s' % (_name(case), '' if not any(offsets) else ' +%s' % (offsets,))
        reached = CL.collect([(name, c) for _, c in CL.calls_of(case, offsets, mode)], mode, reached)
    _print_table(mode, universe, reached, ('forward kernel',))
    missing = _missing(universe, reached, ('forward kernel',))
    assert not any(missing.values()), 'no speed-mode case reaches: %s' % missing


def _new_case_names():
    """The names `_reached` gives the cases this ledger was filled with, and those that are there for a combination the keys cannot tell."""
    from test_gpu_conv import RAW_LEDGER_CALLS
    from test_gpu_conv_ledger import LEDGER_CASES, NOT_SOLE
    from test_gpu_conv_nodes import BCAST_CASES, PAIRS, RES_BLOCKS
    names = ['test_gpu_conv_ledger %s%s' % (_name(c), '' if not any(o) else ' +%s' % (o,)) for c, o in LEDGER_CASES if (c, o) not in NOT_SOLE]
    assert all(v in LEDGER_CASES for v in NOT_SOLE)
    names += ['test_gpu_conv raw ' + n for n, _ in RAW_LEDGER_CALLS if n not in ('out+res off', 'act 5x5')]   # (those two: the issue's own list)
    nodes = ['test_gpu_conv_nodes res_block ' + _name(tuple(c)) for c in RES_BLOCKS] + ['test_gpu_conv_nodes pair ' + _name(p) for p in PAIRS] + \
        ['test_gpu_conv_nodes bcast ' + _name(tuple(c)) for c in BCAST_CASES]
    return names, nodes


def test_a_dropped_case_is_named():
    """Leaving out any one block or raw-ABI case that was added for the ledger loses a key in one of the two modes, and the ledger names
    it; so does leaving out every node case on a frame the mask epilogue takes.  (The node cases are there for their values -- taken and
    untaken frames, sinks -- and share most keys.)"""
    names, nodes = _new_case_names()
    universe = {mode: _universe(mode) for mode in ('bf16x3', 'f32')}
    full = {mode: _reached(mode) for mode in universe}
    assert all(not any(_missing(universe[mode], full[mode]).values()) for mode in universe)
    for name in names:
        lost = {mode: _missing(universe[mode], _reached(mode, drop=name)) for mode in universe}
        assert any(any(m.values()) for m in lost.values()), 'no key is lost without %s' % name
        print('%-90s %s' % (name, [k for m in lost.values() for keys in m.values() for k in keys][:2]))
    lost = _missing(universe['bf16x3'], _reached('bf16x3', drop=nodes))
    assert ('fwd5', 3, 1, 1, 'mask', 1) in lost['forward epilogue'], lost


# ---- residual == out1: every kernel variant that can carry a residual runs once in place (tests/test_gpu_conv_inplace.py)
def _residual_universe(mode):
    """{key: first call that gives it} over every call of the sweep above that carries a residual (the mask epilogue apart)."""
    got = {}

    def add(named_calls):
        for name, call in named_calls:
            if 'Gh' in call or not call['res'] or call['act'] == CL.ACT_MASK:
                continue
            rc, row = CL.fwd_plan(call, mode)
            assert rc == 0, (call, rc)
            got.setdefault(CL.residual_epilogue_key(call, row), call)
    for case in _sweep_cases():
        for (x_off, g_off), out_off in itertools.product(((0, 0), (1, 0), (0, 1), (1, 1)), (0, 1)):
            calls = CL.calls_of(case, (x_off, x_off, g_off, out_off), mode)
            add(calls)
            if out_off:
                add(_raw_variants(calls))
    for node in _mask_nodes():
        add(_node_calls(node, mode))
    return got


# key -> why no in-place case reaches it; at most 5 %
INPLACE_EXEMPT = {'bf16x3': {}, 'f32': {}}


@pytest.mark.parametrize('mode', ['bf16x3', 'f32'])
def test_every_residual_epilogue_runs_in_place(mode):
    """(forward kernel, 16-byte stores, output / residual off the boundary) of every residual-carrying call of the sweep is the key of
    an INPLACE_CASES entry, which test_gpu_conv_inplace.py runs with the residual being the output buffer."""
    from test_gpu_conv_inplace import INPLACE_CASES
    universe = _residual_universe(mode)
    reached = {}
    for case in INPLACE_CASES:
        call = CL.inplace_call(case)
        rc, row = CL.fwd_plan(call, mode)
        assert rc == 0, (case, rc)
        reached.setdefault(CL.residual_epilogue_key(call, row), case)
    exempt = INPLACE_EXEMPT[mode]
    print('\nresidual epilogues that run in place, %s: %d keys' % (mode, len(universe)))
    for key in sorted(universe, key=repr):
        print('  %-70s %s' % (key, reached.get(key, 'EXEMPT: ' + exempt[key] if key in exempt else '-- NOT REACHED --')))
    assert len(universe) >= 20   # (46 in bf16x3 mode, 21 in f32 mode when this was written)
    assert len(exempt) <= 0.05 * len(universe) and all(k in universe for k in exempt)
    missing = sorted((k for k in universe if k not in reached and k not in exempt), key=repr)
    assert not missing, 'no in-place case reaches: %s' % missing


def test_the_frames_of_the_mask_epilogue():
    """The frame lists of tests/test_gpu_conv_nodes.py against the plan's formula: 64 -> 64 channels, aligned tensors."""
    from realvsr_amd import functional as RF
    from test_gpu_conv_nodes import NOT_TAKEN, TAKEN
    assert all(RF.grad_mask_fusable(H, W) is True for H, W in TAKEN), [hw for hw in TAKEN if not RF.grad_mask_fusable(*hw)]
    assert all(RF.grad_mask_fusable(H, W) is False for H, W in NOT_TAKEN), [hw for hw in NOT_TAKEN if RF.grad_mask_fusable(*hw)]
