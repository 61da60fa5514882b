"""Which conv kernel variant a test case runs: the C-ABI calls of the fused conv nodes, worked out from a case without a GPU, and the
ledger keys of the plan (csrc/conv_plan.h) for each call.  Plain helper of test_conv_ledger_host.py and of the GPU case lists.

A *call* is a dict of what rvsr_conv2d_forward / rvsr_conv2d_backward_weight look at apart from the data: sizes, which optional tensors
are present, view modes, and the float offset of every pointer from a 16-byte boundary.  `calls_of` and its siblings restate what
realvsr_amd/functional.py issues for a node (the drift guard in test_gpu_conv_ledger.py records the real arguments and compares);
`fwd_plan` / `wgrad_plan` ask the library's exported plan queries with made-up addresses, as test_host_logic._conv_plan does."""
import ctypes

ACT = {'none': 0, 'relu': 1, 'lrelu': 2}
ACT_MASK = 3
GEMM = {'bf16x3': 0, 'f32': 1, 'bf16x2': 2, 'bf16': 3, 'f16fp8': 0}
FWD_FAMILY = ('thin', 'fwd5', 'fwd2', 'f32')
WGRAD_FAMILY = ('thin', 'wgrad2', 'wgrad5', 'f32_5', '1x1s', '1x1', 'f32_3s1', 's2', 'f32_3s2', 'f32_1', 'f32_7')
_A = 0x10000000   # 16-byte aligned; the plans dereference nothing

_FWD_KEYS = ('C1', 'C2', 'xact', 'in_mode', 'Hs', 'Ws', 'res', 'Co1', 'Co2', 'B', 'k', 'stride', 'w_mode', 'act', 'ps', 'Hout', 'Wout',
             'x_off', 'x2_off', 'xact_off', 'res_off', 'out_off', 'out2_off')
_WG_KEYS = ('C1', 'C2', 'H', 'W', 'gact', 'g_mode', 'Gh', 'Gw', 'Co', 'B', 'k', 'stride', 'Ho', 'Wo', 'x_off', 'x2_off', 'g_off', 'gact_off')


def fwd_call(C1, Co1, Hs, Ws, Hout, Wout, B, *, k=3, stride=1, C2=0, xact=False, in_mode=0, res=False, Co2=0, w_mode=0, act=0, ps=False,
             x_off=0, x2_off=0, xact_off=0, res_off=0, out_off=0, out2_off=0):
    """One rvsr_conv2d_forward call.  Offsets of absent tensors are zero, so that equal calls compare equal."""
    c = dict(C1=C1, C2=C2, xact=bool(xact), in_mode=in_mode, Hs=Hs, Ws=Ws, res=bool(res), Co1=Co1, Co2=Co2, B=B, k=k, stride=stride,
             w_mode=w_mode, act=act, ps=bool(ps), Hout=Hout, Wout=Wout, x_off=x_off % 4, x2_off=x2_off % 4 if C2 else 0,
             xact_off=xact_off % 4 if xact else 0, res_off=res_off % 4 if res else 0, out_off=out_off % 4, out2_off=out2_off % 4 if Co2 else 0)
    assert tuple(c) == _FWD_KEYS
    return c


def wgrad_call(C1, Co, H, W, Ho, Wo, B, *, k=3, stride=1, C2=0, gact=False, g_mode=0, x_off=0, x2_off=0, g_off=0, gact_off=0):
    """One rvsr_conv2d_backward_weight call."""
    Gh, Gw = (2 * Ho, 2 * Wo) if g_mode == 2 else (Ho, Wo)
    c = dict(C1=C1, C2=C2, H=H, W=W, gact=bool(gact), g_mode=g_mode, Gh=Gh, Gw=Gw, Co=Co, B=B, k=k, stride=stride, Ho=Ho, Wo=Wo,
             x_off=x_off % 4, x2_off=x2_off % 4 if C2 else 0, g_off=g_off % 4, gact_off=gact_off % 4 if gact else 0)
    assert tuple(c) == _WG_KEYS
    return c


# ---- the calls as functional._conv / functional._conv_wgrad see them (the drift guard wraps those two)
def _foff(t):
    return 0 if t is None else (t.data_ptr() % 16) // 4


def fwd_call_of_args(x1, weight, out1, *, what=None, x2=None, xact=None, xact_slope=0.0, in_mode=0, bias=None, residual=None, out2=None,
                     stride=1, transposed=False, act=0, slope=0.0, pixel_shuffle=False):
    """The call functional._conv makes for these arguments (same geometry rules as its first lines)."""
    C1, Hs, Ws = x1.shape[-3:]
    if in_mode == 2:
        C1 *= 4
    Co1, Hout, Wout = out1.shape[-3:]
    B = out1.numel() // (Co1 * Hout * Wout)
    if pixel_shuffle:
        Co1, Hout, Wout = Co1 * 4, Hout // 2, Wout // 2
    return fwd_call(C1, Co1, Hs, Ws, Hout, Wout, B, k=weight.shape[-1], stride=stride, C2=0 if x2 is None else x2.shape[-3],
                    xact=xact is not None, in_mode=in_mode, res=residual is not None, Co2=0 if out2 is None else out2.shape[-3],
                    w_mode=1 if transposed else 0, act=act, ps=pixel_shuffle, x_off=_foff(x1), x2_off=_foff(x2), xact_off=_foff(xact),
                    res_off=_foff(residual), out_off=_foff(out1), out2_off=_foff(out2))


def wgrad_call_of_args(x1, gout, gw, gb, *, what=None, x2=None, gact=None, gact_slope=0.0, pixel_shuffled=False, stride=1):
    """The call functional._conv_wgrad makes for these arguments."""
    C1, H, W = x1.shape[-3:]
    B = x1.numel() // (C1 * H * W)
    Gh, Gw = gout.shape[-2:]
    Ho, Wo = (Gh // 2, Gw // 2) if pixel_shuffled else (Gh, Gw)
    return wgrad_call(C1, gw.shape[0], H, W, Ho, Wo, B, k=gw.shape[-1], stride=stride, C2=0 if x2 is None else x2.shape[-3],
                      gact=gact is not None, g_mode=2 if pixel_shuffled else 0, x_off=_foff(x1), x2_off=_foff(x2), g_off=_foff(gout),
                      gact_off=_foff(gact))


# ---- the plans
_plans = {}


def _ptr(slot, off=0, on=True):
    return ctypes.c_void_p(_A + slot * 0x1000000 + 4 * off) if on else None


def fwd_plan(call, mode='bf16x3'):
    """(rc, plan row) of a forward call in a GEMM mode.  'f16fp8': the format flag where the plan grants it, as functional._conv asks."""
    key = ('f', mode) + tuple(call.values())
    if key in _plans:
        return _plans[key]
    from realvsr_amd import _lib
    L = _lib.lib()
    c = call
    row = (ctypes.c_int * 14)(*([-7] * 14))

    def ask(w_mode):
        return L.rvsr_conv2d_forward_plan(_ptr(1, c['x_off']), c['C1'], _ptr(2, c['x2_off'], c['C2']), c['C2'], _ptr(3, c['xact_off'], c['xact']),
                                          0.1, c['in_mode'], c['Hs'], c['Ws'], _ptr(4), _ptr(5), _ptr(6, c['res_off'], c['res']),
                                          _ptr(7, c['out_off']), c['Co1'], _ptr(8, c['out2_off'], c['Co2']), c['Co2'], c['B'], c['k'], c['stride'],
                                          w_mode, c['act'], 0.1, int(c['ps']), c['Hout'], c['Wout'], row)
    L.rvsr_set_gemm_mode_thread(GEMM[mode])
    try:
        rc = -1
        if mode == 'f16fp8':
            rc = ask(c['w_mode'] | 4)
        if rc != 0:
            rc = ask(c['w_mode'])
    finally:
        L.rvsr_set_gemm_mode_thread(-1)
    out = (rc, dict(zip(('family', 'MT', 'vec', 'wide', 'NT', 'act_in', 'CC', 'vec4', 'th', 'tw', 'gx', 'gy', 'gz', 'lds'), row)))
    _plans[key] = out
    return out


def wgrad_plan(call, mode='bf16x3'):
    """(rc, {family, P, gy, gz}) of a weight-gradient call in a GEMM mode."""
    key = ('w', mode) + tuple(call.values())
    if key in _plans:
        return _plans[key]
    from realvsr_amd import _lib
    L = _lib.lib()
    c = call
    row = (ctypes.c_int * 4)(-7, -7, -7, -7)
    L.rvsr_set_gemm_mode_thread(GEMM[mode])
    try:
        rc = L.rvsr_conv2d_backward_weight_plan(_ptr(1, c['x_off']), c['C1'], _ptr(2, c['x2_off'], c['C2']), c['C2'], c['H'], c['W'],
                                                _ptr(3, c['g_off']), _ptr(4, c['gact_off'], c['gact']), 0.1, c['g_mode'], c['Gh'], c['Gw'],
                                                _ptr(5), c['Co'], c['B'], c['k'], c['stride'], c['Ho'], c['Wo'], row)
    finally:
        L.rvsr_set_gemm_mode_thread(-1)
    out = (rc, dict(zip(('family', 'P', 'gy', 'gz'), row)))
    _plans[key] = out
    return out


def mask_taken(call, mode):
    """Whether the plan grants the mask epilogue (act 3) to this data-gradient call; functional falls back to a separate pass where not."""
    return fwd_plan(call, mode)[0] == 0


# ---- the nodes of functional.py
def out_size(H, W, k, stride):
    pad = k // 2
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def calls_of(case, offsets=(0, 0, 0, 0), mode='bf16x3', x_premask=None, grad_premasked=False):
    """The (name, call) pairs conv2d() issues, forward and backward, for a block case (C1, C2, Co, k, stride, act, residual,
    pixel_shuffle, B, H, W).  offsets: float offsets of x1, x2, the output gradient and the residual from a 16-byte boundary (everything
    the node allocates itself is aligned).  x_premask: this conv is the consumer of a premask pair (the activation name of its producer);
    grad_premasked: it is the producer.  `mode` decides only whether the consumer's mask epilogue is taken."""
    C1, C2, Co, k, stride, act, use_res, ps, B, H, W = case
    ox1, ox2, og, ores = offsets
    Ho, Wo = out_size(H, W, k, stride)
    # conv2d() adds a residual outside the node when there is an activation (act' is recovered from the saved output)
    fused_res = use_res and act == 'none'
    has_act = act != 'none' and not grad_premasked      # the saved output feeds act' into both gradient kernels
    calls = [('forward', fwd_call(C1, Co, H, W, Ho, Wo, B, k=k, stride=stride, C2=C2, res=fused_res, act=ACT[act], ps=ps, x_off=ox1,
                                  x2_off=ox2, res_off=ores))]
    in_mode = 2 if ps else (1 if stride == 2 else 0)
    Gh, Gw = (2 * Ho, 2 * Wo) if ps else (Ho, Wo)
    dgrad = dict(k=k, xact=has_act, in_mode=in_mode, w_mode=1, x_off=og)
    masked = False
    if x_premask is not None and k == 3:
        m = fwd_call(Co, C1, Gh, Gw, H, W, B, act=ACT_MASK, res=True, res_off=ox1, **dgrad)
        masked = mask_taken(m, mode)
        if masked:
            calls.append(('dgrad', m))
    if not masked:
        calls.append(('dgrad', fwd_call(Co, C1, Gh, Gw, H, W, B, Co2=C2, **dgrad)))
    calls.append(('wgrad', wgrad_call(C1, Co, H, W, Ho, Wo, B, k=k, stride=stride, C2=C2, gact=has_act, g_mode=2 if ps else 0, x_off=ox1,
                                      x2_off=ox2, g_off=og)))
    return calls


def res_block_calls(C, B, H, W, mode='bf16x3'):
    """The calls of functional.res_block, forward and backward (every tensor aligned)."""
    f = dict(B=B)
    calls = [('conv1', fwd_call(C, C, H, W, H, W, act=ACT['relu'], **f)), ('conv2', fwd_call(C, C, H, W, H, W, res=True, **f)),
             ('wgrad2', wgrad_call(C, C, H, W, H, W, B))]
    m = fwd_call(C, C, H, W, H, W, w_mode=1, act=ACT_MASK, res=True, **f)
    masked = mask_taken(m, mode)
    calls.append(('dgrad2', m if masked else fwd_call(C, C, H, W, H, W, w_mode=1, **f)))
    calls.append(('wgrad1', wgrad_call(C, C, H, W, H, W, B, gact=not masked)))
    calls.append(('dgrad1', fwd_call(C, C, H, W, H, W, w_mode=1, xact=not masked, res=True, **f)))
    return calls


def premask_pair_calls(pair, mode='bf16x3'):
    """The calls of a producer called with grad_premasked=True and its consumer called with x_premask.  pair = (producer, consumer):
    the producer is a block case or a ('bcast', ...) case of cat_bcast_calls, the consumer a block case on the producer's output."""
    prod, cons = pair
    if prod[0] == 'bcast':
        calls = cat_bcast_calls(prod[1:], grad_premasked=True)
        pact = prod[4]
    else:
        calls = calls_of(prod, mode=mode, grad_premasked=True)
        pact = prod[5]
    return [('producer ' + n, c) for n, c in calls] + [('consumer ' + n, c) for n, c in calls_of(cons, mode=mode, x_premask=pact)]


def cat_bcast_calls(case, grad_premasked=False):
    """The calls of functional.conv_cat_bcast for (C1, C2, Co, act, N, B, H, W, x_sink, ref_sink): x_sink None / 'dep' / 'own' (an owner
    that finds a deposit), ref_sink None or the block index of ref inside the sink's tensor."""
    C1, C2, Co, act, N, B, H, W, x_sink, ref_sink = case
    has_act = act != 'none' and not grad_premasked
    blk_off = 0 if ref_sink is None else (ref_sink * B * C2 * H * W) % 4
    return [('conv_a', fwd_call(C1, Co, H, W, H, W, N * B)), ('conv_b', fwd_call(C2, Co, H, W, H, W, B)),
            ('dgrad_b', fwd_call(Co, C2, H, W, H, W, B, w_mode=1, res=ref_sink is not None, res_off=blk_off, out_off=blk_off)),
            ('dgrad_a', fwd_call(Co, C1, H, W, H, W, N * B, w_mode=1, xact=has_act, res=x_sink is not None)),
            ('wgrad_a', wgrad_call(C1, Co, H, W, H, W, N * B, gact=has_act)), ('wgrad_b', wgrad_call(C2, Co, H, W, H, W, B))]


def conv5_calls(case):
    """The calls of a 5x5 block of tests/test_gpu_gan_ops.py: (C, Co, stride, bias, act, B, H, W)."""
    C, Co, stride, _, act, B, H, W = case
    return calls_of((C, 0, Co, 5, stride, act, False, False, B, H, W))


def conv3d_frames_calls(case, need_x=True, need_w=True):
    """The calls of functional.conv3d_frames for (T, f0, f1, B, Ci, Co, H, W, k, bias, residual), forward and backward: one 2-D conv per
    temporal tap over the frame range it meets (functional._c3_taps: the centre tap first, the outer taps accumulate in place), the same
    for the data gradient, one weight gradient per tap.  x, the residual and the output gradient are aligned tensors; a frame range
    starts a whole number of frames in.  need_w: the weight or the bias wants a gradient."""
    from realvsr_amd.functional import _c3_taps
    T, f0, f1, B, Ci, Co, H, W, k, _, use_res = case
    taps = _c3_taps(T, f0, f1)
    xo = lambda a: (a * B * Ci * H * W) % 4    # noqa: E731  (float offset of input frame a)
    yo = lambda o: (o * B * Co * H * W) % 4    # noqa: E731  (of output frame o)
    calls = []
    for i, (dt, a, n, o) in enumerate(taps):
        calls.append(('tap %d' % dt, fwd_call(Ci, Co, H, W, H, W, n * B, k=k, res=use_res if i == 0 else True, x_off=xo(a), out_off=yo(o),
                                              res_off=0 if i == 0 else yo(o))))
    if need_x:
        for i, (dt, a, n, o) in enumerate(taps):
            calls.append(('dgrad tap %d' % dt, fwd_call(Co, Ci, H, W, H, W, n * B, k=k, w_mode=1, res=i > 0, x_off=yo(o), out_off=xo(a),
                                                        res_off=xo(a))))
    if need_w:
        for dt, a, n, o in taps:
            calls.append(('wgrad tap %d' % dt, wgrad_call(Ci, Co, H, W, H, W, n * B, k=k, x_off=xo(a), g_off=yo(o))))
    return calls


def tsa_block_calls(case, need_aligned=True, need_1=True, need_2=True):
    """The calls of functional.tsa_temporal_block for (N, center, B, C, H, W): tAtt_1 on all N * B frames, tAtt_2 on the centre block,
    their weight gradients, and the two data gradients that accumulate in place into the gradient of `aligned` and its centre block."""
    N, center, B, C, H, W = case
    coff = (center * B * C * H * W) % 4
    calls = [('tAtt_1', fwd_call(C, C, H, W, H, W, N * B)), ('tAtt_2', fwd_call(C, C, H, W, H, W, B, x_off=coff))]
    if need_1:
        calls.append(('wgrad tAtt_1', wgrad_call(C, C, H, W, H, W, N * B)))
    if need_2:
        calls.append(('wgrad tAtt_2', wgrad_call(C, C, H, W, H, W, B, x_off=coff)))
    if need_aligned:
        calls.append(('dgrad tAtt_1', fwd_call(C, C, H, W, H, W, N * B, w_mode=1, res=True)))
        calls.append(('dgrad tAtt_2', fwd_call(C, C, H, W, H, W, B, w_mode=1, res=True, res_off=coff, out_off=coff)))
    return calls


def conv_transpose1x1_calls(case):
    """The calls of functional.conv_transpose1x1 for (batch, Ci, Co, H, W): the forward is a transposed-weight 1x1 conv, its data
    gradient a plain one, the weight gradient that of a Ci -> Co conv (copied back through a transpose)."""
    Bn, Ci, Co, H, W = case
    return [('forward', fwd_call(Ci, Co, H, W, H, W, Bn, k=1, w_mode=1)), ('dgrad', fwd_call(Co, Ci, H, W, H, W, Bn, k=1)),
            ('wgrad', wgrad_call(Ci, Co, H, W, H, W, Bn, k=1))]


def inplace_call(case):
    """The functional._conv call of an in-place case of tests/test_gpu_conv_inplace.py: (C1, C2, Co, k, stride, transposed, xact, B, H,
    W, x_off, out_off); the residual IS the output buffer, so it shares the output's offset."""
    C1, C2, Co, k, stride, transposed, xact, B, H, W, x_off, out_off = case
    Ho, Wo = out_size(H, W, k, stride)
    return fwd_call(C1, Co, H, W, Ho, Wo, B, k=k, stride=stride, C2=C2, xact=xact, res=True, w_mode=1 if transposed else 0, x_off=x_off,
                    x2_off=x_off, xact_off=x_off, res_off=out_off, out_off=out_off)


def residual_epilogue_key(call, row):
    """A kernel variant that can carry a residual: the forward kernel, whether it stores 16 bytes at a time, and whether the output or
    the residual is off a 16-byte boundary.  None for a call without a residual or with the mask epilogue (which reads `residual` as a
    mask and never aliases)."""
    if not call['res'] or call['act'] == ACT_MASK:
        return None
    return (fwd_kernel_key(call, row), row['vec4'], bool(call['out_off'] or call['res_off']))


# ---- ledger keys
def fwd_kernel_key(call, row):
    return (FWD_FAMILY[row['family']], call['k'], call['stride'], row['MT'], row['vec'], row['wide'], row['NT'], row['act_in'])


def epilogue_of(call):
    return 'mask' if call['act'] == ACT_MASK else 'pixel-shuffle' if call['ps'] else 'split' if call['Co2'] else 'residual' if call['res'] else 'plain'


def fwd_epilogue_key(call, row):
    return (FWD_FAMILY[row['family']], call['k'], call['stride'], row['wide'], epilogue_of(call), row['vec4'])


def fwd5_staging_key(call, row):
    return None if FWD_FAMILY[row['family']] != 'fwd5' else (row['vec'], call['C2'] > 0, row['act_in'])


def wgrad_keys(call, row):
    fam = WGRAD_FAMILY[row['family']]
    return [(fam, 'act', call['gact']), (fam, 'x2', call['C2'] > 0), (fam, 'g_mode', call['g_mode']), (fam, 'gy>1', row['gy'] > 1),
            (fam, 'gz>1', row['gz'] > 1), (fam, 'P>1', row['P'] > 1)]


def misaligned_keys(call, row):
    """The plan's fallbacks for a pointer off a 16-byte boundary: one key per side of the call that is off, with the kernel it then runs."""
    if 'Gh' in call:
        fam = WGRAD_FAMILY[row['family']]
        return [(fam, side) for side, off in (('x', call['x_off'] or call['x2_off']), ('g', call['g_off'] or call['gact_off'])) if off]
    kernel = (FWD_FAMILY[row['family']], call['k'], call['stride'], row['vec'], row['vec4'])
    return [kernel + (side,) for side, off in (('in', call['x_off'] or call['x2_off'] or call['xact_off']),
                                               ('out', call['out_off'] or call['out2_off'] or call['res_off'])) if off]


LEDGERS = ('forward kernel', 'forward epilogue', 'conv_fwd5 staging', 'weight gradient', 'misaligned pointer')


def keys_of(call, mode):
    """[(ledger name, key)] of one call; a refused forward call (the mask epilogue where the plan has none) has no key."""
    if 'Gh' in call:
        rc, row = wgrad_plan(call, mode)
        assert rc == 0, (call, rc)
        return [('weight gradient', key) for key in wgrad_keys(call, row)] + [('misaligned pointer', key) for key in misaligned_keys(call, row)]
    rc, row = fwd_plan(call, mode)
    if rc != 0:
        assert rc == 1 and call['act'] == ACT_MASK, (call, rc)
        return []
    out = [('forward kernel', fwd_kernel_key(call, row)), ('forward epilogue', fwd_epilogue_key(call, row))]
    out += [('misaligned pointer', key) for key in misaligned_keys(call, row)]
    s = fwd5_staging_key(call, row)
    if s is not None:
        out.append(('conv_fwd5 staging', s))
    return out


def collect(named_calls, mode, into=None):
    """{ledger: {key: name of the first case that reaches it}} over (name, call) pairs."""
    into = {name: {} for name in LEDGERS} if into is None else into
    for name, call in named_calls:
        for ledger, key in keys_of(call, mode):
            into[ledger].setdefault(key, name)
    return into
