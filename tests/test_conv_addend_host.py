"""rvsr_conv2d_forward_addend_plan, no GPU: which calls get the periodic-addend epilogue (out = act(conv + bias + addend[b % period]),
the 8 x 64-tile conv_fwd5 kernel only), which are refused with RVSR_ERR_UNSUPPORTED and an empty message so that conv_cat_bcast runs
its three calls instead, and that period 0 is rvsr_conv2d_forward_plan argument for argument."""
import ctypes

import pytest

import conv_ledger as CL
from test_host_logic import _A, _conv_plan, FWD5

KEYS = ('family', 'MT', 'vec', 'wide', 'NT', 'act_in', 'CC', 'vec4', 'th', 'tw', 'gx', 'gy', 'gz', 'lds')


def _addend_plan(C1=64, Co=64, H=180, W=320, *, B=40, period=8, C2=0, xact=False, in_mode=0, k=3, stride=1, w_mode=0, act=2, addend=True,
                 Co2=0, ps=0, x_off=0, out_off=0, add_off=0, Hout=None, Wout=None, gemm=None):
    """(rc, message, plan row) of rvsr_conv2d_forward_addend_plan; the arguments are test_host_logic._conv_plan's plus the period."""
    from realvsr_amd import _lib
    L = _lib.lib()
    pad = k // 2
    if Hout is None:
        Hout, Wout = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    p = lambda off, on=True: ctypes.c_void_p(_A + off) if on else None   # noqa: E731
    row = (ctypes.c_int * 14)(*([-7] * 14))
    L.rvsr_set_gemm_mode_thread(-1 if gemm is None else gemm)
    try:
        rc = L.rvsr_conv2d_forward_addend_plan(p(0x100000 + x_off), C1, p(0x200000, C2), C2, p(0x300000, xact), 0.1, in_mode, H, W, p(0x400000),
                                               p(0x500000), p(0x600000 + add_off, addend), p(0x700000 + out_off), Co, p(0x800000, Co2), Co2,
                                               B, k, stride, w_mode, act, 0.1, ps, Hout, Wout, period, row)
    finally:
        L.rvsr_set_gemm_mode_thread(-1)
    return rc, L.rvsr_last_error().decode(), dict(zip(KEYS, row))


def test_the_training_sites_are_granted():
    """The L1 and cascade offset convs of the PCD stage, 40 x 64 x 180 x 320 with 8 partials: the row of the plain conv (test_host_logic's
    first row at B = 40), in every split GEMM mode with that mode's term count; Co = 216 (a cut fourth m-block) as well."""
    rc, _, row = _addend_plan()      # (a granted call leaves rvsr_last_error alone: the message is read on refusals only)
    assert rc == 0
    assert row == dict(family=FWD5, MT=2, vec=1, wide=1, NT=3, act_in=0, CC=1, vec4=1, th=8, tw=64, gx=256, gy=1, gz=1, lds=159248)
    assert row == _conv_plan(H=180, W=320, B=40)[2]
    for gemm, nt in ((0, 3), (2, 2), (3, 1)):
        rc, _, row = _addend_plan(gemm=gemm)
        assert rc == 0 and (row['family'], row['wide'], row['NT']) == (FWD5, 1, nt)
    for act in (0, 1, 2):
        assert _addend_plan(act=act)[0] == 0
    rc, _, row = _addend_plan(Co=216, B=2, period=1)
    assert rc == 0 and (row['family'], row['MT'], row['wide']) == (FWD5, 2, 1)
    assert _addend_plan(H=8, W=64, B=6, period=2)[0] == 0 and _addend_plan(H=9, W=64, B=6, period=2)[0] == 0


REFUSED = [
    dict(W=62),                       # W % 4 != 0: element stores
    dict(out_off=4), dict(add_off=4),  # output / addend off the 16-byte boundary: element stores
    dict(x_off=4),                    # scalar staging: no 8 x 64 tile
    dict(Co=32), dict(Co=16),         # MT = 1
    dict(gemm=1),                     # exact f32
    dict(Co=256, ps=1),               # pixel shuffle
    dict(Co=32, Co2=32),              # split output
    dict(act=3),                      # the mask epilogue reads the same operand
    dict(k=1), dict(k=5), dict(stride=2), dict(H=90, W=160, in_mode=1, Hout=180, Wout=320, w_mode=1),
    dict(H=45, W=80),                 # the 16 x 32 tile wastes fewer pixels here (L3): no epilogue there
]


@pytest.mark.parametrize('kw', REFUSED, ids=lambda kw: ','.join('%s=%s' % i for i in kw.items()))
def test_everything_else_is_refused_silently(kw):
    from realvsr_amd import _lib
    rc, msg, row = _addend_plan(**kw)
    assert (rc, msg, row['family']) == (_lib.RVSR_ERR_UNSUPPORTED, '', -1)


def test_bad_periods():
    from realvsr_amd import _lib
    assert _addend_plan(period=-1)[0] == _lib.RVSR_ERR_BAD_ARG
    assert _addend_plan(period=8, addend=False)[0] == _lib.RVSR_ERR_BAD_ARG


@pytest.mark.parametrize('kw', [dict(), dict(H=45, W=80), dict(Co=32), dict(Co=3), dict(stride=2), dict(k=1, C1=32, C2=32), dict(k=5),
                                dict(act=3, addend=True), dict(act=3, addend=True, H=45, W=80), dict(addend=True, act=0)],
                         ids=lambda kw: ','.join('%s=%s' % i for i in kw.items()) or 'default')
def test_period_zero_is_the_plain_entry(kw):
    """One body behind both entries: with period 0 the answer, the message and the row are rvsr_conv2d_forward_plan's."""
    kw = dict(dict(B=2, act=0, addend=False), **kw)
    a = _addend_plan(period=0, **kw)
    kw['residual'] = kw.pop('addend')
    b = _conv_plan(**dict(dict(H=180, W=320), **kw))
    assert (a[0], a[2]) == (b[0], b[2]) and (a[0] == 0 or a[1] == b[1])


def test_the_ledger_cases_of_conv_cat_bcast_fall_back():
    """tests/test_gpu_conv_ledger.py runs conv_cat_bcast with Co = 16 and expects conv_ledger.cat_bcast_calls: conv_a as a plain call.
    The fused attempt for exactly those conv_a calls must be refused, at any alignment of the tensors."""
    from realvsr_amd import _lib
    for case in ((16, 16, 16, 'lrelu', 3, 2, 8, 12, None, None), (16, 16, 16, 'none', 3, 1, 9, 10, 'own', 1)):
        C1, C2, Co, act, N, B, H, W = case[:8]
        plain = [c for _, c in CL.cat_bcast_calls(case) if c.get('w_mode') == 0 and c['B'] == N * B]
        assert len(plain) == 1 and plain[0]['act'] == 0 and not plain[0]['res']       # conv_a as the ledger has it
        for off in (0, 4):
            rc, msg, _ = _addend_plan(C1=C1, Co=Co, H=H, W=W, B=N * B, period=B, act=CL.ACT[act], x_off=off, out_off=off)
            assert (rc, msg) == (_lib.RVSR_ERR_UNSUPPORTED, '')
