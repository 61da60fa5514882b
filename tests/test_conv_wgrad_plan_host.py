"""The weight-gradient plan (csrc/conv_plan.h: conv_wgrad_plan) through its exported query: no GPU, made-up addresses.

Which family a rvsr_conv2d_backward_weight call runs, with how many partial sums and on what grid -- the rows of the config-2 training
step that the LDS-staged 1x1 kernel (conv_wgrad1x1s) takes, every rule that sends a call back to the kernels it does not replace, and
the workspace query against what the chosen family writes."""
import ctypes

_A = 0x10000000   # 16-byte aligned; the plan dereferences nothing
THIN, WGRAD2, WGRAD5, F32_5, W1X1S, W1X1, F32_3S1, WS2, F32_3S2, F32_1 = range(10)


def _plan(C1=64, Co=64, H=180, W=320, *, B=8, C2=0, k=1, stride=1, gact=True, g_mode=0, x_off=0, g_off=0, gemm=None):
    """(rc, {family, P, gy, gz}, workspace bytes of the geometry) for the weight gradient of a conv of (B, C1 [+ C2], H, W)."""
    from realvsr_amd import _lib
    L = _lib.lib()
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    Gh, Gw = (2 * Ho, 2 * Wo) if g_mode == 2 else (Ho, Wo)
    p = lambda off, on=True: ctypes.c_void_p(_A + off) if on else None   # noqa: E731
    row = (ctypes.c_int * 4)(-7, -7, -7, -7)
    L.rvsr_set_gemm_mode_thread(-1 if gemm is None else gemm)
    try:
        rc = L.rvsr_conv2d_backward_weight_plan(p(0x100000 + x_off), C1, p(0x200000, C2), C2, H, W, p(0x300000 + g_off), p(0x400000, gact), 0.1,
                                                g_mode, Gh, Gw, p(0x500000), Co, B, k, stride, Ho, Wo, row)
    finally:
        L.rvsr_set_gemm_mode_thread(-1)
    ws = L.rvsr_conv2d_wgrad_workspace_bytes(C1, C2, Co, B, k, stride, Ho, Wo)
    return rc, dict(zip(('family', 'P', 'gy', 'gz'), row)), ws


# (call, expected row)
_ROWS = [
    # the 1x1 layers of the config-2 step (8 x 180 x 320): the LDS-staged kernel, one workgroup per 64 x 320 block of gW
    (dict(C1=320), dict(family=W1X1S, P=204, gy=1, gz=1)),              # fea_fusion / sAtt_1: as many partials as the 64 x 64-block kernel
    (dict(C1=320, gact=False), dict(family=W1X1S, P=204, gy=1, gz=1)),
    (dict(), dict(family=W1X1S, P=256, gy=1, gz=1)),                    # 64 -> 64
    (dict(C2=64), dict(family=W1X1S, P=256, gy=1, gz=1)),               # cat(max, avg) -> 64: the second input on a block boundary
    (dict(B=8, H=90, W=160), dict(family=W1X1S, P=256, gy=1, gz=1)),
    (dict(C1=384, Co=80), dict(family=W1X1S, P=64, gy=2, gz=2)),        # more than one block each way
    (dict(B=1, H=8, W=8), dict(family=W1X1S, P=1, gy=1, gz=1)),         # fewer 64-pixel tiles than slots
    (dict(B=3, H=13, W=24, C1=320), dict(family=W1X1S, P=12, gy=1, gz=1)),
    (dict(B=1, H=9, W=12), dict(family=W1X1S, P=2)),                    # 108 pixels: whole float4s, not whole octets
    # ... and what it does not take: the kernels that were there before
    (dict(C1=320, x_off=4), dict(family=F32_1, P=204, gy=1, gz=5)),     # a misaligned pointer
    (dict(C1=320, g_off=8), dict(family=F32_1, P=204, gy=1, gz=5)),
    (dict(B=1, H=9, W=33), dict(family=F32_1)),                         # H * W % 4 != 0
    (dict(B=1, H=9, W=30), dict(family=F32_1)),
    (dict(C1=320, B=1, H=1500, W=1200), dict(family=W1X1, gy=1, gz=5)),   # a batch element of 2 GB or more
    (dict(C1=32, C2=32), dict(family=W1X1, P=1024, gy=1, gz=1)),        # a second input off the 64-channel boundary
    (dict(C1=320, gemm=1), dict(family=F32_1, P=204, gy=1, gz=5)),      # GEMM mode f32
    (dict(gemm=1), dict(family=F32_1, P=1024)),
    (dict(C1=320, gemm=2), dict(family=W1X1S, P=204)),                  # three terms in every split mode
    (dict(C1=320, gemm=3), dict(family=W1X1S, P=204)),
    # the other geometries are where they were
    (dict(k=3, B=40), dict(family=WGRAD2, P=256, gy=1, gz=1)),
    (dict(k=3, B=40, gemm=1), dict(family=F32_3S1)),
    (dict(k=3, Co=3), dict(family=THIN, gy=1, gz=1)),
    (dict(k=3, stride=2, B=40), dict(family=WS2, P=512, gy=1, gz=1)),
    (dict(k=3, stride=2, B=40, gemm=1), dict(family=F32_3S2)),
    (dict(k=3, stride=2, H=45, W=78), dict(family=F32_3S2)),            # Wout % 8 != 0
    (dict(k=5, C1=3), dict(family=WGRAD5)),
    (dict(k=5, C1=3, gemm=1), dict(family=F32_5)),
]


def test_conv_wgrad_plan_rows():
    for call, want in _ROWS:
        rc, row, _ = _plan(**call)
        assert rc == 0, call
        got = {key: row[key] for key in want}
        assert got == want, (call, row)
    assert _plan(C1=320)[1]['family'] == W1X1S      # after a per-thread mode the thread is back on the process-wide one


def test_conv_wgrad_workspace_covers_the_plan():
    """What the chosen family writes -- P x (Co x Ctot x taps + Co) floats -- fits the workspace the query asks for, whichever family the
    pointers and the GEMM mode select."""
    for call, _ in _ROWS:
        rc, row, ws = _plan(**call)
        C, Co, k = call.get('C1', 64) + call.get('C2', 0), call.get('Co', 64), call.get('k', 1)
        assert rc == 0 and row['P'] >= 1
        assert ws >= 4 * row['P'] * (Co * C * k * k + Co), (call, row, ws)


def test_conv_wgrad_plan_validates_like_the_call():
    from realvsr_amd import _lib
    L = _lib.lib()
    p = lambda off: ctypes.c_void_p(_A + off)   # noqa: E731
    row = (ctypes.c_int * 4)(-7, -7, -7, -7)
    rc = L.rvsr_conv2d_backward_weight_plan(p(0), 64, None, 0, 45, 80, p(0x100000), None, 0.0, 0, 44, 80, p(0x200000), 64, 1, 1, 1, 44, 80, row)
    assert rc == 2 and 'does not give output' in L.rvsr_last_error().decode() and list(row) == [-7] * 4
    rc = L.rvsr_conv2d_backward_weight_plan(p(0), 64, None, 0, 45, 80, p(0x100000), None, 0.0, 0, 23, 40, p(0x200000), 64, 1, 1, 2, 23, 40, row)
    assert rc == 1 and 'stride' in L.rvsr_last_error().decode()
