"""FSTRN without a GPU: the module tree against the reference's (fixture fstrn.npz), define_G's branch and its refusals, the exported
symbols of the temporal convolution and the PReLU, their plans on host addresses, and the refusal of CPU tensors."""
import ctypes

import pytest
import torch

from conftest import load_golden

CASES = {'t3': dict(k=3, nf=64, scale=1, nframes=3), 't5': dict(k=3, nf=32, scale=1, nframes=5)}
# network_G of train_FSTRN_RealVSR_YCbCr_Split.yml / ..._Combine.yml
OPTION_FILE_G = dict(which_model_G='FSTRN', k=3, nf=64, nframes=3)
SYMBOLS = ('rvsr_tconv3_plan', 'rvsr_tconv3_forward', 'rvsr_prelu_workspace_bytes', 'rvsr_prelu_plan', 'rvsr_prelu_forward',
           'rvsr_prelu_backward')


@pytest.mark.parametrize('tag', ['t3', 't5'])
def test_state_dict_matches_reference(tag):
    from realvsr_amd.archs.FSTRN_arch import FSTRN
    g = load_golden('fstrn')
    sd = FSTRN(**CASES[tag]).state_dict()
    assert len(sd) == 34
    assert list(sd.keys()) == [str(k) for k in g[tag + '.keys']]
    for (k, v), shape in zip(sd.items(), g[tag + '.shapes']):
        assert list(v.shape) == [int(n) for n in shape[:v.dim()]] and all(int(n) == 0 for n in shape[v.dim():]), k
    assert tuple(sd['prelu.weight'].shape) == (1,) and tuple(sd['frb_3.prelu.weight'].shape) == (1,)


def test_define_g_builds_fstrn_from_the_option_file_block():
    from realvsr_amd.VideoSR_archs import define_G
    from realvsr_amd.archs.FSTRN_arch import FSTRN, FRB
    net = define_G({'scale': 1, 'network_G': dict(OPTION_FILE_G)})
    assert isinstance(net, FSTRN) and net.center == 1 and net.nf == 64 and net.scale == 1
    frbs = [m for m in net.children() if isinstance(m, FRB)]
    assert len(frbs) == 5 and [n for n, _ in net.named_children()][1:6] == ['frb_%d' % i for i in range(1, 6)]
    assert isinstance(net.dropout, torch.nn.Dropout) and net.dropout.p == 0.3
    assert define_G({'scale': 1, 'network_G': dict(OPTION_FILE_G, nframes=5)}).center == 2


def test_refusals():
    from realvsr_amd.VideoSR_archs import define_G
    from realvsr_amd.archs.FSTRN_arch import FSTRN, FRB
    for drop in ('k', 'nf', 'nframes'):
        block = {k: v for k, v in OPTION_FILE_G.items() if k != drop}
        with pytest.raises(NotImplementedError, match=drop):
            define_G({'scale': 1, 'network_G': block})
    with pytest.raises(NotImplementedError, match='scale'):
        define_G({'network_G': dict(OPTION_FILE_G)})
    with pytest.raises(NotImplementedError, match='k = 5'):
        define_G({'scale': 1, 'network_G': dict(OPTION_FILE_G, k=5)})
    with pytest.raises(NotImplementedError, match='scale 4'):
        define_G({'scale': 4, 'network_G': dict(OPTION_FILE_G)})
    with pytest.raises(NotImplementedError):
        FSTRN()          # the reference's default is scale 4
    with pytest.raises(NotImplementedError):
        FRB(k=5)


def test_library_exports_the_fstrn_symbols():
    from realvsr_amd import _lib
    L = _lib.lib()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    with open(_lib.SO_PATH.replace('realvsr_amd/csrc/librealvsr_hip.so', 'include/realvsr_hip.h')) as f:
        header = f.read()
    assert all(name + '(' in header for name in SYMBOLS)
    assert 'FSTRN_arch.py' in header


def _tplan(L, T, B, Ci, Co, H, W, s, res, out, pout):
    vec, grid = ctypes.c_int(-1), ctypes.c_int(-1)
    p = [None if a is None else ctypes.c_void_p(a) for a in (s, res, out, pout)]
    rc = L.rvsr_tconv3_plan(T, B, Ci, Co, H, W, *p, ctypes.byref(vec), ctypes.byref(grid))
    return rc, vec.value, grid.value


def test_tconv3_plan_on_host_addresses():
    from realvsr_amd import _lib
    L = _lib.lib()
    a, b, c, d = 1 << 20, 2 << 20, 3 << 20, 4 << 20   # 16-byte-aligned addresses: the plan reads none
    # load width: 16-byte accesses need H * W % 4 == 0 and every streamed tensor 16-byte aligned (absent ones do not count)
    assert _tplan(L, 3, 2, 64, 64, 8, 16, a, b, c, d)[:2] == (0, 1)
    assert _tplan(L, 3, 2, 64, 64, 8, 16, a, None, c, None)[:2] == (0, 1)
    assert _tplan(L, 5, 1, 32, 32, 13, 22, a, b, c, d)[:2] == (0, 0)       # 286 % 4 == 2
    assert _tplan(L, 3, 1, 64, 64, 9, 70, a, b, c, d)[:2] == (0, 0)        # 630 % 4 == 2
    for off in ((4, 0, 0, 0), (0, 4, 0, 0), (0, 0, 4, 0), (0, 0, 0, 4), (8, 0, 0, 0)):
        assert _tplan(L, 3, 2, 64, 64, 8, 16, a + off[0], b + off[1], c + off[2], d + off[3])[:2] == (0, 0)
    # work: one item per 128 pixels of a batch element, at most 1024 workgroups (a workgroup then walks several items)
    assert _tplan(L, 3, 2, 64, 64, 8, 16, a, b, c, d)[2] == 2
    assert _tplan(L, 3, 2, 64, 64, 9, 70, a, b, c, d)[2] == 2 * 5
    assert _tplan(L, 3, 32, 64, 64, 192, 192, a, b, c, d) == (0, 1, 1024)
    # channel counts: anything up to 64 x 64 (partial k-steps and m-tiles are masked), nothing beyond
    for Ci, Co in ((64, 64), (32, 32), (16, 48), (48, 16), (20, 12), (1, 1)):
        assert _tplan(L, 3, 1, Ci, Co, 8, 16, a, b, c, d)[0] == 0
    for Ci, Co in ((128, 64), (64, 65), (65, 3)):
        assert _tplan(L, 3, 1, Ci, Co, 8, 16, a, b, c, d)[0] == 1 and b'64 channels' in L.rvsr_last_error()
    assert _tplan(L, 1, 1, 64, 64, 4096, 4096, a, b, c, d)[0] == 1         # a plane beyond the 32-bit byte offsets of a frame
    # empty shapes are an error, not a refusal
    for shape in ((0, 1, 64, 64, 8, 16), (3, 0, 64, 64, 8, 16), (3, 1, 0, 64, 8, 16), (3, 1, 64, 0, 8, 16), (3, 1, 64, 64, 0, 16),
                  (3, 1, 64, 64, 8, 0)):
        assert _tplan(L, *shape, a, b, c, d)[0] == 2


def _pplan(L, n, f, keep):
    vec, blocks = ctypes.c_int(-1), ctypes.c_int(-1)
    p = [None if a is None else ctypes.c_void_p(a) for a in (*f, keep)]
    rc = L.rvsr_prelu_plan(n, *p, ctypes.byref(vec), ctypes.byref(blocks))
    return rc, vec.value, blocks.value


def test_prelu_plan_on_host_addresses():
    from realvsr_amd import _lib
    L = _lib.lib()
    a, b, c, k = 1 << 20, 2 << 20, 3 << 20, 5 << 20
    assert _pplan(L, 12288, (a, b, c, None, None), k) == (0, 1, 3)
    assert _pplan(L, 12288, (a, None, c, None, None), None) == (0, 1, 3)
    assert _pplan(L, 4290, (a, b, c, None, None), k)[:2] == (0, 0)               # n % 4 == 2
    assert _pplan(L, 12288, (a + 4, b, c, None, None), k)[:2] == (0, 0)
    assert _pplan(L, 12288, (a, b, c + 8, None, None), k)[:2] == (0, 0)
    assert _pplan(L, 12288, (a, b, c, None, None), k + 1)[:2] == (0, 0)          # the mask is read four bytes at a time
    assert _pplan(L, 12288, (a, b, c, None, None), k + 4)[:2] == (0, 1)
    assert _pplan(L, 1, (a, None, c, None, None), None) == (0, 0, 1)
    # the backward streams five: g, a, b, gres, gx
    e, f = 6 << 20, 7 << 20
    assert _pplan(L, 12288, (a, b, c, e, f), k)[:2] == (0, 1)
    assert _pplan(L, 12288, (a, b, c, e + 4, f), k)[:2] == (0, 0)
    assert _pplan(L, 12288, (a, b, c, e, f + 8), k)[:2] == (0, 0)
    assert _pplan(L, 12288, (a, b, None, None, f), None)[:2] == (0, 1)
    assert _pplan(L, 3 * 32 * 64 * 192 * 192, (a, b, c, None, None), k) == (0, 1, 2048)   # never more partial sums than the workspace holds
    assert L.rvsr_prelu_workspace_bytes() >= 4 * 2048
    assert _pplan(L, 0, (a, b, c, None, None), k)[0] == 2


def test_cpu_tensors_are_refused():
    from realvsr_amd import functional as RF
    from realvsr_amd.archs.FSTRN_arch import FSTRN, FRB
    x = torch.randn(3, 1, 16, 4, 8)
    frb = FRB(3, 16)
    with pytest.raises(NotImplementedError):
        RF.tconv3(x, frb.conv3d_2)
    with pytest.raises(NotImplementedError):
        RF.prelu(x, frb.prelu)
    with pytest.raises(NotImplementedError):
        RF.frb(x, frb.prelu, frb.conv3d_1, frb.conv3d_2)
    with pytest.raises(NotImplementedError):
        RF.conv3d_frames(x, torch.nn.Conv3d(16, 16, 3, padding=1))
    with pytest.raises(NotImplementedError):
        RF.conv_transpose1x1(x, torch.nn.ConvTranspose3d(16, 16, 1))
    with pytest.raises(NotImplementedError):
        FSTRN(nf=16, scale=1, nframes=3)(torch.randn(1, 3, 3, 8, 8))


def test_a_slope_per_channel_is_refused():
    from realvsr_amd import functional as RF
    with pytest.raises(NotImplementedError, match='one slope'):
        RF._slope(torch.nn.PReLU(16).weight)
    w = torch.nn.PReLU().weight
    assert RF._slope(w) is w and RF._slope(None) is None
