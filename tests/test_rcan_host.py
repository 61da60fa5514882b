"""RCAN without a GPU: the module tree against the reference's (fixture rcan.npz), define_G's branch, the four exported symbols of the
channel-attention operator and its plan on host addresses."""
import ctypes

import pytest

from conftest import load_golden

CASES = {'s1': dict(num_feat=64, squeeze_factor=16, num_group=2, num_block=2, upscale=1, res_scale=1),
         's2': dict(num_feat=32, squeeze_factor=8, num_group=2, num_block=2, upscale=2, res_scale=0.5)}
# network_G of train_RCAN_RealVSR_YCbCr_Split.yml / ..._Combine.yml
OPTION_FILE_G = dict(which_model_G='RCAN', num_in_ch=3, num_out_ch=3, num_frames=3, num_feat=64, num_group=5, num_block=2,
                     squeeze_factor=16, res_scale=1)


@pytest.mark.parametrize('tag', ['s1', 's2'])
def test_state_dict_matches_reference(tag):
    from realvsr_amd.archs.RCAN_arch import RCAN
    g = load_golden('rcan')
    net = RCAN(num_in_ch=3, num_out_ch=3, num_frames=3, **CASES[tag])
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in g[tag + '.keys']]
    for v, shape in zip(sd.values(), g[tag + '.shapes']):
        assert list(v.shape) == [int(n) for n in shape[:v.dim()]] and all(int(n) == 0 for n in shape[v.dim():])


def test_define_g_builds_rcan_from_the_option_file_block():
    from realvsr_amd.VideoSR_archs import define_G
    from realvsr_amd.archs.RCAN_arch import RCAN, RCAB
    net = define_G({'scale': 1, 'network_G': dict(OPTION_FILE_G)})
    assert isinstance(net, RCAN)
    assert len(net.body) == 5 and len(net.body[0].residual_group) == 2 and isinstance(net.body[0].residual_group[0], RCAB)
    assert len(net.upsample) == 0 and net.conv_first.in_channels == 9
    assert net.body[0].residual_group[0].rcab[3].attention[1].out_channels == 4
    # a block that lacks one of the keys the reference reads is not a buildable request
    for drop in ('num_feat', 'res_scale'):
        block = {k: v for k, v in OPTION_FILE_G.items() if k != drop}
        with pytest.raises(NotImplementedError, match=drop):
            define_G({'scale': 1, 'network_G': block})
    with pytest.raises(NotImplementedError, match='scale'):
        define_G({'network_G': dict(OPTION_FILE_G)})


def test_scale_3_is_refused():
    from realvsr_amd.VideoSR_archs import define_G
    with pytest.raises(NotImplementedError):
        define_G({'scale': 3, 'network_G': dict(OPTION_FILE_G)})
    net = define_G({'scale': 4, 'network_G': dict(OPTION_FILE_G, num_group=1, num_block=1)})
    assert [type(m).__name__ for m in net.upsample] == ['Conv2d', 'PixelShuffle', 'Conv2d', 'PixelShuffle']


def test_library_exports_the_channel_attention_symbols():
    from realvsr_amd import _lib
    L = _lib.lib()
    for name in ('rvsr_channel_attention_workspace_bytes', 'rvsr_channel_attention_plan', 'rvsr_channel_attention_forward',
                 'rvsr_channel_attention_backward'):
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    with open(_lib.SO_PATH.replace('realvsr_amd/csrc/librealvsr_hip.so', 'include/realvsr_hip.h')) as f:
        header = f.read()
    assert all(name + '(' in header for name in _lib.SIGNATURES if name.startswith('rvsr_channel_attention'))


def _plan(L, B, C, H, W, u, x, out):
    slices, vec = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = L.rvsr_channel_attention_plan(B, C, H, W, ctypes.c_void_p(u), ctypes.c_void_p(x) if x else None, ctypes.c_void_p(out),
                                       ctypes.byref(slices), ctypes.byref(vec))
    return rc, slices.value, vec.value


def test_plan_on_host_addresses():
    from realvsr_amd import _lib
    L = _lib.lib()
    a, b, c = 1 << 20, 2 << 20, 3 << 20   # 16-byte-aligned addresses: the plan reads none
    # load width: 16-byte accesses need H * W % 4 == 0 and every streamed tensor 16-byte aligned
    assert _plan(L, 2, 64, 8, 16, a, b, c) == (0, 1, 1)
    assert _plan(L, 2, 64, 8, 16, a, None, c) == (0, 1, 1)
    assert _plan(L, 2, 64, 7, 13, a, b, c) == (0, 1, 0)
    assert _plan(L, 2, 64, 6, 9, a, b, c)[2] == 0          # 54 % 4 == 2
    for off in ((4, 0, 0), (0, 4, 0), (0, 0, 4), (8, 0, 0)):
        assert _plan(L, 2, 64, 8, 16, a + off[0], b + off[1], c + off[2]) == (0, 1, 0)
    # slicing: one workgroup per plane where B * C planes fill the chip, several for a few planes of a large frame
    rc, s_train, _ = _plan(L, 32, 64, 192, 192, a, b, c)
    assert rc == 0 and s_train == 1
    rc, s_infer, vec = _plan(L, 1, 16, 96, 160, a, b, c)
    assert rc == 0 and s_infer > 1 and vec == 1
    for (B, C, H, W), S in (((32, 64, 192, 192), s_train), ((1, 16, 96, 160), s_infer)):
        assert L.rvsr_channel_attention_workspace_bytes(B, C, H, W) >= 4 * B * C * S
    # never more slices than a plane has 4096-element pieces, never more than 64
    for (B, C, H, W), want in (((1, 3, 97, 161), 4), ((1, 64, 1080, 1920), 16), ((2, 8, 33, 31), 1), ((1, 1, 2160, 3840), 64)):
        assert _plan(L, B, C, H, W, a, b, c)[:2] == (0, want)
    # refusals: more channels than the LDS scratch holds, empty shapes
    assert _plan(L, 1, 8192, 8, 8, a, b, c)[0] == 1 and b'LDS' in L.rvsr_last_error()
    assert _plan(L, 0, 64, 8, 8, a, b, c)[0] != 0
