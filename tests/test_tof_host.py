"""TOF without a GPU: the module tree against the reference's (fixtures tof.npz, tof_s4.npz), define_G's branch and its refusals, the exported symbols
of the resampling operators, the plans of the 7x7 convolutions on host addresses, and the refusal of CPU tensors."""
import pytest
import torch

from conftest import load_golden
from conv_ledger import fwd_call, fwd_plan, wgrad_call, wgrad_plan

CASES = {'k3': dict(nframes=3, K=3, in_nc=3, out_nc=3, nf=32, nb=2, upscale=1),
         'k2': dict(nframes=3, K=2, in_nc=3, out_nc=3, nf=16, nb=1, upscale=1),
         'k1s4': dict(nframes=5, K=1, in_nc=3, out_nc=3, nf=16, nb=1, upscale=4)}
# network_G of train_TOF_RealVSR_YCbCr_Split.yml (scale 1 in that file)
OPTION_FILE_G = dict(which_model_G='TOF', nf=64, nc=3, nframes=3, nb=10, K=3)
SYMBOLS = ('rvsr_flow_warp_forward', 'rvsr_flow_warp_backward', 'rvsr_avgpool2_forward', 'rvsr_avgpool2_backward',
           'rvsr_upsample2_ac_forward', 'rvsr_upsample2_ac_backward')
SPYNET_LAYERS = [(6, 32), (8, 32), (32, 64), (64, 32), (32, 16), (16, 2)]
CONV_FWD_F32, CONV_WGRAD_F32_7 = 3, 10


@pytest.mark.parametrize('tag', list(CASES))
def test_state_dict_matches_reference(tag):
    from realvsr_amd.archs.TOF_arch import TOF
    g = {**load_golden('tof'), **load_golden('tof_s4')}      # (k3 and k2; k1s4)
    sd = TOF(**CASES[tag]).state_dict()
    assert list(sd.keys()) == [str(k) for k in g[tag + '.keys']]
    for (k, v), shape in zip(sd.items(), g[tag + '.shapes']):
        assert list(v.shape) == [int(n) for n in shape[:v.dim()]] and all(int(n) == 0 for n in shape[v.dim():]), k
    assert 'align_arch.block0.block.0.weight' in sd and tuple(sd['align_arch.block0.block.0.weight'].shape) == (32, 6, 7, 7)
    assert tuple(sd['align_arch.blocks.%d.block.12.weight' % (CASES[tag]['K'] - 1)].shape) == (2, 16, 7, 7)
    assert ('sr_arch.upconv2.weight' in sd) == (CASES[tag]['upscale'] == 4)


def test_define_g_builds_tof_from_the_option_file_block():
    from realvsr_amd.VideoSR_archs import define_G
    from realvsr_amd.archs.TOF_arch import TOF, SpyNet_Block
    net = define_G({'scale': 1, 'network_G': dict(OPTION_FILE_G)})
    assert isinstance(net, TOF) and net.nframes == 3 and net.align_arch.K == 3 and len(net.align_arch.blocks) == 3
    assert net.sr_arch.conv_first.in_channels == 9 and net.sr_arch.conv_first.out_channels == 64 and len(net.sr_arch.recon_trunk) == 10
    assert net.sr_arch.conv_last.out_channels == 3 and net.sr_arch.upscale == 1 and not hasattr(net.sr_arch, 'upconv1')
    assert isinstance(net.align_arch.block0, SpyNet_Block) and net.align_arch.block0.block[0].in_channels == 6
    kinds = [type(m).__name__ for m in net.align_arch.blocks[0].block]
    assert kinds == ['Conv2d', 'BatchNorm2d', 'ReLU'] * 4 + ['Conv2d']
    net4 = define_G({'scale': 4, 'network_G': dict(OPTION_FILE_G, nframes=5)})
    assert net4.sr_arch.conv_first.in_channels == 15 and net4.sr_arch.upconv2.out_channels == 256


def test_initialisation_follows_the_reference():
    """At upscale 1 only the residual blocks carry the 0.1 scale; at 2 / 4 conv_first, the upconvs, HRconv and conv_last do too."""
    from realvsr_amd.archs.TOF_arch import MSRResNet
    torch.manual_seed(0)
    one, four = MSRResNet(9, 3, 64, 2, 1), MSRResNet(9, 3, 64, 2, 4)
    kaiming = (2.0 / (64 * 9)) ** 0.5
    assert abs(one.recon_trunk[0].conv1.weight.std().item() / (0.1 * kaiming) - 1) < 0.1
    assert one.HRconv.weight.std().item() > 3 * 0.1 * kaiming
    assert abs(four.HRconv.weight.std().item() / (0.1 * kaiming) - 1) < 0.1 and abs(four.upconv2.weight.std().item() / (0.1 * kaiming) - 1) < 0.1
    assert not four.HRconv.bias.any() and not four.conv_last.bias.any()


def test_refusals():
    from realvsr_amd import functional as RF
    from realvsr_amd.VideoSR_archs import define_G
    from realvsr_amd.archs import arch_util
    from realvsr_amd.archs.TOF_arch import TOF, MSRResNet, SpyNet
    for drop in ('nframes', 'K', 'nc', 'nf', 'nb'):
        block = {k: v for k, v in OPTION_FILE_G.items() if k != drop}
        with pytest.raises(NotImplementedError, match=drop):
            define_G({'scale': 1, 'network_G': block})
    with pytest.raises(NotImplementedError, match='scale'):
        define_G({'network_G': dict(OPTION_FILE_G)})
    with pytest.raises(NotImplementedError, match='upscale 3'):
        define_G({'scale': 3, 'network_G': dict(OPTION_FILE_G)})
    with pytest.raises(NotImplementedError, match='upscale 3'):
        MSRResNet(upscale=3)
    x, flow = torch.randn(1, 3, 8, 8), torch.zeros(1, 8, 8, 2)
    for fn in (RF.flow_warp, arch_util.flow_warp):
        with pytest.raises(NotImplementedError, match='reflection'):
            fn(x, flow, padding_mode='reflection')
        with pytest.raises(NotImplementedError, match='bicubic'):
            fn(x, flow, interp_mode='bicubic')
    with pytest.raises(RuntimeError, match='divisible by 2\\*\\*K = 8'):     # (the check comes before any kernel)
        SpyNet(K=3)(torch.randn(1, 3, 20, 16), torch.randn(1, 3, 20, 16))
    with pytest.raises(RuntimeError, match='divisible'):
        TOF(nframes=3, K=2, nf=16, nb=1, upscale=1)(torch.randn(1, 3, 3, 16, 18))


def test_cpu_tensors_are_refused():
    from realvsr_amd import functional as RF
    from realvsr_amd.archs.TOF_arch import TOF
    x = torch.randn(1, 3, 8, 8)
    with pytest.raises(NotImplementedError):
        RF.flow_warp(x, torch.zeros(1, 8, 8, 2))
    with pytest.raises(NotImplementedError):
        RF.avg_pool2(x)
    with pytest.raises(NotImplementedError):
        RF.upsample2_ac(x, 2.0)
    with pytest.raises(NotImplementedError):
        RF.conv2d(x, torch.nn.Conv2d(3, 8, 7, 1, 3))
    with pytest.raises(NotImplementedError):
        TOF(nframes=3, K=1, nf=16, nb=1, upscale=1)(torch.randn(1, 3, 3, 8, 8))
    with pytest.raises(NotImplementedError):
        TOF(nframes=1, K=1, nf=16, nb=1, upscale=1)(torch.randn(1, 1, 3, 8, 8))      # no SpyNet at one frame: the first conv refuses


def test_library_exports_the_flow_symbols():
    from realvsr_amd import _lib
    L = _lib.lib()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert all(name + '(' in header for name in SYMBOLS)
    assert 'TOF_arch.py' in header and 'arch_util.py:47-80' in header


def test_flow_entries_validate_before_they_launch():
    """Bad arguments and unsupported modes return their codes on host addresses: nothing is launched, nothing dereferenced."""
    import ctypes
    from realvsr_amd import _lib
    L = _lib.lib()
    a, b, c = (ctypes.c_void_p(v << 20) for v in (1, 2, 3))
    assert L.rvsr_flow_warp_forward(a, b, c, 1, 3, 8, 8, 0, 2, None) == 1 and b'reflection' in L.rvsr_last_error()
    assert L.rvsr_flow_warp_forward(a, b, c, 1, 3, 8, 8, 2, 0, None) == 1 and b'interpolation' in L.rvsr_last_error()
    assert L.rvsr_flow_warp_forward(a, b, c, 1, 3, 0, 8, 0, 0, None) == 2
    assert L.rvsr_flow_warp_forward(a, None, c, 1, 3, 8, 8, 0, 0, None) == 2
    assert L.rvsr_flow_warp_backward(a, None, b, None, c, 1, 3, 8, 8, 0, 0, None) == 2      # a flow gradient needs the image
    assert L.rvsr_flow_warp_backward(a, None, b, None, None, 1, 3, 8, 8, 0, 0, None) == 0   # neither gradient wanted: nothing to do
    assert L.rvsr_avgpool2_forward(a, None, 6, 1, 8, None) == 0                             # one row pools to nothing: no launch
    assert L.rvsr_avgpool2_forward(a, b, 0, 8, 8, None) == 2
    assert L.rvsr_upsample2_ac_forward(a, None, 6, 8, 8, 2.0, None) == 2
    assert L.rvsr_upsample2_ac_backward(a, b, 6, 0, 8, 2.0, None) == 2


@pytest.mark.parametrize('mode', ['bf16x3', 'f32', 'bf16x2', 'bf16'])
def test_conv7_forward_plan_is_the_exact_f32_family(mode):
    for C, Co in SPYNET_LAYERS + [(64, 136)]:
        for w_mode in (0, 1):
            for B, H, W in ((2, 2, 3), (32, 192, 192)):
                rc, row = fwd_plan(fwd_call(C, Co, H, W, H, W, B, k=7, w_mode=w_mode), mode)
                mt = 1 if Co <= 32 else 2 if Co <= 64 else 4
                assert rc == 0 and (row['family'], row['MT'], row['CC']) == (CONV_FWD_F32, mt, 2 if mt == 4 else 4), (C, Co, mode, row)
                assert row['CC'] % 2 == 0 and row['lds'] <= 64 * 1024, row          # two workgroups per CU, channel pairs over the lane halves
                assert (row['gx'], row['gy'], row['gz']) == ((W + 31) // 32 * ((H + 7) // 8), (Co + 32 * mt - 1) // (32 * mt), B)
    assert fwd_plan(fwd_call(32, 64, 8, 8, 8, 8, 1, k=7), mode)[1]['lds'] == 4 * (4 * 14 * 38 + 49 * 4 * 65)       # 59.5 KB
    assert fwd_plan(fwd_call(64, 136, 8, 8, 8, 8, 1, k=7), mode)[1]['lds'] == 4 * (2 * 14 * 38 + 49 * 2 * 129)     # 54.8 KB


def test_conv7_refusals_of_the_entries():
    from realvsr_amd import _lib
    L = _lib.lib()
    rc, _ = fwd_plan(fwd_call(32, 64, 16, 16, 8, 8, 1, k=7, stride=2))
    assert rc == 1 and b'stride' in L.rvsr_last_error()
    rc, _ = fwd_plan(fwd_call(32, 64, 16, 16, 16, 16, 1, k=7, w_mode=4))
    assert rc == 1 and b'f16 + fp8' in L.rvsr_last_error()
    rc, _ = wgrad_plan(wgrad_call(32, 64, 16, 16, 8, 8, 1, k=7, stride=2))
    assert rc == 1 and b'stride' in L.rvsr_last_error()
    rc, _ = fwd_plan(fwd_call(32, 64, 16, 16, 16, 16, 1, k=9))
    assert rc == 1 and b'kernel size 9' in L.rvsr_last_error()
    assert L.rvsr_conv2d_forward_workspace_bytes(32, 0, 64, 7) == 0      # no packed image exists for 7x7
    assert L.rvsr_conv2d_pack_weights(None, 32, 64, 7, 0, None, 0, None, None) == 0


@pytest.mark.parametrize('mode', ['bf16x3', 'f32'])
def test_conv7_weight_gradient_plan_and_workspace(mode):
    from realvsr_amd import _lib
    L = _lib.lib()
    for C, Co in SPYNET_LAYERS:
        for B, H, W in ((2, 2, 3), (1, 5, 9), (2, 16, 24), (32, 192, 192)):
            for gact in (False, True):
                rc, row = wgrad_plan(wgrad_call(C, Co, H, W, H, W, B, k=7, gact=gact), mode)
                assert rc == 0 and row['family'] == CONV_WGRAD_F32_7 and row['P'] >= 1, (C, Co, B, H, W, row)
                assert (row['gy'], row['gz']) == ((Co + 63) // 64, (C + 7) // 8)
                ws = L.rvsr_conv2d_wgrad_workspace_bytes(C, 0, Co, B, 7, 1, H, W)
                assert ws >= 4 * row['P'] * (Co * C * 49 + Co), (C, Co, B, H, W, row, ws)


def test_packed_weight_cache_leaves_7x7_out():
    from realvsr_amd.caches import PackedWeights
    w = torch.nn.Parameter(torch.randn(32, 8, 7, 7))
    w._rvsr_grad_home = (None, 0, set())     # (as a parameter inside FlatBuffers looks)
    cache = PackedWeights()
    assert cache.get(w, 'conv', 8, 32, 7, 0, 0) is None and not cache.entries
