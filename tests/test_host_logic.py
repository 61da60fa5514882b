"""CPU-side checks of the boundary: the C-ABI library loads and exports every symbol the header
declares, the Python mirror keeps the reference's API / state_dict schema, and nothing silently
falls back to the CPU."""
import os
import re

import pytest
import torch

from conftest import REPO, load_golden, golden_sd


def _header_symbols():
    text = open(os.path.join(REPO, 'include', 'realvsr_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(rvsr_[a-z0-9_]+)\s*\(', text)))


def test_library_exports_every_declared_symbol():
    from realvsr_amd import _lib
    _lib.build()
    L = _lib.lib()
    declared = _header_symbols()
    assert len(declared) >= 24
    for name in declared:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, 'ctypes signature missing for ' + name
    assert sorted(_lib.SIGNATURES) == declared


def test_ctypes_signatures_come_from_the_header():
    """One entry of each kind the header holds, against literal expectations (the table itself is realvsr_amd._lib.parse_header's
    reading of include/realvsr_hip.h)."""
    import ctypes as C
    from realvsr_amd import _lib
    S = _lib.SIGNATURES
    p, i, f, d, z = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t
    same = lambda got, want: got[0] is want[0] and len(got[1]) == len(want[1]) and all(a is b for a, b in zip(got[1], want[1]))  # noqa: E731
    conv_call = [p, i, p, i, p, f, i, i, i, p, p, p, p, i, p, i, i, i, i, i, i, f, i, i, i]
    expected = {
        'rvsr_last_error': (C.c_char_p, []),
        'rvsr_set_gemm_mode': (None, [i]),
        'rvsr_reduce_workspace_bytes': (z, []),
        'rvsr_charbonnier_forward': (i, [p, p, z, f, d, p, p, p]),
        'rvsr_conv2d_forward_plan': (i, conv_call + [C.POINTER(C.c_int)]),                              # host int*
        'rvsr_conv2d_pack_weights': (z, [p, i, i, i, i, p, z, C.POINTER(C.c_longlong), p]),             # host long long*
        'rvsr_bn_lrelu_forward': (i, [p] * 9 + [i] * 4 + [f] * 3 + [p, z, p]),                          # argument 5: a DEVICE long long*
        'rvsr_maxavgpool_forward': (i, [p, p, p, i, i, i, i, p]),                                       # unsigned char*
        'rvsr_dcn_forward_halo': (i, [p, z, i]),                                                        # const unsigned*, read on the host
        'rvsr_conv2d_backward_weight': (i, [p, i, p, i, i, i, p, p, f, i, i, i, p, p, i, i, i, i, i, i, i, p, z, p]),   # five lines
    }
    for name, want in expected.items():
        assert same(S[name], want), (name, S[name])
    assert len(S['rvsr_conv2d_backward_weight'][1]) == 24 and S['rvsr_bn_lrelu_forward'][1][5] is p
    assert (_lib.RVSR_OK, _lib.RVSR_ERR_UNSUPPORTED, _lib.RVSR_ERR_BAD_ARG, _lib.RVSR_ERR_LAUNCH, _lib.RVSR_ERR_WORKSPACE) == (0, 1, 2, 3, 4)


def test_header_parser_refuses_what_it_does_not_know():
    """Nothing is skipped: an unmapped type, a marker on a type that has no typed pointer, and a statement that is no prototype all raise,
    and the message names the entry."""
    import ctypes as C
    from realvsr_amd._lib import parse_header
    sigs, codes = parse_header('#define RVSR_X 7 /* c */\n#define RVSR_HOST\nint rvsr_a(const float* x, /* c */ RVSR_HOST int* n,\n size_t k);')
    assert codes == {'RVSR_X': 7} and list(sigs) == ['rvsr_a']
    assert sigs['rvsr_a'][0] is C.c_int and sigs['rvsr_a'][1] == [C.c_void_p, C.POINTER(C.c_int), C.c_size_t]
    for text in ('int rvsr_ok(int a);\nint rvsr_bad(short x);', 'int rvsr_bad(int a, short* x);', 'short rvsr_bad(void);',
                 'int rvsr_bad(RVSR_HOST float* x);', 'int rvsr_bad(RVSR_HOST int n);', 'int rvsr_bad(int);', 'int rvsr_bad(int a) int rvsr_b(int a);',
                 'int rvsr_bad(int a, void (*f)(int));', 'typedef int rvsr_bad;', 'int rvsr_bad(int a);\nfloat rvsr_bad(int a);'):
        with pytest.raises(ValueError, match='rvsr_bad'):
            parse_header(text)


def test_operators_refuse_cpu_tensors():
    from realvsr_amd.archs.dcn import modulated_deform_conv, ModulatedDeformConvPack
    from realvsr_amd.archs.EDVR_arch import EDVR
    from realvsr_amd import loss as L
    with pytest.raises(NotImplementedError):
        modulated_deform_conv(torch.randn(1, 8, 4, 4), torch.zeros(1, 18, 4, 4), torch.ones(1, 9, 4, 4),
                              torch.randn(8, 8, 3, 3), None, 1, 1, 1, 1, 1)
    with pytest.raises(NotImplementedError):
        ModulatedDeformConvPack(8, 8, 3, padding=1, deformable_groups=1)(torch.randn(1, 8, 4, 4))
    with pytest.raises(NotImplementedError):
        EDVR(nf=16, nframes=3, groups=4, front_RBs=1, back_RBs=1)(torch.rand(1, 3, 3, 8, 8))
    with pytest.raises(NotImplementedError):
        L.LapPyrLoss(3, 'cb', 'cb')(torch.rand(1, 1, 16, 16), torch.rand(1, 1, 16, 16))
    with pytest.raises(NotImplementedError):
        L.LapPyrLoss(3, 'ssim', 'cb')(torch.rand(1, 1, 64, 64), torch.rand(1, 1, 64, 64))
    with pytest.raises(NotImplementedError):
        L.PyramidLoss(3, 'gau', 'hb')(torch.rand(1, 1, 16, 16), torch.rand(1, 1, 16, 16))
    with pytest.raises(ValueError):
        L.LapPyrLoss(3, 'l1', 'cb')      # loss.py:205-206
    with pytest.raises(ValueError):
        L.PyramidLoss(3, 'gau', 'ssim')  # loss.py:176-177


def test_state_dict_schema_matches_reference():
    """Keys/shapes of the fixtures come from instantiating the reference modules (make_golden.py)."""
    from realvsr_amd.archs.EDVR_arch import EDVR, PCD_Align, TSA_Fusion
    from realvsr_amd.archs.dcn import ModulatedDeformConvPack
    for name, mod in [('edvr_tsa', EDVR(nf=16, nc=3, nframes=3, groups=4, front_RBs=2, back_RBs=2, w_TSA=True)),
                      ('pcd_align', PCD_Align(nf=16, groups=4)), ('tsa_fusion', TSA_Fusion(nf=16, nframes=3, center=1)),
                      ('dcn_pack', ModulatedDeformConvPack(16, 12, 3, stride=1, padding=1, dilation=1,
                                                           deformable_groups=4, extra_offset_mask=True))]:
        mod.load_state_dict(golden_sd(load_golden(name)), strict=True)
    net = EDVR(nf=64, nc=3, nframes=5, groups=8, front_RBs=5, back_RBs=10, w_TSA=True)
    assert len(net.state_dict()) == 144 and sum(p.numel() for p in net.parameters()) == 3300131
    pack = ModulatedDeformConvPack(16, 12, 3, padding=1, deformable_groups=4)
    assert float(pack.conv_offset_mask.weight.abs().sum()) == 0.0 and float(pack.bias.abs().sum()) == 0.0


def test_define_g():
    from realvsr_amd.VideoSR_archs import define_G
    from realvsr_amd.archs.EDVR_arch import EDVR_NoUp
    opt = {'network_G': {'which_model_G': 'EDVR_NoUp', 'nf': 64, 'nc': 3, 'nframes': 3, 'groups': 8, 'front_RBs': 5,
                         'back_RBs': 10, 'w_TSA': False}}
    net = define_G(opt)
    assert isinstance(net, EDVR_NoUp) and net.center == 1 and isinstance(net.tsa_fusion, torch.nn.Conv2d)
    from realvsr_amd.archs.TDAN_arch import TDAN
    tdan = define_G({'scale': 1, 'network_G': {'which_model_G': 'TDAN', 'nf': 64, 'nc': 3, 'nframes': 3, 'nb_f': 1,
                                               'nb_b': 1, 'groups': 8}})
    assert isinstance(tdan, TDAN)
    with pytest.raises(NotImplementedError):
        define_G({'network_G': {'which_model_G': 'RCAN'}})


def test_create_model_refuses_cpu_and_unknown_models():
    from realvsr_amd.VideoSR_model import create_model
    opt = {'model': 'VideoSR_AllPair_YCbCr_Split', 'gpu_ids': None, 'is_train': True, 'dist': False,
           'network_G': {'which_model_G': 'EDVR', 'nf': 16, 'nc': 3, 'nframes': 3, 'groups': 4, 'front_RBs': 1,
                         'back_RBs': 1, 'w_TSA': True}}
    with pytest.raises(NotImplementedError):
        create_model(opt)                     # no CPU path
    with pytest.raises(NotImplementedError):
        create_model(dict(opt, model='VideoSRGAN_AllPair_YCbCr_Split'))


@pytest.mark.parametrize('name', ['VideoSR_AllPair_YCbCr_Split', 'VideoSR_AllPair_YCbCr_Combine', 'VideoSRGAN_AllPair_YCbCr_Split'])
def test_every_model_gets_the_training_loops_methods_from_one_base(name, monkeypatch):
    """What realvsr_amd.train calls exists on the class create_model picks, and the methods that do not depend on the losses are
    defined once, in the base of both model classes: neither class carries its own copy or borrows the other's."""
    from realvsr_amd import VideoSR_model as M
    with pytest.raises(NotImplementedError, match='no CPU path'):
        M.create_model({'model': name, 'gpu_ids': None})          # refused before any other key is read
    for cls in (M.VideoSRModel, M.VideoSRGANModel):
        monkeypatch.setattr(cls, '__init__', lambda self, *a, **k: None)
    cls = type(M.create_model({'model': name}))
    assert cls is (M.VideoSRGANModel if 'GAN' in name else M.VideoSRModel)
    for method in ('resume_training', 'update_learning_rate', 'feed_data', 'optimize_parameters', 'get_current_learning_rate',
                   'get_current_log', 'save', 'save_training_state', 'test', 'get_current_metrics', 'get_current_visuals'):
        assert callable(getattr(cls, method)), method
    shared = ('load_network', 'save_network', 'get_current_metrics', 'test', 'get_current_log', 'get_current_visuals',
              'get_current_learning_rate')
    for method in shared:
        assert method not in M.VideoSRGANModel.__dict__ and method not in M.VideoSRModel.__dict__, method
        owners = [c for c in cls.__mro__ if method in c.__dict__]
        assert len(owners) == 1 and issubclass(M.VideoSRModel, owners[0]) and issubclass(M.VideoSRGANModel, owners[0]), method


def test_flat_buffers_layout_and_guards():
    """optim.FlatBuffers: parameters and gradients become views of two identically laid-out buffers (CPU tensors are
    fine for the layout logic); re-binding a gradient is detected."""
    from realvsr_amd.optim import FlatBuffers
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.Conv2d(5, 2, 1))
    before = [p.detach().clone() for p in net.parameters()]
    fb = FlatBuffers([list(net.parameters())])
    assert fb.order[0] is list(net.parameters())[-1]          # reverse registration order
    for p, b in zip(net.parameters(), before):
        assert torch.equal(p.detach(), b)
        assert fb.offset[p] % 64 == 0
        assert p.data_ptr() == fb.param.data_ptr() + 4 * fb.offset[p]
        assert p.grad.data_ptr() == fb.grad.data_ptr() + 4 * fb.offset[p]
    net(torch.randn(2, 3, 6, 6)).sum().backward()
    assert float(fb.grad.abs().sum()) > 0                      # autograd accumulated into the views
    fb.check_bound()
    # zero_grad: one memset, p.grad = None until backward delivers (autograd then ADOPTS the incoming tensor; the fused operators
    # deliver the flat view itself, a plain torch module delivers a temporary that rebind() copies home)
    fb.zero_grad()
    assert all(p.grad is None for p in net.parameters()) and float(fb.grad.abs().sum()) == 0
    fb.check_bound()
    net(torch.randn(2, 3, 6, 6)).sum().backward()
    with pytest.raises(RuntimeError):
        fb.check_bound()                                       # adopted temporaries live outside the flat buffer ...
    want = [p.grad.clone() for p in net.parameters()]
    fb.rebind()
    fb.check_bound()                                           # ... until rebind() copies them home
    for p, w in zip(net.parameters(), want):
        assert p.grad.data_ptr() == fb.grad.data_ptr() + 4 * fb.offset[p] and torch.equal(p.grad, w)
    net.zero_grad(set_to_none=True)
    fb.rebind()
    fb.check_bound()
    # the hook the fused operators use: a parameter without a gradient gets its flat view as the output buffer
    from realvsr_amd.functional import _pgrad
    p0 = next(net.parameters())
    p0.grad = None
    assert _pgrad(p0).data_ptr() == fb.grad.data_ptr() + 4 * fb.offset[p0]
    p0.grad = torch.zeros_like(p0)
    assert _pgrad(p0).data_ptr() != fb.grad.data_ptr() + 4 * fb.offset[p0]


def test_pgrad_hands_a_home_out_once_per_step():
    """functional._pgrad: a parameter used by TWO fused operators in one backward must not get the same
    flat-buffer view twice -- AccumulateGrad has not run between the uses, p.grad is still None, and aliased outputs would turn
    g1 + g2 into 2 * g_last.  Emulated on CPU with an autograd Function that writes its weight gradient the way the fused
    operators do."""
    from realvsr_amd.functional import _pgrad
    from realvsr_amd.optim import FlatBuffers

    class Scale(torch.autograd.Function):     # y = w * x, gradient of w written into _pgrad's buffer
        @staticmethod
        def forward(ctx, x, w):
            ctx.save_for_backward(x)
            ctx.w = w
            return x * w

        @staticmethod
        def backward(ctx, g):
            (x,) = ctx.saved_tensors
            gw = _pgrad(ctx.w)
            gw.copy_(g * x)
            return g * ctx.w, gw

    w = torch.nn.Parameter(torch.tensor([1., 2., 3., 4.]))
    fb = FlatBuffers([[w]])
    fb.zero_grad()
    x1, x2 = torch.tensor([1., 2., 3., 4.]), torch.tensor([10., 20., 30., 40.])
    (Scale.apply(x1, w) + Scale.apply(x2, w)).sum().backward()
    fb.rebind()
    assert torch.equal(w.grad, x1 + x2)                     # not 2 * x1 (or 2 * x2)
    assert w.grad.data_ptr() == fb.grad.data_ptr() + 4 * fb.offset[w]
    # next step: the home can be claimed again; a first use gets the flat view, the second a temporary
    fb.zero_grad()
    a, b = _pgrad(w), _pgrad(w)
    assert a.data_ptr() == fb.grad.data_ptr() + 4 * fb.offset[w] and b.data_ptr() != a.data_ptr()
    # torch.autograd.grad(): the fused backward wrote into the home but autograd handed the result to the caller, not to
    # p.grad -- rebind() must not present that as this step's gradient
    fb.zero_grad()
    (gw,) = torch.autograd.grad(Scale.apply(x1, w).sum(), [w])
    assert torch.equal(gw, x1) and w.grad is None
    fb.rebind()
    assert float(w.grad.abs().sum()) == 0


def test_gradsink_refuses_concat_convs():
    from realvsr_amd import functional as RF
    x = torch.zeros(1, 2, 4, 4)
    conv = torch.nn.Conv2d(4, 2, 3, padding=1)
    with pytest.raises((RuntimeError, NotImplementedError)) as e:
        RF.conv2d(x, conv, x2=x, sink=RF.GradSink())
    # the sink check comes first (a CPU tensor would raise NotImplementedError after it)
    assert 'GradSink' in str(e.value)


def test_gauss_kernel_gain_cache_is_not_fooled_by_address_reuse():
    from realvsr_amd import util
    k = util.gauss_kernel(channels=3)
    assert util._kernel_gain(k) == 1.0 and util._kernel_gain(4 * k) == 4.0
    other = k.clone()
    assert util._kernel_gain(other) == 1.0
    other[0, 0, 0, 0] = 7.0                                   # same object, new version: validated again
    with pytest.raises(NotImplementedError):
        util._kernel_gain(other)
    k.mul_(2.0)                                                # the tag of gauss_kernel() only holds for version 0
    assert util._kernel_gain(k) == 2.0


def test_cutblur_box_follows_python_slice_semantics():
    """with alpha near 0 the reference's cut_ratio can go negative; [cy:cy+ch] then wraps like a python slice.
    And the resolution check precedes every RNG draw (data/augments_video_allpair.py:55-56)."""
    import numpy as np
    from realvsr_amd import augment
    plan = augment.AugPlan()
    np.random.seed(3)
    state = np.random.get_state()
    with pytest.raises(ValueError):
        augment._draw_cutblur(plan, (1, 2, 3, 8, 8), 1.0, 0.7, size1=(1, 2, 3, 4, 4))
    assert all(np.array_equal(a, b) for a, b in zip(state[1:3], np.random.get_state()[1:3]))   # nothing drawn
    # brute-force the reference's arithmetic for a negative ratio and compare the box with an actual slice assignment
    for seed in range(40):
        np.random.seed(seed)
        size = (1, 2, 3, 9, 11)
        plan = augment.AugPlan()
        augment._draw_cutblur(plan, size, 1.0, 0.004)
        np.random.seed(seed)
        np.random.rand(1)
        ratio = np.random.randn() * 0.01 + 0.004
        h, w = size[2], size[3]
        ch, cw = int(h * ratio), int(w * ratio)
        cy, cx = np.random.randint(0, h - ch + 1), np.random.randint(0, w - cw + 1)
        m = np.zeros(size[-2:], bool)
        m[cy:cy + ch, cx:cx + cw] = True
        y0, y1, x0, x1 = plan.box
        m2 = np.zeros(size[-2:], bool)
        m2[y0:y1, x0:x1] = True
        assert np.array_equal(m, m2), (seed, plan.box, (cy, ch, cx, cw))


def test_flat_adam_skips_missing_grads_and_resets_state():
    """torch.optim.Adam semantics the dense flat update must keep: parameters whose grad is None do not move,
    and clearing optimizer.state (MultiStepLR_Restart(clear_state=True)) restarts the moments.  The kernel launch itself needs a
    GPU; here the arithmetic is replaced by torch's so that the host logic around it is what is tested."""
    from realvsr_amd import optim, functional as RF

    def adam_cpu(param, grad, m, v, step_size, b1, b2, eps, wd, bc2s):
        g = grad + wd * param if wd else grad
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        param.addcdiv_(m, v.sqrt() / bc2s + eps, value=-step_size)

    orig = RF.adam_step_
    RF.adam_step_ = adam_cpu
    try:
        torch.manual_seed(0)
        a, b = torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(7))
        ra, rb = torch.nn.Parameter(a.detach().clone()), torch.nn.Parameter(b.detach().clone())
        opt, ref = optim.FlatAdam([a, b], lr=1e-2, weight_decay=0.1), torch.optim.Adam([ra, rb], lr=1e-2, weight_decay=0.1)
        for it in range(4):
            opt.zero_grad()
            ref.zero_grad(set_to_none=True)
            (a * a).sum().backward()
            (ra * ra).sum().backward()
            if it != 1:                        # step 1: b gets no gradient at all
                (b * 3).sum().backward()
                (rb * 3).sum().backward()
            b_before, m_before = b.detach().clone(), opt.state[b]['exp_avg'].clone() if b in opt.state else None
            opt.step()
            ref.step()
            assert torch.allclose(a, ra, atol=1e-6), it
            if it <= 1:
                # (after a skipped step torch's PER-PARAMETER step count lags the group's; FlatAdam counts per group -- documented)
                assert torch.allclose(b, rb, atol=1e-6), it
            if it == 1:
                assert torch.equal(b.detach(), b_before) and torch.equal(opt.state[b]['exp_avg'], m_before)
            if it == 2:                        # restart: the reference's scheduler empties optimizer.state
                from collections import defaultdict
                opt.state = defaultdict(dict)
                ref.state = defaultdict(dict)
        assert float(opt.state[a]['step']) == 1.0
    finally:
        RF.adam_step_ = orig


def test_every_autograd_function_carries_the_device_guard():
    """VERDICT r2 #8 / deform_conv_cuda.cpp:499,581 (at::DeviceGuard): every fused operator's forward AND backward run under
    torch.cuda.device(<device of its tensors>) when that is not the current device.  The guard is applied to all Function
    classes of realvsr_amd.functional at import time; here: none was missed, and it switches (recorded with a stand-in context
    manager on CPU tensors that claim to live on cuda:1)."""
    import torch.autograd
    from realvsr_amd import functional as RF
    fns = [c for c in vars(RF).values() if isinstance(c, type) and issubclass(c, torch.autograd.Function) and c is not torch.autograd.Function]
    assert len(fns) >= 18
    for c in fns:
        assert hasattr(c.forward, '__wrapped__') and hasattr(c.backward, '__wrapped__'), c.__name__

    entered = []

    class FakeTensor:
        is_cuda = True
        device = torch.device('cuda', 1)

    class Recorder:
        def __init__(self, dev):
            self.dev = dev

        def __enter__(self):
            entered.append(self.dev)

        def __exit__(self, *a):
            return False

    import unittest.mock as mock
    with mock.patch.object(torch, 'is_tensor', lambda t: isinstance(t, FakeTensor)), \
            mock.patch.object(torch.cuda, 'current_device', lambda: 0), mock.patch.object(torch.cuda, 'device', Recorder):
        guarded = RF._guarded(lambda ctx, *a: 'ran')
        assert guarded(None, FakeTensor()) == 'ran' and entered == [torch.device('cuda', 1)]
        entered.clear()
        FakeTensor.device = torch.device('cuda', 0)          # already current: no switch
        assert guarded(None, FakeTensor()) == 'ran' and entered == []


def test_no_matrix_core_instruction_overwrites_its_own_operand():
    """hipcc may allocate the destination of an accumulator's FIRST MFMA (SrcC = 0, untied form) on top of an operand that dies at the
    instruction; on the MI355X the products of the upper operand half then come out wrong, differently from run to run (round 5,
    profiles/r05_notes.md; bf16x3.h: mfma_bf16_first).  tools/check_mfma_overlap.py compiles a kernel file to gfx950 ISA and looks for
    the pattern: run here on dcn6_kernels.hip, whose kernels start accumulators that way (no GPU needed; under a minute)."""
    import shutil
    import subprocess
    import sys
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not on PATH')
    csrc = os.path.join(REPO, 'realvsr_amd', 'csrc')
    out = subprocess.run([sys.executable, os.path.join(REPO, 'tools', 'check_mfma_overlap.py'), os.path.join(csrc, 'dcn6_kernels.hip')],
                         capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert '0 overlapping' in out.stdout


def test_packed_weights_validity_rules_on_cpu():
    """caches.PackedWeights, what its docstring promises, without a GPU: the three pack entries of the library are replaced by a
    recorder, the parameters are CPU tensors that carry a `_rvsr_grad_home` as optim.FlatBuffers would give them."""
    import contextlib
    import gc
    import unittest.mock as mock
    from realvsr_amd import _lib, caches

    calls = []

    class FakeLib:
        def rvsr_conv2d_pack_weights(self, w, C, Co, k, mode, buf, n, desc, stream):
            calls.append(('conv', w.value, C, Co, k, mode))
            if desc is not None:
                desc[0], desc[1] = w.value, buf.value
                for i in range(2, 10):
                    desc[i] = 100 * len(calls) + i
            return 64

        def rvsr_dcn_pack_weights(self, w, C, Co, buf, n, desc, stream):
            calls.append(('dcn', w.value, C, Co))
            assert desc is None or len(desc) == 20      # the library writes 20 values
            return 64

        def rvsr_pack_weights_batched(self, tab, n, stream):
            calls.append(('batched', tab.value, n))
            return 0

    def param(*shape):
        p = torch.nn.Parameter(torch.randn(*shape))
        p._rvsr_grad_home = (None, 0, set())
        return p

    with mock.patch.object(_lib, 'lib', lambda: FakeLib()), mock.patch.object(_lib, 'get_gemm_mode', lambda: 'bf16x3'), \
            mock.patch.object(caches, '_stream', lambda: None), mock.patch.object(torch.cuda, 'device', lambda d: contextlib.nullcontext()):
        pw = caches.PackedWeights()
        pw.enabled = True
        w, geo = param(8, 4, 3, 3), ('conv', 4, 8, 3, 0, 64)
        # weights without a home in FlatBuffers are never cached; the f32 mode stages no images at all
        assert pw.get(torch.nn.Parameter(torch.randn(8, 4, 3, 3)), *geo) is None and not pw.entries and not calls
        with mock.patch.object(_lib, 'get_gemm_mode', lambda: 'f32'):
            assert pw.get(w, *geo) is None and not pw.entries
        # first use packs, the second is a hit on the same buffer
        b1 = pw.get(w, *geo)
        assert pw.get(w, *geo) is b1 and pw.stats == {'hits': 1, 'packs': 1, 'batched': 0} and len(calls) == 1
        assert pw.get(w, 'conv', 4, 8, 3, 1, 64) is not b1 and pw.stats['packs'] == 2      # the transposed image is another entry
        # an in-place edit under no_grad bumps the version: packed again (into the same buffer)
        with torch.no_grad():
            w.mul_(2)
        assert pw.get(w, *geo) is b1 and pw.stats['packs'] == 3 and pw.stats['hits'] == 1
        # moved storage, same version: packed again
        version = w._version
        w.data = w.data.clone()
        assert w._version == version
        pw.get(w, *geo)
        assert pw.stats['packs'] == 4 and calls[-1][1] == w.data_ptr()
        # repack(): live entries of unchanged version survive into the new epoch and are the rows of the batched call's table
        dcn = param(8, 8, 3, 3)
        assert pw.get(dcn, 'dcn', 8, 8, 3, 0, 64) is not None and pw.stats['packs'] == 5
        pw.get(w, 'conv', 4, 8, 3, 1, 64)               # (its version is stale since the mul_: packed again)
        assert pw.stats['packs'] == 6
        epoch, hits = pw.epoch, pw.stats['hits']
        pw.repack()
        assert pw.epoch == epoch + 1 and calls[-1][0] == 'batched' and calls[-1][2] == 3 and pw.stats['batched'] == 1
        tab, n = pw.table[torch.device('cpu')]
        assert n == 3 and tab.shape == (3, 6) and tab.dtype == torch.int64 and calls[-1][1] == tab.data_ptr()
        for row, e in zip(tab.tolist(), pw.entries.values()):   # PackDesc: two pointers, then eight 32-bit fields in pairs
            d = e.desc
            assert len(d) == 10 and row == [d[0], d[1]] + [d[2 + 2 * j] | (d[3 + 2 * j] << 32) for j in range(4)]
        assert tab[0, 0] == w.data_ptr() and tab[0, 1] == b1.data_ptr()
        npacks = pw.stats['packs']
        assert pw.get(w, *geo) is b1 and pw.get(dcn, 'dcn', 8, 8, 3, 0, 64) is not None
        assert pw.stats['hits'] == hits + 2 and pw.stats['packs'] == npacks
        pw.repack()                                     # nothing added or dropped: the table is kept
        assert pw.table[torch.device('cpu')][0] is tab and calls[-1] == ('batched', tab.data_ptr(), 3)
        # repack() drops the entries whose version changed or whose parameter died, and rebuilds the table
        with torch.no_grad():
            w.mul_(2)
        del dcn
        gc.collect()
        pw.repack()
        assert not pw.entries and pw.table is None and pw.stats['batched'] == 2    # (nothing left: no launch)
        other = param(8, 4, 3, 3)
        pw.get(w, *geo)
        pw.get(other, *geo)
        pw.repack()
        assert calls[-1][0] == 'batched' and calls[-1][2] == 2
        del other
        gc.collect()
        pw.repack()
        assert len(pw.entries) == 1 and calls[-1][0] == 'batched' and calls[-1][2] == 1 and pw.table[torch.device('cpu')][1] == 1
        # split(): the same persistent pair until the parent changes; images are keyed on the slices
        a, b = pw.split(w, 1)
        assert a.shape == (8, 1, 3, 3) and b.shape == (8, 3, 3, 3) and a.is_contiguous() and b.is_contiguous()
        a2, b2 = pw.split(w, 1)
        assert a2 is a and b2 is b and a._rvsr_parent() is w
        npacks = pw.stats['packs']
        ia = pw.get(a, 'conv', 1, 8, 3, 0, 64)
        assert ia is not None and ia is not b1 and pw.get(a, 'conv', 1, 8, 3, 0, 64) is ia and pw.stats['packs'] == npacks + 1
        assert calls[-1][:2] == ('conv', a.data_ptr())
        with torch.no_grad():
            w.add_(1)                                   # parent edited: same tensors, refreshed in place, their image packed again
        a3, b3 = pw.split(w, 1)
        assert a3 is a and b3 is b and torch.equal(a, w[:, :1]) and torch.equal(b, w[:, 1:])
        assert pw.get(a, 'conv', 1, 8, 3, 0, 64) is ia and pw.stats['packs'] == npacks + 2
        # repack() refreshes the pair in place from the parameter the optimizer rewrote behind the version counter
        w.data.mul_(3)
        assert not torch.equal(a, w[:, :1])
        pw.repack()
        assert torch.equal(a, w[:, :1]) and torch.equal(b, w[:, 1:])
        hits = pw.stats['hits']
        a4, _ = pw.split(w, 1)
        assert a4 is a and pw.get(a, 'conv', 1, 8, 3, 0, 64) is ia and pw.stats['hits'] == hits + 1
        with torch.no_grad():
            w.add_(1)
        pw.repack()                                     # a pair whose parent changed version is forgotten; split() starts afresh
        assert not pw.slices and pw.split(w, 1)[0] is not a
        # invalidate() forgets everything; a disabled cache returns None / fresh copies
        pw.get(w, *geo)
        epoch = pw.epoch
        pw.invalidate()
        assert not pw.entries and not pw.slices and pw.table is None and pw.epoch == epoch + 1
        pw.enabled = False
        assert pw.get(w, *geo) is None and not pw.entries
        f1, f2 = pw.split(w, 1), pw.split(w, 1)
        assert f1[0] is not f2[0] and torch.equal(f1[0], f2[0]) and not pw.slices


# ---- the conv plan (csrc/conv_plan.h) through its exported query: no GPU, made-up addresses
_A = 0x10000000   # 16-byte aligned; the plan dereferences nothing


def _conv_plan(C1=64, Co=64, H=45, W=80, *, B=2, C2=0, xact=False, in_mode=0, k=3, stride=1, w_mode=0, act=0, residual=False, Co2=0,
               x_off=0, out_off=0, Hout=None, Wout=None, gemm=None):
    """(rc, message, plan row) of rvsr_conv2d_forward_plan for a conv of (B, C1 [+ C2], H, W) stored input."""
    import ctypes
    from realvsr_amd import _lib
    L = _lib.lib()
    pad = k // 2
    if Hout is None:
        Hv, Wv = (H // 2, W // 2) if in_mode == 2 else (H, W)
        Hout, Wout = (Hv + 2 * pad - k) // stride + 1, (Wv + 2 * pad - k) // stride + 1
    p = lambda off, on=True: ctypes.c_void_p(_A + off) if on else None   # noqa: E731
    row = (ctypes.c_int * 14)(*([-7] * 14))
    L.rvsr_set_gemm_mode_thread(-1 if gemm is None else gemm)
    try:
        rc = L.rvsr_conv2d_forward_plan(p(0x100000 + x_off), C1, p(0x200000, C2), C2, p(0x300000, xact), 0.1, in_mode, H, W, p(0x400000),
                                        p(0x500000), p(0x600000, residual), p(0x700000 + out_off), Co, p(0x800000, Co2), Co2, B, k, stride,
                                        w_mode, act, 0.1, 0, Hout, Wout, row)
    finally:
        L.rvsr_set_gemm_mode_thread(-1)
    return rc, L.rvsr_last_error().decode(), dict(zip(('family', 'MT', 'vec', 'wide', 'NT', 'act_in', 'CC', 'vec4', 'th', 'tw', 'gx', 'gy',
                                                       'gz', 'lds'), row))


THIN, FWD5, FWD2, F32 = 0, 1, 2, 3
# Expected rows, worked out by hand from the dispatcher this plan replaced (the entry of conv_kernels.hip, rvsr_launch_conv_fwd2 and
# launch_fwd5 / launch_fwd2 of conv2_kernels.hip before the plan existed), B = 2, 64 -> 64 channels, 45 x 80 unless stated.
_PLAN_ROWS = [
    # 3x3 stride 1: conv_fwd5
    (dict(H=180, W=320), dict(family=FWD5, MT=2, vec=1, wide=1, NT=3, act_in=0, CC=1, vec4=1, th=8, tw=64, gx=230, gy=1, gz=1, lds=159248)),
    (dict(), dict(family=FWD5, MT=2, vec=1, wide=0, NT=3, act_in=0, CC=1, vec4=1, th=16, tw=32, gx=18, gy=1, gz=1, lds=153104)),
    (dict(W=30), dict(family=FWD5, MT=2, vec=0, wide=0, NT=3, vec4=0, th=16, tw=32, gx=6, lds=153104)),
    (dict(H=180, W=320, x_off=4, out_off=4), dict(family=FWD5, MT=2, vec=0, wide=0, NT=3, vec4=0, gx=240)),
    (dict(H=180, W=320, x_off=4), dict(family=FWD5, vec=0, wide=0, vec4=1)),
    (dict(H=180, W=320, out_off=4), dict(family=FWD5, vec=1, wide=0, vec4=0)),
    (dict(H=180, W=320, xact=True), dict(family=FWD5, MT=2, vec=1, wide=1, NT=3, act_in=1)),
    (dict(C1=64, H=90, W=160, in_mode=2), dict(family=FWD5, MT=2, vec=2, wide=0, NT=3, vec4=1, gx=18)),
    (dict(H=23, W=40, in_mode=1, Hout=45, Wout=80, w_mode=1), dict(family=FWD5, MT=2, vec=3, wide=0, NT=3, vec4=1, gx=18)),
    (dict(Co=3), dict(family=THIN, MT=1, NT=3, vec4=0, th=8, tw=128, gx=12, gy=1, gz=1, lds=52736)),
    (dict(Co=3, xact=True), dict(family=FWD5, MT=1, vec=1, act_in=1)),          # (the vector-ALU kernel has no act' load)
    (dict(Co=32), dict(family=FWD5, MT=1, vec=1, wide=0, NT=3, vec4=1, th=16, tw=32, gx=18, lds=115728)),
    (dict(Co=32, H=180, W=320), dict(family=FWD5, MT=1, vec=1, wide=0)),        # (the 8 x 64 tile: 64-row m-blocks only)
    (dict(C2=64), dict(family=FWD5, MT=2, vec=1, wide=0, NT=3)),
    (dict(C1=24, C2=16), dict(family=FWD5, MT=2, vec=0, wide=0, NT=3)),         # a second input behind 8 k channels: scalar staging
    (dict(C1=20, C2=16), dict(family=F32, MT=2, CC=16, th=8, tw=32, gx=18, gy=1, gz=2, lds=59200)),
    (dict(C2=64, Co=32, Co2=32), dict(family=FWD5, MT=2, vec=1, vec4=0, wide=0)),   # split output: element stores
    # 1x1, 3x3 stride 2, 5x5: conv_fwd2, or exact f32 where its chunked staging cannot split the concat
    (dict(k=1, C1=32, C2=32), dict(family=FWD2, MT=2, CC=2, NT=3, th=8, tw=32, gx=36, gy=1, gz=1, lds=41216)),
    (dict(k=1, C1=16, C2=16), dict(family=F32, MT=2, CC=32, gx=18, gy=1, gz=2, lds=41088)),
    (dict(k=3, C1=24, C2=16, stride=2), dict(family=F32, MT=2, CC=8)),
    (dict(stride=2), dict(family=FWD2, MT=2, CC=1, NT=3, act_in=0, vec4=1, gx=12, lds=107840)),
    (dict(stride=2, xact=True), dict(family=FWD2, act_in=1)),
    (dict(k=5), dict(family=FWD2, MT=1, CC=1, NT=3, gx=72, lds=78976)),
    (dict(k=5, stride=2), dict(family=FWD2, MT=1, CC=1, NT=3, gx=24, lds=132800)),
    (dict(k=5, H=23, W=40, in_mode=1, Hout=45, Wout=80, w_mode=1), dict(family=F32, MT=2, CC=8, gx=18, gy=1, gz=2, lds=65824)),
    (dict(k=5, Co=216), dict(family=FWD2, MT=1)),
    # GEMM mode 1: exact f32 everywhere but the vector-ALU kernel; modes 2 / 3: fewer terms in conv_fwd5 with 64-row m-blocks on a
    # vector-staged view, three terms everywhere else
    (dict(H=180, W=320, gemm=1), dict(family=F32, MT=2, CC=16, NT=3, gx=230, gy=1, gz=2, lds=59200)),
    (dict(Co=216, gemm=1), dict(family=F32, MT=4, CC=8, gy=2)),
    (dict(Co=3, gemm=1), dict(family=THIN)),
    (dict(H=180, W=320, gemm=2), dict(family=FWD5, MT=2, vec=1, wide=1, NT=2)),
    (dict(H=180, W=320, gemm=3), dict(family=FWD5, MT=2, vec=1, wide=1, NT=1)),
    (dict(gemm=2), dict(family=FWD5, MT=2, vec=1, wide=0, NT=2)),
    (dict(C1=64, H=90, W=160, in_mode=2, gemm=3), dict(family=FWD5, vec=2, NT=1)),
    (dict(H=23, W=40, in_mode=1, Hout=45, Wout=80, w_mode=1, gemm=2), dict(family=FWD5, vec=3, NT=2)),
    (dict(Co=32, gemm=2), dict(family=FWD5, MT=1, vec=1, NT=3)),
    (dict(W=30, gemm=3), dict(family=FWD5, MT=2, vec=0, NT=3)),
    (dict(stride=2, gemm=2), dict(family=FWD2, NT=3)),
    (dict(k=1, gemm=3), dict(family=FWD2, NT=3)),
    # the f16 + fp8 format and the mask epilogue where they exist
    (dict(H=180, W=320, w_mode=4), dict(family=FWD5, MT=2, vec=1, wide=1, NT=4, act_in=0, lds=159248)),
    (dict(w_mode=4, gemm=2), dict(family=FWD5, MT=2, vec=1, wide=0, NT=4)),
    (dict(w_mode=6, C2=64), dict(family=FWD5, vec=1, NT=4)),
    (dict(H=8, W=64, act=3, residual=True, w_mode=1), dict(family=FWD5, MT=2, vec=1, wide=1, NT=3, th=8, tw=64, gx=2)),
    (dict(H=8, W=64, act=3, residual=True, w_mode=1, xact=True, gemm=3), dict(family=FWD5, wide=1, NT=1, act_in=1)),
]
_FMT = 'f16 + fp8'
_REFUSALS = [   # (call, the message names this)
    (dict(w_mode=4, Co=32), _FMT), (dict(w_mode=4, xact=True), _FMT), (dict(w_mode=4, W=30), _FMT), (dict(w_mode=4, gemm=1), _FMT),
    (dict(w_mode=5), _FMT), (dict(w_mode=4, stride=2), _FMT), (dict(w_mode=4, k=1), _FMT), (dict(w_mode=4, Co=3), _FMT),
    (dict(w_mode=4, C1=24, C2=16), _FMT), (dict(w_mode=4, x_off=4), _FMT), (dict(w_mode=4, Co=32, act=3, residual=True), _FMT),
    (dict(act=3, residual=True, H=16, W=24), ''), (dict(act=3, residual=True, H=8, W=64, Co=32), ''),
    (dict(act=3, residual=True, H=8, W=64, gemm=1), ''), (dict(act=3, H=8, W=64), ''), (dict(act=3, residual=True, H=8, W=64, out_off=4), ''),
    (dict(act=3, residual=True, H=8, W=62), ''), (dict(act=3, residual=True, H=16, W=128, stride=2), ''),
]


def test_conv_forward_plan_rows():
    """Which kernel, tile and grid a rvsr_conv2d_forward call gets: one row per family and per coordinate that can differ."""
    for call, want in _PLAN_ROWS:
        rc, _, row = _conv_plan(**call)
        assert rc == 0, call
        got = {key: row[key] for key in want}
        assert got == want, (call, row)
    # after a per-thread mode the thread is back on the process-wide one
    assert _conv_plan(H=180, W=320)[2]['NT'] == 3


def test_conv_forward_plan_refusals():
    """A refusal is RVSR_ERR_UNSUPPORTED with a message that names the format, or -- act 3, where the caller has a plan B -- with none;
    bad arguments keep their own code."""
    assert _conv_plan()[0] == 0
    for call, text in _REFUSALS:
        rc, msg, row = _conv_plan(**call)
        assert rc == 1 and row['family'] == -1, (call, rc, row)
        assert (text in msg) if text else msg == '', (call, msg)
    rc, msg, row = _conv_plan(Hout=44, Wout=80)
    assert rc == 2 and 'output size' in msg and row['family'] == -7      # (a call that is not valid has no plan: the row is untouched)


def test_grad_mask_fusable_asks_the_plan():
    from realvsr_amd import functional as RF
    for hw in ((180, 320), (720, 1280), (8, 64)):
        assert RF.grad_mask_fusable(*hw) is True, hw
    for hw in ((45, 80), (90, 160), (16, 24), (64, 96), (8, 62)):
        assert RF.grad_mask_fusable(*hw) is False, hw
    old = RF._FUSE_GRAD_MASK
    try:
        RF._FUSE_GRAD_MASK = False
        assert RF.grad_mask_fusable(180, 320) is False
    finally:
        RF._FUSE_GRAD_MASK = old


def test_conv_workspace_bytes_pinned():
    """rvsr_conv2d_forward_workspace_bytes / rvsr_conv2d_wgrad_workspace_bytes: values of the library before the weight-gradient plan
    (the query takes the largest slicing among the families that can take the geometry)."""
    from realvsr_amd import _lib
    L = _lib.lib()
    pins = {   # (C1, C2, Co, B, ksize, stride, Hout, Wout): (forward bytes, weight-gradient bytes)
        (64, 0, 64, 40, 3, 1, 180, 320): (147456, 37814272),
        (64, 0, 3, 8, 3, 1, 180, 320): (73728, 5317632),
        (64, 64, 64, 8, 3, 1, 45, 80): (294912, 37781504),
        (64, 0, 64, 8, 3, 2, 45, 80): (147456, 75628544),
        (3, 0, 64, 8, 5, 2, 45, 80): (102400, 4980736),
        (320, 0, 64, 8, 1, 1, 45, 80): (81920, 16763904),
        (16, 0, 33, 1, 5, 1, 7, 9): (102400, 105864),
        (128, 0, 216, 1, 3, 2, 16, 24): (1179648, 31878144),
        (64, 0, 4, 1, 3, 1, 7, 9): (73728, 18464),
    }
    for (C1, C2, Co, B, k, s, H, W), want in pins.items():
        got = (L.rvsr_conv2d_forward_workspace_bytes(C1, C2, Co, k), L.rvsr_conv2d_wgrad_workspace_bytes(C1, C2, Co, B, k, s, H, W))
        assert got == want, (C1, C2, Co, B, k, s, H, W, got)


# ---- the DCN plan (csrc/dcn_plan.h) through its exported queries: no GPU, made-up addresses
_FWD_KEYS = ('family', 'MT', 'CHS', 'NT', 'pack', 'probe', 'nprobe', 'ncand') + tuple(
    '%s%d' % (k, i) for i in range(3) for k in ('halo', 'ge', 'lt', 'ge2', 'thr_ge', 'thr_lt', 'thr_ge2', 'lds')) + ('gx', 'gy', 'gz', 'lds')
_BWD_KEYS = ('in_family', 'NK', 'in_NT', 'CHS', 'in_lds', 'own_probe', 'ncand') + tuple(
    '%s%d' % (k, i) for i in range(5) for k in ('win', 'ge', 'lt', 'thr')) + ('handoff', 'handoff_off', 'w_family', 'R', 'TH', 'w_NT', 'ns', 'nmb',
                                                                             'xcd', 'P', 'Q', 'gy', 'gz', 'w_lds')
DCN_FWD3, DCN_FWD2, DCN_FWD1 = 0, 1, 2
BWDIN6, BWDIN1, BWDW6, BWDW4, BWDW2, BWDW1 = 1, 2, 1, 2, 3, 4


def _dcn_fwd_plan(C=64, Co=64, H=45, W=80, *, B=2, dg=8, stride=1, pad=1, dil=1, probe=False, hint=0, prepacked=False, ws=0, x_off=0, gemm=None):
    """(rc, message, plan row) of rvsr_dcn_pack_forward_plan; ws: workspace bytes relative to the query's (None: no workspace)."""
    import ctypes
    from realvsr_amd import _lib
    L = _lib.lib()
    p = lambda off, on=True: ctypes.c_void_p(_A + off) if on else None   # noqa: E731
    row = (ctypes.c_longlong * 36)(*([-7] * 36))
    need = L.rvsr_modulated_deform_conv_forward_workspace_bytes(C, Co)
    L.rvsr_set_gemm_mode_thread(-1 if gemm is None else gemm)
    try:
        rc = L.rvsr_dcn_pack_forward_plan(p(0x100000 + x_off), p(0x200000), p(0x300000), p(0x400000), p(0x500000), B, C, H, W, Co, stride, pad, dil,
                                          dg, 2 | (0x100 if prepacked else 0) | (hint << 10), 0.1, p(0x600000, probe), p(0x700000, ws is not None),
                                          0 if ws is None else need + ws, row)
    finally:
        L.rvsr_set_gemm_mode_thread(-1)
    return rc, L.rvsr_last_error().decode(), dict(zip(_FWD_KEYS, row))


def _dcn_bwd_plan(C=64, Co=64, H=45, W=80, *, B=2, dg=8, stride=1, pad=1, dil=1, probe=False, gx=True, gom=True, gw=True, ws=0, g_off=0, gemm=None):
    import ctypes
    from realvsr_amd import _lib
    L = _lib.lib()
    p = lambda off, on=True: ctypes.c_void_p(_A + off) if on else None   # noqa: E731
    row = (ctypes.c_longlong * 41)(*([-7] * 41))
    need = L.rvsr_modulated_deform_conv_backward_workspace_bytes(B, C, H, W, Co, stride, pad, dil)
    L.rvsr_set_gemm_mode_thread(-1 if gemm is None else gemm)
    try:
        rc = L.rvsr_dcn_pack_backward_plan(p(0x100000), p(0x200000), p(0x400000), p(0x500000 + g_off), None, 0.1, p(0x800000, gx), p(0x900000, gw),
                                           p(0xa00000, gw), p(0xb00000, gom), B, C, H, W, Co, stride, pad, dil, dg, p(0x600000, probe),
                                           p(0x40000000, ws is not None), 0 if ws is None else need + ws, row)
    finally:
        L.rvsr_set_gemm_mode_thread(-1)
    return rc, L.rvsr_last_error().decode(), dict(zip(_BWD_KEYS, row))


# Expected rows, worked out by hand from the dispatcher these plans replaced (dcn_forward_impl / dcn_backward_impl of dcn_kernels.hip,
# rvsr_launch_dcn_fwd2 / rvsr_launch_dcn_bwdw2, rvsr_launch_dcn_fwd3, rvsr_launch_dcn_bwdin6 / rvsr_launch_dcn_bwdw6 before the plan
# existed); B = 2, 64 -> 64 channels, 8 deformable groups, 45 x 80, pad 1 unless stated.  Counters: 2 * 144 planes * 3 rows * 80 = 69120
# samples; 8 % + 1 = 5530, 1 % + 1 = 692, 2 % + 1 = 1383.
_NOSEL = dict(ge0=-1, lt0=-1, ge20=-1)
_DCN_FWD_ROWS = [
    (dict(), dict(family=DCN_FWD3, MT=2, NT=3, pack=1, probe=0, nprobe=0, ncand=1, halo0=3, gx=18, gy=1, gz=2, lds=78080, **_NOSEL)),
    (dict(hint=7), dict(family=DCN_FWD3, MT=2, ncand=1, halo0=7, lds=110848, **_NOSEL)),
    (dict(hint=11), dict(family=DCN_FWD3, MT=2, ncand=1, halo0=11, lds=151808, **_NOSEL)),
    (dict(Co=128, hint=11), dict(family=DCN_FWD3, MT=4, ncand=1, halo0=7, gy=1, lds=147968, **_NOSEL)),
    (dict(hint=11, x_off=4), dict(family=DCN_FWD3, ncand=1, halo0=3)),           # (the 7 / 11 px tiles stage 16-byte vectors)
    (dict(probe=True), dict(family=DCN_FWD3, MT=2, probe=1, nprobe=69120, ncand=3,
                            halo0=3, ge0=-1, lt0=1, ge20=-1, thr_lt0=5530, lds0=78080,
                            halo1=7, ge1=1, lt1=3, ge21=-1, thr_ge1=5530, thr_lt1=692, lds1=110848,
                            halo2=11, ge2=3, lt2=-1, ge22=1, thr_ge2=692, thr_ge22=5530, lds2=151808)),
    (dict(Co=128, probe=True), dict(family=DCN_FWD3, MT=4, probe=1, ncand=2, halo0=3, ge0=-1, lt0=1, thr_lt0=5530,
                                    halo1=7, ge1=1, lt1=-1, ge21=-1, thr_ge1=5530, halo2=0)),
    (dict(W=30, probe=True), dict(family=DCN_FWD3, probe=1, nprobe=25920, ncand=1, halo0=3, gx=6, **_NOSEL)),
    (dict(stride=2, probe=True), dict(family=DCN_FWD2, MT=2, NT=3, pack=1, probe=0, gx=6, gy=1, gz=2, lds=78080)),
    (dict(dil=2, probe=True), dict(family=DCN_FWD2, MT=2, probe=0, gx=18, lds=78080)),
    (dict(C=32, probe=True), dict(family=DCN_FWD1, MT=2, CHS=0, NT=3, pack=0, probe=0, gx=36, gy=1, gz=2, lds=55584)),
    (dict(gemm=1, probe=True), dict(family=DCN_FWD1, MT=2, CHS=8, pack=0, probe=0, gx=36, lds=55584)),
    (dict(gemm=2), dict(family=DCN_FWD3, MT=2, NT=2)), (dict(gemm=3), dict(family=DCN_FWD3, MT=2, NT=1)),
    (dict(Co=128, gemm=2), dict(family=DCN_FWD3, MT=4, NT=2)), (dict(Co=128, gemm=3), dict(family=DCN_FWD3, MT=4, NT=1)),
    (dict(Co=32, gemm=2), dict(family=DCN_FWD3, MT=1, NT=3)), (dict(Co=32, gemm=3), dict(family=DCN_FWD3, MT=1, NT=3)),
    (dict(stride=2, gemm=3), dict(family=DCN_FWD2, NT=3)),
    (dict(ws=None, probe=True), dict(family=DCN_FWD1, MT=2, CHS=8, pack=0, probe=0)),
    (dict(prepacked=True), dict(family=DCN_FWD3, pack=0)),
    (dict(Co=130), dict(family=DCN_FWD3, MT=4, gy=2)),
]
_WINDOWS5 = dict(ncand=5, win0=2, ge0=-1, lt0=0, win1=4, ge1=0, lt1=1, win2=5, ge2=1, lt2=2, win3=8, ge3=2, lt3=4, win4=12, ge4=4, lt4=-1,
                 thr0=1383, thr1=1383, thr2=1383, thr3=1383)
_DCN_BWD_ROWS = [
    (dict(), dict(in_family=BWDIN6, NK=4, in_NT=3, own_probe=1, handoff=1, handoff_off=37814272, w_family=BWDW6, R=4, TH=8, w_NT=3, ns=32, nmb=1,
                  xcd=1, P=32, Q=32, gy=8, w_lds=157216, **_WINDOWS5)),
    (dict(probe=True), dict(in_family=BWDIN6, own_probe=0, w_family=BWDW6, **_WINDOWS5)),
    (dict(Co=128), dict(in_family=BWDIN6, NK=8, ncand=4, win0=2, ge0=-1, lt0=0, win1=4, ge1=0, lt1=1, win2=5, ge2=1, lt2=2, win3=8, ge3=2, lt3=-1,
                        win4=0, handoff=1, w_family=BWDW6, ns=16, nmb=2, xcd=1, Q=16, gy=16)),
    (dict(gemm=2), dict(in_family=BWDIN6, in_NT=2, w_family=BWDW6, w_NT=2)), (dict(Co=32, gemm=3), dict(in_family=BWDIN6, NK=2, in_NT=3, w_NT=1)),
    (dict(gx=False, gom=False), dict(in_family=0, handoff=0, w_family=BWDW4, w_NT=3, P=32, Q=256, gy=1, gz=8, w_lds=102400)),
    (dict(gx=False, gom=False, gemm=3), dict(w_family=BWDW4, w_NT=1)),
    (dict(gx=False, gom=False, W=30), dict(w_family=BWDW2, P=24, Q=192, gy=1, gz=8, w_lds=98304)),
    (dict(gx=False, gom=False, g_off=4), dict(w_family=BWDW2, P=32, Q=256)),
    (dict(gx=False, gom=False, stride=2), dict(w_family=BWDW2)),
    (dict(gw=False, ws=None), dict(in_family=BWDIN1, CHS=8, in_lds=106880, w_family=0)),       # (dcn_bwdin6 has no workspace)
    (dict(gw=False), dict(in_family=BWDIN6, handoff=0, w_family=0)),
    (dict(C=32), dict(in_family=BWDIN1, CHS=0, in_lds=106880, handoff=0, w_family=BWDW1, P=64, Q=256, gy=1, gz=4, w_lds=82944)),
    (dict(gemm=1), dict(in_family=BWDIN1, CHS=8, in_lds=106880, handoff=0, w_family=BWDW2, P=32, Q=256)),
    (dict(Co=130), dict(in_family=BWDIN1, CHS=8, in_lds=159680, handoff=0, w_family=BWDW4, P=10, Q=80, gy=3, gz=8)),
    (dict(C=2056, dg=257), dict(in_family=BWDIN6, NK=4, handoff=0, w_family=BWDW4, P=1, Q=8, gy=1, gz=257)),
    (dict(stride=2), dict(in_family=BWDIN1, CHS=8, handoff=0, w_family=BWDW2)),
]


def test_dcn_forward_plan_rows():
    """Which kernels a rvsr_dcn_pack_forward call launches: one row per family and per coordinate that can differ."""
    for call, want in _DCN_FWD_ROWS:
        rc, _, row = _dcn_fwd_plan(**call)
        assert rc == 0, call
        assert {key: row[key] for key in want} == want, (call, row)
    # a workspace one byte short, where a bf16 kernel would take the call: refused, and nothing is launched -- no probe pass, no pack
    rc, msg, row = _dcn_fwd_plan(ws=-1, probe=True)
    assert rc == 4 and msg == 'dcn forward: workspace 147455 B < 147456 B', (rc, msg)
    assert (row['family'], row['probe'], row['pack'], row['ncand']) == (-1, 0, 0, 0), row
    assert _dcn_fwd_plan(C=32, ws=-1)[0] == 0                                # (the first-generation kernel reads no weight image)
    rc, msg, row = _dcn_fwd_plan(C=24)
    assert rc == 1 and 'multiple of 8' in msg and row['family'] == -7        # (a call that is not valid has no plan: the row is untouched)


def test_dcn_backward_plan_rows():
    """Which kernels a rvsr_dcn_pack_backward call launches, and the refusals with their texts."""
    for call, want in _DCN_BWD_ROWS:
        rc, _, row = _dcn_bwd_plan(**call)
        assert rc == 0, call
        assert {key: row[key] for key in want} == want, (call, row)
    rc, msg, row = _dcn_bwd_plan(Co=136)
    assert rc == 1 and msg == 'dcn backward: channels_out 136 needs 164480 B of LDS' and row['in_family'] == -1, (rc, msg)
    rc, msg, _ = _dcn_bwd_plan(gom=False)
    assert rc == 2 and msg == 'dcn backward: grad_input/grad_offset/grad_mask must be given together', (rc, msg)
    rc, msg, row = _dcn_bwd_plan(ws=-1)
    assert rc == 4 and msg == 'dcn backward: workspace 40173567 B < 40173568 B' and row['w_family'] == -1, (rc, msg)
    assert _dcn_bwd_plan(ws=None)[0] == 4 and _dcn_bwd_plan(gw=False, ws=-1)[0] == 0


def test_dcn_workspace_bytes_pinned():
    """The three DCN workspace queries: values of the library before dcn_bwd_workspace (dcn_plan.h) gave the layout once."""
    from realvsr_amd import _lib
    L = _lib.lib()
    pins = {   # (B, C, H, W, Co, stride, pad, dil, dg of the DCNv1 query): (forward, backward, DCNv1 bytes)
        (40, 64, 180, 320, 64, 1, 1, 1, 8): (147456, 640745472, 1967849472),
        (8, 64, 45, 80, 128, 1, 1, 1, 8): (294912, 56688640, 73277440),
        (1, 2056, 45, 80, 64, 1, 1, 1, 8): (4755456, 37898240, 39971840),    # 257 units: no hand-off
        (8, 64, 45, 80, 64, 2, 1, 1, 8): (147456, 37814272, 42053632),
        (1, 16, 7, 9, 33, 1, 1, 1, 1): (36864, 4965632, 4970240),
        (2, 32, 9, 33, 72, 1, 2, 2, 1): (147456, 7990272, 8033280),
        (2, 128, 45, 80, 128, 1, 1, 1, 8): (589824, 42500096, 46647296),
        (1, 16, 8, 32, 16, 1, 1, 1, 1): (18432, 2441472, 2459904),
    }
    for (B, C, H, W, Co, s, p, d, dg), want in pins.items():
        got = (L.rvsr_modulated_deform_conv_forward_workspace_bytes(C, Co), L.rvsr_modulated_deform_conv_backward_workspace_bytes(B, C, H, W, Co, s, p, d),
               L.rvsr_deform_conv_workspace_bytes(B, C, H, W, Co, 3, 3, s, p, d, dg))
        assert got == want, (B, C, H, W, Co, s, p, d, got)


def test_dcn_forward_halo_is_the_device_rule(monkeypatch):
    """rvsr_dcn_forward_halo (the host's choice from copied counters) against the thresholds the forward plan hands to the device, at,
    just below and just above both ties (100 c1 == 8 n, 100 c3 == n): equal everywhere; DcnOffsetStats.forward_halo returns it."""
    import ctypes
    import types
    from realvsr_amd import _lib, caches
    L = _lib.lib()

    class HostSlot:   # a ring slot without pinned memory and a GPU event: record() and forward_halo() run as they do on the GPU
        def __init__(self):
            self.counters, self.nsamples, self.tick = torch.zeros(8, dtype=torch.int32), 0, -1
            self.event = types.SimpleNamespace(record=lambda: None, synchronize=lambda: None)
    monkeypatch.setattr(caches, '_Slot', HostSlot)
    n = L.rvsr_dcn_probe_samples(1, 8, 16, 100)
    assert n == 8 * 18 * 100 == 14400 and L.rvsr_dcn_probe_samples(2, 8, 45, 80) == 69120
    for Co in (64, 128):
        rc, _, row = _dcn_fwd_plan(Co=Co, H=16, W=100, B=1, probe=True)
        assert rc == 0 and row['nprobe'] == n and row['ncand'] == (3 if Co == 64 else 2)
        assert (row['thr_lt0'], row['thr_ge1']) == (1153, 1153) and (Co == 128 or (row['thr_lt1'], row['thr_ge2'], row['thr_ge22']) == (145, 145, 1153))
        for c1 in (1151, 1152, 1153):
            for c3 in (143, 144, 145):
                cnt = (ctypes.c_uint * 8)(c1 + 7, c1, c3 + 5, c3, c3, 0, 0, 0)
                runs = [row['halo%d' % k] for k in range(row['ncand'])   # dcn_halo_not_selected with the plan's candidates
                        if not any(row['%s%d' % (key, k)] >= 0 and cmp(cnt[row['%s%d' % (key, k)]], row['thr_%s%d' % (key, k)])
                                   for key, cmp in (('ge', int.__lt__), ('ge2', int.__lt__), ('lt', int.__ge__)))]
                want = 3 if c1 <= 1152 else (7 if c3 <= 144 or Co == 128 else 11)   # ties go the device's way: 100 c <= 8 n, 100 c <= n
                assert runs == [want], (Co, c1, c3, runs)
                assert L.rvsr_dcn_forward_halo(ctypes.cast(cnt, ctypes.c_void_p), n, Co) == want, (Co, c1, c3)
                stats, w = caches.DcnOffsetStats(), torch.zeros(1)
                stats.record(w, torch.tensor(list(cnt), dtype=torch.int32), n)
                assert stats.forward_halo(w, Co) == want
    assert L.rvsr_dcn_forward_halo(ctypes.cast((ctypes.c_uint * 8)(), ctypes.c_void_p), 0, 64) == 0


def test_dcn_fused_ok_asks_the_library():
    from realvsr_amd import functional as RF
    x, w = torch.zeros(1, 16, 8, 32), torch.zeros(16, 16, 3, 3)
    assert RF._dcn_fused_ok(x, w, 1, 1, 1, 1, 2) and RF._dcn_fused_ok(x, w, (2, 2), 1, 1, 1, 4) and RF._dcn_fused_ok(x, w, 1, 1, 1, 1, 16)
    assert not RF._dcn_fused_ok(x.double(), w.double(), 1, 1, 1, 1, 2) and not RF._dcn_fused_ok(x, w, (1, 2), 1, 1, 1, 2)
    assert not RF._dcn_fused_ok(x, w, 1, 1, 1, 2, 2) and not RF._dcn_fused_ok(x, w, 1, 1, 1, 1, 3) and not RF._dcn_fused_ok(x, w, 1, 1, 1, 1, 0)
    assert not RF._dcn_fused_ok(x, torch.zeros(16, 16, 5, 5), 1, 2, 1, 1, 2)
    assert not RF._dcn_fused_ok(torch.zeros(1, 24, 8, 32), torch.zeros(16, 24, 3, 3), 1, 1, 1, 1, 2)      # 12 channels per deformable group
