"""rvsr_assemble_clips (csrc/batch_kernels.hip) and its callers against the numpy restatement tests/batch_reference.py, on the GPU.

Every comparison is torch.equal: without the colour conversion the path is one correctly rounded division and a permutation, with it an
exact-integer rule (include/realvsr_hip.h section 12).  Sources are carved out of larger uint8 buffers at every byte offset mod 4 and
destinations out of NaN-filled buffers whose margins have to stay NaN.  tests/test_data_host.py holds batch_reference itself against
the recorded output of the reference's dataset classes.
"""
import json

import numpy as np
import pytest
import torch

import batch_reference as ref
from conftest import load_golden
from gpu_util import dev

pytestmark = pytest.mark.gpu

PAD = 8   # floats of NaN margin on either side of a destination (32 bytes: the destination stays 16-byte aligned)


def run(u8, flags=None, mode=ref.REVERSE, offset=0, dst_shift=0):
    """assemble_batch on a source that starts `offset` bytes past a 16-byte boundary inside a larger buffer of 0xAB bytes, into a
    destination that starts PAD + dst_shift floats into a NaN-filled buffer; checks both margins; returns (out on the CPU, variant)."""
    from realvsr_amd import data
    d = dev()
    u8 = np.ascontiguousarray(u8)
    n = u8.size
    buf = torch.full((n + 64,), 0xAB, dtype=torch.uint8, device=d)
    assert buf.data_ptr() % 16 == 0
    start = 16 + offset
    buf[start:start + n] = torch.from_numpy(u8.reshape(-1)).to(d)
    src = buf[start:start + n].view(u8.shape)
    B, F, Hs, Ws, C = u8.shape
    total = B * F * C * Hs * Ws
    big = torch.full((total + 2 * PAD + dst_shift,), float('nan'), dtype=torch.float32, device=d)
    out = big[PAD + dst_shift:PAD + dst_shift + total].view(B, F, C, Hs, Ws)
    fl = None if flags is None else torch.as_tensor(np.asarray(flags), dtype=torch.int32).to(d)
    variant, blocks = data.assemble_plan(out, B, F, C, Hs, Ws)
    assert blocks == B * F * ((Hs + 63) // 64) * ((Ws + 63) // 64)
    got = data.assemble_batch(src, fl, mode, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert torch.isnan(big[:PAD + dst_shift]).all() and torch.isnan(big[PAD + dst_shift + total:]).all(), 'a store left the destination'
    assert (buf[:start] == 0xAB).all() and (buf[start + n:] == 0xAB).all()
    return out.cpu(), variant


def expect(u8, flags=None, mode=ref.REVERSE):
    return torch.from_numpy(ref.assemble(u8, flags, mode))


def rand_u8(seed, *shape):
    return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)


SIZES = (1, 2, 3, 5, 7, 8, 31, 32, 33, 63, 64, 65, 67)


@pytest.mark.parametrize('S', SIZES)
def test_sizes_flags_and_offsets(S):
    """Every size around the 64-pixel tile and the 4-pixel store, B = 9 with all flag values mixed in one launch, at every source byte
    offset mod 4; sizes that are multiples of 4 take the vector stores, the others the scalar ones."""
    u8 = rand_u8(S, 9, 3, S, S, 3)
    flags = [0, 1, 2, 3, 4, 5, 6, 7, 5]
    want = expect(u8, flags)
    for offset in range(4):
        got, variant = run(u8, flags, offset=offset)
        assert variant == (1 if S % 4 == 0 else 0)
        assert torch.equal(got, want), 'S %d offset %d' % (S, offset)


@pytest.mark.parametrize('flag', range(8))
def test_each_flag_alone(flag):
    for S, C in ((67, 3), (64, 3), (33, 1)):
        u8 = rand_u8(10 * flag + C, 2, 1, S, S, C)
        got, _ = run(u8, [flag, flag], offset=1)
        assert torch.equal(got, expect(u8, [flag, flag])), (S, C)


@pytest.mark.parametrize('B', [8, 9])
@pytest.mark.parametrize('F', [1, 3, 5])
@pytest.mark.parametrize('C', [1, 3])
def test_batch_frames_channels_modes(B, F, C):
    u8 = rand_u8(B * 100 + F * 10 + C, B, F, 20, 20, C)
    flags = [(3 * i + 1) % 8 for i in range(B)]
    for mode in ((0, 1, 2, 3) if C == 3 else (0, 1)):
        got, variant = run(u8, flags, mode, offset=(B + F + mode) % 4)
        assert variant == 1
        assert torch.equal(got, expect(u8, flags, mode)), mode


def test_crop_of_192():
    u8 = rand_u8(192, 2, 3, 192, 192, 3)
    for flags in ([6, 1], None):
        got, variant = run(u8, flags, offset=3)
        assert variant == 1 and torch.equal(got, expect(u8, flags))


@pytest.mark.parametrize('shape', [(1, 1), (1, 7), (7, 1), (5, 9), (33, 67), (64, 130)])
def test_whole_frames_without_flags(shape):
    Hs, Ws = shape
    for C in (1, 3):
        u8 = rand_u8(Hs * 1000 + Ws + C, 2, 2, Hs, Ws, C)
        for offset in range(4):
            got, _ = run(u8, None, ref.REVERSE, offset=offset)
            assert torch.equal(got, expect(u8, None)), (C, offset)


def test_every_plan_variant_is_reached():
    """Two variants: 16-byte stores (rows of a multiple of 4 pixels in a 16-byte aligned destination) and scalar stores -- reached by an
    odd width and, at a width of 64, by a destination that is only 4-byte aligned."""
    seen = {}
    u8 = rand_u8(5, 1, 2, 64, 64, 3)
    for name, kw in (('vector', {}), ('misaligned dst', {'dst_shift': 1})):
        got, seen[name] = run(u8, [4], **kw)
        assert torch.equal(got, expect(u8, [4]))
    u8 = rand_u8(6, 1, 2, 66, 66, 3)
    got, seen['odd width'] = run(u8, [7])
    assert torch.equal(got, expect(u8, [7]))
    assert seen == {'vector': 1, 'misaligned dst': 0, 'odd width': 0}


def test_all_256_values_equal_numpys_division():
    x = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(x.astype(np.float32) / 255.)
    for C, mode in ((1, 0), (1, 1)):
        got, _ = run(x.reshape(1, 1, 16, 16, 1), None, mode)
        assert torch.equal(got.reshape(-1), want)
    got, _ = run(np.repeat(x, 3).reshape(1, 1, 16, 16, 3), None, ref.REVERSE, offset=1)
    assert torch.equal(got, want.reshape(1, 1, 1, 16, 16).expand(1, 1, 3, 16, 16))


def test_conversion_on_all_triples_in_both_byte_orders():
    """Contract 2: for all 2^24 (R, G, B) the device gives the exact-integer half-even rule, with ==; numpy's float64 bgr2ycbcr agrees
    with the device on every channel value that is not a mathematical tie (206 values, counted from the integer criterion)."""
    from realvsr_amd import data
    d = dev()
    table = torch.from_numpy(np.arange(256, dtype=np.uint8).astype(np.float32) / 255.).to(d)
    n_ties = 0
    for r0 in range(0, 4096, 1024):
        rgb = ref.all_triples(slice(r0, r0 + 1024))
        exact = torch.from_numpy(ref.ycbcr_int(rgb)).to(d).permute(2, 0, 1).long()
        want = table[exact]
        tie = torch.from_numpy(ref.ycbcr_ties(rgb)).to(d).permute(2, 0, 1)
        n_ties += int(tie.sum())
        bgr = np.ascontiguousarray(rgb[..., ::-1])
        numpy_answer = table[torch.from_numpy(ref.ycbcr_numpy(bgr)).to(d).permute(2, 0, 1).long()]
        for src, mode in ((rgb, ref.TO_YCBCR), (bgr, ref.TO_YCBCR | ref.REVERSE)):
            got = data.assemble_batch(torch.from_numpy(src).to(d).view(1, 1, 1024, 4096, 3), None, mode)[0, 0]
            assert torch.equal(got, want), 'rows %d.., mode %d' % (r0, mode)
            assert bool(((got == numpy_answer) | tie).all())
    assert n_ties == 206


@pytest.fixture(scope='module')
def fixture():
    g = load_golden('batch')
    return g, json.loads(str(g['meta']))


def test_recorded_samples_through_the_pinned_stager(fixture):
    """The samples the reference's own dataset classes returned: draw_sample -> ClipBatchStager(pin=True) -> upload() -> kernel, batched
    per (class, size, window) so that a launch mixes flags; both slots of the stager are used."""
    from realvsr_amd import data
    g, meta = fixture
    groups = {}
    for k, m in enumerate(meta['samples']):
        groups.setdefault((m['cls'], m['opt']['GT_size'], m['opt']['N_frames']), []).append(k)
    assert len(groups) == 8
    for (cls, S, N), ks in sorted(groups.items()):
        n_gt = N if cls == 'RealVSRAllPairDataset' else 1
        st = data.ClipBatchStager(len(ks), N, n_gt, S, 3, pin=True, slots=2)
        for rounds in range(2):   # (the second round stages the same batch into the other slot)
            for i, k in enumerate(ks):
                plan, gt_paths, lq_paths, _ = ref.fixture_sample(data.draw_sample, meta, meta['samples'][k])
                st.stage(i, [ref.frame_of_path(p) for p in lq_paths], [ref.frame_of_path(p) for p in gt_paths], plan)
            lq, gt, flags = st.upload()
            assert lq.is_cuda and lq.dtype == torch.uint8 and flags.dtype == torch.int32
            var_L = data.assemble_batch(lq, flags).cpu()
            var_H = data.assemble_batch(gt, flags).cpu()
            for i, k in enumerate(ks):
                assert torch.equal(var_L[i], torch.from_numpy(g['s%d.LQs' % k])), 'sample %d: LQs' % k
                want = torch.from_numpy(g['s%d.GT' % k])
                assert torch.equal(var_H[i] if n_gt == N else var_H[i, 0], want), 'sample %d: GT' % k


def test_refusals():
    from realvsr_amd import data
    d = dev()
    ok = torch.zeros(2, 1, 8, 8, 3, dtype=torch.uint8, device=d)
    flags = torch.zeros(2, dtype=torch.int32, device=d)
    assert tuple(data.assemble_batch(ok, flags).shape) == (2, 1, 3, 8, 8)
    with pytest.raises(RuntimeError):
        data.assemble_batch(ok.cpu(), None)
    with pytest.raises(RuntimeError, match='contiguous'):
        data.assemble_batch(torch.zeros(2, 1, 8, 8, 6, dtype=torch.uint8, device=d)[..., ::2], None)
    with pytest.raises(RuntimeError):
        data.assemble_batch(ok.float(), None)
    with pytest.raises(RuntimeError, match='channels'):
        data.assemble_batch(torch.zeros(2, 1, 8, 8, 2, dtype=torch.uint8, device=d), None)
    with pytest.raises(RuntimeError, match='square'):
        data.assemble_batch(torch.zeros(2, 1, 8, 12, 3, dtype=torch.uint8, device=d), flags)
    with pytest.raises(RuntimeError, match='YCbCr'):
        data.assemble_batch(torch.zeros(2, 1, 8, 8, 1, dtype=torch.uint8, device=d), None, ref.TO_YCBCR)
    with pytest.raises(RuntimeError):
        data.assemble_batch(ok, flags.long())
    with pytest.raises(RuntimeError):
        data.assemble_batch(ok, None, out=torch.zeros(2, 1, 3, 8, 9, device=d))


def test_clip_from_u8_is_read_img_seq():
    from realvsr_amd import infer
    frames = rand_u8(77, 3, 20, 36, 3)
    got = infer.clip_from_u8(torch.from_numpy(frames).to(dev()))
    assert tuple(got.shape) == (3, 3, 20, 36)
    assert torch.equal(got.cpu(), torch.from_numpy(ref.read_img_seq(list(frames))))


# ---------------------------------------------------------------------------------------------------------------- model level
def _packed_and_f32(n_gt, seed):
    """The same batch as the packed uint8 feed and as the f32 tensors the reference's datasets would hand over."""
    B, N, S = 2, 3, 16
    lq, gt = rand_u8(seed, B, N, S, S, 3), rand_u8(seed + 1, B, n_gt, S, S, 3)
    flags = [6, 1]
    packed = {'LQs': torch.from_numpy(lq), 'GT': torch.from_numpy(gt), 'flags': torch.tensor(flags), 'key': ['000_00001', '000_00002']}
    gt_f = torch.from_numpy(ref.assemble(gt, flags))
    plain = {'LQs': torch.from_numpy(ref.assemble(lq, flags)), 'GT': gt_f if n_gt == N else gt_f[:, 0]}
    return packed, plain


def _net():
    return {'which_model_G': 'EDVR_NoUp', 'nf': 64, 'nc': 3, 'nframes': 3, 'groups': 8, 'front_RBs': 1, 'back_RBs': 1,
            'predeblur': False, 'HR_in': False, 'w_TSA': False, 'center': None}


@pytest.mark.parametrize('n_gt', [3, 1])
def test_model_feed_data_packed_equals_f32(n_gt):
    from realvsr_amd.VideoSR_model import create_model
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    opt = {'model': 'VideoSR_AllPair_YCbCr_Split', 'dist': False, 'gpu_ids': [0], 'is_train': True, 'scale': 1, 'augment': None,
           'network_G': _net(), 'path': {'pretrain_model_G': None, 'strict_load': True},
           'train': {'pixel_criterion_y': 'cb', 'pixel_weight_y': 1.0, 'pixel_criterion_c': 'gw', 'pixel_weight_c': 0.5,
                     'weight_decay_G': 0, 'ft_tsa_only': 0, 'lr_G': 1e-4, 'beta1': 0.9, 'beta2': 0.99}}
    model = create_model(opt)
    packed, plain = _packed_and_f32(n_gt, 40)
    model.feed_data(plain)
    var_L, var_H = model.var_L.clone(), model.var_H.clone()
    model.feed_data(packed)
    assert model.var_L.dtype == torch.float32 and tuple(model.var_L.shape) == (2, 3, 3, 16, 16)
    assert tuple(model.var_H.shape) == ((2, 3, 3, 16, 16) if n_gt == 3 else (2, 3, 16, 16))
    assert torch.equal(model.var_L, var_L) and torch.equal(model.var_H, var_H)
    model.optimize_parameters(1)
    assert np.isfinite(model.get_current_log()['l_pix'])
    model.feed_data(packed, need_GT=False)
    assert torch.equal(model.var_L, var_L)


def test_gan_model_feed_data_packed_equals_f32():
    from realvsr_amd.VideoSR_model import create_model
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    train = {'lr_G': 1e-4, 'weight_decay_G': 0, 'beta1_G': 0.9, 'beta2_G': 0.99, 'lr_D': 1e-4, 'weight_decay_D': 0, 'beta1_D': 0.9,
             'beta2_D': 0.99, 'pixel_criterion_s': 'cb', 'pixel_weight_s': 1.0, 'pixel_criterion_d': 'cb', 'pixel_weight_d': 1.0,
             'pixel_criterion_c': 'gw', 'pixel_weight_c': 1.0, 'feature_criterion': 'cb', 'feature_weight': 0.0, 'gan_type': 'ragan',
             'gan_weight': 0.1}
    opt = {'model': 'VideoSRGAN_AllPair_YCbCr_Split', 'dist': False, 'gpu_ids': [0], 'is_train': True, 'scale': 1, 'augment': None,
           'network_G': _net(), 'network_D': {'which_model_D': 'MultiscaleDiscriminator_v4', 'in_nc': 1, 'nf': 16, 'num_D': 2,
                                              'gan_type': 'patch'},
           'path': {'pretrain_model_G': None, 'pretrain_model_D': None, 'strict_load': True}, 'train': train}
    model = create_model(opt)
    packed, plain = _packed_and_f32(3, 50)
    model.feed_data(plain)
    var_L, var_H, var_ref = model.var_L.clone(), model.var_H.clone(), model.var_ref.clone()
    model.feed_data(packed)
    assert torch.equal(model.var_L, var_L) and torch.equal(model.var_H, var_H) and torch.equal(model.var_ref, var_ref)
