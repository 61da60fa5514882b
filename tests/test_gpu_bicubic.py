"""rvsr_bicubic_u8 (csrc/resize_kernels.hip) and its callers against the exact model tests/bicubic_reference.py, on the GPU.

Every comparison is ==: the operator is defined in integers (include/realvsr_hip.h section 13).  Sources are carved out of larger uint8
buffers at an odd byte, destinations out of buffers of guard bytes that have to stay untouched.  tests/test_bicubic_host.py holds the
model itself against the recorded output of the reference's imresize_np and Vimeo-90K classes.
"""
import json
import random

import numpy as np
import pytest
import torch

import bicubic_reference as br
from conftest import load_golden
from gpu_util import dev

pytestmark = pytest.mark.gpu

CHAINS = ((2, br.SAME), (2, br.DOWN), (4, br.SAME), (4, br.DOWN))
GUARD, FILL = 64, 0xA5


def rand_u8(seed, *shape):
    return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)


def carve(shape, d):
    """A uint8 tensor of `shape` inside a larger buffer of guard bytes, starting at an odd byte -> (buffer, view)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + 1,), FILL, dtype=torch.uint8, device=d)
    start = GUARD + (1 if buf.data_ptr() % 2 == 0 else 0)
    assert (buf.data_ptr() + start) % 2 == 1
    return buf, buf[start:start + n].view(shape), start, n


def guards_intact(buf, start, n):
    return bool((buf[:start] == FILL).all()) and bool((buf[start + n:] == FILL).all())


def run(src, scale, mode, geom=None, frame_hw=None, crop_hw=None):
    """The raw entry point on `src` (numpy uint8 [B, F, Hw, Ww, C]) placed at an odd byte of a larger block, into guarded dst and crop;
    returns (dst, crop) on the CPU after checking that no guard byte changed."""
    from realvsr_amd import _lib
    from realvsr_amd._lib import _p, _stream
    d = dev()
    B, F, Hw, Ww, C = src.shape
    frame_hw = frame_hw or (Hw, Ww)
    crop_hw = crop_hw or frame_hw
    out_hw = (crop_hw[0] // scale, crop_hw[1] // scale) if mode == br.DOWN else crop_hw
    sbuf, s, s0, sn = carve(src.shape, d)
    s.copy_(torch.from_numpy(np.ascontiguousarray(src)).to(d))
    dbuf, dst, d0, dn = carve((B, F) + tuple(out_hw) + (C,), d)
    cbuf, crop, c0, cn = carve((B, F) + tuple(crop_hw) + (C,), d)
    g = None if geom is None else torch.tensor(np.asarray(geom), dtype=torch.int32).reshape(B, 4).to(d)
    rc = _lib.lib().rvsr_bicubic_u8(_p(s), _p(dst), _p(crop), _p(g), B, F, C, Hw, Ww, frame_hw[0], frame_hw[1], crop_hw[0], crop_hw[1],
                                    scale, mode, _stream())
    _lib.check(rc, 'bicubic_u8')
    torch.cuda.synchronize()
    assert guards_intact(dbuf, d0, dn) and guards_intact(cbuf, c0, cn), 'a store left the destination'
    assert guards_intact(sbuf, s0, sn) and bool((s.cpu() == torch.from_numpy(src)).all())
    return dst.cpu().numpy(), crop.cpu().numpy()


def check(src, scale, mode, geom=None, frame_hw=None, crop_hw=None):
    B, F, Hw, Ww, C = src.shape
    frame_hw = frame_hw or (Hw, Ww)
    crop_hw = crop_hw or frame_hw
    want_dst, want_crop = br.bicubic_u8(src, geom, frame_hw, crop_hw, scale, mode)
    dst, crop = run(src, scale, mode, geom, frame_hw, crop_hw)
    assert dst.shape == want_dst.shape and (dst == want_dst).all(), 'dst: %d values differ' % int((dst != want_dst).sum())
    assert (crop == want_crop).all(), 'crop'


@pytest.mark.parametrize('scale,mode', CHAINS)
@pytest.mark.parametrize('C', [1, 3])
def test_whole_frames(scale, mode, C):
    """The minimum frames (4 x 6 at scale 2, 8 x 12 at scale 4: every tap row reflects), 8 x 8, 16 x 16, and one tile edge straddled in
    both directions (SAME tiles are 32 x 32 of the frame, DOWN tiles 16 x 16 of the shrunk frame); frames 1 and 3, samples 2."""
    shapes = [(4, 6), (8, 12), (8, 8), (16, 16), (66, 130)] if scale == 2 else [(8, 12), (8, 8), (16, 16), (68, 132)]
    for k, (H, W) in enumerate(shapes):
        F = 3 if k % 2 else 1
        check(rand_u8(100 * scale + 10 * mode + k + C, 2, F, H, W, C), scale, mode)


@pytest.mark.parametrize('scale,mode', CHAINS)
def test_step_image_where_both_clamps_fire(scale, mode):
    src = br.step_image(32, 48)
    N, b = br.numerators(src, scale, mode), br.shift_bits(scale, mode)
    q = (N + (1 << (b - 1))) >> b
    assert q.min() < 0 and q.max() > 255
    check(src[None, None], scale, mode)
    check(np.ascontiguousarray(src[None, None, :, :, :1]), scale, mode)


@pytest.mark.parametrize('scale,mode', CHAINS)
def test_windows_with_a_geometry_per_sample(scale, mode):
    """Crops taken through windows, two samples with different geometry per launch: the four corners, odd origins (multiples of the
    scale for DOWN), a crop that straddles a tile (40), frames 1 and 3, C = 1 and 3 -- each equal to the crop of the whole-frame chain."""
    from realvsr_amd import data
    Hf, Wf = 80, 96
    step = scale if mode == br.DOWN else 1
    for S, F, C in ((16, 3, 3), (40, 1, 1)):
        last_y, last_x = Hf - S, Wf - S
        origins = [(0, 0), (0, last_x), (last_y, 0), (last_y, last_x), (step, 3 * step), (7 * step, 5 * step),
                   (last_y - step, last_x - 3 * step), (last_y // 2 // step * step + step, step)]
        frames = rand_u8(7 * scale + mode + S, len(origins), F, Hf, Wf, C)
        whole = np.stack([np.stack([br.degrade_frame(f, scale, mode) for f in clip]) for clip in frames])
        for i in range(0, len(origins), 2):
            windows, geoms = [], []
            for k in (i, i + 1):
                (wy, wx), (Hw, Ww), geom = data.degrade_window_plan({'rnd_h': origins[k][0], 'rnd_w': origins[k][1], 'size': S}, (Hf, Wf),
                                                                    scale, mode)
                windows.append(frames[k][:, wy:wy + Hw, wx:wx + Ww])
                geoms.append(geom)
            src = np.ascontiguousarray(np.stack(windows))
            dst, crop = run(src, scale, mode, geoms, (Hf, Wf), (S, S))
            for j, k in enumerate((i, i + 1)):
                y0, x0 = origins[k]
                if mode == br.DOWN:
                    want = whole[k][:, y0 // scale:(y0 + S) // scale, x0 // scale:(x0 + S) // scale]
                else:
                    want = whole[k][:, y0:y0 + S, x0:x0 + S]
                assert (dst[j] == want).all(), (S, origins[k])
                assert (crop[j] == frames[k][:, y0:y0 + S, x0:x0 + S]).all(), (S, origins[k])


def test_wrapper_checks_and_shapes():
    from realvsr_amd import data
    d = dev()
    src = rand_u8(3, 2, 2, 16, 24, 3)
    t = torch.from_numpy(src).to(d)
    for scale, mode in CHAINS:
        name = 'down' if mode == br.DOWN else 'same'
        want, _ = br.bicubic_u8(src, None, (16, 24), (16, 24), scale, mode)
        assert (data.bicubic_u8(t, scale, name).cpu().numpy() == want).all()
        dst, crop = data.bicubic_u8(t, scale, mode, want_crop=True)
        assert (dst.cpu().numpy() == want).all() and torch.equal(crop, t)
    from realvsr_amd import _lib
    assert [_lib.lib().rvsr_bicubic_halo(s, m) for s, m in CHAINS] == [7, 3, 15, 6]
    assert _lib.lib().rvsr_bicubic_halo(3, 0) == -1 and _lib.lib().rvsr_bicubic_halo(2, 2) == -1


def test_refusals_are_errors():
    """Everything the entry point or the wrapper refuses comes back as an error; nothing is launched."""
    from realvsr_amd import data
    d = dev()
    ok = torch.zeros(2, 1, 16, 16, 3, dtype=torch.uint8, device=d)
    with pytest.raises(RuntimeError):
        data.bicubic_u8(ok.cpu(), 2)
    with pytest.raises(RuntimeError):
        data.bicubic_u8(ok.float(), 2)
    with pytest.raises(RuntimeError, match='contiguous'):
        data.bicubic_u8(torch.zeros(2, 1, 16, 16, 6, dtype=torch.uint8, device=d)[..., ::2], 2)
    with pytest.raises(RuntimeError, match='channels'):
        data.bicubic_u8(torch.zeros(2, 1, 16, 16, 2, dtype=torch.uint8, device=d), 2)
    with pytest.raises(RuntimeError, match='scale'):
        data.bicubic_u8(ok, 3)
    with pytest.raises(RuntimeError, match='mode'):
        data.bicubic_u8(ok, 2, 'up')
    with pytest.raises(RuntimeError, match='multiple of the scale'):   # odd frame sizes
        data.bicubic_u8(torch.zeros(1, 1, 15, 16, 3, dtype=torch.uint8, device=d), 2)
    with pytest.raises(RuntimeError, match='multiple of the scale'):
        data.bicubic_u8(torch.zeros(1, 1, 16, 18, 3, dtype=torch.uint8, device=d), 4)
    with pytest.raises(RuntimeError, match='below 2'):                 # an edge below 2 * scale
        data.bicubic_u8(torch.zeros(1, 1, 4, 16, 3, dtype=torch.uint8, device=d), 4)
    with pytest.raises(RuntimeError, match='below 2'):
        data.bicubic_u8(torch.zeros(1, 1, 16, 2, 3, dtype=torch.uint8, device=d), 2)
    geom = torch.tensor([[0, 0, 2, 4], [0, 0, 4, 4]], dtype=torch.int32)
    with pytest.raises(ValueError, match='multiples of the scale'):    # an unaligned DOWN origin
        data.bicubic_u8(ok, 4, 'down', geom=geom, frame_hw=(16, 16), crop_hw=(8, 8))
    with pytest.raises(RuntimeError, match='multiple of the scale'):   # an unaligned DOWN crop size
        data.bicubic_u8(ok, 4, 'down', geom=geom.to(d), frame_hw=(16, 16), crop_hw=(6, 8))
    with pytest.raises(ValueError, match='do not cover'):              # a window that does not hold the halo: by its place ...
        data.bicubic_u8(ok, 2, 'same', geom=torch.tensor([[30, 30, 40, 40], [30, 30, 30, 30]], dtype=torch.int32), frame_hw=(64, 64),
                        crop_hw=(2, 2))
    with pytest.raises(RuntimeError, match='does not cover'):          # ... and by its size (the entry point's own check)
        data.bicubic_u8(ok, 2, 'same', geom=torch.tensor([[30, 30, 37, 37]] * 2, dtype=torch.int32).to(d), frame_hw=(64, 64), crop_hw=(8, 8))
    with pytest.raises(RuntimeError, match='exceeds'):
        data.bicubic_u8(ok, 2, 'same', frame_hw=(8, 16))
    with pytest.raises(RuntimeError, match='geom'):
        data.bicubic_u8(ok, 2, 'same', geom=torch.zeros(2, 4, dtype=torch.int64), frame_hw=(64, 64), crop_hw=(2, 2))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def fixture(tmp_path_factory):
    g = load_golden('bicubic')
    meta = json.loads(str(g['meta']))
    root = str(tmp_path_factory.mktemp('vimeo'))
    br.write_tree(g, meta, root)
    return g, meta, root


@pytest.fixture(scope='module')
def model():
    from realvsr_amd.VideoSR_model import create_model
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    net = {'which_model_G': 'EDVR_NoUp', 'nf': 64, 'nc': 3, 'nframes': 3, 'groups': 8, 'front_RBs': 1, 'back_RBs': 1,
           'predeblur': False, 'HR_in': False, 'w_TSA': False, 'center': None}
    opt = {'model': 'VideoSR_AllPair_YCbCr_Split', 'dist': False, 'gpu_ids': [0], 'is_train': True, 'scale': 1, 'augment': None,
           'network_G': net, 'path': {'pretrain_model_G': None, 'strict_load': True},
           'train': {'pixel_criterion_y': 'cb', 'pixel_weight_y': 1.0, 'pixel_criterion_c': 'gw', 'pixel_weight_c': 0.5,
                     'weight_decay_G': 0, 'ft_tsa_only': 0, 'lr_G': 1e-4, 'beta1': 0.9, 'beta2': 0.99}}
    return create_model(opt)


def collate(samples):
    return torch.utils.data.dataloader.default_collate(samples)


@pytest.mark.parametrize('ycbcr', [False, True])
def test_synthesized_batches_equal_the_stored_files_through_the_model(fixture, model, ycbcr):
    """The fixture's tree, every recorded run: synthesize_LQ samples (GT windows only) staged through the pinned ClipBatchStager as
    frames_gt with frames_lq = 0 and fed to VideoSRModel.feed_data give var_L and var_H bit-identical to the batch built from the
    tree's stored LQ and GT files (written by the reference's imresize_np chain) through the existing packed path; with
    RVSR_ASM_TO_YCBCR the degradation runs on the colour bytes and the conversion after it."""
    from realvsr_amd import data
    g, meta, root = fixture
    mode = data.RVSR_ASM_REVERSE | (data.RVSR_ASM_TO_YCBCR if ycbcr else 0)
    for r, run in enumerate(meta['runs']):
        random.seed(run['seed'])
        stored = collate([br.make_dataset(run, root, meta)[i] for i in run['indices']])
        assert stored['LQs'].dtype == torch.uint8
        model.feed_data(dict(stored, mode=mode))
        want_L, want_H = model.var_L.clone(), model.var_H.clone()

        random.seed(run['seed'])
        synth = [br.make_dataset(run, root, meta, synthesize=True)[i] for i in run['indices']]
        B, (N, side, _, C) = len(synth), synth[0]['GT_window'].shape
        stager = data.ClipBatchStager(B, 0, N, side, C, pin=True, slots=2)
        for i, s in enumerate(synth):
            stager.stage(i, [], list(s['GT_window'].numpy()), {'rnd_h': None, 'rnd_w': None, 'size': None, 'flags': s['flags']})
        _, windows, flags = stager.upload()
        assert windows.is_cuda and tuple(windows.shape) == (B, N, side, side, C)
        batch = collate([{k: v for k, v in s.items() if k != 'GT_window'} for s in synth])
        assert torch.equal(batch['flags'].to(flags.device, torch.int32), flags)
        model.feed_data(dict(batch, GT_window=windows, flags=flags, mode=mode))
        assert model.var_L.shape == want_L.shape and model.var_H.shape == want_H.shape
        assert torch.equal(model.var_L, want_L), 'run %d: var_L' % r
        assert torch.equal(model.var_H, want_H), 'run %d: var_H' % r
        model.feed_data(dict(collate(synth), mode=mode), need_GT=False)   # (and straight from the collated host samples)
        assert torch.equal(model.var_L, want_L)


def test_gan_model_takes_the_window_form(fixture):
    from realvsr_amd.VideoSR_model import create_model
    g, meta, root = fixture
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    train = {'lr_G': 1e-4, 'weight_decay_G': 0, 'beta1_G': 0.9, 'beta2_G': 0.99, 'lr_D': 1e-4, 'weight_decay_D': 0, 'beta1_D': 0.9,
             'beta2_D': 0.99, 'pixel_criterion_s': 'cb', 'pixel_weight_s': 1.0, 'pixel_criterion_d': 'cb', 'pixel_weight_d': 1.0,
             'pixel_criterion_c': 'gw', 'pixel_weight_c': 1.0, 'feature_criterion': 'cb', 'feature_weight': 0.0, 'gan_type': 'ragan',
             'gan_weight': 0.1}
    net = {'which_model_G': 'EDVR_NoUp', 'nf': 64, 'nc': 3, 'nframes': 3, 'groups': 8, 'front_RBs': 1, 'back_RBs': 1,
           'predeblur': False, 'HR_in': False, 'w_TSA': False, 'center': None}
    opt = {'model': 'VideoSRGAN_AllPair_YCbCr_Split', 'dist': False, 'gpu_ids': [0], 'is_train': True, 'scale': 1, 'augment': None,
           'network_G': net, 'network_D': {'which_model_D': 'MultiscaleDiscriminator_v4', 'in_nc': 1, 'nf': 16, 'num_D': 2,
                                           'gan_type': 'patch'},
           'path': {'pretrain_model_G': None, 'pretrain_model_D': None, 'strict_load': True}, 'train': train}
    gan = create_model(opt)
    run = meta['runs'][0]
    random.seed(run['seed'])
    gan.feed_data(collate([br.make_dataset(run, root, meta)[i] for i in run['indices']]))
    want = gan.var_L.clone(), gan.var_H.clone(), gan.var_ref.clone()
    random.seed(run['seed'])
    gan.feed_data(collate([br.make_dataset(run, root, meta, synthesize=True)[i] for i in run['indices']]))
    assert torch.equal(gan.var_L, want[0]) and torch.equal(gan.var_H, want[1]) and torch.equal(gan.var_ref, want[2])
