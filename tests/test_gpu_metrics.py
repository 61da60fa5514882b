"""The device-side validation metrics (csrc/metric_kernels.hip through realvsr_amd.metrics) against the float64 restatement of the
reference in tests/metrics_reference.py and the values the reference's own functions recorded in tests/golden/metrics.npz.

Every input is a view inside a NaN-filled buffer, at an odd element offset and with a plane stride larger than H * W: the kernels read
the planes in place (asserted below), nothing they may read is 16-byte aligned by construction, and the cropped-away border and the gaps
between planes hold NaN too.

Bounds.  The quantisation and the PSNR are exact: compared bit for bit and with ==.  SSIM_TOL = 1e-9 absolute is derived, not measured:
each of the five filtered maps is a 121-term sum of positive terms of at most 65025, so any summation order (the device's separable
11 + 11 taps in fused multiply-adds, the helper's 121 taps in turn) errs by at most about 120 * 2^-53 * 65025 = 9e-10 per map, and the
formula divides by factors of at least C1 = 6.5 and C2 = 58.5.  The largest difference each test saw is printed (about 1e-13)."""
import ctypes

import numpy as np
import pytest
import torch

import metrics_reference as MR
from conftest import load_golden
from gpu_util import dev

pytestmark = pytest.mark.gpu

SSIM_TOL = 1e-9
NAN = float('nan')


def _tile():
    from realvsr_amd import _lib
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    assert _lib.lib().rvsr_metric_tile(ctypes.byref(th), ctypes.byref(tw)) == 0
    return th.value, tw.value


def _embed(planes, pad, offset):
    """planes: numpy [P, H, W] float32 -> a [P, 1, H, W] CUDA view into a NaN-filled buffer that starts `offset` elements into it and
    whose planes are H * W + pad elements apart."""
    from realvsr_amd import metrics as M
    P, H, W = planes.shape
    stride = H * W + pad
    buf = torch.full((offset + P * stride + 7,), NAN, dtype=torch.float32, device=dev())
    view = torch.as_strided(buf, (P, 1, H, W), (stride, H * W, W, 1), offset)
    view.copy_(torch.from_numpy(planes).unsqueeze(1))
    kept = M._planes(view[:, 0], 'test')
    assert kept[0].data_ptr() == view.data_ptr() and kept[4] == (stride if P > 1 else H * W), 'the metric must read the view in place'
    assert torch.isnan(buf).sum().item() == buf.numel() - P * H * W
    return view


def _pair(rng, content, P, H, W):
    if content == 'noise':
        return (rng.rand(P, H, W) * 1.1 - 0.05).astype(np.float32), (rng.rand(P, H, W) * 1.1 - 0.05).astype(np.float32)
    if content == 'close':
        a = rng.rand(P, H, W).astype(np.float32)
        return a, (a + 0.02 * rng.randn(P, H, W)).astype(np.float32)
    if content == 'flat':      # constant planes: E[x^2] - mu^2 cancels to rounding noise
        return (np.ones((P, H, W), np.float32) * rng.rand(P, 1, 1).astype(np.float32),
                np.ones((P, H, W), np.float32) * rng.rand(P, 1, 1).astype(np.float32))
    raise ValueError(content)


def _cases():
    """(Hc, Wc) of the CROPPED plane: every H at one W beyond a tile, every W at one H beyond a tile, and the corners; crop_border,
    plane count and content cycle through their values along the list."""
    TH, TW = _tile()
    hs = [11, 12, TH + 9, TH + 10, TH + 11, 2 * TH + 11]
    ws = [11, 13, TW + 9, TW + 10, TW + 11, 2 * TW + 11]
    shapes = [(h, TW + 11) for h in hs] + [(TH + 11, w) for w in ws if w != TW + 11] + [(11, 11), (12, 13), (2 * TH + 11, 2 * TW + 11),
                                                                                     (11, 2 * TW + 11), (2 * TH + 11, 11)]
    crops, planes, contents = [0, 1, 4], [1, 3, 5], ['noise', 'close', 'noise', 'flat']
    return [(h, w, crops[i % 3], planes[(i // 2) % 3], contents[i % 4]) for i, (h, w) in enumerate(shapes)]


@pytest.fixture(scope='module')
def scored():
    """Every case once: inputs, device results, float64 reference -- shared by the PSNR and the SSIM test."""
    from realvsr_amd import metrics as M
    rng = np.random.RandomState(7)
    out = []
    for n, (hc, wc, crop, P, content) in enumerate(_cases()):
        H, W = hc + 2 * crop, wc + 2 * crop
        a, b = _pair(rng, content, P, H, W)
        va, vb = _embed(a, 5 + 2 * n, 1 + 2 * n), _embed(b, 9 + 2 * n, 3)
        got = M.frame_metrics(va, vb, crop_border=crop, ssim=True)
        ref = {'psnr': [MR.psnr_plane(a[p], b[p], crop) for p in range(P)], 'ssim': [MR.ssim_plane(a[p], b[p], crop) for p in range(P)]}
        out.append(((hc, wc, crop, P, content), got, ref))
    return out


def test_quantize_matches_numpy_bit_for_bit():
    from realvsr_amd import metrics as M
    vals = []
    for k in range(256):
        for base in (np.float32(k / 255.0), np.float32((k + 0.5) / 255.0)):
            up = down = base
            vals.append(base)
            for _ in range(4):
                up, down = np.nextafter(up, np.float32(np.inf)), np.nextafter(down, np.float32(-np.inf))
                vals += [up, down]
    vals += [-0.0, -1.0, -1e-30, -3.5, 1.0000001, 1.5, 2.0, 255.0, 1e30, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, 1.1754942e-38, 0.5]
    x = np.array(vals, dtype=np.float32)
    assert x.size == 2 * 256 * 9 + 16
    buf = torch.full((x.size + 4,), NAN, dtype=torch.float32, device=dev())
    buf[1:1 + x.size] = torch.from_numpy(x)
    got = M.quantize_u8(buf[1:1 + x.size])
    assert got.dtype == torch.uint8 and got.shape == (x.size,)
    want = MR.quantize(x)
    bad = np.nonzero(got.cpu().numpy() != want)[0]
    assert bad.size == 0, [(float(x[i]), int(want[i])) for i in bad[:8]]
    assert want.min() == 0 and want.max() == 255 and len(set(want.tolist())) == 256
    # NaN has no defined uint8 in numpy; the device maps it to 0 (documented in include/realvsr_hip.h)
    assert M.quantize_u8(buf[:1]).item() == 0
    # a [B, C, H, W] shape comes back as it went in
    assert M.quantize_u8(torch.full((2, 3, 4, 5), 0.5, device=dev())).shape == (2, 3, 4, 5)


def test_psnr_equals_the_float64_reference(scored):
    for case, got, ref in scored:
        assert got['psnr'] == ref['psnr'], (case, got['psnr'], ref['psnr'])
        assert all(np.isfinite(v) for v in got['psnr'])


def test_psnr_sum_beyond_32_bits_is_exact():
    """2048 x 2048 of 0 against 1: sse = 65025 * 2^22 > 2^32; then one pixel changed, so that a sum that lost its low bits shows."""
    from realvsr_amd import metrics as M
    n = 2048 * 2048
    a = torch.zeros(1, 1, 2048, 2048, device=dev())
    b = torch.ones(1, 1, 2048, 2048, device=dev())
    assert M.psnr_y(a, b) == [M.psnr_from_sse(65025 * 2 ** 22, n)] == [0.0]
    b[0, 0, 1234, 567] = 0.5     # quantises to 128
    sse = 65025 * (n - 1) + 128 * 128
    assert sse > 2 ** 32 and M.psnr_y(a, b) == [M.psnr_from_sse(sse, n)] != [0.0]
    assert M.psnr_y(a, b, crop_border=3) == [M.psnr_from_sse(65025 * (2042 * 2042 - 1) + 128 * 128, 2042 * 2042)]
    assert M.psnr_y(b, b) == [float('inf')]


def test_ssim_within_the_derived_bound(scored):
    worst = 0.0
    for case, got, ref in scored:
        for g, r in zip(got['ssim'], ref['ssim']):
            assert np.isfinite(g), case
            worst = max(worst, abs(g - r))
            assert abs(g - r) <= SSIM_TOL, (case, g, r)
    print('ssim: largest |device - float64 reference| over %d cases: %.3e (bound %.0e)' % (len(scored), worst, SSIM_TOL))


def test_ssim_of_identical_inputs_is_exactly_one():
    from realvsr_amd import metrics as M
    TH, TW = _tile()
    rng = np.random.RandomState(3)
    for (H, W, crop) in ((11, 11, 0), (TH + 11, 2 * TW + 11, 0), (2 * TH + 19, TW + 18, 4)):
        a = (rng.rand(3, H, W) * 1.1 - 0.05).astype(np.float32)
        va, vb = _embed(a, 3, 1), _embed(a, 11, 5)
        got = M.frame_metrics(va, vb, crop_border=crop)
        assert got['ssim'] == [1.0] * 3 and got['psnr'] == [float('inf')] * 3, (H, W, crop, got)


def test_ssim_refuses_a_plane_below_the_window():
    from realvsr_amd import metrics as M
    x = torch.rand(1, 1, 18, 40, device=dev())
    assert len(M.ssim_y(x, x, crop_border=3)) == 1                      # 12 x 34
    with pytest.raises(RuntimeError, match='smaller than the 11 x 11 window'):
        M.ssim_y(x, x, crop_border=4)                                   # 10 high
    with pytest.raises(RuntimeError, match='smaller than the 11 x 11 window'):
        M.ssim_y(x.transpose(2, 3), x.transpose(2, 3), crop_border=4)   # 10 wide
    assert len(M.psnr_y(x, x, crop_border=8)) == 1                      # PSNR takes any non-empty plane: 2 x 24
    with pytest.raises(RuntimeError, match='is empty'):
        M.psnr_y(x, x, crop_border=9)
    with pytest.raises(ValueError):
        M.psnr_y(x, x[:, :, :, :39])


def test_two_runs_are_bit_identical():
    from realvsr_amd import metrics as M
    TH, TW = _tile()
    rng = np.random.RandomState(11)
    a, b = _pair(rng, 'close', 3, 3 * TH + 5, 4 * TW + 3)
    va, vb = _embed(a, 7, 1), _embed(b, 1, 3)
    first = M.frame_metrics(va, vb, crop_border=1)
    torch.empty(1 << 22, device=dev()).normal_()     # other work in between
    assert M.frame_metrics(va, vb, crop_border=1) == first
    assert M.ssim_y(va, vb, crop_border=1) == first['ssim'] and M.psnr_y(va, vb, crop_border=1) == first['psnr']


def test_reference_recorded_values():
    """tests/golden/metrics.npz: what the reference's tensor2img + train.py:301-305 chain, calculate_psnr and calculate_ssim returned."""
    from realvsr_amd import metrics as M
    g = load_golden('metrics')
    worst = 0.0
    for i in range(3):
        a, b = torch.from_numpy(g['a%d' % i]).to(dev()), torch.from_numpy(g['b%d' % i]).to(dev())
        assert np.array_equal(M.quantize_u8(a).permute(1, 2, 0).cpu().numpy(), g['qa%d' % i])
        assert np.array_equal(M.quantize_u8(b).permute(1, 2, 0).cpu().numpy(), g['qb%d' % i])
        assert M.calculate_psnr(a[0], b[0]) == float(g['psnr%d' % i])
        assert M.calculate_psnr(a, b) == float(g['psnr3_%d' % i])
        assert M.psnr_y(a, b) == [float(g['psnr%d' % i])]
        for got, key in ((M.calculate_ssim(a[0], b[0]), 'ssim2d_%d'), (M.calculate_ssim(a[0:1], b[0:1]), 'ssim1_%d'),
                         (M.calculate_ssim(a, b), 'ssim3_%d'), (M.ssim_y(a, b)[0], 'ssim2d_%d')):
            worst = max(worst, abs(got - float(g[key % i])))
            assert abs(got - float(g[key % i])) <= SSIM_TOL, (key % i, got, float(g[key % i]))
    print('ssim: largest |device - recorded reference|: %.3e (bound %.0e)' % (worst, SSIM_TOL))


def _net_opt():
    # the smallest EDVR_NoUp there is: like the reference's, the class only works at nf = 64 (its HRconv is 64 -> 64)
    return {'which_model_G': 'EDVR_NoUp', 'nf': 64, 'nc': 3, 'nframes': 3, 'groups': 8, 'front_RBs': 1, 'back_RBs': 1, 'center': None,
            'predeblur': False, 'HR_in': False, 'w_TSA': True}


@pytest.mark.parametrize('model_name', ['VideoSR_AllPair_YCbCr_Split', 'VideoSRGAN_AllPair_YCbCr_Split'])
def test_model_metrics_equal_the_host_path(model_name):
    """get_current_metrics against the reference's route: get_current_visuals (sample 0 on the host) through the float64 helper; the
    second sample straight from the model's tensors.  A five-dimensional GT is scored at its centre frame, a four-dimensional one as is."""
    from realvsr_amd.VideoSR_model import create_model
    torch.manual_seed(0)
    model = create_model({'model': model_name, 'dist': False, 'gpu_ids': [0], 'is_train': False, 'scale': 1, 'network_G': _net_opt(),
                          'path': {'pretrain_model_G': None, 'strict_load': True}})
    gen = torch.Generator().manual_seed(5)
    lq = torch.rand(2, 3, 3, 16, 16, generator=gen)
    gt5 = (lq + 0.05 * torch.randn(2, 3, 3, 16, 16, generator=gen)).clamp(0, 1)
    for gt in (gt5, gt5[:, 1].contiguous()):
        model.feed_data({'LQs': lq, 'GT': gt})
        model.test()
        got = model.get_current_metrics(ssim=True)
        vis = model.get_current_visuals()
        hq0, gt0 = vis['HQ'].numpy(), (vis['GT'][1] if gt.dim() == 5 else vis['GT']).numpy()
        hq1, gt1 = model.fake_H[1].cpu().numpy(), gt5[1, 1].numpy()
        assert got['psnr'] == [MR.psnr_plane(hq0[0], gt0[0]), MR.psnr_plane(hq1[0], gt1[0])]
        assert all(np.isfinite(v) for v in got['psnr'])
        for g, r in zip(got['ssim'], [MR.ssim_plane(hq0[0], gt0[0]), MR.ssim_plane(hq1[0], gt1[0])]):
            assert abs(g - r) <= SSIM_TOL
        assert model.get_current_metrics() == {'psnr': got['psnr'], 'ssim': []}
        crop = model.get_current_metrics(ssim=True, crop_border=2)
        assert crop['psnr'] == [MR.psnr_plane(hq0[0], gt0[0], 2), MR.psnr_plane(hq1[0], gt1[0], 2)]
        assert abs(crop['ssim'][0] - MR.ssim_plane(hq0[0], gt0[0], 2)) <= SSIM_TOL


def test_evaluate_clip():
    from realvsr_amd import infer, metrics as M
    from realvsr_amd.VideoSR_archs import define_G
    torch.manual_seed(0)
    net = define_G({'network_G': _net_opt(), 'scale': 1}).to(dev()).eval()
    gen = torch.Generator().manual_seed(9)
    clip = torch.rand(5, 3, 16, 16, generator=gen).to(dev())
    gt = (clip.cpu() + 0.05 * torch.randn(5, 3, 16, 16, generator=gen)).clamp(0, 1).to(dev())
    runner = infer.SlidingWindowRunner(net, 3)
    res = infer.evaluate_clip(runner, clip, gt, crop_border=1, ssim=True)
    out = runner(clip)
    assert len(res['psnr']) == len(res['ssim']) == 5
    for t in range(5):
        one = M.frame_metrics(out[t], gt[t], crop_border=1)
        assert [res['psnr'][t]] == one['psnr'] and [res['ssim'][t]] == one['ssim']
        assert res['psnr'][t] == MR.psnr_plane(out[t, 0].cpu().numpy(), gt[t, 0].cpu().numpy(), 1)
    for name in ('psnr', 'ssim'):
        avg = M.center_border_average(res[name], 1)
        assert (res[name + '_avg'], res[name + '_center'], res[name + '_border']) == (avg['avg'], avg['center'], avg['border'])
    assert res['psnr_center'] == sum(res['psnr'][1:4]) / 3 and res['psnr_border'] == (res['psnr'][0] + res['psnr'][4]) / 2
    only = infer.evaluate_clip(runner, clip, gt, crop_border=1, ssim=False)
    assert only['psnr'] == res['psnr'] and 'ssim' not in only and 'ssim_avg' not in only
