"""tests/glue_reference.py against the reference project's own numbers (the committed fixtures), on the CPU: the float64 references that
test_gpu_glue_edges.py holds the HIP kernels to are themselves pinned here, so a mistake in one of them cannot hide a kernel's."""
import numpy as np
import pytest
import torch

import glue_reference as G
from conftest import load_golden, rel_err


def _d(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).double().requires_grad_(grad)


def test_pyramids_match_the_integer_fixture():
    """pyramid_int.npz: level 0 of the band-pass pyramids and every Gaussian level hold values float32 represents exactly -> equal bit for
    bit after the cast; the deeper band-pass levels carry non-integers that the fixture's float32 arithmetic rounded (<= 1.5e-6 on
    values up to 16, measured) -> 1e-6 of the maximum."""
    g = load_golden('pyramid_int')
    for tag in 'abc':
        img = _d(g['img_' + tag])
        for name, lv in (('laplacian', 3), ('lap', 2), ('gau', 3)):
            for i, level in enumerate(G.PYRAMIDS[name](img, lv)):
                want = g['%s_%s_%d' % (name, tag, i)]
                assert tuple(level.shape) == want.shape, (name, tag, i)
                if name == 'gau' or i == 0:
                    assert np.array_equal(level.float().numpy(), want), (name, tag, i)
                else:
                    e = rel_err(level, torch.from_numpy(want))
                    assert e <= 1e-6, (name, tag, i, e)


def _loss_cases():
    cases = {'lappyr_cb': lambda x, y: G.lap_pyr_loss_cb(x, y, 3, 'mean'),
             'pyr_gau_cb': lambda x, y: G.pyramid_loss(x, y, 3, 'gau', 'cb'),
             'pyr_lap_l1': lambda x, y: G.pyramid_loss(x, y, 2, 'lap', 'l1'),
             'pyr_gau_l2': lambda x, y: G.pyramid_loss(x, y, 3, 'gau', 'l2'),
             'cb': lambda x, y: G.charbonnier(x, y),
             'gw': lambda x, y: G.gw_loss(x, y, 4, 'mean'),
             'gw_sum': lambda x, y: G.gw_loss(x, y, 2, 'sum')}
    return [(name, tag, fn) for tag in ('y', 'rgb') for name, fn in cases.items()]


@pytest.mark.parametrize('name,tag,fn', _loss_cases(), ids=lambda v: v if isinstance(v, str) else '')
def test_losses_match_the_fixture(name, tag, fn):
    """losses.npz (from the reference's loss.py in float32): values within 1e-6 relative (measured <= 7e-8), gradients within the 2e-5 of
    test_losses_fixture (measured <= 1.3e-5: the fixture's own float32 rounding in the Charbonnier gradient, whose slope at d = 0 is
    1 / sqrt(eps) = 1000; `lappyr_cb_sum` is left to the float32 kernels for that reason: its float32 rounding alone is 2.8e-5)."""
    g = load_golden('losses')
    x, y = _d(g['x_' + tag], True), _d(g['y_' + tag])
    l = fn(x, y)
    l.backward()
    ref = float(g['%s_%s' % (name, tag)])
    assert abs(l.item() - ref) <= 1e-6 * abs(ref), (l.item(), ref)
    e = rel_err(x.grad, torch.from_numpy(g['g_%s_%s' % (name, tag)]))
    assert e <= 2e-5, e


@pytest.mark.parametrize('tag', ['y', 'rgb'])
def test_lappyr_sum_value_matches_the_fixture(tag):
    """`lappyr_cb_sum` (two levels, reduction 'sum'): the value at the 1e-6 of the other keys.  Its gradient is not compared: the fixture's
    float32 rounding of it is 2.8e-5 (see above)."""
    g = load_golden('losses')
    l = G.lap_pyr_loss_cb(_d(g['x_' + tag]), _d(g['y_' + tag]), 2, 'sum')
    ref = float(g['lappyr_cb_sum_' + tag])
    assert abs(l.item() - ref) <= 1e-6 * abs(ref), (l.item(), ref)


@pytest.mark.parametrize('name,fn', [('hb', lambda x, y: G.huber(x, y)),
                                     ('hb_sum', lambda x, y: G.huber(x, y, 0.05, 'sum')),
                                     ('pyr_gau_hb', lambda x, y: G.pyramid_loss(x, y, 3, 'gau', 'hb')),
                                     ('pyr_lap_hb', lambda x, y: G.pyramid_loss(x, y, 2, 'lap', 'hb'))],
                         ids=['hb', 'hb_sum', 'pyr_gau_hb', 'pyr_lap_hb'])
def test_huber_losses_match_the_fixture(name, fn):
    g = load_golden('losses2')
    x, y = _d(g['x'], True), _d(g['y'])
    l = fn(x, y)
    l.backward()
    ref = float(g[name])
    assert abs(l.item() - ref) <= 1e-6 * abs(ref), (l.item(), ref)
    e = rel_err(x.grad, torch.from_numpy(g['g_' + name]))
    assert e <= 2e-5, e


def test_stand_alone_gauss_operators_match_the_fixture():
    """losses2.npz: conv_gauss (gain 1 and 4) and the pyramid upsample, values and gradients, at the bounds of
    test_conv_gauss_and_upsample_fixture; bit for bit on the integer images."""
    g = load_golden('losses2')
    for tag in 'ab':
        for fname, fn in (('conv_gauss', G.conv_gauss), ('conv_gauss4', lambda t: G.conv_gauss(t, 4.0)), ('upsample', G.pyr_upsample)):
            x = _d(g['%s_%s.in' % (fname, tag)], True)
            out = fn(x)
            out.backward(_d(g['%s_%s.gout' % (fname, tag)]))
            assert rel_err(out, torch.from_numpy(g['%s_%s.out' % (fname, tag)])) <= 1e-6
            assert rel_err(x.grad, torch.from_numpy(g['%s_%s.gin' % (fname, tag)])) <= 2e-6
        ii = _d(g['int_%s.in' % tag])
        assert np.array_equal(G.conv_gauss(ii).float().numpy(), g['int_%s.conv_gauss' % tag])
        assert np.array_equal(G.pyr_upsample(ii).float().numpy(), g['int_%s.upsample' % tag])


def test_max_pool_gradient_goes_to_the_first_maximum():
    """The routing the pool reference stands for: with most windows tied (values from {0, 1, 2}) autograd of maxavgpool's max half equals
    the rule written out in first_max_routing, at an odd and an even size."""
    gen = torch.Generator().manual_seed(11)
    for shape in [(1, 2, 2, 2), (2, 2, 7, 9), (1, 2, 8, 6)]:
        x = torch.randint(0, 3, shape, generator=gen).double().requires_grad_(True)
        out = G.maxavgpool(x)
        C = shape[1]
        gmax = torch.randint(-8, 9, out[:, :C].shape, generator=gen).double()
        out.backward(torch.cat([gmax, torch.zeros_like(gmax)], 1))
        assert torch.equal(x.grad, G.first_max_routing(x.detach(), gmax)), shape


def test_adam_reference_matches_torch_adam():
    """adam_step in float64 against torch.optim.Adam(foreach=False) on a float64 parameter: three steps, with and without weight decay."""
    gen = torch.Generator().manual_seed(12)
    for wd in (0.0, 1e-2):
        p0 = torch.randn(37, generator=gen, dtype=torch.float64)
        par = torch.nn.Parameter(p0.clone())
        opt = torch.optim.Adam([par], lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd, foreach=False)
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        for t in (1, 2, 3):
            gr = torch.randn(37, generator=gen, dtype=torch.float64)
            par.grad = gr.clone()
            opt.step()
            p, m, v = G.adam_step(p, gr, m, v, t, 1e-3, 0.9, 0.99, 1e-8, wd)
        assert rel_err(p - p0, par.detach() - p0) <= 1e-12
        assert rel_err(v, opt.state[par]['exp_avg_sq']) <= 1e-12


def test_frame_major_tsa_is_the_transposed_call():
    gen = torch.Generator().manual_seed(13)
    emb, al = torch.randn(2, 3, 4, 5, 6, generator=gen, dtype=torch.float64), torch.randn(2, 3, 4, 5, 6, generator=gen, dtype=torch.float64)
    ref = torch.randn(2, 4, 5, 6, generator=gen, dtype=torch.float64)
    a = G.tsa_temporal(emb, ref, al)
    b = G.tsa_temporal(emb.transpose(0, 1).contiguous(), ref, al.transpose(0, 1).contiguous(), frame_major=True)
    assert torch.equal(a, b)
    # one entry by hand: frame 2 of batch element 1, channel 3, pixel (4, 5)
    pr = 1 / (1 + torch.exp(-(emb[1, 2, :, 4, 5] * ref[1, :, 4, 5]).sum()))
    assert abs(a[1, 2 * 4 + 3, 4, 5] - al[1, 2, 3, 4, 5] * pr) <= 1e-15
