"""The case list of tests/gan_reference.py held to the conditions its cases are named for, so that test_gpu_gan_edges.py cannot
silently test nothing; and the float64 reference functions against the module-level wiring of the reference project
(nn.BatchNorm2d, nn.BCEWithLogitsLoss).  No GPU."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import gan_reference as GR


def _np_of_library(B, C, HW):
    """NP from the exported pure-host function: workspace = C * NP * 2 doubles + 3 * C floats + 16."""
    from realvsr_amd import _lib
    nbytes = _lib.lib().rvsr_bn_workspace_bytes(B, C, HW)
    q, r = divmod(nbytes - 12 * C - 16, 16 * C)
    assert r == 0
    return q


@pytest.mark.parametrize('name', list(GR.BN_CASES))
def test_bn_case_runs_the_slicing_it_is_named_for(name):
    B, C, H, W, NP, _, _ = GR.BN_CASES[name]
    n = B * H * W
    assert _np_of_library(B, C, H * W) == NP == min(64, -(-n // 8192))
    if 'ragged' in name:
        assert NP > 1 and n % NP != 0
        # at least one inner boundary lies inside a plane, and the slices cross batch elements unless there is only one
        assert any((n * q // NP) % (H * W) != 0 for q in range(1, NP)) and (B == 1 or n // NP > H * W)
    if 'cap64' in name:
        assert -(-n // 8192) > 64 and n > 64 * 8192
    assert B * C * H * W <= 1100000      # "about 1 M floats" at the most
    assert (name == 'n2') == (n == 2) and (name != 'n8193' or (n * 1 // 2, n - n * 1 // 2) == (4096, 4097))
    assert ('c' + str(C) in name.split('_')) == (C in (1, 65, 130))


def test_bn_case_list_covers_the_thresholds():
    ns = {B * H * W for B, C, H, W, *_ in GR.BN_CASES.values()}
    cs = {c[1] for c in GR.BN_CASES.values()}
    assert {2, 6, 8192, 8193, 8405} <= ns and {1, 65, 130} <= cs
    assert {c[4] for c in GR.BN_CASES.values()} >= {1, 2, 3, 64}


@pytest.mark.parametrize('name', list(GR.BN_CASES))
def test_kink_rule_zeroes_at_most_one_percent(name):
    ref = GR.bn_case_reference(name)
    assert ref['share'] <= 0.01, ref['share']
    assert bool((ref['gy'][ref['v'].abs() <= GR.KINK] == 0).all())
    for k in GR.BN_TENSORS:
        assert torch.isfinite(ref[k]).all()


@pytest.mark.parametrize('name', [n for n in GR.BN_CASES if n.endswith('_stats')])
def test_statistics_term_is_visible(name):
    ref = GR.bn_case_reference(name)
    stat, gx = ref['stat'].abs().max().item(), ref['gx'].abs().max().item()
    print('%s: max |statistics part| %.3e, max |gx| %.3e' % (name, stat, gx))
    assert stat >= 0.2 * gx
    # both terms on their own: mean(gz) and mean(gz * xhat) are O(1)
    gz, xhat = ref['gz'], (GR.bn_inputs(name)['x'].double() - ref['mean'].view(1, -1, 1, 1)) * ref['invstd'].view(1, -1, 1, 1)
    assert gz.mean((0, 2, 3)).abs().max().item() > 0.1 and (gz * xhat).mean((0, 2, 3)).abs().max().item() > 0.1


def test_stats_cases_cover_what_the_issue_names():
    names = [n for n in GR.BN_CASES if n.endswith('_stats')]
    assert 'n6_stats' in names and any('cap64' in n for n in names) and sum('ragged_np' in n for n in names) >= 1


def test_ill_conditioned_cases_are_what_they_say():
    x = GR.bn_inputs('ill_const')['x']
    assert bool((x[:, 1] == x[0, 1, 0, 0]).all()) and x[:, 0].std().item() > 1.0
    assert GR.bn_case_reference('ill_const')['invstd'][1].item() == pytest.approx(1e-5 ** -0.5, rel=1e-9)
    x = GR.bn_inputs('ill_mean1e3')['x']
    assert x.mean((0, 2, 3)).abs().min().item() >= 990 and 0.5 < x.std((0, 2, 3)).min().item() < 2.0
    x = GR.bn_inputs('ill_spread1e-4')['x']
    assert (x.mean((0, 2, 3)) - 2).abs().max().item() < 1e-4 and 3e-5 < x.std((0, 2, 3)).max().item() < 3e-4
    for name in GR.ILL_CONDITIONED + ('n2',):
        assert GR.BN_CASES[name][:4] == ((2, 4, 5, 7) if name != 'n2' else (2, 3, 1, 1))
        y = GR.bn_case_yardstick(name)
        print(name, {k: '%.2e' % v for k, v in y.items()})
        assert all(v == v and v < float('inf') for v in y.values())


@pytest.mark.parametrize('name', ['saturated', 'rel_saturated'])
def test_saturated_cases_reach_exact_zero_and_one(name):
    a, b = GR.crit_inputs(name)
    zero, one = GR.saturation_masks(a, b)
    assert int(zero.sum()) >= 4 and int(one.sum()) >= 6         # -200, -1e4 twice each; +30, +200, +1e4 twice each
    for v in GR.SATURATED_LOGITS:
        assert int((a == v).sum()) == 2
    # the ordinary logits stay well inside: nothing else is near a threshold of exactness
    z = a.double() - (0.0 if b is None else b.double().mean())
    assert bool(((z.abs() < 12) | (z.abs() > 25)).all())
    for t in GR.CRIT_TARGETS:
        ref = GR.crit_reference(a, b, t)
        assert all(torch.isfinite(ref[k]).all() for k in ('loss', 'ga'))


def test_tail_case_is_in_the_subnormal_band():
    a, b = GR.crit_inputs('rel_tail')
    assert b.double().mean().item() == 0.0
    s = torch.sigmoid(a.double())
    assert bool((s < 1.1754944e-38).all()) and bool((s > 1e4 * 1.4e-45).all())     # subnormal, yet 1e4 steps above zero: 2e-5 resolves
    assert bool(torch.isinf(torch.exp(-a))) if a.numel() == 1 else bool(torch.isinf(torch.exp(-a)).all())    # exp(89) overflows float32


def test_criterion_case_sizes():
    sizes = {n: (torch.Size(c[0]).numel(), None if c[1] is None else torch.Size(c[1]).numel()) for n, c in GR.CRIT_CASES.items()}
    assert {sizes[n][0] for n in sizes if not n.startswith('rel_')} >= {1, 1023, 1024, 1025, 3 * 1024 + 7}
    assert sizes['rel_nb1_na1025'] == (1025, 1) and sizes['rel_nb1025_na7'] == (7, 1025)
    assert {sizes[n] for n in sizes if n.startswith('rel_n')} >= {(k, k) for k in (1, 1023, 1024, 1025, 3079)}


@pytest.mark.parametrize('cfg', [dict(), dict(affine=False), dict(track_running_stats=False), dict(momentum=0.3, eps=1e-3), dict(train=False),
                                 dict(train=False, track_running_stats=False)], ids=str)
def test_bn_reference_is_the_module(cfg):
    """The functional float64 reference against nn.BatchNorm2d(...).double() -> LeakyReLU, buffers included, to 1e-12."""
    cfg = dict(cfg)
    train = cfg.pop('train', True)
    t = GR.bn_raw(3, 5, 4, 6, 77)
    affine, track = cfg.get('affine', True), cfg.get('track_running_stats', True)
    mod = nn.BatchNorm2d(5, **cfg).double().train(train)
    with torch.no_grad():
        if affine:
            mod.weight.copy_(t['weight'])
            mod.bias.copy_(t['bias'])
        if track:
            mod.running_mean.copy_(t['running_mean'])
            mod.running_var.copy_(t['running_var'])
    ref = GR.bn_reference(t['x'], t['gy'], t['weight'] if affine else None, t['bias'] if affine else None,
                          t['running_mean'] if track else None, t['running_var'] if track else None, train,
                          cfg.get('momentum', 0.1), cfg.get('eps', 1e-5), 0.2)
    xm = t['x'].double().requires_grad_(True)
    ym = nn.LeakyReLU(0.2)(mod(xm))
    ym.backward(ref['gy'].double())
    close = lambda a, b: (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item())   # noqa: E731
    assert close(ref['y'], ym.detach()) and close(ref['gx'], xm.grad)
    if affine:
        assert close(ref['ggamma'], mod.weight.grad) and close(ref['gbeta'], mod.bias.grad)
    else:
        assert ref['ggamma'] is None and ref['gbeta'] is None
    if track:
        assert close(ref['running_mean'], mod.running_mean) and close(ref['running_var'], mod.running_var)
        assert int(mod.num_batches_tracked) == int(train)
        assert torch.equal(ref['running_mean'], t['running_mean'].double()) == (not train)
    else:
        assert ref['running_mean'] is None and mod.running_mean is None
    # the statistics part: zero exactly when the running statistics normalise
    assert (ref['stat'].abs().max().item() < 1e-12) == (not train and track)
    # k1 * gz + stat restates gx with the float64 quantities; lrelu' from v agrees with lrelu' from y
    assert close(ref['k1'] * ref['gz'] + ref['stat'], xm.grad)
    assert torch.equal(ref['v'] > 0, ref['y'] > 0)


def test_three_inputs_reference_is_the_module():
    """One nn.BatchNorm2d(...).double() applied to the three inputs, one backward: outputs, summed parameter gradients, buffers."""
    first, xs, refs, rm, rv = GR.three_inputs_reference()
    assert [tuple(x.shape) for x in xs] == list(GR.THREE) and all(r['share'] <= 0.01 for r in refs)
    mod = nn.BatchNorm2d(6).double()
    with torch.no_grad():
        for p, k in ((mod.weight, 'weight'), (mod.bias, 'bias'), (mod.running_mean, 'running_mean'), (mod.running_var, 'running_var')):
            p.copy_(first[k])
    xm = [x.double().requires_grad_(True) for x in xs]
    ys = [F.leaky_relu(mod(x), 0.2) for x in xm]
    torch.autograd.backward(ys, [r['gy'].double() for r in refs])
    for x, y, r in zip(xm, ys, refs):
        assert (y.detach() - r['y']).abs().max().item() < 1e-12 and (x.grad - r['gx']).abs().max().item() < 1e-12
        assert r['stat'].abs().max().item() >= 0.2 * r['gx'].abs().max().item()
    assert (mod.running_mean - rm).abs().max().item() < 1e-12 and (mod.running_var - rv).abs().max().item() < 1e-12
    assert (mod.weight.grad - sum(r['ggamma'] for r in refs)).abs().max().item() < 1e-12
    assert (mod.bias.grad - sum(r['gbeta'] for r in refs)).abs().max().item() < 1e-12
    assert int(mod.num_batches_tracked) == 3


@pytest.mark.parametrize('target', GR.CRIT_TARGETS)
@pytest.mark.parametrize('name', ['n1025', 'rel_nb1025_na7', 'rel_saturated'])
def test_criterion_reference_is_the_module(name, target):
    a, b = GR.crit_inputs(name)
    ref = GR.crit_reference(a, b, target, g=0.7)
    ar = a.double().requires_grad_(True)
    br = None if b is None else b.double().requires_grad_(True)
    z = ar if br is None else ar - torch.mean(br)
    loss = nn.BCEWithLogitsLoss()(z, torch.empty_like(z).fill_(target))
    (0.7 * loss).backward()
    assert abs(ref['loss'].item() - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
    assert (ref['ga'] - ar.grad).abs().max().item() <= 1e-12
    if b is not None:
        assert (ref['gb'] - br.grad).abs().max().item() <= 1e-12
    # and the formula itself: mean(max(z, 0) - z t + log1p(exp(-|z|)))
    zd = z.detach()
    want = (zd.clamp(min=0) - zd * target + torch.log1p(torch.exp(-zd.abs()))).mean()
    assert abs(want.item() - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))


def test_yardstick_bound_rule():
    ref = torch.tensor([1.0, -4.0])
    assert GR.yardstick_bound(ref, 0.0) == 2e-5 * 4.0
    assert GR.yardstick_bound(ref, 1e-3) == 8e-3
