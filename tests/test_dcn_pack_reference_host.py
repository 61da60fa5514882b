"""tests/dcn_pack_reference.py (the float64 reference of the fused DCN pack node) against tests/dcn_composition.py, the oracle-independent
construction for spatially constant offsets: chunk + sigmoid + operator + activation + autograd agree to 1e-11 with each activation,
forward and every gradient (grad_offset as per-(group, tap) sums over the pixels, d/d logit for the mask part).  No GPU."""
import pytest
import torch

import dcn_composition as DC
import dcn_pack_reference as DR
from conftest import rel_err
from test_oracle_dcn import COMPOSITION_CASES

TOL = 1e-11
SLOPE = 0.1


@pytest.mark.parametrize('act', DR.ACTS)
@pytest.mark.parametrize('case', COMPOSITION_CASES[:2], ids=lambda c: '-'.join(str(v) for v in c))
def test_reference_matches_constant_offset_composition(case, act):
    B, C, Co, dg, H, W, seed = case
    x, dyx, _, w, b, gout = DC.make_case(B, C, Co, dg, H, W, seed, dtype=torch.float32, kind='mixed')
    logits = torch.randn(B, 9 * dg, H, W, generator=torch.Generator().manual_seed(seed + 100))
    om = torch.cat([DC.offset_field(dyx, B, H, W), logits], 1)
    r = DR.reference(x, om, w, b, 1, 1, 1, dg, act, SLOPE, gout)
    assert r['share'] <= DR.KINK_SHARE_MAX and (act != 'none' or bool((r['gout'] == gout).all()))
    # the construction: the same chunk / sigmoid / activation around constant_offset_dcn, float64 autograd, the reference's zeroed gout
    xl, dl, ll, wl, bl = [t.double().clone().requires_grad_(True) for t in (x, dyx, logits, w, b)]
    z = DC.constant_offset_dcn(xl, dl, torch.sigmoid(ll), wl, bl, pad=1, dg=dg)
    out = DR.activation(z, act, SLOPE)
    out.backward(r['gout'].double())
    assert act == 'none' or bool((r['gout'][z.detach().abs() <= DR.KINK] == 0).all())
    errs = dict(z=rel_err(r['z'], z.detach()), out=rel_err(r['out'], out.detach()), gx=rel_err(r['gx'], xl.grad), gw=rel_err(r['gw'], wl.grad),
                gb=rel_err(r['gb'], bl.grad), glogit=rel_err(r['gom'][:, 18 * dg:], ll.grad))
    ok = DC.offset_grad_comparable(dyx)[:, :, None].double()   # (all but taps that sit exactly on the -1 boundary)
    errs['goff sums'] = rel_err(DC.offset_grad_sums(r['gom'][:, :18 * dg], dg) * ok, dl.grad * ok)
    print(case, act, 'kink share %.4f' % r['share'], ' '.join('%s %.1e' % kv for kv in errs.items()))
    assert all(e <= TOL for e in errs.values()), errs


def test_reference_without_bias_and_kink_share():
    """No bias: no bias gradient; the zeroed share is what the mask of |z| <= KINK says, and a case beyond the cap is visible as such."""
    B, C, Co, dg, H, W, seed = COMPOSITION_CASES[0]
    x, dyx, _, w, _, gout = DC.make_case(B, C, Co, dg, H, W, seed, dtype=torch.float32, kind='fractional')
    om = torch.cat([DC.offset_field(dyx, B, H, W), torch.zeros(B, 9 * dg, H, W)], 1)
    r = DR.reference(x, om, w, None, 1, 1, 1, dg, 'lrelu', SLOPE, gout)
    assert r['gb'] is None
    assert abs(r['share'] - (r['z'].abs() <= DR.KINK).double().mean().item()) < 1e-15
    tiny = DR.reference(x * 1e-4, om, w, None, 1, 1, 1, dg, 'relu', SLOPE, gout)   # |z| ~ 1e-4: mostly inside the kink band
    assert tiny['share'] > DR.KINK_SHARE_MAX
