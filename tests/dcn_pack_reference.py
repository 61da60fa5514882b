"""The fused DCN pack node (realvsr_amd.functional.dcn_pack) in float64 (test infrastructure): chunk of the raw conv_offset_mask output
into 18 dg offset channels and 9 dg mask logits, torch.sigmoid, oracle.dcn_oracle.modulated_deform_conv, the activation, float64
autograd.  Plain helper of tests/test_gpu_dcn_pack_node.py, held against tests/dcn_composition.py by test_dcn_pack_reference_host.py.

Inputs are GENERATED in float32 and upcast here, so that the floor of a sampling position cannot differ between this side and the
kernels.  Kink rule (as tests/test_gpu_conv.py): where the exact pre-activation z is within KINK of zero the activation's derivative
legitimately depends on the last bits of the GEMM, so `gout` is zeroed there -- on both sides, the caller runs the node on the returned
gout -- and the zeroed share is returned: a case whose share exceeds KINK_SHARE_MAX tests too little and fails."""
import torch
import torch.nn.functional as F

KINK = 1e-3
KINK_SHARE_MAX = 0.01
ACTS = ('none', 'relu', 'lrelu')


def activation(z, act, slope):
    if act == 'none':
        return z
    if act == 'relu':
        return F.relu(z)
    if act == 'lrelu':
        return F.leaky_relu(z, slope)
    raise ValueError(act)


def reference(x, om, w, b, stride, pad, dil, dg, act, slope, gout):
    """-> dict(z, out, gout (float32, zeroed at the kink), share, gx, gom, gw, gb (None without a bias)), float64 but gout."""
    from oracle.dcn_oracle import modulated_deform_conv
    assert all(t is None or t.dtype == torch.float32 for t in (x, om, w, b, gout)), 'generate in float32: see the module docstring'
    leaves = [None if t is None else t.detach().double().clone().requires_grad_(True) for t in (x, om, w, b)]
    xr, omr, wr, br = leaves
    z = modulated_deform_conv(xr, omr[:, :18 * dg], torch.sigmoid(omr[:, 18 * dg:]), wr, br, stride, pad, dil, 1, dg)
    out = activation(z, act, slope)
    if act == 'none':
        g, share = gout.clone(), 0.0
    else:
        keep = z.detach().abs() > KINK
        g, share = gout * keep.float(), 1.0 - keep.double().mean().item()
    out.backward(g.double())
    return dict(z=z.detach(), out=out.detach(), gout=g, share=share, gx=xr.grad, gom=omr.grad, gw=wr.grad, gb=None if br is None else br.grad)
