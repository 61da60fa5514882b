"""The float64 references of the frame-major nodes (tests/frame_reference.py) against the torch modules they stand for, and the tap
table of functional.conv3d_frames against its definition.  No GPU."""
import torch
import torch.nn as nn

import frame_reference as FR


def _g(seed):
    return torch.Generator().manual_seed(seed)


def test_conv3d_frames_ref_is_nn_conv3d():
    """Over the full frame range, and on every partial range the matching slice of it; k = 3 and k = 1, with and without a bias."""
    g = _g(1)
    for T, B, Ci, Co, H, W, k, bias in ((1, 1, 3, 4, 5, 7, 3, True), (2, 2, 4, 3, 4, 6, 3, True), (5, 1, 3, 5, 5, 7, 3, False),
                                        (4, 2, 4, 4, 3, 5, 1, True)):
        conv = nn.Conv3d(Ci, Co, (3, k, k), padding=(1, k // 2, k // 2), bias=bias).double()
        x = torch.randn(T, B, Ci, H, W, generator=g, dtype=torch.float64)
        with torch.no_grad():
            want = conv(x.permute(1, 2, 0, 3, 4)).permute(2, 0, 1, 3, 4)
            assert tuple(want.shape) == (T, B, Co, H, W)
            assert torch.equal(FR.conv3d_frames_ref(x, conv.weight, conv.bias), want)
            for f0, f1 in ((a, b) for a in range(T) for b in range(a + 1, T + 1)):
                res = torch.randn(f1 - f0, B, Co, H, W, generator=g, dtype=torch.float64)
                assert torch.equal(FR.conv3d_frames_ref(x, conv.weight, conv.bias, None, f0, f1), want[f0:f1])
                assert torch.equal(FR.conv3d_frames_ref(x, conv.weight, conv.bias, res, f0, f1), want[f0:f1] + res)


def test_c3_taps_are_the_definition():
    """_c3_taps(T, f0, f1) for every 0 <= f0 < f1 <= T <= 6: each tap's (first input frame, frames, first output frame) is what
    'output frame t reads input frame t + dt - 1 if it exists' gives, a tap that meets nothing is absent, and the centre tap comes
    first and covers every output frame (it writes; the others accumulate)."""
    from realvsr_amd import functional as RF
    n = 0
    for T in range(1, 7):
        for f0, f1 in ((a, b) for a in range(T) for b in range(a + 1, T + 1)):
            taps = RF._c3_taps(T, f0, f1)
            want = FR.c3_taps_by_definition(T, f0, f1)
            assert len(taps) == len({t[0] for t in taps}), (T, f0, f1, taps)
            assert {t[0]: tuple(t[1:]) for t in taps} == want, (T, f0, f1, taps, want)
            assert taps[0] == (1, f0, f1 - f0, 0), (T, f0, f1, taps)
            n += 1
    assert n == sum(T * (T + 1) // 2 for T in range(1, 7))
    # the edges the network fixtures never meet: a tap that meets no frame, an outer tap cut at either end
    assert [t[0] for t in RF._c3_taps(1, 0, 1)] == [1]
    assert RF._c3_taps(2, 0, 2) == [(1, 0, 2, 0), (0, 0, 1, 1), (2, 1, 1, 0)]
    assert RF._c3_taps(5, 4, 5) == [(1, 4, 1, 0), (0, 3, 1, 0)]


def test_conv_transpose1x1_ref_is_the_modules():
    g = _g(2)
    for lead, Ci, Co, H, W in (((3, 2), 4, 6, 5, 7), ((2,), 6, 4, 3, 4)):
        x = torch.randn(*lead, Ci, H, W, generator=g, dtype=torch.float64)
        m3, m2 = nn.ConvTranspose3d(Ci, Co, 1).double(), nn.ConvTranspose2d(Ci, Co, 1).double()
        with torch.no_grad():
            x4 = x.reshape(-1, Ci, H, W)
            assert torch.equal(FR.conv_transpose1x1_ref(x, m2.weight, m2.bias), m2(x4).reshape(*lead, Co, H, W))
            want3 = m3(x4.unsqueeze(2)).squeeze(2).reshape(*lead, Co, H, W)
            assert torch.equal(FR.conv_transpose1x1_ref(x, m3.weight, m3.bias), want3)
            # (Ci, Co), not (Co, Ci): out[co] = sum_ci w[ci, co] * x[ci]
            einsum = torch.einsum('io,...ihw->...ohw', m3.weight.reshape(Ci, Co), x) + m3.bias.view(Co, 1, 1)
            assert torch.allclose(want3, einsum, rtol=0, atol=1e-12)


def test_tsa_block_ref_is_the_batch_major_formulation():
    g = _g(3)
    for N, center, B, C, H, W in ((1, 0, 1, 4, 5, 7), (3, 1, 2, 4, 4, 6), (5, 0, 1, 3, 5, 7), (5, 4, 2, 4, 3, 5)):
        a = torch.randn(N, B, C, H, W, generator=g, dtype=torch.float64)
        w1, w2 = (torch.randn(C, C, 3, 3, generator=g, dtype=torch.float64) / (3.0 * C) for _ in range(2))
        b1, b2 = (torch.randn(C, generator=g, dtype=torch.float64) * 0.1 for _ in range(2))
        got = FR.tsa_block_ref(a, center, w1, b1, w2, b2)
        want = FR.tsa_block_ref_batch_major(a.transpose(0, 1).contiguous(), center, w1, b1, w2, b2)
        assert tuple(got.shape) == (B, N * C, H, W)
        assert torch.allclose(got, want, rtol=0, atol=1e-13)
        if N > 1:   # the centre matters: another one gives another result
            other = FR.tsa_block_ref(a, (center + 1) % N, w1, b1, w2, b2)
            assert (other - got).abs().max().item() > 1e-6
