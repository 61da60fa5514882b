"""The three facts behind the bit-for-bit pins of the speed modes (tests/modes_reference.py, tests/test_gpu_modes_definition.py), on the
CPU: rounding to bf16 is idempotent; a product of two bf16 values is exact in f32; with integer sample positions and power-of-two masks
the sampled column of the deformable convolution is a bf16 value wherever x is."""
import torch

import modes_reference as MR


def _wide_range_values(n, generator):
    """f32 values whose exponents cover the bf16 range from its denormals (below 2^-126) up to 2^60, both signs, zeros mixed in."""
    mant = 1.0 + torch.rand(n, generator=generator, dtype=torch.float64)
    expo = torch.randint(-133, 61, (n,), generator=generator).double()
    sign = torch.randint(0, 2, (n,), generator=generator).double() * 2 - 1
    v = (sign * mant * torch.exp2(expo)).float()
    v[torch.rand(n, generator=generator) < 0.02] = 0.0
    return v


def test_bf16_round_is_idempotent_and_nearest_even():
    g = torch.Generator().manual_seed(1)
    v = torch.cat([_wide_range_values(1 << 20, g), torch.randn(1 << 20, generator=g)])
    r = MR.bf16_round(v)
    assert r.dtype == torch.float32
    assert torch.equal(MR.bf16_round(r), r)
    # a bf16 value: the low 16 bits of the f32 pattern are zero
    assert bool(((r.view(torch.int32) & 0xFFFF) == 0).all())
    # nearest: within half a unit of the 8-bit significand (normal range), ties to even
    normal = v.abs() >= 2.0 ** -126
    assert bool(((r - v).abs()[normal] <= v.abs()[normal] * 2.0 ** -8).all())
    ties = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8)])
    assert MR.bf16_round(ties).tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0]


def test_the_f32_product_of_two_bf16_values_is_exact():
    """8-bit significands multiply to 16 bits: the f32 product is the float64 product wherever it does not underflow past f32's last
    denormal bit.  Four million pairs, zeros and denormal-range operands and products included."""
    g = torch.Generator().manual_seed(2)
    n = 1 << 22
    a, b = MR.bf16_round(_wide_range_values(n, g)), MR.bf16_round(_wide_range_values(n, g))
    tiny = MR.bf16_round(torch.tensor([2.0 ** -133, 1.5 * 2.0 ** -130, -(2.0 ** -127), 0.0, -0.0]))   # bf16 denormals and zeros
    a = torch.cat([a, tiny.repeat_interleave(5), torch.randn(1 << 16, generator=g).to(torch.bfloat16).float()])
    b = torch.cat([b, (tiny * 2.0 ** 120).repeat(5), torch.randn(1 << 16, generator=g).to(torch.bfloat16).float()])
    exact = a.double() * b.double()
    got = (a * b).double()
    assert bool(torch.isfinite(got).all())
    representable = (exact * 2.0 ** 149) == (exact * 2.0 ** 149).round()    # no bit below 2^-149
    assert int((exact.abs() >= 2.0 ** -126).sum()) > n // 2                      # (most pairs are ordinary products ...)
    assert int(((exact != 0) & (exact.abs() < 2.0 ** -126)).sum()) > 1000       # (... and denormal-range products are there)
    assert bool(representable[(exact == 0) | (exact.abs() >= 2.0 ** -126)].all())   # every zero or normal-range product has its 16 bits
    assert torch.equal(got[representable], exact[representable])
    # the operands the GPU tests use are O(1): exact without exception
    x, w = MR.bf16_round(torch.randn(1 << 20, generator=g)), MR.bf16_round(torch.randn(1 << 20, generator=g) / 24)
    assert torch.equal((x * w).double(), x.double() * w.double())


def test_generated_fields():
    g = torch.Generator().manual_seed(3)
    for reach in (0, 2, 5, 12):
        off = MR.integer_offsets(2, 4, 9, 33, reach, g)
        assert off.shape == (2, 72, 9, 33) and off.dtype == torch.float32
        assert torch.equal(off, off.round()) and float(off.abs().max()) == reach
        y, x = MR.sample_positions(off, 4)
        outside = (y < 0) | (y >= 9) | (x < 0) | (x >= 33)
        assert bool(outside.any()) and bool((~outside).any())
    m = MR.pow2_masks(2, 4, 9, 33, g)
    assert m.shape == (2, 36, 9, 33) and sorted(m.unique().tolist()) == [0.25, 0.5, 1.0]
    # a different field per pixel, tap and group
    off = MR.integer_offsets(1, 2, 8, 8, 5, g)
    assert len(off.view(36, 64).unique(dim=0)) == 36 and len(off.view(36, 64).t().unique(dim=0)) > 60


def test_sampled_columns_of_bf16_inputs_are_bf16_values():
    """The float64 column matrix of the oracle's im2col (oracle/dcn_oracle.py) for bf16-valued x, integer offsets up to a reach beyond
    the frame and masks in {1, 1/2, 1/4}: equal to the plain gather mask * x[position] for in-frame samples, 0 for the others, and
    every entry a bf16 value."""
    from oracle import dcn_oracle as O
    for (B, C, dg, H, W, reach, seed) in ((2, 16, 2, 9, 33, 2, 4), (1, 16, 1, 7, 12, 5, 5), (1, 8, 1, 6, 10, 12, 6)):
        g = torch.Generator().manual_seed(seed)
        x = MR.bf16_round(torch.randn(B, C, H, W, generator=g)).double()
        off = MR.integer_offsets(B, dg, H, W, reach, g)
        mask = MR.pow2_masks(B, dg, H, W, g)
        want, inside = MR.gathered_columns(x, off, mask, dg)
        assert bool(inside.any()) and bool((~inside).any())
        assert bool((want[~inside] == 0).all()) and bool((want[inside] != 0).any())
        for b in range(B):
            col = O.im2col(x[b], off[b].double(), mask[b].double(), 3, 3, 1, 1, 1, dg, H, W)
            assert torch.equal(col, want[b])
            assert torch.equal(MR.bf16_round(col).double(), col)
        # and it is the unrounded x that would break it: the columns of a plain f32 x are not bf16 values
        xf = torch.randn(B, C, H, W, generator=g)
        colf, _ = MR.gathered_columns(xf, off, mask, dg)
        assert not torch.equal(MR.bf16_round(colf), colf)
    # fractional offsets mix corners: not bf16 values even for a bf16 x (why the 'bf16' rows need the integer fields)
    g = torch.Generator().manual_seed(7)
    x = MR.bf16_round(torch.randn(8, 6, 10, generator=g)).double()
    col = O.im2col(x, torch.rand(18, 6, 10, generator=g).double() * 2 - 1, torch.ones(9, 6, 10).double(), 3, 3, 1, 1, 1, 1, 6, 10)
    assert not torch.equal(MR.bf16_round(col).double(), col)
