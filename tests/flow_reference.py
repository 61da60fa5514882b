"""Float64 restatements, by direct indexing, of SpyNet's resampling operators (csrc/flow_kernels.hip): the flow warp with both
gradients, the 2 x 2 average pool and the x2 align_corners=True bilinear upsample with theirs.  No autograd, no grid_sample, no
interpolate: tests/test_flow_reference_host.py holds them to torch's own operators on the CPU, tests/test_gpu_flow.py holds the kernels
to them."""
import torch


WARP_MODES = [('bilinear', 'zeros'), ('bilinear', 'border'), ('nearest', 'zeros'), ('nearest', 'border')]
WARP_SHAPES = [(1, 1, 1, 1), (1, 2, 1, 5), (2, 3, 5, 1), (2, 3, 7, 9), (1, 3, 16, 24), (1, 2, 130, 70)]
POOL_SHAPES = [(1, 1, 1, 1), (2, 3, 2, 3), (1, 2, 5, 9), (2, 3, 7, 9), (1, 2, 258, 130)]


def make_flow(kind, B, H, W, gen):
    """Test flows (B, H, W, 2), float32.  'zero'; 'shift': one integer displacement per batch element; 'random': N(0, 2 px) with the
    fractional part of every component pushed into [0.05, 0.45] or [0.55, 0.95], away from the integers (where floor() and the flow
    gradient jump) and from the halves (where nearest rounds the other way); 'far': beyond +-(W + 3), every tap outside the frame."""
    if kind == 'zero':
        return torch.zeros(B, H, W, 2)
    if kind == 'shift':
        return torch.randint(-3, 4, (B, 1, 1, 2), generator=gen).float().expand(B, H, W, 2).contiguous()
    if kind == 'random':
        f = 2.0 * torch.randn(B, H, W, 2, generator=gen)
        whole, frac = torch.floor(f), f - torch.floor(f)
        frac = torch.where(frac < 0.5, 0.05 + 0.8 * frac, 0.55 + 0.8 * (frac - 0.5))
        return whole + frac
    if kind == 'far':
        sign = torch.where(torch.rand(B, H, W, 2, generator=gen) < 0.5, -1.0, 1.0)
        return sign * (max(H, W) + 3.25 + 5.0 * torch.rand(B, H, W, 2, generator=gen))
    raise ValueError(kind)


def _taps(flow, H, W, interp, padding):
    """Per pixel: the taps [(row index, column index, weight, in the frame)] and d coordinate / d flow for x and y."""
    # the coordinate pixel + flow is formed in the flow's own precision (the operator's definition: one float32 addition on the device),
    # everything after it in float64
    ys, xs = torch.meshgrid(torch.arange(H, dtype=flow.dtype), torch.arange(W, dtype=flow.dtype), indexing='ij')
    cx = (xs + flow[..., 0]).double() if W > 1 else torch.zeros(flow.shape[:-1], dtype=torch.float64)
    cy = (ys + flow[..., 1]).double() if H > 1 else torch.zeros(flow.shape[:-1], dtype=torch.float64)
    dx = torch.full_like(cx, 1.0 if W > 1 else 0.0)
    dy = torch.full_like(cy, 1.0 if H > 1 else 0.0)
    if padding == 'border':
        # grid_sample's clip: the edges themselves count as clipped (the value is constant from there on outwards)
        dx = dx * ((cx > 0) & (cx < W - 1))
        dy = dy * ((cy > 0) & (cy < H - 1))
        cx, cy = cx.clamp(0, W - 1), cy.clamp(0, H - 1)
    elif padding != 'zeros':
        raise NotImplementedError(padding)
    if interp == 'nearest':
        cols, rows = [(torch.round(cx), torch.ones_like(cx))], [(torch.round(cy), torch.ones_like(cy))]   # (round half to even)
    elif interp == 'bilinear':
        x0, y0 = torch.floor(cx), torch.floor(cy)
        cols, rows = [(x0, x0 + 1 - cx), (x0 + 1, cx - x0)], [(y0, y0 + 1 - cy), (y0 + 1, cy - y0)]
    else:
        raise NotImplementedError(interp)
    taps = []
    for r, wr in rows:
        for c, wc in cols:
            ok = (r >= 0) & (r <= H - 1) & (c >= 0) & (c <= W - 1)
            taps.append((r.clamp(0, H - 1).long(), c.clamp(0, W - 1).long(), wr, wc, ok))
    return taps, dx, dy


def warp(x, flow, interp='bilinear', padding='zeros'):
    """x (B, C, H, W), flow (B, H, W, 2) in pixels, x first -> the image sampled at pixel + flow (float64)."""
    B, C, H, W = x.shape
    xd = x.double()
    b = torch.arange(B).view(B, 1, 1, 1)
    c = torch.arange(C).view(1, C, 1, 1)
    out = torch.zeros(B, C, H, W, dtype=torch.float64)
    for r, q, wr, wc, ok in _taps(flow, H, W, interp, padding)[0]:
        out += xd[b, c, r.unsqueeze(1), q.unsqueeze(1)] * (wr * wc * ok).unsqueeze(1)
    return out


def warp_backward(x, flow, gout, interp='bilinear', padding='zeros'):
    """-> (gx (B, C, H, W), gflow (B, H, W, 2)) of `warp` for the output gradient gout (float64)."""
    B, C, H, W = x.shape
    xd, g = x.double(), gout.double()
    taps, dx, dy = _taps(flow, H, W, interp, padding)
    gx = torch.zeros(B * C * H * W, dtype=torch.float64)
    plane = (torch.arange(B).view(B, 1, 1, 1) * C + torch.arange(C).view(1, C, 1, 1)) * (H * W)
    b = torch.arange(B).view(B, 1, 1, 1)
    c = torch.arange(C).view(1, C, 1, 1)
    gcx, gcy = torch.zeros(B, H, W, dtype=torch.float64), torch.zeros(B, H, W, dtype=torch.float64)
    for r, q, wr, wc, ok in taps:
        gx.index_add_(0, (plane + (r * W + q).unsqueeze(1)).reshape(-1), (g * (wr * wc * ok).unsqueeze(1)).reshape(-1))
    if interp == 'bilinear':
        # value = sum over rows r and columns q of x[r, q] wr wc: d wr / d cy = -1 for the upper row, +1 for the lower, likewise the columns
        signs = [(-1, -1), (-1, 1), (1, -1), (1, 1)]   # (row, column) of taps in the order _taps built them
        for (r, q, wr, wc, ok), (sr, sc) in zip(taps, signs):
            v = xd[b, c, r.unsqueeze(1), q.unsqueeze(1)] * ok.unsqueeze(1)
            gcx += (g * v * (sc * wr).unsqueeze(1)).sum(1)
            gcy += (g * v * (sr * wc).unsqueeze(1)).sum(1)
    return gx.view(B, C, H, W), torch.stack([gcx * dx, gcy * dy], -1)


def avg_pool2(x):
    H, W = x.shape[-2:]
    xd = x.double()[..., :H // 2 * 2, :W // 2 * 2]
    return (xd[..., 0::2, 0::2] + xd[..., 0::2, 1::2] + xd[..., 1::2, 0::2] + xd[..., 1::2, 1::2]) / 4


def avg_pool2_backward(x, gout):
    H, W = x.shape[-2:]
    gin = torch.zeros(x.shape, dtype=torch.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            gin[..., dy:H // 2 * 2:2, dx:W // 2 * 2:2] = gout.double() / 4
    return gin


def _ac_matrix(n):
    """(2n, n): row d holds the weights of destination d on the sources; source coordinate d (n - 1) / (2n - 1), 0 for n == 1."""
    m = torch.zeros(2 * n, n, dtype=torch.float64)
    for d in range(2 * n):
        s = d * (n - 1) / (2 * n - 1) if n > 1 else 0.0
        i0 = min(int(s), n - 1)
        i1 = min(i0 + 1, n - 1)
        m[d, i0] += 1.0 - (s - i0)
        m[d, i1] += s - i0
    return m


def upsample2_ac(x, scale=1.0):
    H, W = x.shape[-2:]
    return scale * (_ac_matrix(H) @ x.double() @ _ac_matrix(W).t())


def upsample2_ac_backward(x, gout, scale=1.0):
    H, W = x.shape[-2:]
    return scale * (_ac_matrix(H).t() @ gout.double() @ _ac_matrix(W))
