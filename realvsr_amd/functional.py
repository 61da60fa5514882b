"""Autograd glue between PyTorch tensors and the C ABI of librealvsr_hip.so.

PyTorch is used for device memory, streams and the autograd graph only; every FLOP of the hot
path runs in the HIP kernels (realvsr_amd/csrc).  Each ``Function`` below wraps one fused
operator; CPU tensors are refused (NotImplementedError, like the reference's operator:
codes/models/archs/dcn/deform_conv.py:109-110,124-125).
"""
import functools

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import _p, _stream
from .caches import DcnOffsetStats, PackedWeights, dcn_offset_stats, packed_weights   # noqa: F401  (part of this module's surface)

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
ACT_MASK = 3   # rvsr_conv2d_forward only: out = conv * act'(residual) (include/realvsr_hip.h); internal to the fused backward nodes


def _need_cuda(*ts, any_float=False):
    """any_float: the deformable operators also take f64 / f16 tensors (their general path), everything else is float32."""
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise NotImplementedError('realvsr_amd operators run on MI355X (HIP) tensors only; got a %s tensor'
                                      % t.device.type)
        if t.dtype != torch.float32 and not (any_float and t.dtype in (torch.float64, torch.float16)):
            raise TypeError('realvsr_amd operators are float32 (like the reference training path); got %s' % t.dtype)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError('realvsr_amd operators need all operands on one device; got %s and %s' % (dev, t.device))


def _c(t):
    return None if t is None else t.contiguous()


_workspaces = {}


def _workspace(nbytes, device):
    """Per-(device, stream) scratch buffer, grown on demand (kernels on one stream are ordered,
    so consecutive operators can share it)."""
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


class GradSink:
    """One gradient buffer for an activation that several fused operators consume.

    Autograd sums the gradients of a tensor with k consumers by k - 1 out-of-place adds (3 passes over the tensor each; the
    40 x 64 x 180 x 320 feature maps of the alignment stage have up to four consumers).  The kernels here can do that
    sum themselves: the DCN backward accumulates atomically into whatever its grad_input buffer holds, and the
    data-gradient convs take a fused residual that may be their own output buffer.  A GradSink is created per forward for such an
    activation and handed to its consumers:
      * a DEPOSITOR (every consumer but the owner) adds its gradient into `buf` in place and returns None to autograd;
      * the OWNER -- the consumer created FIRST in forward, hence run LAST in backward -- adds its own gradient the same way,
        closes the sink and returns the buffer: autograd sees one gradient, no adds, no zero fills.
    If the engine ever ran the owner early, the late depositors see `closed` and return their gradients normally: the
    result is the same sum, just through autograd's adds."""
    __slots__ = ('buf', 'closed', 'shape')

    def __init__(self, shape=None):
        self.buf, self.closed, self.shape = None, False, (tuple(shape) if shape is not None else None)

    def get(self, like):
        """The buffer to accumulate into (zeros on first use), or None once the owner has run."""
        if self.closed:
            return None
        if self.buf is None:
            self.buf = torch.zeros_like(like)
        return self.buf

    def close(self):
        self.closed = True
        buf, self.buf = self.buf, None
        return buf


_ADOPT_FLAT_GRADS = True   # parameter gradients are written in place of the flat buffer (optim.FlatBuffers)
_FUSE_GRAD_MASK = True     # ResBlock backward: relu' of the hidden activation in the epilogue of conv2's data gradient
_FUSE_BCAST_ADDEND = True  # conv_cat_bcast forward: conv_b's partial as a periodic addend of conv_a's epilogue (rvsr_conv2d_forward_addend)


def _pgrad(p, zero=False):
    """Output buffer for the gradient of parameter `p` inside a fused backward.

    When the parameter lives in optim.FlatBuffers, has no gradient yet this step (``p.grad is None`` after
    FlatBuffers.zero_grad) and its home has not been handed out since that zero_grad, the buffer is the parameter's own view of
    the flat gradient buffer: the kernel writes the gradient where the optimizer and the bucketed all-reduce read it, and
    autograd's AccumulateGrad adopts the returned view as ``p.grad`` (no ``grad += new`` kernel, no temporary).  The home is
    handed out ONCE per zero_grad (FlatBuffers.claimed): a parameter used by several fused operators in one backward (a module
    applied twice, shared weights) gets an ordinary temporary for every later use -- AccumulateGrad has not run between the uses,
    so ``p.grad`` is still None and a second hand-out would alias the first gradient.  Gradient accumulation over several
    backward passes and parameters outside FlatBuffers also take the temporary; autograd sums as usual."""
    home = getattr(p, '_rvsr_grad_home', None) if p is not None else None
    if home is not None and p.grad is None and p.dtype == torch.float32 and _ADOPT_FLAT_GRADS:
        buf, off, claimed = home
        if id(p) not in claimed:
            claimed.add(id(p))
            v = buf[off:off + p.numel()].view(p.shape)
            if zero:
                v.zero_()   # (accumulating kernels: do not rely on the caller having used FlatBuffers.zero_grad)
            return v
    return torch.zeros_like(p) if zero else torch.empty_like(p)


_PACK_VERIFY = False   # debug (set it from a test): on a cache hit, pack the weight again and compare (caches.PackedWeights.get)


def invalidate_weight_cache():
    """Call after writing parameters behind torch's version counter (``p.data.copy_``, raw writes into ``FlatBuffers.param``, an EMA
    swap, a custom re-init after FlatAdam was built): forgets every cached bf16 weight image; the next use packs afresh.
    ``load_state_dict`` / in-place ops under ``no_grad`` bump the version and need nothing; ``FlatAdam.step`` re-packs by itself."""
    packed_weights.invalidate()


def _conv(x1, weight, out1, *, what, x2=None, xact=None, xact_slope=0.0, in_mode=0, bias=None, residual=None, out2=None, stride=1,
          transposed=False, act=ACT_NONE, slope=0.0, pixel_shuffle=False, addend_period=0):
    """rvsr_conv2d_forward (include/realvsr_hip.h section 2) on contiguous [..., C, H, W] tensors, which carry the geometry (leading
    dimensions fold into the batch): out1 [, out2] = act(conv(cat(x1, x2)) + bias) [+ residual].  transposed: `weight` is
    (C_in, Co, k, k), used transposed and flipped (a data gradient).  in_mode 2: x1 is stored pixel-shuffled, (B, C1/4, Hs, Ws);
    pixel_shuffle: out1 is (B, Co/4, 2*Hout, 2*Wout).  The weight image comes from the per-step cache when `weight` lives in FlatBuffers
    (or is a cached slice of such a parameter), else it is packed per call into the shared scratch.
    addend_period P > 0 (rvsr_conv2d_forward_addend): `residual` is a (P, Co, Hout, Wout) addend, out1[b] = act(conv + bias +
    residual[b % P]); returns False, having launched nothing, where the library has no such epilogue -- the caller has a plan B."""
    C1, Hs, Ws = x1.shape[-3:]
    if in_mode == 2:
        C1 *= 4
    C2 = 0 if x2 is None else x2.shape[-3]
    Co1, Hout, Wout = out1.shape[-3:]
    B = out1.numel() // (Co1 * Hout * Wout)
    if pixel_shuffle:
        Co1, Hout, Wout = Co1 * 4, Hout // 2, Wout // 2
    Co2 = 0 if out2 is None else out2.shape[-3]
    k = weight.shape[-1]
    w_mode = 1 if transposed else 0
    L = _lib.lib()
    nbytes = L.rvsr_conv2d_forward_workspace_bytes(C1, C2, Co1 + Co2, k)
    call = (_p(x1), C1, _p(x2), C2, _p(xact), xact_slope, in_mode, Hs, Ws, _p(weight), _p(bias), _p(residual), _p(out1), Co1, _p(out2), Co2,
            B, k, stride)
    tail = (act, slope, int(pixel_shuffle), Hout, Wout)
    # 'f16fp8' mode (_lib.set_gemm_mode): every forward conv the library's plan grants the f16 + fp8 product format (weight image and kernel)
    if _lib.fmt_f16fp8() and L.rvsr_conv2d_forward_plan(*call, w_mode | 4, *tail, None) == 0:
        w_mode |= 4
    # (5x5 through the zero-insert view: the exact-f32 kernel reads the weights directly, an image would go unused; 7x7 has no image at
    # all, which PackedWeights.get knows)
    buf = None if k == 5 and in_mode == 1 else packed_weights.get(weight, 'conv', C1 + C2, Co1 + Co2, k, w_mode, nbytes)
    if buf is not None:
        ws, w_mode = buf, w_mode | 2
    else:
        ws = _workspace(nbytes, torch.device('cuda', torch.cuda.current_device()))
    if addend_period:
        rc = L.rvsr_conv2d_forward_addend(*call, w_mode, *tail, addend_period, _p(ws), ws.numel(), _stream())
    else:
        rc = L.rvsr_conv2d_forward(*call, w_mode, *tail, _p(ws), ws.numel(), _stream())
    if rc == _lib.RVSR_ERR_UNSUPPORTED and (act == ACT_MASK or addend_period):   # an option of one kernel, the caller has a plan B
        return False
    _lib.check(rc, what)
    return True


def _conv_wgrad(x1, gout, gw, gb, *, what, x2=None, gact=None, gact_slope=0.0, pixel_shuffled=False, stride=1):
    """rvsr_conv2d_backward_weight: gw (Co, C1 + C2, k, k) and gb (Co, or None) of the conv of cat(x1, x2) whose output gradient is gout
    (times act' taken from the saved output `gact`); pixel_shuffled: gout (and gact) are stored (B, Co/4, 2*Hout, 2*Wout)."""
    C1, H, W = x1.shape[-3:]
    B, C2 = x1.numel() // (C1 * H * W), (0 if x2 is None else x2.shape[-3])
    Co, k = gw.shape[0], gw.shape[-1]
    Gh, Gw = gout.shape[-2:]
    Ho, Wo = (Gh // 2, Gw // 2) if pixel_shuffled else (Gh, Gw)
    L = _lib.lib()
    ws = _workspace(L.rvsr_conv2d_wgrad_workspace_bytes(C1, C2, Co, B, k, stride, Ho, Wo), x1.device)
    _lib.check(L.rvsr_conv2d_backward_weight(_p(x1), C1, _p(x2), C2, H, W, _p(gout), _p(gact), gact_slope, 2 if pixel_shuffled else 0,
                                             Gh, Gw, _p(gw), _p(gb), Co, B, k, stride, Ho, Wo, 0, _p(ws), ws.numel(), _stream()), what)


def _wgrad(x1, gout, weight, bias, *, what, **kw):
    """The weight and bias gradient of a conv from its saved input `x1` and its output gradient, written where _pgrad puts the gradients
    of the parameters `weight` and `bias` (None: the conv has no bias).  Returns (gw, gb); the keywords are _conv_wgrad's.  Only the first
    and last dimension of gw are read, so a (Co, Ci, 1, k, k) Conv3d weight passes for its 2-D layout."""
    gw = _pgrad(weight)
    gb = _pgrad(bias) if bias is not None else None
    _conv_wgrad(x1, gout, gw, gb, what=what, **kw)
    return gw, gb


def _res_chain_backward(node, g, skip, x, h, w1, b1, w2, b2, needs):
    """Backward of h = relu(conv1(x)), u = conv2(h) given g = dL/du: (gx, gw1, gb1, gw2, gb2) for needs = (x, w1, b1, w2, b2).
    gx = skip + dgrad1(...): conv1's data-gradient kernel adds `skip`, the gradient that reaches x past the two convs, as its fused
    residual.  `node` prefixes the call names."""
    need_x, need_w1, need_b1, need_w2, need_b2 = needs
    gx = gw1 = gb1 = gw2 = gb2 = None
    if need_w2 or need_b2:
        gw2, gb2 = _wgrad(h, g, w2, b2, what=node + ' wgrad2')
    if need_x or need_w1 or need_b1:
        # gradient w.r.t. conv1's output: conv2's data gradient times relu'(h).  The mask is applied in that kernel's epilogue when it
        # has one (8 x 64 tile; one extra read of h instead of a second read of h in BOTH consumers below), else by the consumers.
        gh = torch.empty_like(x)
        masked = _FUSE_GRAD_MASK and _conv(g, w2, gh, transposed=True, act=ACT_MASK, residual=h, what=node + ' dgrad2')
        if not masked:
            _conv(g, w2, gh, transposed=True, what=node + ' dgrad2')
        hmask = None if masked else h
        if need_w1 or need_b1:
            gw1, gb1 = _wgrad(x, gh, w1, b1, gact=hmask, what=node + ' wgrad1')
        if need_x:
            gx = torch.empty_like(x)
            _conv(gh, w1, gx, transposed=True, xact=hmask, residual=skip, what=node + ' dgrad1')
    return gx, gw1, gb1, gw2, gb2


# ------------------------------------------------------------------------------------------ conv
class _Conv2dFused(Function):
    """act(conv2d(cat(x1, x2), w) + b) [+ residual] [-> PixelShuffle(2)]"""

    @staticmethod
    def forward(ctx, x1, x2, weight, bias, residual, stride, act, slope, pixel_shuffle, sink=None, dep_sink=None, x_premask=None,
                grad_premasked=False):
        # x_premask = (act, slope) of the activation that PRODUCED x1, given when this conv is x1's only consumer: the data gradient then
        # leaves this node already multiplied by act'(x1) (in the dgrad kernel's epilogue where it has one, rvsr_conv2d_forward act = 3),
        # and the producer, called with grad_premasked=True, applies no mask in its own backward -- one read of x1 instead of a read of
        # the producer's output in both of its gradient kernels.  (Multiplying by act' is linear, so it commutes with autograd's sum over
        # consumers; the pairing is still only set up for single-consumer chains, archs/EDVR_arch.py.)
        if x_premask is not None and (x2 is not None or sink is not None or dep_sink is not None or pixel_shuffle or stride != 1):
            raise RuntimeError('conv2d: x_premask is for single-input stride-1 convs without a GradSink')
        if grad_premasked and (act == ACT_NONE or residual is not None):
            # the consumer multiplies by act'(this conv's OUTPUT): with a residual added (or no activation) the output is not an
            # activation output and the pairing would silently drop / misapply the derivative
            raise RuntimeError('conv2d: grad_premasked needs an activation and no residual on the producing conv')
        ctx.x_premask, ctx.grad_premasked = x_premask, bool(grad_premasked)
        if x2 is not None and (sink is not None or dep_sink is not None):
            # an owner that never closes drops what the depositors wrote: sinks are for single-input convs only
            raise RuntimeError('conv2d: a GradSink cannot be combined with a second (concatenated) input')
        _need_cuda(x1, x2, weight, bias, residual)
        ctx.sink = sink           # GradSink of x1: this conv is its OWNER (see GradSink)
        ctx.dep_sink = dep_sink   # GradSink of x1: this conv is a DEPOSITOR (single-input convs only)
        x1, x2, weight, bias, residual = _c(x1), _c(x2), _c(weight), _c(bias), _c(residual)
        B, C1, H, W = x1.shape
        C2 = 0 if x2 is None else x2.shape[1]
        Co, Cw, k, _ = weight.shape
        if Cw != C1 + C2:
            raise RuntimeError('conv2d: weight expects %d input channels, got %d' % (Cw, C1 + C2))
        pad = k // 2
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        if pixel_shuffle:
            out = x1.new_empty(B, Co // 4, 2 * Ho, 2 * Wo)
        else:
            out = x1.new_empty(B, Co, Ho, Wo)
        _conv(x1, weight, out, x2=x2, bias=bias, residual=residual, stride=stride, act=act, slope=slope, pixel_shuffle=pixel_shuffle,
              what='conv2d_forward')
        ctx.cfg = (stride, act, slope, bool(pixel_shuffle), k, bias is not None, residual is not None)
        ctx.save_for_backward(x1, x2, weight, out if act != ACT_NONE else None)
        ctx.bias_p = bias   # only to find its gradient buffer (_pgrad)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x1, x2, weight, act_out = ctx.saved_tensors
        stride, act, slope, ps, k, has_bias, has_res = ctx.cfg
        gout = gout.contiguous()
        gslope = 0.0 if act == ACT_RELU else slope
        if ctx.grad_premasked:
            act_out = None   # gout arrives multiplied by act'(out) already (the consumer's x_premask)
        need_x1, need_x2, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        gx1 = gx2 = gw = gb = None
        if ctx.sink is not None and not need_x1:
            # the owner always closes: what the depositors wrote is x1's gradient even if autograd wants none from this conv
            ctx.sink.close()
        if need_x1 or (x2 is not None and need_x2):
            # owner of a GradSink (single-input convs only): add this data gradient onto what the other consumers of x1 deposited
            dep = ctx.sink.close() if (ctx.sink is not None and x2 is None) else None
            deposit = ctx.dep_sink is not None and x2 is None and not ctx.dep_sink.closed
            if deposit and ctx.dep_sink.buf is not None:
                dep = ctx.dep_sink.buf            # a later depositor: add in place
            gx1 = dep if dep is not None else torch.empty_like(x1)
            gx2 = torch.empty_like(x2) if x2 is not None else None
            in_mode = 2 if ps else (1 if stride == 2 else 0)
            masked = False
            if ctx.x_premask is not None:
                pslope = 0.0 if ctx.x_premask[0] == ACT_RELU else ctx.x_premask[1]
                masked = _FUSE_GRAD_MASK and k == 3 and _conv(gout, weight, gx1, transposed=True, xact=act_out, xact_slope=gslope, in_mode=in_mode,
                                                              act=ACT_MASK, slope=pslope, residual=x1, what='conv2d_backward_data')
            if not masked:
                _conv(gout, weight, gx1, transposed=True, xact=act_out, xact_slope=gslope, in_mode=in_mode, residual=dep, out2=gx2,
                      what='conv2d_backward_data')
                if ctx.x_premask is not None:   # no fused epilogue for this frame / GEMM mode: the mask as a separate pass (the producer applies none)
                    gx1.mul_(torch.where(x1 > 0, 1.0, pslope))
            if deposit:   # the first depositor's output IS the sink's buffer (no zero fill); autograd gets no gradient from here
                ctx.dep_sink.buf = gx1
                gx1 = None
        if need_w or (has_bias and ctx.needs_input_grad[3]):
            gw, gb = _wgrad(x1, gout, weight, ctx.bias_p, x2=x2, gact=act_out, gact_slope=gslope, pixel_shuffled=ps, stride=stride,
                            what='conv2d_backward_weight')
        gres = gout if has_res else None
        return gx1, gx2, gw, gb, gres, None, None, None, None, None, None, None, None


class _ResBlockFused(Function):
    """x + conv2(relu(conv1(x))) as ONE autograd node (arch_util.ResidualBlock_noBN, reference
    codes/models/archs/arch_util.py:37-52).  Forward is the same two fused kernels as two conv2d()
    calls; the point is the backward: grad_x = grad_out + dgrad1(...) is produced by conv1's
    data-gradient kernel with grad_out as its fused residual, instead of a separate full-tensor
    add by autograd (3 passes over a B x 64 x H x W tensor per block)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        _need_cuda(x, w1, b1, w2, b2)
        x, w1, b1, w2, b2 = _c(x), _c(w1), _c(b1), _c(w2), _c(b2)
        B, C, H, W = x.shape
        if w1.shape != (C, C, 3, 3) or w2.shape != (C, C, 3, 3):
            raise RuntimeError('res_block: expected two %dx%dx3x3 convs' % (C, C))
        h, out = torch.empty_like(x), torch.empty_like(x)
        _conv(x, w1, h, bias=b1, act=ACT_RELU, what='res_block conv1')
        _conv(h, w2, out, bias=b2, residual=x, what='res_block conv2')
        ctx.save_for_backward(x, h, w1, w2)
        ctx.bias_p = (b1, b2)   # only to find their gradient buffers (_pgrad)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, h, w1, w2 = ctx.saved_tensors
        gout = gout.contiguous()
        return _res_chain_backward('res_block', gout, gout, x, h, w1, ctx.bias_p[0], w2, ctx.bias_p[1], ctx.needs_input_grad)


class _ConvCatBcast(Function):
    """act(conv3x3(cat([x, ref.repeat(N, 1, 1, 1)], 1), w) + b) for a frame-major x [N*B, C1, H, W] and ref [B, C2, H, W],
    WITHOUT the repeat and without convolving the same reference N times:

        conv(cat(x, repeat(ref))) = conv_a(x) + conv_b(ref),     w = [w_a | w_b] along the input channels.

    PCD_Align convolves cat([nbr, ref]) four times per frame (EDVR_arch.py:100, 109, 118, 127) and the reference
    features are those of the window's centre frame for all N frames (:297-303): conv_b runs on B frames instead of
    N*B (fwd, dgrad and wgrad: 2.0 -> 1.2 conv-equivalents each), the 2x-wide conv reads half the channels, and the
    N copies of ref are never materialised.  The glue is one in-place pass (add broadcast + activation) forward and
    one reduction over N backward; act' is taken from the saved output as everywhere else."""

    @staticmethod
    def forward(ctx, x, ref, weight, bias, N, act, slope, x_sink=None, x_owner=False, ref_sink=None, ref_block=0, grad_premasked=False):
        ctx.grad_premasked = bool(grad_premasked)   # the only consumer multiplies its data gradient by act'(out) (conv2d x_premask)
        _need_cuda(x, ref, weight, bias)
        x, ref, weight, bias = _c(x), _c(ref), _c(weight), _c(bias)
        # GradSinks (see GradSink): x_sink collects the gradient of x (this conv deposits, or owns it when x_owner);
        # ref_sink is the sink of the [N*B] tensor whose block `ref_block` IS ref: the ref gradient is added into that block
        ctx.sinks = (x_sink, bool(x_owner), ref_sink, int(ref_block))
        NB, C1, H, W = x.shape
        B, C2 = ref.shape[0], ref.shape[1]
        Co, Cw, k, _ = weight.shape
        if NB != N * B or Cw != C1 + C2 or k != 3 or tuple(ref.shape[2:]) != (H, W):
            raise RuntimeError('conv_cat_bcast: x %s, ref %s, weight %s, N %d do not fit' % (tuple(x.shape), tuple(ref.shape), tuple(weight.shape), N))
        w_a, w_b = packed_weights.split(weight, C1)   # persistent per-step copies when the weight lives in FlatBuffers
        out = x.new_empty(NB, Co, H, W)
        part = x.new_empty(B, Co, H, W)
        _conv(ref, w_b, part, what='conv_cat_bcast conv_b')
        # the partial as an addend of conv_a's epilogue where that kernel has one (8 x 64 tile), else a pass of its own over `out`
        if not (_FUSE_BCAST_ADDEND and _conv(x, w_a, out, bias=bias, residual=part, addend_period=B, act=act, slope=slope,
                                             what='conv_cat_bcast conv_a')):
            _conv(x, w_a, out, bias=bias, what='conv_cat_bcast conv_a')
            _lib.check(_lib.lib().rvsr_bcast_add_act(_p(out), _p(part), part.numel(), N, act, slope, _stream()), 'bcast_add_act')
        ctx.cfg = (N, act, slope, bias is not None)
        ctx.w_ab = (w_a, w_b)   # (python references: the cached slices carry the attribute the weight-image cache keys on)
        # the cached slices are PERSISTENT tensors that repack() / split() overwrite in place, behind save_for_backward's version
        # check: remember what they were copied from, backward refuses to run on newer weights
        ctx.w_tag = (weight._version, packed_weights.epoch if getattr(w_a, '_rvsr_parent', None) is not None else None)
        ctx.save_for_backward(x, ref, out if act != ACT_NONE else None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, ref, act_out = ctx.saved_tensors
        w_a, w_b = ctx.w_ab
        if ctx.w_tag[1] is not None:
            parent = w_a._rvsr_parent()
            if parent is None or parent._version != ctx.w_tag[0] or packed_weights.epoch != ctx.w_tag[1]:
                raise RuntimeError('conv_cat_bcast: the weights were modified (optimizer step / in-place write) between this forward '
                                   'and its backward')
        N, act, slope, has_bias = ctx.cfg
        gout = gout.contiguous()
        B, Co = ref.shape[0], w_a.shape[0]
        gslope = 0.0 if act == ACT_RELU else slope
        if ctx.grad_premasked:
            act_out = None
        gx = gref = gw = gb = None
        # gradient of the broadcast partial: sum over the N frames of gout * act'
        gpart = x.new_empty(B, Co, *x.shape[2:])
        _lib.check(_lib.lib().rvsr_bcast_reduce_act(_p(gout), _p(act_out), _p(gpart), gpart.numel(), N, gslope, _stream()), 'bcast_reduce_act')
        x_sink, x_owner, ref_sink, ref_block = ctx.sinks
        # (the reference gradient first: when this conv owns x's sink and ref is a block of x, the deposit must precede the close)
        if ctx.needs_input_grad[1]:
            blk = None
            if ref_sink is not None and not ref_sink.closed:
                full = ref_sink.buf
                if full is None:
                    full = ref_sink.buf = ref.new_zeros(ref_sink.shape)
                blk = full[ref_block * B:(ref_block + 1) * B]
            gref = blk if blk is not None else torch.empty_like(ref)
            _conv(gpart, w_b, gref, transposed=True, residual=blk, what='conv_cat_bcast dgrad_b')
            if blk is not None:
                gref = None  # deposited into the block of the full tensor's sink
        if ctx.needs_input_grad[0]:
            dep = None
            if x_sink is not None:
                dep = x_sink.close() if x_owner else x_sink.get(x)
            gx = dep if dep is not None else torch.empty_like(x)
            # a fresh sink buffer is all zeros: adding it as the residual is exact and keeps one code path
            _conv(gout, w_a, gx, transposed=True, xact=act_out, xact_slope=gslope, residual=dep, what='conv_cat_bcast dgrad_a')
            if dep is not None and not x_owner:
                gx = None    # deposited: the owner returns the buffer
        if ctx.needs_input_grad[2] or (has_bias and ctx.needs_input_grad[3]):
            gw_a, gw_b = torch.empty_like(w_a), torch.empty_like(w_b)
            gb = w_a.new_empty(Co) if has_bias else None
            _conv_wgrad(x, gout, gw_a, gb, gact=act_out, gact_slope=gslope, what='conv_cat_bcast wgrad_a')
            _conv_wgrad(ref, gpart, gw_b, None, what='conv_cat_bcast wgrad_b')
            gw = torch.cat([gw_a, gw_b], 1)
        return gx, gref, gw, gb, None, None, None, None, None, None, None, None


def conv_cat_bcast(x, ref, conv, N, act=ACT_NONE, slope=0.1, x_sink=None, x_owner=False, ref_sink=None, ref_block=0, grad_premasked=False):
    """act(conv(cat([x, ref.repeat(N, 1, 1, 1)], 1))) for frame-major x [N*B, ...] and ref [B, ...] (3x3, stride 1)."""
    return _ConvCatBcast.apply(x, ref, conv.weight, conv.bias, int(N), act, float(slope), x_sink, x_owner, ref_sink, ref_block, grad_premasked)


def res_block(x, conv1, conv2):
    """x + conv2(relu(conv1(x))) with the identity add fused in both directions."""
    return _ResBlockFused.apply(x, conv1.weight, conv1.bias, conv2.weight, conv2.bias)


def conv2d(x, conv, act=ACT_NONE, slope=0.1, x2=None, residual=None, pixel_shuffle=False, sink=None, dep_sink=None, x_premask=None,
           grad_premasked=False):
    """Fused conv block driven by an ``nn.Conv2d`` parameter holder (weight, bias, stride).

    out = act(conv(cat(x, x2))) [+ residual]; with ``pixel_shuffle`` the activation commutes with
    the shuffle, so lrelu(pixel_shuffle(conv(x))) (EDVR_arch.py:311-312) is one kernel."""
    stride = conv.stride[0] if isinstance(conv.stride, tuple) else conv.stride
    if grad_premasked and residual is not None:
        raise RuntimeError('conv2d: grad_premasked cannot be combined with a residual (out + residual is not an activation output)')
    if residual is not None and act != ACT_NONE:
        # act'(.) is recovered from the saved activation output, so the residual is added outside
        out = _Conv2dFused.apply(x, x2, conv.weight, conv.bias, None, stride, act, slope, pixel_shuffle, sink, dep_sink, x_premask,
                                 grad_premasked)
        return out + residual
    return _Conv2dFused.apply(x, x2, conv.weight, conv.bias, residual, stride, act, slope, pixel_shuffle, sink, dep_sink, x_premask,
                              grad_premasked)


_mask_fusable = {}   # (H, W, GEMM mode) -> the plan's answer


def grad_mask_fusable(H, W):
    """Whether the data-gradient kernel of a 3x3 stride-1 conv on H x W frames has the mask epilogue (act 3 of rvsr_conv2d_forward): the
    library's plan is asked about the call this stands for, 64 -> 64 channels on aligned tensors.  Where it has not, x_premask costs a
    separate pass."""
    L = _lib.lib()
    key = (H, W, L.rvsr_get_gemm_mode())
    if key not in _mask_fusable:
        a = _lib.c_fp(1 << 20)   # any 16-byte-aligned address: the plan reads none
        _mask_fusable[key] = L.rvsr_conv2d_forward_plan(a, 64, None, 0, None, 0.0, 0, H, W, a, None, a, a, 64, None, 0, 1, 3, 1, 1,
                                                        ACT_MASK, 0.1, 0, H, W, None) == 0
    return _FUSE_GRAD_MASK and _mask_fusable[key]


# ------------------------------------------------------------------------------------------ DCN
# ---- the general path of the deformable operator (include/realvsr_hip.h section 1c, csrc/dcn_generic.hip): any kernel size, anisotropic
# stride / padding / dilation, groups, any channels per deformable group, f32 / f64 / f16.  The fused kernels take the calls they cover.
_GENERIC_DTYPES = {torch.float32: 0, torch.float64: 1, torch.float16: 2}


def _pair2(v):
    from torch.nn.modules.utils import _pair
    a, b = _pair(v)
    return int(a), int(b)


def _dcn_fused_ok(input, weight, stride, padding, dilation, groups, dg):
    """Whether the fused f32 kernels cover this call: f32, and a geometry they take (dcn_fused_takes, csrc/dcn_plan.h)."""
    (sh, sw), (ph, pw), (dh, dw) = _pair2(stride), _pair2(padding), _pair2(dilation)
    B, C, H, W = input.shape
    Co, _, kh, kw = weight.shape
    return input.dtype == torch.float32 and _lib.lib().rvsr_dcn_fused_takes(B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, groups, dg) == 0


def _generic_geom(input, weight, stride, padding, dilation):
    (sh, sw), (ph, pw), (dh, dw) = _pair2(stride), _pair2(padding), _pair2(dilation)
    B, C, H, W = input.shape
    Co, _, kh, kw = weight.shape
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    return (B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw), Ho, Wo


def _generic_check(input, offset, mask, weight, bias, groups, dg, Ho, Wo):
    dt = _GENERIC_DTYPES.get(input.dtype)
    if dt is None:
        raise TypeError('deformable convolution: element type %s (f32, f64 and f16 are implemented)' % input.dtype)
    B, C = input.shape[:2]
    Co, cg, kh, kw = weight.shape
    for name, t in (('offset', offset), ('mask', mask), ('weight', weight), ('bias', bias)):
        if t is not None and t.dtype != input.dtype:
            raise TypeError('deformable convolution: %s is %s, input is %s' % (name, t.dtype, input.dtype))
    if C % groups or Co % groups or cg * groups != C:
        raise RuntimeError('deformable convolution: channels (%d -> %d, weight %s) not divisible into %d groups' % (C, Co, tuple(weight.shape), groups))
    if dg <= 0 or C % dg:
        raise RuntimeError('deformable convolution: %d input channels not divisible into %d deformable groups' % (C, dg))
    if Ho <= 0 or Wo <= 0:
        raise ValueError('convolution input is too small (output would be %dx%d)' % (Ho, Wo))
    if tuple(offset.shape) != (B, 2 * dg * kh * kw, Ho, Wo):
        raise RuntimeError('deformable convolution: offset has shape %s, expected %s' % (tuple(offset.shape), (B, 2 * dg * kh * kw, Ho, Wo)))
    if mask is not None and tuple(mask.shape) != (B, dg * kh * kw, Ho, Wo):
        raise RuntimeError('deformable convolution: mask has shape %s, expected %s' % (tuple(mask.shape), (B, dg * kh * kw, Ho, Wo)))
    return dt


def _generic_dcn_forward(input, offset, mask, weight, bias, stride, padding, dilation, groups, dg):
    geo, Ho, Wo = _generic_geom(input, weight, stride, padding, dilation)
    dt = _generic_check(input, offset, mask, weight, bias, groups, dg, Ho, Wo)
    input, offset, weight = input.contiguous(), offset.contiguous(), weight.contiguous()
    mask = None if mask is None else mask.contiguous()
    bias = None if bias is None else bias.contiguous()
    out = input.new_empty(input.shape[0], weight.shape[0], Ho, Wo)
    L = _lib.lib()
    ws = _workspace(L.rvsr_deform_conv_generic_forward_workspace_bytes(dt, *geo[1:4], *geo[5:]), input.device)
    _lib.check(L.rvsr_deform_conv_generic_forward(dt, _p(input), _p(weight), _p(bias), _p(offset), _p(mask), _p(out), *geo, groups, dg,
                                                  _p(ws), ws.numel(), _stream()), 'deform_conv_generic_forward')
    return out


def _generic_dcn_backward(input, offset, mask, weight, grad_output, stride, padding, dilation, groups, dg, need_input, need_weight, with_bias):
    geo, Ho, Wo = _generic_geom(input, weight, stride, padding, dilation)
    dt = _GENERIC_DTYPES[input.dtype]
    input, offset, weight, grad_output = input.contiguous(), offset.contiguous(), weight.contiguous(), grad_output.contiguous()
    mask = None if mask is None else mask.contiguous()
    gx = torch.zeros_like(input) if need_input else None
    goff = torch.empty_like(offset) if need_input else None
    gmask = torch.empty_like(mask) if (need_input and mask is not None) else None
    gw = torch.zeros_like(weight) if need_weight else None
    gb = weight.new_zeros(weight.shape[0]) if with_bias else None
    L = _lib.lib()
    ws = _workspace(L.rvsr_deform_conv_generic_workspace_bytes(dt, *geo[1:4], *geo[5:]), input.device)
    _lib.check(L.rvsr_deform_conv_generic_backward(dt, _p(input), _p(weight), _p(offset), _p(mask), _p(grad_output), _p(gx), _p(goff), _p(gmask),
                                                   _p(gw), _p(gb), *geo, groups, dg, _p(ws), ws.numel(), _stream()), 'deform_conv_generic_backward')
    return gx, goff, gmask, gw, gb


class ModulatedDeformConvFunction(Function):
    """Same signature and semantics as the reference's autograd Function
    (codes/models/archs/dcn/deform_conv.py:97-153)."""

    @staticmethod
    def forward(ctx, input, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, groups=1,
                deformable_groups=1):
        if not input.is_cuda:
            raise NotImplementedError
        _need_cuda(input, offset, mask, weight, bias, any_float=True)
        if not input.is_contiguous():
            raise RuntimeError('input tensor has to be contiguous')      # deform_conv_cuda.cpp:497
        if not weight.is_contiguous():
            raise RuntimeError('weight tensor has to be contiguous')     # deform_conv_cuda.cpp:498
        offset, mask = offset.contiguous(), mask.contiguous()
        ctx.generic = not _dcn_fused_ok(input, weight, stride, padding, dilation, groups, deformable_groups)
        if ctx.generic:   # any kernel size / anisotropic geometry / groups / f64, f16: the general path (realvsr_hip.h section 1c)
            ctx.cfg = (stride, padding, dilation, groups, deformable_groups, bias is not None)   # as given: _generic_dcn_backward takes pairs
            ctx.save_for_backward(input, offset, mask, weight, bias)
            return _generic_dcn_forward(input, offset, mask, weight, bias, stride, padding, dilation, groups, deformable_groups)
        stride, padding, dilation = _pair2(stride)[0], _pair2(padding)[0], _pair2(dilation)[0]   # (isotropic here; pairs are accepted)
        ctx.cfg = (stride, padding, dilation, groups, deformable_groups, bias is not None)   # ints: the fused backward
        B, C, H, W = input.shape
        Co, _, kh, kw = weight.shape
        Ho = (H + 2 * padding - (dilation * (kh - 1) + 1)) // stride + 1
        Wo = (W + 2 * padding - (dilation * (kw - 1) + 1)) // stride + 1
        output = input.new_empty(B, Co, Ho, Wo)
        L = _lib.lib()
        ws = _workspace(L.rvsr_modulated_deform_conv_forward_workspace_bytes(C, Co), input.device)
        _lib.check(L.rvsr_modulated_deform_conv_forward(
            _p(input), _p(weight), _p(bias), _p(offset), _p(mask), _p(output), B, C, H, W, Co, kh, kw, stride, stride,
            padding, padding, dilation, dilation, groups, deformable_groups, int(bias is not None), _p(ws), ws.numel(),
            _stream()),
            'modulated_deform_conv_forward')
        ctx.save_for_backward(input, offset, mask, weight, bias)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        if not grad_output.is_cuda:
            raise NotImplementedError
        input, offset, mask, weight, bias = ctx.saved_tensors
        stride, padding, dilation, groups, dg, with_bias = ctx.cfg
        if ctx.generic:
            gx, goff, gmask, gw, gb = _generic_dcn_backward(input, offset, mask, weight, grad_output, stride, padding, dilation, groups, dg, True, True,
                                                            with_bias)
            return gx, goff, gmask, gw, gb, None, None, None, None, None
        grad_output = grad_output.contiguous()
        B, C, H, W = input.shape
        Co, _, kh, kw = weight.shape
        grad_input = torch.zeros_like(input)
        grad_offset = torch.empty_like(offset)
        grad_mask = torch.empty_like(mask)
        grad_weight = torch.zeros_like(weight)
        grad_bias = torch.zeros_like(bias) if with_bias else None
        L = _lib.lib()
        nbytes = L.rvsr_modulated_deform_conv_backward_workspace_bytes(B, C, H, W, Co, stride, padding, dilation)
        ws = _workspace(nbytes, input.device)
        _lib.check(L.rvsr_modulated_deform_conv_backward(
            _p(input), _p(weight), _p(bias), _p(offset), _p(mask), _p(grad_input), _p(grad_weight), _p(grad_bias),
            _p(grad_offset), _p(grad_mask), _p(grad_output), B, C, H, W, Co, kh, kw, stride, stride, padding, padding,
            dilation, dilation, groups, dg, int(with_bias), _p(ws), ws.numel(), _stream()),
            'modulated_deform_conv_backward')
        return grad_input, grad_offset, grad_mask, grad_weight, grad_bias, None, None, None, None, None


def modulated_deform_conv(input, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1):
    """The reference's functional entry point (deform_conv.py:99-100 binds it to ModulatedDeformConvFunction.apply).  groups > 1
    (deform_conv_cuda.cpp:539-561: one im2col over all channels, then one GEMM per group on that group's slice of the columns) is
    composed from `groups` calls of the groups == 1 operator on channel slices -- possible whenever a group's channels see whole
    deformable groups (deformable_groups % groups == 0) or lie inside one (groups % deformable_groups == 0)."""
    if groups == 1:
        return ModulatedDeformConvFunction.apply(input, offset, mask, weight, bias, stride, padding, dilation, 1, deformable_groups)
    if not input.is_cuda:
        raise NotImplementedError
    C, Co, dg = input.shape[1], weight.shape[0], deformable_groups
    slices_fused = (C % groups == 0 and (dg % groups == 0 or groups % dg == 0) and
                    _dcn_fused_ok(input[:, :C // groups], weight, stride, padding, dilation, 1, max(dg // groups, 1)))
    if not slices_fused:   # (the general path takes groups as the reference does: one GEMM per group on the shared columns)
        return ModulatedDeformConvFunction.apply(input, offset, mask, weight, bias, stride, padding, dilation, groups, deformable_groups)
    K = weight.shape[2] * weight.shape[3]
    if C % groups or Co % groups or weight.shape[1] * groups != C:
        raise RuntimeError('modulated_deform_conv: channels (%d -> %d) not divisible into %d groups' % (C, Co, groups))
    if dg % groups and groups % dg:
        raise RuntimeError('modulated_deform_conv: groups %d / deformable_groups %d: a group would see part of a deformable group; '
                           'not implemented on the HIP path' % (groups, dg))
    cg, og = C // groups, Co // groups
    outs = []
    for g in range(groups):
        if dg % groups == 0:
            d0, dn = g * (dg // groups), dg // groups
        else:
            d0, dn = g // (groups // dg), 1
        outs.append(ModulatedDeformConvFunction.apply(
            input[:, g * cg:(g + 1) * cg].contiguous(), offset[:, 2 * K * d0:2 * K * (d0 + dn)], mask[:, K * d0:K * (d0 + dn)],
            weight[g * og:(g + 1) * og].contiguous(), None if bias is None else bias[g * og:(g + 1) * og], stride, padding, dilation, 1, dn))
    return torch.cat(outs, 1)


class DeformConvFunction(Function):
    """DCNv1, same signature and semantics as the reference's autograd Function (codes/models/archs/dcn/deform_conv.py:15-95):
    (input, offset, weight, stride, padding, dilation, groups, deformable_groups, im2col_step); stride / padding / dilation are
    ints or pairs.  Runs the modulated kernels on a mask of ones (include/realvsr_hip.h section 1b)."""

    @staticmethod
    def forward(ctx, input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, im2col_step=64):
        from torch.nn.modules.utils import _pair
        if input is not None and input.dim() != 4:
            raise ValueError('Expected 4D tensor as input, got {}D tensor instead.'.format(input.dim()))
        ctx.stride, ctx.padding, ctx.dilation = _pair(stride), _pair(padding), _pair(dilation)
        ctx.groups, ctx.deformable_groups, ctx.im2col_step = groups, deformable_groups, im2col_step
        out_size = DeformConvFunction._output_size(input, weight, ctx.padding, ctx.dilation, ctx.stride)
        if not input.is_cuda:
            raise NotImplementedError
        _need_cuda(input, offset, weight, any_float=True)
        cur = min(im2col_step, input.shape[0])
        assert (input.shape[0] % cur) == 0, 'im2col step must divide batchsize'
        input, offset, weight = input.contiguous(), offset.contiguous(), weight.contiguous()   # deform_conv_cuda.cpp:170-172
        if offset.shape[0] != input.shape[0]:
            raise RuntimeError('invalid batch size of offset')                               # deform_conv_cuda.cpp:193
        ctx.save_for_backward(input, offset, weight)
        ctx.generic = not _dcn_fused_ok(input, weight, ctx.stride, ctx.padding, ctx.dilation, groups, deformable_groups)
        if ctx.generic:   # the general path (realvsr_hip.h section 1c): mask == NULL is DCNv1
            return _generic_dcn_forward(input, offset, None, weight, None, ctx.stride, ctx.padding, ctx.dilation, groups, deformable_groups)
        output = input.new_empty(out_size)
        DeformConvFunction._call('rvsr_deform_conv_forward', ctx, input, weight, cur, [input, weight, offset, output], [])
        return output

    @staticmethod
    def _call(name, ctx, input, weight, cur, tensors, extra):
        L = _lib.lib()
        B, C, H, W = input.shape
        Co, _, kh, kw = weight.shape
        (sh, sw), (ph, pw), (dh, dw) = ctx.stride, ctx.padding, ctx.dilation
        n = L.rvsr_deform_conv_workspace_bytes(B, C, H, W, Co, kw, kh, sw, pw, dw, ctx.deformable_groups)
        ws = _workspace(n, input.device)
        _lib.check(getattr(L, name)(*[_p(t) for t in tensors], B, C, H, W, Co, kw, kh, sw, sh, pw, ph, dw, dh, ctx.groups,
                                    ctx.deformable_groups, *extra, cur, _p(ws), ws.numel(), _stream()), name[5:])

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input, offset, weight = ctx.saved_tensors
        grad_input = grad_offset = grad_weight = None
        if not grad_output.is_cuda:
            raise NotImplementedError
        cur = min(ctx.im2col_step, input.shape[0])
        grad_output = grad_output.contiguous()
        if ctx.generic:
            gx, goff, _, gw, _ = _generic_dcn_backward(input, offset, None, weight, grad_output, ctx.stride, ctx.padding, ctx.dilation, ctx.groups,
                                                       ctx.deformable_groups, ctx.needs_input_grad[0] or ctx.needs_input_grad[1],
                                                       ctx.needs_input_grad[2], False)
            return gx, goff, gw, None, None, None, None, None, None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            grad_input, grad_offset = torch.zeros_like(input), torch.zeros_like(offset)
            DeformConvFunction._call('rvsr_deform_conv_backward_input', ctx, input, weight, cur,
                                     [input, offset, grad_output, grad_input, grad_offset, weight], [])
        if ctx.needs_input_grad[2]:
            grad_weight = torch.zeros_like(weight)
            DeformConvFunction._call('rvsr_deform_conv_backward_parameters', ctx, input, weight, cur,
                                     [input, offset, grad_output, grad_weight], [1.0])
        return grad_input, grad_offset, grad_weight, None, None, None, None, None, None

    @staticmethod
    def _output_size(input, weight, padding, dilation, stride):
        size = (input.size(0), weight.size(0))
        for d in range(input.dim() - 2):
            kernel = dilation[d] * (weight.size(d + 2) - 1) + 1
            size += ((input.size(d + 2) + 2 * padding[d] - kernel) // stride[d] + 1,)
        if not all(s > 0 for s in size):
            raise ValueError('convolution input is too small (output would be {})'.format('x'.join(map(str, size))))
        return size


deform_conv = DeformConvFunction.apply


class _DcnPackFused(Function):
    """DCN fed directly by the raw conv_offset_mask output (chunk/cat/sigmoid fused)."""

    @staticmethod
    def forward(ctx, x, om, weight, bias, stride, padding, dilation, dg, act, slope, sink=None):
        _need_cuda(x, om, weight, bias)
        x, om, weight, bias = _c(x), _c(om), _c(weight), _c(bias)
        ctx.sink = sink   # GradSink of x: the DCN is a depositor (its backward accumulates atomically into the buffer)
        B, C, H, W = x.shape
        Co = weight.shape[0]
        if weight.shape[2:] != (3, 3):
            raise RuntimeError('fused DCN pack supports 3x3 kernels')
        Ho = (H + 2 * padding - (dilation * 2 + 1)) // stride + 1
        Wo = (W + 2 * padding - (dilation * 2 + 1)) // stride + 1
        if tuple(om.shape) != (B, 27 * dg, Ho, Wo):
            raise RuntimeError('conv_offset_mask output has shape %s, expected %s' % (tuple(om.shape), (B, 27 * dg, Ho, Wo)))
        out = x.new_empty(B, Co, Ho, Wo)
        L = _lib.lib()
        nbytes = L.rvsr_modulated_deform_conv_forward_workspace_bytes(C, Co)
        ws = packed_weights.get(weight, 'dcn', C, Co, 3, 0, nbytes)          # per-step weight image (act bit 8: already packed)
        flags = 0x100 if ws is not None else 0
        if ws is None:
            ws = _workspace(nbytes, x.device)
        # Halo of the forward's LDS tile.  Training: chosen HERE from the offset counters the previous backward of this layer left
        # (copied to the host asynchronously, see DcnOffsetStats) -- one kernel launch, no probe pass in the forward.  Inference (no
        # gradient wanted): a probe pass + selection on the device.
        training = any(ctx.needs_input_grad)
        probe = None
        if training:
            flags |= dcn_offset_stats.forward_halo(weight, Co) << 10
        elif stride == 1 and dilation == 1:
            probe = torch.zeros(8, dtype=torch.int32, device=x.device)
        _lib.check(L.rvsr_dcn_pack_forward(_p(x), _p(weight), _p(bias), _p(om), _p(out), B, C, H, W, Co, stride,
                                           padding, dilation, dg, act | flags, slope, _p(probe), _p(ws), ws.numel(), _stream()),
                   'dcn_pack_forward')
        ctx.cfg = (stride, padding, dilation, dg, act, slope, bias is not None)
        ctx.save_for_backward(x, om, weight, out if act != ACT_NONE else None)
        ctx.bias_p = bias   # only to find its gradient buffer (_pgrad)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, om, weight, act_out = ctx.saved_tensors
        stride, padding, dilation, dg, act, slope, has_bias = ctx.cfg
        gout = gout.contiguous()
        B, C, H, W = x.shape
        Co = weight.shape[0]
        dep = ctx.sink.get(x) if ctx.sink is not None else None
        gx = dep if dep is not None else torch.zeros_like(x)
        gom = torch.empty_like(om)
        gw = _pgrad(weight, zero=True)   # (the DCN backward accumulates into grad_weight / grad_bias)
        gb = _pgrad(ctx.bias_p, zero=True) if has_bias else None
        L = _lib.lib()
        nbytes = L.rvsr_modulated_deform_conv_backward_workspace_bytes(B, C, H, W, Co, stride, padding, dilation)
        ws = _workspace(nbytes, x.device)
        gslope = 0.0 if act == ACT_RELU else slope
        # offset counters of this layer: the backward selects its window halo from them on the device, and a copy travels to the host
        # (asynchronously; the next forward of this layer waits for it) for the forward of the next step
        probe = None
        if stride == 1 and dilation == 1 and C % (8 * dg) == 0:
            probe = torch.zeros(8, dtype=torch.int32, device=x.device)
            _lib.check(L.rvsr_dcn_offset_probe(_p(om), B, om.shape[2], om.shape[3], dg, _p(probe), _stream()), 'dcn_offset_probe')
            dcn_offset_stats.record(weight, probe, L.rvsr_dcn_probe_samples(B, dg, om.shape[2], om.shape[3]))
        _lib.check(L.rvsr_dcn_pack_backward(_p(x), _p(weight), _p(om), _p(gout), _p(act_out), gslope, _p(gx), _p(gw),
                                            _p(gb), _p(gom), B, C, H, W, Co, stride, padding, dilation, dg, _p(probe), _p(ws),
                                            ws.numel(), _stream()), 'dcn_pack_backward')
        return (None if dep is not None else gx), gom, gw, gb, None, None, None, None, None, None, None


def dcn_pack(x, om, weight, bias, stride, padding, dilation, deformable_groups, act=ACT_NONE, slope=0.1, sink=None):
    return _DcnPackFused.apply(x, om, weight, bias, stride, padding, dilation, deformable_groups, act, slope, sink)


# ------------------------------------------------------------------------------------------ resampling / fusion
class _UpsampleBilinear(Function):
    @staticmethod
    def forward(ctx, x, factor, scale):
        _need_cuda(x)
        x = x.contiguous()
        B, C, H, W = x.shape
        out = x.new_empty(B, C, H * factor, W * factor)
        _lib.check(_lib.lib().rvsr_upsample_bilinear_forward(_p(x), _p(out), B * C, H, W, factor, scale, _stream()),
                   'upsample_bilinear_forward')
        ctx.cfg = (factor, scale, B, C, H, W)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        factor, scale, B, C, H, W = ctx.cfg
        gout = gout.contiguous()
        gin = gout.new_empty(B, C, H, W)
        _lib.check(_lib.lib().rvsr_upsample_bilinear_backward(_p(gout), _p(gin), B * C, H, W, factor, scale, _stream()),
                   'upsample_bilinear_backward')
        return gin, None, None


def upsample_bilinear(x, factor=2, scale=1.0):
    """scale * F.interpolate(x, scale_factor=factor, mode='bilinear', align_corners=False)"""
    return _UpsampleBilinear.apply(x, factor, float(scale))


class _MaxAvgPool(Function):
    @staticmethod
    def forward(ctx, x):
        _need_cuda(x)
        x = x.contiguous()
        B, C, H, W = x.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        out = x.new_empty(B, 2 * C, Ho, Wo)
        arg = torch.empty(B, C, Ho, Wo, dtype=torch.uint8, device=x.device)
        _lib.check(_lib.lib().rvsr_maxavgpool_forward(_p(x), _p(out), _p(arg), B, C, H, W, _stream()), 'maxavgpool_forward')
        ctx.cfg = (B, C, H, W)
        ctx.save_for_backward(arg)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        (arg,) = ctx.saved_tensors
        B, C, H, W = ctx.cfg
        gout = gout.contiguous()
        gin = gout.new_empty(B, C, H, W)
        _lib.check(_lib.lib().rvsr_maxavgpool_backward(_p(gout), _p(arg), _p(gin), B, C, H, W, _stream()),
                   'maxavgpool_backward')
        return gin


def maxavgpool(x):
    """cat([max_pool2d(x, 3, 2, 1), avg_pool2d(x, 3, 2, 1)], 1)"""
    return _MaxAvgPool.apply(x)


class _TSATemporal(Function):
    @staticmethod
    def forward(ctx, emb, emb_ref, aligned):
        _need_cuda(emb, emb_ref, aligned)
        emb, emb_ref, aligned = emb.contiguous(), emb_ref.contiguous(), aligned.contiguous()
        B, N, C, H, W = aligned.shape
        mod = aligned.new_empty(B, N * C, H, W)
        prob = aligned.new_empty(B, N, H, W)
        _lib.check(_lib.lib().rvsr_tsa_temporal_forward(_p(emb), _p(emb_ref), _p(aligned), _p(mod), _p(prob), B, N, C,
                                                        H, W, 0, _stream()), 'tsa_temporal_forward')
        ctx.save_for_backward(emb, emb_ref, aligned, prob)
        return mod

    @staticmethod
    @once_differentiable
    def backward(ctx, gmod):
        emb, emb_ref, aligned, prob = ctx.saved_tensors
        B, N, C, H, W = aligned.shape
        gmod = gmod.contiguous()
        galigned, gemb, gemb_ref = torch.empty_like(aligned), torch.empty_like(emb), torch.empty_like(emb_ref)
        _lib.check(_lib.lib().rvsr_tsa_temporal_backward(_p(gmod), _p(emb), _p(emb_ref), _p(aligned), _p(prob),
                                                         _p(galigned), _p(gemb), _p(gemb_ref), B, N, C, H, W, 0,
                                                         _stream()), 'tsa_temporal_backward')
        return gemb, gemb_ref, galigned


def tsa_temporal(emb, emb_ref, aligned):
    """aligned * sigmoid(sum_c emb * emb_ref), returned as (B, N*C, H, W)"""
    return _TSATemporal.apply(emb, emb_ref, aligned)


class _TSATemporalBlock(Function):
    """The temporal-attention front of TSA_Fusion (EDVR_arch.py:171-181) as ONE autograd node on the frame-major batch the
    alignment stage produces: emb = tAtt_1(aligned), emb_ref = tAtt_2(aligned[center]), mod[b, n*C + c] =
    aligned[n, b, c] * sigmoid(<emb[n, b], emb_ref[b]>).  `aligned` is [N, B, C, H, W]; no stack / transposing copy.
    Backward writes the gradient of `aligned` exactly once: the modulation gradient, then tAtt_1's data gradient with that
    buffer as its fused residual, then tAtt_2's into the centre block (three full-size autograd adds, a zero fill and two
    590 MB transposes per step at config 2 otherwise)."""

    @staticmethod
    def forward(ctx, aligned, center, w1, b1, w2, b2):
        _need_cuda(aligned, w1, b1, w2, b2)
        aligned, w1, b1, w2, b2 = _c(aligned), _c(w1), _c(b1), _c(w2), _c(b2)
        N, B, C, H, W = aligned.shape
        if tuple(w1.shape) != (C, C, 3, 3) or tuple(w2.shape) != (C, C, 3, 3):
            raise RuntimeError('tsa_temporal_block: expected two %dx%dx3x3 convs' % (C, C))
        emb = aligned.new_empty(N, B, C, H, W)
        emb_ref = aligned.new_empty(B, C, H, W)
        _conv(aligned, w1, emb, bias=b1, what='tsa tAtt_1')
        _conv(aligned[center], w2, emb_ref, bias=b2, what='tsa tAtt_2')
        mod = aligned.new_empty(B, N * C, H, W)
        prob = aligned.new_empty(B, N, H, W)
        _lib.check(_lib.lib().rvsr_tsa_temporal_forward(_p(emb), _p(emb_ref), _p(aligned), _p(mod), _p(prob), B, N, C, H, W, 1, _stream()),
                   'tsa_temporal_forward')
        ctx.center = center
        ctx.bias_p = (b1, b2)   # only to find their gradient buffers (_pgrad)
        ctx.save_for_backward(aligned, emb, emb_ref, prob, w1, w2)
        return mod

    @staticmethod
    @once_differentiable
    def backward(ctx, gmod):
        aligned, emb, emb_ref, prob, w1, w2 = ctx.saved_tensors
        N, B, C, H, W = aligned.shape
        center = ctx.center
        gmod = gmod.contiguous()
        galigned, gemb, gemb_ref = torch.empty_like(aligned), torch.empty_like(emb), torch.empty_like(emb_ref)
        _lib.check(_lib.lib().rvsr_tsa_temporal_backward(_p(gmod), _p(emb), _p(emb_ref), _p(aligned), _p(prob), _p(galigned), _p(gemb),
                                                         _p(gemb_ref), B, N, C, H, W, 1, _stream()), 'tsa_temporal_backward')
        gw1 = gb1 = gw2 = gb2 = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            gw1, gb1 = _wgrad(aligned, gemb, w1, ctx.bias_p[0], what='tsa wgrad tAtt_1')
        if ctx.needs_input_grad[4] or ctx.needs_input_grad[5]:
            gw2, gb2 = _wgrad(aligned[center], gemb_ref, w2, ctx.bias_p[1], what='tsa wgrad tAtt_2')
        if ctx.needs_input_grad[0]:
            # galigned += dgrad(tAtt_1)(gemb), in place: the kernel's fused residual is its own output buffer (every lane reads
            # the residual values of exactly the addresses it then stores)
            _conv(gemb, w1, galigned, transposed=True, residual=galigned, what='tsa dgrad tAtt_1')
            gcen = galigned[center]
            _conv(gemb_ref, w2, gcen, transposed=True, residual=gcen, what='tsa dgrad tAtt_2')
        else:
            galigned = None
        return galigned, None, gw1, gb1, gw2, gb2


def tsa_temporal_block(aligned_nb, center, tAtt_1, tAtt_2):
    """aligned_nb: [N, B, C, H, W] frame-major -> modulated features [B, N*C, H, W]"""
    return _TSATemporalBlock.apply(aligned_nb, int(center), tAtt_1.weight, tAtt_1.bias, tAtt_2.weight, tAtt_2.bias)


class _TSAOutput(Function):
    @staticmethod
    def forward(ctx, fea, att, att_add):
        _need_cuda(fea, att, att_add)
        fea, att, att_add = fea.contiguous(), att.contiguous(), att_add.contiguous()
        out = torch.empty_like(fea)
        _lib.check(_lib.lib().rvsr_tsa_output_forward(_p(fea), _p(att), _p(att_add), _p(out), fea.numel(), _stream()),
                   'tsa_output_forward')
        ctx.save_for_backward(fea, att)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        fea, att = ctx.saved_tensors
        g = g.contiguous()
        gfea, gatt = torch.empty_like(fea), torch.empty_like(att)
        _lib.check(_lib.lib().rvsr_tsa_output_backward(_p(g), _p(fea), _p(att), _p(gfea), _p(gatt), fea.numel(),
                                                       _stream()), 'tsa_output_backward')
        return gfea, gatt, g


def tsa_output(fea, att, att_add):
    """fea * sigmoid(att) * 2 + att_add"""
    return _TSAOutput.apply(fea, att, att_add)


# ------------------------------------------------------------------------------------------ pyramid / loss
class _PyrDown(Function):
    @staticmethod
    def forward(ctx, x):
        _need_cuda(x)
        x = x.contiguous()
        B, C, H, W = x.shape
        out = x.new_empty(B, C, (H + 1) // 2, (W + 1) // 2)
        _lib.check(_lib.lib().rvsr_pyr_down_forward(_p(x), _p(out), B * C, H, W, _stream()), 'pyr_down_forward')
        ctx.cfg = (B, C, H, W)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        B, C, H, W = ctx.cfg
        gout = gout.contiguous()
        gin = gout.new_empty(B, C, H, W)
        _lib.check(_lib.lib().rvsr_pyr_down_backward(_p(gout), _p(gin), B * C, H, W, _stream()), 'pyr_down_backward')
        return gin


def pyr_down(x):
    """downsample(conv_gauss(x, gauss_kernel)) (utils/util.py:503-510)"""
    return _PyrDown.apply(x)


class _PyrUpDiff(Function):
    @staticmethod
    def forward(ctx, cur, down):
        _need_cuda(cur, down)
        cur, down = cur.contiguous(), down.contiguous()
        B, C, H, W = cur.shape
        if tuple(down.shape) != (B, C, H // 2, W // 2) or H % 2 or W % 2:
            # same failure the reference hits as a shape mismatch in `current - up` (utils/util.py:550)
            raise RuntimeError('pyramid level %s cannot be rebuilt from %s' % (tuple(cur.shape), tuple(down.shape)))
        out = torch.empty_like(cur)
        _lib.check(_lib.lib().rvsr_pyr_updiff_forward(_p(cur), _p(down), _p(out), B * C, H, W, _stream()),
                   'pyr_updiff_forward')
        ctx.cfg = (B, C, H, W)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        B, C, H, W = ctx.cfg
        gout = gout.contiguous()
        gdown = gout.new_empty(B, C, H // 2, W // 2)
        _lib.check(_lib.lib().rvsr_pyr_updiff_backward(_p(gout), _p(gdown), B * C, H, W, _stream()),
                   'pyr_updiff_backward')
        return gout, gdown


def pyr_updiff(cur, down):
    """cur - upsample(down) (utils/util.py:513-516,548-551)"""
    return _PyrUpDiff.apply(cur, down)


def _reduce_workspace(device):
    return _workspace(_lib.lib().rvsr_reduce_workspace_bytes(), device)


def _scalar_loss(x, n, mean=True):
    """What a scalar-loss forward starts from: the 0-d output, the reduction workspace, and the scale of the sum (1 / n for a mean)."""
    return x.new_empty(()), _reduce_workspace(x.device), (1.0 / n if mean else 1.0)


def _pair_grads(ctx, gx):
    """(gx, gy) of a loss of x - y: the second operand's gradient is the negated first, formed only when wanted."""
    return gx, (-gx if ctx.needs_input_grad[1] else None)


class _Charbonnier(Function):
    @staticmethod
    def forward(ctx, x, y, eps, mean):
        _need_cuda(x, y)
        x, y = x.contiguous(), y.contiguous()
        n = x.numel()
        out, ws, scale = _scalar_loss(x, n, mean)
        _lib.check(_lib.lib().rvsr_charbonnier_forward(_p(x), _p(y), n, eps, scale, _p(out), _p(ws), _stream()),
                   'charbonnier_forward')
        ctx.cfg = (eps, scale)
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        eps, scale = ctx.cfg
        g = g.contiguous()
        gx = torch.empty_like(x)
        _lib.check(_lib.lib().rvsr_charbonnier_backward(_p(x), _p(y), _p(g), scale, eps, _p(gx), x.numel(), _stream()),
                   'charbonnier_backward')
        return (*_pair_grads(ctx, gx), None, None)


def charbonnier(x, y, eps=1e-6, reduction='mean'):
    return _Charbonnier.apply(x, y, float(eps), reduction == 'mean')


class _GWLoss(Function):
    @staticmethod
    def forward(ctx, x1, x2, w, mean):
        _need_cuda(x1, x2)
        x1, x2 = x1.contiguous(), x2.contiguous()
        B, C, H, W = x1.shape
        out, ws, scale = _scalar_loss(x1, x1.numel(), mean)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        fac = x1.new_empty(3, B, C, H, W) if need else None
        _lib.check(_lib.lib().rvsr_gwloss_forward(_p(x1), _p(x2), B * C, H, W, float(w), scale, _p(out),
                                         _p(fac[0]) if need else None, _p(fac[1]) if need else None,
                                         _p(fac[2]) if need else None, _p(ws), _stream()), 'gwloss_forward')
        ctx.cfg = (scale, B, C, H, W)
        ctx.save_for_backward(fac)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (fac,) = ctx.saved_tensors
        scale, B, C, H, W = ctx.cfg
        g = g.contiguous()
        gx = fac.new_empty(B, C, H, W)
        _lib.check(_lib.lib().rvsr_gwloss_backward(_p(fac[0]), _p(fac[1]), _p(fac[2]), _p(g), scale, _p(gx), B * C, H, W,
                                                   _stream()), 'gwloss_backward')
        return (*_pair_grads(ctx, gx), None, None)


def gw_loss(x1, x2, w=4, reduction='mean'):
    """Gradient-weighted loss (codes/models/loss.py:54-80), one fused pass."""
    return _GWLoss.apply(x1, x2, float(w), reduction == 'mean')


class _PixelLoss(Function):
    """scale * sum f(x - y), f = |d| / d^2 / Huber / Charbonnier (rvsr_pixel_loss_*)."""

    @staticmethod
    def forward(ctx, x, y, mode, param, mean):
        _need_cuda(x, y)
        if x.shape != y.shape:
            raise RuntimeError('pixel loss: shapes %s and %s differ' % (tuple(x.shape), tuple(y.shape)))
        x, y = x.contiguous(), y.contiguous()
        n = x.numel()
        out, ws, scale = _scalar_loss(x, n, mean)
        _lib.check(_lib.lib().rvsr_pixel_loss_forward(_p(x), _p(y), n, mode, param, scale, _p(out), _p(ws), _stream()),
                   'pixel_loss_forward')
        ctx.cfg = (mode, param, scale)
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        mode, param, scale = ctx.cfg
        g = g.contiguous()
        gx = torch.empty_like(x)
        _lib.check(_lib.lib().rvsr_pixel_loss_backward(_p(x), _p(y), _p(g), mode, param, scale, _p(gx), x.numel(),
                                                       _stream()), 'pixel_loss_backward')
        return (*_pair_grads(ctx, gx), None, None, None)


PIX_L1, PIX_L2, PIX_HUBER, PIX_CHARBONNIER = 0, 1, 2, 3


def pixel_loss(x, y, mode, param=0.0, reduction='mean'):
    """nn.L1Loss / nn.MSELoss / HuberLoss(delta=param) / CharbonnierLoss(eps=param) as one reduction kernel."""
    return _PixelLoss.apply(x, y, int(mode), float(param), reduction == 'mean')


class _SSIMLoss(Function):
    """1 - mean(ssim_map(x, y)) with the 11x11 sigma-1.5 window (IQA_pytorch.SSIM(...)(x, y, as_loss=True))."""

    @staticmethod
    def forward(ctx, x, y):
        _need_cuda(x, y)
        if x.shape != y.shape or x.dim() != 4:
            raise RuntimeError('ssim: expected two equal (B, C, H, W) tensors, got %s and %s' % (tuple(x.shape), tuple(y.shape)))
        x, y = x.contiguous(), y.contiguous()
        B, C, H, W = x.shape
        out, ws, scale = _scalar_loss(x, max(B * C * (H - 10) * (W - 10), 1))
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        maps = x.new_empty(3, B * C, H - 10, W - 10) if need and H > 10 and W > 10 else None
        _lib.check(_lib.lib().rvsr_ssim_forward(_p(x), _p(y), B * C, H, W, scale, _p(out),
                                       _p(maps[0]) if maps is not None else None,
                                       _p(maps[1]) if maps is not None else None,
                                       _p(maps[2]) if maps is not None else None, _p(ws), _stream()), 'ssim_forward')
        ctx.cfg = (scale, B * C, H, W)
        ctx.save_for_backward(x, y, maps)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y, maps = ctx.saved_tensors
        scale, planes, H, W = ctx.cfg
        g = g.contiguous()
        L = _lib.lib()
        gx = gy = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            _lib.check(L.rvsr_ssim_backward(_p(x), _p(y), _p(maps[0]), _p(maps[1]), _p(maps[2]), _p(g), scale, _p(gx),
                                            planes, H, W, _stream()), 'ssim_backward')
        if ctx.needs_input_grad[1]:
            # SSIM is symmetric: the derivative maps w.r.t. the second image are those of ssim(y, x)
            tmp, ws, _ = _scalar_loss(x, 1)
            m2 = torch.empty_like(maps)
            _lib.check(L.rvsr_ssim_forward(_p(y), _p(x), planes, H, W, scale, _p(tmp), _p(m2[0]), _p(m2[1]), _p(m2[2]),
                                           _p(ws), _stream()), 'ssim_forward (swapped)')
            gy = torch.empty_like(y)
            _lib.check(L.rvsr_ssim_backward(_p(y), _p(x), _p(m2[0]), _p(m2[1]), _p(m2[2]), _p(g), scale, _p(gy), planes,
                                            H, W, _stream()), 'ssim_backward (swapped)')
        return gx, gy


def ssim_loss(x, y):
    return _SSIMLoss.apply(x, y)


class _ConvGauss(Function):
    @staticmethod
    def forward(ctx, x, gain):
        _need_cuda(x)
        x = x.contiguous()
        B, C, H, W = x.shape
        out = torch.empty_like(x)
        _lib.check(_lib.lib().rvsr_conv_gauss_forward(_p(x), _p(out), B * C, H, W, gain, _stream()), 'conv_gauss_forward')
        ctx.cfg = (B * C, H, W, gain)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        planes, H, W, gain = ctx.cfg
        gout = gout.contiguous()
        gin = torch.empty_like(gout)
        _lib.check(_lib.lib().rvsr_conv_gauss_backward(_p(gout), _p(gin), planes, H, W, gain, _stream()),
                   'conv_gauss_backward')
        return gin, None


def conv_gauss(x, gain=1.0):
    """conv_gauss(x, gain * gauss_kernel()) (utils/util.py:503-506)"""
    return _ConvGauss.apply(x, float(gain))


class _PyrUpsample(Function):
    @staticmethod
    def forward(ctx, x):
        _need_cuda(x)
        x = x.contiguous()
        B, C, H, W = x.shape
        out = x.new_empty(B, C, 2 * H, 2 * W)
        _lib.check(_lib.lib().rvsr_pyr_upsample_forward(_p(x), _p(out), B * C, H, W, _stream()), 'pyr_upsample_forward')
        ctx.cfg = (B, C, H, W)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        B, C, H, W = ctx.cfg
        gout = gout.contiguous()
        gin = gout.new_empty(B, C, H, W)
        _lib.check(_lib.lib().rvsr_pyr_upsample_backward(_p(gout), _p(gin), B * C, H, W, _stream()),
                   'pyr_upsample_backward')
        return gin


def pyr_upsample(x):
    """upsample(x) of the pyramid helpers (utils/util.py:513-516)"""
    return _PyrUpsample.apply(x)


# ------------------------------------------------------------------------------------------ optimizer / augmentation
def adam_step_(param, grad, exp_avg, exp_avg_sq, step_size, beta1, beta2, eps, weight_decay, bias_correction2_sqrt):
    """In-place Adam update of one flat f32 buffer (rvsr_adam_step); no autograd."""
    _need_cuda(param, grad, exp_avg, exp_avg_sq)
    n = param.numel()
    for t in (grad, exp_avg, exp_avg_sq):
        if t.numel() != n or not t.is_contiguous():
            raise RuntimeError('adam_step_: buffers must be contiguous and of equal length')
    with torch.cuda.device(param.device):
        _lib.check(_lib.lib().rvsr_adam_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), n, step_size, beta1, beta2,
                                             eps, weight_decay, bias_correction2_sqrt, _stream()), 'adam_step')


def augment_clips(im1, im2, perm=(0, 1, 2), box_mode=0, box=(0, 0, 0, 0), v=1.0, colour=None):
    """One pass over a clip pair [..., 3, H, W] (rvsr_augment_clips): channel permutation, CutBlur box paste
    (box = (y0, y1, x0, x1)), blend with a per-frame colour.  Returns two new tensors; no autograd (data path)."""
    _need_cuda(im1, im2, colour)
    if im1.shape != im2.shape or im1.dim() < 3 or im1.shape[-3] != 3:
        raise ValueError('augment_clips: expected two equal [..., 3, H, W] clips, got %s and %s'
                         % (tuple(im1.shape), tuple(im2.shape)))
    im1, im2 = im1.contiguous(), im2.contiguous()
    H, W = im1.shape[-2:]
    frames = im1.numel() // (3 * H * W)
    if colour is not None:
        colour = colour.contiguous()
        if colour.numel() != frames * 3:
            raise ValueError('augment_clips: colour must hold one value per (frame, channel)')
    out1, out2 = torch.empty_like(im1), torch.empty_like(im2)
    with torch.cuda.device(im1.device):
        _lib.check(_lib.lib().rvsr_augment_clips(_p(im1), _p(im2), _p(out1), _p(out2), _p(colour), frames, H, W,
                                                 int(perm[0]), int(perm[1]), int(perm[2]), int(box_mode), int(box[0]),
                                                 int(box[1]), int(box[2]), int(box[3]), float(v), _stream()),
                   'augment_clips')
    return out1, out2


# ------------------------------------------------------------------------------------------ GAN discriminator
class _BatchNormLReLU(Function):
    """lrelu(batch_norm(x), slope) as one operator (the BN -> LeakyReLU(0.2) pairs of discriminator_arch.PatchDiscriminator).
    Train mode: batch statistics, running statistics and num_batches_tracked updated on the device; eval: running statistics."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, num_batches_tracked, train, momentum, eps, slope):
        _need_cuda(x, weight, bias, running_mean, running_var)
        if num_batches_tracked is not None and (not num_batches_tracked.is_cuda or num_batches_tracked.dtype != torch.int64):
            raise TypeError('bn_lrelu: num_batches_tracked must be an int64 device tensor')
        x = x.contiguous()
        B, C, H, W = x.shape
        y = torch.empty_like(x)
        mean, invstd = x.new_empty(C), x.new_empty(C)
        L = _lib.lib()
        ws = _workspace(L.rvsr_bn_workspace_bytes(B, C, H * W), x.device)
        _lib.check(L.rvsr_bn_lrelu_forward(_p(x), _p(weight), _p(bias), _p(running_mean), _p(running_var), _p(num_batches_tracked), _p(y),
                                           _p(mean), _p(invstd), B, C, H * W, int(train), momentum, eps, slope, _p(ws), ws.numel(),
                                           _stream()), 'bn_lrelu_forward')
        ctx.cfg = (bool(train), slope)
        ctx.weight_p, ctx.bias_p = weight, bias
        ctx.save_for_backward(x, y, weight, mean, invstd)
        ctx.mark_non_differentiable(mean, invstd)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, y, weight, mean, invstd = ctx.saved_tensors
        train, slope = ctx.cfg
        B, C, H, W = x.shape
        gy = gy.contiguous()
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gw = _pgrad(ctx.weight_p) if ctx.needs_input_grad[1] else None
        gb = _pgrad(ctx.bias_p) if ctx.needs_input_grad[2] else None
        L = _lib.lib()
        ws = _workspace(L.rvsr_bn_workspace_bytes(B, C, H * W), x.device)
        _lib.check(L.rvsr_bn_lrelu_backward(_p(gy), _p(y), _p(x), _p(weight), _p(mean), _p(invstd), _p(gx), _p(gw), _p(gb), B, C, H * W,
                                            int(train), slope, _p(ws), ws.numel(), _stream()), 'bn_lrelu_backward')
        return gx, gw, gb, None, None, None, None, None, None, None


def batch_norm_lrelu(x, bn, slope=0.2):
    """lrelu(bn(x), slope) for an ``nn.BatchNorm2d`` ``bn`` with torch's train / eval semantics (running statistics tracked with
    ``bn.momentum``; num_batches_tracked += 1 per train-mode call)."""
    if bn.momentum is None:
        raise NotImplementedError('bn_lrelu: momentum=None (cumulative moving average) is not supported')
    use_batch = bn.training or bn.running_mean is None
    track = bn.training and bn.track_running_stats and bn.running_mean is not None
    rm = bn.running_mean if (track or not use_batch) else None
    rv = bn.running_var if (track or not use_batch) else None
    nbt = bn.num_batches_tracked if track else None
    return _BatchNormLReLU.apply(x, bn.weight, bn.bias, rm, rv, nbt, use_batch, float(bn.momentum), float(bn.eps), float(slope))


class _GANCriterion(Function):
    """mean(BCEWithLogits(a - shift, target)), shift = mean(b) (relativistic) or 0."""

    @staticmethod
    def forward(ctx, a, b, target):
        _need_cuda(a, b)
        a = a.contiguous()
        b = _c(b)
        out = a.new_empty(())
        saved = a.new_empty(2)
        scale = 1.0 / a.numel()
        nb = 0 if b is None else b.numel()
        _lib.check(_lib.lib().rvsr_gan_loss_forward(_p(a), a.numel(), _p(b), nb, target, scale, _p(out), _p(saved), _stream()),
                   'gan_loss_forward')
        ctx.cfg = (target, scale, nb, b.shape if b is not None else None)
        ctx.save_for_backward(a, saved)
        ctx.mark_non_differentiable(saved)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, saved = ctx.saved_tensors
        target, scale, nb, bshape = ctx.cfg
        g = g.contiguous()
        ga = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        gb = a.new_empty(bshape) if (nb and ctx.needs_input_grad[1]) else None
        if ga is None and gb is None:
            return None, None, None
        _lib.check(_lib.lib().rvsr_gan_loss_backward(_p(a), a.numel(), nb, _p(saved), _p(g), target, scale, _p(ga), _p(gb), _stream()),
                   'gan_loss_backward')
        return ga, gb, None


def gan_criterion(a, target, other=None):
    """``BCEWithLogitsLoss()(a, full_like(a, target))``; with ``other``: ``(a - mean(other), target)`` -- the relativistic term of
    RaGAN, the gradient reaching ``other`` through the mean (VideoSRGAN_AllPair_model_YCbCr_Split.py:253-258, 286-296)."""
    return _GANCriterion.apply(a, other, float(target))


# ------------------------------------------------------------------------------------------ channel attention (RCAN)
def _ca_forward(u, x, w1, b1, w2, b2, res_scale):
    """rvsr_channel_attention_forward on contiguous tensors: (out, pooled, hidden, gate); out = (x or 0) + res_scale * u * gate."""
    B, C, H, W = u.shape
    Cr = w1.shape[0]
    if tuple(w1.shape[:2]) != (Cr, C) or tuple(w2.shape[:2]) != (C, Cr) or w1.numel() != Cr * C or w2.numel() != C * Cr \
            or b1 is None or b2 is None or b1.numel() != Cr or b2.numel() != C:
        raise RuntimeError('channel_attention: expected biased 1x1 convs %d -> Cr -> %d, got weights %s and %s'
                           % (C, C, tuple(w1.shape), tuple(w2.shape)))
    if x is not None and x.shape != u.shape:
        raise RuntimeError('channel_attention: residual %s does not match %s' % (tuple(x.shape), tuple(u.shape)))
    out = torch.empty_like(u)
    pooled, hidden, gate = u.new_empty(B, C), u.new_empty(B, Cr), u.new_empty(B, C)
    L = _lib.lib()
    ws = _workspace(L.rvsr_channel_attention_workspace_bytes(B, C, H, W), u.device)
    _lib.check(L.rvsr_channel_attention_forward(_p(u), _p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(out), _p(pooled), _p(hidden), _p(gate),
                                                B, C, Cr, H, W, res_scale, _p(ws), ws.numel(), _stream()), 'channel_attention_forward')
    return out, pooled, hidden, gate


def _ca_backward(gout, u, w1, w2, pooled, hidden, gate, res_scale, gw1=None, gb1=None, gw2=None, gb2=None):
    """rvsr_channel_attention_backward: gu; the parameter gradients are written into the buffers given (None: not computed)."""
    B, C, H, W = u.shape
    gu = torch.empty_like(u)
    L = _lib.lib()
    ws = _workspace(L.rvsr_channel_attention_workspace_bytes(B, C, H, W), u.device)
    _lib.check(L.rvsr_channel_attention_backward(_p(gout), _p(u), _p(w1), _p(w2), _p(pooled), _p(hidden), _p(gate), _p(gu), _p(gw1), _p(gb1),
                                                 _p(gw2), _p(gb2), B, C, w1.shape[0], H, W, res_scale, _p(ws), ws.numel(), _stream()),
               'channel_attention_backward')
    return gu


class _ChannelAttention(Function):
    """(x or 0) + res_scale * u * sigmoid(conv_up(relu(conv_down(mean_hw u)))) as one operator (RCAN_arch.py:30-70): four passes over the
    tensor forward and four backward instead of the ~10 each of the composed torch ops."""

    @staticmethod
    def forward(ctx, u, x, w1, b1, w2, b2, res_scale):
        _need_cuda(u, x, w1, b1, w2, b2)
        u, x, w1, b1, w2, b2 = _c(u), _c(x), _c(w1), _c(b1), _c(w2), _c(b2)
        out, pooled, hidden, gate = _ca_forward(u, x, w1, b1, w2, b2, res_scale)
        ctx.res_scale, ctx.has_x = res_scale, x is not None
        ctx.params = (w1, b1, w2, b2)   # only to find their gradient buffers (_pgrad)
        ctx.save_for_backward(u, w1, w2, pooled, hidden, gate)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        u, w1, w2, pooled, hidden, gate = ctx.saved_tensors
        gout = gout.contiguous()
        need = ctx.needs_input_grad
        gu = None
        g = [None, None, None, None]
        if need[0] or any(need[2:6]):
            g = [_pgrad(p) if need[2 + i] else None for i, p in enumerate(ctx.params)]
            gu = _ca_backward(gout, u, w1, w2, pooled, hidden, gate, ctx.res_scale, *g)
        return (gu if need[0] else None), (gout if ctx.has_x and need[1] else None), g[0], g[1], g[2], g[3], None


def channel_attention(u, conv_down, conv_up, x=None, res_scale=1.0):
    """RCAN's ChannelAttention driven by its two 1x1 ``nn.Conv2d`` holders, with the residual add of RCAB fused:
    out = (x or 0) + res_scale * u * sigmoid(conv_up(relu(conv_down(avg_pool(u)))))."""
    return _ChannelAttention.apply(u, x, conv_down.weight, conv_down.bias, conv_up.weight, conv_up.bias, float(res_scale))


class _RCABFused(Function):
    """x + res_scale * CA(conv2(relu(conv1(x)))) as ONE autograd node (RCAB, RCAN_arch.py:51-70), built the way _ResBlockFused is: forward
    is conv1 + ReLU, conv2, and the channel-attention operator with x as its fused residual; backward takes gu from the channel-attention
    backward, then runs the residual block's chain on it -- conv1's data-gradient kernel adds gout as its fused residual, so the identity
    gradient costs no pass of its own."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, wd, bd, wu, bu, res_scale):
        _need_cuda(x, w1, b1, w2, b2, wd, bd, wu, bu)
        x, w1, b1, w2, b2, wd, bd, wu, bu = _c(x), _c(w1), _c(b1), _c(w2), _c(b2), _c(wd), _c(bd), _c(wu), _c(bu)
        B, C, H, W = x.shape
        if w1.shape != (C, C, 3, 3) or w2.shape != (C, C, 3, 3):
            raise RuntimeError('rcab: expected two %dx%dx3x3 convs' % (C, C))
        h, u = torch.empty_like(x), torch.empty_like(x)
        _conv(x, w1, h, bias=b1, act=ACT_RELU, what='rcab conv1')
        _conv(h, w2, u, bias=b2, what='rcab conv2')
        out, pooled, hidden, gate = _ca_forward(u, x, wd, bd, wu, bu, res_scale)
        ctx.save_for_backward(x, h, u, w1, w2, wd, wu, pooled, hidden, gate)
        ctx.res_scale = res_scale
        ctx.params = (b1, b2, wd, bd, wu, bu)   # only to find their gradient buffers (_pgrad)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, h, u, w1, w2, wd, wu, pooled, hidden, gate = ctx.saved_tensors
        b1, b2, wd_p, bd_p, wu_p, bu_p = ctx.params
        gout = gout.contiguous()
        need = ctx.needs_input_grad
        if not any(need[:9]):
            return (None,) * 10
        gca = [_pgrad(p) if need[5 + i] else None for i, p in enumerate((wd_p, bd_p, wu_p, bu_p))]
        gu = _ca_backward(gout, u, wd, wu, pooled, hidden, gate, ctx.res_scale, *gca)
        return (*_res_chain_backward('rcab', gu, gout, x, h, w1, b1, w2, b2, need[:5]), *gca, None)


def rcab(x, conv1, conv2, conv_down, conv_up, res_scale=1.0):
    """x + res_scale * channel_attention(conv2(relu(conv1(x)))) with the identity add fused in both directions."""
    return _RCABFused.apply(x, conv1.weight, conv1.bias, conv2.weight, conv2.bias, conv_down.weight, conv_down.bias, conv_up.weight,
                            conv_up.bias, float(res_scale))


# ------------------------------------------------------------------------------------------ FSTRN: frame-major 3-D convs, PReLU, FRB
# Activations are FRAME-MAJOR, [T, B, C, H, W] contiguous: a range of frames is a contiguous batch for the [..., C, H, W] kernels above, and
# the three temporal taps of a pixel are three pointers one frame apart (csrc/conv3d_kernels.hip).
_FUSE_TCONV3 = True   # off: the (3,1,1) convolution composed from three 1x1 convs over frame ranges -- the fallback and the yardstick


def _c3_wgrad(x, gout, weight, bias, taps, what):
    """(gw, gb) of a kernel-3-in-time convolution with weight (Co, Ci, 3, k, k), into the parameters' gradient buffers: the 2-D
    weight-gradient kernel once per tap over the frame range the tap meets (deterministic partial sums), scattered into the dt slices.
    The first tap covers every output frame and carries the bias gradient; a tap that meets no frame (T == 1) gets zeros."""
    gw = _pgrad(weight)
    gb = _pgrad(bias) if bias is not None else None
    tmp = gw.new_empty(gw.shape[0], gw.shape[1], *gw.shape[3:])
    for i, (dt, a, n, o) in enumerate(taps):
        _conv_wgrad(x[a:a + n], gout[o:o + n], tmp, gb if i == 0 else None, what=what)
        gw[:, :, dt].copy_(tmp)
    for dt in set(range(3)) - {t[0] for t in taps}:
        gw[:, :, dt].zero_()
    return gw, gb


def _c3_taps(T, f0, f1):
    """The temporal taps of a kernel-3 / padding-1 convolution evaluated at output frames [f0, f1) of T input frames, as
    (dt, first input frame, frames, first output frame relative to f0).  The centre tap comes first: it covers every output frame, so
    it WRITES the output and the outer taps accumulate onto it."""
    taps = []
    for dt in (1, 0, 2):
        a, b = max(f0 + dt - 1, 0), min(f1 + dt - 1, T)
        if b > a:
            taps.append((dt, a, b - a, a - dt + 1 - f0))
    return taps


class _Conv3dFrames(Function):
    """nn.Conv3d(Ci, Co, (3, k, k), padding (1, k // 2, k // 2)) at output frames [f0, f1) [+ residual], as accumulated 2-D convolutions
    over frame ranges with the weight slices w[:, :, dt]; an accumulating call takes its own output buffer as the fused residual."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, f0, f1):
        _need_cuda(x, weight, bias, residual)
        x, weight, bias, residual = _c(x), _c(weight), _c(bias), _c(residual)
        T, B, Ci, H, W = x.shape
        Co, Cw, kt, k, k2 = weight.shape
        if Cw != Ci or kt != 3 or k != k2 or not 0 <= f0 < f1 <= T:
            raise RuntimeError('conv3d_frames: x %s, weight %s, frames [%d, %d) do not fit' % (tuple(x.shape), tuple(weight.shape), f0, f1))
        out = x.new_empty(f1 - f0, B, Co, H, W)
        if residual is not None and residual.shape != out.shape:
            raise RuntimeError('conv3d_frames: residual %s does not match %s' % (tuple(residual.shape), tuple(out.shape)))
        wdt = [weight[:, :, dt].contiguous() for dt in range(3)]
        for i, (dt, a, n, o) in enumerate(_c3_taps(T, f0, f1)):
            dst = out[o:o + n]
            _conv(x[a:a + n], wdt[dt], dst, bias=bias if i == 0 else None, residual=residual if i == 0 else dst, what='conv3d_frames')
        ctx.cfg = (f0, f1, bias is not None, residual is not None)
        ctx.params = (weight, bias)   # only to find their gradient buffers (_pgrad)
        ctx.save_for_backward(x, *wdt)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, *wdt = ctx.saved_tensors
        f0, f1, has_bias, has_res = ctx.cfg
        weight, bias = ctx.params
        gout = gout.contiguous()
        T = x.shape[0]
        taps = _c3_taps(T, f0, f1)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            # the centre tap writes frames [f0, f1); frames outside that only an outer tap reaches start from zero
            gx = torch.empty_like(x) if (f0, f1) == (0, T) else torch.zeros_like(x)
            for i, (dt, a, n, o) in enumerate(taps):
                dst = gx[a:a + n]
                _conv(gout[o:o + n], wdt[dt], dst, transposed=True, residual=None if i == 0 else dst, what='conv3d_frames dgrad')
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            gw, gb = _c3_wgrad(x, gout, weight, bias, taps, 'conv3d_frames wgrad')
        return gx, gw, gb, (gout if has_res else None), None, None


def conv3d_frames(x, conv3d, frames=None, residual=None):
    """A 3 x k x k ``nn.Conv3d`` (padding 1 in time, k // 2 in space) on frame-major x [T, B, C, H, W] at the output frames
    ``frames = (f0, f1)`` (None: all) [+ residual]: returns [f1 - f0, B, Co, H, W]."""
    f0, f1 = (0, x.shape[0]) if frames is None else frames
    return _Conv3dFrames.apply(x, conv3d.weight, conv3d.bias, residual, int(f0), int(f1))


def _slope(t):
    if t is not None and t.numel() != 1:
        raise NotImplementedError('prelu: one slope per channel is not on the MI355X path; nn.PReLU() (one slope) is')
    return t


def _prelu_forward(a, b, slope, keep=None, scale=1.0):
    """rvsr_prelu_forward: prelu(a [+ b]) [* keep * scale]; keep: a bool / uint8 tensor of a's shape."""
    y = torch.empty_like(a)
    _lib.check(_lib.lib().rvsr_prelu_forward(_p(a), _p(b), _p(slope), _p(keep), scale, _p(y), a.numel(), _stream()), 'prelu_forward')
    return y


def _prelu_backward(g, a, b, slope, keep=None, scale=1.0, gres=None, gslope=None, need_gx=True):
    """rvsr_prelu_backward: gx = g * [keep * scale] * prelu'(a [+ b]) [+ gres]; the slope gradient is written into `gslope` (None: not
    computed)."""
    gx = torch.empty_like(a) if need_gx else None
    L = _lib.lib()
    ws = _workspace(L.rvsr_prelu_workspace_bytes(), a.device)
    _lib.check(L.rvsr_prelu_backward(_p(g), _p(a), _p(b), _p(slope), _p(keep), scale, _p(gres), _p(gx), _p(gslope), a.numel(), _p(ws), ws.numel(),
                                     _stream()), 'prelu_backward')
    return gx


def _keep_bytes(keep, like):
    if keep is None:
        return None
    if keep.dtype not in (torch.bool, torch.uint8) or keep.shape != like.shape or keep.device != like.device:
        raise RuntimeError('prelu: keep must be a bool / uint8 tensor of shape %s on %s' % (tuple(like.shape), like.device))
    return keep.contiguous()


class _PReLU(Function):
    """prelu(a [+ b]) [* keep * scale] in one pass; the gradient of a is also that of b."""

    @staticmethod
    def forward(ctx, a, b, slope, keep, scale):
        _need_cuda(a, b, slope)
        a, b, slope, keep = _c(a), _c(b), _c(_slope(slope)), _keep_bytes(keep, a)
        if b is not None and b.shape != a.shape:
            raise RuntimeError('prelu: the second addend %s does not match %s' % (tuple(b.shape), tuple(a.shape)))
        ctx.scale, ctx.has_b, ctx.slope_p = scale, b is not None, slope
        ctx.save_for_backward(a, b, slope, keep)
        return _prelu_forward(a, b, slope, keep, scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b, slope, keep = ctx.saved_tensors
        need_x = ctx.needs_input_grad[0] or (ctx.has_b and ctx.needs_input_grad[1])
        gslope = _pgrad(ctx.slope_p) if ctx.needs_input_grad[2] else None
        gx = None
        if need_x or gslope is not None:
            gx = _prelu_backward(g.contiguous(), a, b, slope, keep, ctx.scale, gslope=gslope, need_gx=need_x)
        return (gx if ctx.needs_input_grad[0] else None), (gx if ctx.has_b and ctx.needs_input_grad[1] else None), gslope, None, None


def prelu(x, prelu_mod, b=None, keep=None, p=0.0):
    """``nn.PReLU()`` (one learnable slope, read on the device) of x [+ b], and -- with a keep mask -- ``nn.Dropout(p)`` of the result in
    the same pass: prelu(x + b) * keep * float32(1 / (1 - p))."""
    scale = float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)) if keep is not None else 1.0
    return _PReLU.apply(x, b, prelu_mod.weight, keep, scale)


def _tconv3_run(s, w, bias=None, residual=None, slope=None, transposed=False):
    """out [, pout] of rvsr_tconv3_forward on frame-major s [T, B, Ci, H, W]; w: the Conv3d weight (Co, Ci, 3, 1, 1), or with `transposed`
    the weight whose data gradient this is.  With _FUSE_TCONV3 off, or for channel counts the kernel refuses, the same result composed
    from three accumulated 1x1 convs over frame ranges (and a PReLU pass for pout)."""
    T, B, Ci, H, W = s.shape
    Co = w.shape[1] if transposed else w.shape[0]
    if w.shape[1 if not transposed else 0] != Ci or tuple(w.shape[2:]) != (3, 1, 1):
        raise RuntimeError('tconv3: s %s and weight %s do not fit' % (tuple(s.shape), tuple(w.shape)))
    out = s.new_empty(T, B, Co, H, W)
    if residual is not None and residual.shape != out.shape:
        raise RuntimeError('tconv3: residual %s does not match %s' % (tuple(residual.shape), tuple(out.shape)))
    pout = torch.empty_like(out) if slope is not None else None
    if _FUSE_TCONV3:
        rc = _lib.lib().rvsr_tconv3_forward(_p(s), _p(w), _p(bias), _p(residual), _p(slope), _p(out), _p(pout), T, B, Ci, Co, H, W,
                                            int(transposed), _stream())
        if rc == 0:
            return out, pout
        if rc != _lib.RVSR_ERR_UNSUPPORTED:   # channel counts the kernel does not take -- the composed path below
            _lib.check(rc, 'tconv3')
    for i, (dt, a, n, o) in enumerate(_c3_taps(T, 0, T)):
        dst = out[o:o + n]
        _conv(s[a:a + n], w[:, :, 2 - dt if transposed else dt].contiguous(), dst, bias=bias if i == 0 else None,
              residual=residual if i == 0 else dst, transposed=transposed, what='tconv3 (composed)')
    if pout is not None:
        pout = _prelu_forward(out, None, slope)
    return out, pout


def _tconv3_wgrad(s, gout, weight, bias):
    """(gw, gb) of the temporal convolution with weight (Co, Ci, 3, 1, 1): _c3_wgrad over all frames with the 1x1 kernel."""
    return _c3_wgrad(s, gout, weight, bias, _c3_taps(s.shape[0], 0, s.shape[0]), 'tconv3 wgrad')


class _TConv3(Function):
    """The (3,1,1) temporal convolution with bias [+ residual]; with a slope also pout = prelu(out) as a second output."""

    @staticmethod
    def forward(ctx, s, weight, bias, residual, slope):
        _need_cuda(s, weight, bias, residual, slope)
        s, weight, bias, residual, slope = _c(s), _c(weight), _c(bias), _c(residual), _c(_slope(slope))
        out, pout = _tconv3_run(s, weight, bias, residual, slope)
        ctx.cfg = (bias is not None, residual is not None, slope is not None)
        ctx.params = (weight, bias, slope)   # only to find their gradient buffers (_pgrad)
        ctx.save_for_backward(s, weight, slope, out if slope is not None else None)
        if slope is None:
            return out
        return out, pout

    @staticmethod
    @once_differentiable
    def backward(ctx, gout, gpout=None):
        s, weight, slope, out = ctx.saved_tensors
        has_bias, has_res, has_slope = ctx.cfg
        weight_p, bias_p, slope_p = ctx.params
        need = ctx.needs_input_grad
        g = gout.contiguous()
        gslope = None
        if has_slope:   # the gradient arriving at pout goes back through the PReLU and joins the gradient of out
            gslope = _pgrad(slope_p) if need[4] else None
            g = _prelu_backward(gpout.contiguous(), out, None, slope, gres=g, gslope=gslope)
        gs = gw = gb = None
        if need[0]:
            gs, _ = _tconv3_run(g, weight, transposed=True)
        if need[1] or (has_bias and need[2]):
            gw, gb = _tconv3_wgrad(s, g, weight_p, bias_p)
        return gs, gw, gb, (g if has_res and need[3] else None), gslope


def tconv3(s, conv3d, residual=None, prelu_mod=None):
    """A (3,1,1) ``nn.Conv3d`` (padding (1,0,0)) on frame-major s [T, B, C, H, W] [+ residual]; with ``prelu_mod`` (an ``nn.PReLU()``)
    returns (out, prelu(out)), the activation in the same kernel."""
    return _TConv3.apply(s, conv3d.weight, conv3d.bias, residual, None if prelu_mod is None else prelu_mod.weight)


class _FRBFused(Function):
    """x + conv3d_2(conv3d_1(prelu(x))) as ONE autograd node (FRB, FSTRN_arch.py:11-22) on frame-major x: the PReLU (unless `px`, its
    output, arrives from the previous block's kernel), the (1,3,3) convolution as a 3x3 convolution over T * B images, and the temporal
    convolution with x as its fused residual and -- given the NEXT block's slope -- that block's PReLU as a second output.  Backward: the
    gradient arriving at pout goes through the PReLU with gout as the fused skip gradient; the block's own PReLU backward adds the skip
    gradient the same way, so no identity gradient costs a pass of its own."""

    @staticmethod
    def forward(ctx, x, px, slope, w1, b1, w2, b2, next_slope):
        _need_cuda(x, px, slope, w1, b1, w2, b2, next_slope)
        x, px, slope, w1, b1, w2, b2, next_slope = _c(x), _c(px), _c(_slope(slope)), _c(w1), _c(b1), _c(w2), _c(b2), _c(_slope(next_slope))
        T, B, C, H, W = x.shape
        if tuple(w1.shape) != (C, C, 1, 3, 3) or tuple(w2.shape) != (C, C, 3, 1, 1):
            raise RuntimeError('frb: expected a %dx%dx(1,3,3) and a %dx%dx(3,1,1) conv, got %s and %s' % (C, C, C, C, tuple(w1.shape), tuple(w2.shape)))
        own = px is None
        if own:
            px = _prelu_forward(x, None, slope)
        w1s = w1[:, :, 0]   # (a view with the 2-D layout: the middle dimension has one element)
        h = torch.empty_like(x)
        _conv(px, w1s, h, bias=b1, what='frb conv3d_1')
        out, pout = _tconv3_run(h, w2, b2, x, next_slope)
        ctx.own, ctx.has_next = own, next_slope is not None
        ctx.params = (slope, w1, b1, w2, b2, next_slope)   # only to find their gradient buffers (_pgrad)
        ctx.save_for_backward(x if own else None, px, h, out if next_slope is not None else None, slope, w1, w2, next_slope)
        if next_slope is None:
            return out
        return out, pout

    @staticmethod
    @once_differentiable
    def backward(ctx, gout, gpout=None):
        x, px, h, out, slope, w1, w2, next_slope = ctx.saved_tensors
        slope_p, w1_p, b1_p, w2_p, b2_p, next_p = ctx.params
        need = ctx.needs_input_grad
        g = gout.contiguous()
        gnext = None
        if ctx.has_next:
            gnext = _pgrad(next_p) if need[7] else None
            g = _prelu_backward(gpout.contiguous(), out, None, next_slope, gres=g, gslope=gnext)
        gw1 = gb1 = gw2 = gb2 = gslope = gx = gpx = None
        if need[5] or need[6]:   # (the weight-gradient kernels produce weight and bias gradient in one call, as in the conv nodes above)
            gw2, gb2 = _tconv3_wgrad(h, g, w2_p, b2_p)
        # what lies below conv3d_2: the gradient of px, wanted by this block's own PReLU (for x or the slope) or by the previous block's node
        need_gpx = (need[0] or need[2]) if ctx.own else need[1]
        if need[3] or need[4] or need_gpx:
            gh, _ = _tconv3_run(g, w2, transposed=True)
            if need[3] or need[4]:
                gw1, gb1 = _wgrad(px, gh, w1_p, b1_p, what='frb wgrad1')   # ((C, C, 1, 3, 3): the 2-D layout)
            if need_gpx:
                gpx = torch.empty_like(px)
                _conv(gh, w1[:, :, 0], gpx, transposed=True, what='frb dgrad1')
        if ctx.own:   # through this block's own PReLU, the skip gradient added in the same pass
            if need_gpx:
                gslope = _pgrad(slope_p) if need[2] else None
                gx = _prelu_backward(gpx, x, None, slope, gres=g, gslope=gslope, need_gx=need[0])
            gpx = None
        elif need[0]:   # x and px are the two outputs of the previous block's node: the skip gradient and the PReLU's, separately
            gx = g
        gw1, gb1 = (gw1 if need[3] else None), (gb1 if need[4] else None)
        gw2, gb2 = (gw2 if need[5] else None), (gb2 if need[6] else None)
        return gx, gpx, gslope, gw1, gb1, gw2, gb2, gnext


def frb(x, prelu_mod, conv1, conv2, px=None, next_prelu=None):
    """One FRB on frame-major x [T, B, C, H, W]: x + conv2(conv1(prelu(x))).  px: prelu(x) when the previous block's kernel has already
    produced it; next_prelu: the next block's ``nn.PReLU()`` -- the call then returns (out, next_prelu(out))."""
    return _FRBFused.apply(x, px, None if px is not None else prelu_mod.weight, conv1.weight, conv1.bias, conv2.weight, conv2.bias,
                           None if next_prelu is None else next_prelu.weight)


class _ConvT1x1(Function):
    """``nn.ConvTranspose3d(Ci, Co, (1,1,1))`` on [..., Ci, H, W]: a 1x1 convolution with the transposed weight (Ci, Co, 1, 1, 1)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _need_cuda(x, weight, bias)
        x, weight, bias = _c(x), _c(weight), _c(bias)
        Ci, Co = weight.shape[:2]
        if x.shape[-3] != Ci or weight.numel() != Ci * Co:
            raise RuntimeError('conv_transpose1x1: x %s and weight %s do not fit' % (tuple(x.shape), tuple(weight.shape)))
        out = x.new_empty(*x.shape[:-3], Co, *x.shape[-2:])
        _conv(x, weight.view(Ci, Co, 1, 1), out, bias=bias, transposed=True, what='conv_transpose1x1')
        ctx.params = (weight, bias)   # only to find their gradient buffers (_pgrad)
        ctx.save_for_backward(x, weight)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, weight = ctx.saved_tensors
        weight_p, bias_p = ctx.params
        Ci, Co = weight.shape[:2]
        gout = gout.contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            _conv(gout, weight.view(Ci, Co, 1, 1), gx, what='conv_transpose1x1 dgrad')
        if ctx.needs_input_grad[1] or (bias_p is not None and ctx.needs_input_grad[2]):
            # the 1x1 weight-gradient kernel gives (Co, Ci) and the bias gradient of gout; the parameter is stored (Ci, Co)
            gwt = x.new_empty(Co, Ci, 1, 1)
            gb = _pgrad(bias_p) if bias_p is not None else None
            _conv_wgrad(x, gout, gwt, gb, what='conv_transpose1x1 wgrad')
            gw = _pgrad(weight_p)
            gw.view(Ci, Co).copy_(gwt.view(Co, Ci).t())
        return gx, gw, gb


def conv_transpose1x1(x, convt):
    """A kernel-1 / stride-1 ``nn.ConvTranspose3d`` (or 2d) on [..., C, H, W]."""
    if any(k != 1 for k in convt.kernel_size) or any(st != 1 for st in convt.stride):
        raise NotImplementedError('conv_transpose1x1: kernel %s / stride %s; only kernel 1, stride 1 is on the MI355X path'
                                  % (tuple(convt.kernel_size), tuple(convt.stride)))
    return _ConvT1x1.apply(x, convt.weight, convt.bias)


# ------------------------------------------------------------------------------------------ TOF: SpyNet's resampling operators
_WARP_INTERP = {'bilinear': 0, 'nearest': 1}
_WARP_PADDING = {'zeros': 0, 'border': 1}


class _FlowWarp(Function):
    """arch_util.flow_warp: grid_sample(align_corners=True) of x (B, C, H, W) at pixel + flow (B, H, W, 2)."""

    @staticmethod
    def forward(ctx, x, flow, interp, padding):
        _need_cuda(x, flow)
        x, flow = x.contiguous(), flow.contiguous()
        B, C, H, W = x.shape
        if tuple(flow.shape) != (B, H, W, 2):
            raise RuntimeError('flow_warp: x %s needs a flow of %s, got %s' % (tuple(x.shape), (B, H, W, 2), tuple(flow.shape)))
        out = torch.empty_like(x)
        _lib.check(_lib.lib().rvsr_flow_warp_forward(_p(x), _p(flow), _p(out), B, C, H, W, interp, padding, _stream()), 'flow_warp_forward')
        ctx.cfg = (interp, padding)
        ctx.save_for_backward(x, flow)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, flow = ctx.saved_tensors
        interp, padding = ctx.cfg
        B, C, H, W = x.shape
        gout = gout.contiguous()
        # either gradient is skipped when autograd wants none (TOF: the frames are data, gx is never needed); gx is accumulated atomically
        gx = torch.zeros_like(x) if ctx.needs_input_grad[0] else None
        gflow = torch.empty_like(flow) if ctx.needs_input_grad[1] else None
        _lib.check(_lib.lib().rvsr_flow_warp_backward(_p(gout), _p(x), _p(flow), _p(gx), _p(gflow), B, C, H, W, interp, padding, _stream()),
                   'flow_warp_backward')
        return gx, gflow, None, None


def flow_warp(x, flow, interp_mode='bilinear', padding_mode='zeros'):
    """F.grid_sample(x, normalised(pixel + flow), mode=interp_mode, padding_mode=padding_mode, align_corners=True): x (B, C, H, W), flow
    (B, H, W, 2) in pixels, x first.  'bilinear' / 'nearest' with 'zeros' / 'border'.  The flow gradient is deterministic; the image
    gradient is accumulated with float atomics (order-dependent in its last bits)."""
    if interp_mode not in _WARP_INTERP:
        raise NotImplementedError("flow_warp: interp_mode %r; 'bilinear' and 'nearest' are on the MI355X path" % (interp_mode,))
    if padding_mode not in _WARP_PADDING:
        raise NotImplementedError("flow_warp: padding_mode %r; 'zeros' and 'border' are on the MI355X path" % (padding_mode,))
    return _FlowWarp.apply(x, flow, _WARP_INTERP[interp_mode], _WARP_PADDING[padding_mode])


class _AvgPool2(Function):
    @staticmethod
    def forward(ctx, x):
        _need_cuda(x)
        x = x.contiguous()
        B, C, H, W = x.shape
        out = x.new_empty(B, C, H // 2, W // 2)
        _lib.check(_lib.lib().rvsr_avgpool2_forward(_p(x), _p(out), B * C, H, W, _stream()), 'avgpool2_forward')
        ctx.cfg = (B, C, H, W)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        B, C, H, W = ctx.cfg
        gout = gout.contiguous()
        gin = gout.new_empty(B, C, H, W)
        _lib.check(_lib.lib().rvsr_avgpool2_backward(_p(gout) if gout.numel() else None, _p(gin), B * C, H, W, _stream()), 'avgpool2_backward')
        return gin


def avg_pool2(x):
    """F.avg_pool2d(x, 2, 2): sizes floor, an odd last row or column takes no part."""
    return _AvgPool2.apply(x)


class _Upsample2AC(Function):
    @staticmethod
    def forward(ctx, x, scale):
        _need_cuda(x)
        x = x.contiguous()
        B, C, H, W = x.shape
        out = x.new_empty(B, C, 2 * H, 2 * W)
        _lib.check(_lib.lib().rvsr_upsample2_ac_forward(_p(x), _p(out), B * C, H, W, scale, _stream()), 'upsample2_ac_forward')
        ctx.cfg = (scale, B, C, H, W)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        scale, B, C, H, W = ctx.cfg
        gout = gout.contiguous()
        gin = gout.new_empty(B, C, H, W)
        _lib.check(_lib.lib().rvsr_upsample2_ac_backward(_p(gout), _p(gin), B * C, H, W, scale, _stream()), 'upsample2_ac_backward')
        return gin, None


def upsample2_ac(x, scale=1.0):
    """scale * F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True)"""
    return _Upsample2AC.apply(x, float(scale))


# ------------------------------------------------------------------------------------------ device guard
def _guarded(fn):
    """Run an operator on the device of its tensors: HIP launches go to the CURRENT device, and `_stream()` /
    `_workspace()` are the current device's, so a module living on cuda:1 while cuda:0 is current (DataParallel
    replicas, VideoSR_AllPair_model_YCbCr_Split.py:36; the reference's extension does the same with
    at::DeviceGuard, deform_conv_cuda.cpp:499,581) must switch first."""
    @functools.wraps(fn)
    def wrapper(ctx, *args):
        for a in args:
            if torch.is_tensor(a) and a.is_cuda:
                if a.device.index != torch.cuda.current_device():
                    with torch.cuda.device(a.device):
                        return fn(ctx, *args)
                break
        return fn(ctx, *args)
    return wrapper


for _cls in list(globals().values()):
    if isinstance(_cls, type) and issubclass(_cls, Function) and _cls is not Function:
        _cls.forward = staticmethod(_guarded(_cls.forward))
        _cls.backward = staticmethod(_guarded(_cls.backward))
