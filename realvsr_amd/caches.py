"""The two host-side caches of the operator glue (realvsr_amd.functional): the bf16 weight images packed once per optimizer step
(PackedWeights) and the per-layer DCN offset counters that pick the forward's tile halo (DcnOffsetStats)."""
import ctypes
import os
import weakref

import torch

from . import _lib
from ._lib import _p, _stream


def _version(t):
    """Version of the parameter a weight tensor stands for: its own, or its parent's for a cached input-channel slice."""
    parent = getattr(t, '_rvsr_parent', None)
    if parent is None:
        return t._version
    parent = parent()
    return -1 if parent is None else parent._version


class _Record:
    """What a cache record remembers of the weight it was made from."""
    __slots__ = ('ref', 'version', 'epoch', 'data_ptr')

    def stamp(self, weight, epoch):
        self.ref, self.version, self.epoch, self.data_ptr = weakref.ref(weight), _version(weight), epoch, weight.data_ptr()

    def stands_for(self, weight, epoch):
        """Whether this record is still valid for `weight`: the very same object, alive, with an unchanged version counter and unmoved
        storage, packed in `epoch`.  epoch=None leaves the epoch out: repack() asks right after the parameters were rewritten in place
        behind the version counter -- every record is then one epoch old by construction, and it is repack() that brings the survivors
        up to date."""
        return (weight is not None and self.ref() is weight and self.version == _version(weight)
                and self.data_ptr == weight.data_ptr() and (epoch is None or self.epoch == epoch))


class _Image(_Record):
    """One packed image: `buf` holds it, `desc` are the 10 descriptor values the pack entry reported."""
    __slots__ = ('buf', 'desc')

    def __init__(self, buf, desc, weight, epoch):
        self.buf, self.desc = buf, desc
        self.stamp(weight, epoch)

    def table_row(self):
        """The 48-byte PackDesc row of rvsr_pack_weights_batched (two pointers + eight 32-bit fields) as six int64."""
        d = self.desc
        return [d[0], d[1]] + [(d[2 + 2 * j] & 0xffffffff) | ((d[3 + 2 * j] & 0xffffffff) << 32) for j in range(4)]


class _SlicePair(_Record):
    """weight[:, :C1] and weight[:, C1:] as persistent contiguous tensors."""
    __slots__ = ('w_a', 'w_b')

    def __init__(self, weight, C1, epoch):
        self.w_a, self.w_b = weight[:, :C1].detach().contiguous(), weight[:, C1:].detach().contiguous()
        self.w_a._rvsr_parent = self.w_b._rvsr_parent = weakref.ref(weight)
        self.stamp(weight, epoch)

    def refresh(self, weight, C1, epoch):
        with torch.no_grad():
            self.w_a.copy_(weight[:, :C1])
            self.w_b.copy_(weight[:, C1:])
        self.stamp(weight, epoch)


class PackedWeights:
    """bf16 hi/lo weight images (what the conv / DCN kernels stage into LDS), packed ONCE per optimizer step.

    A conv block needs its weights re-packed ([m-block][chunk][hi|lo][tap][octet][row][8] bf16) -- once for the forward and once,
    transposed and flipped, for the data gradient.  The library does that per call into the workspace (~150 launches of a 5 us
    kernel per training step).  Here the images of parameters that live in optim.FlatBuffers are kept in their own tensors,
    the first use of an image packs it with one call (rvsr_conv2d_pack_weights / rvsr_dcn_pack_weights), and from then on
    ``FlatAdam.step`` re-packs ALL registered images with ONE launch (rvsr_pack_weights_batched) right after the update.
    Validity: an entry is used only while (a) the very same parameter object is alive, (b) its torch version counter is
    unchanged (load_state_dict, in-place edits under no_grad bump it) and (c) it was packed in the current epoch; everything
    that writes parameters behind torch's back (the flat Adam kernel, a broadcast into the flat buffer, a raw copy into it) must
    call ``repack()`` (re-pack now) or ``invalidate()`` (forget).  Foreign weights (not in FlatBuffers) take the per-call path.
    RVSR_PACK_CACHE=0 turns the cache off."""

    def __init__(self):
        self.entries = {}          # (id(weight), kind, C_in, Co, k, w_mode) -> _Image
        self.slices = {}           # (id(weight), C1) -> _SlicePair
        self.epoch = 0
        self.table = None          # device copy of the descriptor table, rebuilt when entries were added or dropped
        self.enabled = os.environ.get('RVSR_PACK_CACHE', '1') != '0'
        self.stats = {'hits': 0, 'packs': 0, 'batched': 0}

    def invalidate(self):
        self.entries.clear()
        self.slices.clear()
        self.table = None
        self.epoch += 1

    def split(self, weight, C1):
        """weight[:, :C1] and weight[:, C1:] as PERSISTENT contiguous tensors (conv_cat_bcast convolves the two halves of a concat
        conv separately): copied on first sight and after every optimizer step (repack), so that their packed images can be
        cached like those of whole parameters.  Falls back to fresh copies for weights outside FlatBuffers."""
        if not self.enabled or getattr(weight, '_rvsr_grad_home', None) is None:
            return weight[:, :C1].contiguous(), weight[:, C1:].contiguous()
        key = (id(weight), C1)
        e = self.slices.get(key)
        if e is not None and e.stands_for(weight, self.epoch):
            return e.w_a, e.w_b
        if e is not None and e.ref() is weight and e.w_a.device == weight.device:
            e.refresh(weight, C1, self.epoch)
        else:
            e = self.slices[key] = _SlicePair(weight, C1, self.epoch)
        return e.w_a, e.w_b

    @staticmethod
    def _pack(kind, weight, C_in, Co, k, w_mode, buf, desc):
        L = _lib.lib()
        if kind == 'conv':
            return L.rvsr_conv2d_pack_weights(_p(weight), C_in, Co, k, w_mode, _p(buf), buf.numel(), desc, _stream())
        return L.rvsr_dcn_pack_weights(_p(weight), C_in, Co, _p(buf), buf.numel(), desc, _stream())

    def get(self, weight, kind, C_in, Co, k, w_mode, nbytes):
        """Packed image tensor for (weight, kind, geometry), or None when the weight is not cacheable."""
        if not self.enabled or _lib.get_gemm_mode() == 'f32':
            return None
        if kind == 'conv' and k == 7:   # exact-f32 kernels in every GEMM mode: no image exists, and repack() never sees these weights
            return None
        if getattr(weight, '_rvsr_grad_home', None) is None and getattr(weight, '_rvsr_parent', None) is None:
            return None
        key = (id(weight), kind, C_in, Co, k, w_mode)
        e = self.entries.get(key)
        if e is not None and e.stands_for(weight, self.epoch):
            self.stats['hits'] += 1
            from . import functional   # (the debug switch stays where tests and notes set it: functional._PACK_VERIFY)
            if functional._PACK_VERIFY:
                self._verify(e, weight, kind, C_in, Co, k, w_mode)
            return e.buf
        buf = e.buf if e is not None and e.buf.numel() >= nbytes and e.buf.device == weight.device else \
            torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=weight.device)
        # rvsr_dcn_pack_weights WRITES 20 values (the second descriptor, desc[10:], is the zeroed slot of an image that left the library)
        desc = (ctypes.c_longlong * 20)()
        if self._pack(kind, weight, C_in, Co, k, w_mode, buf, desc) == 0:
            return None
        self.stats['packs'] += 1
        self.entries[key] = _Image(buf, list(desc[:10]), weight, self.epoch)
        self.table = None
        return buf

    def _verify(self, e, weight, kind, C_in, Co, k, w_mode):
        """functional._PACK_VERIFY = True (debug): on a cache hit, pack the weight again and compare -- catches writes that bypassed both torch's
        version counter and repack()/invalidate() (p.data.copy_, raw writes into FlatBuffers.param, EMA swaps)."""
        tmp = torch.empty_like(e.buf)
        n = int(self._pack(kind, weight, C_in, Co, k, w_mode, tmp, None))
        if not torch.equal(tmp[:n], e.buf[:n]):
            raise RuntimeError('PackedWeights: stale bf16 weight image (the parameter was written without a version bump; call '
                               'realvsr_amd.functional.invalidate_weight_cache() after such writes)')

    def repack(self):
        """Re-pack every live image in one launch (the parameters were just updated in place) and start a new epoch."""
        self.epoch += 1
        if not self.enabled or not self.entries:
            return
        for key, e in list(self.slices.items()):     # refresh the persistent input-channel slices first: their images are packed below
            parent = e.ref()
            if e.stands_for(parent, None):
                e.refresh(parent, key[1], self.epoch)
            else:
                del self.slices[key]
        for key in [key for key, e in self.entries.items() if not e.stands_for(e.ref(), None)]:
            del self.entries[key]
            self.table = None
        if not self.entries:
            return
        by_dev = {}
        for e in self.entries.values():
            by_dev.setdefault(e.buf.device, []).append(e)
        if self.table is None:
            self.table = {dev: (torch.tensor([e.table_row() for e in es], dtype=torch.int64).to(dev), len(es))
                          for dev, es in by_dev.items()}
        for dev, es in by_dev.items():
            tab, n = self.table[dev]
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().rvsr_pack_weights_batched(_p(tab), n, _stream()), 'pack_weights_batched')
            for e in es:
                e.epoch = self.epoch
        self.stats['batched'] += 1


class _Slot:
    """One ring slot of a DCN layer: the counters of one backward on their way to the host."""
    __slots__ = ('counters', 'event', 'nsamples', 'tick')

    def __init__(self):
        self.counters, self.event, self.nsamples, self.tick = torch.zeros(8, dtype=torch.int32).pin_memory(), torch.cuda.Event(), 0, -1


class _Layer:
    __slots__ = ('ref', 'ring', 'records', 'halo')

    def __init__(self, weight, nslots):
        self.ref, self.ring, self.records = weakref.ref(weight), [_Slot() for _ in range(nslots)], 0
        self.halo = {}   # {tick: halo decided from that tick's counters} (the last decision only)


class DcnOffsetStats:
    """Per DCN layer: the sampled offset counters of its last backwards (components beyond 2.5 .. 11.5 px), brought to the host with a
    non-blocking copy + event, so that a later forward of the layer can pick its LDS tile halo (3 / 7 / 11 px) on the host and launch
    exactly one kernel.  The forward uses the counters recorded LAG = 3 OPTIMIZER STEPS back (`advance()`, called by FlatAdam.step; the
    layer's last backward of that step) and waits for that copy: the choice is a function of the data, never of host timing (a
    query-and-keep-the-old-decision would make the kernel choice, and with it the last bits of the forward, depend on how far the host
    happens to run ahead), and a host that is up to three steps ahead of the GPU -- which is what absorbs an 80 ms pause of Python's
    garbage collector, tools/cpu_launch_time.py -- never blocks on it, however many backwards per step a layer has (the per-frame PCD path
    has N).  Without an optimizer that calls advance() the lag is counted in backwards of the layer instead.  Offsets of a layer change
    slowly from step to step, and the choice affects speed and the last bits of rounding only (samples beyond the tile gather from global
    memory with the same rules) -- which also means that data-parallel ranks, whose offsets differ, may run different tile sizes: their
    forwards are equal to rounding, not bitwise.  The rule is the device's: rvsr_dcn_forward_halo evaluates the candidates of the forward
    plan (csrc/dcn_plan.h) on the copied counters."""
    LAG = 3

    def __init__(self):
        self.layers = {}     # id(weight) -> _Layer
        self.step = None     # optimizer steps seen (None: nobody advances -- ticks are the layer's own record count)

    def advance(self):
        self.step = 1 if self.step is None else self.step + 1

    def _tick(self, layer):
        return self.step if self.step is not None else layer.records

    def record(self, weight, probe_dev, nsamples):
        layer = self.layers.get(id(weight))
        if layer is None or layer.ref() is not weight:
            layer = self.layers[id(weight)] = _Layer(weight, self.LAG + 1)
            for k in [k for k, v in self.layers.items() if v.ref() is None]:
                del self.layers[k]
        tick = self._tick(layer)
        slot = layer.ring[tick % (self.LAG + 1)]
        slot.counters.copy_(probe_dev, non_blocking=True)
        slot.event.record()
        slot.nsamples = int(nsamples)
        slot.tick = tick
        layer.halo.pop(tick, None)
        layer.records += 1

    def forward_halo(self, weight, Co):
        layer = self.layers.get(id(weight))
        if layer is None or layer.ref() is not weight or layer.records == 0:
            return 0
        want = self._tick(layer) - self.LAG
        # the record of `want`; while the ring fills (or after steps without a backward of this layer): the oldest one it holds
        live = [s for s in layer.ring if s.tick >= 0]
        older = [s for s in live if s.tick <= want]
        slot = max(older, key=lambda s: s.tick) if older else min(live, key=lambda s: s.tick)
        if slot.tick not in layer.halo:
            c, n = slot.counters, slot.nsamples
            slot.event.synchronize()
            layer.halo = {slot.tick: _lib.lib().rvsr_dcn_forward_halo(c.data_ptr(), n, Co)}
        return layer.halo[slot.tick]


packed_weights = PackedWeights()
dcn_offset_stats = DcnOffsetStats()
