"""What the *_step.py tools share, each thing once: the two ways they time a call with device events, the seeded clip batch, and for the
generator tools (rcan, fstrn, tof) the Split-model option dictionary and the timed training loop.  The tools run as scripts, so this
directory is on their sys.path.  torch is imported where it is used: the parent process of the data tools measures nothing and never
loads it."""


def median(v):
    return sorted(v)[len(v) // 2]


def event_ms(fn, inner):
    """ms per call: one event pair around `inner` calls."""
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(inner):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / inner


def lap_ms(fn, reps, warmup):
    """The sorted per-call ms of `reps` calls after `warmup` untimed ones: an event after every call."""
    import torch
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))


def clip_batch(B, S, seed):
    """{'LQs', 'GT'} of B x 3 x 3 x S x S uniform noise on the current device, LQs drawn first."""
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    return {'LQs': torch.rand(B, 3, 3, S, S, device='cuda', generator=g), 'GT': torch.rand(B, 3, 3, S, S, device='cuda', generator=g)}


def split_opt(network_G):
    """The Split model on one GPU with LapPyr(ssim, cb) on Y + GWLoss on CbCr, as the generators' option files train it."""
    return {'model': 'VideoSR_AllPair_YCbCr_Split', 'dist': False, 'gpu_ids': [0], 'is_train': True, 'scale': 1, 'augment': None,
            'network_G': network_G,
            'path': {}, 'train': {'pixel_criterion_y': 'lappyr', 'pixel_weight_y': 1.0, 'pixel_criterion_c': 'gw', 'pixel_weight_c': 1.0,
                                  'weight_decay_G': 0, 'ft_tsa_only': 0, 'lr_G': 1e-4, 'beta1': 0.9, 'beta2': 0.99}}


def train_ms_step(model, data, warmup, steps):
    """ms per feed_data + optimize_parameters(step, log=False): `warmup` untimed steps, then one event pair around `steps` more."""
    import torch
    for step in range(1, warmup + 1):
        model.feed_data(data)
        model.optimize_parameters(step, log=False)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for step in range(warmup + 1, warmup + steps + 1):
        model.feed_data(data)
        model.optimize_parameters(step, log=False)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps
