"""Optimisers of the GCRNN training loop on flat buffers.

The reference steps `torch.optim.Adam(lr, betas)` per model (kStepPredGRNNs.py:158-161, 794-796; stepped at
Modules/train_rnn.py:276). Here every parameter is a view into ONE flat parameter buffer and every `.grad` a view into
ONE flat gradient buffer (parallel.FlatGradAllReduce -- the buffer the data-parallel all-reduce reduces in place), so an
optimiser step is one HIP kernel over the flat buffers (C ABI `gcrnn_adam_flat`) instead of ~10 launches per tensor, and
the step counter lives on the device: the whole zero_grad -> forward -> loss -> BPTT -> Adam sequence is capturable as one
hipGraph with the all-reduce outside.

The drivers' other training options live here too: `trainer = 'SGD' | 'ADAM' | 'RMSprop'` (kStepPredGRNNs.py:158-161, built at
:706-715) as FlatSGD / FlatAdam / FlatRMSprop behind `make_trainer`, and `doLearningRateDecay` (a StepLR stepped at the top of every
epoch, Modules/train_rnn.py:149-155, 197-200) as `StepDecay`. For decay to reach a step that was captured in a hipGraph the learning
rate is a one-element fp64 DEVICE tensor that the kernels read (`gcrnn_sgd_flat`, `gcrnn_rmsprop_flat`, `gcrnn_adam_flat_dlr`):
`set_lr` is a stream-ordered fill, and the next replay steps with the new value.
"""
import ctypes as C

import torch

from .parallel import FlatGradAllReduce


class _FlatOptimizer(object):
    """What the flat optimisers share: the parameters become views of ONE flat buffer (the gradients already are views of `sync.flat`),
    the learning rate lives in a one-element fp64 device tensor `lr_dev` (None: a host value, FlatAdam's default path), and a step is
    `_step_hip` (the product path, raw pointers on the current stream) or `_step_torch` (CPU tensors: test-only, see `step`).
    Subclasses list their state buffers in `_state` and their hyper-parameters in `_hyper`."""

    _state = ()
    _hyper = ()

    def __init__(self, params, lr, sync=None, device_lr=True):
        self.sync = sync if sync is not None else FlatGradAllReduce(params)
        ps = self.sync.params
        name = type(self).__name__
        assert ps, 'no trainable parameters'
        dt, dev = ps[0].dtype, ps[0].device
        assert all(p.dtype == dt and p.device == dev for p in ps), name + ': one dtype and one device'
        assert dt in (torch.float32, torch.float64) and self.sync.dtype == dt
        self._lr = float(lr)
        self.lr_dev = torch.full((1,), float(lr), dtype=torch.float64, device=dev) if device_lr else None
        self.schedule = None                                          # a StepDecay attaches itself: its count travels in state_dict
        self.flat_p = torch.empty(self.sync.numel, dtype=dt, device=dev)
        off = 0
        with torch.no_grad():
            for p in ps:
                n = p.numel()
                self.flat_p[off:off + n].copy_(p.reshape(-1))
                p.data = self.flat_p[off:off + n].view_as(p)          # the module's tensors now alias the flat buffer
                off += n

    @property
    def lr(self):
        """The learning rate in force (read back from the device where it lives there: a synchronisation, not for a hot loop)."""
        return self._lr if self.lr_dev is None else float(self.lr_dev.item())

    @lr.setter
    def lr(self, value):
        if self.lr_dev is None:
            self._lr = float(value)
        else:
            self.set_lr(value)

    def set_lr(self, value):
        """Write the device learning rate with a stream-ordered fill: no kernel of this library, no synchronisation; a captured step
        that is replayed behind it on the same stream steps with the new value."""
        if self.lr_dev is None:
            raise RuntimeError('%s(device_lr=False): the learning rate is a launch argument of gcrnn_adam_flat (a host double that a '
                               'captured step has baked in), so it cannot be changed behind a capture; build the optimiser with '
                               'device_lr=True' % type(self).__name__)
        self.lr_dev.fill_(float(value))

    def zero_grad(self, set_to_none=False):
        self.sync.zero_grad()

    def _check_alias(self):
        off = 0
        for p in self.sync.params:
            if p.data_ptr() != self.flat_p.data_ptr() + off * self.flat_p.element_size():
                raise RuntimeError('%s: a parameter no longer aliases the flat buffer (module moved or cast after the '
                                   'optimiser was built); build the optimiser after .to(device / dtype)' % type(self).__name__)
            off += p.numel()

    @torch.no_grad()
    def step(self, grad_scale=1.0):
        self.sync.attach_()
        self._check_alias()
        g = self.sync.flat
        if self.flat_p.is_cuda:
            from . import _lib
            self._step_hip(_lib, g, float(grad_scale), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        else:
            # TEST-ONLY branch (CPU tensors): the same update in torch ops, so that the N > 1 logic around the optimiser (flat buffers,
            # sharded batches, the collective) can run over gloo in a container without a GPU (tests/test_parallel_gloo.py). The product
            # path -- the recurrence and everything on its data -- has no CPU implementation (GcrnnError on CPU tensors).
            self._step_torch(g * grad_scale if grad_scale != 1.0 else g)
        from . import ops
        ops.parameters_changed()      # (written through raw pointers: the parameters' version counters did not move -- cached packs of the old values must not answer)

    def _ptr(self, t):
        return C.c_void_p(t.data_ptr())

    def state_dict(self):
        sd = {'flat_p': self.flat_p.clone(), 'lr': self.lr}
        sd.update((k, getattr(self, a).clone()) for k, a in self._state)
        sd.update((k, getattr(self, k)) for k in self._hyper)
        if self.schedule is not None:
            sd['schedule'] = self.schedule.state_dict()
        return sd

    def load_state_dict(self, sd):
        self.flat_p.copy_(sd['flat_p'])
        for k, a in self._state:
            getattr(self, a).copy_(sd[k])
        for k in self._hyper:
            setattr(self, k, tuple(sd[k]) if isinstance(sd[k], (tuple, list)) else sd[k])
        self.lr = sd['lr']
        if self.schedule is not None and 'schedule' in sd:
            self.schedule.load_state_dict(sd['schedule'])
        from . import ops
        ops.parameters_changed()


class FlatAdam(_FlatOptimizer):
    """Adam (no weight decay, no amsgrad -- the drivers' configuration) over the flat buffers of `params`.

        opt = FlatAdam(model.parameters(), lr=1e-3, betas=(0.9, 0.999))
        opt.zero_grad(); loss.backward(); opt.sync.all_reduce_(); opt.step()

    Parameters must share one dtype (fp32 or fp64: master weights) and one device. On a CPU tensor set (the gloo tests)
    the same update is evaluated with torch ops on the flat views -- the HIP kernel is the product path on a GPU.
    device_lr=False (default): `lr` is a host value handed to `gcrnn_adam_flat` as a launch argument (a captured step keeps the value
    it was captured with; `set_lr` raises). device_lr=True: `lr` lives in the device scalar `lr_dev`, the step is
    `gcrnn_adam_flat_dlr` (same arithmetic, bit for bit) and `set_lr` / `StepDecay` reach a captured step."""

    _state = (('m', 'm'), ('v', 'v'), ('step', 'step_dev'))
    _hyper = ('betas', 'eps')

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, sync=None, device_lr=False):
        super().__init__(params, lr, sync, device_lr)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.m = torch.zeros_like(self.flat_p)
        self.v = torch.zeros_like(self.flat_p)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=self.flat_p.device)

    def _step_hip(self, _lib, g, grad_scale, st):
        head = (_lib.dtype_code(self.flat_p.dtype), self._ptr(self.flat_p), self._ptr(g), self._ptr(self.m), self._ptr(self.v),
                self.flat_p.numel())
        tail = (self.betas[0], self.betas[1], self.eps, grad_scale, self._ptr(self.step_dev), st)
        if self.lr_dev is None:
            _lib.check(_lib.lib.gcrnn_adam_flat(*head, self._lr, *tail), 'adam_flat')
        else:
            _lib.check(_lib.lib.gcrnn_adam_flat_dlr(*head, self._ptr(self.lr_dev), *tail), 'adam_flat_dlr')

    def _step_torch(self, gs):
        b1, b2 = self.betas
        self.step_dev += 1
        t = float(self.step_dev.item())
        self.m.lerp_(gs, 1 - b1)
        self.v.mul_(b2).addcmul_(gs, gs, value=1 - b2)
        denom = (self.v.sqrt() / (1 - b2 ** t) ** 0.5).add_(self.eps)
        self.flat_p.addcdiv_(self.m, denom, value=-self.lr / (1 - b1 ** t))


class FlatSGD(_FlatOptimizer):
    """torch.optim.SGD(lr) as the drivers build it (kStepPredGRNNs.py:710-711: no momentum, no weight decay) over the flat buffers:
    one launch of `gcrnn_sgd_flat`, p -= lr * (g * grad_scale), `lr` on the device."""

    def __init__(self, params, lr, sync=None):
        super().__init__(params, lr, sync)

    def _step_hip(self, _lib, g, grad_scale, st):
        _lib.check(_lib.lib.gcrnn_sgd_flat(_lib.dtype_code(self.flat_p.dtype), self._ptr(self.flat_p), self._ptr(g), self.flat_p.numel(),
                                           self._ptr(self.lr_dev), grad_scale, st), 'sgd_flat')

    def _step_torch(self, gs):
        self.flat_p.add_(gs, alpha=-self.lr)


class FlatRMSprop(_FlatOptimizer):
    """torch.optim.RMSprop(lr, alpha) with torch's defaults for the rest (eps 1e-8, no momentum, not centered; the drivers pass
    alpha = beta1, kStepPredGRNNs.py:712-714) over the flat buffers: one launch of `gcrnn_rmsprop_flat`,
    v = alpha v + (1 - alpha) g^2;  p -= lr * g / (sqrt(v) + eps), `lr` on the device."""

    _state = (('v', 'v'),)
    _hyper = ('alpha', 'eps')

    def __init__(self, params, lr, alpha=0.99, eps=1e-8, sync=None):
        super().__init__(params, lr, sync)
        self.alpha, self.eps = float(alpha), float(eps)
        self.v = torch.zeros_like(self.flat_p)

    def _step_hip(self, _lib, g, grad_scale, st):
        _lib.check(_lib.lib.gcrnn_rmsprop_flat(_lib.dtype_code(self.flat_p.dtype), self._ptr(self.flat_p), self._ptr(g), self._ptr(self.v),
                                               self.flat_p.numel(), self._ptr(self.lr_dev), self.alpha, self.eps, grad_scale, st),
                   'rmsprop_flat')

    def _step_torch(self, gs):
        self.v.mul_(self.alpha).addcmul_(gs, gs, value=1 - self.alpha)
        self.flat_p.addcdiv_(gs, self.v.sqrt().add_(self.eps), value=-self.lr)


class StepDecay(object):
    """The drivers' learning-rate schedule (`learningRateDecayRate` / `learningRateDecayPeriod`, Modules/train_rnn.py:149-155) for the
    flat optimisers: `step()` counts epochs and multiplies the CURRENT learning rate by `rate` whenever the count reaches a multiple of
    `period` -- the recursive form of torch's StepLR, not lr0 * rate ** (epoch // period), so the values equal torch's to the bit.
    The new value goes to the device scalar (`set_lr`): a captured step replayed afterwards uses it. The schedule attaches itself to
    the optimiser, whose state_dict then carries the count (a checkpoint restores the schedule with the learning rate).
    Given a torch.optim.Optimizer, StepDecay(...) returns torch.optim.lr_scheduler.StepLR(optim, period, rate) instead."""

    def __new__(cls, optim, period, rate):
        if isinstance(optim, torch.optim.Optimizer):
            return torch.optim.lr_scheduler.StepLR(optim, period, rate)
        return super().__new__(cls)

    def __init__(self, optim, period, rate):
        if getattr(optim, 'lr_dev', None) is None:
            optim.set_lr(optim.lr)                                     # raises, saying why (FlatAdam's default keeps lr on the host)
        self.optim, self.period, self.rate, self.epoch = optim, int(period), float(rate), 0
        optim.schedule = self

    def step(self):
        self.epoch += 1
        if self.epoch % self.period == 0:
            self.optim.set_lr(self.optim.lr * self.rate)

    def get_last_lr(self):
        return [self.optim.lr]

    def state_dict(self):
        return {'epoch': self.epoch, 'period': self.period, 'rate': self.rate}

    def load_state_dict(self, sd):
        self.epoch, self.period, self.rate = int(sd['epoch']), int(sd['period']), float(sd['rate'])


TRAINERS = ('SGD', 'ADAM', 'RMSprop')


def make_trainer(trainer, params, learningRate, beta1, beta2, flat=True):
    """The drivers' optimiser branch (kStepPredGRNNs.py:706-715): 'ADAM' -> Adam(lr, betas=(beta1, beta2)); 'SGD' -> SGD(lr);
    'RMSprop' -> RMSprop(lr, alpha=beta1). flat=True: the flat classes of this module with the learning rate on the device (decay
    reaches a captured step); flat=False: the torch.optim classes exactly as the reference constructs them."""
    if trainer == 'ADAM':
        return FlatAdam(params, lr=learningRate, betas=(beta1, beta2), device_lr=True) if flat else \
            torch.optim.Adam(params, lr=learningRate, betas=(beta1, beta2))
    if trainer == 'SGD':
        return FlatSGD(params, lr=learningRate) if flat else torch.optim.SGD(params, lr=learningRate)
    if trainer == 'RMSprop':
        return FlatRMSprop(params, lr=learningRate, alpha=beta1) if flat else torch.optim.RMSprop(params, lr=learningRate, alpha=beta1)
    raise ValueError("trainer %r: options are 'SGD', 'ADAM', 'RMSprop'" % (trainer,))
