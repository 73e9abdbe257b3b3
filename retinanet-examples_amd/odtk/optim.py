"""The optimisation step of `odtk train` beyond the reference's: `FusedSGD`, torch.optim.SGD whose whole update -- GradScaler's
unscale and skip-on-overflow, the clip coefficient of the global gradient norm, weight decay, momentum, the weight update and the
exponential moving average of the weights -- is ONE streaming HIP pass over the parameters (csrc/optim.hpp: odtk_optim_sgd_step;
the norm is one more pass over the gradients, odtk_optim_grad_norm), and `ModelEMA`, the averaged weights that are validated, saved
and used by `odtk infer`.  Nothing here runs unless `--ema`, `--clip-grad-norm` or `--fused-step` is given (odtk/train.py).

The definition -- the contract the kernels are pinned to (tests/optim_ref.py restates it in numpy) -- per element, every operation in
float32 and rounded on its own:

    skipped -- nothing changes -- when found_inf != 0 or the gradient norm is not finite (clipping only); otherwise
    g = grad;  g = g / grad_scale (under a GradScaler);  g = g * coef (clipping);  g = g + wd * p (wd != 0)
    buf = g on the parameter's first step, else (momentum * buf) + g;   p = p - (lr * buf);   e = e + (1 - decay) * (p - e)

    norm = float32(sqrt(sum of double(g') * double(g'))) over every gradient element, g' = g / grad_scale in float32
    coef = min(1, max_norm / (norm + 1e-6)) in float32 (torch.nn.utils.clip_grad_norm_)

which is torch's SGD (dampening 0, no Nesterov) + clip_grad_norm_ + lerp.  `FusedSGD._step_reference` is that definition in torch
ops, one op per rounding: what runs for CPU tensors and for parameters that are not float32.  Float32 parameters on a GPU always
take the kernels: a missing library is an error there, not a fall-back.
"""
import contextlib
import math
import struct
from collections import OrderedDict

import torch


def _round_f32(value):
    """A Python float rounded once to float32 (what the kernel arguments and a float32 tensor op see)."""
    return struct.unpack('f', struct.pack('f', value))[0]


class ModelEMA:
    """Exponential moving average of a model's weights: float32 copies of the parameters, updated by `FusedSGD.step` inside its
    pass, and copies of the buffers, taken after each step.

    decay_at(t) = min(decay, (1 + t) / (10 + t)) in Python double -- the warm-up of the YOLO recipes: early steps move the average
    fast --, t = the number of `FusedSGD.step` calls so far.  A step that is skipped on overflow still counts (the decision never
    comes back to the host) and leaves the average unchanged."""

    def __init__(self, model, decay=0.9998, updates=0):
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError('ModelEMA: decay must be in (0, 1), got %r' % (decay,))
        self.decay, self.updates = decay, int(updates)
        self.model = model
        self.shadow = OrderedDict()                                 # the model's state_dict keys -> averaged parameter / copied buffer
        self._of = {}                                               # parameter -> its average
        params = dict(model.named_parameters())
        for name, value in model.state_dict().items():
            if name in params:
                self.shadow[name] = params[name].detach().clone().float()     # (clone keeps the strides: channels_last weights)
                self._of[params[name]] = self.shadow[name]
            else:
                self.shadow[name] = value.detach().clone()
        buffers = dict(model.named_buffers())
        self._buffers = [(copy, buffers[name]) for name, copy in self.shadow.items() if name in buffers]

    def decay_at(self, t):
        return min(self.decay, (1.0 + t) / (10.0 + t))

    def one_minus_decay(self):
        """1 - decay of the step about to run, rounded once to float32."""
        return _round_f32(1.0 - self.decay_at(self.updates))

    def of(self, param):
        """The average of `param` (None for a tensor the model did not have when the average was made)."""
        return self._of.get(param)

    def stepped(self):
        """Behind every optimisation step: the step counts, the buffers (live batch-norm statistics) are copied."""
        self.updates += 1
        if self._buffers:
            with torch.no_grad():
                torch._foreach_copy_([dst for dst, _ in self._buffers], [src for _, src in self._buffers])

    def state_dict(self):
        return {'decay': self.decay, 'updates': self.updates,
                'state_dict': OrderedDict((k, v.detach().clone()) for k, v in self.shadow.items())}

    def load_state_dict(self, state):
        """The averages and the step count of a checkpoint; the decay stays the one this object was made with."""
        stored = state['state_dict']
        if set(stored) != set(self.shadow):
            raise ValueError('ModelEMA.load_state_dict: the stored average is of another model')
        with torch.no_grad():
            for name, value in stored.items():
                self.shadow[name].copy_(value)
        self.updates = int(state['updates'])

    @contextlib.contextmanager
    def swapped(self, model=None):
        """Inside, `model` holds the averaged weights; on exit it holds the training weights again, bit for bit.  The fused
        inference engine is dropped both ways (Model.invalidate_engine), so it never serves stale folded weights."""
        model = self.model if model is None else model
        params = dict(model.named_parameters())
        backup = {name: p.detach().clone() for name, p in params.items()}
        with torch.no_grad():
            for name, p in params.items():
                p.copy_(self.shadow[name])
        if hasattr(model, 'invalidate_engine'):
            model.invalidate_engine()
        try:
            yield model
        finally:
            with torch.no_grad():
                for name, p in params.items():
                    p.copy_(backup[name])
            if hasattr(model, 'invalidate_engine'):
                model.invalidate_engine()


class FusedSGD(torch.optim.SGD):
    """torch.optim.SGD (momentum, weight decay; dampening 0, no Nesterov) with the step of the module docstring.  The state_dict
    is SGD's (`momentum_buffer`): checkpoints written with or without it load into each other.

    max_norm: clip the global L2 norm of the gradients to it (None: no clipping).  `bind_ema(ema)`: the step also updates that
    ModelEMA.  Under torch.amp.GradScaler, `scaler.step(optimizer)` hands `grad_scale` and `found_inf` over as device tensors
    (`_step_supports_amp_scaling`): the gradients stay scaled and the step divides.  (torch 2.10's scaler still walks them once to
    look for infs -- an in-place unscale by 1.0 -- before it does so.)"""

    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0, max_norm=None):
        if max_norm is not None and not (math.isfinite(max_norm) and max_norm > 0):
            raise ValueError('FusedSGD: max_norm must be finite and > 0, got %r' % (max_norm,))
        super().__init__(params, lr=lr, momentum=momentum, weight_decay=weight_decay)
        self._step_supports_amp_scaling = True
        self.max_norm = None if max_norm is None else float(max_norm)
        self.ema = None
        self._norm_state = None                                    # float32[4]: norm, coef, the skip word, 0 (csrc/optim.hpp)

    def bind_ema(self, ema):
        self.ema = ema

    @property
    def last_grad_norm(self):
        """The gradient norm of the last step as a 0-d tensor on the parameters' device (None before the first clipped step); reading
        its value is a host synchronisation: the training loop does so at its logging step only."""
        return None if self._norm_state is None else self._norm_state[0]

    # -- the step -------------------------------------------------------------------------------------------
    def _gather(self):
        """[(group, [(param, grad, momentum buffer or None)])] of the parameters that have a gradient."""
        plan = []
        for group in self.param_groups:
            if group.get('nesterov') or group.get('dampening') or group.get('maximize'):
                raise RuntimeError('FusedSGD: nesterov, dampening and maximize are not implemented')
            if isinstance(group['lr'], torch.Tensor):
                raise RuntimeError('FusedSGD: a tensor learning rate would need a host synchronisation per step')
            entries = []
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError('FusedSGD does not support sparse gradients')
                entries.append((p, p.grad, self.state[p].get('momentum_buffer')))
            plan.append((group, entries))
        return plan

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = getattr(self, 'grad_scale', None), getattr(self, 'found_inf', None)
        plan = self._gather()
        tensors = [p for _, entries in plan for p, _, _ in entries]
        one_minus_decay = self.ema.one_minus_decay() if self.ema is not None else 0.0
        if tensors:
            device = tensors[0].device
            fused = device.type == 'cuda' and all(t.device == device and t.dtype == torch.float32 and g.dtype == torch.float32
                                                  for _, entries in plan for t, g, _ in entries)
            (self._step_fused if fused else self._step_reference)(plan, device, one_minus_decay, grad_scale, found_inf)
        if self.ema is not None:
            self.ema.stepped()
        return loss

    def _state_for(self, device):
        if self._norm_state is None or self._norm_state.device != device:
            self._norm_state = torch.zeros(4, dtype=torch.float32, device=device)
        return self._norm_state

    def _step_fused(self, plan, device, one_minus_decay, grad_scale, found_inf):
        from . import _C
        _C.library()                                                # raises when it has not been built: no fall-back on a GPU
        scale = None if grad_scale is None else grad_scale.reshape(()).to(device=device, dtype=torch.float32)
        inf = None if found_inf is None else found_inf.reshape(()).to(device=device, dtype=torch.float32)
        launches = []                                               # (group, first, params, grads, buffers, emas)
        for group, entries in plan:
            for first in (True, False):
                params, grads, buffers, emas = [], [], [], []
                for p, g, buf in entries:
                    if (buf is None) != first:
                        continue
                    if g.stride() != p.stride():
                        g = torch.empty_like(p).copy_(g)            # (a gradient in another layout than its parameter: rare)
                    if buf is None:                                 # zeros, not empty: a first step that is skipped on overflow writes nothing
                        buf = self.state[p]['momentum_buffer'] = torch.zeros_like(p)
                    elif buf.stride() != p.stride():
                        buf = self.state[p]['momentum_buffer'] = torch.empty_like(p).copy_(buf)
                    params.append(p)
                    grads.append(g)
                    buffers.append(buf)
                    emas.append(self.ema.of(p) if self.ema is not None else None)
                if params:
                    launches.append((group, first, _C.optim_tensors(params, grads, buffers, emas)))
        state = None
        if self.max_norm is not None:
            state = self._state_for(device)
            _C.optim_grad_norm([g for _, _, groups in launches for g in groups], scale, self.max_norm, state)
        for group, first, groups in launches:
            _C.optim_sgd_step(groups, group['lr'], group['momentum'], group['weight_decay'], first, one_minus_decay, scale, inf, state,
                              device=device)

    def _step_reference(self, plan, device, one_minus_decay, grad_scale, found_inf):
        """The definition in torch float32 ops, one op per rounding (no `alpha=`, no `lerp`, no `addcmul`: those may fuse)."""
        f32 = dict(dtype=torch.float32, device=device)
        scale = None if grad_scale is None else grad_scale.reshape(()).to(**f32)
        unscaled = [[(g.float() / scale) if scale is not None else g.float() for _, g, _ in entries] for _, entries in plan]
        skip = None if found_inf is None else found_inf.reshape(()).to(**f32) != 0
        coef = None
        if self.max_norm is not None:
            total = torch.zeros((), dtype=torch.float64, device=device)
            for grads in unscaled:
                for g in grads:
                    total = total + (g.double() * g.double()).sum()
            norm = total.sqrt().float()
            coef = torch.tensor(self.max_norm, **f32) / (norm + 1e-6)
            coef = torch.where(coef != coef, coef, torch.clamp(coef, max=1.0))
            bad = ~torch.isfinite(norm)
            skip = bad if skip is None else (skip | bad)
            state = self._state_for(device)
            state[0], state[1] = norm, coef
            state.view(torch.int32)[2] = bad.to(torch.int32)
        for (group, entries), grads in zip(plan, unscaled):
            lr, momentum, wd = group['lr'], group['momentum'], group['weight_decay']
            for (p, _, buf), g in zip(entries, grads):
                p32 = p.detach().float()
                if coef is not None:
                    g = g * coef
                if wd != 0:
                    g = g + p32 * wd
                new_buf = g.clone() if buf is None else (buf.float() * momentum) + g
                new_p = p32 - (new_buf * lr)
                e = self.ema.of(p) if self.ema is not None else None
                new_e = None if e is None else e + (new_p - e) * one_minus_decay
                if skip is not None:                                # no host synchronisation: the old values are written back
                    if buf is not None:
                        new_buf = torch.where(skip, buf.float(), new_buf)
                    new_p = torch.where(skip, p32, new_p)
                    if e is not None:
                        new_e = torch.where(skip, e, new_e)
                if buf is None:
                    if skip is None:
                        self.state[p]['momentum_buffer'] = new_buf.to(p.dtype)
                    else:                                           # a skipped first step leaves no buffer behind: zeros act as none
                        self.state[p]['momentum_buffer'] = torch.where(skip, torch.zeros_like(new_buf), new_buf).to(p.dtype)
                else:
                    buf.copy_(new_buf)
                p.copy_(new_p)
                if e is not None:
                    e.copy_(new_e)
