"""The last third of a training step (promonet/train/core.py:335-369) on the
library's own kernels (pm_optim.h), without a host read:

    scaler.scale(generator_losses).backward()
    gradient_statistics = promonet_amd.optim.gradient_stats(generator)
    scaler.step(generator_optimizer)        # AdamW below, clip=GRADIENT_CLIP_*
    scaler.update()

`AdamW` is a `torch.optim.Optimizer` whose `step()` is two passes over the
list of parameters that have a gradient: the statistics pass (max, min, mean,
norm and the count of non-finite gradients, the clip coefficient, found_inf,
and the optimizer's step advanced on the device) and the update pass. Under a
stock `torch.amp.GradScaler` it takes the scale and found_inf through torch's
protocol for fused optimizers; `GradScaler` below also leaves torch's own
inf-check pass out and updates the scale with the library's kernel. Nothing
here runs on the CPU: CPU parameters raise.
"""
import ctypes
from collections import defaultdict

import torch
from torch.amp.grad_scaler import OptState, _refresh_per_optimizer_state

from . import _lib

_DTYPES = {torch.float32: _lib.PM_F32, torch.float16: _lib.PM_F16,
           torch.bfloat16: _lib.PM_BF16}
STATS_KEYS = ('gradients/max', 'gradients/min', 'gradients/mean',
              'gradients/norm')
MAX_FOUND = 8       # found_inf scalars one pm_optim_scaler_update reads


def _gradient(parameter):
    """The gradient as the kernels read it: dense, in the parameter's order"""
    gradient = parameter.grad
    if gradient.is_sparse:
        raise ValueError('sparse gradients are not supported')
    if gradient.dtype not in _DTYPES:
        raise ValueError(
            f'gradients must be fp32, f16 or bf16, got {gradient.dtype}')
    return gradient if gradient.is_contiguous() else gradient.contiguous()


def _pointers(tensors):
    return (ctypes.c_void_p * len(tensors))(*(t.data_ptr() for t in tensors))


class _List:
    """The host arrays of one list of gradients, and the workspace it needs"""

    def __init__(self, gradients):
        count = len(gradients)
        self.count = count
        self.grad = _pointers(gradients)
        self.numel = (ctypes.c_longlong * count)(
            *(g.numel() for g in gradients))
        self.dtype = (ctypes.c_int * count)(
            *(_DTYPES[g.dtype] for g in gradients))
        self.bytes = _lib.lib().pm_optim_workspace_bytes(self.numel, count)
        if not self.bytes:
            raise ValueError('a gradient is empty')


def _scalar(tensor, device, name):
    """The pointer of an optional fp32 device scalar"""
    if tensor is None:
        return None
    if tensor.numel() != 1 or tensor.dtype != torch.float32:
        raise ValueError(f'{name} must be one fp32 value')
    if tensor.device != device:
        raise ValueError(f'{name} is on {tensor.device}, not on {device}')
    return tensor.data_ptr()


def _grad_stats(entries, stats, workspace, grad_scale=None, found_inf=None,
                clip=None, betas=(0., 0.), state=None):
    device = stats.device
    with torch.cuda.device(device):
        _lib.check(_lib.lib().pm_optim_grad_stats(
            entries.grad, entries.numel, entries.dtype, entries.count,
            _scalar(grad_scale, device, 'grad_scale'),
            _scalar(found_inf, device, 'found_inf'),
            -1. if clip is None else float(clip), betas[0], betas[1],
            None if state is None else state.data_ptr(), stats.data_ptr(),
            workspace.data_ptr(), workspace.numel(), _lib.stream()))


def _stats_block(module_or_params):
    """The statistics pass alone -> its block of PM_OPTIM_STATS floats"""
    if isinstance(module_or_params, torch.nn.Module):
        module_or_params = module_or_params.parameters()
    gradients = [_gradient(p) for p in module_or_params if p.grad is not None]
    if not gradients:
        raise ValueError('no parameter has a gradient')
    for gradient in gradients:
        _lib.require_gpu(gradient)
    entries = _List(gradients)
    device = gradients[0].device
    stats = torch.empty(_lib.OPTIM_STATS, device=device)
    workspace = torch.empty(entries.bytes, dtype=torch.uint8, device=device)
    _grad_stats(entries, stats, workspace)
    return stats


def gradient_stats(module_or_params):
    """`torchutil.gradients.stats` on the device: {'gradients/max',
    'gradients/min', 'gradients/mean', 'gradients/norm'} over every gradient
    of a module (or of an iterable of parameters) as 0-d fp32 device tensors;
    nothing is synchronised. max and min are exact; mean is the sum over the
    count of elements and norm the L2 norm of the concatenation, both summed
    in a fixed order (fp32 inside a chunk, the chunks in double) and rounded
    once. NaN and +-inf gradients are left out of all four.

    torchutil is not installed where this was written: beyond 'gradients/max'
    and 'gradients/min', which the reference's training loop reads, the key
    set and the definitions of its other entries are UNPINNED."""
    stats = _stats_block(module_or_params)
    return {key: stats[index] for index, key in enumerate(STATS_KEYS)}


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW's update (decoupled weight decay, bias-corrected
    moments; no amsgrad, no maximize) with the reference's defaults, as the
    library's two passes. `clip` is GRADIENT_CLIP_GENERATOR: the reference's
    clip by the largest gradient magnitude, decided and applied on the device.

    state_dict() / load_state_dict() have torch.optim.AdamW's layout (per
    parameter step, exp_avg, exp_avg_sq). The step and the powers of the betas
    live on the device and are ONE set for the optimizer: every group has the
    same betas, a loaded state has one step, and a parameter that has no
    gradient in a step is left out of it while the step still advances.

    The hyper-parameters are arguments of the launches: a captured graph keeps
    the values it was captured with."""
    _step_supports_amp_scaling = True

    def __init__(self, params, lr=2e-4, betas=(.8, .99), eps=1e-9,
                 weight_decay=1e-2, clip=None):
        if lr < 0 or eps < 0 or weight_decay < 0:
            raise ValueError('lr, eps and weight_decay must be at least 0')
        if not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError(f'betas must be in [0, 1), got {betas}')
        if clip is not None and not clip >= 0:
            raise ValueError(f'clip must be at least 0, got {clip}')
        super().__init__(params, dict(
            lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self.clip = clip
        self._device = None
        self._cached = None

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        betas = self.param_groups[0]['betas']
        for group in self.param_groups:
            if tuple(group['betas']) != tuple(betas):
                raise ValueError('every group must have the same betas')
            for parameter in group['params']:
                if parameter.dtype != torch.float32:
                    raise ValueError(
                        f'parameters must be fp32, got {parameter.dtype}')
                if not parameter.is_contiguous():
                    raise ValueError('parameters must be contiguous')

    # -- device state ------------------------------------------------------

    def _setup(self, device, step=0):
        """{step, beta1^step, beta2^step} as doubles, the powers multiplied up
        as the device does, and the statistics block"""
        beta1, beta2 = self.param_groups[0]['betas']
        power1 = power2 = 1.
        for _ in range(step):
            power1 *= beta1
            power2 *= beta2
        self._device = device
        self._state = torch.tensor(
            [float(step), power1, power2], dtype=torch.float64, device=device)
        self._stats = torch.zeros(_lib.OPTIM_STATS, device=device)
        self._workspace = torch.empty(0, dtype=torch.uint8, device=device)

    def _moments(self, parameter):
        state = self.state[parameter]
        if not state:
            state['step'] = torch.tensor(0.)
            state['exp_avg'] = torch.zeros_like(
                parameter, memory_format=torch.contiguous_format)
            state['exp_avg_sq'] = torch.zeros_like(
                parameter, memory_format=torch.contiguous_format)
        return state['exp_avg'], state['exp_avg_sq']

    def _entries(self):
        """Per group the host arrays of the parameters that have a gradient,
        and those of the whole list; kept while the parameters and their
        gradients stay at the same addresses (the gradients that
        zero_grad(set_to_none=True) drops come back there as a rule: the
        arrays hold no reference to them), and built again otherwise"""
        parameters = [[p for p in group['params'] if p.grad is not None]
                      for group in self.param_groups]
        flat = [p for group in parameters for p in group]
        if not flat:
            return None
        key = [(p.data_ptr(), p.grad.data_ptr(), p.grad.dtype,
                p.grad.is_contiguous()) for p in flat]
        cached = self._cached
        if cached is not None and cached['key'] == key:
            return cached
        for parameter in flat:
            _lib.require_gpu(parameter)
            if parameter.device != flat[0].device:
                raise ValueError('every parameter must be on one device')
        if self._device is None:
            self._setup(flat[0].device)
        groups, gradients = [], []
        for group in parameters:
            if not group:
                groups.append(None)
                continue
            moments = [self._moments(p) for p in group]
            dense = [_gradient(p) for p in group]
            entries = _List(dense)
            entries.param = _pointers(group)
            entries.exp_avg = _pointers([m[0] for m in moments])
            entries.exp_avg_sq = _pointers([m[1] for m in moments])
            groups.append(entries)
            gradients.extend(dense)
        whole = _List(gradients)
        if whole.bytes > self._workspace.numel():
            self._workspace = torch.empty(
                whole.bytes, dtype=torch.uint8, device=self._device)
        cached = {'key': key, 'groups': groups, 'whole': whole}
        # a gradient that had to be copied is read from its copy, which lives
        # as long as this step: nothing is kept then
        if all(contiguous for *_, contiguous in key):
            self._cached = cached
            return cached
        self._cached = None
        return dict(cached, copies=gradients)

    # -- the step ------------------------------------------------------------

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        cached = self._entries()
        if cached is None:
            return loss
        lib = _lib.lib()
        betas = self.param_groups[0]['betas']
        _grad_stats(
            cached['whole'], self._stats, self._workspace,
            getattr(self, 'grad_scale', None),
            getattr(self, 'found_inf', None), self.clip, betas, self._state)
        with torch.cuda.device(self._device):
            for group, entries in zip(self.param_groups, cached['groups']):
                if entries is None:
                    continue
                _lib.check(lib.pm_optim_adamw_step(
                    entries.param, entries.exp_avg, entries.exp_avg_sq,
                    entries.grad, entries.numel, entries.dtype, entries.count,
                    self._stats.data_ptr(), self._state.data_ptr(),
                    group['lr'], betas[0], betas[1], group['eps'],
                    group['weight_decay'], _lib.stream()))
        return loss

    def stats(self):
        """The last step's five figures as device tensors (views of one block
        that the next step overwrites): 'gradients/max', 'gradients/min',
        'gradients/mean', 'gradients/norm' and 'gradients/nonfinite'"""
        if self._device is None:
            raise RuntimeError('no step has been taken')
        figures = {key: self._stats[index]
                   for index, key in enumerate(STATS_KEYS)}
        figures['gradients/nonfinite'] = self._stats[_lib.OPTIM_NONFINITE]
        return figures

    def found_inf_scalar(self):
        """The last step's found_inf (1 fp32 device value: 1. if the step was
        skipped)"""
        return self._stats[_lib.OPTIM_FOUND_INF:_lib.OPTIM_FOUND_INF + 1]

    # -- checkpoints ---------------------------------------------------------

    def state_dict(self):
        if self._device is not None:
            step = self._state[0].item()
            for state in self.state.values():
                if state:
                    state['step'] = torch.tensor(step, dtype=torch.float32)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        betas = self.param_groups[0]['betas']
        if any(tuple(g['betas']) != tuple(betas) for g in self.param_groups):
            raise ValueError('every group must have the same betas')
        steps = {int(state['step']) for state in self.state.values() if state}
        if len(steps) > 1:
            raise ValueError(
                f'the parameters are at different steps {sorted(steps)}: this '
                'optimizer keeps one step')
        device = None
        for parameter, state in self.state.items():
            if not state:
                continue
            device = parameter.device
            state['step'] = torch.tensor(float(state['step']))
            for key in ('exp_avg', 'exp_avg_sq'):
                state[key] = state[key].to(
                    parameter.device, torch.float32).contiguous()
        self._cached = None
        if device is not None and device.type == 'cuda':
            self._setup(device, steps.pop())


class GradScaler(torch.amp.GradScaler):
    """torch.amp.GradScaler whose step() hands an `AdamW` of this module the
    scale and leaves torch's own pass over the gradients out (the statistics
    pass finds the non-finite values and unscales inside the update), and
    whose update() is pm_optim_scaler_update. Any other optimizer, and a
    scaler that is not on a GPU, takes torch's path unchanged; state_dict()
    is torch's."""

    def step(self, optimizer, *args, **kwargs):
        if not self._enabled or not isinstance(optimizer, AdamW):
            return super().step(optimizer, *args, **kwargs)
        if 'closure' in kwargs:
            raise RuntimeError(
                'Closure use is not currently supported if GradScaler is '
                'enabled.')
        self._check_scale_growth_tracker('step')
        state = self._per_optimizer_states[id(optimizer)]
        if state['stage'] is OptState.STEPPED:
            raise RuntimeError(
                'step() has already been called since the last update().')
        if state['stage'] is OptState.UNSCALED:
            # unscale_() ran torch's pass: the gradients are as they are
            found = list(state['found_inf_per_device'].values())
            incoming = found[0] if len(found) == 1 else sum(
                f.to(self._scale.device) for f in found)
            optimizer.grad_scale, optimizer.found_inf = None, incoming
        else:
            optimizer.grad_scale, optimizer.found_inf = self._scale, None
        try:
            result = optimizer.step(*args, **kwargs)
        finally:
            del optimizer.grad_scale
            del optimizer.found_inf
        if optimizer._device is not None:
            state['found_inf_per_device'] = {
                optimizer._device: optimizer.found_inf_scalar()}
        elif not state['found_inf_per_device']:
            # no parameter had a gradient: nothing was found
            state['found_inf_per_device'] = {
                self._scale.device: torch.zeros(1, device=self._scale.device)}
        state['stage'] = OptState.STEPPED
        return result

    def update(self, new_scale=None):
        if not self._enabled:
            return
        scale, tracker = self._check_scale_growth_tracker('update')
        if new_scale is not None or not scale.is_cuda:
            return super().update(new_scale)
        found = [
            f.to(scale.device, torch.float32).reshape(1)
            for state in self._per_optimizer_states.values()
            for f in state['found_inf_per_device'].values()]
        assert found, 'No inf checks were recorded prior to update.'
        every = found
        if len(found) > MAX_FOUND:
            # more scalars than one kernel reads: their sum stands for them
            found = [torch.stack(found).sum(0)]
        with torch.cuda.device(scale.device):
            _lib.check(_lib.lib().pm_optim_scaler_update(
                scale.data_ptr(), tracker.data_ptr(), _pointers(found),
                len(found), self._growth_factor, self._backoff_factor,
                self._growth_interval, _lib.stream()))
        if found is not every:
            # (the kernel cleared the sum)
            torch._foreach_zero_(every)
        self._per_optimizer_states = defaultdict(_refresh_per_optimizer_state)
