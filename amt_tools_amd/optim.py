"""
Adam and Adadelta whose step is ONE HIP launch over all parameters (csrc/optim.hip, include/amtx_optim.h), with optional
global gradient-norm clipping inside that launch -- the reference's commented-out `clip_grad_norm_(model.parameters(), 3)`
(amt_tools/train.py:135).

    optimizer = amt_tools_amd.optim.Adam(model.parameters(), lr=6e-4)                 # or Adadelta(model.parameters(), lr=1.0)
    train(model, train_loader, optimizer, ...)                                        # the reference's train(), unchanged

Both classes derive directly from torch.optim.Optimizer, so the reference's resume line
`super(type(optimizer), optimizer).__init__(model.parameters(), optimizer.defaults)` (train.py:111) lands on the base class; everything
a step needs besides `defaults`, `param_groups` and `state` is rebuilt on demand, which is also why the objects pickle.  The state has
torch's keys, shapes and dtypes (`step` a float32 scalar on the CPU), and the param groups carry torch's keys: a `state_dict()` of
either class loads into torch's class of the same name and the other way round.

Which path a parameter takes: float32, on a ROCm device and dense (contiguous, or channels-last for 4-d: the training path holds conv
weights channels-last) -> the HIP launch; anything else (CPU parameters, other dtypes, non-dense views) -> torch's own single-tensor
functional update.  A model may mix both.  The math is torch's either way; the scalars lr / bias_correction1 and sqrt(bias_correction2)
are computed here in double precision from the step count, as torch does, and handed to the kernel.

`max_norm`: the 2-norm of ALL gradients of ALL groups is limited to it, torch.nn.utils.clip_grad_norm_'s coefficient.  On the HIP path one
more launch sums the squares into a device float which the update kernel reads; the coefficient never goes through the host and
`p.grad` is never written.  `last_grad_norm` is that norm as a device scalar (reading it is the caller's synchronisation), `None`
when `max_norm` is off.  `launches_last_step` counts the library launches of the last step.
"""
import numpy as np
import torch
from torch.optim.adadelta import adadelta as _torch_adadelta
from torch.optim.adam import adam as _torch_adam

from . import _lib

__all__ = ['Adam', 'Adadelta']

# torch's param-group keys beyond the hyperparameters, with the only values these classes implement
_TORCH_FLAGS = {'Adam': {'amsgrad': False, 'foreach': None, 'maximize': False, 'capturable': False, 'differentiable': False, 'fused': None,
                         'decoupled_weight_decay': False},
                'Adadelta': {'foreach': None, 'capturable': False, 'maximize': False, 'differentiable': False}}
_STATE_KEYS = {'Adam': ('exp_avg', 'exp_avg_sq'), 'Adadelta': ('square_avg', 'acc_delta')}


def _refuse(kind, flags):
    """ValueError for every keyword of torch's class that asks for something these classes do not implement; TypeError for any other."""
    for key, value in flags.items():
        if key not in _TORCH_FLAGS[kind]:
            raise TypeError(f'{kind}() got an unexpected keyword argument {key!r}')
        if value is not None and value is not False:
            raise ValueError(f'amt_tools_amd.optim.{kind} does not implement {key}={value!r}; use torch.optim.{kind} for it')


def _check_hyper(lr, eps, weight_decay, max_norm, **unit_interval):
    if torch.is_tensor(lr):
        raise ValueError('a tensor lr is not implemented: pass a float')
    if not 0.0 <= lr:
        raise ValueError(f'Invalid learning rate: {lr}')
    if not 0.0 <= eps:
        raise ValueError(f'Invalid epsilon value: {eps}')
    if not 0.0 <= weight_decay:
        raise ValueError(f'Invalid weight_decay value: {weight_decay}')
    for name, value in unit_interval.items():
        if torch.is_tensor(value) or not 0.0 <= value <= 1.0:
            raise ValueError(f'Invalid {name} value: {value}')
    if max_norm is not None and not (isinstance(max_norm, (int, float)) and max_norm >= 0.0):
        raise ValueError(f'Invalid max_norm: {max_norm}')


def _dense(t):
    return t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))


def _same_layout(a, b):
    return all(sa == sb for sa, sb, n in zip(a.stride(), b.stride(), a.shape) if n > 1)


def _on_hip(p):
    return p.is_cuda and torch.version.hip is not None and p.dtype == torch.float32 and not p.is_sparse and _dense(p)


def _workspace(opt, device, floats):
    """(partials, out) of one device, kept outside what is pickled; allocated once, grown only when the parameter set grows."""
    cache = opt.__dict__.setdefault('_workspaces', {})
    ws = cache.get(device)
    if ws is None or ws[0].numel() < floats:
        ws = cache[device] = (torch.empty(max(floats, 1), dtype=torch.float32, device=device), torch.zeros(2, dtype=torch.float32, device=device))
    return ws


def _table(items):
    """The HOST table of include/amtx_optim.h for (param, grad, state_a, state_b) tuples."""
    table = np.empty((len(items), 5), dtype=np.int64)
    for row, (p, g, a, b) in zip(table, items):
        row[0], row[1], row[2], row[3], row[4] = p.data_ptr(), g.data_ptr(), a.data_ptr(), b.data_ptr(), p.numel()
    return table


@torch.no_grad()
def _step(opt, kind):
    keys = _STATE_KEYS[kind]
    max_norm = opt.defaults.get('max_norm')
    hip, stock = [], []      # per group: {(device, step): [(p, g, a, b)]} and ([p], [g], [a], [b], [step])
    for group in opt.param_groups:
        for key in _TORCH_FLAGS[kind]:
            if group.get(key) not in (None, False):
                raise ValueError(f'amt_tools_amd.optim.{kind} does not implement {key}={group[key]!r} (set in a param group or a loaded state)')
        buckets, lists = {}, ([], [], [], [], [])
        for p in group['params']:
            g = p.grad
            if g is None:
                continue
            if g.is_sparse:
                raise RuntimeError(f'{kind} does not support sparse gradients')
            state = opt.state[p]
            if len(state) == 0:
                state['step'] = torch.tensor(0.0, dtype=torch.float32)
                for k in keys:
                    state[k] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if _on_hip(p):
                for k in keys:      # a state loaded from a checkpoint of another memory layout or dtype: brought to the parameter's, once
                    s = state[k]
                    if s.dtype != p.dtype or s.device != p.device or not _same_layout(s, p):
                        state[k] = torch.empty_like(p, memory_format=torch.preserve_format).copy_(s)
                if state['step'].device.type != 'cpu':      # a checkpoint of a capturable / fused optimizer
                    state['step'] = state['step'].to('cpu', torch.float32)
                if g.dtype != p.dtype or g.device != p.device or not _same_layout(g, p):
                    g = torch.empty_like(p, memory_format=torch.preserve_format).copy_(g)      # the one copy: the parameter's layout
                state['step'] += 1
                buckets.setdefault((p.device, float(state['step'])), []).append((p, g, state[keys[0]], state[keys[1]]))
            else:
                for lst, v in zip(lists, (p, g, state[keys[0]], state[keys[1]], state['step'])):
                    lst.append(v)
        hip.append(buckets)
        stock.append(lists)

    launches = 0
    sumsq = {}            # device -> the device float the update kernel reads
    norm = None
    if max_norm is not None:
        by_device = {}
        for buckets in hip:
            for (device, _), items in buckets.items():
                by_device.setdefault(device, []).extend(items)
        outs = {}
        for device, items in by_device.items():
            table = _table(items)
            floats = _lib.call('amtx_optim_num_blocks', np.ascontiguousarray(table[:, 4]), len(items))
            partials, out = _workspace(opt, device, floats)
            _lib.call('amtx_optim_grad_sumsq', table, len(items), partials, partials.numel(), out, device=device)
            launches += 1
            outs[device] = out
        stock_grads = [g for lists in stock for g in lists[1]]
        if len(outs) == 1 and not stock_grads:
            (device, out), = outs.items()
            sumsq[device], norm = out[0:1], out[1]
        elif not outs:
            if stock_grads:
                norm = torch.nn.utils.get_total_norm(stock_grads, 2.0)       # clip_grad_norm_'s own first half
        else:
            # parameters on both paths or on several devices: the squares meet on the first HIP device (torch glue; the stock path's
            # coefficient then takes a copy back to its device)
            first = next(iter(outs))
            total = sum(out[0].to(first) for out in outs.values())
            if stock_grads:
                total = total + torch.nn.utils.get_total_norm(stock_grads, 2.0).to(first, torch.float32) ** 2
            norm = total.sqrt()
            for device, out in outs.items():
                out[0] = total.to(device)
                out[1] = norm.to(device)
                sumsq[device] = out[0:1]
        if norm is not None and stock_grads:
            # clip_grad_norm_'s second half on COPIES: p.grad keeps its bits
            coef = torch.clamp(float(max_norm) / (norm + 1e-6), max=1.0)
            for lists in stock:
                lists[1][:] = [g * coef.to(g.device) for g in lists[1]]

    for group, buckets, lists in zip(opt.param_groups, hip, stock):
        for (device, step), items in buckets.items():
            table = _table(items)
            clip = (sumsq[device], float(max_norm)) if max_norm is not None else (None, 0.0)
            if kind == 'Adam':
                beta1, beta2 = group['betas']
                step_size = group['lr'] / (1 - beta1 ** step)
                bias_correction2_sqrt = (1 - beta2 ** step) ** 0.5
                launches += _lib.call('amtx_optim_adam_step', table, len(items), step_size, bias_correction2_sqrt, beta1, beta2, group['eps'],
                                      group['weight_decay'], *clip, device=device)
            else:
                launches += _lib.call('amtx_optim_adadelta_step', table, len(items), group['lr'], group['rho'], group['eps'],
                                      group['weight_decay'], *clip, device=device)
        params, grads, a, b, steps = lists
        if not params:
            continue
        has_complex = any(torch.is_complex(p) for p in params)
        if kind == 'Adam':
            beta1, beta2 = group['betas']
            _torch_adam(params, grads, a, b, [], steps, foreach=False, capturable=False, differentiable=False, fused=False,
                        has_complex=has_complex, amsgrad=False, beta1=beta1, beta2=beta2, lr=group['lr'], weight_decay=group['weight_decay'],
                        eps=group['eps'], maximize=False)
        else:
            _torch_adadelta(params, grads, a, b, steps, foreach=False, capturable=False, differentiable=False,
                            has_complex=has_complex, lr=group['lr'], rho=group['rho'], eps=group['eps'], weight_decay=group['weight_decay'],
                            maximize=False)
    opt.__dict__['launches_last_step'] = launches
    opt.__dict__['last_grad_norm'] = norm


def _run(opt, kind, closure):
    loss = None
    if closure is not None:
        with torch.enable_grad():
            loss = closure()
    _step(opt, kind)
    return loss


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam (amsgrad off, maximize off) with the step as one HIP launch; `max_norm`: global gradient-norm clipping in that launch."""
    launches_last_step = 0
    last_grad_norm = None

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, max_norm=None, **torch_flags):
        _refuse('Adam', dict(torch_flags, amsgrad=amsgrad))
        _check_hyper(lr, eps, weight_decay, max_norm, **{'beta parameter at index 0': betas[0], 'beta parameter at index 1': betas[1]})
        if betas[0] == 1.0 or betas[1] == 1.0:
            raise ValueError(f'Invalid beta parameters: {betas}')
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_norm=max_norm, **_TORCH_FLAGS['Adam']))

    def step(self, closure=None):
        return _run(self, 'Adam', closure)


class Adadelta(torch.optim.Optimizer):
    """torch.optim.Adadelta (maximize off) with the step as one HIP launch; `max_norm`: global gradient-norm clipping in that launch."""
    launches_last_step = 0
    last_grad_norm = None

    def __init__(self, params, lr=1.0, rho=0.9, eps=1e-6, weight_decay=0, foreach=None, *, max_norm=None, **torch_flags):
        _refuse('Adadelta', dict(torch_flags, foreach=foreach))
        _check_hyper(lr, eps, weight_decay, max_norm, rho=rho)
        super().__init__(params, dict(lr=lr, rho=rho, eps=eps, weight_decay=weight_decay, max_norm=max_norm, **_TORCH_FLAGS['Adadelta']))

    def step(self, closure=None):
        return _run(self, 'Adadelta', closure)
