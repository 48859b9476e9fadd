"""The training-mode BatchNorm + ReLU + MaxPool kernels (csrc/bn.hip) against torch in float64, on the inputs and at the bounds of
tests/bn_ref.py: channels whose mean is large against their spread (r = |mean| / std up to about 4500), channels of exactly zero
variance, every channel-count path of the statistics pass, the capped grid, odd and minimal pooled widths, exact pooling ties, negative
and zero gamma, a dead channel, no affine parameters, and nn.BatchNorm2d's bookkeeping through autograd.bn_relu_pool.

The C ABI is called directly so that stats [4][C] (mean, invstd, gamma, beta) can be held to its own bounds.  tests/test_bn_ref.py shows
on the CPU that an ideal fp32 evaluation of the same inputs meets a third of every bound asserted here; each figure is printed before it
is asserted (pytest -s)."""
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import bn_ref as R                                   # noqa: E402
from amt_tools_amd import _lib, autograd             # noqa: E402

DEV = 'cuda:0'
CASES = R.bn_cases()
BY_NAME = {c['name']: c for c in CASES}


@pytest.fixture(autouse=True)
def guarded_workspaces(monkeypatch):
    monkeypatch.setattr(_lib, 'GUARD_BYTES', 256)


def _reference(case):
    """Inputs and float64 reference of a case: every case belongs to one test, which computes them once and leaves them unchanged."""
    t = case['make']()
    return t, R.bn_relu_pool_ref(t['x'], t['gamma'], t['beta'], t['running_mean'], t['running_var'], case['eps'], case['momentum'],
                                 case['pool'], t['gy'] if case['grads'] else None)


def _cl(t):
    """(B, C, T, F) -> the kernels' memory [B][T][F][C] on the device."""
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _run_abi(case, t):
    B, C, T, F = case['shape']
    Fo = F // 2 if case['pool'] else F
    dev = lambda v: None if v is None else v.to(DEV)                                 # noqa: E731
    x, gamma, beta = _cl(t['x']), dev(t['gamma']), dev(t['beta'])
    rm, rv = t['running_mean'].to(DEV), t['running_var'].to(DEV)
    y = torch.empty((B, C, T, Fo), device=DEV, memory_format=torch.channels_last)
    stats = torch.empty((4, C), device=DEV)
    ws = _lib.alloc_workspace(int(_lib.call('amtx_bn_train_workspace_bytes', C)), DEV)
    _lib.call('amtx_bn_relu_pool_train_fwd', x, B * T, F, C, int(case['pool']), gamma, beta, float(case['eps']), float(case['momentum']), rm, rv,
              y, stats, ws, ws.numel(), device=DEV)
    got = {'y': y, 'running_mean': rm, 'running_var': rv, 'mean': stats[0], 'invstd': stats[1], 'stats': stats, 'dx': None, 'dgamma': None,
           'dbeta': None}
    if case['grads']:
        gy = _cl(t['gy'])
        dx = torch.empty_like(x, memory_format=torch.channels_last)
        dgamma = torch.empty(C, device=DEV) if case['affine'] else None
        dbeta = torch.empty(C, device=DEV) if case['affine'] else None
        _lib.call('amtx_bn_relu_pool_train_bwd', x, B * T, F, C, int(case['pool']), stats, gy, dx, dgamma, dbeta, ws, ws.numel(), device=DEV)
        got.update(dx=dx, dgamma=dgamma, dbeta=dbeta)
    torch.cuda.synchronize()
    assert ws._base is not None and _lib.guards_intact(ws), 'a BatchNorm kernel wrote outside its workspace'
    return got


def _run_module(case, t):
    C = case['shape'][1]
    bn = torch.nn.BatchNorm2d(C, eps=case['eps'], momentum=case['momentum'])
    with torch.no_grad():
        bn.weight.copy_(t['gamma'])
        bn.bias.copy_(t['beta'])
        bn.running_mean.copy_(t['running_mean'])
        bn.running_var.copy_(t['running_var'])
    bn = bn.to(DEV)
    x = _cl(t['x']).requires_grad_(True)
    assert autograd.bn_relu_pool_supported(x, bn)
    y = autograd.bn_relu_pool(x, bn, case['pool'])
    y.backward(_cl(t['gy']))
    return {'y': y.detach(), 'running_mean': bn.running_mean, 'running_var': bn.running_var, 'dx': x.grad, 'dgamma': bn.weight.grad,
            'dbeta': bn.bias.grad, 'mean': None, 'invstd': None}, bn


def _check(case, got, ref):
    cpu = {k: None if v is None else v.detach().cpu() for k, v in got.items()}
    rows = R.errors(case, cpu, ref)
    print(f'\n{case["name"]}: r = {R.conditioning(ref, case["eps"]):.4g}')
    for k, err, bound in rows:
        print(f'    {k:18s} {err:.3e}   bound {bound:.3e}')
    for k, err, bound in rows:
        assert err <= bound, (case['name'], k, err, bound)
    for v in cpu.values():
        assert v is None or bool(torch.isfinite(v).all())
    return cpu


@pytest.mark.parametrize('name', [c['name'] for c in CASES if c['via'] == 'abi'])
def test_bn_relu_pool_train_kernels_match_float64(name):
    case = BY_NAME[name]
    t, ref = _reference(case)
    got = _run_abi(case, t)
    cpu = _check(case, got, ref)
    C = case['shape'][1]
    # stats rows 2, 3: the affine parameters as the second pass reads them (1, 0 without)
    assert torch.equal(cpu['stats'][2], t['gamma'] if case['affine'] else torch.ones(C))
    assert torch.equal(cpu['stats'][3], t['beta'] if case['affine'] else torch.zeros(C))
    for c in case.get('constant', ()):
        # an exactly constant channel: variance 0 in the reference, so invstd = 1 / sqrt(eps) and y = relu(beta)
        assert ref['var'][c] == 0
        assert abs(cpu['invstd'][c].item() * case['eps'] ** 0.5 - 1) <= R.INVSTD_REL
        assert R.rel(cpu['y'][:, c], ref['y'][:, c]) <= 2e-6
    if 'dead' in case:
        assert cpu['y'][:, case['dead']].abs().max() == 0 and cpu['dbeta'][case['dead']] == 0 and cpu['dgamma'][case['dead']] == 0
    if name == 'well-null-affine':
        ones = dict(t, gamma=torch.ones(C), beta=torch.zeros(C))
        same = _run_abi(dict(case, affine=True), ones)
        assert all(torch.equal(same[k], got[k]) for k in ('y', 'dx', 'stats', 'running_mean', 'running_var'))
    # deterministic: fixed summation order, no atomics
    again = _run_abi(case, t)
    assert all(got[k] is None or torch.equal(again[k], got[k]) for k in got), name


@pytest.mark.parametrize('name', [c['name'] for c in CASES if c['via'] == 'autograd'])
def test_bn_relu_pool_module_bookkeeping(name):
    """autograd.bn_relu_pool with nn.BatchNorm2d's own eps and momentum (1.0: the running statistics become the batch's), counting
    num_batches_tracked."""
    case = BY_NAME[name]
    t, ref = _reference(case)
    got, bn = _run_module(case, t)
    _check(case, got, ref)
    assert int(bn.num_batches_tracked) == 1
    if case['momentum'] == 1.0:
        n = t['x'].numel() // case['shape'][1]
        assert R.rel(bn.running_mean.cpu(), ref['mean']) <= 1e-6 and R.rel(bn.running_var.cpu(), ref['var'] * n / (n - 1)) <= 1e-6
    autograd.bn_relu_pool(_cl(t['x']), bn, case['pool'])
    assert int(bn.num_batches_tracked) == 2
