"""tests/bn_ref.py without any kernel: the float64 reference agrees with nn.BatchNorm2d in float64, and every bound that
tests/test_gpu_bn_train.py holds the BatchNorm kernels to is met with a factor 3 to spare by an ideal fp32 evaluation (exact statistics
rounded once, fp32 per-element arithmetic) of the very same inputs -- so a bound the kernels miss is the kernels' doing, not the inputs'."""
import copy

import pytest

torch = pytest.importorskip('torch')

import bn_ref as R            # noqa: E402

CASES = R.bn_cases()
BY_NAME = {c['name']: c for c in CASES}


def _run(case, fn):
    t = case['make']()
    return t, fn(t['x'], t['gamma'], t['beta'], t['running_mean'], t['running_var'], case['eps'], case['momentum'], case['pool'],
                 t['gy'] if case['grads'] else None)


@pytest.mark.parametrize('name', [c['name'] for c in CASES])
def test_ideal_fp32_evaluation_meets_a_third_of_every_bound(name):
    """The stored mean is the one exception to the factor 3: rounding it to fp32 is already up to half of its allowance of one ulp."""
    case = BY_NAME[name]
    t, ref = _run(case, R.bn_relu_pool_ref)
    ideal = R.bn_relu_pool_ideal_fp32(t['x'], t['gamma'], t['beta'], t['running_mean'], t['running_var'], case['eps'], case['momentum'],
                                      case['pool'], t['gy'] if case['grads'] else None)
    rows = R.errors(case, ideal, ref)
    assert {k for k, _, _ in rows} >= {'y', 'running_mean', 'running_var', 'mean', 'invstd'}
    if case['grads']:
        assert {k for k, _, _ in rows} >= ({'dx', 'dgamma', 'dbeta'} if case['affine'] else {'dx'})
    for k, err, bound in rows:
        assert err <= (bound if k.startswith('mean') else bound / 3), (k, err, bound)


def test_cases_are_what_the_gpu_suite_is_meant_to_reach():
    names = [c['name'] for c in CASES]
    cond = [c for c in CASES if c['family'] == 'cond']
    assert len(cond) == 4 * 2 * 4 * 2 and {c['shape'] for c in cond} == set(R.COND_SHAPES)
    r = {}
    for c in cond:
        if c['shape'] == (2, 32, 9, 229) and not c['pool'] and not c['grads']:
            r[tuple(c['name'].split('-')[3:5])] =R.conditioning(_run(c, R.bn_relu_pool_ref)[1], c['eps'])
    assert r[('0.3', '1.5')] < 0.5 and 6 < r[('10', '1.5')] < 15 and 190 < r[('10', '0.05')] < 450 and 1900 < r[('100', '0.05')] < 4500, r
    # degenerate channels: exactly zero variance, 1 / sqrt(eps)
    case = BY_NAME['degenerate-pool']
    t, ref = _run(case, R.bn_relu_pool_ref)
    assert ref['var'][1] == 0 and ref['var'][2] == 0 and 0 < ref['var'][3] < 1e-3
    assert torch.equal(ref['invstd'][1:3], torch.full((2,), case['eps'], dtype=torch.float64).rsqrt())
    assert 5 < R.conditioning(ref, case['eps'], slice(4, None)) < 15
    # the ReLU of every gradient case of the ill-conditioned families is open, with room for an fp32 evaluation
    for c in CASES:
        if c['family'] != 'well' and c['grads']:
            t, ref = _run(dict(c, pool=False, grads=False), R.bn_relu_pool_ref)
            assert ref['y'].min() > 1.0, c['name']
    # the dead channel is dead, the tied pairs are tied, the cap case passes the cap
    t, ref = _run(dict(BY_NAME['well-gamma-signs-flat'], grads=False), R.bn_relu_pool_ref)
    assert ref['y'][:, 3].max() == 0 and ref['y'][:, 2].min() == ref['y'][:, 2].max() > 0 and t['gamma'][1] < 0
    t = BY_NAME['well-ties']['make']()
    assert torch.equal(t['x'][0, :, :, 1::2], t['x'][0, :, :, 0::2]) and not torch.equal(t['x'][1, :, :, 1::2], t['x'][1, :, :, 0::2])
    B, C, T, F = R.CAP_SHAPE
    assert 'well-cap' in names and B * T * F > 1024 * 16 * (256 // (C // 4))


@pytest.mark.parametrize('name', ['cond-1x48x7x18-pool-10-1.5-fwd', 'well-module-momentum-0.01'])
def test_reference_matches_batchnorm2d_module_in_float64(name):
    case = BY_NAME[name]
    t = case['make']()
    C = case['shape'][1]
    bn = torch.nn.BatchNorm2d(C, eps=case['eps'], momentum=case['momentum']).double()
    with torch.no_grad():
        bn.weight.copy_(t['gamma'])
        bn.bias.copy_(t['beta'])
        bn.running_mean.copy_(t['running_mean'])
        bn.running_var.copy_(t['running_var'])
    mod = torch.nn.Sequential(bn, torch.nn.ReLU(), torch.nn.MaxPool2d((1, 2)))
    x = t['x'].double().requires_grad_(True)
    y = mod(x)
    y.backward(t['gy'].double())
    ref = R.bn_relu_pool_ref(t['x'], t['gamma'], t['beta'], t['running_mean'], t['running_var'], case['eps'], case['momentum'], True, t['gy'])
    assert int(bn.num_batches_tracked) == 1
    for k, want in (('y', y.detach()), ('dx', x.grad), ('dgamma', bn.weight.grad), ('dbeta', bn.bias.grad), ('running_mean', bn.running_mean),
                    ('running_var', bn.running_var)):
        assert ref[k].dtype == torch.float64 and torch.equal(ref[k], want), k
    # the statistics the reference reports are the ones the module used: running statistics from them, unbiased variance
    n = x.numel() // C
    m = case['momentum']
    assert torch.allclose(ref['running_mean'], (1 - m) * t['running_mean'].double() + m * ref['mean'], rtol=1e-13, atol=0)
    assert torch.allclose(ref['running_var'], (1 - m) * t['running_var'].double() + m * ref['var'] * n / (n - 1), rtol=1e-12, atol=0)
    assert torch.allclose(ref['invstd'], (ref['var'] + case['eps']).rsqrt(), rtol=1e-15, atol=0)
    # a second step counts on
    mod(x.detach())
    assert int(bn.num_batches_tracked) == 2
    # the inputs of a case are the same on every call, and the reference leaves them alone
    t2 = copy.deepcopy(case)['make']()
    assert all(torch.equal(t[k], t2[k]) for k in t)
