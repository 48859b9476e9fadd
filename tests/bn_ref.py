"""Training-mode BatchNorm2d -> ReLU -> [MaxPool2d((1, 2))] of csrc/bn.hip: a float64 reference, the best an fp32 kernel behind the same
interface can do, the cases the tests run and the bounds they are held to.

Host only: imports nothing but torch, calls no kernel.  tests/test_bn_ref.py pins the reference to nn.BatchNorm2d in float64 and proves
that every bound is reachable, with a factor 3 to spare, on the very inputs tests/test_gpu_bn_train.py feeds the kernels.

Tensors are torch's: x (B, C, T, F), gy like the output (B, C, T, F // 2 or F); the kernels' channels-last memory [B][T][F][C] is
x.contiguous(memory_format=torch.channels_last).  r = max over channels of |mean| / sqrt(var + eps) is the conditioning of a case: the
kernels hand the batch mean to their second pass as an fp32 number (stats [4][C]), whose rounding alone moves xhat by up to 2^-25 r.

Bounds (bounds(r, family)), each relative to the largest reference element of the tensor:
    y                      2e-6 + 2^-24 r        dx, dbeta   2e-5 + 2^-24 r        dgamma   2e-5 + 2^-22 r
    running mean / var     1e-6 + 2^-24 r
    stats mean             |mean - ref| <= 2^-23 |ref| + 1e-7 sqrt(var_ref + eps)      stats invstd   4e-6 relative
The constants are what tests/test_gpu_train.py::test_bn_relu_pool_training_matches_torch has always asserted; the family 'well'
(r about 0.2) holds them without the r term.
"""
import torch

FAMILIES = ('cond', 'degenerate', 'well')
MEAN_ULP, MEAN_ABS_STD, INVSTD_REL = 2.0 ** -23, 1e-7, 4e-6


def bounds(r, family):
    """Relative bounds of one case; r is not credited to the well-conditioned family."""
    rr = 0.0 if family == 'well' else float(r)
    return {'y': 2e-6 + 2.0 ** -24 * rr, 'dx': 2e-5 + 2.0 ** -24 * rr, 'dbeta': 2e-5 + 2.0 ** -24 * rr, 'dgamma': 2e-5 + 2.0 ** -22 * rr,
            'running_mean': 1e-6 + 2.0 ** -24 * rr, 'running_var': 1e-6 + 2.0 ** -24 * rr}


def rel(a, b):
    """max |a - b| over the largest |b| (tests/test_gpu_train.py::_rel)."""
    return (a.double() - b.double()).abs().max().item() / max(1e-12, b.double().abs().max().item())


def conditioning(ref, eps, channels=slice(None)):
    return (ref['mean'][channels].abs() / (ref['var'][channels] + eps).sqrt()).max().item()


# ------------------------------------------------------------------------------------------------------------------------------
# float64 reference: torch's own batch_norm, relu, max_pool2d and autograd
# ------------------------------------------------------------------------------------------------------------------------------
def bn_relu_pool_ref(x, gamma, beta, running_mean, running_var, eps, momentum, pool, gy=None):
    """Everything in float64; gamma / beta may be None (no affine), gy may be None (no backward).  Returns a dict: y, dx, dgamma, dbeta
    (None without gy / affine), mean, var (biased), invstd [C], running_mean, running_var (updated copies: the unbiased variance goes
    into running_var, like nn.BatchNorm2d)."""
    F = torch.nn.functional
    x64 = x.detach().double().requires_grad_(gy is not None)
    g64 = None if gamma is None else gamma.detach().double().requires_grad_(gy is not None)
    b64 = None if beta is None else beta.detach().double().requires_grad_(gy is not None)
    rm, rv = running_mean.detach().double().clone(), running_var.detach().double().clone()
    y = torch.relu(F.batch_norm(x64, rm, rv, g64, b64, training=True, momentum=momentum, eps=eps))
    if pool:
        y = F.max_pool2d(y, (1, 2))
    out = {'y': y.detach(), 'dx': None, 'dgamma': None, 'dbeta': None, 'running_mean': rm, 'running_var': rv}
    if gy is not None:
        y.backward(gy.double())
        out['dx'] = x64.grad
        out['dgamma'] = None if g64 is None else g64.grad
        out['dbeta'] = None if b64 is None else b64.grad
    xd = x.detach().double()
    out['mean'] = xd.mean(dim=(0, 2, 3))
    out['var'] = (xd - out['mean'].view(1, -1, 1, 1)).square().mean(dim=(0, 2, 3))          # two-pass: exactly 0 for a constant channel
    out['invstd'] = 1.0 / (out['var'] + eps).sqrt()
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the best an fp32 kernel with stats [4][C] can do: exact statistics and sums, rounded once; fp32 per-element arithmetic
# ------------------------------------------------------------------------------------------------------------------------------
def bn_relu_pool_ideal_fp32(x, gamma, beta, running_mean, running_var, eps, momentum, pool, gy=None):
    """Mean, variance and the two backward sums in float64, rounded to fp32; every per-element step in fp32 in the kernels' order:
    z = ((x - mean) * invstd) * gamma + beta; the pooling pair's winner is the first on z0 >= z1; dz = gy where the winner's z > 0;
    dx = gamma * invstd * (dz - c0 - xhat * c1) with c0 = sum(dz) / n, c1 = sum(dz * xhat) / n.  Not a model of csrc/bn.hip: it only
    shows what the interface allows.  Same dict as bn_relu_pool_ref, fp32 tensors."""
    assert x.dtype == torch.float32
    B, C, T, F = x.shape
    n = B * T * F
    ref = bn_relu_pool_ref(x, None, None, running_mean, running_var, eps, momentum, False)
    mean, invstd = ref['mean'].float(), ref['invstd'].float()
    g = torch.ones(C) if gamma is None else gamma.float()
    b = torch.zeros(C) if beta is None else beta.float()
    v = lambda t: t.view(1, C, 1, 1)                               # noqa: E731
    xhat = (x - v(mean)) * v(invstd)
    z = xhat * v(g) + v(b)
    if pool:
        Fo = F // 2
        z0, z1 = z[..., 0:2 * Fo:2], z[..., 1:2 * Fo:2]
        first = z0 >= z1
        zmax = torch.where(first, z0, z1)
    else:
        zmax = z
    out = {'y': zmax.clamp_min(0.0), 'dx': None, 'dgamma': None, 'dbeta': None, 'mean': mean, 'var': ref['var'].float(), 'invstd': invstd,
           'running_mean': ref['running_mean'].float(), 'running_var': ref['running_var'].float()}
    if gy is None:
        return out
    d = torch.where(zmax > 0, gy.float(), torch.zeros(()))
    dz = torch.zeros_like(x)
    if pool:
        dz[..., 0:2 * Fo:2] = torch.where(first, d, torch.zeros(()))
        dz[..., 1:2 * Fo:2] = torch.where(first, torch.zeros(()), d)
    else:
        dz = d
    s = dz.double().sum(dim=(0, 2, 3))
    q = (dz.double() * xhat.double()).sum(dim=(0, 2, 3))
    c0, c1 = (s / n).float(), (q / n).float()
    out['dx'] = v(g * invstd) * (dz - v(c0) - xhat * v(c1))
    if gamma is not None:
        out['dgamma'], out['dbeta'] = q.float(), s.float()
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# checks shared by the CPU test (ideal fp32, a third of every bound) and the GPU test (the kernels, the whole bound)
# ------------------------------------------------------------------------------------------------------------------------------
def errors(case, got, ref):
    """[(name, measured, bound)] of everything `case` asks to be checked in `got` (a dict like bn_relu_pool_ref's; stats mean / invstd
    only where got holds them).  The mean's figure is |mean - ref| over its own allowance, bound 1.  A case with `regular_from` is
    checked a second time over the channels from there on alone, at their own r and their own largest elements."""
    eps, fam = case['eps'], case['family']
    rows = []
    for lo in (0,) + ((case['regular_from'],) if case.get('regular_from') else ()):
        bd = bounds(conditioning(ref, eps, slice(lo, None)), fam)
        tag = f'[{lo}:]' if lo else ''
        names = ['y', 'running_mean', 'running_var'] + (['dx', 'dgamma', 'dbeta'] if case['grads'] else [])
        for k in names:
            if ref[k] is None:
                assert got[k] is None, k
                continue
            a, b = (got[k][:, lo:], ref[k][:, lo:]) if ref[k].dim() == 4 else (got[k][lo:], ref[k][lo:])
            rows.append((k + tag, rel(a, b), bd[k]))
        if got.get('mean') is not None:
            m, mr, vr = got['mean'][lo:].double(), ref['mean'][lo:], ref['var'][lo:]
            rows.append(('mean' + tag, ((m - mr).abs() / (MEAN_ULP * mr.abs() + MEAN_ABS_STD * (vr + eps).sqrt())).max().item(), 1.0))
            rows.append(('invstd' + tag, ((got['invstd'][lo:].double() - ref['invstd'][lo:]).abs() / ref['invstd'][lo:]).max().item(), INVSTD_REL))
    return rows


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
COND_SHAPES = ((2, 32, 9, 229), (1, 48, 7, 18), (2, 4, 3, 5), (1, 80, 3, 57))
COND_OFFSET_STD = ((0.3, 1.5), (10.0, 1.5), (10.0, 0.05), (100.0, 0.05))
CAP_SHAPE = (1, 512, 90, 400)                    # 36000 positions, 2 per block: more than the 1024 partials hold without wrapping


def _case(name, family, shape, pool, make, grads=True, eps=1e-5, momentum=0.1, via='abi', affine=True, regular_from=None, **kw):
    return dict(name=name, family=family, shape=shape, pool=pool, make=make, grads=grads, eps=eps, momentum=momentum, via=via,
                affine=affine, regular_from=regular_from, **kw)


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31)


def _inputs(name, shape, pool, offset=0.3, std=1.5, alternate=False, open_relu=False, edit=None):
    """x = randn * std + offset; with `alternate` the offset's sign alternates over the channels and the odd ones have half the spread; gamma = rand + 0.5; beta = randn * 0.2, or 8 gamma (`open_relu`: every
    pre-activation positive); running_mean = randn * 0.1; running_var = rand + 0.5; gy = randn.  `edit(t)` may change the dict in place."""
    B, C, T, F = shape
    g = torch.Generator().manual_seed(_seed(name))
    x = torch.randn(B, C, T, F, generator=g)
    if not alternate:
        x = x * std + offset
    else:
        sign = torch.tensor([1.0 if c % 2 == 0 else -1.0 for c in range(C)]).view(1, C, 1, 1)
        scale = torch.tensor([std if c % 2 == 0 else 0.5 * std for c in range(C)]).view(1, C, 1, 1)
        x = x * scale + sign * offset
    gamma = torch.rand(C, generator=g) + 0.5
    beta = 8.0 * gamma if open_relu else torch.randn(C, generator=g) * 0.2
    t = {'x': x, 'gamma': gamma, 'beta': beta, 'running_mean': torch.randn(C, generator=g) * 0.1, 'running_var': torch.rand(C, generator=g) + 0.5,
         'gy': torch.randn(B, C, T, F // 2 if pool else F, generator=g)}
    if edit is not None:
        edit(t)
    t['x'] = t['x'].float().contiguous()
    return t


def _degenerate(t):
    x = t['x']
    x[:, 1] = 100.1                              # a dead filter: its bias everywhere
    x[:, 2] = 0.0
    x[:, 3] = 10.0
    x[1, 3, 4, 100] = 11.5                       # constant but for one element


def _ties(t):
    x = t['x']
    x[0, :, :, 1::2] = x[0, :, :, 0:-1:2]        # half the map: both members of every pooling pair are the same number


def _gamma_signs(t):
    t['gamma'][1] = -t['gamma'][1]               # the pair's winner is the smaller x
    t['gamma'][2] = 0.0                          # every z = beta: the first member wins
    t['beta'][2] = 0.3
    t['beta'][3] = -20.0                         # no pre-activation of this channel is positive: y = 0, dz = 0


def _null_affine(t):
    t['gamma'] = t['beta'] = None


def bn_cases():
    """Every input of tests/test_gpu_bn_train.py, by name; case['make']() builds the tensors (seeded, no files)."""
    cases = []
    add = lambda *a, **k: cases.append(_case(*a, **k))                                   # noqa: E731

    def gen(name, shape, pool, **kw):
        return lambda: _inputs(name, shape, pool, **kw)

    # conditioning family: forward checks with the usual affine, gradient checks with the ReLU held open
    for shape in COND_SHAPES:
        for pool in (False, True):
            for offset, std in COND_OFFSET_STD:
                for grads in (False, True):
                    name = f'cond-{"x".join(map(str, shape))}-{"pool" if pool else "flat"}-{offset:g}-{std:g}-{"grad" if grads else "fwd"}'
                    add(name, 'cond', shape, pool, gen(name, shape, pool, offset=offset, std=std, alternate=True, open_relu=grads), grads=grads)
    # degenerate variance
    for pool in (False, True):
        name = f'degenerate-{"pool" if pool else "flat"}'
        add(name, 'degenerate', (2, 32, 9, 229), pool, gen(name, (2, 32, 9, 229), pool, offset=10.0, std=1.5, alternate=True, open_relu=True, edit=_degenerate),
            regular_from=4, constant=(1, 2))
    # structure and edges, well-conditioned.  Positions per block of the statistics pass = 16 x (256 threads / (C / 4) groups):
    #   C = 4: 4096, 80: 192, 160: 96, 260: 48 (65 groups, 3 rows, 61 idle threads), 1024: 16 (one row) -- two blocks each
    for shape, pool in (((2, 4, 33, 64), True), ((2, 80, 5, 21), False), ((1, 160, 6, 18), True), ((1, 260, 5, 11), True), ((1, 1024, 3, 7), True),
                        ((1, 1024, 3, 7), False)):
        name = f'well-channels-{"x".join(map(str, shape))}-{"pool" if pool else "flat"}'
        add(name, 'well', shape, pool, gen(name, shape, pool))
    add('well-cap', 'well', CAP_SHAPE, True, gen('well-cap', CAP_SHAPE, True))
    for shape in ((2, 8, 3, 3), (2, 8, 3, 2), (1, 8, 1, 8)):      # unpaired last column; one pair per row; a single row
        name = f'well-pooled-{"x".join(map(str, shape))}'
        add(name, 'well', shape, True, gen(name, shape, True))
    add('well-ties', 'well', (2, 8, 4, 12), True, gen('well-ties', (2, 8, 4, 12), True, edit=_ties))
    for pool in (False, True):
        name = f'well-gamma-signs-{"pool" if pool else "flat"}'
        add(name, 'well', (2, 8, 4, 12), pool, gen(name, (2, 8, 4, 12), pool, edit=_gamma_signs), dead=3)
    add('well-null-affine', 'well', (2, 8, 4, 12), True, gen('well-null-affine', (2, 8, 4, 12), True, edit=_null_affine), affine=False)
    for momentum in (0.01, 1.0):
        name = f'well-module-momentum-{momentum:g}'
        add(name, 'well', (2, 8, 4, 12), True, gen(name, (2, 8, 4, 12), True), eps=1e-3, momentum=momentum, via='autograd')
    assert len({c['name'] for c in cases}) == len(cases)
    return cases
