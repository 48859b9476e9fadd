"""amt_tools_amd.optim on the GPU (csrc/optim.hip).  Yardstick: torch's own class on the CPU in float64, from the same float32 starting values
and the same float32 gradients -- never the kernel itself.

Tolerance, derived: after K steps a float32 parameter has been rounded K times, at most half an ulp each (2^-24 |p|); the update's own
rounding is a few ulps of a step far smaller than max|p|.  Per tensor max|p_hip - p_64| <= K * 2^-23 * max|p_64|, twice the rounding
bound, and the same form for each state map against its own maximum.  The parameters move 1e-3 .. 5e-2 in ten steps, so a missed element,
a wrong bias correction or a swapped state map misses by four orders of magnitude.  Every case prints its worst ratio to the bound."""
import functools
import os

import numpy as np
import pytest
import torch

from amt_tools_amd import _lib, autograd, optim, tools

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
K = 10
with open(os.path.join(os.path.dirname(_lib.HEADER_PATH), 'amtx_optim.h')) as _f:
    _text = _f.read()
CAPACITY = int(_text.split('#define AMTX_OPTIM_MAX_TENSORS')[1].split()[0])
CHUNK = int(_text.split('#define AMTX_OPTIM_CHUNK')[1].split()[0])

CLASSES = {'Adam': (optim.Adam, torch.optim.Adam, dict(lr=6e-4)), 'Adadelta': (optim.Adadelta, torch.optim.Adadelta, dict(lr=1.0))}
STATE = {'Adam': ('exp_avg', 'exp_avg_sq'), 'Adadelta': ('square_avg', 'acc_delta')}
SHAPES = {'list': [(n,) for n in (1, 3, 4, 5, 63, 64, 65, 1023, 1025, 4099, 0, CHUNK + 1)],
          'conv': [(32, 32, 3, 3)],
          'many': [(5,)] * (CAPACITY + 3)}


@functools.lru_cache(maxsize=None)
def _inputs(which, steps=K, zero_grads=False):
    """(float32 starting values, float32 gradients per step): randn * 0.1, gradient scale 10^((i mod 5) - 3) for tensor i."""
    g = torch.Generator().manual_seed(sorted(SHAPES).index(which))
    p0 = [torch.randn(s, generator=g) * 0.1 for s in SHAPES[which]]
    if zero_grads:
        return p0, [[torch.zeros(s) for s in SHAPES[which]] for _ in range(steps)]
    grads = [[torch.randn(s, generator=g) * 10.0 ** (i % 5 - 3) for i, s in enumerate(SHAPES[which])] for _ in range(steps)]
    return p0, grads


@functools.lru_cache(maxsize=None)
def _reference(kind, which, weight_decay, max_norm=None, steps=K):
    """torch's class on the CPU in float64: per tensor (p, state_a, state_b) after `steps` steps, and the gradient norm of every step."""
    p0, grads = _inputs(which, steps)
    params = [torch.nn.Parameter(p.double()) for p in p0]
    opt = CLASSES[kind][1](params, weight_decay=weight_decay, **CLASSES[kind][2])
    norms = []
    for k in range(steps):
        for p, g in zip(params, grads[k]):
            p.grad = g.double()
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm)))
        opt.step()
    return [(p.detach(), opt.state[p][STATE[kind][0]], opt.state[p][STATE[kind][1]]) for p in params], norms


def _check(tag, kind, opt, params, ref, steps):
    """Every parameter and state map within steps * 2^-23 * max|reference| of the float64 reference; prints the worst ratio."""
    worst = 0.0
    for i, (p, (rp, ra, rb)) in enumerate(zip(params, ref)):
        if p.numel() == 0:
            assert p not in opt.state or opt.state[p][STATE[kind][0]].numel() == 0
            continue
        st = opt.state[p]
        assert float(st['step']) == steps and st['step'].device.type == 'cpu' and st['step'].dtype == torch.float32
        for name, got, want in (('param', p.detach(), rp), (STATE[kind][0], st[STATE[kind][0]], ra), (STATE[kind][1], st[STATE[kind][1]], rb)):
            assert got.dtype == torch.float32 and got.shape == want.shape and got.stride() == p.stride()
            err = float((got.cpu().double() - want).abs().max())
            bound = steps * 2.0 ** -23 * float(want.abs().max())
            assert err <= bound, (tag, i, name, err, bound)
            worst = max(worst, err / bound)
    print(f'[{tag}] worst error / bound over parameters and state maps: {worst:.3f}')
    return worst


def _run(kind, params, grads_of_step, steps=K, **kw):
    """`steps` steps of the class under test; grads_of_step(k) -> the device gradients of step k (assigned as they are)."""
    opt = CLASSES[kind][0](params, **dict(CLASSES[kind][2], **kw))
    launches = []
    for k in range(steps):
        for p, g in zip(params, grads_of_step(k)):
            p.grad = g
        opt.step()
        launches.append(opt.launches_last_step)
    torch.cuda.synchronize()
    return opt, launches


CONFIGS = [(kind, wd) for kind in ('Adam', 'Adadelta') for wd in (0, 1e-2)]


@pytest.mark.parametrize('kind,wd', CONFIGS)
def test_own_allocations(kind, wd):
    p0, grads = _inputs('list')
    params = [torch.nn.Parameter(p.to(DEV)) for p in p0]
    dgrads = [[g.to(DEV) for g in gs] for gs in grads]
    opt, launches = _run(kind, params, lambda k: dgrads[k], weight_decay=wd)
    assert launches == [1] * K and opt.last_grad_norm is None
    _check(f'own allocations {kind} wd {wd}', kind, opt, params, _reference(kind, 'list', wd)[0], K)
    for k in (0, K - 1):                                   # gradients are read, never written
        assert all(torch.equal(d.cpu(), g) for d, g in zip(dgrads[k], grads[k]))


def _flat(tensors, fill_values):
    """One flat buffer holding the tensors back to back behind one guard word (odd offsets: most views are only 4-byte aligned), one more
    guard word after every third tensor and 64 at the end; guard words hold a NaN pattern.  -> (flat, views, guard mask)."""
    offs, off = [], 1
    for i, t in enumerate(tensors):
        offs.append(off)
        off += t.numel() + (i % 3 == 2)
    total = off + 64
    bits = torch.full((total,), 0x7FC0BEEF, dtype=torch.int32)
    flat = bits.view(torch.float32).clone()
    guard = torch.ones(total, dtype=torch.bool)
    for t, o in zip(tensors, offs):
        n = t.numel()
        flat[o:o + n] = t.reshape(-1) if fill_values else 0.0
        guard[o:o + n] = False
    flat = flat.to(DEV)
    return flat, [flat[o:o + t.numel()].view(t.shape) for t, o in zip(tensors, offs)], guard


@pytest.mark.parametrize('kind,wd', CONFIGS)
def test_views_at_odd_offsets_of_flat_buffers_and_the_words_between_them(kind, wd):
    """Parameters, gradients and both state maps are views into flat buffers, the DataParallelOptimizer situation; most tensors are only 4-byte
    aligned (the one-element-per-lane path), a few land on 16 bytes (float4 beside guard words).  No word outside a tensor changes."""
    p0, grads = _inputs('list')
    pflat, pviews, guard = _flat(p0, True)
    params = [torch.nn.Parameter(v) for v in pviews]
    assert all(p.data_ptr() == v.data_ptr() for p, v in zip(params, pviews))
    assert sum(p.data_ptr() % 16 != 0 for p in params) >= 6 and sum(p.data_ptr() % 16 == 0 and p.numel() > 4 for p in params) >= 1
    gflats = [_flat(gs, True) for gs in grads]
    gbefore = [gf[0].clone() for gf in gflats]
    aflat, aviews, _ = _flat(p0, False)
    bflat, bviews, _ = _flat(p0, False)
    opt = CLASSES[kind][0](params, weight_decay=wd, **CLASSES[kind][2])
    for p, a, b in zip(params, aviews, bviews):
        opt.state[p] = {'step': torch.tensor(0.0), STATE[kind][0]: a, STATE[kind][1]: b}
    for k in range(K):
        for p, g in zip(params, gflats[k][1]):
            p.grad = g
        opt.step()
        assert opt.launches_last_step == 1
    torch.cuda.synchronize()
    for p, a, b in zip(params, aviews, bviews):            # the state maps are still the views handed in
        assert opt.state[p][STATE[kind][0]].data_ptr() == a.data_ptr() and opt.state[p][STATE[kind][1]].data_ptr() == b.data_ptr()
    _check(f'flat views {kind} wd {wd}', kind, opt, params, _reference(kind, 'list', wd)[0], K)
    for name, flat in (('param', pflat), ('state_a', aflat), ('state_b', bflat)):
        words = flat.cpu().view(torch.int32)[guard]
        assert bool((words == 0x7FC0BEEF).all()), name
    for gf, before in zip(gflats, gbefore):
        assert torch.equal(gf[0].view(torch.int32), before.view(torch.int32))


@pytest.mark.parametrize('grad_layout', ['channels_last', 'contiguous'])
@pytest.mark.parametrize('kind', ['Adam', 'Adadelta'])
def test_channels_last_parameter(kind, grad_layout):
    """A conv weight held channels-last; its gradient channels-last too, or contiguous (brought to the parameter's layout by one copy)."""
    p0, grads = _inputs('conv')
    params = [torch.nn.Parameter(p0[0].to(DEV).contiguous(memory_format=torch.channels_last))]
    fmt = torch.channels_last if grad_layout == 'channels_last' else torch.contiguous_format
    dgrads = [[gs[0].to(DEV).contiguous(memory_format=fmt)] for gs in grads]
    assert params[0].stride() == (288, 1, 96, 32) and (dgrads[0][0].stride() == params[0].stride()) == (grad_layout == 'channels_last')
    opt, launches = _run(kind, params, lambda k: dgrads[k], weight_decay=1e-2)
    assert launches == [1] * K
    _check(f'channels-last parameter, {grad_layout} gradient, {kind}', kind, opt, params, _reference(kind, 'conv', 1e-2)[0], K)


@pytest.mark.parametrize('kind', ['Adam', 'Adadelta'])
def test_a_table_longer_than_one_launch(kind):
    """AMTX_OPTIM_MAX_TENSORS + 3 tensors of 5 elements: the launches the pure query answers, and every tensor updated.  K steps like the
    other cases: the bound's form is for K = 10 (after two steps torch's own float32 acc_delta is already 1.17 of it on these inputs)."""
    p0, grads = _inputs('many')
    params = [torch.nn.Parameter(p.to(DEV)) for p in p0]
    dgrads = [[g.to(DEV) for g in gs] for gs in grads]
    opt, launches = _run(kind, params, lambda k: dgrads[k], weight_decay=1e-2)
    numels = np.full(len(params), 5, dtype=np.int64)
    assert launches == [_lib.call('amtx_optim_num_launches', numels, len(params))] * K == [2] * K
    _check(f'{len(params)} tensors {kind}', kind, opt, params, _reference(kind, 'many', 1e-2)[0], K)


@pytest.mark.parametrize('kind', ['Adam', 'Adadelta'])
def test_zero_gradients_leave_every_bit(kind):
    p0, grads = _inputs('list', 3, True)
    params = [torch.nn.Parameter(p.to(DEV)) for p in p0]
    dgrads = [[g.to(DEV) for g in gs] for gs in grads]
    opt, _ = _run(kind, params, lambda k: dgrads[k], steps=3, weight_decay=0)
    for p, start in zip(params, p0):
        assert torch.equal(p.detach().cpu().view(torch.int32), start.view(torch.int32))
        for key in STATE[kind]:
            assert p.numel() == 0 or not bool(opt.state[p][key].view(torch.int32).any())      # the fresh state's +0.0 words


@pytest.mark.parametrize('max_norm', [3.0, 1e6])
@pytest.mark.parametrize('kind', ['Adam', 'Adadelta'])
def test_clipping_inside_the_launch(kind, max_norm):
    """Yardstick: clip_grad_norm_ on the float64 gradients, then the float64 step.  last_grad_norm within 2^-20 relative of the float64 norm
    (a fixed-order float32 sum of 13 block partials of at most 4096 squares each); p.grad keeps its bits; two runs from the same start give
    the same bits, also with the partials buffer and the result pre-filled with NaN."""
    p0, grads = _inputs('list')
    ref, ref_norms = _reference(kind, 'list', 1e-2, max_norm)
    assert min(ref_norms) > 100.0                             # well above 3; far below 1e6
    runs = []
    for poison in (False, True):
        params = [torch.nn.Parameter(p.to(DEV)) for p in p0]
        dgrads = [[g.to(DEV) for g in gs] for gs in grads]
        opt = CLASSES[kind][0](params, weight_decay=1e-2, max_norm=max_norm, **CLASSES[kind][2])
        if poison:
            partials, out = optim._workspace(opt, params[0].device, 4096)
            partials.fill_(float('nan'))
            out.fill_(float('nan'))
        worst = 0.0
        for k in range(K):
            for p, g in zip(params, dgrads[k]):
                p.grad = g
            opt.step()
            assert opt.launches_last_step == 2                # the sum of squares, the update
            norm = opt.last_grad_norm
            assert norm.device == params[0].device and norm.dim() == 0
            worst = max(worst, abs(float(norm) - ref_norms[k]) / ref_norms[k])
        assert worst <= 2.0 ** -20, worst
        print(f'[clipping {kind} max_norm {max_norm}] worst relative error of last_grad_norm {worst:.2e} (bound {2.0 ** -20:.2e})')
        for k in (0, K - 1):
            assert all(torch.equal(d.cpu().view(torch.int32), g.view(torch.int32)) for d, g in zip(dgrads[k], grads[k]))
        _check(f'clipping {kind} max_norm {max_norm}{" (poisoned partials)" if poison else ""}', kind, opt, params, ref, K)
        runs.append([p.detach().cpu() for p in params])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------------
# integration on real models: torch's GPU step is the yardstick here (same seed, same kernels in front of the optimizer)
# ------------------------------------------------------------------------------------------------------------------------------
def _of_model_and_batch():
    from amt_tools_amd.models import OnsetsFrames
    from amt_tools_amd.synth import synth_labels
    torch.manual_seed(0)
    model = OnsetsFrames(229, tools.PianoProfile(), 1, 2, device=DEV)
    model.change_device()
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    B, T = 2, 64
    lab = [synth_labels(i, num_frames=T) for i in range(B)]
    g = torch.Generator().manual_seed(1)
    batch = {tools.KEY_FEATS: torch.rand(B, 1, 229, T, generator=g), tools.KEY_MULTIPITCH: torch.from_numpy(np.stack([l[0] for l in lab])),
             tools.KEY_ONSETS: torch.from_numpy(np.stack([l[1] for l in lab]))}
    return model, batch


def _tab_model_and_batch():
    from amt_tools_amd.models import TabCNN
    from amt_tools_amd.synth import synth_tabcnn_state_dict
    model = TabCNN(192, tools.GuitarProfile(num_frets=19), 1, 1, device=DEV)
    sd = synth_tabcnn_state_dict(0, dim_in=192, in_channels=1, model_complexity=1, num_groups=6, num_classes=21)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.change_device()
    model.train()
    B, T = 2, 16
    g = torch.Generator().manual_seed(1)
    return model, {tools.KEY_FEATS: torch.rand((B, 1, 192, T), generator=g), tools.KEY_TABLATURE: torch.randint(-1, 21, (B, 6, T), generator=g)}


def _two_training_steps(make, cls, **kw):
    model, batch = make()
    opt = cls(model.parameters(), **kw)
    after, launches = [], []
    before = autograd.fallback_total()
    for _ in range(2):
        opt.zero_grad()
        model.run_on_batch(batch)[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL].backward()
        opt.step()
        after.append({k: p.detach().clone() for k, p in model.named_parameters()})
        launches.append(getattr(opt, 'launches_last_step', None))
    torch.cuda.synchronize()
    return after, launches, autograd.fallback_total() - before, (model, batch, opt)


@pytest.mark.parametrize('name', ['OnsetsFrames-Adam', 'TabCNN-Adadelta'])
def test_two_training_steps_against_torchs_gpu_step(name):
    """Two training steps (Dropout p = 0) with the class under test and, from the same seed, with torch's class on the GPU: after each step
    every parameter within 2 * 2^-23 * max|torch's|, one launch per step, no fallback taken.  Measured on an MI355X: every parameter
    bit-identical (the kernel rounds where torch's multi-tensor kernels round).  The second step is what makes this sharp: the gradient of a
    conv bias in front of BatchNorm is rounding noise, and a one-ulp difference after the first step moves such a bias by lr at the second."""
    make, mine, theirs, kw = {'OnsetsFrames-Adam': (_of_model_and_batch, optim.Adam, torch.optim.Adam, dict(lr=6e-4)),
                              'TabCNN-Adadelta': (_tab_model_and_batch, optim.Adadelta, torch.optim.Adadelta, dict(lr=1.0))}[name]
    got, launches, moved, _ = _two_training_steps(make, mine, **kw)
    want, _, _, _ = _two_training_steps(make, theirs, **kw)
    assert launches == [1, 1] and moved == 0
    worst, at = 0.0, None
    for step in range(2):
        for k, w in want[step].items():
            err = float((got[step][k].double() - w.double()).abs().max())
            bound = 2 * 2.0 ** -23 * float(w.abs().max())
            if bound > 0 and err / bound > worst:
                worst, at = err / bound, (step, k, err, bound)
    print(f'[{name}] {len(want[0])} parameter tensors, worst error / bound against torch on the GPU: {worst:.3f} at {at}')
    for step in range(2):
        for k, w in want[step].items():
            err = float((got[step][k].double() - w.double()).abs().max())
            assert err <= 2 * 2.0 ** -23 * float(w.abs().max()), (step, k, err)


def test_the_step_is_the_new_kernel_and_no_aten_kernel():
    _, _, _, (model, batch, opt) = _two_training_steps(_of_model_and_batch, optim.Adam, lr=6e-4)
    opt.zero_grad()
    model.run_on_batch(batch)[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL].backward()
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        opt.step()
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA or 'kernel' in e.key.lower()]
    assert any('optim_step_kernel' in n for n in names), names
    assert not [n for n in names if 'multi_tensor_apply' in n or 'vectorized_elementwise' in n], names
