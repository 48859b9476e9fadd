"""amt_tools_amd.optim on the CPU: parameters that do not qualify for the HIP launch go through torch's own functional update, so the classes
give torch's bits here; state exchange with torch's classes, the reference's resume re-init, pickling, the refused keywords, clipping,
the pure launch split of csrc/optim.hip, and the classes under DataParallelOptimizer over two gloo ranks.  No GPU."""
import io
import os
import pickle
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from amt_tools_amd import _lib, optim, tools
from amt_tools_amd.dp import DataParallelOptimizer, broadcast_parameters, shard_indices
from amt_tools_amd.models import OnsetsFrames

SHAPES = [(7,), (3, 5), (4, 2, 3, 3), ()]
PAIRS = [(optim.Adam, torch.optim.Adam, dict(lr=6e-4)), (optim.Adadelta, torch.optim.Adadelta, dict(lr=1.0))]
IDS = ['Adam', 'Adadelta']


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g) * 0.1) for s in SHAPES]


def _grads(step, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + step)
    return [torch.randn(s, generator=g) * 10.0 ** (i - 2) for i, s in enumerate(SHAPES)]


def _set_grads(params, step, skip_odd=None):
    """Fresh gradients of `step`; parameter `skip_odd` has no gradient at odd steps."""
    for i, (p, g) in enumerate(zip(params, _grads(step))):
        p.grad = None if (i == skip_odd and step % 2 == 1) else g.clone()


def _assert_same(opt_a, params_a, opt_b, params_b):
    for a, b in zip(params_a, params_b):
        np.testing.assert_array_equal(a.detach().numpy(), b.detach().numpy())
        sa, sb = opt_a.state.get(a, {}), opt_b.state.get(b, {})
        assert sorted(sa) == sorted(sb)
        for k in sa:
            assert sa[k].dtype == sb[k].dtype and sa[k].shape == sb[k].shape and sa[k].device == sb[k].device, k
            np.testing.assert_array_equal(sa[k].numpy(), sb[k].numpy())


@pytest.mark.parametrize('weight_decay', [0, 1e-2])
@pytest.mark.parametrize('mine,theirs,kw', PAIRS, ids=IDS)
def test_cpu_parameters_get_the_bits_of_torchs_class(mine, theirs, kw, weight_decay):
    pa, pb = _params(), _params()
    a, b = mine(pa, weight_decay=weight_decay, **kw), theirs(pb, weight_decay=weight_decay, **kw)
    for step in range(5):
        _set_grads(pa, step, skip_odd=1)
        _set_grads(pb, step, skip_odd=1)
        a.step()
        b.step()
        _assert_same(a, pa, b, pb)
    assert float(a.state[pa[1]]['step']) == 3.0 and float(a.state[pa[0]]['step']) == 5.0      # a step without a gradient is no step
    assert a.state[pa[0]]['step'].dtype == torch.float32 and a.state[pa[0]]['step'].device.type == 'cpu' and a.state[pa[0]]['step'].dim() == 0
    assert a.launches_last_step == 0 and a.last_grad_norm is None
    assert type(a).__bases__ == (torch.optim.Optimizer,)


def test_a_parameter_that_never_had_a_gradient_gets_no_state():
    params = _params()
    opt = optim.Adam(params)
    _set_grads(params, 0)
    params[2].grad = None
    opt.step()
    assert params[2] not in opt.state and len(opt.state) == 3


@pytest.mark.parametrize('mine,theirs,kw', PAIRS, ids=IDS)
@pytest.mark.parametrize('first', ['mine', 'theirs'])
def test_state_dicts_are_exchanged_with_torchs_class(mine, theirs, kw, first):
    """Three steps with one class, its state_dict loaded into the other, two more steps: the bits of five uninterrupted steps."""
    kw = dict(kw, weight_decay=1e-2)
    ref_p = _params()
    ref = theirs(ref_p, **kw)
    for step in range(5):
        _set_grads(ref_p, step)
        ref.step()
    pa = _params()
    a = (mine if first == 'mine' else theirs)(pa, **kw)
    for step in range(3):
        _set_grads(pa, step)
        a.step()
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    b = (theirs if first == 'mine' else mine)(pb, **kw)
    b.load_state_dict(a.state_dict())
    for step in range(3, 5):
        _set_grads(pb, step)
        b.step()
    _assert_same(b, pb, ref, ref_p)


@pytest.mark.parametrize('mine,theirs,kw', PAIRS, ids=IDS)
def test_resume_reinit_saved_state_and_pickle(mine, theirs, kw):
    """amt_tools/train.py:111 re-runs the base-class __init__ in place with (params, defaults) and then loads the saved state; the
    state_dict goes through torch.save / torch.load; the optimizer object itself pickles and goes on stepping."""
    kw = dict(kw, max_norm=3.0)
    ref_p, pa = _params(), _params()
    ref, a = mine(ref_p, **kw), mine(pa, **kw)
    for step in range(4):
        _set_grads(ref_p, step)
        ref.step()
    for step in range(2):
        _set_grads(pa, step)
        a.step()
    buf = io.BytesIO()
    torch.save(a.state_dict(), buf)
    buf.seek(0)
    saved = torch.load(buf)
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    super(type(a), a).__init__(pb, a.defaults)
    assert a.defaults['max_norm'] == 3.0 and len(a.state) == 0
    a.load_state_dict(saved)
    _set_grads(pb, 2)
    a.step()
    b = pickle.loads(pickle.dumps(a))
    assert sorted(a.__getstate__()) == ['defaults', 'param_groups', 'state']          # no workspace, no table: nothing device-bound is pickled
    pc = b.param_groups[0]['params']
    _set_grads(pc, 3)
    b.step()
    _assert_same(b, pc, ref, ref_p)
    assert b.last_grad_norm is not None


def test_keywords_that_are_not_implemented_raise_value_error():
    p = _params()
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(foreach=True), dict(fused=True), dict(capturable=True), dict(differentiable=True),
               dict(decoupled_weight_decay=True), dict(lr=torch.tensor(1e-3)), dict(lr=-1.0), dict(betas=(1.0, 0.999)), dict(max_norm=-1.0)):
        with pytest.raises(ValueError):
            optim.Adam(p, **kw)
    for kw in (dict(maximize=True), dict(foreach=True), dict(capturable=True), dict(differentiable=True), dict(lr=torch.tensor(1.0)), dict(rho=1.5),
               dict(eps=-1.0)):
        with pytest.raises(ValueError):
            optim.Adadelta(p, **kw)
    with pytest.raises(TypeError):
        optim.Adam(p, momentum=0.9)
    with pytest.raises(TypeError):
        optim.Adadelta(p, amsgrad=False)                       # not a keyword of torch's Adadelta either
    optim.Adam(p, amsgrad=False, foreach=None, fused=None)     # torch's defaults spelled out are what is implemented
    opt = optim.Adam(p)
    opt.param_groups[0]['amsgrad'] = True
    _set_grads(p, 0)
    with pytest.raises(ValueError, match='amsgrad'):
        opt.step()


@pytest.mark.parametrize('max_norm', [3.0, 1e6])
@pytest.mark.parametrize('mine,theirs,kw', PAIRS, ids=IDS)
def test_clipping_on_cpu_is_clip_grad_norm_on_copies(mine, theirs, kw, max_norm):
    pa, pb = _params(), _params()
    a, b = mine(pa, max_norm=max_norm, **kw), theirs(pb, **kw)
    for step in range(3):
        _set_grads(pa, step, skip_odd=0)
        _set_grads(pb, step, skip_odd=0)
        kept = [None if p.grad is None else p.grad.clone() for p in pa]
        a.step()
        total = torch.nn.utils.clip_grad_norm_(pb, max_norm)
        b.step()
        _assert_same(a, pa, b, pb)
        np.testing.assert_array_equal(a.last_grad_norm.numpy(), total.numpy())
        for p, g in zip(pa, kept):
            assert (p.grad is None) == (g is None) and (g is None or torch.equal(p.grad, g))      # p.grad keeps its bits
    assert float(total) > 3.0


def test_launch_split_query():
    cap = _lib.call('amtx_optim_num_launches', np.ones(10000, dtype=np.int64), 10000)
    with open(os.path.join(os.path.dirname(_lib.HEADER_PATH), 'amtx_optim.h')) as f:
        text = f.read()
    capacity = int(text.split('#define AMTX_OPTIM_MAX_TENSORS')[1].split()[0])
    chunk = int(text.split('#define AMTX_OPTIM_CHUNK')[1].split()[0])
    assert capacity >= 48 and cap == -(-10000 // capacity)
    for n, launches in ((1, 1), (capacity, 1), (capacity + 1, 2), (3 * capacity + 2, 4)):
        numels = np.full(n, 5, dtype=np.int64)
        assert _lib.call('amtx_optim_num_launches', numels, n) == launches
        assert _lib.call('amtx_optim_num_blocks', numels, n) == n
    numels = np.array([0, chunk, chunk + 1, 0, 3 * chunk - 1, 1], dtype=np.int64)
    assert _lib.call('amtx_optim_num_blocks', numels, 6) == 0 + 1 + 2 + 0 + 3 + 1 and _lib.call('amtx_optim_num_launches', numels, 6) == 1
    assert _lib.call('amtx_optim_num_launches', np.zeros(capacity + 1, dtype=np.int64), capacity + 1) == 0      # nothing to launch
    tail = np.array([0] * capacity + [1], dtype=np.int64)
    assert _lib.call('amtx_optim_num_launches', tail, capacity + 1) == 1 and _lib.call('amtx_optim_num_launches', None, 0) == 0
    with pytest.raises(_lib.AmtxError, match='negative numel'):
        _lib.call('amtx_optim_num_launches', np.array([4, -1], dtype=np.int64), 2)
    with pytest.raises(_lib.AmtxError, match='num_tensors'):
        _lib.call('amtx_optim_num_launches', numels, 2 ** 31)


def test_entry_points_refuse_bad_tables_before_any_launch():
    """Null pointers where a tensor has elements, negative sizes, more tensors than an int holds, an address that is no float's: the
    project's argument error (-1) with a message; nothing is launched, so this needs no GPU."""
    L = _lib.lib()
    host = np.zeros(8, dtype=np.float32)
    a = host.ctypes.data
    good = [a, a, a, a, 4]

    def adam(table, n=None, sumsq=None, max_norm=0.0):
        t = np.array(table, dtype=np.int64).reshape(-1, 5)
        return L.amtx_optim_adam_step(_lib.ptr(t), len(t) if n is None else n, 1e-3, 1.0, 0.9, 0.999, 1e-8, 0.0, sumsq, max_norm, None)

    def adadelta(table):
        t = np.array(table, dtype=np.int64).reshape(-1, 5)
        return L.amtx_optim_adadelta_step(_lib.ptr(t), len(t), 1.0, 0.9, 1e-6, 0.0, None, 0.0, None)

    for col in range(4):
        bad = list(good)
        bad[col] = 0
        for fn in (adam, adadelta):
            assert fn([good, bad]) == -1 and b'tensor 1: null pointer' in L.amtx_last_error()
    assert adam([a, a, a, a, -4]) == -1 and b'numel=-4' in L.amtx_last_error()
    assert adam([a, a + 2, a, a, 4]) == -1 and b'4-byte aligned' in L.amtx_last_error()
    assert adam(good, n=2 ** 31) == -1 and b'num_tensors' in L.amtx_last_error()
    assert adam(good, n=-1) == -1
    assert adam(good, sumsq=_lib.ptr(host), max_norm=-1.0) == -1 and b'max_norm' in L.amtx_last_error()
    assert L.amtx_optim_adam_step(None, 1, 1e-3, 1.0, 0.9, 0.999, 1e-8, 0.0, None, 0.0, None) == -1 and b'null table' in L.amtx_last_error()
    assert L.amtx_optim_adam_step(_lib.ptr(np.array(good, dtype=np.int64)), 1, 1e-3, 0.0, 0.9, 0.999, 1e-8, 0.0, None, 0.0, None) == -1
    # numel 0 is legal whatever its addresses hold, and an empty table launches nothing
    assert adam([0, 0, 0, 0, 0]) == 0 and adadelta([0, 0, 0, 0, 0]) == 0 and adam([], n=0) == 0
    t = np.array([[0, 0, 0, 0, 4]], dtype=np.int64)
    assert L.amtx_optim_grad_sumsq(_lib.ptr(t), 1, _lib.ptr(host), 8, _lib.ptr(host), None) == -1 and b'null pointer' in L.amtx_last_error()
    t = np.array([[0, a, 0, 0, 4]], dtype=np.int64)                # the sum of squares looks at the gradient column alone
    assert L.amtx_optim_grad_sumsq(_lib.ptr(t), 1, _lib.ptr(host), 0, _lib.ptr(host), None) == -1 and b'partials holds 0 floats' in L.amtx_last_error()
    assert L.amtx_optim_grad_sumsq(_lib.ptr(t), 1, _lib.ptr(host), 8, None, None) == -1 and b'null out' in L.amtx_last_error()


# ------------------------------------------------------------------------------------------------------------------------------
# under DataParallelOptimizer, two gloo ranks (the manner of tests/test_dp.py)
# ------------------------------------------------------------------------------------------------------------------------------
DIM_IN, T = 16, 10


def _make_model(seed):
    torch.manual_seed(seed)
    model = OnsetsFrames(DIM_IN, tools.PianoProfile(), 1, 2)
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    return model


def _batch(idx):
    rng = np.random.default_rng(100 + idx)
    return {tools.KEY_FEATS: torch.from_numpy(rng.random((1, 1, DIM_IN, T)).astype(np.float32)),
            tools.KEY_MULTIPITCH: torch.from_numpy((rng.random((1, 88, T)) < 0.1).astype(np.float32)),
            tools.KEY_ONSETS: torch.from_numpy((rng.random((1, 88, T)) < 0.03).astype(np.float32))}


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    states = {}
    for name, cls in (('mine', optim.Adam), ('torch', torch.optim.Adam)):
        model = _make_model(seed=rank)
        broadcast_parameters(model, src=0)
        opt = DataParallelOptimizer(model.parameters(), optimizer_cls=cls, lr=1e-2)
        for it in range(2):
            mine = [_batch(4 * it + i) for i in shard_indices(4, rank, world)]
            opt.zero_grad()
            batch = {k: torch.cat([b[k] for b in mine]) for k in mine[0]}
            model.run_on_batch(batch)[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL].backward()
            opt.step()
        states[name] = {k: v.clone() for k, v in model.state_dict().items()}
        states[name + '_views'] = all(p.grad.data_ptr() >= opt._flat.data_ptr() for p in model.parameters())
        states[name + '_steps'] = float(opt.state_dict()['state'][0]['step'])
    torch.save(states, out + f'.{rank}')
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


@pytest.mark.timeout(300)
def test_two_gloo_ranks_end_with_torchs_weights_on_both_ranks(tmp_path):
    out = str(tmp_path / 'dp')
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = torch.load(out + '.0'), torch.load(out + '.1')
    assert r0['mine_views'] and r0['mine_steps'] == 2.0
    for k, v in r0['mine'].items():
        assert torch.equal(v, r1['mine'][k]), k                 # identical on both ranks
        assert torch.equal(v, r0['torch'][k]), k                # ... and what optimizer_cls=torch.optim.Adam leaves: the same functional update
