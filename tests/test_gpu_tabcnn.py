"""TabCNN on the HIP engine (csrc/tab.hip, amtx_tab_*): eval-mode inference under no_grad on a GPU, against the reference's golden
logits and the stock torch path on the CPU (itself pinned to the reference by tests/test_model_cpu.py)."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

from amt_tools_amd import _lib, autograd, tools
from amt_tools_amd.models import TabCNN, _TabEngine
from amt_tools_amd.synth import synth_clip, synth_tabcnn_state_dict

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
# max |logit - fp32 reference logit|.  x3: measured 1.53e-5 on the golden fixture and 2.34e-5 at config-1 size (B 2 x 1292 frames),
# gated at 5e-5; the other shapes are held to the project's fp32-class 1e-4.  bf16: measured 1.27e-2 at config-1 size, gated at 2.5e-2
# -- and asserted NOT to be within 1e-4 (the throughput mode).
X3_GATE = 5e-5
SHAPE_GATE = 1e-4
BF16_GATE = 2.5e-2


def _sd(seed, **kw):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in synth_tabcnn_state_dict(seed, **kw).items()}


def _model(dim_in, frets=19, in_channels=1, device=DEV, precision='x3', seed=0, online=False):
    profile = tools.GuitarProfile(num_frets=frets)
    m = TabCNN(dim_in, profile, in_channels, 1, device=device, precision=precision)
    m.load_state_dict(_sd(seed, dim_in=dim_in, in_channels=in_channels, num_groups=6, num_classes=frets + 2))
    m.change_device()
    m.eval()
    if online:
        m.toggle_online()
    return m


def _feats(B, Cc, Fd, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((B, Cc, Fd, T), generator=g)                    # CQT features lie in [0, 1]


@torch.no_grad()
def _logits_and_tab(model, feats):
    pre = model.pre_proc({tools.KEY_FEATS: feats})
    out = {tools.KEY_OUTPUT: model(pre[tools.KEY_FEATS])}
    logits = out[tools.KEY_OUTPUT][tools.KEY_TABLATURE]
    tab = model.post_proc(out)[tools.KEY_TABLATURE]
    return logits.cpu().numpy(), tab.cpu().numpy()


def _compare(got, ref, classes, gate):
    """max logit error; tablature equal except where the reference's two best classes of a group are within 2x the gate."""
    (lg, tg), (lr, tr) = got, ref
    err = float(np.abs(lg - lr).max())
    top2 = np.sort(lr.reshape(lr.shape[0], lr.shape[1], -1, classes), axis=-1)[..., -2:]
    near = np.swapaxes(top2[..., 1] - top2[..., 0], -1, -2) < 2 * gate            # (B, G, T)
    diff = tg != tr
    assert not np.any(diff & ~near), (err, int(diff.sum()))
    return err, int(diff.sum())


def _engine_runs(model):
    eng = model.__dict__.get('_engine')
    return 0 if eng is None else eng.forwards


def test_golden_fixture_x3():
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'tabcnn_eval.npz'))
    before = autograd.fallback_total()
    model = _model(int(g['dim_in']), seed=int(g['seed']))
    feats = torch.from_numpy(g['feats'])
    with torch.no_grad():
        pre = model.pre_proc({tools.KEY_FEATS: feats})
        raw = model(pre[tools.KEY_FEATS])[tools.KEY_TABLATURE]
        out = model.run_on_batch({tools.KEY_FEATS: feats, tools.KEY_TABLATURE: torch.from_numpy(g['tablature_ref'])})
    err = float(np.abs(raw.cpu().numpy() - g['logits']).max())
    print(f'golden x3 max logit error {err:.2e}')
    assert err < X3_GATE
    np.testing.assert_array_equal(out[tools.KEY_TABLATURE].cpu().numpy(), g['out_tablature'])
    assert abs(out[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL].item() - float(g['loss_total'])) < 1e-4
    assert _engine_runs(model) == 2 and autograd.fallback_total() == before


@pytest.fixture(scope='module')
def config1():
    """B = 2 GuitarSet-length tracks (1292 frames), dim_in 192: inputs and the stock path's results on the CPU."""
    feats = _feats(2, 1, 192, 1292, seed=7)
    return feats, _logits_and_tab(_model(192, device='cpu', seed=3), feats)


@pytest.mark.parametrize('precision', ['x3', 'bf16'])
def test_engine_matches_stock_at_config1_size(config1, precision):
    feats, ref = config1
    model = _model(192, seed=3, precision=precision)
    got = _logits_and_tab(model, feats.to(DEV))
    assert _engine_runs(model) == 1
    gate = X3_GATE if precision == 'x3' else BF16_GATE
    err, ndiff = _compare(got, ref, 21, gate)
    print(f'{precision}: max logit error {err:.2e}, {ndiff} of {got[1].size} tablature cells differ (near-ties)')
    assert err < gate
    if precision == 'x3':
        assert ndiff <= 10
    else:
        assert err > 1e-4                                       # bf16 is the throughput mode, not fp32-class
        assert ndiff <= 0.01 * got[1].size


SHAPES = [dict(dim_in=145, T=30), dict(dim_in=192, in_channels=6, T=20), dict(dim_in=192, frets=22, T=20), dict(dim_in=9, T=12),
          dict(dim_in=384, T=17)] + [dict(dim_in=192, T=t) for t in (1, 8, 9, 10, 63, 64, 65)] + \
         [dict(dim_in=192, T=t, online=True) for t in (5, 9, 40)] + [dict(dim_in=48, T=33, B=7), dict(dim_in=48, T=12, B=1)]


@pytest.mark.parametrize('case', SHAPES, ids=lambda c: '-'.join(f'{k}{v}' for k, v in c.items()))
def test_shapes_against_stock(case):
    case = dict(case)
    B, T = case.pop('B', 2), case.pop('T')
    Cc = case.get('in_channels', 1)
    feats = _feats(B, Cc, case['dim_in'], T, seed=T)
    before = autograd.fallback_total()
    ref = _logits_and_tab(_model(device='cpu', seed=5, **case), feats)
    model = _model(seed=5, **case)
    got = _logits_and_tab(model, feats.to(DEV))
    assert _engine_runs(model) == 1 and autograd.fallback_total() == before
    assert got[0].shape == ref[0].shape and got[1].shape == ref[1].shape
    err, ndiff = _compare(got, ref, case.get('frets', 19) + 2, SHAPE_GATE)
    print(f'{case} B {B} T {T}: max logit error {err:.2e}, {ndiff} near-tie cells differ')
    assert err < SHAPE_GATE, err


def test_copy_of_windows_and_grad_enabled_take_the_stock_path():
    model = _model(64, seed=2)
    feats = _feats(2, 1, 64, 21).to(DEV)
    win = model.pre_proc({tools.KEY_FEATS: feats})[tools.KEY_FEATS]

    def stock(w):
        B, T = w.shape[:2]
        return model.dense(model.conv(w.reshape(B * T, 1, 64, 9)).reshape(B, T, -1))

    with torch.no_grad():
        eng = model(win)[tools.KEY_TABLATURE]
        assert _engine_runs(model) == 1
        cp = model(win.contiguous())[tools.KEY_TABLATURE]
        assert _engine_runs(model) == 1
        torch.testing.assert_close(cp, stock(win.contiguous()), rtol=0, atol=1e-6)
    out = model(win)[tools.KEY_TABLATURE]                              # grad enabled, parameters require grad
    assert out.requires_grad and _engine_runs(model) == 1
    with torch.no_grad():
        torch.testing.assert_close(out.detach(), stock(win), rtol=0, atol=1e-6)
    assert float((out.detach() - eng).abs().max()) < X3_GATE
    # a training-mode forward never touches the engine
    model.train()
    model(win)
    assert _engine_runs(model) == 1


def test_unsupported_configuration_is_noted():
    before = autograd.fallback_total()
    m = TabCNN(40, tools.GuitarProfile(num_frets=19), 1, 2, device=DEV)
    m.change_device()
    m.eval()
    with torch.no_grad():
        out = m.run_on_batch({tools.KEY_FEATS: _feats(1, 1, 40, 10)})
    assert out[tools.KEY_TABLATURE].shape == (1, 6, 10) and '_engine' not in m.__dict__
    assert autograd.fallback_total() == before + 1 and 'TabCNN.forward' in autograd.fallbacks()


def test_weight_resync():
    model = _model(96, seed=4)
    cpu = _model(96, seed=4, device='cpu')
    feats = _feats(2, 1, 96, 25)
    _logits_and_tab(model, feats.to(DEV))
    with torch.no_grad():
        model.conv[2].weight[3, 5, 1, 1] += 0.25
        model.dense[0].bias.add_(0.1)
        cpu.conv[2].weight[3, 5, 1, 1] += 0.25
        cpu.dense[0].bias.add_(0.1)
    err, _ = _compare(_logits_and_tab(model, feats.to(DEV)), _logits_and_tab(cpu, feats), 21, X3_GATE)
    assert err < X3_GATE


def test_workspace_guard_bands_and_chunking(monkeypatch):
    monkeypatch.setattr(_lib, 'GUARD_BYTES', 4096)
    model = _model(80, seed=6)
    for B, T in ((3, 1), (1, 37), (5, 66), (2, 9)):
        _logits_and_tab(model, _feats(B, 1, 80, T, seed=B + T).to(DEV))
        ws = model.__dict__['_engine'].workspace
        assert ws._base is not None and _lib.guards_intact(ws), (B, T)
    feats = _feats(5, 1, 80, 150, seed=1).to(DEV)
    whole = _logits_and_tab(model, feats)
    eng = model.__dict__['_engine']
    monkeypatch.setattr(_TabEngine, 'WORKSPACE_CAP', eng.workspace_bytes(2, 40))
    eng.workspace = None
    assert len(eng._chunks(5, 150)) > 4
    part = _logits_and_tab(model, feats)
    assert _lib.guards_intact(eng.workspace) and eng.workspace.numel() <= eng.workspace_bytes(2, 40)
    assert np.abs(part[0] - whole[0]).max() < 1e-5
    _compare(part, whole, 21, 1e-5)


def test_end_to_end_audio_batched():
    from amt_tools_amd.features import CQT
    from amt_tools_amd.inference import run_offline, run_offline_batched
    clips = np.stack([synth_clip(i, num_samples=3 * 22050) for i in range(3)]).astype(np.float32)
    mod = CQT(sample_rate=22050, hop_length=512, n_bins=192, bins_per_octave=24)
    model = _model(192, seed=8)
    model.frontend = torch.nn.Sequential(mod.frontend())
    res = run_offline_batched(clips, model, batch_size=2)
    runs = _engine_runs(model)
    assert runs == 2
    stock = _model(192, seed=8)
    for i in range(3):
        with torch.no_grad():                                                          # as validate() runs it
            one = run_offline({tools.KEY_AUDIO: clips[i]}, model)
        np.testing.assert_array_equal(res[i][tools.KEY_TABLATURE], one[tools.KEY_TABLATURE])
        feats = torch.from_numpy(mod.process_audio(clips[i])[None]).to(DEV)           # the same HIP features, stock model on the GPU
        win = stock.pre_proc({tools.KEY_FEATS: feats})[tools.KEY_FEATS].contiguous()
        with torch.no_grad():
            lr = stock(win)[tools.KEY_TABLATURE]
            tr = stock.dense[-1].finalize_output(lr)
        same = one[tools.KEY_TABLATURE][None] == tr.cpu().numpy()
        top2 = np.sort(lr.cpu().numpy().reshape(1, -1, 6, 21), axis=-1)[..., -2:]
        near = np.swapaxes(top2[..., 1] - top2[..., 0], -1, -2) < 2 * X3_GATE
        assert np.all(same | near), i
    assert _engine_runs(model) == runs + 3


def test_pickle_and_deepcopy_after_engine_ran():
    model = _model(64, seed=9)
    feats = _feats(2, 1, 64, 19).to(DEV)
    first = _logits_and_tab(model, feats)
    assert '_engine' in model.__dict__
    for clone in (copy.deepcopy(model), pickle.loads(pickle.dumps(model))):
        assert '_engine' not in clone.__dict__
        again = _logits_and_tab(clone, feats)
        np.testing.assert_array_equal(again[0], first[0])
        np.testing.assert_array_equal(again[1], first[1])
