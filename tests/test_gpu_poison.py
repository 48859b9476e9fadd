"""No result may depend on memory nobody initialised: stale workspace contents, pad columns, halo rows, partial-sum slots, output elements
a kernel forgot to write.  The rest of the GPU suite cannot see such a read -- a fresh engine per case gets zero pages from the driver, the
guard pattern 0xA5 is a harmless finite number and only detects writes, and a repeated call gets its previous output block back from the
caching allocator.  Here every case runs with all allocations (tests/poison.py: torch.empty / torch.empty_like wrapped) and every
persistent workspace filled with 0x00, then 0xFF (NaN; -1 as an integer), then 0x7F (3.39e38; NaN as f16; 2139062143 as an int32 count),
same inputs, weights and seeds: what the public call returns must be BIT-IDENTICAL across the fills and free of NaN / Inf.  The engine
cases also run a shape sequence on ONE engine object, a large call first: the small calls then see the large call's real, finite,
plausible activations beyond their own rows, and must still return the bits of the same call on a fresh engine.

Equality without a tolerance rests on the determinism the suite already asserts (test_engine_is_deterministic_run_to_run,
test_two_steps_from_the_same_seed_are_bit_identical, the bit-for-bit DP tests).  Raw buffers that are partly valid by design (the `pairs`
of amtx_notes_decode beyond `counts`) are not compared: only what the API returns.  LDS and registers cannot be poisoned from a test."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from amt_tools_amd import _lib, autograd, tools                                             # noqa: E402
from amt_tools_amd.synth import synth_clip, synth_state_dict, synth_tabcnn_state_dict       # noqa: E402
from poison import PATTERNS, Poison, assert_same, fill_storage, refill, snapshot            # noqa: E402

DEV = 'cuda:0'
SEQUENCE = ((44, 140), (3, 17), (1, 1), (17, 9))        # (clips, frames): a large call first, then smaller and ragged ones


@pytest.fixture
def poison(monkeypatch):
    return Poison(monkeypatch, 0x00)


def _tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------------------------------------
# Onsets & Frames engine: amtx_of_forward (+ amtx_of_offsets), with and without raw logits
# ------------------------------------------------------------------------------------------------------------------------------
ENGINE_CONFIGS = [('OnsetsFrames', 2, 1, 229, 'bf16'), ('OnsetsFrames', 2, 1, 229, 'x3'), ('OnsetsFrames', 2, 1, 229, 'f16'),
                  # model_complexity 3: 96 channels x 57 columns = 5472 fc1 inputs, padded to the GEMM's k-tile (kfc_pad != kfc)
                  ('OnsetsFrames2', 3, 1, 229, 'bf16'), ('OnsetsFrames2', 3, 1, 229, 'f16'), ('OnsetsFrames', 2, 6, 72, 'bf16'), ('OnsetsFrames', 2, 6, 72, 'f16'),
                  ('OnsetsFrames', 2, 1, 54, 'bf16'), ('OnsetsFrames', 2, 1, 8, 'x3'),
                  ('OnsetsFrames', 4, 1, 229, 'bf16'), ('OnsetsFrames', 5, 1, 229, 'bf16'), ('OnsetsFrames2', 3, 1, 229, 'x3'),
                  ('OnsetsFrames', 4, 3, 72, 'x3')]


def _of_model(cls, mc, ch, dim_in, precision, sd):
    import amt_tools_amd.models as M
    model = getattr(M, cls)(dim_in, tools.PianoProfile(), ch, mc, device=DEV, precision=precision)
    model.load_state_dict(_tensors(sd))
    model.change_device()
    model.eval()
    return model


def _engine_ws(model):
    eng = model.__dict__.get('_engine')
    return None if eng is None else eng.workspace


def _of_run(model, feats, pattern=None):
    """Both public entries: engine_logits (want_logits on: rolls + the raw logits of every bank) and the label-free run_on_batch
    (want_logits off: rolls only).  With `pattern`, the engine's workspace is refilled in place before each of the two calls."""
    out = {}
    with torch.no_grad():
        if pattern is not None:
            refill(_engine_ws(model), pattern)
        out['engine_logits'] = snapshot(model.engine_logits(feats))
        if pattern is not None:
            refill(_engine_ws(model), pattern)
        out['run_on_batch'] = snapshot(model.run_on_batch({tools.KEY_FEATS: feats}))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('cls,mc,ch,dim_in,precision', ENGINE_CONFIGS)
def test_engine_results_do_not_depend_on_workspace_or_output_contents(poison, cls, mc, ch, dim_in, precision):
    sd = synth_state_dict(7, dim_in=dim_in, in_channels=ch, model_complexity=mc, offsets=cls == 'OnsetsFrames2')
    rng = np.random.default_rng(dim_in)
    feats = {bt: torch.from_numpy(rng.random((bt[0], ch, dim_in, bt[1])).astype(np.float32)).cuda() for bt in SEQUENCE}
    # the reference of every shape: a fresh engine whose workspace is exactly as large as the call needs, everything 0x00
    poison.pattern = 0x00
    ref = {bt: _of_run(_of_model(cls, mc, ch, dim_in, precision, sd), feats[bt]) for bt in SEQUENCE}
    for bt in SEQUENCE:
        assert set(ref[bt]['engine_logits']) >= {'onsets', 'multi_pitch', 'pitch_head', 'onsets_bin', 'multi_pitch_bin'}
        assert ref[bt]['engine_logits']['onsets'].shape == (bt[0], bt[1], 88)
    # (1) one engine, nothing refilled: the small calls meet the (44, 140) call's real activations beyond their rows and in their pads
    model = _of_model(cls, mc, ch, dim_in, precision, sd)
    for bt in SEQUENCE:
        assert_same(_of_run(model, feats[bt]), ref[bt], f'{cls} mc{mc} {precision} {bt} after {SEQUENCE[0]} on one engine')
    assert _engine_ws(model).numel() > _lib.lib().amtx_of_workspace_bytes(model._get_engine(torch.device(DEV)).handle, 17, 9)
    # (2) poison: outputs and the workspace filled at allocation, the (then oversized) workspace refilled before every later call
    for pattern in PATTERNS[1:]:
        poison.pattern = pattern
        model = _of_model(cls, mc, ch, dim_in, precision, sd)
        before = poison.filled
        for i, bt in enumerate(SEQUENCE):
            assert_same(_of_run(model, feats[bt], None if i == 0 else pattern), ref[bt], f'{cls} mc{mc} {precision} {bt} fill {pattern:#04x}')
        assert poison.filled > before


# ------------------------------------------------------------------------------------------------------------------------------
# power path (MelSpec fused into the first conv: amtx_of_forward_power) and feats16 path (amtx_cqt_forward16[_split] -> _feats16)
# ------------------------------------------------------------------------------------------------------------------------------
def _frontend_ws(model):
    mod = model.frontend[0].module
    return mod.__dict__.get('_workspace')


def _audio_run(model, audio, pattern=None, labelled=False):
    with torch.no_grad():
        if pattern is not None:
            refill(_engine_ws(model), pattern)
            refill(_frontend_ws(model), pattern)
        batch = {tools.KEY_AUDIO: audio}
        if labelled:                             # ground truth present: the engine also copies its raw logits out (the loss reads them)
            T = int(model.run_on_batch({tools.KEY_AUDIO: audio})[tools.KEY_MULTIPITCH].shape[-1])
            lab = torch.zeros(audio.shape[0], 88, T)
            lab[:, ::5, ::3] = 1.0
            batch.update({tools.KEY_MULTIPITCH: lab, tools.KEY_ONSETS: lab.clone()})
            if pattern is not None:
                refill(_engine_ws(model), pattern)
                refill(_frontend_ws(model), pattern)
        out = snapshot(model.run_on_batch(batch))
    torch.cuda.synchronize()
    return out


def _audio_case(poison, make_model, shapes, what, engine_check):
    audio = {bn: torch.from_numpy(np.stack([synth_clip(i, num_samples=bn[1]) for i in range(bn[0])])).cuda() for bn in shapes}
    poison.pattern = 0x00
    ref = {}
    for bn in shapes:
        model = make_model()
        ref[bn] = (_audio_run(model, audio[bn]), _audio_run(make_model(), audio[bn], labelled=True))
        engine_check(model)
    model = make_model()
    for bn in shapes:
        assert_same(_audio_run(model, audio[bn]), ref[bn][0], f'{what} {bn} after {shapes[0]} on one engine')
    for pattern in PATTERNS[1:]:
        poison.pattern = pattern
        model, labelled = make_model(), make_model()
        for i, bn in enumerate(shapes):
            assert_same(_audio_run(model, audio[bn], None if i == 0 else pattern), ref[bn][0], f'{what} {bn} fill {pattern:#04x}')
            assert_same(_audio_run(labelled, audio[bn], None if i == 0 else pattern, labelled=True), ref[bn][1], f'{what} {bn} labelled, fill {pattern:#04x}')


@pytest.mark.parametrize('precision', ['bf16', 'x3'])
def test_power_path_results_do_not_depend_on_memory_contents(poison, precision):
    from amt_tools_amd.features import MelSpec
    sd = synth_state_dict(3, dim_in=229, in_channels=1, model_complexity=2)

    def make():
        model = _of_model('OnsetsFrames', 2, 1, 229, precision, sd)
        model.frontend = torch.nn.Sequential(MelSpec(sample_rate=22050, hop_length=512, n_mels=229, n_fft=2048).frontend())
        model.change_device()
        return model

    def check(model):
        assert model._get_engine(torch.device(DEV)).fuses_db_scale()          # the path under test is amtx_of_forward_power

    _audio_case(poison, make, ((9, 512 * 60), (3, 512 * 20), (2, 5000), (1, 700)), f'power path {precision}', check)


@pytest.mark.parametrize('precision,form', [('bf16', 1), ('x3', 2)])
def test_feats16_path_results_do_not_depend_on_memory_contents(poison, precision, form):
    from amt_tools_amd.features import HCQT
    sd = synth_state_dict(5, dim_in=72, in_channels=6, model_complexity=2)

    def make():
        model = _of_model('OnsetsFrames', 2, 6, 72, precision, sd)
        mod = HCQT(sample_rate=22050, hop_length=512, fmin=32.7, harmonics=[0.5, 1, 2, 3, 4, 5], n_bins=72, bins_per_octave=12)
        model.frontend = torch.nn.Sequential(mod.frontend())
        model.change_device()
        return model

    def check(model):
        assert model._get_engine(torch.device(DEV)).takes_feats16() == form   # amtx_cqt_forward16 (1) / _split (2) -> amtx_of_forward_feats16
        assert _frontend_ws(model) is not None

    _audio_case(poison, make, ((4, 40000), (1, 22050), (2, 512 * 33 + 7)), f'feats16 path {precision}', check)


# ------------------------------------------------------------------------------------------------------------------------------
# the front-ends on their own
# ------------------------------------------------------------------------------------------------------------------------------
def _spec_modules():
    from amt_tools_amd.features import MelSpec, STFT
    return {'melspec_ring': lambda: MelSpec(sample_rate=22050, hop_length=512, n_mels=229, n_fft=2048),        # spec_power_ring_kernel
            'melspec_general': lambda: MelSpec(sample_rate=22050, hop_length=256, n_mels=229, n_fft=2048),     # the general n_fft 2048 kernel
            'melspec_pow2': lambda: MelSpec(sample_rate=16000, hop_length=256, n_mels=80, n_fft=1024),         # spec_power_pow2_kernel
            'melspec_09': lambda: MelSpec(sample_rate=22050, hop_length=512, n_mels=229, n_fft=2048, librosa_version='0.9'),
            'stft': lambda: STFT(sample_rate=22050, hop_length=512, n_fft=2048),
            'stft_linear': lambda: STFT(sample_rate=16000, hop_length=512, n_fft=2048, decibels=False)}


@pytest.mark.parametrize('name', sorted(_spec_modules()))
def test_spectrogram_frontends_do_not_depend_on_memory_contents(poison, name):
    """process_batch = amtx_spec_power (clip_max cleared, then an atomic max) + amtx_spec_scale; power_batch returns the maxima themselves."""
    shapes = ((5, 512 * 40 + 13), (1, 512 * 40 + 13), (3, 5000), (1, 1500), (2, 512 * 9))
    audio = {bn: torch.from_numpy(np.stack([synth_clip(i, num_samples=bn[1]) for i in range(bn[0])])).cuda() for bn in shapes}
    results = {}
    for pattern in PATTERNS:
        poison.pattern = pattern
        mod = _spec_modules()[name]()
        for bn in shapes:
            power, clip_max = mod.power_batch(audio[bn])
            got = snapshot({'feats': mod.process_batch(audio[bn]), 'model_layout': mod.process_batch(audio[bn], model_layout=True),
                            'power': power, 'clip_max': clip_max})
            assert got['clip_max'].shape == (bn[0],) and (got['clip_max'] > 0).all()
            if pattern == PATTERNS[0]:
                results[bn] = got
            else:
                assert_same(got, results[bn], f'{name} {bn} fill {pattern:#04x}')
    assert poison.filled > 0


def _cqt_modules():
    from amt_tools_amd.features import CQT, HCQT, VQT
    return {'cqt_one_level': lambda: CQT(sample_rate=22050, hop_length=512, fmin=4000.0, n_bins=12, bins_per_octave=12),      # one octave, no early downsampling: nl == 1
            'cqt_one_level_09': lambda: CQT(sample_rate=22050, hop_length=512, fmin=4000.0, n_bins=12, bins_per_octave=12, librosa_version='0.9'),
            'cqt_config1': lambda: CQT(sample_rate=22050, hop_length=512, n_bins=192, bins_per_octave=24),                    # 8 levels
            'cqt_config1_09': lambda: CQT(sample_rate=22050, hop_length=512, n_bins=192, bins_per_octave=24, librosa_version='0.9'),
            'hcqt_config3': lambda: HCQT(sample_rate=22050, hop_length=512, fmin=32.7, harmonics=[0.5, 1, 2, 3, 4, 5], n_bins=72, bins_per_octave=12),
            'hcqt_linear': lambda: HCQT(sample_rate=22050, hop_length=512, n_bins=72, bins_per_octave=12, decibels=False),
            'vqt': lambda: VQT(sample_rate=22050, hop_length=256, n_bins=60, bins_per_octave=12, gamma=5.0)}


@pytest.mark.parametrize('name', sorted(_cqt_modules()))
def test_cqt_frontends_do_not_depend_on_memory_contents(poison, name):
    """amtx_cqt_forward with one pyramid level and with several (both sides of `direct0 && nl == 1`, where `maxbuf` is cleared), both centre
    paddings; a shape sequence on one module, whose grow-only workspace keeps the large call's pyramid."""
    shapes = ((3, 60000), (1, 44100), (2, 512 * 65 + 7), (1, 50000))
    audio = {bn: torch.from_numpy(np.stack([synth_clip(i, num_samples=bn[1]) for i in range(bn[0])])).cuda() for bn in shapes}
    poison.pattern = 0x00
    ref = {bn: snapshot(_cqt_modules()[name]().process_batch(audio[bn])) for bn in shapes}       # fresh module: workspace == need
    mod = _cqt_modules()[name]()
    for bn in shapes:
        assert_same(snapshot(mod.process_batch(audio[bn])), ref[bn], f'{name} {bn} after {shapes[0]} on one module')
    for pattern in PATTERNS[1:]:
        poison.pattern = pattern
        mod = _cqt_modules()[name]()
        for bn in shapes:
            refill(mod.__dict__.get('_workspace'), pattern)
            assert_same(snapshot(mod.process_batch(audio[bn])), ref[bn], f'{name} {bn} fill {pattern:#04x}')
        ws = mod.__dict__['_workspace']
        assert ws.numel() >= _lib.lib().amtx_cqt_workspace_bytes(mod._get_plan(torch.device(DEV)), *shapes[0])


def test_rms_norm_does_not_depend_on_memory_contents(poison):
    rng = np.random.default_rng(2)
    clips = {}
    for B, N in ((1, 1), (1, 4097), (3, 22050), (5, 999), (2, 70001)):
        x = (rng.standard_normal((B, N)) * rng.uniform(0.01, 3.0, (B, 1))).astype(np.float32)
        if B > 2:
            x[1] = 0.0                                       # a silent clip: rms 0, returned as it is
        clips[(B, N)] = torch.from_numpy(x).cuda()
    ref = {}
    for pattern in PATTERNS:
        poison.pattern = pattern
        for key, x in clips.items():
            got = snapshot(tools.rms_norm_batch(x))
            if pattern == PATTERNS[0]:
                ref[key] = got
            else:
                assert_same(got, ref[key], f'rms_norm {key} fill {pattern:#04x}')


# ------------------------------------------------------------------------------------------------------------------------------
# TabCNN inference: whole and chunked
# ------------------------------------------------------------------------------------------------------------------------------
def _tab_model(dim_in, in_channels, precision='x3'):
    from amt_tools_amd.models import TabCNN
    m = TabCNN(dim_in, tools.GuitarProfile(num_frets=19), in_channels, 1, device=DEV, precision=precision)
    m.load_state_dict(_tensors(synth_tabcnn_state_dict(6, dim_in=dim_in, in_channels=in_channels, num_groups=6, num_classes=21)))
    m.change_device()
    m.eval()
    return m


def _tab_run(model, feats, pattern=None):
    with torch.no_grad():
        if pattern is not None:
            refill(_engine_ws(model), pattern)
        pre = model.pre_proc({tools.KEY_FEATS: feats})
        out = {tools.KEY_OUTPUT: model(pre[tools.KEY_FEATS])}
        logits = out[tools.KEY_OUTPUT][tools.KEY_TABLATURE]
        res = {'logits': snapshot(logits), 'tablature': snapshot(model.post_proc(out)[tools.KEY_TABLATURE])}
        if pattern is not None:
            refill(_engine_ws(model), pattern)
        res['run_on_batch'] = snapshot(model.run_on_batch({tools.KEY_FEATS: feats}))
    torch.cuda.synchronize()
    assert model.__dict__['_engine'].forwards > 0            # the HIP engine ran, not the stock path
    return res


@pytest.mark.parametrize('chunked', [False, True], ids=['whole', 'chunked'])
@pytest.mark.parametrize('in_channels,dim_in,precision', [(1, 80, 'x3'), (6, 45, 'x3'), (1, 192, 'bf16')])
def test_tabcnn_engine_does_not_depend_on_memory_contents(poison, monkeypatch, in_channels, dim_in, precision, chunked):
    from amt_tools_amd.models import _TabEngine
    shapes = ((5, 65), (2, 9), (3, 1), (1, 65), (1, 1))
    g = torch.Generator().manual_seed(dim_in)
    feats = {bt: torch.rand((bt[0], in_channels, dim_in, bt[1]), generator=g).to(DEV) for bt in shapes}
    if chunked:
        probe = _tab_model(dim_in, in_channels, precision)
        _tab_run(probe, feats[(1, 1)])
        eng = probe.__dict__['_engine']
        monkeypatch.setattr(_TabEngine, 'WORKSPACE_CAP', eng.workspace_bytes(2, 20))
        assert len(eng._chunks(5, 65)) > 4
    poison.pattern = 0x00
    ref = {bt: _tab_run(_tab_model(dim_in, in_channels, precision), feats[bt]) for bt in shapes}
    model = _tab_model(dim_in, in_channels, precision)
    for bt in shapes:
        assert_same(_tab_run(model, feats[bt]), ref[bt], f'TabCNN {in_channels}ch {bt} after {shapes[0]} on one engine')
    for pattern in PATTERNS[1:]:
        poison.pattern = pattern
        model = _tab_model(dim_in, in_channels, precision)
        for i, bt in enumerate(shapes):
            assert_same(_tab_run(model, feats[bt], None if i == 0 else pattern), ref[bt], f'TabCNN {in_channels}ch {bt} fill {pattern:#04x}')


# ------------------------------------------------------------------------------------------------------------------------------
# note decoding on the device
# ------------------------------------------------------------------------------------------------------------------------------
def test_device_note_decoder_does_not_depend_on_memory_contents(poison):
    """amtx_notes_decode + amtx_notes_rows through transcribe.py: one shared grid and per-clip grids, more than the scan kernel's 1024-clip
    chunk, clips without a note, and a first row buffer that is too small (the retry path).  The note lists must be equal."""
    from amt_tools_amd.transcribe import decode_notes_batch, decode_notes_batch_async, multi_pitch_to_notes
    rng = np.random.default_rng(1)
    B, T = 6, 625
    mp = (rng.random((B, 88, T)) < 0.2).astype(np.float32)
    on = (rng.random((B, 88, T)) < 0.05).astype(np.float32)
    mp[0] = 1.0
    on[1] = 0.0
    on[2, :, ::2] = 1.0
    on[2, :, 1::2] = 0.0
    times = np.arange(T) * 512 / 22050.0
    B2, T2 = 1100, 64
    mp2 = (rng.random((B2, 88, T2)) < 0.08).astype(np.float32)
    on2 = (rng.random((B2, 88, T2)) < 0.02).astype(np.float32)
    mp2[::7] = 0.0
    on2[::7] = 0.0
    hops = rng.integers(128, 1024, B2)
    times2 = (np.arange(T2)[None, :] * hops[:, None] / 22050.0).astype(np.float32)
    mpd, ond, mpd2, ond2 = (torch.from_numpy(a).cuda() for a in (mp, on, mp2, on2))
    ref = None
    for pattern in PATTERNS:
        poison.pattern = pattern
        got = {'shared_grid': decode_notes_batch(ond, mpd, times), 'no_onsets': decode_notes_batch(None, mpd, times),
               'three_frames': decode_notes_batch(ond[:2, :, :3].contiguous(), mpd[:2, :, :3].contiguous(), times[:3]),
               'per_clip_grids': decode_notes_batch(ond2, mpd2, times2),
               'capacity_retry': decode_notes_batch_async(ond2, mpd2, times2, rows_capacity=100).result()}
        got = snapshot(got)
        if ref is None:
            ref = got
            for b in range(B):                               # the 0x00 run is itself the host decoder's result
                assert np.array_equal(got['shared_grid'][b], multi_pitch_to_notes(mp[b], times, 21, on[b]))
            assert sum(len(n) for n in got['per_clip_grids']) > 100 * 3 and len(got['per_clip_grids']) == B2
        else:
            assert_same(got, ref, f'note decoder fill {pattern:#04x}')
    assert_same(ref['capacity_retry'], ref['per_clip_grids'], 'capacity retry')


# ------------------------------------------------------------------------------------------------------------------------------
# training: one forward + backward, autograd's scratch poisoned before the forward and again between forward and backward
# ------------------------------------------------------------------------------------------------------------------------------
def _refill_training_scratch(pattern):
    for ws in autograd._WS.values():
        refill(ws, pattern)


def _of_training_step(cls, mc, pattern):
    import amt_tools_amd.models as M
    torch.manual_seed(0)
    model = getattr(M, cls)(229, tools.PianoProfile(), 1, mc, device=DEV)
    model.change_device()
    model.train()
    B, T = 2, 50
    g = torch.Generator().manual_seed(3)
    feats = torch.rand(B, 1, 229, T, generator=g).cuda()
    lab = (torch.rand(B, 88, T, generator=g) < 0.05).float().cuda()
    batch = {tools.KEY_FEATS: feats, tools.KEY_MULTIPITCH: lab, tools.KEY_ONSETS: lab.clone()}
    if cls == 'OnsetsFrames2':
        batch[tools.KEY_OFFSETS] = lab.clone()
    return _step(model, batch, pattern)


def _tab_training_step(dim_in, cin, weighted, pattern):
    from amt_tools_amd.models import TabCNN
    model = TabCNN(dim_in, tools.GuitarProfile(num_frets=19), cin, 1, device=DEV)
    model.load_state_dict(_tensors(synth_tabcnn_state_dict(0, dim_in=dim_in, in_channels=cin, model_complexity=1, num_groups=6, num_classes=21)))
    if weighted:
        model.dense[-1].set_weights(np.random.default_rng(0).uniform(0.25, 2.0, 6 * 21), device=DEV)
    model.change_device()
    model.train()                                            # Dropout on: the seed below fixes its masks
    g = torch.Generator().manual_seed(dim_in)
    B, T = 3, 37 if cin == 1 else 9
    batch = {tools.KEY_FEATS: torch.rand((B, cin, dim_in, T), generator=g), tools.KEY_TABLATURE: torch.randint(-1, 21, (B, 6, T), generator=g)}
    return _step(model, batch, pattern)


def _step(model, batch, pattern):
    fb0 = autograd.fallback_total()
    _refill_training_scratch(pattern)
    torch.manual_seed(1234)
    out = model.run_on_batch(batch)
    loss = out[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL]
    torch.cuda.synchronize()
    _refill_training_scratch(pattern)                        # the backward kernels' partials reuse the scratch the forward used
    loss.backward()
    torch.cuda.synchronize()
    assert autograd.fallback_total() == fb0, autograd.fallbacks()          # the HIP path is what ran
    assert autograd._WS, 'the HIP autograd path did not run'
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert all(v is not None for v in grads.values())
    res = {'loss': {k: v for k, v in out[tools.KEY_LOSS].items()}, 'grads': grads,
           'outputs': {k: v for k, v in out.items() if k != tools.KEY_LOSS and torch.is_tensor(v)},
           'buffers': dict(model.named_buffers())}
    return snapshot(res)


TRAIN_CASES = {'OnsetsFrames_mc2': lambda p: _of_training_step('OnsetsFrames', 2, p), 'OnsetsFrames2_mc3': lambda p: _of_training_step('OnsetsFrames2', 3, p),
               'TabCNN_1ch': lambda p: _tab_training_step(192, 1, False, p), 'TabCNN_6ch_weighted': lambda p: _tab_training_step(45, 6, True, p)}


@pytest.mark.parametrize('name', sorted(TRAIN_CASES))
def test_training_step_does_not_depend_on_memory_contents(poison, name):
    ref = None
    try:
        for pattern in PATTERNS:
            for reuse in (False, True):                      # scratch allocated under the fill, then the same (oversized) scratch refilled
                if not reuse:
                    autograd._WS.clear()
                poison.pattern = pattern
                got = TRAIN_CASES[name](pattern)
                if ref is None:
                    ref = got
                else:
                    assert_same(got, ref, f'{name} fill {pattern:#04x}{", scratch reused" if reuse else ""}')
    finally:
        autograd._WS.clear()


# ------------------------------------------------------------------------------------------------------------------------------
# kernel level: the C ABI called directly, the caller's workspace and outputs poisoned, each against its own 0x00 run
# ------------------------------------------------------------------------------------------------------------------------------
def _stream():
    return _lib.current_stream()


def _ws(nbytes, pattern, extra=4096):
    """A workspace LARGER than asked for (the grow-only buffers of the product are), filled with the pattern."""
    return refill(_lib.alloc_workspace(int(nbytes) + extra, DEV), pattern)


def _out(shape, pattern, dtype=torch.float32, **kw):
    return fill_storage(torch.empty(shape, dtype=dtype, device=DEV, **kw), pattern)


def _across_patterns(run, what):
    ref = None
    for pattern in PATTERNS:
        got = snapshot(run(pattern))
        torch.cuda.synchronize()
        if ref is None:
            ref = got
        else:
            assert_same(got, ref, f'{what} fill {pattern:#04x}')
    return ref


# K = 4, 8: most slices of a split contraction are empty; (4999, 132, 36), (130, 1024, 176): off every tile size; (8, 12, 20000): a long
# contraction into a small C (the split-contraction case proper); (1, 4, 4): one element per thread at the most
@pytest.mark.parametrize('a_trans', [False, True])
@pytest.mark.parametrize('b_trans', [False, True])
@pytest.mark.parametrize('M,N,K', [(1, 4, 4), (37, 88, 256), (4999, 132, 36), (130, 1024, 176), (8, 12, 20000), (300, 36, 8), (132, 4, 3648), (260, 516, 4)])
def test_matmul_f32_does_not_depend_on_workspace_or_output_contents(M, N, K, a_trans, b_trans):
    L = _lib.lib()
    if a_trans:
        M += (-M) % 4                                        # the contiguous extent of a transposed operand is a multiple of 4
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn((K, M) if a_trans else (M, K), generator=g).cuda()
    b = torch.randn((K, N) if b_trans else (N, K), generator=g).cuda()
    bias = torch.randn(N, generator=g).cuda()
    need = int(L.amtx_matmul_workspace_bytes(M, N, K))

    def run(pattern):
        res = {}
        for with_bias in (False, True):
            c = _out((M, N), pattern)
            ws = _ws(need, pattern)
            _lib.check(L.amtx_matmul_f32(_lib.ptr(a), a.stride(0), int(a_trans), _lib.ptr(b), b.stride(0), int(b_trans), _lib.ptr(bias) if with_bias else None,
                                         _lib.ptr(c), N, M, N, K, _lib.ptr(ws), ws.numel(), _stream()), 'amtx_matmul_f32')
            res[with_bias] = c
        cpad = _out((M, N + 4), pattern)                     # ldc != n: no workspace is used, and the pad columns of C are not the kernel's
        _lib.check(L.amtx_matmul_f32(_lib.ptr(a), a.stride(0), int(a_trans), _lib.ptr(b), b.stride(0), int(b_trans), None, _lib.ptr(cpad), N + 4, M, N, K,
                                     None, 0, _stream()), 'amtx_matmul_f32 (padded C)')
        res['padded'] = cpad[:, :N]
        return res

    ref = _across_patterns(run, f'amtx_matmul_f32 {M}x{N}x{K} a_trans={a_trans} b_trans={b_trans}')
    want = (a.double().T if a_trans else a.double()) @ (b.double() if b_trans else b.double().T)
    # (a sanity check that the 0x00 run is the product at all; its accuracy is tests/test_gpu_train.py's subject)
    assert np.abs(ref[False] - want.cpu().numpy()).max() <= 1e-3 * max(1.0, float(want.abs().max()))
    assert np.abs(ref['padded'] - want.cpu().numpy()).max() <= 1e-3 * max(1.0, float(want.abs().max()))       # (no split contraction: other bits)


@pytest.mark.parametrize('M,N,K', [(1, 4, 4), (37, 88, 256), (625, 512, 3648), (5000, 88, 512), (130, 1024, 176), (4999, 132, 36)])
def test_linear_bwd_does_not_depend_on_workspace_or_output_contents(M, N, K):
    L = _lib.lib()
    g = torch.Generator().manual_seed(M + N + K)
    dy, x, w = torch.randn(M, N, generator=g).cuda(), torch.randn(M, K, generator=g).cuda(), torch.randn(N, K, generator=g).cuda()
    need = int(L.amtx_linear_bwd_workspace_bytes(M, N, K))

    def run(pattern):
        dx, dw, db = _out((M, K), pattern), _out((N, K), pattern), _out((N,), pattern)
        ws = _ws(need, pattern)
        _lib.check(L.amtx_linear_bwd(_lib.ptr(dy), N, _lib.ptr(x), K, _lib.ptr(w), K, _lib.ptr(dx), K, _lib.ptr(dw), _lib.ptr(db), M, N, K,
                                     _lib.ptr(ws), ws.numel(), _stream()), 'amtx_linear_bwd')
        db_only = _out((N,), pattern)                        # the column-sum use (autograd._colsum)
        ws2 = _ws(int(L.amtx_linear_bwd_workspace_bytes(M, N, 4)), pattern)
        _lib.check(L.amtx_linear_bwd(_lib.ptr(dy), N, None, 0, None, 0, None, 0, None, _lib.ptr(db_only), M, N, 4, _lib.ptr(ws2), ws2.numel(), _stream()),
                   'amtx_linear_bwd (db only)')
        return {'dx': dx, 'dw': dw, 'db': db, 'db_only': db_only}

    ref = _across_patterns(run, f'amtx_linear_bwd {M}x{N}x{K}')
    want = dy.double().T @ x.double()
    assert np.abs(ref['dw'] - want.cpu().numpy()).max() <= 1e-3 * max(1.0, float(want.abs().max()))          # sanity only, as above


@pytest.mark.parametrize('ci,co', [(1, 32), (32, 32), (32, 64), (48, 96), (16, 16), (8, 32)])
@pytest.mark.parametrize('B,T,F', [(1, 1, 2), (2, 7, 13), (3, 20, 57), (1, 33, 229)])
def test_conv3x3_train_does_not_depend_on_workspace_or_output_contents(ci, co, B, T, F):
    L = _lib.lib()
    g = torch.Generator().manual_seed(ci * 1000 + co + B + T + F)
    x = torch.randn(B, T, F, ci, generator=g).cuda()         # channels-last maps as the kernels index them: (rows, bins, channels)
    dy = torch.randn(B, T, F, co, generator=g).cuda()
    w = (torch.randn(co, ci, 3, 3, generator=g) / 3.0).cuda()
    bias = torch.randn(co, generator=g).cuda()
    need = int(L.amtx_conv3x3_train_workspace_bytes(B * T, F, ci, co))

    def run(pattern):
        y = _out((B, T, F, co), pattern)
        ws = _ws(need, pattern)
        _lib.check(L.amtx_conv3x3_train_fwd(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(y), B * T, T, F, ci, co, _lib.ptr(ws), ws.numel(), _stream()),
                   'amtx_conv3x3_train_fwd')
        dx = _out((B, T, F, ci), pattern) if ci % 4 == 0 else None
        dw, db = _out((co, ci, 3, 3), pattern), _out((co,), pattern)
        refill(ws, pattern)
        _lib.check(L.amtx_conv3x3_bwd(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(w), _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db), B * T, T, F, ci, co,
                                      _lib.ptr(ws), ws.numel(), _stream()), 'amtx_conv3x3_bwd')
        return {'y': y, 'dx': dx, 'dw': dw, 'db': db}

    ref = _across_patterns(run, f'amtx_conv3x3 train {ci}->{co} {(B, T, F)}')
    want = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), bias.double(), padding=1).permute(0, 2, 3, 1)
    assert np.abs(ref['y'] - want.cpu().numpy()).max() <= 1e-3 * max(1.0, float(want.abs().max()))           # sanity only, as above


@pytest.mark.parametrize('B,C_,T,F,pool', [(2, 32, 9, 229, False), (2, 32, 9, 229, True), (3, 64, 5, 114, True), (1, 48, 7, 18, True), (1, 96, 3, 2, True),
                                           (2, 4, 3, 5, False), (1, 48, 3, 57, True)])
def test_bn_relu_pool_train_does_not_depend_on_workspace_or_output_contents(B, C_, T, F, pool):
    L = _lib.lib()
    g = torch.Generator().manual_seed(B * 100 + C_ + T + F)
    x = (torch.randn(B, T, F, C_, generator=g) * 1.5 + 0.3).cuda()
    gamma, beta = (torch.rand(C_, generator=g) + 0.5).cuda(), (torch.randn(C_, generator=g) * 0.2).cuda()
    Fo = F // 2 if pool else F
    dy = torch.randn(B, T, Fo, C_, generator=g).cuda()
    need = int(L.amtx_bn_train_workspace_bytes(C_))

    def run(pattern):
        rm, rv = torch.zeros(C_, device=DEV), torch.ones(C_, device=DEV)
        y, stats = _out((B, T, Fo, C_), pattern), _out((4, C_), pattern)
        ws = _ws(need, pattern)
        _lib.check(L.amtx_bn_relu_pool_train_fwd(_lib.ptr(x), B * T, F, C_, int(pool), _lib.ptr(gamma), _lib.ptr(beta), 1e-5, 0.1, _lib.ptr(rm), _lib.ptr(rv),
                                                 _lib.ptr(y), _lib.ptr(stats), _lib.ptr(ws), ws.numel(), _stream()), 'amtx_bn_relu_pool_train_fwd')
        dx, dgamma, dbeta = _out((B, T, F, C_), pattern), _out((C_,), pattern), _out((C_,), pattern)
        refill(ws, pattern)
        _lib.check(L.amtx_bn_relu_pool_train_bwd(_lib.ptr(x), B * T, F, C_, int(pool), _lib.ptr(stats), _lib.ptr(dy), _lib.ptr(dx), _lib.ptr(dgamma),
                                                 _lib.ptr(dbeta), _lib.ptr(ws), ws.numel(), _stream()), 'amtx_bn_relu_pool_train_bwd')
        return {'y': y, 'stats': stats, 'running_mean': rm, 'running_var': rv, 'dx': dx, 'dgamma': dgamma, 'dbeta': dbeta}

    ref = _across_patterns(run, f'amtx_bn_relu_pool_train {(B, C_, T, F, pool)}')
    assert ref['y'].min() >= 0 and ref['y'].max() > 0


@pytest.mark.parametrize('B,T,K,weighted', [(8, 625, 88, False), (3, 70, 88, True), (1, 1, 4, False), (2, 33, 120, True)])
def test_bce_logits_loss_does_not_depend_on_workspace_or_output_contents(B, T, K, weighted):
    L = _lib.lib()
    g = torch.Generator().manual_seed(B * 1000 + T)
    x = (torch.randn(B, T, K, generator=g) * 4).cuda()
    y = (torch.rand(B, K, T, generator=g) < 0.1).float().cuda()
    w = (torch.rand(K, generator=g) + 0.5).cuda() if weighted else None
    need = int(L.amtx_bce_logits_loss_workspace_bytes(B, T, K))

    def run(pattern):
        loss, grad, loss_only = _out((), pattern), _out((B, T, K), pattern), _out((), pattern)
        ws = _ws(need, pattern)
        _lib.check(L.amtx_bce_logits_loss(_lib.ptr(x), K, _lib.ptr(y), _lib.ptr(w), B, T, K, _lib.ptr(loss), _lib.ptr(grad), _lib.ptr(ws), ws.numel(), _stream()),
                   'amtx_bce_logits_loss')
        refill(ws, pattern)
        _lib.check(L.amtx_bce_logits_loss(_lib.ptr(x), K, _lib.ptr(y), _lib.ptr(w), B, T, K, _lib.ptr(loss_only), None, _lib.ptr(ws), ws.numel(), _stream()),
                   'amtx_bce_logits_loss (no gradient)')
        return {'loss': loss, 'grad': grad, 'loss_only': loss_only}

    ref = _across_patterns(run, f'amtx_bce_logits_loss {(B, T, K, weighted)}')
    assert ref['loss'] == ref['loss_only'] and ref['loss'] > 0


@pytest.mark.parametrize('B,T,G,Cn,ld,weighted', [(3, 57, 6, 21, 128, False), (3, 57, 6, 21, 128, True), (1, 1, 6, 21, 128, False), (2, 200, 4, 32, 128, True)])
def test_softmax_groups_loss_does_not_depend_on_workspace_or_output_contents(B, T, G, Cn, ld, weighted):
    L = _lib.lib()
    g = torch.Generator().manual_seed(B + T + G + Cn)
    x = (4 * torch.randn(B * T, ld, generator=g)).cuda()     # rows `ld` apart: the strided row view the model hands over
    y = torch.randint(-1, Cn, (B, G, T), generator=g).cuda()
    w = (torch.rand(G * Cn, generator=g) + 0.25).cuda() if weighted else None
    need = int(L.amtx_softmax_groups_loss_workspace_bytes(B, T, G, Cn))

    def run(pattern):
        loss, grad = _out((), pattern), _out((B, T, G * Cn), pattern)
        ws = _ws(need, pattern)
        _lib.check(L.amtx_softmax_groups_loss(_lib.ptr(x), ld, _lib.ptr(y), _lib.ptr(w), B, T, G, Cn, _lib.ptr(loss), _lib.ptr(grad), _lib.ptr(ws), ws.numel(),
                                              _stream()), 'amtx_softmax_groups_loss')
        return {'loss': loss, 'grad': grad}

    ref = _across_patterns(run, f'amtx_softmax_groups_loss {(B, T, G, Cn, ld, weighted)}')
    assert ref['loss'] > 0
