"""GPU parity: HIP spectral front-end (through the C ABI) vs the fp64 oracle restatement.

Tolerance: the scaled features live in [0, 1]; the fp32 on-device FFT differs from the fp64 oracle by
rounding noise that is largest (in dB) in bins near the -80 dB floor.  Bound: 2e-5 absolute in the
scaled domain (SURVEY 8(c) asks for <= 1e-5 .. 1e-4; measured on MI355X: 9e-6 on the log-mel shape -- the bound is 2 x that, so a
regression of the FFT's accuracy shows), 2e-6 relative on linear power."""
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import frontend_np as fe          # noqa: E402
from amt_tools_amd.synth import synth_clip    # noqa: E402

TOL_SCALED = 2e-5
# the generic power-of-two kernel (in-place radix-2 passes, n_fft != 2048): STFT magnitudes in dB measure 2.4e-5 .. 3.0e-5 on MI355X
TOL_POW2 = 6e-5


def _mods():
    from amt_tools_amd.features import MelSpec, STFT
    return MelSpec, STFT


@pytest.mark.parametrize('lv', ['0.10', '0.9'])
@pytest.mark.parametrize('htk', [False, True])
def test_melspec_matches_oracle(lv, htk):
    MelSpec, _ = _mods()
    y = synth_clip(3, num_samples=60000)
    mod = MelSpec(sample_rate=22050, hop_length=512, n_mels=229, n_fft=2048, htk=htk, librosa_version=lv)
    got = mod.process_audio(y)
    ref = fe.melspec_process_audio(y, 22050, 512, 229, 2048, htk=htk, lv=lv)
    assert got.shape == ref.shape == (1, 229, 1 + 60000 // 512) and got.dtype == np.float32
    assert np.abs(got - ref).max() < TOL_SCALED
    assert got.max() == 1.0 and got.min() >= 0.0


@pytest.mark.parametrize('n_mels,sr', [(40, 16000), (64, 22050), (128, 44100), (300, 22050), (512, 22050)])
def test_melspec_other_filterbank_sizes(n_mels, sr):
    """Other row counts / sample rates: one to eight rounds of 64 rows, both homes of the tap table (LDS up to 80 tap slots,
    device memory beyond: 512 rows)."""
    MelSpec, _ = _mods()
    y = synth_clip(11, num_samples=50000)
    mod = MelSpec(sample_rate=sr, hop_length=512, n_mels=n_mels, n_fft=2048)
    got = mod.process_audio(y)
    ref = fe.melspec_process_audio(y, sr, 512, n_mels, 2048)
    assert got.shape == ref.shape == (1, n_mels, 1 + 50000 // 512)
    assert np.abs(got - ref).max() < TOL_SCALED


def test_melspec_linear_power_and_filterbank():
    MelSpec, _ = _mods()
    y = synth_clip(5, num_samples=40000)
    mod = MelSpec(sample_rate=16000, hop_length=512, decibels=False)
    got = mod.process_audio(y)
    ref = fe.melspec_process_audio(y, 16000, 512, 229, 2048, decibels=False)
    assert np.abs(got - ref).max() <= 2e-6 * ref.max() + 1e-12
    # identical up to triangle-corner taps that are ~1e-16 in one construction and exactly 0 in the other
    np.testing.assert_allclose(mod.filterbank(), fe.mel_filterbank(16000, 2048, 229), rtol=0, atol=1e-12)


@pytest.mark.parametrize('decibels', [True, False])
def test_stft_matches_oracle(decibels):
    _, STFT = _mods()
    y = synth_clip(7, num_samples=30000)
    mod = STFT(sample_rate=22050, hop_length=512, n_fft=2048, decibels=decibels)
    got = mod.process_audio(y)
    ref = fe.stft_process_audio(y, 512, 2048, decibels=decibels)
    assert got.shape == ref.shape == (1, 1025, 1 + 30000 // 512)
    if decibels:
        assert np.abs(got - ref).max() < TOL_SCALED
    else:
        assert np.abs(got - ref).max() <= 2e-6 * ref.max()


@pytest.mark.parametrize('n', [1, 2, 511, 512, 513, 1023, 1025, 2047, 2048, 2049, 5000])
def test_short_and_ragged_lengths(n):
    MelSpec, _ = _mods()
    rng = np.random.default_rng(n)
    y = rng.standard_normal(n).astype(np.float32)
    mod = MelSpec(sample_rate=22050)
    got = mod.process_audio(y)
    ref = fe.melspec_process_audio(y, 22050)
    assert got.shape == ref.shape == (1, 229, mod.get_expected_frames(y))
    assert np.abs(got - ref).max() < TOL_SCALED


def test_empty_audio_conventions():
    MelSpec, STFT = _mods()
    assert MelSpec().process_audio(np.zeros(0, dtype=np.float32)).shape == (1, 229, 0)
    assert STFT().process_audio(np.zeros(0, dtype=np.float32)).shape == (1, 2048, 0)   # reference quirk


def test_silence_maps_to_one():
    MelSpec, _ = _mods()
    got = MelSpec(sample_rate=22050).process_audio(np.zeros(4096, dtype=np.float32))
    ref = fe.melspec_process_audio(np.zeros(4096, dtype=np.float32), 22050)
    np.testing.assert_array_equal(got, ref.astype(np.float32))


def test_not_centered_matches_oracle():
    MelSpec, _ = _mods()
    y = synth_clip(9, num_samples=20000)
    mod = MelSpec(sample_rate=22050, center=False)
    got = mod.process_audio(y)
    ref = fe.melspec_process_audio(y, 22050, center=False)
    assert got.shape == ref.shape and got.shape[-1] == mod.get_expected_frames(y)
    assert np.abs(got - ref).max() < TOL_SCALED


def test_batch_clip_maxima_are_independent_and_ref_override():
    MelSpec, _ = _mods()
    clips = np.stack([synth_clip(i, num_samples=33333) * (10.0 ** (-i)) for i in range(3)])
    mod = MelSpec(sample_rate=22050)
    x = torch.from_numpy(clips).cuda()
    got = mod.process_batch(x).cpu().numpy()
    assert got.shape == (3, 1, 229, 1 + 33333 // 512)
    for i in range(3):
        ref = fe.melspec_process_audio(clips[i], 22050)
        assert np.abs(got[i] - ref).max() < TOL_SCALED
    # model layout is the transpose
    got_t = mod.process_batch(x, model_layout=True).cpu().numpy()
    np.testing.assert_array_equal(got_t, np.swapaxes(got, -1, -2))
    # track-level reference (finding F7): features of a slice normalised by a larger track maximum
    power, cmax = mod.power_batch(x)
    ref_pow = (cmax * 100.0).contiguous()
    shifted = mod.scale_batch(power, cmax, ref=ref_pow).cpu().numpy()
    S = fe.melspectrogram(clips[0], 22050)
    db = 10 * np.log10(np.maximum(1e-10, S)) - 10 * np.log10(S.max() * 100.0)
    db = np.maximum(db, db.max() - 80.0)
    assert np.abs(shifted[0, 0] - (db / 80 + 1)).max() < TOL_SCALED


def test_full_size_clip_properties():
    """BASELINE-size clip (319 999 samples -> 625 frames): exact quadratic scaling of the power map under a
    power-of-two gain (every fp32 operation scales exactly) and agreement of the map maximum with the
    reduction output."""
    MelSpec, _ = _mods()
    mod = MelSpec(sample_rate=22050, decibels=False)
    y = synth_clip(0)
    x = torch.from_numpy(np.stack([y, 4.0 * y])).cuda()
    power, cmax = mod.power_batch(x)
    assert power.shape == (2, 625, 229)
    assert torch.equal(power[1], 16.0 * power[0])
    assert torch.equal(cmax, power.amax(dim=(1, 2)))


def test_rms_norm_batch_matches_reference_fixture():
    """amtx_rms_norm against outputs of the REFERENCE's own `tools.rms_norm` (amt_tools/tools/utils.py:2789-2814), recorded by
    tools/gen_golden.py in tests/golden/rms_norm.npz (a seed per clip + every 97th output sample + the output's sum of squares):
    float32 clips of three scales, a 7-sample and a 1-sample clip and a silent clip (returned as is)."""
    from amt_tools_amd import tools
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'rms_norm.npz'))
    stride = int(g['stride'])
    for i, (n, sc) in enumerate(zip(g['lengths'], g['scales'])):
        x = (np.random.default_rng(700 + i).standard_normal(int(n)) * sc).astype(np.float32)
        got = tools.rms_norm_batch(torch.from_numpy(x[None]).cuda()).cpu().numpy()[0]
        ref = g[f'out_{i}_float32']
        assert got.dtype == np.float32 and str(g[f'dtype_{i}_float32']) == 'float32'
        assert np.abs(got[::stride] - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max()), i
        assert abs(float(np.sum(got.astype(np.float64) ** 2)) - float(g[f'sumsq_{i}_float32'])) <= 1e-5 * max(1.0, float(g[f'sumsq_{i}_float32'])), i
        if sc == 0:
            assert np.all(got == 0)
    # a batch of clips of one length: every row normalised on its own
    rng = np.random.default_rng(3)
    clips = (rng.standard_normal((4, 100001)) * np.array([[0.01], [1.0], [30.0], [0.0]])).astype(np.float32)
    got = tools.rms_norm_batch(torch.from_numpy(clips).cuda()).cpu().numpy()
    assert np.all(got[3] == 0)
    for b in range(3):
        assert abs(np.sqrt(np.mean(got[b].astype(np.float64) ** 2)) - 1.0) < 1e-5


@pytest.mark.parametrize('n_fft', [128, 512, 1024, 4096])
@pytest.mark.parametrize('kind', ['mel', 'stft'])
def test_other_frame_lengths_match_oracle(n_fft, kind):
    """STFT / MelSpec take any n_fft (amt_tools/features/stft.py:15-40, mel.py:15-38): powers of two 128 .. 4096 besides the tuned 2048
    run on the generic radix-2 kernel; same tolerances as the 2048 path, both librosa padding conventions, linear and dB output."""
    MelSpec, STFT = _mods()
    y = synth_clip(20 + n_fft % 7, num_samples=30000)
    hop = max(32, n_fft // 4)
    for lv in ('0.10', '0.9'):
        if kind == 'mel':
            n_mels = min(229, n_fft // 8)
            mod = MelSpec(sample_rate=22050, hop_length=hop, n_mels=n_mels, n_fft=n_fft, librosa_version=lv)
            ref = fe.melspec_process_audio(y, 22050, hop, n_mels, n_fft, lv=lv)
        else:
            mod = STFT(sample_rate=22050, hop_length=hop, n_fft=n_fft, librosa_version=lv)
            ref = fe.stft_process_audio(y, hop, n_fft, lv=lv)
        got = mod.process_audio(y)
        assert got.shape == ref.shape and got.dtype == np.float32
        assert np.abs(got - ref).max() < TOL_POW2, (n_fft, kind, lv)
    lin = STFT(sample_rate=22050, hop_length=hop, n_fft=n_fft, decibels=False)
    ref = fe.stft_process_audio(y, hop, n_fft, decibels=False)
    assert np.abs(lin.process_audio(y) - ref).max() <= 4e-6 * ref.max()


def test_short_window_not_centered_stft_is_the_bookkeeping_goldens_module():
    """The `stft_nc` module of tests/golden/feature_bookkeeping.npz (n_fft 1024, win_length 800, hop 256, center=False, 16 kHz) now
    also runs on the GPU: values and frame counts against the oracle (= what librosa.stft returns for the reference's padded
    audio: frames are n_fft long).  Reference quirk, recorded not fixed: its own get_expected_frames counts win_length-long frames
    (features/waveform.py:43-67), so for win_length < n_fft it predicts one frame more than its process_audio returns -- the mirror
    reproduces the prediction (tests/test_feature_bookkeeping.py, golden) and the kernels reproduce the output."""
    _, STFT = _mods()
    mod = STFT(sample_rate=16000, hop_length=256, n_fft=1024, win_length=800, center=False)
    for n in (1024, 1025, 2047, 2048, 2049, 4095, 4096, 22050):
        y = synth_clip(n % 5, num_samples=n)
        got = mod.process_audio(y)
        ref = fe.stft_process_audio(y, 256, 1024, win_length=800, center=False)
        assert got.shape == ref.shape and got.shape[-1] >= 1, (n, got.shape, ref.shape)
        assert np.abs(got - ref).max() < TOL_POW2, n
    # the same window shape on the tuned 2048 kernel (win_length < n_fft there too), centred
    y = synth_clip(2, num_samples=20000)
    wide = STFT(sample_rate=22050, hop_length=512, n_fft=2048, win_length=1500)
    assert np.abs(wide.process_audio(y) - fe.stft_process_audio(y, 512, 2048, win_length=1500)).max() < TOL_POW2      # measured 2.6e-5


_RING_VS_GENERAL = r'''
import os, sys
import numpy as np, torch
sys.path.insert(0, os.getcwd())
from amt_tools_amd.features import MelSpec
from amt_tools_amd.synth import synth_clip
mod = MelSpec(sample_rate=22050, hop_length=512, n_mels=229, n_fft=2048, librosa_version=sys.argv[2])
outs = []
for n in (319999, 512 * 37 + 11, 2049, 70001, 1025):
    a = np.stack([synth_clip(i, num_samples=n) for i in range(5)])
    a[1] *= 1e-3
    a[3] = 0
    power, cmax = mod.power_batch(torch.from_numpy(a).cuda())
    outs += [power.cpu().numpy(), cmax.cpu().numpy()]
np.savez(sys.argv[1], *outs)
'''


@pytest.mark.parametrize('lv', ['0.10', '0.9'])
def test_ring_kernel_returns_the_bits_of_the_general_kernel(tmp_path, lv):
    """The BASELINE log-mel shape (n_fft 2048, hop 512, 229 Slaney rows at 22.05 kHz) runs on spec_power_ring_kernel (clip ring in LDS, mel
    weights in registers); AMTX_SPEC_NO_RING=1 keeps the general spec_power_kernel.  Same arithmetic, same order: the power mel
    spectrograms and the clip maxima must be IDENTICAL, for full-size clips, ragged lengths (frames that straddle the clip end,
    chunks with inactive waves), both padding modes (zeros / reflection), a silent clip and clips 60 dB apart."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = {}
    for tag, extra in (('ring', {}), ('general', {'AMTX_SPEC_NO_RING': '1'})):
        env = dict(os.environ)
        env.update(extra)
        files[tag] = str(tmp_path / f'{tag}.npz')
        subprocess.check_call([sys.executable, '-c', _RING_VS_GENERAL, files[tag], lv], env=env, cwd=root)
    ring, general = np.load(files['ring']), np.load(files['general'])
    assert len(ring.files) == 10
    for k in ring.files:
        np.testing.assert_array_equal(ring[k], general[k])
    assert ring['arr_0'].shape == (5, 625, 229) and ring['arr_0'].max() > 0


# (module, the case of tests/golden/frontend_trace.json that names its kernel): the five routes of spec.hip's spec_route
SPEC_ROUTES = {
    'ring': (lambda M, S: M(sample_rate=22050, hop_length=512, n_mels=229, n_fft=2048), '22050 2048 512 229 1 0'),
    'general_mel_lds': (lambda M, S: M(sample_rate=22050, hop_length=512, n_mels=128, n_fft=2048), '22050 2048 512 128 1 0'),
    'general_mel': (lambda M, S: M(sample_rate=22050, hop_length=512, n_mels=64, n_fft=2048), '22050 2048 512 64 1 0'),
    'general_stft': (lambda M, S: S(sample_rate=22050, hop_length=512, n_fft=2048), '22050 2048 512 0 1 0'),
    'pow2': (lambda M, S: M(sample_rate=16000, hop_length=256, n_mels=80, n_fft=1024), '16000 1024 256 80 1 0'),
}


@pytest.mark.parametrize('route', sorted(SPEC_ROUTES))
def test_each_call_launches_the_one_kernel_of_the_recorded_trace(route):
    """process_batch (equal clips) and process_clips of a TrackBank of the same plan (clip table) each launch exactly one spec_power* kernel:
    the instantiation -- template arguments and source type -- the host trace recorded for that plan (tests/test_frontend_trace.py)."""
    import json
    import re
    import sys
    from amt_tools_amd.tracks import TrackBank
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'san'))
    import frontend_trace
    make, plan = SPEC_ROUTES[route]
    mod = make(*_mods())
    n_fft, hop = int(plan.split()[1]), int(plan.split()[2])
    n = 2 * n_fft + 3 * hop + 7
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'frontend_trace.json')) as f:
        golden = json.load(f)
    assert golden['cases_sha256'] == frontend_trace.cases_sha256()
    cases, recorded_run = frontend_trace.cases(), frontend_trace.expand(golden)['']

    def recorded(entry, x):                # the kernel of the run without a switch, as 'spec_power..._kernel<...>'
        _, _, (launch,) = recorded_run[cases.index('spec %s %s 2 %d' % (entry, plan, x))]
        return re.search(r'spec_power\w*_kernel<[^>]*>', launch).group(0)
    tracks = [synth_clip(20 + i, num_samples=n) for i in range(2)]
    audio = torch.from_numpy(np.stack(tracks)).to('cuda:0')
    bank = TrackBank(tracks, mod, 'cuda:0')
    clips = bank.clips([0, 1], [0, 0], 1 + n // hop)
    for name, run, want in (('process_batch', lambda: mod.process_batch(audio), recorded('power', 512 * 9)),
                            ('process_clips', lambda: mod.process_clips(clips), recorded('power_clips', 1 + 512 * 9 // hop))):
        run()                                                         # plan creation, the bank's upload and the LDS grant stay out of the profile
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            run()
            torch.cuda.synchronize()
        ran = [(m.group(0), e.count) for e in prof.key_averages() for m in [re.search(r'spec_power\w*_kernel<[^>]*>', e.key)] if m]
        print(f'SPECROUTE {route} {name}: {ran}')
        assert ran == [(want, 1)], (route, name, want, [e.key for e in prof.key_averages()])
