"""Clips cut from device-resident tracks (amtx_spec_power_clips, amt_tools_amd/tracks.py) on the GPU.

The acceptance criterion is an identity, not a tolerance: a frame's arithmetic and summation order do not depend on where the frame's
header comes from, so the rows and maxima of a clip are the BITS of amtx_spec_power run on the clip's whole track.  Everything here
that compares this package with itself uses assert_array_equal.  The one tolerance is TOL_SCALED = 2e-5 against the fp64 oracle: the
front-end bound of tests/test_gpu_frontend.py, for the same comparison on whole clips.

Set-up shared by the kernel tests: three tracks of 40 000, 5 000 and 1 500 samples back to back WITHOUT a gap, in a buffer that is a
slice of a larger NaN-filled tensor, 64 elements in from each end -- one sample read outside a track (a neighbour's, or a NaN) changes
bits."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from amt_tools_amd import _lib, tools                                  # noqa: E402
from amt_tools_amd.synth import synth_clip, synth_state_dict           # noqa: E402
from amt_tools_amd.tracks import TrackBank, frame_start                # noqa: E402
from poison import PATTERNS, Poison, assert_same, snapshot             # noqa: E402

DEV = 'cuda:0'
TOL_SCALED = 2e-5
LENGTHS = (40000, 5000, 1500)
STARTS = (0, 40000, 45000)
NUM_FRAMES = 33                      # 32 frames per block: two chunks, the second nearly empty


def _plans():
    from amt_tools_amd.features import MelSpec, STFT
    return {'ring_zeros': lambda: MelSpec(sample_rate=22050, hop_length=512, n_mels=229, n_fft=2048, librosa_version='0.10'),
            'ring_reflect': lambda: MelSpec(sample_rate=22050, hop_length=512, n_mels=229, n_fft=2048, librosa_version='0.9'),
            'general_lds_table': lambda: MelSpec(sample_rate=44100, n_mels=128),
            'general_memory_table': lambda: MelSpec(sample_rate=22050, n_mels=512),
            'stft_2048': lambda: STFT(n_fft=2048),
            'stft_pow2': lambda: STFT(n_fft=512, hop_length=128),            # track 2 has 12 frames
            'not_centered': lambda: MelSpec(center=False)}


@functools.lru_cache(maxsize=None)
def _tracks():
    """(the three tracks on the host, the packed device buffer inside its NaN frame)."""
    tracks = [synth_clip(40 + i, num_samples=n) for i, n in enumerate(LENGTHS)]
    frame = torch.full((64 + sum(LENGTHS) + 64,), float('nan'), dtype=torch.float32, device=DEV)
    buf = frame[64:64 + sum(LENGTHS)]
    buf.copy_(torch.from_numpy(np.concatenate(tracks)))
    assert torch.isnan(frame[:64]).all() and torch.isnan(frame[-64:]).all() and buf.data_ptr() == frame.data_ptr() + 256
    return tracks, buf


@functools.lru_cache(maxsize=None)
def _whole_tracks(name):
    """(module, [power map (T_i, F) of track i], [its maximum]) from amtx_spec_power on each track ALONE: computed once per plan."""
    mod = _plans()[name]()
    tracks, _ = _tracks()
    powers, maxima = [], []
    for y in tracks:
        power, cmax = mod.power_batch(torch.from_numpy(y).to(DEV).unsqueeze(0))
        powers.append(power[0].cpu().numpy())
        maxima.append(cmax.cpu().numpy()[0])
    for a in powers:
        a.setflags(write=False)
    return mod, powers, maxima


def _ff_filled(shape):
    """A float32 device tensor whose every byte is 0xFF (NaN): what the kernel does not write shows."""
    t = torch.empty(shape, dtype=torch.float32, device=DEV)
    t.view(torch.uint8).fill_(0xFF)
    return t


@pytest.mark.parametrize('name', sorted(_plans()))
def test_rows_and_maxima_are_the_whole_track_bits(name):
    """ONE launch of six clips -- a track's left edge, a first frame that is no multiple of the block's 32 frames, a track's right edge,
    a whole track shorter than the clip's map (frames < num_frames), the tail of that track, and a track whose every window touches
    both of its ends: rows [0, frames) are the whole-track rows, the rows beyond are zeros, clip_max is the maximum of the valid rows."""
    mod, powers, _ = _whole_tracks(name)
    _, buf = _tracks()
    plan = mod._get_plan(DEV)
    counts = [int(_lib.call('amtx_spec_num_frames', plan, n)) for n in LENGTHS]
    assert counts == [p.shape[0] for p in powers] and counts[0] >= 37 + NUM_FRAMES
    if name == 'stft_pow2':
        assert counts[2] == 12
    tail1 = 3 if counts[1] - 3 <= NUM_FRAMES else counts[1] - NUM_FRAMES
    clips = [(0, 0), (0, 37), (0, counts[0] - NUM_FRAMES), (1, 0), (1, tail1), (2, 0)]            # (track, first frame)
    desc = np.array([[STARTS[k], LENGTHS[k], first, min(NUM_FRAMES, counts[k] - first)] for k, first in clips], dtype=np.int64)
    assert (desc[:, 3] >= 1).all() and (desc[:, 2] + desc[:, 3] <= np.array(counts)[[k for k, _ in clips]]).all()
    if name not in ('stft_pow2',):
        assert desc[3, 3] == counts[1] < NUM_FRAMES and desc[4, 2] + desc[4, 3] == counts[1] and desc[5, 3] == counts[2]
    F = powers[0].shape[1]
    power, cmax = _ff_filled((len(clips), NUM_FRAMES, F)), _ff_filled((len(clips),))
    _lib.call('amtx_spec_power_clips', plan, buf, torch.from_numpy(desc).to(DEV), len(clips), NUM_FRAMES, power, cmax, device=DEV)
    power, cmax = power.cpu().numpy(), cmax.cpu().numpy()
    for b, ((k, first), frames) in enumerate(zip(clips, desc[:, 3])):
        want = powers[k][first:first + frames]
        np.testing.assert_array_equal(power[b, :frames], want, err_msg=f'{name}: clip {b} (track {k}, first frame {first})')
        np.testing.assert_array_equal(power[b, frames:], np.zeros((NUM_FRAMES - frames, F), dtype=np.float32), err_msg=f'{name}: clip {b} tail')
        np.testing.assert_array_equal(cmax[b], want.max(), err_msg=f'{name}: clip {b} maximum')


@pytest.mark.parametrize('name', sorted(_plans()))
def test_maxima_only_launch_and_bank_db_ref(name):
    """power = NULL: the three tracks as three descriptors of their own lengths in one launch give the three amtx_spec_power maxima,
    exactly -- and that is what TrackBank.db_ref holds."""
    mod, powers, maxima = _whole_tracks(name)
    tracks, buf = _tracks()
    counts = [p.shape[0] for p in powers]
    desc = np.array([[STARTS[k], LENGTHS[k], 0, counts[k]] for k in range(3)], dtype=np.int64)
    cmax = _ff_filled((3,))
    _lib.call('amtx_spec_power_clips', mod._get_plan(DEV), buf, torch.from_numpy(desc).to(DEV), 3, max(counts), None, cmax, device=DEV)
    np.testing.assert_array_equal(cmax.cpu().numpy(), np.array(maxima))
    np.testing.assert_array_equal(np.array(maxima), [p.max() for p in powers])
    bank = TrackBank(tracks, mod, DEV)
    np.testing.assert_array_equal(bank.frame_counts, counts)
    np.testing.assert_array_equal(bank.db_ref.cpu().numpy(), np.array(maxima))
    np.testing.assert_array_equal(bank.audio.cpu().numpy(), np.concatenate(tracks))


def test_bank_refuses_a_frame_count_that_is_not_the_plans():
    """A module that is not centred with win_length < n_fft expects one frame more than its plan computes (the reference's own quirk,
    tests/test_gpu_frontend.py): the bank says so when it goes to the device instead of framing clips from padding."""
    from amt_tools_amd.features import STFT
    mod = STFT(sample_rate=16000, hop_length=256, n_fft=1024, win_length=800, center=False)
    bank = TrackBank([synth_clip(1, num_samples=4096)], mod, DEV)
    assert bank.frame_counts.tolist() == [14]
    with pytest.raises(ValueError, match='expects 14 frames, its plan computes 13'):
        bank.db_ref


# ------------------------------------------------------------------------------------------------------------------------------
# feature semantics: a track 40 dB quieter before sample 45 000 than after
# ------------------------------------------------------------------------------------------------------------------------------
def _two_level_track():
    y = synth_clip(3, num_samples=60000).copy()
    y[:45000] *= 0.01
    return y


def test_features_are_the_slices_of_the_track_map():
    from amt_tools_amd.features import MelSpec
    from oracle import frontend_np as fe
    mod = MelSpec(sample_rate=16000, hop_length=512, n_mels=229, n_fft=2048)
    y = _two_level_track()
    other = synth_clip(8, num_samples=7001)                  # a first track, so that the track under test does not start the buffer
    bank = TrackBank([other, y], mod, DEV)
    T = 1 + 60000 // 512
    firsts = [frame_start(5 * 512 + 100, 512), T - NUM_FRAMES]
    assert firsts == [5, 85]
    clips = bank.clips([1, 1], firsts, NUM_FRAMES)
    whole = mod.process_batch(torch.from_numpy(y).to(DEV).unsqueeze(0))[0].cpu().numpy()            # (1, F, T)
    assert whole.shape == (1, 229, T)
    oracle = fe.melspec_process_audio(y, 16000, 512, 229, 2048)
    got = mod.process_clips(clips).cpu().numpy()
    got_t = mod.process_clips(clips, model_layout=True).cpu().numpy()
    assert got.shape == (2, 1, 229, NUM_FRAMES) and got_t.shape == (2, 1, NUM_FRAMES, 229)
    for b, first in enumerate(firsts):
        np.testing.assert_array_equal(got[b], whole[..., first:first + NUM_FRAMES])
        np.testing.assert_array_equal(got_t[b], np.swapaxes(whole[..., first:first + NUM_FRAMES], -1, -2))
        err = np.abs(got[b] - oracle[..., first:first + NUM_FRAMES]).max()
        print(f'clip at frame {first}: max abs error against the oracle {err:.3e}')
        assert err < TOL_SCALED
    # not vacuous: the same clip's own samples through the ordinary path (own maximum, own padding) are 40 dB of 80 away on the frames
    # whose windows (2 hops to each side) lie inside the clip
    own = mod.process_batch(torch.from_numpy(y[5 * 512:5 * 512 + 32 * 512]).to(DEV).unsqueeze(0))[0].cpu().numpy()
    assert own.shape == (1, 229, NUM_FRAMES)
    gap = np.abs(own[..., 2:-2] - whole[..., 5 + 2:5 + NUM_FRAMES - 2]).max()
    print(f'clip-own features against the track slices, interior frames: {gap:.3f}')
    assert gap > 0.25


# ------------------------------------------------------------------------------------------------------------------------------
# the model seam
# ------------------------------------------------------------------------------------------------------------------------------
def test_onsets_frames_takes_clips_under_key_audio():
    from amt_tools_amd.features import MelSpec
    from amt_tools_amd.models import OnsetsFrames, PendingFeatures
    mod = MelSpec(sample_rate=16000, hop_length=512, n_mels=229, n_fft=2048)
    sd = synth_state_dict(7, dim_in=229, in_channels=1, model_complexity=2)
    model = OnsetsFrames(229, tools.PianoProfile(), 1, 2, device=DEV, precision='x3')
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model.frontend = torch.nn.Sequential(mod.frontend())
    model.change_device()
    model.eval()
    tracks = [_two_level_track(), synth_clip(9, num_samples=30000)]
    bank = TrackBank(tracks, mod, DEV)
    ids, firsts, T = [0, 1, 0], [60, 0, 118 - 40], 40
    clips = bank.clips(ids, firsts, T)
    whole = [mod.process_batch(torch.from_numpy(y).to(DEV).unsqueeze(0))[0] for y in tracks]        # (1, F, T_k)
    slices = torch.stack([whole[k][..., f:f + T] for k, f in zip(ids, firsts)]).contiguous()         # (3, 1, F, T)
    audio = torch.from_numpy(np.stack([y[:512 * 39 + 7] for y in (tracks[0], tracks[1], tracks[0])])).to(DEV)
    with torch.no_grad():
        before = model.run_on_batch({tools.KEY_AUDIO: audio})
        model.__dict__['_in_run_on_batch'] = True
        try:
            pre = model.pre_proc({tools.KEY_AUDIO: clips})
        finally:
            model.__dict__.pop('_in_run_on_batch')
        assert isinstance(pre[tools.KEY_FEATS], PendingFeatures) and pre[tools.KEY_FEATS].ref is None       # the dB scale stays in the conv kernel
        np.testing.assert_array_equal(pre[tools.KEY_FEATS].clip_max.cpu().numpy(), bank.db_ref.cpu().numpy()[ids])
        got = model.run_on_batch({tools.KEY_AUDIO: clips})
        want = model.run_on_batch({tools.KEY_FEATS: slices})
    for key in (tools.KEY_ONSETS, tools.KEY_MULTIPITCH):
        assert got[key].shape == (3, 88, T)
        np.testing.assert_array_equal(got[key].cpu().numpy(), want[key].cpu().numpy())

    # training mode: pre_proc yields the feature bits themselves; one labelled step runs through
    model.train()
    feats = model.pre_proc({tools.KEY_AUDIO: clips})[tools.KEY_FEATS]                                 # (B, 1, T, F): frequency <-> time swapped
    assert torch.is_tensor(feats)
    np.testing.assert_array_equal(feats.transpose(-1, -2).cpu().numpy(), slices.cpu().numpy())
    rng = np.random.default_rng(0)
    batch = {tools.KEY_AUDIO: clips,
             tools.KEY_MULTIPITCH: torch.from_numpy((rng.random((3, 88, T)) < 0.05).astype(np.float32)),
             tools.KEY_ONSETS: torch.from_numpy((rng.random((3, 88, T)) < 0.02).astype(np.float32))}
    loss = model.run_on_batch(batch)[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL]
    loss.backward()
    assert torch.isfinite(loss).item()
    for pname, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all().item(), pname

    # an audio-tensor batch runs exactly as before
    model.eval()
    with torch.no_grad():
        after = model.run_on_batch({tools.KEY_AUDIO: audio})
    for key in (tools.KEY_ONSETS, tools.KEY_MULTIPITCH):
        np.testing.assert_array_equal(after[key].cpu().numpy(), before[key].cpu().numpy())

    # clips need the model's one spectral front-end
    bare = OnsetsFrames(229, tools.PianoProfile(), 1, 2, device=DEV)
    with pytest.raises(TypeError, match='exactly one SpectralFrontend'):
        bare.pre_proc({tools.KEY_AUDIO: clips})


# ------------------------------------------------------------------------------------------------------------------------------
# uninitialised memory
# ------------------------------------------------------------------------------------------------------------------------------
def test_bank_and_clips_do_not_depend_on_memory_contents(monkeypatch):
    """Bank construction (the maxima launch) + process_clips with every torch.empty allocation filled with 0x00, 0xFF, 0x7F."""
    from amt_tools_amd.features import MelSpec
    poison = Poison(monkeypatch, 0x00)
    tracks, _ = _tracks()
    ref = None
    for pattern in PATTERNS:
        poison.pattern = pattern
        mod = MelSpec(sample_rate=22050, hop_length=512, n_mels=229, n_fft=2048)
        bank = TrackBank(tracks, mod, DEV)
        clips = bank.clips([0, 0, 1, 2], [0, 41, 7, 0], 3)
        power, track_max = mod.power_clips(clips)
        got = snapshot({'db_ref': bank.db_ref, 'feats': mod.process_clips(clips), 'model_layout': mod.process_clips(clips, model_layout=True),
                        'power': power, 'track_max': track_max})
        if ref is None:
            ref = got
        else:
            assert_same(got, ref, f'fill {pattern:#04x}')
    assert poison.filled > 0 and (ref['db_ref'] > 0).all()
