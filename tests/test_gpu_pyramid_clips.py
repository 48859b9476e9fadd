"""CQT-family clips cut from the resident decimation pyramids of whole tracks (include/amtx_pyramid.h, amt_tools_amd/tracks.py
PyramidBank) on the GPU.

The acceptance criterion is an identity: the bank's level signals are produced by the whole-track forward's own kernels on the whole
track, and the basis kernel computes a frame from its window alone, in a fixed order -- so a clip's maps are the BITS of the track's own
map, columns [first_frame, first_frame + frames).  Everything that compares this package with itself uses assert_array_equal.  The one
tolerance is TOL = 1e-3 against the fp64 oracle: the bound tests/test_gpu_cqt.py holds for the same clip and plan on the whole map.

Shared set-up of the kernel tests: tracks of 50 000, 23 001 and 17 001 samples (odd lengths: (len + 1) / 2 halvings, level ends that are
no multiple of 4) and, for zero-padded plans, one of 1 500 samples (3 frames), in audio and pyramid buffers that are slices of NaN-filled
tensors 64 elements in from each end; the tracks lie back to back with the alignment gaps NaN-filled too, so one sample read outside a
track changes bits.

One plan of the issue's list has no identity to hold: VQT(n_bins=72).  Its default gamma shortens the low filters to an n_fft of 64 and
less, which sends the WHOLE plan to the generic GEMM in the whole-track forward (tests/test_gpu_cqt.py says so of the same plan), and the
generic-GEMM basis path gets no clip form: such a plan answers AMTX_ERR_UNSUPPORTED.  The case stays in the list and asserts exactly that
(_assert_no_clip_form); 'vqt_gamma2', a VQT whose filters stay at 128 taps and more, stands beside it for the identity."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from amt_tools_amd import _lib, tools                                                   # noqa: E402
from amt_tools_amd.synth import synth_clip, synth_state_dict, synth_tabcnn_state_dict   # noqa: E402
from amt_tools_amd.tracks import PyramidBank, PyramidClips                              # noqa: E402
from poison import PATTERNS, Poison, assert_same, snapshot                              # noqa: E402

DEV = 'cuda:0'
TOL = 1e-3
LENGTHS = (50000, 23001, 17001, 1500)
NUM_FRAMES = 33                      # three groups of 16 frames, the last with one frame


def _plans():
    from amt_tools_amd.features import CQT, HCQT, VQT
    return {'tabcnn_zeros': lambda: CQT(22050, 512, n_bins=192, bins_per_octave=24, librosa_version='0.10'),       # deepest level: hop 4
            'tabcnn_reflect': lambda: CQT(22050, 512, n_bins=192, bins_per_octave=24, librosa_version='0.9'),
            'hcqt': lambda: HCQT(22050, 512, n_bins=72),                     # 6 harmonics, 144-column levels: a second column slice
            'vqt': lambda: VQT(n_bins=72),                                  # a generic-GEMM plan: no clip form (module docstring)
            'vqt_gamma2': lambda: VQT(n_bins=72, gamma=2.0),
            'cqt_linear': lambda: CQT(n_bins=84, decibels=False)}


GEMM_PLANS = ('vqt',)


def _assert_no_clip_form(name):
    """The whole-track forward takes every track; the layout query answers AMTX_ERR_UNSUPPORTED; the bank says so on the device."""
    mod = _plans()[name]()
    tracks = [synth_clip(40 + i, num_samples=n) for i, n in enumerate(LENGTHS)]
    for y in tracks:
        assert mod.process_batch(torch.from_numpy(y).to(DEV).unsqueeze(0)).shape == (1, 1, 72, mod.get_expected_frames(y))
    arrays = [(C.c_int64 * 16)() for _ in range(3)]
    rc = _lib.lib().amtx_cqt_track_layout(mod._get_plan(DEV), 50000, *arrays, C.byref(C.c_int64()))
    assert rc == _lib.ERR_UNSUPPORTED
    bank = PyramidBank(tracks, mod, DEV)
    with pytest.raises(NotImplementedError, match='VQT: .*no clip form'):
        bank.db_ref
    with pytest.raises(NotImplementedError, match='no clip form'):
        bank.clips([0], [0], NUM_FRAMES)


def _host(t):
    a = t.float().cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()
    a.setflags(write=False)
    return a


def _nan_framed(n):
    frame = torch.full((64 + n + 64,), float('nan'), dtype=torch.float32, device=DEV)
    return frame[64:64 + n]


@functools.lru_cache(maxsize=None)
def _setup(name):
    """Per plan, computed once: the module, its tracks, every track's whole maps from the ordinary forward on that track ALONE (fp32,
    bf16, the two planes of the split) and a bank built through the C ABI in NaN-framed buffers."""
    mod = _plans()[name]()
    reflect = str(mod.librosa_version).startswith('0.9')
    tracks = [synth_clip(40 + i, num_samples=n) for i, n in enumerate(LENGTHS[:3 if reflect else 4])]
    whole = []
    for y in tracks:
        x = torch.from_numpy(y).to(DEV).unsqueeze(0)                    # the whole-track forward accepts every track of every plan
        whole.append({'f32': _host(mod.process_batch(x)[0]), 'b16': _host(mod.process_batch16(x)[0]),
                      'split': _host(mod.process_batch16(x, split=True)[:, 0])})
    plan = mod._get_plan(DEV)
    cols, H = _lib.call('amtx_cqt_track_cols', plan), _lib.call('amtx_cqt_num_harmonics', plan)
    table = np.zeros((len(tracks), cols), dtype=np.int64)
    start = place = 0
    for i, y in enumerate(tracks):
        lens, strides, rows = ((C.c_int64 * 16)() for _ in range(3))
        frames = C.c_int64()
        levels = _lib.call('amtx_cqt_track_layout', plan, y.size, lens, strides, rows, C.byref(frames))
        assert cols == 4 + 3 * levels + H and frames.value == whole[i]['f32'].shape[-1] == mod.get_expected_frames(y)
        assert (strides[0] == 0) == (not reflect) and all(s % 4 == 0 for s in strides[:levels])
        table[i, :4] = (start, y.size, max(rows[:H]), frames.value)
        for l in range(levels):
            table[i, 4 + 3 * l:7 + 3 * l] = (place, lens[l], strides[l])
            place += strides[l]
        table[i, 4 + 3 * levels:] = rows[:H]
        start += -(-y.size // 4) * 4                                     # the only gap: up to the next multiple of 4 elements
    audio, pyramid = _nan_framed(start), _nan_framed(place)
    for row, y in zip(table, tracks):
        audio[row[0]:row[0] + y.size] = torch.from_numpy(y).to(DEV)
    assert torch.isnan(audio[23001 + 50000:23004 + 50000]).all() and torch.isnan(pyramid).all()
    table_dev = torch.from_numpy(table).to(DEV)
    db_ref = torch.empty((len(tracks), H), dtype=torch.float32, device=DEV)
    db_ref.view(torch.uint8).fill_(0xFF)
    _lib.call('amtx_cqt_pyramid_build', plan, audio, audio.numel(), table, table_dev, len(tracks), pyramid, pyramid.numel(), db_ref, device=DEV)
    assert not torch.isnan(pyramid).any()                               # every element of every level's stride is written
    bank = types.SimpleNamespace(module=mod, audio=audio, pyramid=pyramid, table=table_dev, db_ref=db_ref)
    return mod, tracks, whole, bank


def _clips_of(bank, rows):
    """PyramidClips of descriptor rows (track, first frame, frames) over a hand-built bank."""
    desc = np.array(rows, dtype=np.int64)
    ids = torch.from_numpy(desc[:, 0]).to(DEV)
    clips = PyramidClips(bank, desc, torch.from_numpy(desc).to(DEV), bank.db_ref[ids])
    return clips


def _ff_filled(shape):
    t = torch.empty(shape, dtype=torch.float32, device=DEV)
    t.view(torch.uint8).fill_(0xFF)
    return t


@pytest.mark.parametrize('name', sorted(_plans()))
def test_clip_maps_are_the_whole_track_bits(name):
    """ONE launch per form over: a track's left edge, a first frame that is no multiple of 16, a track's right edge, the right edge of
    an odd-length track, a clip with fewer frames than its map has columns that ends where its track ends and, for zero-padded plans, a
    whole track of 3 frames."""
    if name in GEMM_PLANS:
        return _assert_no_clip_form(name)
    mod, tracks, whole, bank = _setup(name)
    counts = [w['f32'].shape[-1] for w in whole]
    assert counts[:3] == [98, 45, 34]
    rows = [(0, 0, NUM_FRAMES), (0, 37, NUM_FRAMES), (0, counts[0] - NUM_FRAMES, NUM_FRAMES), (1, counts[1] - NUM_FRAMES, NUM_FRAMES),
            (2, 5, counts[2] - 5)]
    if len(tracks) == 4:
        assert counts[3] == 3
        rows.append((3, 0, 3))
    clips = _clips_of(bank, rows)
    assert clips.num_frames == NUM_FRAMES and clips.num_clips == len(rows)
    B, H, F = len(rows), whole[0]['f32'].shape[0], whole[0]['f32'].shape[1]

    power = _ff_filled((B, H, F, NUM_FRAMES))
    _lib.call('amtx_cqt_power_clips', mod._get_plan(DEV), bank.audio, bank.pyramid, bank.table, clips.desc_dev, B, NUM_FRAMES, power, device=DEV)
    power = power.cpu().numpy()
    via_module, db_ref = mod.power_clips(clips)
    np.testing.assert_array_equal(via_module.cpu().numpy(), power)
    np.testing.assert_array_equal(db_ref.cpu().numpy(), bank.db_ref.cpu().numpy()[[r[0] for r in rows]])
    got = mod.process_clips(clips).cpu().numpy()
    got_t = mod.process_clips(clips, model_layout=True).cpu().numpy()
    got16 = _host(mod.process_clips16(clips))
    got16s = _host(mod.process_clips16(clips, split=True))
    assert got.shape == (B, H, F, NUM_FRAMES) and got_t.shape == (B, H, NUM_FRAMES, F)
    assert got16.shape == (B, NUM_FRAMES, F, 8) and got16s.shape == (2, B, NUM_FRAMES, F, 8)
    for b, (k, first, frames) in enumerate(rows):
        what = f'{name}: clip {b} (track {k}, first frame {first})'
        assert np.isfinite(power[b, ..., :frames]).all() and power[b, ..., :frames].max() > 0, what
        np.testing.assert_array_equal(power[b, ..., frames:], np.zeros((H, F, NUM_FRAMES - frames), dtype=np.float32), err_msg=what + ' tail')
        want = whole[k]['f32'][..., first:first + frames]
        np.testing.assert_array_equal(got[b, ..., :frames], want, err_msg=what)
        np.testing.assert_array_equal(got_t[b, :, :frames], np.swapaxes(want, -1, -2), err_msg=what + ' model layout')
        np.testing.assert_array_equal(got16[b, :frames], whole[k]['b16'][first:first + frames], err_msg=what + ' bf16')
        np.testing.assert_array_equal(got16s[:, b, :frames], whole[k]['split'][:, first:first + frames], err_msg=what + ' split')


@pytest.mark.parametrize('name', sorted(_plans()))
def test_bank_maxima_are_the_tracks_references(name):
    """db_ref[k, h] is the maximum of harmonic h's power map over that harmonic's OWN frames of track k: equal to the maximum of the
    power_clips map of the whole track for the single-harmonic plans, at least that for HCQT (whose map is truncated to the smallest
    frame count) -- and the PyramidBank's own device state holds the same bits as the hand-built bank."""
    if name in GEMM_PLANS:
        return _assert_no_clip_form(name)
    mod, tracks, whole, raw = _setup(name)
    bank = PyramidBank(tracks, mod, DEV)
    np.testing.assert_array_equal(bank.frame_counts, [w['f32'].shape[-1] for w in whole])
    np.testing.assert_array_equal(bank.db_ref.cpu().numpy(), raw.db_ref.cpu().numpy())
    np.testing.assert_array_equal(bank.pyramid.cpu().numpy(), raw.pyramid.cpu().numpy())
    np.testing.assert_array_equal(bank.table.cpu().numpy(), raw.table.cpu().numpy())
    assert bank.db_ref.shape == (len(tracks), whole[0]['f32'].shape[0])
    for k, T in enumerate(bank.frame_counts):
        clips = bank.clips([k], [0], int(T))
        power, ref = mod.power_clips(clips)
        top = power[0].amax(dim=(-1, -2)).cpu().numpy()
        np.testing.assert_array_equal(ref.cpu().numpy()[0], bank.db_ref.cpu().numpy()[k])
        if name == 'hcqt':
            assert (bank.db_ref.cpu().numpy()[k] >= top).all() and (top > 0).all()
        else:
            np.testing.assert_array_equal(bank.db_ref.cpu().numpy()[k], top)
        # ... and the dB identity, which depends on the exact reference, through the bank's own clips
        np.testing.assert_array_equal(mod.process_clips(clips).cpu().numpy()[0], whole[k]['f32'])


@pytest.mark.parametrize('lv', ['0.10', '0.9'])
def test_clips_match_the_oracle_like_the_whole_map(lv):
    """The clip and plan of tests/test_gpu_cqt.py::test_cqt_config1_matches_oracle, same bound."""
    from amt_tools_amd.features import CQT
    from oracle import cqt_np as cq
    y = synth_clip(2, num_samples=50000)
    mod = CQT(sample_rate=22050, hop_length=512, n_bins=192, bins_per_octave=24, librosa_version=lv)
    ref = cq.cqt_process_audio(y, sample_rate=22050, hop_length=512, n_bins=192, bins_per_octave=24, lv=lv)
    T = ref.shape[-1]
    firsts = [0, 37, T - NUM_FRAMES]
    got = mod.process_clips(PyramidBank([y], mod, DEV).clips([0, 0, 0], firsts, NUM_FRAMES)).cpu().numpy()
    for b, first in enumerate(firsts):
        err = np.abs(got[b] - ref[..., first:first + NUM_FRAMES]).max()
        print(f'librosa {lv}, clip at frame {first}: max abs error against the oracle {err:.3e}')
        assert err < TOL


@pytest.mark.parametrize('kw', [dict(n_bins=84), dict(n_bins=192, bins_per_octave=24)], ids=['84', '192_24'])
def test_track_level_scale_is_not_the_clips_own(kw):
    """A track 40 dB quieter before sample 45 000 than after: the clip at frame 5 is the track map's slice, and the same clip's own
    samples through the ordinary path (own maximum, own padding) are far from it on interior frames.  The CPU oracle gives 0.508 for both
    plans: 0.25 leaves a factor of two."""
    from amt_tools_amd.features import CQT
    mod = CQT(sample_rate=22050, hop_length=512, **kw)
    y = synth_clip(3, num_samples=60000).copy()
    y[:45000] *= 0.01
    other = synth_clip(8, num_samples=7001)                  # a first track, so that the track under test does not start the buffer
    bank = PyramidBank([other, y], mod, DEV)
    whole = mod.process_batch(torch.from_numpy(y).to(DEV).unsqueeze(0))[0].cpu().numpy()
    got = mod.process_clips(bank.clips([1], [5], NUM_FRAMES)).cpu().numpy()[0]
    np.testing.assert_array_equal(got, whole[..., 5:5 + NUM_FRAMES])
    own = mod.process_batch(torch.from_numpy(y[5 * 512:5 * 512 + 32 * 512]).to(DEV).unsqueeze(0))[0].cpu().numpy()
    assert own.shape == got.shape
    gap = np.abs(own[..., 2:31] - whole[..., 5 + 2:5 + 31]).max()
    print(f'clip-own features against the track slices, frames 2 .. 30: {gap:.3f}')
    assert gap > 0.25


def _tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def test_tabcnn_takes_clips_under_key_audio():
    from amt_tools_amd.features import CQT
    from amt_tools_amd.models import TabCNN
    mod = CQT(sample_rate=22050, hop_length=512, n_bins=192, bins_per_octave=24)
    model = TabCNN(192, tools.GuitarProfile(num_frets=19), 1, 1, device=DEV)
    model.load_state_dict(_tensors(synth_tabcnn_state_dict(5, dim_in=192, in_channels=1, model_complexity=1, num_groups=6, num_classes=21)))
    model.frontend = torch.nn.Sequential(mod.frontend())
    model.change_device()
    model.eval()
    tracks = [synth_clip(3, num_samples=60000), synth_clip(9, num_samples=30001)]
    bank = PyramidBank(tracks, mod, DEV)
    ids, firsts, T = [0, 1, 0], [60, 0, 118 - 40], 40
    clips = bank.clips(ids, firsts, T)
    whole = [mod.process_batch(torch.from_numpy(y).to(DEV).unsqueeze(0))[0] for y in tracks]        # (1, F, T_k)
    slices = torch.stack([whole[k][..., f:f + T] for k, f in zip(ids, firsts)]).contiguous()         # (3, 1, F, T)
    audio = torch.from_numpy(np.stack([y[:512 * 39 + 7] for y in (tracks[0], tracks[1], tracks[0])])).to(DEV)

    def outputs(batch):
        with torch.no_grad():
            return {k: v.cpu().numpy() for k, v in model.run_on_batch(batch).items() if torch.is_tensor(v)}
    before = outputs({tools.KEY_AUDIO: audio})
    got, want = outputs({tools.KEY_AUDIO: clips}), outputs({tools.KEY_FEATS: slices})
    assert tools.KEY_TABLATURE in got and sorted(got) == sorted(want)
    for key in got:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)

    # training mode: one labelled step on the clips runs through
    model.train()
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    batch = {tools.KEY_AUDIO: clips, tools.KEY_TABLATURE: torch.from_numpy(rng.integers(-1, 21, (3, 6, T)))}
    loss = model.run_on_batch(batch)[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL]
    loss.backward()
    assert torch.isfinite(loss).item()
    for pname, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all().item(), pname

    # an audio-tensor batch runs exactly as before
    model.eval()
    after = outputs({tools.KEY_AUDIO: audio})
    for key in before:
        np.testing.assert_array_equal(after[key], before[key], err_msg=key)


@pytest.mark.parametrize('precision', ['bf16', 'x3'])
def test_onsets_frames_takes_hcqt_clips_in_the_conv_kernels_format(precision):
    from amt_tools_amd.features import HCQT, MelSpec
    from amt_tools_amd.models import OnsetsFrames, PendingFeatures16
    mod = HCQT(22050, 512, n_bins=72)
    model = OnsetsFrames(72, tools.PianoProfile(), 6, 2, device=DEV, precision=precision)
    model.load_state_dict(_tensors(synth_state_dict(7, dim_in=72, in_channels=6, model_complexity=2)))
    model.frontend = torch.nn.Sequential(mod.frontend())
    model.change_device()
    model.eval()
    tracks = [synth_clip(3, num_samples=60000), synth_clip(9, num_samples=30001)]
    bank = PyramidBank(tracks, mod, DEV)
    ids, firsts, T = [0, 1, 0], [60, 0, 118 - 40], 40
    clips = bank.clips(ids, firsts, T)
    whole = [mod.process_batch(torch.from_numpy(y).to(DEV).unsqueeze(0))[0] for y in tracks]        # (6, F, T_k)
    slices = torch.stack([whole[k][..., f:f + T] for k, f in zip(ids, firsts)]).contiguous()         # (3, 6, F, T)
    with torch.no_grad():
        model.__dict__['_in_run_on_batch'] = True
        try:
            pre = model.pre_proc({tools.KEY_AUDIO: clips})
        finally:
            model.__dict__.pop('_in_run_on_batch')
        pending = pre[tools.KEY_FEATS]
        assert isinstance(pending, PendingFeatures16)
        assert pending.feats16.shape == ((2,) if precision == 'x3' else ()) + (3, T, 72, 8)
        np.testing.assert_array_equal(pending.materialize().cpu().numpy(), slices.transpose(-1, -2).cpu().numpy())
        got = model.run_on_batch({tools.KEY_AUDIO: clips})
        want = model.run_on_batch({tools.KEY_FEATS: slices})
    for key in (tools.KEY_ONSETS, tools.KEY_MULTIPITCH):
        assert got[key].shape == (3, 88, T)
        np.testing.assert_array_equal(got[key].cpu().numpy(), want[key].cpu().numpy())
    # a model over another front-end refuses the pyramid's clips
    other = OnsetsFrames(229, tools.PianoProfile(), 1, 2, device=DEV)
    other.frontend = torch.nn.Sequential(MelSpec(sample_rate=16000, n_mels=229).frontend())
    other.change_device()
    for mode in (other.eval, other.train):
        mode()
        with pytest.raises(TypeError, match='a TrackClips batch needs a model whose frontend is exactly one SpectralFrontend'):
            other.run_on_batch({tools.KEY_AUDIO: clips})


def test_bank_and_clips_do_not_depend_on_memory_contents(monkeypatch):
    """Bank construction (decimations, pads, the maxima launch) + every clip form with every torch.empty allocation filled with 0x00,
    0xFF, 0x7F."""
    from amt_tools_amd.features import CQT, HCQT
    poison = Poison(monkeypatch, 0x00)
    tracks = [synth_clip(40 + i, num_samples=n) for i, n in enumerate(LENGTHS[1:3])]
    for make in (lambda: CQT(22050, 512, n_bins=192, bins_per_octave=24, librosa_version='0.9'), lambda: HCQT(22050, 512, n_bins=72)):
        ref = None
        for pattern in PATTERNS:
            poison.pattern = pattern
            mod = make()
            bank = PyramidBank(tracks, mod, DEV)
            clips = bank.clips([0, 0, 1], [0, 41, 7], 3)
            power, track_max = mod.power_clips(clips)
            got = snapshot({'db_ref': bank.db_ref, 'pyramid': bank.pyramid, 'feats': mod.process_clips(clips),
                            'model_layout': mod.process_clips(clips, model_layout=True), 'feats16': mod.process_clips16(clips).view(torch.int16),
                            'split': mod.process_clips16(clips, split=True).view(torch.int16), 'power': power, 'track_max': track_max})
            if ref is None:
                ref = got
            else:
                assert_same(got, ref, f'fill {pattern:#04x}')
        assert poison.filled > 0 and (ref['db_ref'] > 0).all()


def test_a_plan_outside_the_windowed_kernel_has_no_clip_form():
    """48 bins per octave need 512-tap filters: the whole-track forward computes them on the generic GEMM, which has no clip form."""
    from amt_tools_amd.features import CQT
    mod = CQT(22050, 512, n_bins=96, bins_per_octave=48)
    y = synth_clip(1, num_samples=20000)
    assert mod.process_batch(torch.from_numpy(y).to(DEV).unsqueeze(0)).shape == (1, 1, 96, 40)      # the plan itself works
    bank = PyramidBank([y], mod, DEV)
    with pytest.raises(NotImplementedError, match='no clip form'):
        bank.db_ref
    # and a reflect-padded plan refuses a track whose deepest level is not longer than its pad, naming the track
    short = PyramidBank([synth_clip(1, num_samples=50000), synth_clip(2, num_samples=16000)],
                        CQT(22050, 512, n_bins=192, bins_per_octave=24, librosa_version='0.9'), DEV)
    with pytest.raises(ValueError, match='track 1 .16000 samples.*reflect padding needs a longer track'):
        short.db_ref
