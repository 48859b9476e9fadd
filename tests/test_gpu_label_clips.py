"""Label clips cut from the run-length encoded label maps of resident tracks (include/amtx_labels.h, amt_tools_amd/tracks.py LabelBank /
ClipLoader) on the GPU.

The acceptance criterion is an identity: a clip's labels are the columns [first_frame, first_frame + T) of the track's own maps, so the
reference is plain NumPy slicing of the host maps and every comparison is assert_array_equal -- on the uint32 view for floating maps (NaN
and -0.0 are in play), on the values for integer maps.  No tolerance anywhere.

Shared set-up: four tracks of 97, 1, 64 and 130 frames with a floating key of 5 rows and an integer key of 3 rows (key-major offsets that
are not trivial); rows that are all zero, constant, alternating every frame, of seeded random run lengths, and of special values (0.25,
-0.0, NaN; -1, 20, 2^31 - 1, -2^31).  A second bank holds the realistic 3 x 88 floating keys of the piano recipe."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from amt_tools_amd import _lib, autograd, cache, tools                                 # noqa: E402
from amt_tools_amd.synth import synth_clip, synth_state_dict, synth_tabcnn_state_dict  # noqa: E402
from amt_tools_amd.tracks import ClipLoader, LabelBank, PyramidBank, TrackBank, draw_clips   # noqa: E402
from poison import PATTERNS, Poison, snapshot                                          # noqa: E402

DEV = 'cuda:0'
WIDTHS = (97, 1, 64, 130)
I32 = np.iinfo(np.int32)


def _random_runs(rng, T, values):
    """A row of T frames in runs of random lengths 1 .. 9, each run one of `values` (neighbours may repeat: encode_rows merges them)."""
    row = np.concatenate([np.full(int(rng.integers(1, 10)), values[int(rng.integers(len(values)))]) for _ in range(T)])
    return row[:T]


def _float_rows(rng, T):
    special = np.array([0.25, -0.0, np.nan, 0.0, 1.0], dtype=np.float32)
    return np.stack([np.zeros(T, dtype=np.float32), np.full(T, 1.0, dtype=np.float32), (np.arange(T) % 2).astype(np.float32),
                     _random_runs(rng, T, np.array([0.0, 1.0], dtype=np.float32)), _random_runs(rng, T, special)])


def _int_rows(rng, T):
    special = np.array([-1, 20, I32.max, I32.min, 0], dtype=np.int64)
    return np.stack([np.where(np.arange(T) % 2, 20, -1).astype(np.int64), _random_runs(rng, T, np.arange(-1, 21)), _random_runs(rng, T, special)])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _want(maps, key, ids, firsts, T):
    """The reference: NumPy slices of the host maps, (B, rows, T), float32 or int64 as clips() returns them."""
    a = np.stack([maps[i][key][:, f:f + T] for i, f in zip(ids, firsts)])
    return a.astype(np.float32) if a.dtype.kind == 'f' else a.astype(np.int64)


def _check(bank, maps, ids, firsts, T, what=''):
    got = bank.clips(ids, firsts, T)
    assert sorted(got) == sorted(maps[0])
    for key, t in got.items():
        want = _want(maps, key, ids, firsts, T)
        assert t.is_cuda and t.is_contiguous() and tuple(t.shape) == want.shape, (what, key)
        assert t.dtype == (torch.float32 if want.dtype == np.float32 else torch.int64), (what, key)
        np.testing.assert_array_equal(_bits(t.cpu().numpy()), _bits(want), err_msg=f'{what} {key}: tracks {list(ids)}, first frames {list(firsts)}')
    return got


@functools.lru_cache(maxsize=None)
def _small():
    rng = np.random.default_rng(7)
    maps = [{'f5': _float_rows(rng, T), 'i3': _int_rows(rng, T)} for T in WIDTHS]
    for entry in maps:
        for a in entry.values():
            a.setflags(write=False)
    return maps, LabelBank(maps, device=DEV)


@functools.lru_cache(maxsize=None)
def _piano():
    """Two tracks of 64 and 130 frames with the piano recipe's three 88-row keys, from synthetic notes through cache.notes_to_*."""
    profile = tools.PianoProfile()
    rng = np.random.default_rng(11)
    notes, times = [], []
    for T in (64, 130):
        grid = np.arange(T) * 512 / 16000.0
        onsets = rng.uniform(0.0, grid[-1], 60)
        notes.append((rng.integers(21, 109, 60).astype(np.float64), np.stack([onsets, onsets + rng.uniform(0.03, 1.0, 60)], axis=1)))
        times.append(grid)
    maps = [{tools.KEY_MULTIPITCH: cache.notes_to_multi_pitch(p, i, t, profile), tools.KEY_ONSETS: cache.notes_to_onsets(p, i, t, profile),
             tools.KEY_OFFSETS: cache.notes_to_offsets(p, i, t, profile)} for (p, i), t in zip(notes, times)]
    return maps, LabelBank.from_notes(notes, times, profile, device=DEV)


def _places(T):
    """Every (track, first frame) of a clip of T frames over the tracks that have them: first frames 0, a middle frame and frame_count - T
    (the 1-frame track only at T = 1)."""
    return [(k, f) for k, n in enumerate(WIDTHS) if n >= T for f in sorted({0, (n - T) // 2, n - T})]


@pytest.mark.parametrize('T', [1, 37, 64, 65, 130])
def test_clips_are_the_columns_of_the_host_maps(T):
    maps, bank = _small()
    places = _places(T)
    for k, f in places:                                                   # B = 1: every (track, first frame) on its own
        _check(bank, maps, [k], [f], T, 'B=1')
    batch = [places[(2 * j + 1) % len(places)] for j in range(5)]             # B = 5: tracks and positions mixed, some track more than once
    assert len({k for k, _ in batch}) < 5
    _check(bank, maps, [k for k, _ in batch], [f for _, f in batch], T, 'B=5')
    if T == 130:                                                          # the realistic keys on the 130-frame track, and a shorter clip of it
        pmaps, pbank = _piano()
        assert pbank.rows_total == 264 and not pbank.int_keys
        _check(pbank, pmaps, [1], [0], 130, 'piano')
        _check(pbank, pmaps, [1, 0, 1, 1, 0], [0, 27, 93, 40, 0], 37, 'piano B=5')


def test_layout_is_what_the_loss_kernels_take_without_a_copy():
    maps, bank = _small()
    B, T = 5, 37
    got = bank.clips([0, 3, 2, 0, 3], [0, 93, 27, 60, 5], T)
    f5, i3 = got['f5'], got['i3']
    assert f5.dtype == torch.float32 and tuple(f5.shape) == (B, 5, T) and i3.dtype == torch.int64 and tuple(i3.shape) == (B, 3, T)
    # autograd.py: BCELogitsLossFunction's `.contiguous().float()` and SoftmaxGroupsLossFunction's `.to(int64).contiguous()` are no-ops
    assert f5.detach().contiguous().float().data_ptr() == f5.data_ptr() and f5.is_contiguous()
    assert i3.detach().to(device=i3.device, dtype=torch.int64).contiguous().data_ptr() == i3.data_ptr() and i3.is_contiguous()
    # key-major views into one allocation per dtype kind
    _, pbank = _piano()
    p = pbank.clips([1, 0], [3, 0], 33)
    base = p[tools.KEY_MULTIPITCH].data_ptr()
    assert [p[k].data_ptr() - base for k in pbank.keys] == [0, 88 * 2 * 33 * 4, 2 * 88 * 2 * 33 * 4]
    assert all(p[k].is_contiguous() and tuple(p[k].shape) == (2, 88, 33) for k in pbank.keys)


def _sweep_rows(kind):
    """A 67-frame track: an alternating row, a random row, and rows whose only change is at frame f, for f in {1, 2, 3, 63, 64, 65, 66}."""
    rng = np.random.default_rng(3)
    rows = [np.arange(67) % 2, _random_runs(rng, 67, np.array([0, 1]))] + [(np.arange(67) >= f).astype(np.int64) for f in (1, 2, 3, 63, 64, 65, 66)]
    return np.stack(rows).astype(np.float32 if kind == 'f' else np.int64)


def test_every_first_frame_of_a_short_clip_against_every_run_boundary():
    """T = 3, first frames 0 .. 64 in one batch of 65: a run boundary falls on f0, f0 + 1, f0 + T - 1 and f0 + T for some clip."""
    maps = [{'f': _sweep_rows('f'), 'i': _sweep_rows('i') * 21 - 1}]
    bank = LabelBank(maps, device=DEV)
    assert bank.frame_counts.tolist() == [67]
    _check(bank, maps, [0] * 65, list(range(65)), 3, 'sweep')


@pytest.mark.parametrize('T', [1024, 1025, 1100])
def test_a_window_of_more_runs_than_a_wave_stages_is_searched_in_memory(T):
    """The kernel stages up to 1024 first frames of a clip's window per wave; an alternating row has one run per frame, so T = 1024 fills
    the staging area and T = 1025 and 1100 take the path that searches the run table in memory.  The other rows stay staged."""
    rng = np.random.default_rng(5)
    n = 1500
    maps = [{'f': np.stack([(np.arange(n) % 2).astype(np.float32), _random_runs(rng, n, np.array([0.0, 1.0, np.nan], dtype=np.float32)),
                            np.zeros(n, dtype=np.float32)]),
             'i': np.stack([np.arange(n) % 22 - 1, _random_runs(rng, n, np.arange(-1, 21))]).astype(np.int64)}]
    bank = LabelBank(maps, device=DEV)
    assert bank.runs_per_track.tolist() == [len(bank.run_first)] and len(bank.run_first) > 3000
    _check(bank, maps, [0, 0, 0], [0, 173, n - T], T, 'long window')


def test_every_element_is_written_whatever_the_memory_held(monkeypatch):
    maps, bank = _small()
    ids, firsts, T = [0, 3, 2, 0, 3], [0, 93, 27, 60, 5], 37
    poison = Poison(monkeypatch, 0x00)
    ref = None
    for pattern in PATTERNS:
        poison.pattern = pattern
        got = snapshot({k: (v.view(torch.int32) if v.dtype == torch.float32 else v) for k, v in bank.clips(ids, firsts, T).items()})
        if ref is None:
            ref = got
        else:
            assert ref['f5'].tobytes() == got['f5'].tobytes() and ref['i3'].tobytes() == got['i3'].tobytes(), f'fill {pattern:#04x}'
    assert poison.filled > 0
    np.testing.assert_array_equal(ref['f5'].view(np.uint32), _bits(_want(maps, 'f5', ids, firsts, T)))
    np.testing.assert_array_equal(ref['i3'], _want(maps, 'i3', ids, firsts, T))


@pytest.mark.parametrize('kind', ['float', 'int'])
def test_nothing_outside_the_output_is_written(kind):
    """The output group of one launch inside a larger 0xFF-filled tensor, 64 elements in from each end (an odd T: rows 4-byte aligned)."""
    maps, bank = _small()
    ids, firsts, T = [0, 3, 2, 0, 3], [0, 93, 27, 60, 5], 37
    B = len(ids)
    row_ptr, run_first, run_bits = bank._device_state()
    desc = torch.tensor([[k, f, T] for k, f in zip(ids, firsts)], dtype=torch.int64, device=DEV)
    dtype, key, rows, row_lo, out_kind = (torch.float32, 'f5', 5, 0, 0) if kind == 'float' else (torch.int64, 'i3', 3, 5, 1)
    frame = torch.empty((64 + rows * B * T + 64,), dtype=dtype, device=DEV)
    frame.view(torch.uint8).fill_(0xFF)
    out = frame[64:64 + rows * B * T]
    _lib.call('amtx_label_clips', row_ptr, run_first, run_bits, len(bank), bank.rows_total, row_lo, row_lo + rows,
              np.array([row_lo, row_lo + rows], dtype=np.int64), 1, desc, B, T, out, out_kind, device=DEV)
    torch.cuda.synchronize()
    edges = torch.cat([frame[:64], frame[-64:]]).view(torch.uint8).cpu().numpy()
    assert (edges == 0xFF).all()
    np.testing.assert_array_equal(_bits(out.view(B, rows, T).cpu().numpy()), _bits(_want(maps, key, ids, firsts, T)))


def test_two_calls_give_the_same_bits():
    maps, bank = _small()
    args = ([3, 0, 3, 2, 0], [93, 11, 0, 27, 60], 37)
    a, b = snapshot(bank.clips(*args)), snapshot(bank.clips(*args))
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key


# ------------------------------------------------------------------------------------------------------------------------------
# through the loader and the models
# ------------------------------------------------------------------------------------------------------------------------------
def _tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _loader_batch_and_its_host_twin(bank, labels, maps, T, seed):
    """(batch A from ClipLoader, batch B: the same clips with the labels sliced on the host and uploaded)."""
    loader = ClipLoader(bank, labels, num_frames=T, batch_size=len(bank), seed=seed)
    assert len(loader) == 1
    (a,) = list(loader)
    rng = np.random.RandomState(seed)
    ids = rng.permutation(len(bank))
    firsts = draw_clips(rng, bank.lengths, bank.module.hop_length, T, ids)
    b = {tools.KEY_AUDIO: bank.clips(ids, firsts, T)}
    np.testing.assert_array_equal(a[tools.KEY_AUDIO].desc, b[tools.KEY_AUDIO].desc)
    for key in maps[0]:
        b[key] = torch.from_numpy(_want(maps, key, ids, firsts, T)).to(DEV)
        np.testing.assert_array_equal(_bits(a[key].cpu().numpy()), _bits(b[key].cpu().numpy()))
    return a, b


def _losses_are_bit_equal(model, a, b):
    before = autograd.fallback_total()
    losses = []
    for batch in (a, b):
        torch.manual_seed(1234)
        loss = model.run_on_batch(batch)[tools.KEY_LOSS]
        losses.append({k: v.detach().cpu().numpy().copy() for k, v in loss.items()})
    assert autograd.fallback_total() == before, autograd.fallbacks()
    assert sorted(losses[0]) == sorted(losses[1]) and tools.KEY_LOSS_TOTAL in losses[0]
    for k in losses[0]:
        assert np.isfinite(losses[0][k]).all() and losses[0][k].tobytes() == losses[1][k].tobytes(), (k, losses[0][k], losses[1][k])
    return losses[0]


def test_onsets_frames2_trains_on_a_loader_batch_as_on_host_labels():
    from amt_tools_amd.features import MelSpec
    from amt_tools_amd.models import OnsetsFrames2
    mod = MelSpec(sample_rate=16000, hop_length=512, n_mels=229, n_fft=2048)
    model = OnsetsFrames2(229, tools.PianoProfile(), 1, 2, device=DEV)
    model.load_state_dict(_tensors(synth_state_dict(31, dim_in=229, in_channels=1, model_complexity=2, offsets=True)))
    model.frontend = torch.nn.Sequential(mod.frontend())
    model.change_device()
    model.train()
    tracks = [synth_clip(3, num_samples=60000), synth_clip(9, num_samples=30000), synth_clip(5, num_samples=20001)]
    bank = TrackBank(tracks, mod, DEV)
    profile, rng = tools.PianoProfile(), np.random.default_rng(2)
    notes, times = [], []
    for n in bank.frame_counts:
        grid = np.arange(n) * 512 / 16000.0
        onsets = rng.uniform(0.0, grid[-1], 40)
        notes.append((rng.integers(21, 109, 40).astype(np.float64), np.stack([onsets, onsets + rng.uniform(0.03, 1.0, 40)], axis=1)))
        times.append(grid)
    labels = LabelBank.from_notes(notes, times, profile, bank=bank)
    maps = [{tools.KEY_MULTIPITCH: cache.notes_to_multi_pitch(p, i, t, profile), tools.KEY_ONSETS: cache.notes_to_onsets(p, i, t, profile),
             tools.KEY_OFFSETS: cache.notes_to_offsets(p, i, t, profile)} for (p, i), t in zip(notes, times)]
    a, b = _loader_batch_and_its_host_twin(bank, labels, maps, 24, seed=3)
    assert sorted(a) == sorted([tools.KEY_AUDIO, tools.KEY_MULTIPITCH, tools.KEY_ONSETS, tools.KEY_OFFSETS]) and a[tools.KEY_ONSETS].sum().item() > 0
    losses = _losses_are_bit_equal(model, a, b)
    assert 'loss_offsets' in losses


def test_tabcnn_trains_on_a_loader_batch_as_on_host_labels():
    from amt_tools_amd.features import CQT
    from amt_tools_amd.models import TabCNN
    mod = CQT(sample_rate=22050, hop_length=512, n_bins=192, bins_per_octave=24)
    model = TabCNN(192, tools.GuitarProfile(num_frets=19), 1, 1, device=DEV)
    model.load_state_dict(_tensors(synth_tabcnn_state_dict(5, dim_in=192, in_channels=1, model_complexity=1, num_groups=6, num_classes=21)))
    model.frontend = torch.nn.Sequential(mod.frontend())
    model.change_device()
    model.train()
    tracks = [synth_clip(3, num_samples=60000), synth_clip(9, num_samples=30001)]
    bank = PyramidBank(tracks, mod, DEV)
    rng = np.random.default_rng(4)
    maps = [{tools.KEY_TABLATURE: np.stack([_random_runs(rng, int(n), np.arange(-1, 20)) for _ in range(6)]).astype(np.int64),
             tools.KEY_MULTIPITCH: np.stack([_random_runs(rng, int(n), np.array([0.0, 0.0, 1.0])) for _ in range(44)])} for n in bank.frame_counts]
    labels = LabelBank(maps, bank=bank)
    a, b = _loader_batch_and_its_host_twin(bank, labels, maps, 40, seed=1)
    assert a[tools.KEY_TABLATURE].dtype == torch.int64 and tuple(a[tools.KEY_TABLATURE].shape) == (2, 6, 40)
    assert a[tools.KEY_MULTIPITCH].dtype == torch.float32 and tuple(a[tools.KEY_MULTIPITCH].shape) == (2, 44, 40)
    _losses_are_bit_equal(model, a, b)
