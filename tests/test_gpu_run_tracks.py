"""Whole resident tracks from overlapped clips on the device: amtx_stitch_clips (include/amtx_stitch.h, csrc/stitch.hip) against
tracks.stitch_host bit for bit, into poisoned memory between guard bands; inference.run_tracks against model.run_on_batch on the plan's
clips (the kept columns, exactly) and on whole tracks as one clip; evaluate.validate_tracks against the host evaluators fed with
run_tracks' output and the banks' NumPy references.  Every comparison is equality."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from amt_tools_amd import _lib, autograd, evaluate as ev, tools, transcribe           # noqa: E402
from amt_tools_amd.features import CQT, MelSpec                                        # noqa: E402
from amt_tools_amd.inference import run_tracks                                         # noqa: E402
from amt_tools_amd.synth import synth_clip, synth_state_dict, synth_tabcnn_state_dict  # noqa: E402
from amt_tools_amd.tracks import (LabelBank, NoteBank, PyramidBank, TrackBank, TrackMaps, seam_clips, stitch_clips,   # noqa: E402
                                  stitch_host)
from poison import PATTERNS, fill_storage                                              # noqa: E402

DEV = 'cuda:0'
HOP, SR = 512, 22050
T, MARGIN = 40, 6
ROWS = 5
GUARD = 256                                  # bytes in front of and behind the destination
GUITAR = tools.GuitarProfile(num_frets=19)
DTYPES = {4: (torch.float32, np.float32, np.uint32), 8: (torch.int64, np.int64, np.uint64)}


# ------------------------------------------------------------------------------------------------------------------------------
# the kernel
# ------------------------------------------------------------------------------------------------------------------------------
def _source(elem_bytes, batch, seed):
    """A (batch, ROWS, T) batch tensor of random bit patterns -- float32: NaN payloads and -0.0 among them; int64: -1 among them."""
    rng = np.random.default_rng(seed)
    if elem_bytes == 4:
        bits = rng.integers(0, 2 ** 32, size=(batch, ROWS, T), dtype=np.uint64).astype(np.uint32)
        bits[0, 0, :4] = (0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000)
        return bits.view(np.float32)
    values = rng.integers(-2 ** 62, 2 ** 62, size=(batch, ROWS, T))
    values[:, :, ::7] = -1
    return values


def _arena(elem_bytes, elems, pattern):
    """`elems` destination elements between two guard bands, all of one allocation whose every byte is `pattern`."""
    arena = fill_storage(torch.empty(2 * GUARD + elems * elem_bytes, dtype=torch.uint8, device=DEV), pattern)
    return arena, arena[GUARD:GUARD + elems * elem_bytes].view(DTYPES[elem_bytes][0])


def _bits(elem_bytes, a):
    return np.ascontiguousarray(a).view(DTYPES[elem_bytes][2])


@pytest.mark.parametrize('elem_bytes', [4, 8])
def test_stitch_clips_equals_stitch_host_bit_for_bit_inside_guard_bands(elem_bytes):
    """The plan of the 118-frame track (B = 4) and, in a second call, the 59-frame track's two clips: afterwards every element of both
    tracks holds the expected bits -- no poison is left -- and the bands around the destination are intact."""
    plan = seam_clips([118, 59], T, MARGIN)
    assert plan.track_ids.tolist() == [0, 0, 0, 0, 1, 1]
    maps = TrackMaps([118, 59], DEV)
    maps.add('k', (ROWS,), DTYPES[elem_bytes][0])                                   # for its bookkeeping: the destination is the arena's
    desc = maps.descriptors('k', plan.track_ids, plan.kept)
    elems = 177 * ROWS
    first, second = _source(elem_bytes, 4, 1), _source(elem_bytes, 2, 2)
    for pattern in PATTERNS:
        arena, dst = _arena(elem_bytes, elems, pattern)
        want = np.full(elems, 0, dtype=DTYPES[elem_bytes][1])
        want.view(np.uint8)[:] = pattern
        # after the first call: the 118-frame track is whole, the 59-frame track still poison
        assert stitch_clips(dst, torch.from_numpy(first).to(DEV), desc[:4]) is dst
        stitch_host(want, first, desc[:4])
        assert np.array_equal(_bits(elem_bytes, dst.cpu().numpy()), _bits(elem_bytes, want))
        assert (_bits(elem_bytes, want[118 * ROWS:]).view(np.uint8) == pattern).all()
        stitch_clips(dst, torch.from_numpy(second).to(DEV), desc[4:], torch.from_numpy(desc[4:]).to(DEV))
        stitch_host(want, second, desc[4:])
        got = arena.cpu().numpy()
        assert np.array_equal(got[GUARD:-GUARD].view(DTYPES[elem_bytes][2]), _bits(elem_bytes, want)), hex(pattern)
        assert (got[:GUARD] == pattern).all() and (got[-GUARD:] == pattern).all(), hex(pattern)
        # plain slicing, once more: every frame of both tracks comes from exactly one clip
        for t, (lo, L, src, rows) in enumerate(((0, 118, first, range(4)), (118 * ROWS, 59, second, range(2)))):
            track = _bits(elem_bytes, want[lo:lo + ROWS * L]).reshape(ROWS, L)
            for b, (d, s, c) in zip(rows, plan.kept[plan.track_ids == t]):
                assert np.array_equal(track[:, d:d + c], _bits(elem_bytes, src)[b, :, s:s + c])


@pytest.mark.parametrize('elem_bytes', [4, 8])
def test_one_column_and_a_whole_clip(elem_bytes):
    src = _source(elem_bytes, 1, 3)
    for row in ([ROWS, 50, 49, T - 1, 1], [0, T, 0, 0, T], [2 * ROWS, T + 3, 3, 0, T]):
        elems = row[0] + ROWS * row[1] + 7
        arena, dst = _arena(elem_bytes, elems, 0xFF)
        want = np.empty(elems, dtype=DTYPES[elem_bytes][1])
        want.view(np.uint8)[:] = 0xFF
        stitch_clips(dst, torch.from_numpy(src).to(DEV), [row])
        stitch_host(want, src, [row])
        got = arena.cpu().numpy()
        assert np.array_equal(got[GUARD:-GUARD].view(DTYPES[elem_bytes][2]), _bits(elem_bytes, want)), row
        assert (got[:GUARD] == 0xFF).all() and (got[-GUARD:] == 0xFF).all()
        ones = np.iinfo(DTYPES[elem_bytes][2]).max                           # the named columns and nothing else: what is not all ones any more
        assert (_bits(elem_bytes, want) != ones).sum() == (_bits(elem_bytes, src)[0, :, row[3]:row[3] + row[4]] != ones).sum() > 0


@pytest.mark.parametrize('elem_bytes', [4, 8])
def test_the_entry_point_refuses_a_bad_row_with_nothing_written(elem_bytes):
    src = torch.from_numpy(_source(elem_bytes, 2, 4)).to(DEV)
    elems = 2 * ROWS * 50
    arena, dst = _arena(elem_bytes, elems, 0x7F)
    good = [0, 50, 10, 0, T]
    bad_rows = (([0, 50, 11, 0, T], 'clip 1: frames .* leave the track'), ([0, 50, 0, 1, T], 'clip 1: columns .* leave the clip'),
                ([0, 50, 0, 0, T + 1], 'clip 1: columns .* leave the clip'), ([ROWS * 50 + 1, 50, 0, 0, T], 'clip 1: the track map .* leaves the 500 elements'),
                ([0, 101, 0, 0, T], 'clip 1: the track map'), ([elems + 1, 0, 0, 0, 0], 'clip 1: the track map'),
                ([-1, 50, 0, 0, T], 'clip 1: a negative entry'), ([0, -50, 0, 0, T], 'negative'), ([0, 50, -1, 0, T], 'negative'),
                ([0, 50, 0, -1, T], 'negative'), ([0, 50, 0, 0, -1], 'negative'), ([2 ** 62, 2 ** 62, 0, 0, T], 'clip 1: the track map'))
    for row, text in bad_rows:
        desc = np.array([good, row], dtype=np.int64)
        with pytest.raises(_lib.AmtxError, match=text):
            stitch_clips(dst, src, desc)
    call = lambda *a: _lib.call('amtx_stitch_clips', *a, device=DEV)       # noqa: E731
    desc = np.array([good, good], dtype=np.int64)
    desc_dev = torch.from_numpy(desc).to(DEV)
    for args, text in (((src, 2, 2, ROWS, T, desc, desc_dev, dst, elems), 'elem_bytes=2'), ((src, elem_bytes, 0, ROWS, T, desc, desc_dev, dst, elems), 'batch=0'),
                       ((src, elem_bytes, 2, 0, T, desc, desc_dev, dst, elems), 'rows=0'), ((src, elem_bytes, 2, ROWS, 0, desc, desc_dev, dst, elems), 'num_frames=0'),
                       ((src, elem_bytes, 2, ROWS, T, desc, desc_dev, dst, 0), 'dst_elems=0'), ((src, elem_bytes, 2, ROWS, T, None, desc_dev, dst, elems), 'null argument'),
                       ((src, elem_bytes, 2, ROWS, T, desc, desc_dev, dst.view(torch.uint8)[1:], elems), 'aligned')):
        with pytest.raises(_lib.AmtxError, match=text):
            call(*args)
    assert (arena.cpu().numpy() == 0x7F).all()                              # nothing was written, by any of them
    for bad, kind in ((src.double() if elem_bytes == 4 else src.int(), TypeError), (src[0, 0], ValueError)):
        with pytest.raises(kind):
            stitch_clips(dst, bad, desc)


# ------------------------------------------------------------------------------------------------------------------------------
# run_tracks
# ------------------------------------------------------------------------------------------------------------------------------
def _tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def piano_setup():
    """The recipe of tests/test_gpu_note_clips.py with a fourth track that is shorter than a clip."""
    from amt_tools_amd.models import OnsetsFrames
    mod = MelSpec(sample_rate=SR, hop_length=HOP, n_mels=229, n_fft=2048)
    model = OnsetsFrames(229, tools.PianoProfile(), 1, 2, device=DEV, precision='bf16')
    model.load_state_dict(_tensors(synth_state_dict(0, dim_in=229, in_channels=1, model_complexity=2)))
    model.frontend = torch.nn.Sequential(mod.frontend())
    model.change_device()
    model.eval()
    bank = TrackBank([synth_clip(3, num_samples=60000), synth_clip(9, num_samples=30000), synth_clip(5, num_samples=HOP * T - 1),
                      synth_clip(7, num_samples=HOP * 23 - 1)], mod, DEV)
    assert bank.frame_counts.tolist() == [118, 59, 40, 23]
    return model, bank


@functools.lru_cache(maxsize=None)
def tab_setup():
    from amt_tools_amd.models import TabCNN
    mod = CQT(sample_rate=SR, hop_length=HOP, n_bins=192, bins_per_octave=24)
    model = TabCNN(192, GUITAR, 1, 1, device=DEV)
    model.load_state_dict(_tensors(synth_tabcnn_state_dict(5, dim_in=192, in_channels=1, model_complexity=1, num_groups=6, num_classes=21)))
    model.frontend = torch.nn.Sequential(mod.frontend())
    model.change_device()
    model.eval()
    bank = PyramidBank([synth_clip(3, num_samples=60000), synth_clip(9, num_samples=30001), synth_clip(5, num_samples=HOP * T - 1),
                        synth_clip(7, num_samples=17001)], mod, DEV)
    assert bank.frame_counts.tolist() == [118, 59, 40, 34]
    return model, bank


def _clips_on_host(model, bank, ids, firsts, frames):
    with torch.no_grad():
        preds = model.run_on_batch({tools.KEY_AUDIO: bank.clips(ids, firsts, frames)})
        return {k: v.cpu().numpy().copy() for k, v in preds.items() if torch.is_tensor(v)}


def _whole(model, bank, t):
    """Track t whole, as one clip of its own length: {key: (rows, L_t)}."""
    return {k: v[0] for k, v in _clips_on_host(model, bank, [t], [0], int(bank.frame_counts[t])).items()}


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    view = np.uint32 if got.dtype.itemsize == 4 else np.uint64
    same = np.ascontiguousarray(got).view(view) == np.ascontiguousarray(want).view(view)
    assert same.all(), (what, 'first difference at', tuple(int(i) for i in np.argwhere(~same)[0]), int((~same).sum()), 'of', same.size)


@pytest.mark.parametrize('batch_size', [3, 256])
def test_run_tracks_returns_the_kept_columns_of_run_on_batch_on_the_plans_clips(batch_size):
    model, bank = piano_setup()
    plan = seam_clips(bank.frame_counts, T, MARGIN)
    assert plan.first_frames.tolist() == [0, 28, 56, 78, 0, 19, 0] and plan.short.tolist() == [3]
    # the reference: the plan's clips through run_on_batch in the same batches, the kept columns placed by plain slicing
    want = {}
    for lo in range(0, len(plan.track_ids), batch_size):
        sel = slice(lo, lo + batch_size)
        host = _clips_on_host(model, bank, plan.track_ids[sel], plan.first_frames[sel], T)
        for j, (t, (d, s, c)) in enumerate(zip(plan.track_ids[sel].tolist(), plan.kept[sel].tolist())):
            for key, value in host.items():
                full = want.setdefault(t, {}).setdefault(key, np.full(value.shape[1:-1] + (int(bank.frame_counts[t]),), -7, dtype=value.dtype))
                full[..., d:d + c] = value[j][..., s:s + c]
    want[3] = _whole(model, bank, 3)
    fallbacks = autograd.fallback_total()
    got = run_tracks(bank, model, T, MARGIN, batch_size=batch_size, decode_notes=True)
    assert autograd.fallback_total() == fallbacks
    assert list(got) == [0, 1, 2, 3]
    for t in range(4):
        assert sorted(got[t]) == sorted(list(want[t]) + [tools.KEY_NOTES]) and tools.KEY_ONSETS in got[t] and tools.KEY_MULTIPITCH in got[t]
        for key in want[t]:
            assert got[t][key].shape[-1] == bank.frame_counts[t]
            _same_bits(got[t][key], want[t][key], (t, key))
    # a track that fits one clip is the whole track's own result, in whatever batch its clip ran
    for t in (2, 3):
        for key, value in _whole(model, bank, t).items():
            _same_bits(got[t][key], value, ('whole', t, key))
    # notes: the decoder on the track's stitched maps alone, on the grid of the track's own length
    notes = 0
    for t in range(4):
        preds = {key: torch.from_numpy(got[t][key]).to(DEV).unsqueeze(0) for key in (tools.KEY_ONSETS, tools.KEY_MULTIPITCH)}
        alone = transcribe.decode_notes_for(preds, model, None).result()[0]
        assert np.array_equal(np.asarray(got[t][tools.KEY_NOTES]), np.asarray(alone)) and np.asarray(alone).shape[1:] == (3,)
        notes += len(alone)
    assert notes > 0
    # keep, the request's order and a rank's share
    some = run_tracks(bank, model, T, MARGIN, track_ids=[3, 1, 0], batch_size=batch_size, keep=(tools.KEY_ONSETS,), rank=0, world=2)
    assert list(some) == [3, 0] and all(list(v) == [tools.KEY_ONSETS] for v in some.values())
    for t in some:
        _same_bits(some[t][tools.KEY_ONSETS], got[t][tools.KEY_ONSETS], ('keep', t))
    only_notes = run_tracks(bank, model, T, MARGIN, track_ids=[1], batch_size=batch_size, keep=(), decode_notes=True)
    assert list(only_notes[1]) == [tools.KEY_NOTES] and np.array_equal(only_notes[1][tools.KEY_NOTES], got[1][tools.KEY_NOTES])
    assert run_tracks(bank, model, T, MARGIN, track_ids=[1], rank=1, world=2) == {}


@pytest.mark.parametrize('margin', [4, 7])
def test_tabcnn_from_overlapped_clips_is_the_whole_track(margin):
    """A TabCNN frame sees 9 frames of features: from margin 4 on the stitched tablature is the whole track's, an identity in exact
    arithmetic."""
    model, bank = tab_setup()
    fallbacks = autograd.fallback_total()
    for batch_size in (3, 256):
        got = run_tracks(bank, model, T, margin, batch_size=batch_size, decode_notes=True, keep=(tools.KEY_TABLATURE, tools.KEY_MULTIPITCH))
        for t in range(4):
            whole = _whole(model, bank, t)[tools.KEY_TABLATURE]
            assert sorted(got[t]) == sorted([tools.KEY_TABLATURE, tools.KEY_MULTIPITCH, tools.KEY_NOTES]) and whole.dtype == np.int64
            _same_bits(got[t][tools.KEY_TABLATURE], whole, (margin, batch_size, t))
            times = np.arange(whole.shape[-1]) * HOP / SR
            notes = transcribe._tab_to_stacked_notes_host(whole, times, GUITAR)
            assert list(got[t][tools.KEY_NOTES]) == list(notes)
            for s in notes:
                assert np.array_equal(got[t][tools.KEY_NOTES][s][0], notes[s][0]) and np.array_equal(got[t][tools.KEY_NOTES][s][1], notes[s][1])
            collapsed = tools.stacked_multi_pitch_to_multi_pitch(tools.tablature_to_stacked_multi_pitch(whole, GUITAR))
            assert np.array_equal(got[t][tools.KEY_MULTIPITCH], collapsed)
    # the pitch map alone: the tablature it is expanded from is stitched, and stays on the device
    pitch = run_tracks(bank, model, T, margin, track_ids=[1], keep=(tools.KEY_MULTIPITCH,))
    assert list(pitch[1]) == [tools.KEY_MULTIPITCH] and np.array_equal(pitch[1][tools.KEY_MULTIPITCH], got[1][tools.KEY_MULTIPITCH])
    assert autograd.fallback_total() == fallbacks


# ------------------------------------------------------------------------------------------------------------------------------
# validate_tracks
# ------------------------------------------------------------------------------------------------------------------------------
def piano_combo():
    return ev.ComboEvaluator([ev.MultipitchEvaluator(), ev.NoteEvaluator(), ev.NoteEvaluator(offset_ratio=0.2, results_key='notes-with-offsets')])


@functools.lru_cache(maxsize=None)
def piano_truth():
    """Ground truth as tests/test_gpu_note_clips.py builds it: what the model itself transcribes (here: run_tracks), with a third of the
    notes dropped, a third moved by one hop and random notes added -- every count is away from 0 and from the total."""
    model, bank = piano_setup()
    own = run_tracks(bank, model, T, MARGIN, keep=(), decode_notes=True)
    rng = np.random.default_rng(8)
    truth = []
    for t, n in enumerate(bank.frame_counts):
        rows = np.array(own[t][tools.KEY_NOTES], dtype=np.float64).reshape(-1, 3)
        rows = rows[rng.random(len(rows)) < 0.67]
        rows[:, 0] += (rng.random(len(rows)) < 0.33) * HOP / SR
        rows[:, 1] = np.maximum(rows[:, 1], rows[:, 0])
        onsets = rng.integers(0, n - 1, 12) * HOP / SR
        truth.append(np.concatenate([rows, np.stack([onsets, onsets + rng.integers(1, 30, 12) * HOP / SR, rng.integers(21, 109, 12).astype(np.float64)], axis=1)]))
    return truth


def _piano_banks(bank, truth):
    times = [np.arange(n) * HOP / SR for n in bank.frame_counts]
    labels = LabelBank.from_notes([(t[:, 2], t[:, :2]) for t in truth], times, tools.PianoProfile(), keys=(tools.KEY_MULTIPITCH,), bank=bank)
    return labels, NoteBank(truth, bank=bank)


def _host_scores(make, predictions, labels, notes, note_ref):
    """The host evaluators' process_track on run_tracks' host output, labels.host_map and notes.host_whole, track by track."""
    combo = make()
    for t, est in predictions.items():
        reference = {key: labels.host_map(t, key) for key in labels.keys}
        reference[tools.KEY_NOTES] = note_ref(notes.host_whole([t]))
        combo.process_track(est, reference, t)
    return combo


def _same_per_track(combo, want, tracks):
    for got_e, want_e in zip(combo.evaluators, want.evaluators):
        def same(a, b, path):
            if isinstance(b, dict):
                assert isinstance(a, dict) and list(a) == list(b), path
                for k in b:
                    same(a[k], b[k], path + (k,))
            else:
                assert np.array_equal(np.asarray(a), np.asarray(b)) and np.size(b) == tracks, path
        same(got_e.results, want_e.results, (type(want_e).__name__,))


@pytest.mark.parametrize('batch_size', [3, 256])
def test_validate_tracks_equals_the_host_evaluators_on_onsets_and_frames(batch_size, tmp_path):
    model, bank = piano_setup()
    labels, notes = _piano_banks(bank, piano_truth())
    assert notes.integral and notes.slices == 1
    predictions = run_tracks(bank, model, T, MARGIN, batch_size=batch_size, decode_notes=True)
    want = _host_scores(piano_combo, predictions, labels, notes, lambda groups: groups[0])
    fallbacks = autograd.fallback_total()
    combo = piano_combo()
    combo.set_save_dir(str(tmp_path))
    average = ev.validate_tracks(bank, labels, notes, model, combo, T, MARGIN, batch_size=batch_size)
    assert autograd.fallback_total() == fallbacks
    assert average == want.average_results() and list(average) == [tools.KEY_MULTIPITCH, tools.KEY_NOTES, 'notes-with-offsets']
    _same_per_track(combo, want, 4)
    assert 0 < average[tools.KEY_MULTIPITCH][tools.KEY_F1] < 1
    assert 0 < average[tools.KEY_NOTES][tools.KEY_F1] < 1 and 0 < average['notes-with-offsets'][tools.KEY_F1] < 1
    assert sorted(p.name for p in tmp_path.iterdir()) == [f'{t}.txt' for t in range(4)]
    # a rank's share: positions 1 and 3 of the request
    shard = piano_combo()
    ev.validate_tracks(bank, labels, notes, model, shard, T, MARGIN, batch_size=batch_size, rank=1, world=2)
    for got_e, want_e in zip(shard.evaluators, want.evaluators):
        assert np.array_equal(got_e.results[tools.KEY_F1], np.asarray(want_e.results[tools.KEY_F1])[1::2])
    # the request's order, absolute times (a whole track starts at 0), one evaluator that is no combination
    alone = ev.NoteEvaluator()
    ev.validate_tracks(bank, None, NoteBank(piano_truth(), bank=bank, relative_times=False), model, alone, T, MARGIN, track_ids=[2, 0], batch_size=batch_size)
    assert np.array_equal(alone.results[tools.KEY_F1], np.asarray(want.evaluators[1].results[tools.KEY_F1])[[2, 0]])


def test_a_fractional_reference_pitch_takes_the_host_matcher():
    model, bank = piano_setup()
    truth = [t.copy() for t in piano_truth()]
    truth[1][0, 2] += 0.5
    labels, _ = _piano_banks(bank, [np.concatenate([t[:, :2], np.floor(t[:, 2:])], axis=1) for t in truth])
    notes = NoteBank(truth, bank=bank)
    assert not notes.integral
    predictions = run_tracks(bank, model, T, MARGIN, decode_notes=True)
    want = _host_scores(piano_combo, predictions, labels, notes, lambda groups: groups[0])
    combo = piano_combo()
    average = ev.validate_tracks(bank, labels, notes, model, combo, T, MARGIN, batch_size=3)
    assert average == want.average_results()
    _same_per_track(combo, want, 4)


def test_whole_equals_host_whole_as_a_view_and_as_a_gather():
    _, bank = piano_setup()
    notes = NoteBank(piano_truth(), bank=bank)
    rows_dev = notes._device_state()[0]
    for ids in ([0], [1, 2], [0, 1, 2, 3], [3, 1], [2, 2]):
        got, groups = notes.whole(ids), notes.host_whole(ids)
        rows = np.concatenate(groups)
        assert got.offsets.dtype == torch.int32 and got.total == len(rows) and got.slices == 1 and got.keys is None
        assert np.array_equal(got.offsets.cpu().numpy(), np.concatenate(([0], np.cumsum([len(g) for g in groups]))))
        assert np.array_equal(got.rows.cpu().numpy().view(np.uint64), rows.view(np.uint64))
        consecutive = ids in ([0], [1, 2], [0, 1, 2, 3])
        assert (got.rows.untyped_storage().data_ptr() == rows_dev.untyped_storage().data_ptr()) == consecutive
    empty = NoteBank([np.zeros((0, 3)), np.array([[0.0, 0.0, 60.0]])], relative_times=False)
    got = empty.whole([0])
    assert got.total == 0 and got.offsets.tolist() == [0, 0] and got.rows.shape == (1, 3)
    assert empty.whole([1]).rows.cpu().numpy().tolist() == [[0.0, 0.0, 60.0]]             # offset == 0: kept


def test_validate_tracks_equals_the_host_evaluators_on_tabcnn():
    model, bank = tab_setup()
    # ground truth: the model's own whole-track tablature with half of its cells redrawn
    rng = np.random.default_rng(50)
    own = run_tracks(bank, model, T, 4, decode_notes=True)
    tabs = []
    for t, n in enumerate(bank.frame_counts.tolist()):
        redrawn = np.repeat(rng.integers(-1, 20, size=(6, n // 4 + 1)), 4, axis=-1)[:, :n]
        tabs.append(np.where(rng.random((6, n)) < 0.5, own[t][tools.KEY_TABLATURE], redrawn))
    stacked = [transcribe._tab_to_stacked_notes_host(tab, np.arange(tab.shape[1]) * HOP / SR, GUITAR) for tab in tabs]
    labels = LabelBank([{tools.KEY_TABLATURE: tab} for tab in tabs], bank=bank)
    notes = NoteBank(stacked, bank=bank)
    assert notes.slices == 6 and notes.integral and len(notes.rows) > 20
    make = lambda: ev.ComboEvaluator([ev.TablatureEvaluator(GUITAR), ev.StackedNoteEvaluator(offset_ratio=0.2),       # noqa: E731
                                      ev.StackedNoteEvaluator(average_slices=True, results_key='notes-avg')])
    want = _host_scores(make, own, labels, notes, lambda groups: {key: (g[:, 2], g[:, :2]) for key, g in zip(notes.keys, groups)})
    fallbacks = autograd.fallback_total()
    for batch_size in (3, 256):
        combo = make()
        average = ev.validate_tracks(bank, labels, notes, model, combo, T, 4, batch_size=batch_size)
        assert average == want.average_results()
        _same_per_track(combo, want, 4)
        assert 0 < average[tools.KEY_TABLATURE][tools.KEY_F1] < 1 and list(average[tools.KEY_NOTES]) == list(range(6))
    assert autograd.fallback_total() == fallbacks
