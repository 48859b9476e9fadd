"""The note ground truth of clips on the device (include/amtx_noteclips.h, csrc/noteclips.hip, tracks.NoteBank) against the bank's NumPy
restatement, bit for bit -- also from poisoned memory, inside 0xFF guard bands and into a buffer that is too small --, and
evaluate.validate_clips end to end against the host evaluators fed with the same predictions and NumPy-sliced references.  Every
comparison is equality."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from amt_tools_amd import _lib, autograd, evaluate as ev, tools, transcribe           # noqa: E402
from amt_tools_amd.features import CQT, MelSpec                                        # noqa: E402
from amt_tools_amd.inference import BankClips, _batched, run_offline_batched           # noqa: E402
from amt_tools_amd.synth import synth_clip, synth_state_dict, synth_tabcnn_state_dict  # noqa: E402
from amt_tools_amd.tracks import LabelBank, NoteBank, PyramidBank, TrackBank, cover_clips   # noqa: E402
from poison import PATTERNS, Poison                                                    # noqa: E402

DEV = 'cuda:0'
HOP, SR = 512, 22050
SIZES = (0, 1, 63, 64, 65, 129, 300)          # notes per group: survivors straddle every 64-row chunk edge
FRAMES = 400
GUITAR = tools.GuitarProfile(num_frets=19)


class _Grid(object):
    """What NoteBank reads of an audio bank: SIZES-many tracks of FRAMES frames under a MelSpec's frame bookkeeping (host code only)."""
    frame_counts = np.full(len(SIZES), FRAMES)
    device = DEV
    module = MelSpec(sample_rate=SR, hop_length=HOP, n_mels=229, n_fft=2048)

    def __len__(self):
        return len(SIZES)


def _group(rng, n):
    """n notes with onsets, offsets exactly on the k * hop / sample_rate grid (strict and non-strict comparisons both meet equality)."""
    on = rng.integers(0, FRAMES - 1, n)
    off = np.minimum(on + rng.integers(0, 120, n), FRAMES)
    return np.stack([on * HOP / SR, off * HOP / SR, rng.integers(40, 77, n).astype(np.float64)], axis=1)


@functools.lru_cache(maxsize=None)
def grid_bank(slices, relative=True):
    rng = np.random.default_rng(10 + slices)
    if slices == 1:
        notes = [_group(rng, n) for n in SIZES]
    else:                                       # string s of track i holds SIZES[(i + s) % 7] notes
        notes = []
        for i in range(len(SIZES)):
            groups = [_group(rng, SIZES[(i + s) % len(SIZES)]) for s in range(slices)]
            notes.append({s: (g[:, 2], g[:, :2]) for s, g in enumerate(groups)})
    return NoteBank(notes, bank=_Grid(), relative_times=relative)


def request(batch, T):
    """`batch` clips of T frames: the tracks in turn, first frames spread over the track (0 and the last possible one among them)."""
    ids = np.arange(batch) % len(SIZES)
    firsts = (np.arange(batch) * 37) % (FRAMES - T + 1)
    if batch > 1:
        firsts[-1] = FRAMES - T
    return ids, firsts, T


def host_pair(bank, req):
    groups = bank.host_clips(*req)
    offsets = np.concatenate(([0], np.cumsum([len(g) for g in groups]))).astype(np.int32)
    return np.concatenate(groups + [np.zeros((0, 3))], axis=0), offsets


def assert_equals_host(bank, req, got, what):
    rows, offsets = host_pair(bank, req)
    assert got.offsets.dtype == torch.int32 and got.rows.dtype == torch.float64 and got.slices == bank.slices and got.keys == bank.keys
    assert np.array_equal(got.offsets.cpu().numpy(), offsets), what
    assert got.total == len(rows) and got.rows.shape == (max(len(rows), 1), 3)
    assert np.array_equal(got.rows.cpu().numpy()[:len(rows)].view(np.uint64), rows.view(np.uint64)), what
    return len(rows)


@pytest.mark.parametrize('relative', [True, False])
@pytest.mark.parametrize('slices', [1, 6])
def test_clips_equal_the_host_restatement_bit_for_bit(slices, relative):
    bank = grid_bank(slices, relative)
    assert sorted(np.diff(bank.group_ptr)[:7 if slices == 1 else None].tolist())[-1] == 300
    kept = 0
    for batch in (1, 5, 65):
        for T in (1, 40, 397):
            kept += assert_equals_host(bank, request(batch, T), bank.clips(*request(batch, T)), (batch, T))
    assert kept > 5000
    # every track on its own, whole: all of its notes survive (all end after time 0 or are dropped for offset == 0 by the rule)
    for track in range(len(SIZES)):
        assert_equals_host(bank, ([track], [0], FRAMES), bank.clips([track], [0], FRAMES), track)


def raw_call(bank, req, capacity, fill, spare_rows=0):
    """amtx_note_clips into views of ONE allocation filled with `fill`: 256 guard bytes in front of and behind rows_out (capacity +
    spare_rows rows, of which the call may write `capacity`), offsets and the workspace.  Returns (rows, offsets, the bytes the call must
    not have touched)."""
    ids, windows = bank._request(*req)
    rows_dev, group_ptr = bank._device_state()
    batch, groups = len(ids), len(ids) * bank.slices
    ws_bytes = int(_lib.call('amtx_note_clips_workspace_bytes', batch, bank.slices))
    assert ws_bytes == 4 * groups
    pad = lambda n: -(-n // 256) * 256          # noqa: E731
    sizes = [(capacity + spare_rows) * 24, (groups + 1) * 4, ws_bytes]
    starts = np.cumsum([256] + [pad(n) + 256 for n in sizes])
    arena = torch.full((int(starts[-1]),), fill, dtype=torch.uint8, device=DEV)
    rows_out, offsets, ws = (arena[int(s):int(s) + n] for s, n in zip(starts, sizes))
    _lib.call('amtx_note_clips', rows_dev, group_ptr, len(bank), bank.slices, torch.from_numpy(ids).to(DEV), torch.from_numpy(windows).to(DEV),
              batch, int(bank.relative_times), rows_out, capacity, offsets, ws, ws_bytes, device=DEV)
    host = arena.cpu().numpy()
    untouched = np.ones(len(host), dtype=bool)
    for s, n in zip(starts[:2], (capacity * 24, sizes[1])):
        untouched[int(s):int(s) + n] = False
    untouched[int(starts[2]):int(starts[2]) + ws_bytes] = False
    return (host[int(starts[0]):int(starts[0]) + sizes[0]].view(np.float64).reshape(-1, 3), host[int(starts[1]):int(starts[1]) + sizes[1]].view(np.int32),
            host[untouched])


@pytest.mark.parametrize('slices', [1, 6])
def test_same_bits_from_poisoned_memory_and_inside_guard_bands(slices, monkeypatch):
    bank = grid_bank(slices)
    req = request(65, 40)
    want_rows, want_offsets = host_pair(bank, req)
    total = len(want_rows)
    assert total > 1000
    for fill in PATTERNS:
        rows, offsets, rest = raw_call(bank, req, total, fill)
        assert np.array_equal(offsets, want_offsets) and np.array_equal(rows.view(np.uint64), want_rows.view(np.uint64)), hex(fill)
        assert (rest == fill).all(), hex(fill)                       # nothing else was written, the 0xFF bands among it
    poison = Poison(monkeypatch, 0x00)
    for fill in PATTERNS:                                            # the allocations of NoteBank.clips itself
        poison.pattern = fill
        before = poison.filled
        assert_equals_host(bank, req, bank.clips(*req), hex(fill))
        assert poison.filled >= before + 3                           # rows_out, offsets, the workspace
    again = bank.clips(*req), bank.clips(*req)                       # two calls: the same bits
    assert torch.equal(again[0].rows.view(torch.int64), again[1].rows.view(torch.int64)) and torch.equal(again[0].offsets, again[1].offsets)


@pytest.mark.parametrize('slices', [1, 6])
def test_a_buffer_one_row_short_reports_the_total_and_the_retry_is_whole(slices):
    bank = grid_bank(slices)
    req = request(5, 397)
    want_rows, want_offsets = host_pair(bank, req)
    total = len(want_rows)
    rows, offsets, rest = raw_call(bank, req, total - 1, 0xFF, spare_rows=1)
    assert offsets[-1] == total and np.array_equal(offsets, want_offsets)
    assert np.array_equal(rows[:total - 1].view(np.uint64), want_rows[:total - 1].view(np.uint64))
    assert (rows[total - 1:].view(np.uint8) == 0xFF).all() and (rest == 0xFF).all()       # the row past the capacity is not written
    short = bank.clips(*req, rows_capacity=total - 1)
    assert short.total is None and int(short.offsets[-1]) == total > short.rows.shape[0]
    retry = bank.clips(*req, rows_capacity=int(short.offsets[-1]))
    assert np.array_equal(retry.rows.cpu().numpy().view(np.uint64), want_rows.view(np.uint64)) and np.array_equal(retry.offsets.cpu().numpy(), want_offsets)


def test_the_entry_point_refuses_bad_sizes():
    bank = grid_bank(1)
    rows_dev, group_ptr = bank._device_state()
    buf = torch.zeros(64, dtype=torch.float64, device=DEV)
    args = lambda batch, slices, cap, ws_bytes: (rows_dev, group_ptr, 7, slices, buf, buf, batch, 1, buf, cap, buf, buf, ws_bytes)     # noqa: E731
    for bad, text in ((args(0, 1, 4, 64), 'batch=0'), (args(2, 0, 4, 64), 'slices=0'), (args(2, 1, 0, 64), 'rows_capacity=0'),
                      (args(2, 1, 4, 4), 'workspace of 4 bytes, 8 needed')):
        with pytest.raises(_lib.AmtxError, match=text):
            _lib.call('amtx_note_clips', *bad, device=DEV)
    assert _lib.call('amtx_note_clips_workspace_bytes', 0, 1) == 0 and _lib.call('amtx_note_clips_workspace_bytes', 65, 6) == 65 * 6 * 4


# ------------------------------------------------------------------------------------------------------------------------------
# validate_clips end to end
# ------------------------------------------------------------------------------------------------------------------------------
T = 40


def _tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _requests(bank):
    """The clips that cover every track, and three more at first frames that are no multiple of the clip."""
    ids, firsts, _ = cover_clips(bank.frame_counts, T)
    return np.concatenate([ids, [0, 0, 1]]), np.concatenate([firsts, [17, int(bank.frame_counts[0]) - T, 19]])


def _predictions(model, bank, ids, firsts):
    """run_on_batch on the bank's clips, brought to the host: one predictions dictionary per clip, notes decoded as the drivers do."""
    with torch.no_grad():
        preds = model.run_on_batch({tools.KEY_AUDIO: bank.clips(ids, firsts, T)})
        notes = transcribe.decode_notes_for(preds, model, None).result()
    host = tools.dict_to_array(preds)
    return [dict({k: v[j] for k, v in host.items() if isinstance(v, np.ndarray)}, **{tools.KEY_NOTES: notes[j]}) for j in range(len(ids))]


def _same_per_clip(combo, want, clips):
    for got_e, want_e in zip(combo.evaluators, want.evaluators):
        def same(a, b, path):
            if isinstance(b, dict):
                assert isinstance(a, dict) and list(a) == list(b), path
                for k in b:
                    same(a[k], b[k], path + (k,))
            else:
                assert np.array_equal(np.asarray(a), np.asarray(b)) and np.size(b) == clips, path
        same(got_e.results, want_e.results, (type(want_e).__name__,))


@functools.lru_cache(maxsize=None)
def piano_setup():
    from amt_tools_amd.models import OnsetsFrames
    mod = MelSpec(sample_rate=SR, hop_length=HOP, n_mels=229, n_fft=2048)
    model = OnsetsFrames(229, tools.PianoProfile(), 1, 2, device=DEV, precision='bf16')
    model.load_state_dict(_tensors(synth_state_dict(0, dim_in=229, in_channels=1, model_complexity=2)))
    model.frontend = torch.nn.Sequential(mod.frontend())
    model.change_device()
    model.eval()
    bank = TrackBank([synth_clip(3, num_samples=60000), synth_clip(9, num_samples=30000), synth_clip(5, num_samples=HOP * T - 1)], mod, DEV)
    assert bank.frame_counts.tolist() == [118, 59, 40]
    # ground truth: what the model itself transcribes from the covering clips, at absolute times, with a third of the notes dropped, a
    # third moved by one hop and random notes added: every count is away from 0 and from the total
    ids, firsts, left_out = cover_clips(bank.frame_counts, T)
    assert ids.tolist() == [0, 0, 1, 2] and left_out == 38 + 19
    rng = np.random.default_rng(8)
    truth = [[] for _ in range(len(bank))]
    for k, f, est in zip(ids, firsts, _predictions(model, bank, ids, firsts)):
        rows = np.array(est[tools.KEY_NOTES], dtype=np.float64).reshape(-1, 3)
        rows = rows[rng.random(len(rows)) < 0.67]
        rows[:, :2] += f * HOP / SR
        rows[:, 0] += (rng.random(len(rows)) < 0.33) * HOP / SR
        rows[:, 1] = np.maximum(rows[:, 1], rows[:, 0])
        truth[k].append(rows)
    for k, n in enumerate(bank.frame_counts):
        onsets = rng.integers(0, n - 1, 12) * HOP / SR
        truth[k].append(np.stack([onsets, onsets + rng.integers(1, 30, 12) * HOP / SR, rng.integers(21, 109, 12).astype(np.float64)], axis=1))
    truth = [np.concatenate(t, axis=0) for t in truth]
    return model, bank, truth


def piano_combo():
    return ev.ComboEvaluator([ev.MultipitchEvaluator(), ev.NoteEvaluator(), ev.NoteEvaluator(offset_ratio=0.2, results_key='notes-with-offsets')])


def _piano_banks(bank, truth):
    profile = tools.PianoProfile()
    times = [np.arange(n) * HOP / SR for n in bank.frame_counts]
    labels = LabelBank.from_notes([(t[:, 2], t[:, :2]) for t in truth], times, profile, keys=(tools.KEY_MULTIPITCH,), bank=bank)
    return labels, NoteBank(truth, bank=bank)


def _host_scores(make, model, bank, labels, notes, ids, firsts, note_ref):
    """The host evaluators on run_on_batch's predictions of the same bank clips and NumPy-sliced references."""
    combo = make()
    sliced = notes.host_clips(ids, firsts, T)
    for i, (k, f, est) in enumerate(zip(ids, firsts, _predictions(model, bank, ids, firsts))):
        reference = {key: labels.host_map(k, key)[:, f:f + T] for key in labels.keys}
        reference[tools.KEY_NOTES] = note_ref(sliced[i * notes.slices:(i + 1) * notes.slices])
        combo.process_track(est, reference, i)
    return combo


@pytest.mark.parametrize('batch_size', [3, 256])
def test_validate_clips_equals_the_host_evaluators_on_onsets_and_frames(batch_size, tmp_path):
    model, bank, truth = piano_setup()
    labels, notes = _piano_banks(bank, truth)
    assert notes.integral and notes.slices == 1
    ids, firsts = _requests(bank)
    want = _host_scores(piano_combo, model, bank, labels, notes, ids, firsts, lambda groups: groups[0])
    fallbacks = autograd.fallback_total()
    combo = piano_combo()
    combo.set_save_dir(str(tmp_path))
    average = ev.validate_clips(bank, labels, notes, model, combo, ids, firsts, T, batch_size=batch_size)
    assert autograd.fallback_total() == fallbacks
    assert average == want.average_results() and list(average) == [tools.KEY_MULTIPITCH, tools.KEY_NOTES, 'notes-with-offsets']
    _same_per_clip(combo, want, len(ids))
    assert 0 < average[tools.KEY_NOTES][tools.KEY_F1] < 1 and 0 < average['notes-with-offsets'][tools.KEY_F1] < 1
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(f'{i}.txt' for i in range(len(ids)))
    # this rank's share
    shard = piano_combo()
    ev.validate_clips(bank, labels, notes, model, shard, ids, firsts, T, batch_size=batch_size, rank=1, world=2)
    assert np.array_equal(shard.evaluators[1].results[tools.KEY_F1], np.asarray(want.evaluators[1].results[tools.KEY_F1])[1::2])


def test_a_fractional_reference_pitch_takes_the_host_matcher():
    model, bank, truth = piano_setup()
    truth = [t.copy() for t in truth]
    truth[1][0, 2] += 0.5
    labels, notes = _piano_banks(bank, [np.concatenate([t[:, :2], np.floor(t[:, 2:])], axis=1) for t in truth])
    notes = NoteBank(truth, bank=bank)
    assert not notes.integral
    ids, firsts = _requests(bank)
    want = _host_scores(piano_combo, model, bank, labels, notes, ids, firsts, lambda groups: groups[0])
    combo = piano_combo()
    average = ev.validate_clips(bank, labels, notes, model, combo, ids, firsts, T, batch_size=3)
    assert average == want.average_results()
    _same_per_clip(combo, want, len(ids))


def test_validate_clips_equals_the_host_evaluators_on_tabcnn():
    from amt_tools_amd.models import TabCNN
    mod = CQT(sample_rate=SR, hop_length=HOP, n_bins=192, bins_per_octave=24)
    model = TabCNN(192, GUITAR, 1, 1, device=DEV)
    model.load_state_dict(_tensors(synth_tabcnn_state_dict(5, dim_in=192, in_channels=1, model_complexity=1, num_groups=6, num_classes=21)))
    model.frontend = torch.nn.Sequential(mod.frontend())
    model.change_device()
    model.eval()
    bank = PyramidBank([synth_clip(3, num_samples=60000), synth_clip(9, num_samples=30001)], mod, DEV)
    assert (bank.frame_counts >= T).all()
    # ground truth: the model's own tablature of the covering clips with half of its cells redrawn; the uncovered tails are silent
    rng = np.random.default_rng(50)
    tabs = [np.full((6, int(n)), -1, dtype=np.int64) for n in bank.frame_counts]
    cover_ids, cover_firsts, _ = cover_clips(bank.frame_counts, T)
    for k, f, est in zip(cover_ids, cover_firsts, _predictions(model, bank, cover_ids, cover_firsts)):
        tabs[k][:, f:f + T] = np.where(rng.random((6, T)) < 0.5, est[tools.KEY_TABLATURE], np.repeat(rng.integers(-1, 20, size=(6, T // 4)), 4, axis=-1))
    stacked = [transcribe._tab_to_stacked_notes_host(tab, np.arange(tab.shape[1]) * HOP / SR, GUITAR) for tab in tabs]
    labels = LabelBank([{tools.KEY_TABLATURE: tab} for tab in tabs], bank=bank)
    notes = NoteBank(stacked, bank=bank)
    assert notes.slices == 6 and notes.keys == list(stacked[0].keys()) and notes.integral and len(notes.rows) > 20
    make = lambda: ev.ComboEvaluator([ev.TablatureEvaluator(GUITAR), ev.StackedNoteEvaluator(offset_ratio=0.2),       # noqa: E731
                                      ev.StackedNoteEvaluator(average_slices=True, results_key='notes-avg')])
    ids, firsts = _requests(bank)
    want = _host_scores(make, model, bank, labels, notes, ids, firsts,
                        lambda groups: {key: (g[:, 2], g[:, :2]) for key, g in zip(notes.keys, groups)})
    fallbacks = autograd.fallback_total()
    for batch_size in (3, 256):
        combo = make()
        average = ev.validate_clips(bank, labels, notes, model, combo, ids, firsts, T, batch_size=batch_size)
        assert average == want.average_results()
        _same_per_clip(combo, want, len(ids))
        assert 0 < average[tools.KEY_TABLATURE][tools.KEY_F1] < 1 and list(average[tools.KEY_NOTES]) == list(range(6))
    assert autograd.fallback_total() == fallbacks


def test_both_batch_sources_go_through_the_one_driver_with_the_same_results():
    """Tracks of exactly one clip each: the bank's clip of a whole track is framed and scaled as the host clip is, so the uploaded route
    (run_offline_batched, validate_batched) and the bank route (_batched over a BankClips, validate_clips) see the same features and
    have to return the same predictions and the same results, per clip."""
    model, _, _ = piano_setup()
    mod = model.frontend[0].module
    clips = np.stack([synth_clip(20 + i, num_samples=HOP * T - 1) for i in range(5)])
    bank = TrackBank(list(clips), mod, DEV)
    assert bank.frame_counts.tolist() == [T] * 5
    ids, firsts = np.arange(5), np.zeros(5, dtype=np.int64)
    uploaded = run_offline_batched(clips, model, batch_size=2, decode_notes=True)
    resident, calls = {}, []

    def enqueue(idx, preds, extra):
        calls.append(('enqueue', list(idx), extra))
        return idx, preds, transcribe.decode_notes_for(preds, model, None)

    def finish(pending):
        idx, preds, handle = pending
        calls.append(('finish', list(idx)))
        host = tools.dict_to_array(preds)
        for j, i in enumerate(idx):
            resident[i] = dict({k: v[j] for k, v in host.items() if isinstance(v, np.ndarray)}, **{tools.KEY_NOTES: handle.result()[j]})

    _batched(BankClips(bank, ids, firsts, T), model, 2, 0, 1, enqueue, finish, lambda idx: ('extra', list(idx)))
    assert calls == [('enqueue', [0, 1], ('extra', [0, 1])), ('enqueue', [2, 3], ('extra', [2, 3])), ('finish', [0, 1]),
                     ('enqueue', [4], ('extra', [4])), ('finish', [2, 3]), ('finish', [4])]
    assert sorted(resident) == sorted(uploaded) == list(range(5))
    for i in range(5):
        assert sorted(resident[i]) == sorted(uploaded[i])
        for k in uploaded[i]:
            assert np.asarray(resident[i][k]).tobytes() == np.asarray(uploaded[i][k]).tobytes(), (i, k)
    # the two validation loops on the same ground truth
    rng = np.random.default_rng(4)
    truth = []
    for i in range(5):
        rows = np.array(uploaded[i][tools.KEY_NOTES], dtype=np.float64).reshape(-1, 3)
        onsets = rng.integers(0, T - 1, 6) * HOP / SR
        truth.append(np.concatenate([rows[rng.random(len(rows)) < 0.6], np.stack([onsets, onsets + 3 * HOP / SR, rng.integers(21, 109, 6).astype(np.float64)], axis=1)]))
    labels, notes = _piano_banks(bank, truth)
    references = [{tools.KEY_MULTIPITCH: labels.host_map(i, tools.KEY_MULTIPITCH), tools.KEY_NOTES: notes.host_clips([i], [0], T)[0]} for i in range(5)]
    a, b = piano_combo(), piano_combo()
    assert ev.validate_batched(clips, references, model, a, batch_size=2) == ev.validate_clips(bank, labels, notes, model, b, ids, firsts, T, batch_size=2)
    _same_per_clip(a, b, 5)
    assert sum(len(uploaded[i][tools.KEY_NOTES]) for i in range(5)) > 0
