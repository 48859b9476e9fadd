"""evaluate.sweep_tracks and run_tracks(thresholds=...) on the device, by identity with code that exists: the cell (0.5, 0.5) is
validate_tracks(exact=True); every other cell is the host evaluators on rolls that amtx_pianoroll_fwd cut from run_tracks' own
whole-track logits; run_tracks at a pair gives those rolls and their notes.  Every comparison is equality."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from amt_tools_amd import evaluate as ev, inference, tools, transcribe                  # noqa: E402
from amt_tools_amd.features import MelSpec                                              # noqa: E402
from amt_tools_amd.inference import KEY_LOGITS, run_tracks                              # noqa: E402
from amt_tools_amd.synth import synth_clip, synth_state_dict                            # noqa: E402
from amt_tools_amd.tracks import LabelBank, NoteBank, TrackBank                         # noqa: E402
from test_gpu_run_tracks import DEV, HOP, SR, _tensors, piano_combo                     # noqa: E402

T, MARGIN = 64, 3
ONSET_THRESHOLDS, FRAME_THRESHOLDS = (0.5, 0.3, 0.7), (0.5, 0.35)
SEED = 0
MAPS = (tools.KEY_ONSETS, tools.KEY_MULTIPITCH)


@functools.lru_cache(maxsize=None)
def setup(precision):
    """Two tracks of 150 and 70 frames (MelSpec 229) and OnsetsFrames at model_complexity 2 -- the smallest with a recurrence --, seeded."""
    from amt_tools_amd.models import OnsetsFrames
    mod = MelSpec(sample_rate=SR, hop_length=HOP, n_mels=229, n_fft=2048)
    model = OnsetsFrames(229, tools.PianoProfile(), 1, 2, device=DEV, precision=precision)
    model.load_state_dict(_tensors(synth_state_dict(SEED, dim_in=229, in_channels=1, model_complexity=2)))
    model.frontend = torch.nn.Sequential(mod.frontend())
    model.change_device()
    model.eval()
    bank = TrackBank([synth_clip(3, num_samples=HOP * 150 - 1), synth_clip(9, num_samples=HOP * 70 - 1)], mod, DEV)
    assert bank.frame_counts.tolist() == [150, 70]
    return model, bank


@functools.lru_cache(maxsize=None)
def truth(precision):
    """Ground truth from the model's own whole-track transcription, as tests/test_gpu_run_tracks.py perturbs it: a third of the notes
    dropped, a third moved by a hop, random notes added -> (LabelBank, NoteBank)."""
    model, bank = setup(precision)
    own = run_tracks(bank, model, T, MARGIN, keep=(), decode_notes=True, exact=True)
    rng = np.random.default_rng(8)
    rows_of = []
    for t, n in enumerate(bank.frame_counts):
        rows = np.array(own[t][tools.KEY_NOTES], dtype=np.float64).reshape(-1, 3)
        rows = rows[rng.random(len(rows)) < 0.67]
        rows[:, 0] += (rng.random(len(rows)) < 0.33) * HOP / SR
        rows[:, 1] = np.maximum(rows[:, 1], rows[:, 0])
        onsets = rng.integers(0, n - 1, 12) * HOP / SR
        rows_of.append(np.concatenate([rows, np.stack([onsets, onsets + rng.integers(1, 30, 12) * HOP / SR, rng.integers(21, 109, 12).astype(np.float64)], axis=1)]))
    times = [np.arange(n) * HOP / SR for n in bank.frame_counts]
    labels = LabelBank.from_notes([(r[:, 2], r[:, :2]) for r in rows_of], times, tools.PianoProfile(), keys=(tools.KEY_MULTIPITCH,), bank=bank)
    return labels, NoteBank(rows_of, bank=bank)


@functools.lru_cache(maxsize=None)
def swept(precision):
    model, bank = setup(precision)
    labels, notes = truth(precision)
    combo = piano_combo()
    out = ev.sweep_tracks(bank, labels, notes, model, combo, T, MARGIN, ONSET_THRESHOLDS, FRAME_THRESHOLDS, batch_size=3)
    assert all(e.results == {} for e in combo.evaluators)                      # the evaluator's own results are not touched
    return out


@functools.lru_cache(maxsize=None)
def cut(precision):
    """{(onset_thr, frame_thr): {track: predictions}} on the host: rolls cut by amtx_pianoroll_fwd from run_tracks' own logits (no host
    sigmoid), notes by the host decoder on those rolls."""
    model, bank = setup(precision)
    logits = run_tracks(bank, model, T, MARGIN, keep=(KEY_LOGITS,), exact=True)
    out = {}
    for a in ONSET_THRESHOLDS:
        for b in FRAME_THRESHOLDS:
            out[(a, b)] = {}
            for t, entry in logits.items():
                rolls = {key: inference.logits_to_map(torch.from_numpy(entry[KEY_LOGITS][key]).to(DEV).unsqueeze(0), thr)[0].cpu().numpy()
                         for key, thr in zip(MAPS, (a, b))}
                times = np.arange(rolls[MAPS[1]].shape[-1]) * HOP / SR
                rolls[tools.KEY_NOTES] = transcribe.multi_pitch_to_notes(rolls[tools.KEY_MULTIPITCH], times, 21, rolls[tools.KEY_ONSETS])
                out[(a, b)][t] = rolls
    return out


def _host_average(precision, pair, tracks=(0, 1)):
    labels, notes = truth(precision)
    combo = piano_combo()
    for t in tracks:
        reference = {key: labels.host_map(t, key) for key in labels.keys}
        reference[tools.KEY_NOTES] = notes.host_whole([t])[0]
        combo.process_track(cut(precision)[pair][t], reference, t)
    return combo.average_results()


@pytest.mark.parametrize('precision', ['bf16', 'x3'])
def test_the_default_cell_is_validate_tracks_exact(precision):
    model, bank = setup(precision)
    labels, notes = truth(precision)
    average = ev.validate_tracks(bank, labels, notes, model, piano_combo(), T, MARGIN, batch_size=3, exact=True)
    got = swept(precision)
    assert list(got) == [(a, b) for a in ONSET_THRESHOLDS for b in FRAME_THRESHOLDS]
    assert list(got[(0.5, 0.5)]) == list(average) == [tools.KEY_MULTIPITCH, tools.KEY_NOTES, 'notes-with-offsets']
    for key in average:
        assert list(got[(0.5, 0.5)][key]) == list(average[key])
        for metric, value in average[key].items():
            assert isinstance(got[(0.5, 0.5)][key][metric], float) and got[(0.5, 0.5)][key][metric] == value, (key, metric)
    assert 0 < average[tools.KEY_NOTES][tools.KEY_F1] < 1 and 0 < average[tools.KEY_MULTIPITCH][tools.KEY_F1] < 1


@pytest.mark.parametrize('precision', ['bf16', 'x3'])
def test_every_cell_is_the_host_evaluators_on_rolls_cut_from_the_logits(precision):
    got = swept(precision)
    for pair, results in got.items():
        print(f'SWEEP {precision} {pair}: frame F1 {results[tools.KEY_MULTIPITCH][tools.KEY_F1]:.4f} note F1 {results[tools.KEY_NOTES][tools.KEY_F1]:.4f} '
              f'with offsets {results["notes-with-offsets"][tools.KEY_F1]:.4f}')
        assert results == _host_average(precision, pair), pair
    # the grid matters: note F1 differs between cells, and a MultipitchEvaluator's entry follows the frame threshold alone
    assert len({results[tools.KEY_NOTES][tools.KEY_F1] for results in got.values()}) >= 2
    for b in FRAME_THRESHOLDS:
        assert all(got[(a, b)][tools.KEY_MULTIPITCH] == got[(ONSET_THRESHOLDS[0], b)][tools.KEY_MULTIPITCH] for a in ONSET_THRESHOLDS)
    assert got[(0.5, FRAME_THRESHOLDS[0])][tools.KEY_MULTIPITCH] != got[(0.5, FRAME_THRESHOLDS[1])][tools.KEY_MULTIPITCH]


def test_a_ranks_share_a_request_and_single_evaluators():
    model, bank = setup('bf16')
    labels, notes = truth('bf16')
    pair = (0.3, 0.35)
    share = ev.sweep_tracks(bank, labels, notes, model, piano_combo(), T, MARGIN, ONSET_THRESHOLDS, FRAME_THRESHOLDS, rank=1, world=2)
    assert share[pair] == _host_average('bf16', pair, tracks=(1,))
    # one note evaluator that is no combination, no LabelBank; a LossWrapper is ignored; the request's order does not change a mean of two
    alone = ev.sweep_tracks(bank, None, notes, model, ev.NoteEvaluator(), T, MARGIN, [0.3], [0.35], track_ids=[1, 0])
    assert list(alone) == [pair] and alone[pair] == swept('bf16')[pair][tools.KEY_NOTES]
    frames = ev.sweep_tracks(bank, labels, None, model, ev.ComboEvaluator([ev.LossWrapper(), ev.MultipitchEvaluator()]), T, MARGIN, [0.3], [0.35])
    assert frames[pair] == {tools.KEY_MULTIPITCH: swept('bf16')[pair][tools.KEY_MULTIPITCH]}
    assert ev.sweep_tracks(bank, labels, notes, model, piano_combo(), T, MARGIN, [0.5], [0.5], track_ids=[0], rank=1, world=2)[(0.5, 0.5)] == \
        {tools.KEY_MULTIPITCH: {}, tools.KEY_NOTES: {}, 'notes-with-offsets': {}}


def test_a_small_first_buffer_and_a_fractional_reference_pitch_take_the_host_matcher(monkeypatch):
    model, bank = setup('bf16')
    labels, notes = truth('bf16')
    pair = (0.3, 0.35)
    want = {k: v for k, v in swept('bf16')[pair].items() if k != tools.KEY_MULTIPITCH}
    real = transcribe.decode_notes_grid_async
    monkeypatch.setattr(transcribe, 'decode_notes_grid_async', lambda *args, **kw: real(*args, rows_capacity=8, event_bytes=1 << 16, **kw))
    combo = ev.ComboEvaluator(piano_combo().evaluators[1:])
    assert ev.sweep_tracks(bank, None, notes, model, combo, T, MARGIN, ONSET_THRESHOLDS, FRAME_THRESHOLDS)[pair] == want
    monkeypatch.undo()
    rows = [r.copy() for r in notes.host_whole([0, 1])]
    rows[0][0, 2] += 0.25                                                      # no edge: the pitch tolerance is 50 cents
    fractional = NoteBank(rows, bank=bank)
    assert not fractional.integral
    got = ev.sweep_tracks(bank, None, fractional, model, ev.NoteEvaluator(), T, MARGIN, [0.3], [0.35])[pair]
    combo = ev.NoteEvaluator()
    for t in (0, 1):
        combo.process_track({tools.KEY_NOTES: cut('bf16')[pair][t][tools.KEY_NOTES]}, {tools.KEY_NOTES: rows[t]}, t)
    assert got == combo.average_results()


@pytest.mark.parametrize('precision', ['bf16', 'x3'])
def test_run_tracks_applies_a_threshold_pair(precision):
    model, bank = setup(precision)
    keep = MAPS + (KEY_LOGITS,)
    plain = run_tracks(bank, model, T, MARGIN, batch_size=3, keep=keep, decode_notes=True, exact=True)
    default = run_tracks(bank, model, T, MARGIN, batch_size=3, keep=keep, decode_notes=True, exact=True, thresholds=(0.5, 0.5))
    pair = (0.3, 0.35)
    other = run_tracks(bank, model, T, MARGIN, batch_size=3, keep=MAPS, decode_notes=True, exact=True, thresholds=pair)
    assert list(plain) == list(default) == list(other) == [0, 1]
    changed = 0
    for t in (0, 1):
        assert sorted(default[t]) == sorted(plain[t]) and sorted(other[t]) == sorted(MAPS + (tools.KEY_NOTES,))
        for key in MAPS:
            assert np.array_equal(default[t][key], plain[t][key]) and default[t][key].dtype == plain[t][key].dtype
            assert np.array_equal(default[t][KEY_LOGITS][key].view(np.uint32), plain[t][KEY_LOGITS][key].view(np.uint32))
            assert np.array_equal(other[t][key], cut(precision)[pair][t][key]) and other[t][key].dtype == np.float32
            changed += int((other[t][key] != plain[t][key]).sum())
        assert np.array_equal(default[t][tools.KEY_NOTES], plain[t][tools.KEY_NOTES])
        assert np.array_equal(other[t][tools.KEY_NOTES], cut(precision)[pair][t][tools.KEY_NOTES])
    assert changed > 0
    # without keep, and notes only
    assert np.array_equal(run_tracks(bank, model, T, MARGIN, exact=True, thresholds=pair, track_ids=[1])[1][tools.KEY_ONSETS], other[1][tools.KEY_ONSETS])
    assert np.array_equal(run_tracks(bank, model, T, MARGIN, keep=(), decode_notes=True, exact=True, thresholds=pair)[0][tools.KEY_NOTES], other[0][tools.KEY_NOTES])


def test_refusals_on_the_device():
    model, bank = setup('bf16')
    labels, notes = truth('bf16')
    with pytest.raises(ValueError, match='exact=True'):
        run_tracks(bank, model, T, MARGIN, thresholds=(0.5, 0.5))
    with pytest.raises(ValueError, match='pair'):
        run_tracks(bank, model, T, MARGIN, exact=True, thresholds=(0.5,))
    for kwargs, text in ((dict(on=()), 'at least one'), (dict(fr=(0.5, float('nan'))), 'finite'), (dict(on=np.linspace(0, 1, 33)), 'at most 32'),
                         (dict(margin=2), 'margin >= 3'), (dict(e=ev.ComboEvaluator([ev.StackedNoteEvaluator()])), 'not StackedNoteEvaluator'),
                         (dict(lab=None), 'needs a LabelBank'), (dict(frames=4), 'num_frames')):
        e, on, fr = kwargs.get('e', piano_combo()), kwargs.get('on', ONSET_THRESHOLDS), kwargs.get('fr', FRAME_THRESHOLDS)
        with pytest.raises(ValueError, match=text):
            ev.sweep_tracks(bank, kwargs.get('lab', labels), notes, model, e, kwargs.get('frames', T), kwargs.get('margin', MARGIN), on, fr)
    model.train()
    try:
        with pytest.raises(ValueError, match='eval mode'):
            ev.sweep_tracks(bank, labels, notes, model, piano_combo(), T, MARGIN, ONSET_THRESHOLDS, FRAME_THRESHOLDS)
    finally:
        model.eval()
