"""Threshold grids on the host: evaluate.multipitch_grid_counts and transcribe.decode_notes_grid on host arrays against a loop over
thresholds of the code that already exists (MultipitchEvaluator's counting, multi_pitch_to_notes) on random maps, exactly; the argument
errors of evaluate.sweep_tracks and of run_tracks(thresholds=...), raised before anything is launched."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from amt_tools_amd import evaluate as ev, inference, tools, transcribe               # noqa: E402

THRESHOLDS = (0.0, 0.25, 0.5, 0.75, 1.0, 1.5)


def _maps(seed, B=3, K=7, T=70):
    """Probability maps with cells ON thresholds, a NaN and the values 0 and 1 among them, and a {0, 1} reference."""
    rng = np.random.default_rng(seed)
    prob = rng.random((B, K, T)).astype(np.float32)
    prob[rng.random(prob.shape) < 0.2] = np.float32(0.5)
    prob[rng.random(prob.shape) < 0.05] = np.float32(1.0)
    prob[rng.random(prob.shape) < 0.05] = np.float32(0.0)
    prob[0, 1, 3] = np.nan
    return prob, (rng.random(prob.shape) < 0.3).astype(np.float32)


def test_cut_activations_is_the_device_expression():
    prob = np.array([0.0, 0.4999, 0.5, 0.5001, 1.0, np.nan, np.inf, -np.inf], dtype=np.float32)
    assert transcribe.cut_activations(prob, 0.5).tolist() == [0, 0, 1, 1, 1, 1, 1, 0]
    assert transcribe.cut_activations(prob, 0.0).tolist() == [1, 1, 1, 1, 1, 1, 1, 0]
    assert transcribe.cut_activations(prob, 1.5).tolist() == [0, 0, 0, 0, 0, 1, 1, 0]
    assert transcribe.cut_activations(prob, 0.5).dtype == np.float32


@pytest.mark.parametrize('as_tensor', [False, True])
def test_host_grid_counts_equal_the_evaluators_counting_per_threshold(as_tensor):
    prob, ref = _maps(1)
    got = ev.multipitch_grid_counts(torch.from_numpy(prob) if as_tensor else prob, torch.from_numpy(ref) if as_tensor else ref, THRESHOLDS)
    assert got.shape == (3, len(THRESHOLDS), 3) and got.dtype == np.int64
    for g, thr in enumerate(THRESHOLDS):
        for b in range(3):
            want = ev.MultipitchEvaluator.counts(transcribe.cut_activations(prob[b], thr)[None], ref[b][None])[0]
            assert got[b, g].tolist() == want.tolist(), (b, thr)
    assert len({tuple(got[0, g]) for g in range(len(THRESHOLDS))}) >= 4            # the thresholds tell the maps apart
    assert got[0, 0, 1] == prob[0].size - 0 and got[0, -1, 1] == 1                  # threshold 0: every cell; above 1: the NaN alone


@pytest.mark.parametrize('with_onsets', [True, False])
def test_host_grid_decode_equals_multi_pitch_to_notes_per_pair(with_onsets):
    mp, _ = _maps(2)
    on, _ = _maps(3)
    times = np.arange(mp.shape[-1]) * 512 / 22050
    pairs = [(0.5, 0.5), (0.9, 0.25), (0.5, 0.5), (0.0, 1.0), (1.5, 0.75)]
    got = transcribe.decode_notes_grid(on if with_onsets else None, mp, times, pairs, low=21)
    assert len(got) == len(pairs) * 3
    totals = []
    for p, (on_thr, mp_thr) in enumerate(pairs):
        for b in range(3):
            want = transcribe.multi_pitch_to_notes(transcribe.cut_activations(mp[b], mp_thr), times, 21,
                                                   transcribe.cut_activations(on[b], on_thr) if with_onsets else None)
            assert got[p * 3 + b].dtype == np.float64 and np.array_equal(got[p * 3 + b], want), (p, b)
        totals.append(sum(len(got[p * 3 + b]) for b in range(3)))
    assert len(set(totals)) >= 3 and totals[0] == totals[2]
    # CPU tensors take the same path
    again = transcribe.decode_notes_grid(torch.from_numpy(on) if with_onsets else None, torch.from_numpy(mp), times, np.array(pairs), low=21)
    assert all(np.array_equal(a, b) for a, b in zip(again, got))


def test_grid_decode_argument_errors():
    mp, _ = _maps(2)
    times = np.arange(mp.shape[-1]) * 512 / 22050
    with pytest.raises(ValueError, match=r'one \(T,\) time grid'):
        transcribe.decode_notes_grid(None, mp, np.tile(times, (3, 1)), [(0.5, 0.5)])
    with pytest.raises(ValueError, match='at least one'):
        transcribe.decode_notes_grid(None, mp, times, [])


class _Model(object):
    """Enough of a model for the checks that run before anything is launched."""
    training = False
    device = 'cpu'


def _of_model():
    from amt_tools_amd.models import OnsetsFrames
    model = OnsetsFrames.__new__(OnsetsFrames)
    torch.nn.Module.__init__(model)
    model.device = 'cpu'
    model.eval()
    return model


class _Bank(object):
    frame_counts = np.array([100, 80])

    def __len__(self):
        return 2


class _Labels(_Bank):
    keys = (tools.KEY_MULTIPITCH,)


class _Notes(_Bank):
    stacked, relative_times, integral, slices = False, True, True, 1


def test_sweep_tracks_argument_errors():
    model, bank, labels, notes = _of_model(), _Bank(), _Labels(), _Notes()
    good = ev.ComboEvaluator([ev.MultipitchEvaluator(), ev.NoteEvaluator(), ev.LossWrapper()])
    sweep = lambda e=good, on=(0.5,), fr=(0.5,), m=model, margin=3, lab=labels, nb=notes: ev.sweep_tracks(bank, lab, nb, m, e, 64, margin, on, fr)   # noqa: E731
    # the exact route's own checks
    with pytest.raises(ValueError, match='OnsetsFrames'):
        sweep(m=_Model())
    with pytest.raises(ValueError, match='margin >= 3'):
        sweep(margin=2)
    # the leaves
    for bad in (ev.TablatureEvaluator(tools.GuitarProfile()), ev.SoftmaxAccuracy(), ev.StackedNoteEvaluator(), ev.StackedMultipitchEvaluator()):
        with pytest.raises(ValueError, match=f'not {type(bad).__name__}'):
            sweep(e=ev.ComboEvaluator([ev.MultipitchEvaluator(), bad]))
    with pytest.raises(ValueError, match='frame thresholds'):
        sweep(e=ev.MultipitchEvaluator(unpack_key=tools.KEY_ONSETS))
    # the banks, as validate_tracks
    with pytest.raises(ValueError, match='needs a LabelBank'):
        sweep(lab=None)
    with pytest.raises(ValueError, match='needs a NoteBank'):
        sweep(nb=None)
    # the thresholds
    for axis in ('on', 'fr'):
        name = {'on': 'onset_thresholds', 'fr': 'frame_thresholds'}[axis]
        for bad, text in (((), 'at least one'), ((0.5, float('nan')), 'finite'), ((float('inf'),), 'finite'), ((-0.1, 0.5), 'not negative'),
                          (tuple(np.linspace(0, 1, 33)), 'at most 32')):
            with pytest.raises(ValueError, match=f'{name}.*{text}'):
                sweep(**{axis: bad})
    # all of the above passed: the last check is the device
    with pytest.raises(ValueError, match='has to be on a GPU'):
        sweep(on=tuple(np.linspace(0, 1, 32)), fr=(0.0, 1.0, 1.5))
    assert all(e.results == {} for e in good.evaluators)


def test_run_tracks_thresholds_argument_errors():
    model, bank = _of_model(), _Bank()
    with pytest.raises(ValueError, match='exact=True'):
        inference.run_tracks(bank, model, 64, 3, thresholds=(0.5, 0.5))
    for bad, text in (((0.5,), 'pair'), ((0.5, 0.5, 0.5), 'pair'), ((0.5, float('nan')), 'finite'), ((-1.0, 0.5), 'not negative')):
        with pytest.raises(ValueError, match=text):
            inference.run_tracks(bank, model, 64, 3, exact=True, thresholds=bad)
