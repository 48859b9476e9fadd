"""amt_tools_amd.evaluate on the host: the evaluator classes against what the reference's own classes returned (tests/golden/evaluators.npz,
tools/gen_golden_eval.py), the note matcher against a brute force (tests/eval_cases.py), and the plumbing train() relies on."""
import warnings

import numpy as np
import pytest

from amt_tools_amd import evaluate as ev, tools
from conftest import load_golden
import eval_cases as ec

G = load_golden('evaluators.npz')
KINDS = [str(k) for k in G['kinds']]
PROFILE = tools.GuitarProfile(num_frets=19)


def flatten(results, prefix=''):
    keys, values = [], []
    for k, v in results.items():
        if isinstance(v, dict):
            kk, vv = flatten(v, f'{prefix}{k}/')
            keys, values = keys + kk, values + vv
        else:
            keys.append(f'{prefix}{k}')
            values.append(v)
    return keys, values


def assert_golden(case, results):
    """Structure and keys equal; values within a few float64 roundings (the operation order inside hmean is the only room given)."""
    keys, values = flatten(results)
    assert keys == [str(k) for k in G[f'{case}__keys']], case
    np.testing.assert_allclose(np.array(values, dtype=np.float64), G[f'{case}__values'], rtol=1e-14, atol=1e-15, err_msg=case)


def test_the_fixture_holds_the_edge_cases():
    assert {'silent_est', 'silent_ref', 'both_silent', 'perfect', 'duplicate_pitch'} <= set(KINDS)
    assert not G['stacked_silent_est_est'].any() and G['stacked_silent_est_ref'].any()
    assert G['stacked_silent_ref_est'].any() and not G['stacked_silent_ref_ref'].any()
    assert not G['stacked_both_silent_est'].any() and not G['stacked_both_silent_ref'].any()
    assert np.array_equal(G['stacked_perfect_est'], G['stacked_perfect_ref']) and np.array_equal(G['tab_perfect_est'], G['tab_perfect_ref'])
    tab = G['tab_duplicate_pitch_est']
    tuning = np.array(PROFILE.get_midi_tuning())
    assert tab[0, 3] >= 0 and tab[0, 3] + tuning[0] == tab[1, 3] + tuning[1]
    assert 'f_measure' in str(G['provenance'])


@pytest.mark.parametrize('kind', KINDS)
def test_map_and_tablature_evaluators_equal_the_reference(kind):
    est, ref = G[f'stacked_{kind}_est'], G[f'stacked_{kind}_ref']
    assert_golden(f'stacked_{kind}', ev.StackedMultipitchEvaluator().evaluate(est, ref))
    assert_golden(f'stacked_avg_{kind}', ev.StackedMultipitchEvaluator(average_slices=True).evaluate(est, ref))
    assert_golden(f'multipitch_{kind}', ev.MultipitchEvaluator().evaluate(est[0], ref[0]))
    te, tr = G[f'tab_{kind}_est'], G[f'tab_{kind}_ref']
    assert_golden(f'tablature_{kind}', ev.TablatureEvaluator(PROFILE).evaluate(te, tr))
    assert_golden(f'softmax_{kind}', ev.SoftmaxAccuracy().evaluate(te, tr))


def golden_combo():
    return ev.ComboEvaluator([ev.LossWrapper(), ev.MultipitchEvaluator(unpack_key='mp0'), ev.StackedMultipitchEvaluator(results_key='per-slice'),
                              ev.TablatureEvaluator(PROFILE), ev.SoftmaxAccuracy(results_key=tools.KEY_TABLATURE)])


def golden_track(n, kind):
    loss = {tools.KEY_LOSS_TOTAL: np.float64(G[f'combo_track{n}_loss'][0]), tools.KEY_LOSS_PITCH: np.float64(G[f'combo_track{n}_loss'][1])}
    est = {tools.KEY_LOSS: loss, tools.KEY_MULTIPITCH: G[f'stacked_{kind}_est'], tools.KEY_TABLATURE: G[f'tab_{kind}_est'], 'mp0': G[f'stacked_{kind}_est'][0]}
    ref = {tools.KEY_MULTIPITCH: G[f'stacked_{kind}_ref'], tools.KEY_TABLATURE: G[f'tab_{kind}_ref'], 'mp0': G[f'stacked_{kind}_ref'][0]}
    return est, ref


def test_combo_evaluator_routes_appends_and_averages_like_the_reference(tmp_path):
    combo = golden_combo()
    combo.set_save_dir(str(tmp_path / 'results'))
    tracked = dict()
    for n, kind in enumerate(('random', 'perfect', 'duplicate_pitch')):
        results = combo.process_track(*golden_track(n, kind), f'track{n}')
        assert_golden(f'combo_track{n}', results)
        tracked = ev.append_results(tracked, results)
    assert_golden('combo_average', combo.average_results())
    keys, values = flatten(tracked)
    assert keys == [str(k) for k in G['appended__keys']]
    np.testing.assert_allclose(np.stack(values), G['appended__values'], rtol=1e-14, atol=1e-15)
    assert_golden('appended_average', ev.average_results(tracked))
    # routing: SoftmaxAccuracy shares the tablature evaluator's results key, every evaluator keeps its own tracked results
    assert list(combo.average_results()) == [tools.KEY_LOSS, tools.KEY_MULTIPITCH, 'per-slice', tools.KEY_TABLATURE]
    assert list(combo.evaluators[4].results) == [tools.KEY_ACCURACY] and len(combo.evaluators[4].results[tools.KEY_ACCURACY]) == 3
    text = (tmp_path / 'results' / 'track1.txt').read_text()
    assert '-----per-slice-----' in text and f' {tools.KEY_TDR} : ' in text and f' {tools.KEY_ACCURACY} : 1.0' in text
    combo.reset_results()
    assert all(e.results == {} for e in combo.evaluators)


def test_loss_wrapper_with_and_without_a_loss():
    lw = ev.LossWrapper()
    assert lw.process_track({tools.KEY_LOSS: {tools.KEY_LOSS_TOTAL: np.float64(2.0)}}, None) == {tools.KEY_LOSS_TOTAL: 2.0}
    lw.process_track({tools.KEY_LOSS: {tools.KEY_LOSS_TOTAL: np.float64(4.0)}}, None)
    assert lw.average_results() == {tools.KEY_LOSS_TOTAL: 3.0}
    with pytest.warns(RuntimeWarning, match='not found in estimates'):
        assert lw.unpack({tools.KEY_MULTIPITCH: 1}) == (None, None)


class Writer(object):
    def __init__(self):
        self.calls = []

    def add_scalar(self, tag, value, global_step=None):
        self.calls.append((tag, value, global_step))


def test_finalize_logs_the_averages_and_resets():
    combo = golden_combo()
    combo.set_patterns(['f1', 'loss_total'])
    for n, kind in enumerate(('random', 'perfect')):
        combo.process_track(*golden_track(n, kind))
    average = combo.average_results()
    writer = Writer()
    combo.finalize(writer, step=7)
    tags = [c[0] for c in writer.calls]
    assert tags == ['validation/loss/loss_total', 'validation/multi_pitch/f1-score', 'validation/per-slice/0/f1-score', 'validation/per-slice/1/f1-score',
                    'validation/per-slice/2/f1-score', 'validation/tablature/f1-score']
    assert all(step == 7 and isinstance(v, float) for _, v, step in writer.calls)
    assert writer.calls[1][1] == average[tools.KEY_MULTIPITCH][tools.KEY_F1] and writer.calls[0][1] == 1.0
    assert all(e.results == {} for e in combo.evaluators)
    assert ev.pattern_match('f1-score', ['f1']) and not ev.pattern_match('recall', ['f1']) and not ev.pattern_match('recall')


# ------------------------------------------------------------------------------------------------------------------------------
# note matching
# ------------------------------------------------------------------------------------------------------------------------------
def test_n_decimals_is_the_constant_the_cases_restate():
    assert ev.N_DECIMALS == ec.D and ev.ONSET_TOLERANCE == ec.ONSET_TOL and ev.OFFSET_MIN_TOLERANCE == ec.OFFSET_MIN_TOL


@pytest.mark.parametrize('ratio', ec.RATIOS)
@pytest.mark.parametrize('name', sorted(ec.cases()))
def test_host_matcher_equals_the_brute_force(name, ratio):
    est, ref = ec.cases()[name]
    assert np.array_equal(ev.note_edges(est[:, 2], est[:, :2], ref[:, 2], ref[:, :2], ratio), ec.brute_edges(est, ref, ratio))
    assert ev.match_notes_count(est[:, 2], est[:, :2], ref[:, 2], ref[:, :2], ratio) == ec.expected(name, ratio)
    shuffled = np.random.default_rng(0).permutation(len(est))
    got = ev.NoteEvaluator(offset_ratio=ratio).evaluate(est[shuffled], ref)
    m = ec.expected(name, ratio)
    if len(est) == 0 or len(ref) == 0:
        assert got == {tools.KEY_PRECISION: 0.0, tools.KEY_RECALL: 0.0, tools.KEY_F1: 0.0}
    else:
        p, r = m / len(est), m / len(ref)
        assert got == {tools.KEY_PRECISION: p, tools.KEY_RECALL: r, tools.KEY_F1: 0.0 if m == 0 else 2 * p * r / (p + r)}


def test_own_augmenting_paths_equal_scipy(monkeypatch):
    import builtins
    real = builtins.__import__

    def no_scipy(name, *a, **k):
        if name.startswith('scipy'):
            raise ImportError(name)
        return real(name, *a, **k)
    for name in ('greedy_a', 'greedy_b', 'jittered', 'long_list', 'random_3'):
        est, ref = ec.cases()[name]
        with monkeypatch.context() as mp:
            mp.setattr(builtins, '__import__', no_scipy)
            got = ev.match_notes_count(est[:, 2], est[:, :2], ref[:, 2], ref[:, :2], 0.2)
        assert got == ec.expected(name, 0.2), name


def test_tolerance_edges_are_where_the_cases_say():
    """At the tolerance and up to half a rounding unit past it a pair matches; from one rounding unit past it on it does not."""
    est, ref = ec.cases()['tolerance_edges']
    edges = ec.brute_edges(est, ref, 0.2).diagonal().reshape(-1, 4)            # rows: the deltas; columns: late / early onset, two offsets
    deltas = [0.0, ec.UNIT, -ec.UNIT, 0.4 * ec.UNIT, 0.6 * ec.UNIT, -0.4 * ec.UNIT, -0.6 * ec.UNIT]
    for d, row in zip(deltas, edges):
        assert row.all() == (d < 0.5 * ec.UNIT) and row.any() == row.all(), (d, row)


@pytest.mark.parametrize('name', ['greedy_a', 'greedy_b'])
def test_earliest_first_greedy_is_not_maximum_under_the_offset_rule(name):
    est, ref = ec.cases()[name]
    assert ec.greedy_matched(est, ref, 0.2) < ec.expected(name, 0.2) == len(est)
    assert ec.greedy_matched(est, ref, None) == ec.expected(name, None)          # onsets only: windows are contiguous runs
    assert ev.match_notes_count(est[:, 2], est[:, :2], ref[:, 2], ref[:, :2], 0.2) == len(est)


def test_fractional_pitches_follow_the_50_cent_rule():
    est = np.array([[1.0, 2.0, 60.5], [1.0, 2.0, 62.51]])
    ref = np.array([[1.0, 2.0, 60.0], [1.0, 2.0, 62.0]])
    assert ev.note_edges(est[:, 2], est[:, :2], ref[:, 2], ref[:, :2]).tolist() == [[True, False], [False, False]]


def test_stacked_note_evaluator_pairs_slices_by_position():
    est, ref = ec.cases()['random_2']
    stacked_est = {s: (est[s::3, 2], est[s::3, :2]) for s in range(3)}
    stacked_ref = {s: (ref[s::3, 2], ref[s::3, :2]) for s in range(3)}
    got = ev.StackedNoteEvaluator(offset_ratio=0.2).evaluate(stacked_est, stacked_ref)
    assert list(got) == [0, 1, 2]
    for s in range(3):
        m = ec.brute_matched(est[s::3], ref[s::3], 0.2)
        assert got[s][tools.KEY_PRECISION] == m / len(est[s::3]) and got[s][tools.KEY_RECALL] == m / len(ref[s::3])
    avg = ev.StackedNoteEvaluator(offset_ratio=0.2, average_slices=True).evaluate(stacked_est, stacked_ref)
    assert avg[tools.KEY_RECALL] == float(np.mean([got[s][tools.KEY_RECALL] for s in range(3)]))


# ------------------------------------------------------------------------------------------------------------------------------
# validate
# ------------------------------------------------------------------------------------------------------------------------------
class StubDataset(object):
    def __init__(self, tracks):
        self._data = tracks
        self.tracks = list(tracks)

    def get_track_data(self, track_id):
        return self._data[track_id]


def test_validate_runs_the_model_track_by_track():
    torch = pytest.importorskip('torch')
    from amt_tools_amd.models import OnsetsFrames
    from amt_tools_amd.synth import synth_state_dict
    from amt_tools_amd.transcribe import NoteTranscriber, multi_pitch_to_notes
    from amt_tools_amd.inference import run_offline
    profile = tools.PianoProfile()
    model = OnsetsFrames(229, profile, 1, 2, device='cpu')
    sd = synth_state_dict(3, dim_in=229, in_channels=1, model_complexity=2)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    T = 12
    times = (np.arange(T) * 512 / 22050.0).astype(np.float32)
    rng = np.random.default_rng(8)
    tracks = {}
    for name in ('a', 'b'):
        mp = (rng.random((88, T)) < 0.1).astype(np.float32)
        tracks[name] = {tools.KEY_TRACK: name, tools.KEY_FEATS: rng.random((1, 229, T)).astype(np.float32), tools.KEY_TIMES: times,
                        tools.KEY_MULTIPITCH: mp, tools.KEY_NOTES: multi_pitch_to_notes(mp, times)}
    combo = ev.ComboEvaluator([ev.MultipitchEvaluator(), ev.NoteEvaluator()])
    estimator = NoteTranscriber(profile)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        average = ev.validate(model, StubDataset(tracks), combo, estimator)
    want = ev.ComboEvaluator([ev.MultipitchEvaluator(), ev.NoteEvaluator()])
    for name in ('a', 'b'):
        want.process_track(run_offline(tracks[name], model, estimator), tracks[name], name)
    assert average == want.average_results() and list(average) == [tools.KEY_MULTIPITCH, tools.KEY_NOTES]
    assert len(combo.evaluators[0].results[tools.KEY_F1]) == 2
    with pytest.raises(NotImplementedError):
        ev.validate(model, StubDataset(tracks), combo, estimator, online=True)
