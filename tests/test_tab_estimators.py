"""The guitar estimators on the host -- tools.tablature_to_stacked_multi_pitch / stacked_multi_pitch_to_multi_pitch / notes_to_stacked_notes
and transcribe.ComboEstimator / TablatureWrapper / StackedMultiPitchCollapser / StackedNoteTranscriber -- against what the reference's own
classes returned for the same tablatures (tests/golden/tab_estimators.npz, tools/gen_golden_tab.py): bit for bit, dtypes and shapes
included, and through the two inference drivers on a CPU TabCNN."""
import numpy as np
import pytest
import torch

from amt_tools_amd import tools, transcribe
from amt_tools_amd.inference import run_offline, run_offline_batched
from amt_tools_amd.models import TabCNN
from amt_tools_amd.synth import synth_tabcnn_state_dict
from conftest import load_golden

G = load_golden('tab_estimators.npz')
LENGTHS = tuple(int(t) for t in G['lengths'])
NOTE_LENGTHS = tuple(t for t in LENGTHS if t not in G['no_notes_lengths'])
WINDOWS = tuple(None if w < 0 else float(w) for w in G['windows'])
MIN_DURATIONS = tuple(None if m < 0 else float(m) for m in G['min_durations'])
GRIDS = ('float64', 'float32')
PROFILE = tools.GuitarProfile(num_frets=19)


def golden_notes(T, grid, window, min_dur):
    """{string: (pitches, intervals)} of one recorded case."""
    tag = f'T{T}_{grid}_w{"n" if window is None else window}_m{"n" if min_dur is None else min_dur}'
    c = list(G['note_cases']).index(tag)
    off = G['note_offsets'][c]
    return {s: (G['notes'][off[s]:off[s + 1], 2], G['notes'][off[s]:off[s + 1], :2]) for s in range(len(off) - 1)}


def assert_stacked_notes_equal(got, ref):
    assert list(got.keys()) == list(ref.keys())
    for s in ref:
        (gp, gi), (rp, ri) = got[s], ref[s]
        assert gp.dtype == np.float64 and gi.dtype == np.float64, (s, gp.dtype, gi.dtype)
        assert gp.shape == rp.shape and gi.shape == ri.shape == (len(rp), 2), (s, gp.shape, gi.shape, rp.shape)
        assert np.array_equal(gp, rp) and np.array_equal(gi, ri), s


def test_fixture_covers_the_cases_it_is_meant_to():
    assert LENGTHS == (1, 2, 63, 64, 65, 129, 200) and NOTE_LENGTHS == (63, 64, 65, 129, 200)
    assert (PROFILE.low, PROFILE.high) == (int(G['midi_low']), int(G['midi_high'])) and PROFILE.get_midi_tuning() == list(G['midi_tuning'])
    tab = G['tab_T200']
    assert (tab[0] == -1).all() and tab[1, 0] >= 0 and (tab[1] >= 0).all()          # a silent string; a note at frame 0, no gaps
    assert tab[5, 0] == 19 and 0 in tab[5] and -1 in tab[5] and (tab[[1, 3, 5], -1] >= 0).all()
    plain, inhibited = golden_notes(200, 'float64', None, None), golden_notes(200, 'float64', 0.05, None)
    assert len(plain[0][0]) == 0 and plain[0][1].shape == (0, 2)
    assert 0 < len(inhibited[2][0]) < len(plain[2][0])                                # re-strikes inside the window vanish, others stay
    assert len(golden_notes(200, 'float64', None, 0.1)[4][0]) < len(plain[4][0])


@pytest.mark.parametrize('T', LENGTHS)
def test_maps_equal_the_reference(T):
    tab = G[f'tab_T{T}']
    stacked = tools.tablature_to_stacked_multi_pitch(tab, PROFILE)
    assert stacked.dtype == np.float64 and stacked.shape == (6, 44, T) and np.array_equal(stacked, G[f'stacked_T{T}'])
    collapsed = tools.stacked_multi_pitch_to_multi_pitch(stacked)
    assert collapsed.dtype == np.float64 and collapsed.shape == (44, T) and np.array_equal(collapsed, G[f'collapsed_T{T}'])
    as_tensor = tools.tablature_to_stacked_multi_pitch(torch.from_numpy(tab), PROFILE)
    assert str(as_tensor.dtype) == 'torch.' + str(G['stacked_dtype_from_int64_tensor']) and np.array_equal(as_tensor.numpy(), stacked)
    batch = tools.tablature_to_stacked_multi_pitch(torch.from_numpy(np.stack([tab, tab[::-1]]).astype(np.float32)), PROFILE)
    assert batch.dtype == torch.float32 and batch.shape == (2, 6, 44, T) and np.array_equal(batch[0].numpy(), stacked)
    assert np.array_equal(tools.stacked_multi_pitch_to_multi_pitch(batch)[0].numpy(), collapsed)
    assert np.array_equal(transcribe.TablatureWrapper(PROFILE).estimate({tools.KEY_TABLATURE: tab}), stacked)
    assert np.array_equal(transcribe.StackedMultiPitchCollapser(PROFILE).estimate({tools.KEY_MULTIPITCH: stacked}), collapsed)


def test_combo_estimator_feeds_each_estimator_the_updated_dict():
    tab = G['tab_T65']
    raw = {tools.KEY_TABLATURE: tab}
    combo = transcribe.ComboEstimator([transcribe.TablatureWrapper(profile=PROFILE), transcribe.StackedMultiPitchCollapser(profile=PROFILE)])
    out = combo.process_track(raw, 'track')
    assert sorted(out.keys()) == [tools.KEY_MULTIPITCH, tools.KEY_TABLATURE] and list(raw.keys()) == [tools.KEY_TABLATURE]
    assert out[tools.KEY_TABLATURE] is tab and np.array_equal(out[tools.KEY_MULTIPITCH], G['collapsed_T65'])
    # own keys: the stacked map survives next to its collapse, and the note transcriber reads the stacked one
    times = G['times_T65_float64']
    combo = transcribe.ComboEstimator([transcribe.TablatureWrapper(PROFILE, estimates_key='stacked', save_dir=None),
                                       transcribe.StackedMultiPitchCollapser(PROFILE, stacked_key='stacked'),
                                       transcribe.StackedNoteTranscriber(PROFILE, multi_pitch_key='stacked')])
    out = combo.process_track({tools.KEY_TABLATURE: tab, tools.KEY_TIMES: times})
    assert np.array_equal(out['stacked'], G['stacked_T65']) and np.array_equal(out[tools.KEY_MULTIPITCH], G['collapsed_T65'])
    assert_stacked_notes_equal(out[tools.KEY_NOTES], golden_notes(65, 'float64', None, None))
    assert transcribe.TablatureWrapper.get_default_key() == tools.KEY_MULTIPITCH == transcribe.StackedMultiPitchCollapser(PROFILE).get_key()
    assert transcribe.StackedNoteTranscriber.get_default_key() == tools.KEY_NOTES


@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('T', NOTE_LENGTHS)
def test_stacked_notes_equal_the_reference(T, grid):
    times = G[f'times_T{T}_{grid}']
    assert times.dtype == np.dtype(grid)
    raw = {tools.KEY_MULTIPITCH: G[f'stacked_T{T}'], tools.KEY_TIMES: times}
    for window in WINDOWS:
        for min_dur in MIN_DURATIONS:
            est = transcribe.StackedNoteTranscriber(profile=PROFILE, inhibition_window=window, minimum_duration=min_dur)
            assert_stacked_notes_equal(est.process_track(raw)[tools.KEY_NOTES], golden_notes(T, grid, window, min_dur))


@pytest.mark.parametrize('T', (1, 2))
def test_grids_too_short_for_a_hop_length_raise_like_the_reference(T):
    assert T in G['no_notes_lengths']
    raw = {tools.KEY_MULTIPITCH: G[f'stacked_T{T}'], tools.KEY_TIMES: G[f'times_T{T}_float64']}
    with pytest.raises(ValueError):
        transcribe.StackedNoteTranscriber(PROFILE).estimate(raw)


def test_notes_to_stacked_notes():
    ref = golden_notes(129, 'float32', None, None)[3]
    order = np.random.default_rng(1).permutation(len(ref[0]))
    got = tools.notes_to_stacked_notes(ref[0][order], ref[1][order], 'E')
    assert list(got.keys()) == ['E']
    assert_stacked_notes_equal({0: got['E']}, {0: ref})
    empty = tools.notes_to_stacked_notes(np.array([]), np.array([]), 2)[2]
    assert empty[0].shape == (0,) and empty[1].shape == (0, 2) and empty[0].dtype == empty[1].dtype == np.float64


def _cpu_tabcnn():
    model = TabCNN(24, PROFILE, 1, 1, device='cpu')
    sd = synth_tabcnn_state_dict(5, dim_in=24, in_channels=1, model_complexity=1, num_groups=6, num_classes=21)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model.eval()
    return model


def test_drivers_on_a_cpu_tabcnn():
    model = _cpu_tabcnn()
    T = 40
    feats = np.random.default_rng(3).random((3, 1, 24, T)).astype(np.float32)
    times = np.arange(T) * 512 / 22050.0
    combo = transcribe.ComboEstimator([transcribe.TablatureWrapper(profile=PROFILE), transcribe.StackedMultiPitchCollapser(profile=PROFILE)])
    singles = []
    for i in range(3):
        out = run_offline({tools.KEY_TRACK: f't{i}', tools.KEY_FEATS: feats[i], tools.KEY_TIMES: times}, model, combo)
        tab = out[tools.KEY_TABLATURE]
        assert tab.shape == (6, T) and tab.dtype == np.int64 and (tab >= 0).any()
        assert np.array_equal(out[tools.KEY_MULTIPITCH], tools.tablature_to_stacked_multi_pitch(tab, PROFILE).max(axis=0))
        singles.append(out)
    batched = run_offline_batched(feats, model, times=times, batch_size=2, decode_notes=True, keep=(tools.KEY_TABLATURE, tools.KEY_MULTIPITCH))
    assert sorted(batched.keys()) == [0, 1, 2]
    for i in range(3):
        tab = batched[i][tools.KEY_TABLATURE]
        assert np.array_equal(tab, singles[i][tools.KEY_TABLATURE])
        assert np.array_equal(batched[i][tools.KEY_MULTIPITCH], singles[i][tools.KEY_MULTIPITCH])
        stacked = tools.tablature_to_stacked_multi_pitch(tab, PROFILE)
        ref = transcribe.StackedNoteTranscriber(PROFILE).estimate({tools.KEY_MULTIPITCH: stacked, tools.KEY_TIMES: times})
        assert sum(len(p) for p, _ in ref.values()) > 0
        assert_stacked_notes_equal(batched[i][tools.KEY_NOTES], ref)
    notes_only = run_offline_batched(feats, model, times=times, decode_notes=True, keep=())
    assert list(notes_only[1].keys()) == [tools.KEY_NOTES]
    assert_stacked_notes_equal(notes_only[1][tools.KEY_NOTES], batched[1][tools.KEY_NOTES])


def test_tab_kernels_are_declared_and_refuse_bad_arguments():
    """No compute: every call below fails its argument checks before a launch."""
    L = _lib_checked()
    tab = np.zeros((1, 6, 8), dtype=np.int64)
    out = np.zeros((1, 6, 44, 8), dtype=np.float32)
    start = np.array([0, 5, 10, 15, 19, 24], dtype=np.int32)
    from amt_tools_amd import _lib
    # class 19 of the top string would be row 44 of a 44-row map
    bad = start.copy()
    bad[5] = 25
    assert L.amtx_tab_expand(_lib.ptr(tab), 1, 6, 8, _lib.ptr(bad), 20, 44, _lib.ptr(out), None, None) == -1
    assert b'do not fit' in L.amtx_last_error()
    assert L.amtx_tab_expand(_lib.ptr(tab), 1, 6, 8, _lib.ptr(start), 21, 44, _lib.ptr(out), None, None) == -1
    assert L.amtx_tab_expand(_lib.ptr(tab), 1, 6, 8, _lib.ptr(start), 20, 44, None, None, None) == -1          # no output requested
    assert L.amtx_tab_expand(_lib.ptr(tab), 1, 17, 8, _lib.ptr(start), 20, 44, _lib.ptr(out), None, None) == _lib.ERR_UNSUPPORTED
    rows, off, ext, rel = np.zeros((4, 3)), np.zeros(7, dtype=np.int32), np.zeros(9), np.zeros(8, dtype=np.int32)
    tuning = np.array(PROFILE.get_midi_tuning(), dtype=np.int32)
    args = lambda classes, release, cap: (_lib.ptr(tab), 1, 6, 8, _lib.ptr(tuning), classes, _lib.ptr(ext), 0, release, 0, 0, 0.0, _lib.ptr(rows), cap,   # noqa: E731
                                          _lib.ptr(off), None)
    assert L.amtx_tab_notes(*args(65, _lib.ptr(rel), 4)) == _lib.ERR_UNSUPPORTED
    assert L.amtx_tab_notes(*args(20, None, 0)) == -1


def _lib_checked():
    from amt_tools_amd import _lib
    L = _lib.lib()
    for name in ('amtx_tab_expand', 'amtx_tab_notes'):
        assert name in _lib.declared_symbols() and name in _lib.signatures() and hasattr(L, name), name
    return L
