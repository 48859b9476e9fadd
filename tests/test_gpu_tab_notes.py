"""Tablature decoding on the device (csrc/tabnotes.hip): amtx_tab_expand and amtx_tab_notes against the reference's recorded results
(tests/golden/tab_estimators.npz) and against this package's host estimators -- themselves pinned to that fixture in
tests/test_tab_estimators.py -- on random tablatures; then TabCNN end to end through run_offline_batched.  Everything is compared
for equality: the maps hold 0 and 1, the notes are float64 values gathered from the time grid."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from amt_tools_amd import _lib, tools, transcribe                                    # noqa: E402
from amt_tools_amd.inference import run_offline_batched                               # noqa: E402
from amt_tools_amd.models import TabCNN                                               # noqa: E402
from amt_tools_amd.synth import synth_tabcnn_state_dict                               # noqa: E402
from conftest import load_golden                                                      # noqa: E402
from poison import Poison                                                             # noqa: E402

DEV = 'cuda:0'
G = load_golden('tab_estimators.npz')
PROFILE = tools.GuitarProfile(num_frets=19)
GOLDEN_LENGTHS = tuple(int(t) for t in G['lengths'])
NOTE_LENGTHS = tuple(t for t in GOLDEN_LENGTHS if t not in G['no_notes_lengths'])
RANDOM_LENGTHS = (1, 63, 64, 65, 200)
OPTIONS = [(w, m) for w in (None, 0.05) for m in (None, 0.0, 0.1)]                   # the six option combinations of the fixture
HOP = 512 / 22050.0


def golden_notes(T, grid, window, min_dur):
    tag = f'T{T}_{grid}_w{"n" if window is None else window}_m{"n" if min_dur is None else min_dur}'
    off = G['note_offsets'][list(G['note_cases']).index(tag)]
    return {s: (G['notes'][off[s]:off[s + 1], 2], G['notes'][off[s]:off[s + 1], :2]) for s in range(len(off) - 1)}


@functools.lru_cache(maxsize=None)
def random_tab(T, num_classes=20):
    """(3, 6, T) int64: per clip two strings that change every frame (few classes: chains of onsets inside one inhibition window), two with
    sticky runs, one silent, one sounding a single class throughout."""
    rng = np.random.default_rng(900 + T + num_classes)
    tab = np.full((3, 6, T), -1, dtype=np.int64)
    for b in range(3):
        tab[b, 0] = rng.choice(np.array([-1, 0, 1, num_classes - 1]), size=T)
        tab[b, 1] = rng.integers(-1, num_classes, size=T)
        for s in (2, 3):
            t = 0
            while t < T:
                n = int(rng.integers(1, 10))
                tab[b, s, t:t + n] = int(rng.integers(0, num_classes)) if rng.random() < 0.7 else -1
                t += n
        tab[b, 5] = num_classes - 1
    tab.setflags(write=False)
    return tab


@functools.lru_cache(maxsize=None)
def host_maps(T):
    stacked = tools.tablature_to_stacked_multi_pitch(random_tab(T), PROFILE)
    return stacked.astype(np.float32), stacked.max(axis=-3).astype(np.float32)


def assert_stacked_notes_equal(got, ref):
    assert list(got.keys()) == list(ref.keys())
    for s in ref:
        (gp, gi), (rp, ri) = got[s], ref[s]
        assert gp.dtype == np.float64 and gi.dtype == np.float64 and gp.shape == rp.shape and gi.shape == ri.shape == (len(rp), 2), (s, gp.shape, gi.shape)
        assert np.array_equal(gp, rp) and np.array_equal(gi, ri), s


# ------------------------------------------------------------------------------------------------------------------------------
# amtx_tab_expand
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('want', ['stacked', 'collapsed', 'both'])
@pytest.mark.parametrize('pattern', [0x00, 0xFF])
def test_expand_equals_the_host_function(monkeypatch, want, pattern):
    """Golden and random tablatures, output buffers pre-filled with zeros and with 0xFF bytes (NaN as fp32): every element is written."""
    poison = Poison(monkeypatch, pattern)
    st_on, co_on = want in ('stacked', 'both'), want in ('collapsed', 'both')
    cases = [(G[f'tab_T{T}'], G[f'stacked_T{T}'].astype(np.float32), G[f'collapsed_T{T}'].astype(np.float32)) for T in GOLDEN_LENGTHS]
    cases += [(random_tab(T),) + host_maps(T) for T in RANDOM_LENGTHS]
    for tab, stacked, collapsed in cases:
        before = poison.filled
        st, co = tools.tab_expand(torch.from_numpy(np.array(tab)).to(DEV), PROFILE, stacked=st_on, collapsed=co_on)
        assert poison.filled - before == st_on + co_on
        assert (st is None) == (not st_on) and (co is None) == (not co_on)
        if st_on:
            assert st.dtype == torch.float32 and torch.equal(st.cpu(), torch.from_numpy(stacked)), tab.shape
        if co_on:
            assert co.dtype == torch.float32 and torch.equal(co.cpu(), torch.from_numpy(collapsed)), tab.shape


def test_expand_through_the_public_functions_and_odd_views():
    tab = torch.from_numpy(np.array(random_tab(200))).to(DEV)
    stacked, collapsed = host_maps(200)
    got = tools.tablature_to_stacked_multi_pitch(tab, PROFILE)
    assert got.shape == (3, 6, 44, 200) and torch.equal(got.cpu(), torch.from_numpy(stacked))
    assert torch.equal(tools.stacked_multi_pitch_to_multi_pitch(got).cpu(), torch.from_numpy(collapsed))
    combo = transcribe.ComboEstimator([transcribe.TablatureWrapper(profile=PROFILE), transcribe.StackedMultiPitchCollapser(profile=PROFILE)])
    out = combo.process_track({tools.KEY_TABLATURE: tab[1]})
    assert out[tools.KEY_MULTIPITCH].is_cuda and torch.equal(out[tools.KEY_MULTIPITCH].cpu(), torch.from_numpy(collapsed[1]))
    # a non-contiguous tablature, one whose frames start at an address that is no multiple of 16 (the scalar-store kernel), a bare (S, T)
    assert torch.equal(tools.tab_expand(tab[:, :, ::2], PROFILE)[0].cpu(), torch.from_numpy(np.ascontiguousarray(stacked[..., ::2])))
    odd = tab.reshape(-1)[1:1 + 6 * 196].reshape(6, 196)
    ref = tools.tablature_to_stacked_multi_pitch(odd.cpu().numpy(), PROFILE)
    st, co = tools.tab_expand(odd, PROFILE, collapsed=True)
    assert st.shape == (6, 44, 196) and torch.equal(st.cpu().double(), torch.from_numpy(ref)) and torch.equal(co.cpu().double(), torch.from_numpy(ref.max(axis=0)))


def test_expand_refuses_a_profile_that_leaves_the_map():
    class Narrow(tools.GuitarProfile):
        def get_range_len(self):
            return 43                                    # class 19 of the top string would be row 43 of a 43-row map

    tab = torch.zeros((1, 6, 8), dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.AmtxError, match='do not fit'):
        tools.tab_expand(tab, Narrow(num_frets=19))


# ------------------------------------------------------------------------------------------------------------------------------
# amtx_tab_notes
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', ['float64', 'float32'])
@pytest.mark.parametrize('T', NOTE_LENGTHS)
def test_notes_equal_the_reference(T, grid):
    tab = torch.from_numpy(G[f'tab_T{T}'][None]).to(DEV)
    times = G[f'times_T{T}_{grid}']
    for window, min_dur in OPTIONS:
        got = transcribe.decode_tab_notes_batch(tab, times, PROFILE, window, min_dur)
        assert len(got) == 1
        assert_stacked_notes_equal(got[0], golden_notes(T, grid, window, min_dur))


@functools.lru_cache(maxsize=None)
def host_notes(T, window, min_dur, per_clip):
    tab = random_tab(T)
    return [transcribe._tab_to_stacked_notes_host(tab[b], clip_times(T, per_clip)[b] if per_clip else clip_times(T, per_clip), PROFILE, window, min_dur)
            for b in range(3)]


def clip_times(T, per_clip):
    """One float64 grid for the batch, or a float32 grid per clip with its own hop (a 0.05 s inhibition window is 3, 4 and 5 frames)."""
    if not per_clip:
        return np.arange(T) * HOP
    return (np.arange(T)[None, :] * np.array([HOP, 0.6 * HOP, 0.45 * HOP])[:, None]).astype(np.float32)


@pytest.mark.parametrize('per_clip', [False, True])
@pytest.mark.parametrize('T', [63, 64, 65, 200])
def test_notes_equal_the_host_classes_on_random_tablatures(T, per_clip):
    tab = torch.from_numpy(np.array(random_tab(T))).to(DEV)
    times = clip_times(T, per_clip)
    for window, min_dur in OPTIONS:
        ref = host_notes(T, window, min_dur, per_clip)
        got = transcribe.decode_tab_notes_batch(tab, times, PROFILE, window, min_dur)
        assert len(got) == 3
        for b in range(3):
            assert_stacked_notes_equal(got[b], ref[b])
        # a first buffer of ONE row: the device reports the true total and the decoder runs once more into a buffer of that size
        handle = transcribe.decode_tab_notes_batch_async(tab, times, PROFILE, window, min_dur, rows_capacity=1)
        assert handle._rows.shape[0] == 1
        again = handle.result()
        assert handle._rows.shape[0] == sum(len(p) for clip in ref for p, _ in clip.values()) > 1
        for b in range(3):
            assert_stacked_notes_equal(again[b], ref[b])


def test_notes_do_not_depend_on_old_buffer_contents(monkeypatch):
    tab = torch.from_numpy(np.array(random_tab(200))).to(DEV)
    ref = host_notes(200, 0.05, 0.0, False)
    for pattern in (0xFF, 0x7F):
        Poison(monkeypatch, pattern)
        got = transcribe.decode_tab_notes_batch(tab, clip_times(200, False), PROFILE, 0.05, 0.0)
        for b in range(3):
            assert_stacked_notes_equal(got[b], ref[b])


def test_short_grids_raise_like_the_host_classes():
    for T in (1, 2):
        with pytest.raises(ValueError):
            transcribe.decode_tab_notes_batch_async(torch.zeros((1, 6, T), dtype=torch.int64, device=DEV), np.arange(T) * HOP, PROFILE)


def test_more_than_64_classes_under_a_window_take_the_host_path():
    """Lane k of a wave holds the inhibition state of class k: a 65-class profile keeps the host classes when a window is set, and the
    kernel (which needs no such state) without one."""
    wide = tools.TablatureProfile(['E2', 'A2'], 65)
    rng = np.random.default_rng(65)
    tab = rng.choice(np.array([-1, 0, 63, 64]), size=(2, 2, 130))
    tab_d = torch.from_numpy(tab).to(DEV)
    times = np.arange(130) * HOP
    for window in (None, 0.05):
        handle = transcribe.decode_tab_notes_batch_async(tab_d, times, wide, window, None)
        assert isinstance(handle, transcribe._HostTabNotes if window is not None else transcribe._PendingTabNotes)
        got = handle.result()
        for b in range(2):
            ref = transcribe._tab_to_stacked_notes_host(tab[b], times, wide, window, None)
            assert any(p.max(initial=0) == wide.get_midi_tuning()[s] + 64 for s, (p, _) in ref.items())
            assert_stacked_notes_equal(got[b], ref)
    L = _lib.lib()
    rows, off = torch.empty((8, 3), dtype=torch.float64, device=DEV), torch.empty((5,), dtype=torch.int32, device=DEV)
    ext, rel = torch.zeros(131, dtype=torch.float64, device=DEV), torch.zeros(130, dtype=torch.int32, device=DEV)
    tuning = np.array(wide.get_midi_tuning(), dtype=np.int32)
    rc = L.amtx_tab_notes(_lib.ptr(tab_d), 2, 2, 130, _lib.ptr(tuning), 65, _lib.ptr(ext), 0, _lib.ptr(rel), 0, 0, 0.0, _lib.ptr(rows), 8, _lib.ptr(off), None)
    assert rc == _lib.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------------------------
# TabCNN end to end
# ------------------------------------------------------------------------------------------------------------------------------
def test_run_offline_batched_decodes_tabcnn_output_on_the_device():
    model = TabCNN(24, PROFILE, 1, 1, device=DEV)
    sd = synth_tabcnn_state_dict(5, dim_in=24, in_channels=1, model_complexity=1, num_groups=6, num_classes=21)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model.change_device()
    model.eval()
    T = 70
    feats = np.random.default_rng(3).random((3, 1, 24, T)).astype(np.float32)
    times = np.arange(T) * HOP
    out = run_offline_batched(feats, model, times=times, batch_size=2, decode_notes=True, keep=(tools.KEY_TABLATURE, tools.KEY_MULTIPITCH))
    assert sorted(out.keys()) == [0, 1, 2]
    notes = 0
    for i in range(3):
        assert sorted(out[i].keys()) == sorted([tools.KEY_TABLATURE, tools.KEY_MULTIPITCH, tools.KEY_NOTES])
        tab = out[i][tools.KEY_TABLATURE]
        assert tab.shape == (6, T) and tab.dtype == np.int64
        stacked = transcribe.TablatureWrapper(PROFILE).estimate({tools.KEY_TABLATURE: tab})
        collapsed = transcribe.StackedMultiPitchCollapser(PROFILE).estimate({tools.KEY_MULTIPITCH: stacked})
        assert out[i][tools.KEY_MULTIPITCH].dtype == np.float32 and np.array_equal(out[i][tools.KEY_MULTIPITCH], collapsed)
        ref = transcribe.StackedNoteTranscriber(PROFILE).estimate({tools.KEY_MULTIPITCH: stacked, tools.KEY_TIMES: times})
        assert_stacked_notes_equal(out[i][tools.KEY_NOTES], ref)
        notes += sum(len(p) for p, _ in ref.values())
    assert notes > 0
    only = run_offline_batched(feats, model, times=times, decode_notes=True, keep=())
    assert list(only[2].keys()) == [tools.KEY_NOTES] and sorted(only[2][tools.KEY_NOTES].keys()) == list(range(6))
