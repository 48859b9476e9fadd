#!/usr/bin/env python3
"""
Golden vectors of the guitar estimators: tests/golden/tab_estimators.npz.  Like tools/gen_golden.py (whose import stubs it
reuses by importing it) this runs ONLY where the reference checkout is present; the test-suite reads the fixture, never the
reference.

Recorded: what the REAL amt_tools classes -- TablatureWrapper, StackedMultiPitchCollapser, ComboEstimator,
StackedNoteTranscriber -- make of hand-made tablatures with GuitarProfile(num_frets=19): tablatures, time grids, pitch maps
and note arrays, nothing else.

Tablature rows (strings), cut to T in {1, 2, 63, 64, 65, 129, 200} frames:
  0  silent throughout
  1  different classes back to back with no gap, a note sounding at frame 0
  2  the same class struck again after a one-frame gap: after a one-frame note (the second onset is INSIDE an inhibition window
     of 0.05 s = 2.15 hops) and after a three-frame note (outside it), over and over so that some pairs straddle frames 63 | 64 | 65
  3  sticky random runs (notes of 1 .. 12 frames with silences between them)
  4  a new random class or silence EVERY frame from a small set: one-frame notes, chains of inhibited onsets
  5  the top string: fret 19 (class 19) from frame 0, class 0, silence, ...
and the last two frames of strings 1, 3 and 5 sound one class, so a note runs into the last frame.
Each with float64 and float32 time grids, inhibition_window None / 0.05 s, minimum_duration None / 0 / 0.1 s.  The reference cannot
transcribe grids of fewer than three frames (estimate_hop_length raises ValueError): for T 1 and 2 only the maps are recorded.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden                                   # noqa: E402,F401  (installs the stubs, puts the reference on sys.path)
from gen_golden import OUT, rtools                  # noqa: E402

# librosa.note_to_midi answers a LIST of note names with an ndarray (gen_golden's stand-in returns a list, enough for the profile's
# range); tools.tablature_to_stacked_multi_pitch subtracts an int from it (utils.py:2025)
sys.modules['librosa'].note_to_midi = lambda note: np.asarray(gen_golden._note_to_midi(note))
from amt_tools.transcribe import ComboEstimator, StackedMultiPitchCollapser, StackedNoteTranscriber, TablatureWrapper   # noqa: E402

LENGTHS = (1, 2, 63, 64, 65, 129, 200)
WINDOWS = (None, 0.05)
MIN_DURATIONS = (None, 0.0, 0.1)
HOP, SR = 512, 22050


def tablature(T):
    rng = np.random.default_rng(7000 + T)
    L = max(T, 8)
    tab = np.full((6, L), -1, dtype=np.int64)
    # 1: back to back, from frame 0
    t, k = 0, 3
    while t < L:
        n = int(rng.integers(1, 7))
        tab[1, t:t + n] = k
        k = (k + int(rng.integers(1, 6))) % 20
        t += n
    # 2: re-strikes after a one-frame gap; the pattern is 13 frames long, so its phase against the 64-frame chunks drifts
    pattern = [4, -1, 4, -1, -1, -1, 9, 9, 9, -1, 9, 9, -1]
    tab[2] = np.resize(np.array(pattern), L)
    # 3: sticky runs
    t = 0
    while t < L:
        n = int(rng.integers(1, 13))
        tab[3, t:t + n] = int(rng.integers(0, 20)) if rng.random() < 0.6 else -1
        t += n
    # 4: something else every frame, few classes: many onsets of one class close together
    tab[4] = rng.choice(np.array([-1, 0, 1, 19]), size=L)
    # 5: top string -- top fret from frame 0, class 0, silence
    pattern = [19, 19, 19, 0, 0, -1, 0, 19, -1, -1, 19, 0, 0, 0, 0, 0, -1]
    tab[5] = np.resize(np.array(pattern), L)
    tab = tab[:, :T].copy()
    if T >= 2:
        tab[1, -2:] = 11
        tab[3, -2:] = 2
        tab[5, -2:] = 19
    return tab


def tag(T, dt, window, min_dur):
    return f'T{T}_{np.dtype(dt).name}_w{"n" if window is None else window}_m{"n" if min_dur is None else min_dur}'


def main():
    profile = rtools.GuitarProfile(num_frets=19)
    rec = {'lengths': np.array(LENGTHS), 'windows': np.array([-1.0 if w is None else w for w in WINDOWS]),
           'min_durations': np.array([-1.0 if m is None else m for m in MIN_DURATIONS]), 'hop_length': HOP, 'sample_rate': SR,
           'midi_low': profile.low, 'midi_high': profile.high, 'midi_tuning': np.array(profile.get_midi_tuning())}
    no_notes, cases, case_offsets, all_rows, total = [], [], [], [], 0
    for T in LENGTHS:
        tab = tablature(T)
        rec[f'tab_T{T}'] = tab
        stacked = TablatureWrapper(profile=profile).process_track({rtools.KEY_TABLATURE: tab.copy()})[rtools.KEY_MULTIPITCH]
        collapsed = StackedMultiPitchCollapser(profile=profile).process_track({rtools.KEY_MULTIPITCH: stacked.copy()})[rtools.KEY_MULTIPITCH]
        combo = ComboEstimator([TablatureWrapper(profile=profile), StackedMultiPitchCollapser(profile=profile)])
        both = combo.process_track({rtools.KEY_TABLATURE: tab.copy()})
        assert sorted(both.keys()) == [rtools.KEY_MULTIPITCH, rtools.KEY_TABLATURE] and np.array_equal(both[rtools.KEY_MULTIPITCH], collapsed)
        rec[f'stacked_T{T}'], rec[f'collapsed_T{T}'] = stacked, collapsed
        as_tensor = rtools.tablature_to_stacked_multi_pitch(torch.from_numpy(tab.copy()), profile)
        assert as_tensor.dtype == torch.int64 and np.array_equal(as_tensor.numpy(), stacked)
        for dt in (np.float64, np.float32):
            times = (np.arange(T) * HOP / float(SR)).astype(dt)
            rec[f'times_T{T}_{np.dtype(dt).name}'] = times
            for window in WINDOWS:
                for min_dur in MIN_DURATIONS:
                    est = StackedNoteTranscriber(profile=profile, inhibition_window=window, minimum_duration=min_dur)
                    raw = {rtools.KEY_MULTIPITCH: stacked.copy(), rtools.KEY_TIMES: times.copy()}
                    try:
                        notes = est.process_track(raw)[rtools.KEY_NOTES]
                    except ValueError:
                        assert T < 3
                        if T not in no_notes:
                            no_notes.append(T)
                        continue
                    assert T >= 3 and sorted(notes.keys()) == list(range(6))
                    rows, off = [], [0]
                    for s in range(6):
                        pitches, intervals = notes[s]
                        assert pitches.dtype == np.float64 and intervals.dtype == np.float64, (pitches.dtype, intervals.dtype)
                        assert pitches.shape == (len(pitches),) and intervals.shape == (len(pitches), 2), (pitches.shape, intervals.shape)
                        rows.append(np.concatenate([intervals, pitches[:, None]], axis=-1))
                        off.append(off[-1] + len(pitches))
                    cases.append(tag(T, dt, window, min_dur))
                    case_offsets.append(total + np.array(off))
                    all_rows += rows
                    total += off[-1]
    # ONE array of rows [onset_s, offset_s, midi pitch] for all cases (a zip member per case would cost more than its notes): string s of
    # case c owns rows notes[note_offsets[c, s]:note_offsets[c, s + 1]]
    rec['notes'], rec['note_cases'], rec['note_offsets'] = np.concatenate(all_rows, axis=0), np.array(cases), np.stack(case_offsets)
    rec['no_notes_lengths'] = np.array(sorted(no_notes))
    rec['stacked_dtype_from_int64_tensor'] = np.array('int64')
    path = os.path.join(OUT, 'tab_estimators.npz')
    np.savez_compressed(path, **rec)
    count = lambda key: int(np.diff(rec['note_offsets'][cases.index(key)][[0, -1]])[0])      # noqa: E731
    print(path, os.path.getsize(path), 'bytes;', len(rec), 'arrays; T 200:', count(tag(200, np.float64, None, None)), 'notes,',
          count(tag(200, np.float64, 0.05, None)), 'with the window,', count(tag(200, np.float64, 0.05, 0.1)),
          'with window and minimum duration; no notes for T', rec['no_notes_lengths'])


if __name__ == '__main__':
    main()
