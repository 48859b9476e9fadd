#!/usr/bin/env python3
"""
Golden vectors of note slicing: tests/golden/note_clips.npz.  Like tools/gen_golden_tab.py (and through tools/gen_golden.py's import
stubs) this runs ONLY where the reference checkout is present; the test-suite reads the fixture, never the reference.  Data only.

Recorded:
* `notes_T{i}`: batched notes (N, 3) [onset_s, offset_s, pitch] of three tracks (300, 65 and 0 notes), times exactly on the
  k * hop / sample_rate grid so that `offset > start` and `onset <= stop` both meet equality, plus a few zero-length notes;
  `stack_T{i}_S{s}`: the same tracks dealt onto 6 strings (pitch % 6) as stacked notes.
* `windows` (W, 3): (track, start_time, stop_time) of every recorded slice, and for relative_times r in (0, 1)
  `sliced_r{r}` / `sliced_r{r}_offsets`: what the REAL amt_tools.tools.slice_batched_notes returned for the batched tracks, row arrays
  back to back with an offsets table; `stacked_r{r}` / `stacked_r{r}_offsets`: the same per (window, string) for the stacked tracks.
* `window_cases` (C, 4): (first_frame, num_frames, hop_length, sample_rate), and `sec_mel` / `sec_cqt` / `sec_cqt48` (C, 2): sec_start,
  sec_stop by the arithmetic of TranscriptionDataset.get_track_data (amt_tools/datasets/common.py:116, :343-358, snap_to_frame) with the
  own get_sample_range of MelSpec, CQT(192 bins, 24 per octave) and CQT(48 bins, 12 per octave), plus `seq_*`: the seq_length each gives.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden                                   # noqa: E402,F401  (installs the stubs, puts the reference on sys.path)
from gen_golden import OUT, rtools                  # noqa: E402
from amt_tools.features import CQT, MelSpec         # noqa: E402
from amt_tools.features import vqt as rvqt          # noqa: E402

HOP, SR = 512, 22050
C1_HZ = 32.70319566257483                           # librosa.note_to_hz('C1')


def _early_downsample_count(nyquist, filter_cutoff, hop_length, n_octaves):
    """librosa.core.constantq.__early_downsample_count as published."""
    count1 = max(0, int(np.ceil(np.log2(nyquist / filter_cutoff)) - 1) - 1)
    twos, h = 0, int(hop_length)
    while h > 0 and h % 2 == 0:
        twos, h = twos + 1, h // 2
    return min(count1, max(0, twos - n_octaves + 1))


# The three librosa helpers VQT.get_early_ds_count calls (features/vqt.py:81-98) are short and documented; their behaviour is restated
# here so that the reference's own get_sample_range runs (the stub would hand back MagicMocks)
sys.modules['librosa'].cqt_frequencies = lambda n_bins, fmin, bins_per_octave=12, tuning=0.0: fmin * 2.0 ** (np.arange(n_bins) / float(bins_per_octave))
rvqt.window_bandwidth = lambda window: {'hann': 1.50018310546875}[window]
rvqt.early_downsample_count = _early_downsample_count
SIZES = (300, 65, 0)
FRAMES = 400


def track_notes(seed, n):
    rng = np.random.default_rng(seed)
    on = rng.integers(0, FRAMES - 1, n)
    length = rng.integers(0, 40, n)                 # some zero-length notes
    off = np.minimum(on + length, FRAMES)
    return np.stack([on * HOP / SR, off * HOP / SR, rng.integers(40, 77, n).astype(np.float64)], axis=1)


def main():
    rec = {'hop_length': HOP, 'sample_rate': SR, 'sizes': np.array(SIZES)}
    tracks = [track_notes(100 + i, n) for i, n in enumerate(SIZES)]
    windows = []
    for i, notes in enumerate(tracks):
        rec[f'notes_T{i}'] = notes
        for s in range(6):
            rec[f'stack_T{i}_S{s}'] = notes[notes[:, 2] % 6 == s]
        for first, frames in ((0, 40), (17, 40), (100, 1), (360, 40), (3, 397), (200, 64)):
            windows.append((i, first * HOP / SR, (first * HOP + frames * HOP - 1) / SR))
        windows.append((i, 50 * HOP / SR, 90 * HOP / SR))              # both edges exactly on note times
    rec['windows'] = np.array(windows, dtype=np.float64)
    for relative in (False, True):
        flat, off, sflat, soff = [], [0], [], [0]
        for track, start, stop in windows:
            got = rtools.slice_batched_notes(tracks[int(track)].copy(), start, stop, relative)
            flat.append(got)
            off.append(off[-1] + len(got))
            for s in range(6):
                got = rtools.slice_batched_notes(rec[f'stack_T{int(track)}_S{s}'].copy(), start, stop, relative)
                sflat.append(got)
                soff.append(soff[-1] + len(got))
        r = int(relative)
        rec[f'sliced_r{r}'], rec[f'sliced_r{r}_offsets'] = np.concatenate(flat, axis=0), np.array(off)
        rec[f'stacked_r{r}'], rec[f'stacked_r{r}_offsets'] = np.concatenate(sflat, axis=0), np.array(soff)
    cases = [(f, n, hop, sr) for hop, sr in ((512, 22050), (512, 16000), (256, 44100)) for n in (1, 40, 200, 625) for f in (0, 1, 7, 1000, 123457)]
    rec['window_cases'] = np.array(cases, dtype=np.int64)
    for name, make in (('mel', lambda hop, sr: MelSpec(sample_rate=sr, hop_length=hop, n_mels=229, n_fft=2048)),
                       ('cqt', lambda hop, sr: CQT(sample_rate=sr, hop_length=hop, fmin=C1_HZ, n_bins=192, bins_per_octave=24)),
                       # four octaves from C1: three early downsamples, so the sample range ends 8 samples before num_frames * hop_length
                       ('cqt48', lambda hop, sr: CQT(sample_rate=sr, hop_length=hop, fmin=C1_HZ, n_bins=48, bins_per_octave=12))):
        secs, seqs = [], []
        for first, frames, hop, sr in cases:
            module = make(hop, sr)
            seq_length = max(module.get_sample_range(frames))              # datasets/common.py:116
            sample_start = first * module.hop_length                       # :343, :348 (snap_to_frame)
            sample_end = sample_start + seq_length                         # :351
            secs.append((sample_start / module.sample_rate, sample_end / module.sample_rate))        # :357-358
            seqs.append(int(seq_length))
        rec[f'sec_{name}'], rec[f'seq_{name}'] = np.array(secs, dtype=np.float64), np.array(seqs, dtype=np.int64)
    path = os.path.join(OUT, 'note_clips.npz')
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), 'bytes;', len(rec), 'arrays;', len(windows), 'windows;', len(rec['sliced_r1']), 'sliced rows;',
          'seq_length 625 frames hop 512:', int(rec['seq_mel'][cases.index((0, 625, 512, 22050))]))


if __name__ == '__main__':
    main()
