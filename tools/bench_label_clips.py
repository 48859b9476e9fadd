#!/usr/bin/env python3
"""Label clips from a LabelBank against the host slicing and upload they replace, for the two training recipes:

  piano   : Onsets & Frames, 8 clips x 625 frames, multi_pitch / onsets / offsets of 88 rows, float32   (5.3 MB per batch)
  tabcnn  : TabCNN, 30 clips x 200 frames, a 6-row int64 tablature plus the 44-row float32 multi_pitch

  (a) bank    : labels.clips(ids, first_frames, T)          (host validation, a (B, 3) descriptor upload, one launch per dtype kind)
  (b) upload  : NumPy slices of the whole-track host maps, stacked into pinned memory per key, .to(device)

Four synthetic tracks of two minutes; the maps come from cache.notes_to_* on synthetic notes (the tablature: per string, the fret of the
string's sounding note).  A warm-up, then REPEATS timings with the two routes alternating in one process: the host clock around each
route, the device synchronised before and after, because both routes are host work as much as device work.  Medians and the min .. max
spread are printed as one JSON line per recipe, with the label bank's bytes and its runs per track.  No threshold: the numbers go into
DESIGN.md 6f."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np      # noqa: E402
import torch            # noqa: E402

from amt_tools_amd import cache, tools               # noqa: E402
from amt_tools_amd.tracks import LabelBank           # noqa: E402

HOP = 512
RECIPES = {'piano': (8, 625, 16000), 'tabcnn': (30, 200, 22050)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {'median_ms': round(float(np.median(ms)), 4), 'min_ms': round(float(ms[0]), 4), 'max_ms': round(float(ms[-1]), 4)}


def synth_notes(rng, profile, seconds, per_second):
    n = int(seconds * per_second)
    onsets = np.sort(rng.uniform(0.0, seconds - 0.1, n))
    return rng.integers(profile.low, profile.high + 1, n).astype(np.float64), np.stack([onsets, onsets + rng.uniform(0.05, 1.5, n)], axis=1)


def piano_maps(rng, seconds, sr):
    profile = tools.PianoProfile()
    times = np.arange(1 + int(seconds * sr) // HOP) * HOP / sr
    pitches, intervals = synth_notes(rng, profile, seconds, 8.0)
    return {tools.KEY_MULTIPITCH: cache.notes_to_multi_pitch(pitches, intervals, times, profile),
            tools.KEY_ONSETS: cache.notes_to_onsets(pitches, intervals, times, profile),
            tools.KEY_OFFSETS: cache.notes_to_offsets(pitches, intervals, times, profile)}


def tabcnn_maps(rng, seconds, sr):
    profile = tools.GuitarProfile(num_frets=19)
    times = np.arange(1 + int(seconds * sr) // HOP) * HOP / sr
    tab, collapsed = [], np.zeros((profile.get_range_len(), len(times)))
    for open_pitch in profile.get_midi_tuning():
        pitches, intervals = synth_notes(rng, profile, seconds, 1.5)
        on_string = (pitches >= open_pitch) & (pitches <= open_pitch + 19)
        rows = cache.notes_to_multi_pitch(pitches[on_string], intervals[on_string], times, profile)
        frets = rows[open_pitch - profile.low:open_pitch - profile.low + 20]
        tab.append(np.where(frets.any(axis=0), frets.argmax(axis=0), -1))          # one sounding fret per string and frame, -1 = silent
        collapsed = np.maximum(collapsed, rows)
    return {tools.KEY_TABLATURE: np.stack(tab).astype(np.int64), tools.KEY_MULTIPITCH: collapsed}


def run(name, args, dev):
    B, T, sr = RECIPES[name]
    rng = np.random.default_rng(0)
    make = piano_maps if name == 'piano' else tabcnn_maps
    maps = [make(rng, args.minutes * 60 - i, sr) for i in range(args.tracks)]
    labels = LabelBank(maps, device=dev)
    dtypes = {key: (np.float32, torch.float32) if a.dtype.kind == 'f' else (np.int64, torch.int64) for key, a in maps[0].items()}
    pinned = {key: torch.empty((B, a.shape[0], T), dtype=dtypes[key][1]).pin_memory() for key, a in maps[0].items()}

    def upload(ids, firsts):
        out = {}
        for key, buf in pinned.items():
            view = buf.numpy()
            for b, (k, f) in enumerate(zip(ids, firsts)):
                view[b] = maps[k][key][:, f:f + T]                                  # slice, convert and stack in one pass
            out[key] = buf.to(dev, non_blocking=True)
        return out

    draws = []
    for _ in range(args.warmup + args.repeats):
        ids = rng.integers(0, len(labels), size=B)
        draws.append((ids, np.array([rng.integers(0, labels.frame_counts[k] - T + 1) for k in ids])))
    t = {'bank': [], 'upload': []}
    for i, (ids, firsts) in enumerate(draws):
        ms_bank, got = timed(lambda: labels.clips(ids, firsts, T))
        ms_upload, want = timed(lambda: upload(ids, firsts))
        for key in want:                                                            # the two routes hold the same bits
            a, b = (x[key].view(torch.int32) if x[key].dtype == torch.float32 else x[key] for x in (got, want))
            assert torch.equal(a, b), key
        if i >= args.warmup:
            t['bank'].append(ms_bank)
            t['upload'].append(ms_upload)
    batch_bytes = sum(B * a.shape[0] * T * np.dtype(dtypes[key][0]).itemsize for key, a in maps[0].items())
    host_bytes = sum(a.shape[0] * a.shape[1] * np.dtype(dtypes[key][0]).itemsize for m in maps for key, a in m.items())
    return {'bench': 'label_clips', 'recipe': name, 'clips': B, 'frames': T, 'tracks': len(labels), 'frames_per_track': labels.frame_counts.tolist(),
            'rows_per_track': labels.rows_total, 'repeats': args.repeats, 'batch_bytes': int(batch_bytes),
            'label_bank_device_bytes': labels.nbytes, 'whole_maps_bytes': int(host_bytes), 'runs_per_track': labels.runs_per_track.tolist(),
            'a_clips_from_label_bank': stats(t['bank']), 'b_slice_stack_pinned_upload': stats(t['upload'])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tracks', type=int, default=4)
    ap.add_argument('--minutes', type=float, default=2.0, help='length of every synthetic track')
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--recipes', nargs='+', default=sorted(RECIPES), choices=sorted(RECIPES))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    for name in args.recipes:
        print(json.dumps(run(name, args, dev)), flush=True)


if __name__ == '__main__':
    main()
