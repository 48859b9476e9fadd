#!/usr/bin/env python3
"""A 5 x 5 grid of onset and frame thresholds over whole resident tracks, three ways, on one GPU -- the workload of
tools/bench_run_tracks_exact.py: eight synthetic tracks of --frames frames, bf16 OnsetsFrames as bench.py builds
it, 625-frame clips, margin 3, a MultipitchEvaluator and two NoteEvaluators; ground truth is the model's own transcription, perturbed.

  (a) sweep_tracks     one exact pass with logits; per track two probability maps, ONE amtx_eval_multipitch_grid_counts, ONE
                       amtx_notes_decode_grid over the 25 pairs, amtx_notes_rows, one amtx_eval_notes_match of 25 groups per evaluator
  (b) composition      the same pass and logits; then per pair and track amtx_pianoroll_fwd at the thresholds, amtx_notes_decode +
                       amtx_notes_rows, amtx_eval_multipitch_counts, amtx_eval_notes_match: what needs no new kernel
  (c) validate_tracks  ONE validate_tracks(exact=True): the cost of a single pair

Times: wall time to a device synchronise, median (min .. max) of --repeat runs after one warm-up each, the routes alternating in one
process.  Also: amtx_notes_decode_grid alone on one track's maps (device time between two events), for the pairs-per-wave tile the
process runs with (AMTX_NOTES_GRID_TILE = 1, 2, 4 or 8; default 1).  Prints; no threshold.
Usage: python tools/bench_sweep_tracks.py [--frames 5000] [--repeat 5]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from amt_tools_amd import _lib, evaluate as ev, inference, tools, transcribe
from amt_tools_amd.inference import run_tracks
from amt_tools_amd.synth import synth_clip
from amt_tools_amd.tracks import LabelBank, NoteBank, TrackBank

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=5000)
ap.add_argument('--repeat', type=int, default=5)
args = ap.parse_args()
DEV, TRACKS, T, MARGIN, HOP = 'cuda:0', 8, 625, 3, 512
ONSET_THR, FRAME_THR = (0.3, 0.4, 0.5, 0.6, 0.7), (0.3, 0.4, 0.5, 0.6, 0.7)

model, mel, _ = bench.build_model(DEV, 'bf16')
model.frontend = torch.nn.Sequential(mel.frontend())
model.eval()
SR = mel.get_sample_rate()
samples = args.frames * HOP - 1
bank = TrackBank([np.tile(y, -(-samples // len(y)))[:samples] for y in (synth_clip(i) for i in range(TRACKS))], mel, DEV)
assert bank.frame_counts.tolist() == [args.frames] * TRACKS, bank.frame_counts
bank.audio                                                                 # resident before anything is timed

# ground truth: the model's own notes with a third dropped, a third moved by a hop and random notes added
own = run_tracks(bank, model, T, MARGIN, keep=(), decode_notes=True, exact=True)
rng = np.random.default_rng(8)
truth = []
for t in range(TRACKS):
    rows = np.array(own[t][tools.KEY_NOTES], dtype=np.float64).reshape(-1, 3)
    rows = rows[rng.random(len(rows)) < 0.67]
    rows[:, 0] += (rng.random(len(rows)) < 0.33) * HOP / SR
    rows[:, 1] = np.maximum(rows[:, 1], rows[:, 0])
    onsets = rng.integers(0, args.frames - 1, 40) * HOP / SR
    truth.append(np.concatenate([rows, np.stack([onsets, onsets + rng.integers(1, 30, 40) * HOP / SR, rng.integers(21, 109, 40).astype(np.float64)], axis=1)]))
times = [np.arange(args.frames) * HOP / SR] * TRACKS
labels = LabelBank.from_notes([(r[:, 2], r[:, :2]) for r in truth], times, tools.PianoProfile(), keys=(tools.KEY_MULTIPITCH,), bank=bank)
notes = NoteBank(truth, bank=bank)


def combo():
    return ev.ComboEvaluator([ev.MultipitchEvaluator(), ev.NoteEvaluator(), ev.NoteEvaluator(offset_ratio=0.2, results_key='notes-with-offsets')])


def sweep():
    out = ev.sweep_tracks(bank, labels, notes, model, combo(), T, MARGIN, ONSET_THR, FRAME_THR)
    torch.cuda.synchronize()
    return out


def composition():
    """Route (b): per pair the existing kernels on rolls cut from the same logits; the counts come back per pair."""
    e = combo()
    frame_e, note_es = e.evaluators[0], e.evaluators[1:]
    tracked = {}
    with torch.no_grad():
        mine, _, logits = inference._exact_tracks(bank, model, T, MARGIN, want_logits=True)
        grid = inference._frame_times(model, args.frames)
        for a in ONSET_THR:
            for b in FRAME_THR:
                cell = [dict() for _ in e.evaluators]
                for j, t in enumerate(mine.tolist()):
                    on = inference.logits_to_map(logits[j][tools.KEY_ONSETS], a)
                    mp = inference.logits_to_map(logits[j][tools.KEY_MULTIPITCH], b)
                    frame = frame_e.counts_batch(mp, labels.clips([t], [0], args.frames)[tools.KEY_MULTIPITCH])
                    rows, offsets = transcribe.decode_notes_batch_async(on, mp, grid, model.profile.low).device_rows()
                    whole = notes.whole([t])
                    matched = [n.match_batch((rows, offsets), (whole.rows, whole.offsets))[0] for n in note_es]
                    host = [frame.cpu().numpy()[0]] + [m.cpu().numpy() for m in matched]
                    for k, (leaf, counts) in enumerate(zip(e.evaluators, host)):
                        cell[k] = ev.append_results(cell[k], leaf.results_from_counts(counts))
                average = {}
                for leaf, res in zip(e.evaluators, cell):
                    ev.ComboEvaluator._merge(average, leaf.results_key, ev.average_results(res))
                tracked[(a, b)] = average
    torch.cuda.synchronize()
    return tracked


def single():
    out = ev.validate_tracks(bank, labels, notes, model, combo(), T, MARGIN, exact=True)
    torch.cuda.synchronize()
    return out


routes = [('(a) sweep_tracks          ', sweep), ('(b) per-pair composition  ', composition), ('(c) one validate_tracks   ', single)]
results, walls = {}, {name: [] for name, _ in routes}
for name, fn in routes:
    results[name] = fn()                                                   # warm-up: every shape of the timed window
for _ in range(args.repeat):
    for name, fn in routes:                                                # alternating
        t0 = time.perf_counter()
        fn()
        walls[name].append(time.perf_counter() - t0)
P = len(ONSET_THR) * len(FRAME_THR)
print(f'{TRACKS} resident tracks of {args.frames} frames, bf16 OnsetsFrames, clips of {T} frames, margin {MARGIN}, {len(ONSET_THR)} x {len(FRAME_THR)} thresholds')
med = {}
for name, _ in routes:
    dts = sorted(walls[name])
    med[name] = dts[len(dts) // 2]
    print(f'  {name}: {med[name] * 1e3:8.1f} ms median of {len(dts)} (min {dts[0] * 1e3:.1f}, max {dts[-1] * 1e3:.1f})')
a, b, c = (med[name] for name, _ in routes)
print(f'  (a) takes {a / b:.2f} of (b) and {a / c:.2f} of (c), {P * c / a:.1f} times faster than {P} runs of (c): it ' + ('beats' if a < b else 'LOSES to') + ' the composition')
same = results[routes[0][0]] == results[routes[1][0]]
print(f'  (a) and (b) hold the same results in all {P} cells: {same}; cell (0.5, 0.5) of (a) is (c): {results[routes[0][0]][(0.5, 0.5)] == results[routes[2][0]]}')
f1 = [results[routes[0][0]][(x, y)][tools.KEY_NOTES][tools.KEY_F1] for x in ONSET_THR for y in FRAME_THR]
print(f'  note F1 over the grid: {min(f1):.4f} .. {max(f1):.4f}')

# the grid decoder alone, on one track
with torch.no_grad():
    _, _, logits = inference._exact_tracks(bank, model, T, MARGIN, track_ids=[0], want_logits=True)
on_prob, mp_prob = (inference.logits_to_map(logits[0][key], -1.0) for key in (tools.KEY_ONSETS, tools.KEY_MULTIPITCH))
pairs_d = torch.tensor([[x, y] for x in ONSET_THR for y in FRAME_THR], dtype=torch.float32).to(DEV)
cap = args.frames // 2 + 2
events = torch.empty((P * 88, cap, 2), dtype=torch.int32, device=DEV)
counts = torch.empty((P * 88,), dtype=torch.int32, device=DEV)
spans = []
for i in range(25):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    _lib.call('amtx_notes_decode_grid', on_prob, mp_prob, 1, 88, args.frames, pairs_d, P, cap, events, counts, device=DEV)
    stop.record()
    stop.synchronize()
    if i >= 5:
        spans.append(start.elapsed_time(stop) * 1e3)
spans.sort()
print(f'  amtx_notes_decode_grid alone, {P} pairs x 88 keys x {args.frames} frames, tile {os.environ.get("AMTX_NOTES_GRID_TILE", "1 (default)")}: '
      f'{spans[len(spans) // 2]:.1f} us median of {len(spans)} (min {spans[0]:.1f}, max {spans[-1]:.1f}), {int(counts.sum())} events')
