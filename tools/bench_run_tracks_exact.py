#!/usr/bin/env python3
"""Whole resident tracks, three ways, on one GPU -- the workload of DESIGN.md section 6i: eight synthetic tracks of --frames frames
(synth_clip audio tiled), bf16 OnsetsFrames as bench.py builds it, 625-frame clips, every track's onset and pitch maps brought to the host.

  (w) whole        each track whole as a batch of one through run_on_batch: the exact whole-track result, 2 x L_t dependent steps per track
  (a) run_tracks   segment-wise, margin 16: overlapped clips through the whole engine, kept columns stitched
  (x) exact=True   margin 3: the clips run the engine's acoustic phase, both recurrences run once over all whole tracks

Times: wall time to a device synchronise, median (min .. max) of --repeat runs after one warm-up each, the routes alternating in one
process.  For (x) also: the piano-roll cells and the logits that differ from (w)'s.  Prints; no threshold.
Usage: python tools/bench_run_tracks_exact.py [--frames 5000] [--repeat 5]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from amt_tools_amd import tools
from amt_tools_amd.inference import KEY_LOGITS, run_tracks
from amt_tools_amd.synth import synth_clip
from amt_tools_amd.tracks import TrackBank, seam_clips

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=5000)
ap.add_argument('--repeat', type=int, default=5)
args = ap.parse_args()
DEV, TRACKS, T, HOP = 'cuda:0', 8, 625, 512
KEYS = (tools.KEY_ONSETS, tools.KEY_MULTIPITCH)

model, mel, _ = bench.build_model(DEV, 'bf16')
model.frontend = torch.nn.Sequential(mel.frontend())
model.eval()
samples = args.frames * HOP - 1
bank = TrackBank([np.tile(y, -(-samples // len(y)))[:samples] for y in (synth_clip(i) for i in range(TRACKS))], mel, DEV)
assert bank.frame_counts.tolist() == [args.frames] * TRACKS, bank.frame_counts
bank.audio                                                                 # resident before anything is timed


def whole(logits=False):
    out = {}
    with torch.no_grad():
        for t in range(TRACKS):
            clips = bank.clips([t], [0], args.frames)
            if logits:                                                     # the engine's raw logits, the features staged as run_on_batch stages them
                model.__dict__['_in_run_on_batch'] = True
                try:
                    raw = model(model.pre_proc({tools.KEY_AUDIO: clips})[tools.KEY_FEATS])
                finally:
                    model.__dict__.pop('_in_run_on_batch', None)
                    model.__dict__.pop('_engine_out', None)
                out[t] = {key: raw[key][0].cpu().numpy() for key in KEYS}
            else:
                preds = model.run_on_batch({tools.KEY_AUDIO: clips})
                out[t] = {key: preds[key][0].cpu().numpy() for key in KEYS}
    torch.cuda.synchronize()
    return out


def tracks(margin, keep=KEYS, **kwargs):
    out = run_tracks(bank, model, T, margin, keep=keep, **kwargs)
    torch.cuda.synchronize()
    return out


routes = [('(w) whole, batch of one   ', whole), ('(a) run_tracks margin 16  ', lambda: tracks(16)), ('(x) exact=True, margin 3  ', lambda: tracks(3, exact=True))]
results, times = {}, {name: [] for name, _ in routes}
for name, fn in routes:
    results[name] = fn()                                                   # warm-up: every shape of the timed window
for _ in range(args.repeat):
    for name, fn in routes:                                                # alternating
        t0 = time.perf_counter()
        fn()
        times[name].append(time.perf_counter() - t0)
print(f'{TRACKS} resident tracks of {args.frames} frames, bf16 OnsetsFrames, clips of {T} frames, batches of 256')
for (name, _), m in zip(routes, (None, 16, 3)):
    dts = sorted(times[name])
    clips = '' if m is None else f', {len(seam_clips(bank.frame_counts, T, m).track_ids)} clips'
    print(f'  {name}: {dts[len(dts) // 2] * 1e3:8.1f} ms median of {len(dts)} (min {dts[0] * 1e3:.1f}, max {dts[-1] * 1e3:.1f}){clips}')
med = {name: sorted(times[name])[len(times[name]) // 2] for name, _ in routes}
w, a, x = (med[name] for name, _ in routes)
print(f'  (x) takes {x / w:.2f} of (w) and {x / a:.2f} of (a): it ' + ('beats' if x < w else 'LOSES to') + ' the whole-track route')

reference = results[routes[0][0]]
cells = lambda got: {key: sum(int((got[t][key] != reference[t][key]).sum()) for t in range(TRACKS)) for key in KEYS}      # noqa: E731
size = sum(reference[t][KEYS[0]].size for t in range(TRACKS))
for name in (routes[1][0], routes[2][0]):
    d = cells(results[name])
    print(f'  {name.strip()} against (w): {d[KEYS[0]]} of {size} onset cells differ, {d[KEYS[1]]} of {size} pitch cells')
raw_w, raw_x = whole(logits=True), tracks(3, keep=KEYS + (KEY_LOGITS,), exact=True)
for key in KEYS:
    diff = [np.abs(raw_x[t][KEY_LOGITS][key] - raw_w[t][key]) for t in range(TRACKS)]
    bits = sum(int((raw_x[t][KEY_LOGITS][key].view(np.uint32) != raw_w[t][key].view(np.uint32)).sum()) for t in range(TRACKS))
    print(f'  (x) {key} logits against (w): {bits} of {size} differ in their bits, max abs difference {max(float(d.max()) for d in diff):.3e}')
