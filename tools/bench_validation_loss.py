#!/usr/bin/env python3
"""What the validation loss costs on one GPU.  Two measurements, no threshold.

  (a) the loop   the workload of tools/bench_validate_clips.py -- N clips x 625 frames of 8 resident synthetic tracks, the bf16 engine,
                 batches of 256 -- with LossWrapper() in front of its evaluators: evaluate.validate_clips with losses=True (the model runs
                 labelled, per-clip float64 sums come back) against losses=False (the LossWrapper warns and tracks nothing).  Wall time to a
                 device synchronise, the median of three after one warm-up, with min .. max.  On a checkout that has no `losses` keyword
                 (the commit before it) only the second call is measured: the yardstick for the losses=False route.
  (b) the kernel device events around 20 launches at 256 x 625 x 88: amtx_bce_clip_sums over whole clips; the same under the window table
                 of tracks.seam_clips(625 frames, margin 64) for 256 clips of 8 tracks; amtx_bce_logits_loss without gradient on the same
                 tensors -- it reads the same bytes and answers the batch mean.

Usage: python tools/bench_validation_loss.py [num_clips=1024] [batch=256]"""
import inspect
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from amt_tools_amd import _lib, evaluate as ev, tools, transcribe
from amt_tools_amd.synth import synth_clip, synth_labels, CLIP_FRAMES
from amt_tools_amd.tracks import LabelBank, NoteBank, TrackBank, seam_clips

args = [a for a in sys.argv[1:] if not a.startswith('--')]
N = int(args[0]) if args else 1024
B = int(args[1]) if len(args) > 1 else 256
TRACKS, REPEAT, T, HOP, SR = 8, 16, CLIP_FRAMES, 512, 22050
DEV = 'cuda:0'
HAS_LOSSES = 'losses' in inspect.signature(ev.validate_clips).parameters
warnings.simplefilter('ignore', RuntimeWarning)           # the LossWrapper's warning of the losses=False route

# ---- (a) the loop
model, mel, sd = bench.build_model(DEV, 'bf16')
model.frontend = torch.nn.Sequential(mel.frontend())
model.eval()
tracks = [np.tile(synth_clip(i), REPEAT) for i in range(TRACKS)]
bank = TrackBank(tracks, mel, DEV)
maps, truth = [], []
for i, frames in enumerate(bank.frame_counts):
    mp, on = (np.tile(m, (1, REPEAT + 1))[:, :frames] for m in synth_labels(i))
    maps.append({tools.KEY_MULTIPITCH: mp, tools.KEY_ONSETS: on})
    truth.append(transcribe.multi_pitch_to_notes(mp, np.arange(frames) * HOP / float(SR), 21, on))
labels = LabelBank(maps, bank=bank)
notes = NoteBank(truth, bank=bank)
ids = np.arange(N) % TRACKS
firsts = (np.arange(N) * 73) % (bank.frame_counts[ids] - T + 1)
bank.audio, labels._device_state(), notes._device_state()                  # resident before anything is timed


def combo():
    return ev.ComboEvaluator([ev.LossWrapper(), ev.MultipitchEvaluator(), ev.NoteEvaluator(), ev.NoteEvaluator(offset_ratio=0.2, results_key='notes-with-offsets')])


def route(losses):
    def run():
        average = ev.validate_clips(bank, labels, notes, model, combo(), ids, firsts, T, batch_size=B, **({'losses': True} if losses else {}))
        torch.cuda.synchronize()
        return average
    return run


def timed(fn):
    result = fn()
    dts = []
    for _ in range(3):
        t0 = time.perf_counter()
        result = fn()
        dts.append(time.perf_counter() - t0)
    return result, sorted(dts)


print(f'(a) {N} clips x {T} frames of {TRACKS} resident tracks, batches of {B}, bf16 engine; validate_clips has the losses keyword: {HAS_LOSSES}')
off, dts = timed(route(False))
print(f'  losses=False: {dts[1] * 1e3:8.1f} ms median of 3 (min {dts[0] * 1e3:.1f}, max {dts[2] * 1e3:.1f}); loss tracked: {off[tools.KEY_LOSS]}')
if HAS_LOSSES:
    on, dts = timed(route(True))
    print(f'  losses=True : {dts[1] * 1e3:8.1f} ms median of 3 (min {dts[0] * 1e3:.1f}, max {dts[2] * 1e3:.1f}); loss tracked: {on[tools.KEY_LOSS]}')
    print(f'  the other leaves score the same either way: {all(on[k] == off[k] for k in off if k != tools.KEY_LOSS)}')

# ---- (b) the kernel
if HAS_LOSSES:
    KB, KEYS, LAUNCHES = 256, 88, 20
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(KB, T, KEYS, generator=g) * 4).to(DEV)
    y = (torch.rand(KB, KEYS, T, generator=g) < 0.1).float().to(DEV)
    plan = seam_clips(np.full(TRACKS, T + (KB // TRACKS - 1) * (T - 128)), T, 64)
    assert len(plan.track_ids) == KB
    table = np.ascontiguousarray(plan.kept[:, 1:3], dtype=np.int32)
    table_dev = torch.from_numpy(table).to(DEV)
    sums = torch.empty(KB, dtype=torch.float64, device=DEV)
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    ws = _lib.alloc_workspace(max(int(_lib.call('amtx_bce_clip_sums_workspace_bytes', KB, T, KEYS)), int(_lib.call('amtx_bce_logits_loss_workspace_bytes', KB, T, KEYS))), DEV)

    def events(launch):
        launch()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(LAUNCHES):
            launch()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) * 1e3 / LAUNCHES

    whole = events(lambda: _lib.call('amtx_bce_clip_sums', x, KEYS, y, None, None, None, KB, T, KEYS, sums, ws, ws.numel(), device=DEV))
    windowed = events(lambda: _lib.call('amtx_bce_clip_sums', x, KEYS, y, None, table, table_dev, KB, T, KEYS, sums, ws, ws.numel(), device=DEV))
    mean = events(lambda: _lib.call('amtx_bce_logits_loss', x, KEYS, y, None, KB, T, KEYS, loss, None, ws, ws.numel(), device=DEV))
    kept = table[:, 1].sum() / float(KB * T)
    print(f'(b) {KB} x {T} x {KEYS}, device events around {LAUNCHES} launches, microseconds per launch')
    print(f'  amtx_bce_clip_sums, whole clips            : {whole:8.1f}')
    print(f'  amtx_bce_clip_sums, seam windows (margin 64): {windowed:8.1f}   ({kept * 100:.1f} % of the frames kept)')
    print(f'  amtx_bce_logits_loss, no gradient           : {mean:8.1f}')
