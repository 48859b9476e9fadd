#!/usr/bin/env python3
"""Whole resident tracks, two ways, on one GPU: eight synthetic tracks of --frames frames (synth_clip audio tiled), bf16 OnsetsFrames as
bench.py builds it, every track's onset and pitch maps and its decoded notes brought to the host.

  (a) run_tracks   inference.run_tracks: 625-frame overlapped clips (tracks.seam_clips) through the batched driver, the kept columns
                   stitched into whole-track maps on the device (amtx_stitch_clips); margins 0, 16, 64 and 128
  (w) whole        what the package offered before: each track whole as a batch of one through run_on_batch (the exact whole-track
                   result).  If the engine refuses the length with an error, the length is halved until it is accepted, all routes use
                   that length, and the refused lengths are printed; nothing longer is tried afterwards.

  (b) per margin, the deviation of (a), segment-wise inference, from (w): the share of roll cells that differ, and the note F1 of (a)'s
      notes scored against (w)'s notes (NoteEvaluator, onsets only, and with offset_ratio 0.2), mean over the tracks.  Synthetic
      weights: the rolls are no transcription of the audio, only the two routes' outputs are compared.
  (c) the stitch kernel alone: device events around 20 amtx_stitch_clips launches back to back, per launch, for a batch of 256 x 88 x 625 float32 (the plan of
      eight 16 032-frame tracks at margin 64: every clip keeps 497 to 561 columns), against dst.copy_(src) of as many bytes.

Times: wall time to a device synchronise, median (min .. max) of --repeat runs after one warm-up each, the routes alternating.  Prints; no
threshold.  Usage: python tools/bench_run_tracks.py [--frames 5000] [--repeat 5]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from amt_tools_amd import _lib, evaluate as ev, tools, transcribe
from amt_tools_amd.inference import run_tracks
from amt_tools_amd.synth import synth_clip
from amt_tools_amd.tracks import TrackBank, TrackMaps, seam_clips

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=5000)
ap.add_argument('--repeat', type=int, default=5)
args = ap.parse_args()
DEV, TRACKS, T, HOP, MARGINS = 'cuda:0', 8, 625, 512, (0, 16, 64, 128)
KEYS = (tools.KEY_ONSETS, tools.KEY_MULTIPITCH)

model, mel, _ = bench.build_model(DEV, 'bf16')
model.frontend = torch.nn.Sequential(mel.frontend())
model.eval()


def make_bank(frames):
    samples = frames * HOP - 1
    tracks = [np.tile(y, -(-samples // len(y)))[:samples] for y in (synth_clip(i) for i in range(TRACKS))]
    bank = TrackBank(tracks, mel, DEV)
    assert bank.frame_counts.tolist() == [frames] * TRACKS, bank.frame_counts
    bank.audio                                                             # resident before anything is timed
    return bank


def whole(bank):
    """Route (w): {track: {key: (88, L) host array, KEY_NOTES: (K, 3)}}."""
    out = {}
    with torch.no_grad():
        for t in range(len(bank)):
            preds = model.run_on_batch({tools.KEY_AUDIO: bank.clips([t], [0], int(bank.frame_counts[t]))})
            notes = transcribe.decode_notes_for(preds, model, None)
            out[t] = {key: preds[key][0].cpu().numpy() for key in KEYS}
            out[t][tools.KEY_NOTES] = notes.result()[0]
    torch.cuda.synchronize()
    return out


def stitched(bank, margin):
    out = run_tracks(bank, model, T, margin, decode_notes=True, keep=KEYS)
    torch.cuda.synchronize()
    return out


frames, refused = args.frames, []
while True:
    bank = make_bank(frames)
    try:
        reference = whole(bank)
        break
    except _lib.AmtxError as e:                                            # a refusal with an error text; anything else ends the run
        refused.append((frames, str(e)))
        if frames <= T:
            raise
        frames = max(T, frames // 2)
for n, text in refused:
    print(f'the engine refused whole tracks of {n} frames: {text}')
print(f'{TRACKS} resident tracks of {frames} frames, bf16 OnsetsFrames, clips of {T} frames, batches of 256'
      + (f' (largest whole-track length accepted of the halving from {args.frames}; nothing longer tried)' if refused else ''))

routes = [('(w) whole, batch of one', lambda: whole(bank))] + [(f'(a) run_tracks margin {m:3d}', (lambda m=m: stitched(bank, m))) for m in MARGINS]
results, times = {}, {name: [] for name, _ in routes}
for name, fn in routes:
    results[name] = fn()                                                   # warm-up: every shape of the timed window
for _ in range(args.repeat):
    for name, fn in routes:                                                # alternating
        t0 = time.perf_counter()
        fn()
        times[name].append(time.perf_counter() - t0)
for (name, _), m in zip(routes, (None,) + MARGINS):
    dts = sorted(times[name])
    clips = '' if m is None else f', {len(seam_clips(bank.frame_counts, T, m).track_ids)} clips'
    print(f'  {name}: {dts[len(dts) // 2] * 1e3:8.1f} ms median of {len(dts)} (min {dts[0] * 1e3:.1f}, max {dts[-1] * 1e3:.1f}){clips}')

# (b) deviation from whole-track inference
for (name, _), m in zip(routes[1:], MARGINS):
    got = results[name]
    differ = {key: sum(int((got[t][key] != reference[t][key]).sum()) for t in range(TRACKS)) / sum(reference[t][key].size for t in range(TRACKS)) for key in KEYS}
    f1 = []
    for e in (ev.NoteEvaluator(), ev.NoteEvaluator(offset_ratio=0.2)):
        f1.append(float(np.mean([e.evaluate(np.asarray(got[t][tools.KEY_NOTES]).reshape(-1, 3), np.asarray(reference[t][tools.KEY_NOTES]).reshape(-1, 3))[tools.KEY_F1]
                                 for t in range(TRACKS)])))
    print(f'  margin {m:3d} against whole tracks: onset cells that differ {differ[tools.KEY_ONSETS]:.6f}, pitch cells {differ[tools.KEY_MULTIPITCH]:.6f}; '
          f'note F1 {f1[0]:.4f}, with offsets {f1[1]:.4f} ({sum(len(reference[t][tools.KEY_NOTES]) for t in range(TRACKS))} whole-track notes)')

# (c) the stitch kernel alone
L, ROWS, B = 31 * 497 + T, 88, 256
plan = seam_clips([L] * TRACKS, T, 64)
assert len(plan.track_ids) == B
maps = TrackMaps([L] * TRACKS, DEV)
maps.add('roll', (ROWS,), torch.float32)
desc = maps.descriptors('roll', plan.track_ids, plan.kept)
desc_dev = torch.from_numpy(desc).to(DEV)
src = torch.rand((B, ROWS, T), dtype=torch.float32, device=DEV)
kept = int(plan.kept[:, 2].sum()) * ROWS
assert kept == maps.flat('roll').numel()
flat_src, flat_dst = torch.rand(kept, dtype=torch.float32, device=DEV), torch.empty(kept, dtype=torch.float32, device=DEV)


def event_times(fn, warmup=5, reps=30, inner=20):
    """Microseconds per call: device events around `inner` calls back to back (a single call of this size is shorter than the host's own
    work per launch), sorted over `reps` repetitions."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / inner)
    return sorted(out)


flat = maps.flat('roll')
stitch = event_times(lambda: _lib.call('amtx_stitch_clips', src, 4, B, ROWS, T, desc, desc_dev, flat, flat.numel(), device=DEV))
copy = event_times(lambda: flat_dst.copy_(flat_src))
want = np.empty(kept, dtype=np.float32)
from amt_tools_amd.tracks import stitch_host       # noqa: E402
assert np.array_equal(maps.flat('roll').cpu().numpy().view(np.uint32), stitch_host(want, src.cpu().numpy(), desc).view(np.uint32))
for name, us in (('amtx_stitch_clips', stitch), ('dst.copy_(src)   ', copy)):
    print(f'  (c) {name}: {us[len(us) // 2]:7.1f} us median of {len(us)} (min {us[0]:.1f}, max {us[-1]:.1f}), {kept * 4 / 1e6:.1f} MB read and as many written: '
          f'{2 * kept * 4 / us[len(us) // 2] / 1e6:.2f} TB/s at the median')
