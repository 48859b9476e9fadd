#!/usr/bin/env python3
"""Scoring clips of resident tracks, two ways: N clips x 625 frames of 8 synthetic tracks (synth_clip audio tiled to 10 000 frames, synth_labels
tiled as ground truth, notes from the tiled maps) against MultipitchEvaluator + NoteEvaluator (onsets only, and with offset_ratio 0.2) on
one GPU (bf16 engine, as bench.py builds it), batches of 256.

  (a) clips   evaluate.validate_clips: the audio, the label maps and the notes are resident (TrackBank, LabelBank, NoteBank); per batch
              only clip descriptors go to the device and count tensors come back
  (b) host    what the package offered before for the same clips: evaluate.validate_batched on the host arrays of the clips (pinned
              float32, sliced out of the tracks beforehand) with host-sliced references (sliced beforehand too: neither is timed)

The two routes see different features -- the bank scales a clip against its TRACK's maximum, the host route against the clip's own -- so
their results are not compared with each other; each is checked against the host evaluators applied to its own predictions.  Prints both
times (median, min and max of three after one warm-up each) and the bytes each copies either way.  No threshold.
Usage: python tools/bench_validate_clips.py [num_clips=1024] [batch=256]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from amt_tools_amd import evaluate as ev, tools, transcribe
from amt_tools_amd.inference import run_offline_batched
from amt_tools_amd.synth import synth_clip, synth_labels, CLIP_FRAMES
from amt_tools_amd.tracks import LabelBank, NoteBank, TrackBank, clip_windows

args = [a for a in sys.argv[1:] if not a.startswith('--')]
N = int(args[0]) if args else 1024
B = int(args[1]) if len(args) > 1 else 256
TRACKS, REPEAT, T, HOP, SR = 8, 16, CLIP_FRAMES, 512, 22050
model, mel, sd = bench.build_model('cuda:0', 'bf16')
model.frontend = torch.nn.Sequential(mel.frontend())
model.eval()

tracks = [np.tile(synth_clip(i), REPEAT) for i in range(TRACKS)]
bank = TrackBank(tracks, mel, 'cuda:0')
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

# route (b)'s inputs: the reference's own slices of the same clips (datasets/common.py:343-376), made once
seq_length = int(max(mel.get_sample_range(T)))
host = torch.empty((N, seq_length), dtype=torch.float32).pin_memory()
for i, (k, f) in enumerate(zip(ids, firsts)):
    host[i] = torch.from_numpy(tracks[k][f * HOP:f * HOP + seq_length])
sliced = notes.host_clips(ids, firsts, T)
references = [{tools.KEY_MULTIPITCH: maps[k][tools.KEY_MULTIPITCH][:, f:f + T], tools.KEY_NOTES: sliced[i]} for i, (k, f) in enumerate(zip(ids, firsts))]
assert clip_windows(mel, firsts[:1], T)[0, 1] == (firsts[0] * HOP + seq_length) / SR


def combo():
    return ev.ComboEvaluator([ev.MultipitchEvaluator(), ev.NoteEvaluator(), ev.NoteEvaluator(offset_ratio=0.2, results_key='notes-with-offsets')])


def route_a():
    average = ev.validate_clips(bank, labels, notes, model, combo(), ids, firsts, T, batch_size=B)
    torch.cuda.synchronize()
    return average


def route_b():
    average = ev.validate_batched(host, references, model, combo(), batch_size=B)
    torch.cuda.synchronize()
    return average


def check_a():
    """The host evaluators on run_on_batch's predictions of the same bank clips."""
    c = combo()
    with torch.no_grad():
        for s in range(0, N, B):
            preds = model.run_on_batch({tools.KEY_AUDIO: bank.clips(ids[s:s + B], firsts[s:s + B], T)})
            decoded = transcribe.decode_notes_for(preds, model, None).result()
            mp = preds[tools.KEY_MULTIPITCH].cpu().numpy()
            for j in range(len(decoded)):
                c.process_track({tools.KEY_MULTIPITCH: mp[j], tools.KEY_NOTES: decoded[j]}, references[s + j], s + j)
    return c.average_results()


def check_b():
    out = run_offline_batched(host, model, batch_size=B, decode_notes=True, keep=(tools.KEY_MULTIPITCH,))
    c = combo()
    for i in range(N):
        c.process_track(out[i], references[i], i)
    return c.average_results()


def timed(fn):
    result = fn()
    dts = []
    for _ in range(3):
        t0 = time.perf_counter()
        result = fn()
        dts.append(time.perf_counter() - t0)
    return result, sorted(dts)


def counted(fn):
    """One run of fn with every host-to-device Tensor.to / .cuda and every device-to-host Tensor.cpu counted: (bytes up, bytes down)."""
    up, down = [0], [0]
    real = {name: getattr(torch.Tensor, name) for name in ('to', 'cuda', 'cpu')}

    def size(t):
        return t.numel() * t.element_size()

    def to(t, *a, **k):
        r = real['to'](t, *a, **k)
        if not t.is_cuda and r.is_cuda:
            up[0] += size(t)
        return r

    def cuda(t, *a, **k):
        if not t.is_cuda:
            up[0] += size(t)
        return real['cuda'](t, *a, **k)

    def cpu(t, *a, **k):
        if t.is_cuda:
            down[0] += size(t)
        return real['cpu'](t, *a, **k)
    torch.Tensor.to, torch.Tensor.cuda, torch.Tensor.cpu = to, cuda, cpu
    try:
        fn()
    finally:
        torch.Tensor.to, torch.Tensor.cuda, torch.Tensor.cpu = real['to'], real['cuda'], real['cpu']
    return up[0], down[0]


a, dts_a = timed(route_a)
b, dts_b = timed(route_b)
up_a, down_a = counted(route_a)
up_b, down_b = counted(route_b)
print(f'{N} clips x {T} frames of {TRACKS} resident tracks ({int(bank.frame_counts[0])} frames each), batches of {B}')
for name, dts, up, down in (('(a) validate_clips                     ', dts_a, up_a, down_a), ('(b) validate_batched on the host clips ', dts_b, up_b, down_b)):
    print(f'  {name}: {dts[1] * 1e3:8.1f} ms median of 3 (min {dts[0] * 1e3:.1f}, max {dts[2] * 1e3:.1f}), {up / 1e6:.3f} MB to the device, '
          f'{down / 1e6:.3f} MB to the host')
print(f'  resident: audio {bank.audio.numel() * 4 / 1e6:.1f} MB, label runs {labels.nbytes / 1e6:.3f} MB, note rows {notes.nbytes / 1e6:.3f} MB')
print(f'  (a) equals the host evaluators on its own predictions: {a == check_a()}; (b): {b == check_b()}')
for name, r in (('(a)', a), ('(b)', b)):
    print(f'  {name} f1 {r[tools.KEY_MULTIPITCH][tools.KEY_F1]:.4f} / {r[tools.KEY_NOTES][tools.KEY_F1]:.4f} / {r["notes-with-offsets"][tools.KEY_F1]:.4f}')
