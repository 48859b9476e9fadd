#!/usr/bin/env python3
"""BASELINE config 1 on one GPU, host to host: the guitar twin of tools/bench_transcribe.py.  Synthetic audio in pinned host memory -> H2D ->
CQT (192 bins) + TabCNN engine -> stacked notes {string: (pitches, intervals)} per track on the host, three ways over the same clips:
  forward   run_offline_batched without decoding, the tablature brought back to the host (what the package did before it had a decoder)
  device    + amtx_tab_notes on the device, only the note rows cross PCIe (decode_notes=True, keep=())
  host      the forward run, then this package's host estimators (TablatureWrapper + StackedNoteTranscriber) track by track
Two warm-up runs each, then the median and best of five.  Seed-generated weights make a tablature that changes class almost every frame:
far more notes per track than real playing, the worst case for both decoders.  Prints ONE JSON line.
Usage: python tools/bench_tab_transcribe.py [tracks=32] [batch=32] [frames=1292] [--bf16]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from amt_tools_amd import tools, transcribe
from amt_tools_amd.features import CQT
from amt_tools_amd.inference import run_offline_batched
from amt_tools_amd.models import TabCNN
from amt_tools_amd.synth import synth_clip, synth_tabcnn_state_dict

args = [a for a in sys.argv[1:] if not a.startswith('--')]
N = int(args[0]) if args else 32
B = int(args[1]) if len(args) > 1 else 32
T = int(args[2]) if len(args) > 2 else 1292
HOP, SR = 512, 22050
dev = torch.device('cuda:0')
profile = tools.GuitarProfile(num_frets=19)
cqt = CQT(sample_rate=SR, hop_length=HOP, n_bins=192, bins_per_octave=24)
model = TabCNN(192, profile, 1, 1, device=dev, precision='bf16' if '--bf16' in sys.argv else 'x3')
model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth_tabcnn_state_dict(3, dim_in=192).items()})
model.frontend = torch.nn.Sequential(cqt.frontend())
model.change_device()
model.eval()
n_samples = int(cqt.get_sample_range(T)[-1])
base = np.stack([synth_clip(i, num_samples=n_samples) for i in range(4)]).astype(np.float32)
host = torch.from_numpy(np.tile(base, ((N + 3) // 4, 1))[:N]).pin_memory()
times = np.arange(T) * HOP / float(SR)


def forward():
    res = run_offline_batched(host, model, times=times, batch_size=B, keep=(tools.KEY_TABLATURE,))
    torch.cuda.synchronize()
    return res


def device():
    res = run_offline_batched(host, model, times=times, batch_size=B, decode_notes=True, keep=())
    torch.cuda.synchronize()
    return {i: r[tools.KEY_NOTES] for i, r in res.items()}


def on_host():
    return {i: transcribe._tab_to_stacked_notes_host(r[tools.KEY_TABLATURE], times, profile) for i, r in forward().items()}


def timed(fn):
    fn()
    fn()
    dts = []
    for _ in range(5):
        t0 = time.perf_counter()
        out = fn()
        dts.append((time.perf_counter() - t0) * 1e3)
    return out, round(float(np.median(dts)), 2), round(min(dts), 2)


tabs, fwd_ms, fwd_best = timed(forward)
assert tabs[0][tools.KEY_TABLATURE].shape == (6, T), tabs[0][tools.KEY_TABLATURE].shape
dev_notes, dev_ms, dev_best = timed(device)
host_notes, host_ms, host_best = timed(on_host)


def kernel_us(fn, iters=50):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / iters, 1)


# the kernels alone on the N tablatures (device resident, back-to-back launches: allocation and launch overhead included)
tab_d = torch.from_numpy(np.stack([tabs[i][tools.KEY_TABLATURE] for i in range(N)])).to(dev)
kernels = dict(expand_stacked_us=kernel_us(lambda: tools.tab_expand(tab_d, profile, stacked=True)),
               expand_collapsed_us=kernel_us(lambda: tools.tab_expand(tab_d, profile, stacked=False, collapsed=True)),
               expand_both_us=kernel_us(lambda: tools.tab_expand(tab_d, profile, stacked=True, collapsed=True)),
               notes_us=kernel_us(lambda: transcribe.decode_tab_notes_batch_async(tab_d, times, profile)),
               notes_window_minimum_us=kernel_us(lambda: transcribe.decode_tab_notes_batch_async(tab_d, times, profile, 0.05, 0.1)),
               expand_both_bytes=int(N * 7 * 44 * T * 4), tablature_bytes=int(tab_d.numel() * 8))
same = all(np.array_equal(dev_notes[i][s][k], host_notes[i][s][k]) for i in host_notes for s in range(6) for k in (0, 1))
print(json.dumps(dict(tool='bench_tab_transcribe', gpu=torch.cuda.get_device_name(dev), tracks=N, batch=B, frames_per_track=T, precision=model.precision,
                      notes=int(sum(len(p) for n in host_notes.values() for p, _ in n.values())), device_equals_host=bool(same),
                      forward_only_ms=fwd_ms, forward_only_ms_best=fwd_best, device_notes_ms=dev_ms, device_notes_ms_best=dev_best,
                      host_notes_ms=host_ms, host_notes_ms_best=host_best,
                      decode_cost_device_ms=round(dev_ms - fwd_ms, 2), decode_cost_host_ms=round(host_ms - fwd_ms, 2), kernels=kernels)))
