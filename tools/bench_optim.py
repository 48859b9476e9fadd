#!/usr/bin/env python3
"""Device time of one optimizer step() on the parameter sets of OnsetsFrames (model_complexity 2, Adam), OnsetsFrames2 (model_complexity 3,
Adam) and TabCNN (Adadelta), gradients present, on one GPU.  Routes, alternated step by step in one process, each on its own copy of the
parameters (conv weights channels-last, as the training path holds them):
  hip         amt_tools_amd.optim's class (csrc/optim.hip, one launch)
  torch       torch's class with its defaults (the multi-tensor path)
  fused       torch.optim.Adam(fused=True), where it exists (Adam only)
  *_clip      the same with global gradient-norm clipping at 3: max_norm=3 for hip, clip_grad_norm_(params, 3) + step() for the others
A step is timed with device events on the launch stream; --warmup steps first, then the min .. median .. max over --iters.  For the hip
route the bytes the update moves (28 per element: 4 reads, 3 writes) over the median give its HBM rate and the fraction of the read rate
tools/hbm_read.hip measures (6.1 TB/s).  Then one whole training step of the 8 clips x 625 frames recipe (MelSpec + OnsetsFrames fwd + bwd +
step, bench.py --mode train at one GPU) with the hip route and with the torch route, wall time to a device synchronise.
Prints ONE JSON line.

Usage: python tools/bench_optim.py [--warmup 5] [--iters 30] [--sets of1,of2,tabcnn] [--no-train-step]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from amt_tools_amd import optim, tools

HBM_READ_TBS = 6.1          # tools/hbm_read.hip
DEV = 'cuda:0'


def parameter_set(name):
    from amt_tools_amd.models import OnsetsFrames, OnsetsFrames2, TabCNN
    torch.manual_seed(0)
    if name == 'of1':
        model = OnsetsFrames(229, tools.PianoProfile(), 1, 2, device=DEV)
    elif name == 'of2':
        model = OnsetsFrames2(229, tools.PianoProfile(), 1, 3, device=DEV)
    else:
        model = TabCNN(192, tools.GuitarProfile(num_frets=19), 1, 1, device=DEV)
    model.change_device()
    return [p.detach() for p in model.parameters()]


def routes_of(kind):
    mine, theirs = (optim.Adam, torch.optim.Adam) if kind == 'Adam' else (optim.Adadelta, torch.optim.Adadelta)
    kw = dict(lr=6e-4) if kind == 'Adam' else dict(lr=1.0)
    routes = {'hip': (lambda ps: mine(ps, **kw), None), 'torch': (lambda ps: theirs(ps, **kw), None),
              'hip_clip': (lambda ps: mine(ps, max_norm=3.0, **kw), None), 'torch_clip': (lambda ps: theirs(ps, **kw), 3.0)}
    if kind == 'Adam':
        routes['fused'] = (lambda ps: theirs(ps, fused=True, **kw), None)
        routes['fused_clip'] = (lambda ps: theirs(ps, fused=True, **kw), 3.0)
    return routes


def bench_set(name, warmup, iters):
    kind = 'Adadelta' if name == 'tabcnn' else 'Adam'
    base = parameter_set(name)
    g = torch.Generator(device=DEV).manual_seed(1)
    grads = [torch.empty_like(p).normal_(generator=g).mul_(1e-2) for p in base]
    steps = {}
    for route, (make, clip) in routes_of(kind).items():
        params = [torch.nn.Parameter(p.clone()) for p in base]        # clone keeps the memory layout
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
        opt = make(params)

        def step(opt=opt, params=params, clip=clip):
            if clip is not None:
                torch.nn.utils.clip_grad_norm_(params, clip)
            opt.step()
        steps[route] = step
    times = {r: [] for r in steps}
    for it in range(warmup + iters):
        for route, step in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            step()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[route].append(e0.elapsed_time(e1) * 1e3)
    numel = sum(p.numel() for p in base)
    rec = {'optimizer': kind, 'tensors': len(base), 'elements': numel,
           'us_min_median_max': {r: [round(min(t), 1), round(statistics.median(t), 1), round(max(t), 1)] for r, t in times.items()}}
    med = statistics.median(times['hip'])
    rec['hip_tb_per_s'] = round(28 * numel / med / 1e6, 3)
    rec['hip_fraction_of_hbm_read_rate'] = round(28 * numel / med / 1e6 / HBM_READ_TBS, 3)
    rec['hip_not_slower_than_torch'] = med <= statistics.median(times['torch'])
    return rec


def train_step(warmup, iters):
    """bench.py's training step (8 clips x 625 frames, MelSpec front-end inside the model) with each optimizer route, alternated."""
    import bench
    from amt_tools_amd.features import MelSpec
    from amt_tools_amd.models import OnsetsFrames
    from amt_tools_amd.synth import synth_clip, synth_labels
    B = 8
    audio = torch.from_numpy(np.stack([synth_clip(i) for i in range(B)])).to(DEV)
    lab = [synth_labels(i) for i in range(B)]
    batch = {tools.KEY_AUDIO: audio, tools.KEY_MULTIPITCH: torch.from_numpy(np.stack([l[0] for l in lab])).to(DEV),
             tools.KEY_ONSETS: torch.from_numpy(np.stack([l[1] for l in lab])).to(DEV)}
    steps = {}
    for route, cls in (('hip', optim.Adam), ('torch', torch.optim.Adam)):
        torch.manual_seed(0)
        model = OnsetsFrames(bench.N_MELS, tools.PianoProfile(), 1, 2, device=DEV)
        model.frontend = torch.nn.Sequential(MelSpec(sample_rate=bench.SR, hop_length=bench.HOP, n_mels=bench.N_MELS, n_fft=bench.N_FFT,
                                                     device=DEV).frontend())
        model.change_device()
        model.train()
        opt = cls(model.parameters(), lr=6e-4)

        def step(model=model, opt=opt):
            opt.zero_grad()
            model.run_on_batch(batch)[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL].backward()
            opt.step()
        steps[route] = step
    times = {r: [] for r in steps}
    for it in range(warmup + iters):
        for route, step in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            if it >= warmup:
                times[route].append((time.perf_counter() - t0) * 1e3)
    return {'workload': 'OnsetsFrames(mc 2) + MelSpec(229) fwd + bwd + Adam, 8 clips x 625 frames, wall ms per step',
            'ms_min_median_max': {r: [round(min(t), 3), round(statistics.median(t), 3), round(max(t), 3)] for r, t in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--sets', default='of1,of2,tabcnn')
    ap.add_argument('--no-train-step', action='store_true')
    a = ap.parse_args()
    rec = {'device': torch.cuda.get_device_name(0), 'warmup': a.warmup, 'iters': a.iters}
    for name in a.sets.split(','):
        rec[name] = bench_set(name, a.warmup, a.iters)
    if not a.no_train_step:
        rec['train_step'] = train_step(3, 10)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
