#!/usr/bin/env python3
"""One TabCNN training step at the reference recipe's shape (examples/papers/tabcnn.py: GuitarSet, batches of 30 x 200 frames, CQT 192
bins, Adadelta lr 1.0) on one GPU: the stock path (MIOpen / hipBLASLt convolving every 9-frame window, TabCNN.use_hip_train off) against
the HIP path (shared-window convolutions on the split-bf16 training GEMMs, csrc/tabtrain.hip's pool and loss), alternated step by step in
one process.  A step is pre_proc + forward + loss + backward + Adadelta, ending in a device synchronise; both paths are warmed up first and
the median over --iters steps is reported, with frames per second and the largest gradient difference between the two paths on one batch
(Dropout off, same weights).  Prints ONE JSON line.

Per-kernel split: run the HIP path alone under rocprofv3, then summarise the trace by kernel family:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o tab -- python3 tools/bench_tabcnn_train.py --paths hip --iters 10
  python3 tools/bench_tabcnn_train.py --summarize OUT --steps 13        (steps = warmup + iters of that run)

Usage: python tools/bench_tabcnn_train.py [--batch 30] [--frames 200] [--bins 192] [--warmup 3] [--iters 20] [--paths hip,stock]"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from amt_tools_amd import autograd, tools
from amt_tools_amd.models import TabCNN
from amt_tools_amd.synth import synth_tabcnn_state_dict


def make_model(bins, hip, dropout=True, seed=0):
    m = TabCNN(bins, tools.GuitarProfile(num_frets=19), 1, 1, device='cuda:0')
    sd = synth_tabcnn_state_dict(seed, dim_in=bins, in_channels=1, model_complexity=1, num_groups=6, num_classes=21)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    if not dropout:
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
    m.use_hip_train = hip
    m.change_device()
    m.train()
    return m


def step_flops(B, T, bins, hip):
    """Multiply-adds x 2 of the convolutions and dense layers, forward + input gradients + weight gradients (conv1 has no input gradient)."""
    H = (bins - 6) // 2
    if hip:
        pos = B * (T + 8) * bins                            # padded convolutions over every whole sequence
        conv = [pos * 9 * ci * co for ci, co in ((1, 32), (32, 64), (64, 64))]
    else:
        conv = [B * T * (bins - 2 - 2 * i) * (7 - 2 * i) * 9 * ci * co for i, (ci, co) in enumerate(((1, 32), (32, 64), (64, 64)))]
    dense = [B * T * 64 * H * 128, B * T * 128 * 126]
    return 2 * (conv[0] * 2 + (conv[1] + conv[2]) * 3 + sum(dense) * 3)


def summarize(out_dir, steps):
    """Per-step kernel time of a rocprofv3 --kernel-trace CSV, by family."""
    files = glob.glob(os.path.join(out_dir, '**', '*kernel_trace.csv'), recursive=True)
    assert files, f'no kernel trace CSV under {out_dir}'
    per = {}
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row.get('Kernel_Name') or row.get('Name') or ''
                per[name] = per.get(name, 0) + int(row['End_Timestamp']) - int(row['Start_Timestamp'])

    def family(n):
        low = n.lower()
        if 'tab_pool' in low:
            return 'pool'
        if 'sm_loss' in low:
            return 'loss'
        if any(t in low for t in ('miopen', 'cijk_', 'rocblas', 'hipblas', 'igemm')):
            return 'vendor'
        if any(t in low for t in ('xgemm', 'xconv', 'xwgrad', 'xreduce', 'xcolsum', 'conv_w_permute', 'conv1')):
            return 'HIP conv + linear GEMMs'
        if any(t in low for t in ('threshold', 'clamp', 'relu')):
            return 'ReLU glue'
        return 'other ATen glue'
    fam = {}
    for n, ns in per.items():
        fam[family(n)] = fam.get(family(n), 0) + ns
    total = sum(fam.values())
    res = {k: round(v / steps / 1e6, 3) for k, v in sorted(fam.items(), key=lambda kv: -kv[1])}
    top = sorted(per.items(), key=lambda kv: -kv[1])[:15]
    print(json.dumps({'kernel_ms_per_step': round(total / steps / 1e6, 3), 'by_family_ms_per_step': res,
                      'top_kernels_ms_per_step': [[n[:90], round(ns / steps / 1e6, 3)] for n, ns in top]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=30)
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--bins', type=int, default=192)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--paths', default='hip,stock')
    ap.add_argument('--summarize', default=None, help='summarise a rocprofv3 output directory instead of timing')
    ap.add_argument('--steps', type=int, default=1)
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize, a.steps)
        return
    paths = a.paths.split(',')
    B, T, Fb = a.batch, a.frames, a.bins
    g = torch.Generator().manual_seed(0)
    batch = {tools.KEY_FEATS: torch.rand((B, 1, Fb, T), generator=g).cuda(), tools.KEY_TABLATURE: torch.randint(-1, 21, (B, 6, T), generator=g).cuda()}
    models = {p: make_model(Fb, p == 'hip') for p in paths}
    opts = {p: torch.optim.Adadelta(models[p].parameters(), lr=1.0) for p in paths}

    def step(p):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opts[p].zero_grad()
        models[p].run_on_batch(batch)[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL].backward()
        opts[p].step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    fb0 = autograd.fallback_total()
    for _ in range(a.warmup):
        for p in paths:
            step(p)
    times = {p: [] for p in paths}
    for _ in range(a.iters):
        for p in paths:
            times[p].append(step(p))
    rec = {'shape': [B, T, Fb], 'warmup': a.warmup, 'iters': a.iters, 'device': torch.cuda.get_device_name(0)}
    for p in paths:
        ms = statistics.median(times[p])
        rec[p] = {'ms_per_step': round(ms, 3), 'min_ms': round(min(times[p]), 3), 'frames_per_s': round(B * T / ms * 1e3, 1),
                  'gflop_per_step': round(step_flops(B, T, Fb, p == 'hip') / 1e9, 1)}
    if 'hip' in paths:
        rec['hip']['fallbacks_taken'] = autograd.fallback_total() - fb0 - (a.warmup + a.iters) * ('stock' in paths)
    if len(paths) == 2:
        rec['speedup'] = round(rec['stock']['ms_per_step'] / rec['hip']['ms_per_step'], 2)
        # gradients of both paths on the same batch and weights, Dropout off
        grads = {}
        for p in paths:
            m = make_model(Fb, p == 'hip', dropout=False, seed=1)
            m.run_on_batch(batch)[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL].backward()
            grads[p] = {k: q.grad.detach().double() for k, q in m.named_parameters()}
        rec['max_grad_rel_diff'] = max(float((grads['hip'][k] - grads['stock'][k]).abs().max() / grads['stock'][k].abs().max())
                                       for k in grads['stock'])
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
