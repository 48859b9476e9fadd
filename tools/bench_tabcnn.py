#!/usr/bin/env python3
"""TabCNN (BASELINE config 1: CQT(192 bins, 24/oct) -> TabCNN -> 6 strings x 21 classes) on one GPU: the stock torch path (MIOpen /
hipBLASLt convolving every 9-frame window) against the HIP engine (csrc/tab.hip, shared-window convolutions) in x3 and bf16, at the same
inputs, run alternately in one process.  Two batch shapes -- whole 1292-frame tracks (a validation batch) and GuitarSet training-shaped
samples (30 x 200 frames) -- each with features in and with audio in (the HIP CQT included).  Parity is measured against the stock path run
over sub-batches of 4 clips.  Prints ONE JSON line.

Usage: python tools/bench_tabcnn.py [--tracks 32] [--warmup 3] [--iters 10] [--cases val,train] [--inputs feats,audio]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from amt_tools_amd import tools
from amt_tools_amd.features import CQT
from amt_tools_amd.models import TabCNN
from amt_tools_amd.synth import synth_clip, synth_tabcnn_state_dict

MFLOP_WINDOWED = 78.1      # per frame, the reference's per-window convolutions (39.06 M MAC)
MFLOP_SHARED = 22.3        # per frame, the convolutions run once per sequence (11.15 M MAC)
BF16_PEAK_TFLOPS = 2500.0  # MI355X dense bf16 MFMA (spec)
HOP = 512
PARITY_CLIPS = 4


def stock_forward(model, win):
    """TabCNN.forward's stock branch (what runs for every other case): the windows reshaped to B*T images, Conv2d x 3, pool, Linear."""
    B, T = win.shape[:2]
    emb = model.conv(win.reshape(B * T, model.in_channels, model.dim_in, model.frame_width))
    return model.dense(emb.reshape(B, T, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tracks', type=int, default=32, help='1292-frame tracks in the validation batch')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--cases', default='val,train')
    ap.add_argument('--inputs', default='feats,audio')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    profile = tools.GuitarProfile(num_frets=19)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth_tabcnn_state_dict(3, dim_in=192).items()}
    cqt = CQT(sample_rate=22050, hop_length=HOP, n_bins=192, bins_per_octave=24)
    models = {}
    for prec in ('x3', 'bf16'):
        m = TabCNN(192, profile, 1, 1, device=dev, precision=prec)
        m.load_state_dict(sd)
        m.frontend = torch.nn.Sequential(cqt.frontend())
        m.change_device()
        m.eval()
        models[prec] = m
    stock = models['x3']          # the stock path needs no engine: same weights, called through the stock branch
    shapes = {'val': (args.tracks, 1292), 'train': (30, 200)}
    result = dict(tool='bench_tabcnn', gpu=torch.cuda.get_device_name(dev), mflop_per_frame_windowed=MFLOP_WINDOWED,
                  mflop_per_frame_shared=MFLOP_SHARED, bf16_peak_tflops=BF16_PEAK_TFLOPS, warmup=args.warmup, iters=args.iters, cases={})
    head = stock.dense[-1]
    for case in args.cases.split(','):
        B, T = shapes[case]
        n_samples = int(cqt.get_sample_range(T)[-1])
        base = np.stack([synth_clip(i, num_samples=n_samples) for i in range(4)]).astype(np.float32)
        audio = torch.from_numpy(base).to(dev).repeat((B + 3) // 4, 1)[:B].contiguous()
        with torch.no_grad():
            feats = cqt.process_batch(audio)
        feats = feats if feats.dim() == 4 else feats.unsqueeze(1)
        assert feats.shape[-1] == T, feats.shape
        for inp in args.inputs.split(','):
            def run(path, sl=slice(None)):
                with torch.no_grad():
                    batch = {tools.KEY_AUDIO: audio[sl]} if inp == 'audio' else {tools.KEY_FEATS: feats[sl]}
                    m = stock if path == 'stock' else models[path]
                    win = m.pre_proc(batch)[tools.KEY_FEATS]
                    if path == 'stock':
                        logits = stock_forward(stock, win)
                        return logits, head.finalize_output(logits)
                    out = {tools.KEY_OUTPUT: m(win)}
                    logits = out[tools.KEY_OUTPUT][tools.KEY_TABLATURE]
                    return logits, m.post_proc(out)[tools.KEY_TABLATURE]
            paths = ('stock', 'x3', 'bf16')
            outs = {}
            for _ in range(args.warmup):
                for p in paths:
                    outs[p] = run(p)
            torch.cuda.synchronize(dev)
            times = {p: [] for p in paths}
            for _ in range(args.iters):
                for p in paths:                  # alternating, each timed between device synchronisations
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize(dev)
                    e0.record()
                    outs[p] = run(p)
                    e1.record()
                    torch.cuda.synchronize(dev)
                    times[p].append(e0.elapsed_time(e1))
            frames = B * T
            rec = dict(batch=B, frames_per_clip=T, frames=frames)
            # parity reference: the stock path over sub-batches of PARITY_CLIPS clips (every tensor of it far below 2^31 elements)
            parts = [run('stock', slice(i, i + PARITY_CLIPS)) for i in range(0, B, PARITY_CLIPS)]
            ref_logits, ref_tab = torch.cat([q[0] for q in parts]), torch.cat([q[1] for q in parts])
            for p in paths:
                ms = float(np.median(times[p]))
                fps = frames / (ms * 1e-3)
                r = dict(ms_per_batch=round(ms, 3), ms_min=round(float(np.min(times[p])), 3), frames_per_s=round(fps, 1))
                if p == 'stock':
                    r['algorithmic_tflops'] = round(fps * MFLOP_WINDOWED * 1e-6, 2)
                    r['max_logit_err_vs_subbatches'] = float((outs[p][0] - ref_logits).abs().max())
                else:
                    work = MFLOP_SHARED * (3 if p == 'x3' else 1)      # x3 issues three MFMAs per product
                    r['algorithmic_tflops'] = round(fps * MFLOP_SHARED * 1e-6, 2)
                    r['mfma_peak_fraction'] = round(fps * work * 1e-6 / BF16_PEAK_TFLOPS, 4)
                    lg, tb = outs[p]
                    r['max_logit_err_vs_stock'] = float((lg - ref_logits).abs().max())          # stock over sub-batches
                    r['tab_cells_differ'] = int((tb != ref_tab).sum())
                    r['max_logit_err_vs_stock_whole_batch'] = float((lg - outs['stock'][0]).abs().max())
                    r['speedup_vs_stock'] = round(float(np.median(times['stock'])) / ms, 2)
                rec[p] = r
            result['cases'][f'{case}_{inp}'] = rec
    print(json.dumps(result))


if __name__ == '__main__':
    main()
