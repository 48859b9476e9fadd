#!/usr/bin/env python3
"""Training clips' features from a TrackBank against the route without one, on the BASELINE log-mel plan (22.05 kHz, hop 512, 229 mels,
n_fft 2048): 8 clips x 625 frames per step, drawn from a bank of a few long synthetic tracks.

  (a) bank     : bank.clips(ids, first_frames, 625) -> process_clips            (descriptor table built and uploaded, track-level dB)
  (b) upload   : a prepared (8, 319 999) host batch -> device -> process_batch   (clip-own dB, clip-edge padding: the route without a bank)
  (c) kernels  : amtx_spec_power_clips against amtx_spec_power on 8 x 625 frames each, LAUNCHES per timing

Device events, a warm-up, then REPEATS timings of each with (a) / (b) and the two kernels of (c) alternating in one process; medians and
the min .. max spread are printed as one JSON line.  No threshold: the numbers go into DESIGN.md 6e."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np      # noqa: E402
import torch            # noqa: E402

from amt_tools_amd import _lib                       # noqa: E402
from amt_tools_amd.features import MelSpec           # noqa: E402
from amt_tools_amd.synth import synth_clip           # noqa: E402
from amt_tools_amd.tracks import TrackBank           # noqa: E402

B, T, HOP = 8, 625, 512
N = (T - 1) * HOP + HOP - 1          # 319 999 samples: 625 frames


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {'median_ms': round(float(np.median(ms)), 4), 'min_ms': round(float(ms[0]), 4), 'max_ms': round(float(ms[-1]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tracks', type=int, default=4)
    ap.add_argument('--minutes', type=float, default=2.0, help='length of every synthetic track')
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20, help='kernel launches per timing of (c)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    mod = MelSpec(sample_rate=22050, hop_length=HOP, n_mels=229, n_fft=2048)
    rng = np.random.default_rng(0)
    n_track = int(args.minutes * 60 * 22050)
    tracks = []
    for i in range(args.tracks):
        seg = synth_clip(i)
        gains = rng.uniform(0.05, 1.0, size=n_track // seg.size + 1).astype(np.float32)
        tracks.append(np.concatenate([g * seg for g in gains])[:n_track - 1000 * i])
    bank = TrackBank(tracks, mod, dev)
    bank.db_ref                                                            # upload + the maxima launch, outside every timing
    draws = []
    for _ in range(args.warmup + args.repeats):
        ids = rng.integers(0, len(bank), size=B)
        firsts = np.array([rng.integers(0, bank.frame_counts[k] - T) for k in ids])       # the clip's N samples end inside the track
        host = np.stack([tracks[k][f * HOP:f * HOP + N] for k, f in zip(ids, firsts)])
        draws.append((ids, firsts, host))

    def route_bank(d):
        return mod.process_clips(bank.clips(d[0], d[1], T), model_layout=True)

    def route_upload(d):
        return mod.process_batch(torch.from_numpy(d[2]).to(dev), model_layout=True)

    plan = mod._get_plan(dev)
    clips = bank.clips(draws[0][0], draws[0][1], T)
    x = torch.from_numpy(draws[0][2]).to(dev)
    power = torch.empty((B, T, 229), dtype=torch.float32, device=dev)
    cmax = torch.empty((B,), dtype=torch.float32, device=dev)

    def kernel_clips():
        for _ in range(args.launches):
            _lib.call('amtx_spec_power_clips', plan, bank.audio, clips.desc_dev, B, T, power, cmax, device=dev)

    def kernel_equal():
        for _ in range(args.launches):
            _lib.call('amtx_spec_power', plan, x, N, x.stride(0), B, power, cmax, device=dev)

    t = {'bank': [], 'upload': [], 'kernel_clips': [], 'kernel_equal': []}
    for i, d in enumerate(draws):
        row = {'bank': timed(lambda: route_bank(d)), 'upload': timed(lambda: route_upload(d)),
               'kernel_clips': timed(kernel_clips) / args.launches, 'kernel_equal': timed(kernel_equal) / args.launches}
        if i >= args.warmup:
            for k, v in row.items():
                t[k].append(v)
    out = {'bench': 'track_clips', 'clips': B, 'frames': T, 'tracks': len(bank), 'track_samples': int(bank.lengths[0]), 'repeats': args.repeats,
           'a_process_clips_from_bank': stats(t['bank']), 'b_upload_then_process_batch': stats(t['upload']),
           'c_kernel_power_clips': stats(t['kernel_clips']), 'c_kernel_power_equal_clips': stats(t['kernel_equal'])}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
