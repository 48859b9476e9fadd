#!/usr/bin/env python3
"""CQT-family training clips from a PyramidBank against the route without one, for the two workloads that sit on these front-ends:

  tabcnn   : the TabCNN recipe, 30 clips x 200 frames, CQT 192 bins / 24 per octave (22.05 kHz, hop 512)
  config3  : BASELINE config 3's front-end, 8 clips x 625 frames, HCQT 6 harmonics x 72 bins

  (a) bank    : bank.clips(ids, first_frames, T) -> process_clips          (no decimation, no upload: basis products over resident levels)
  (b) upload  : a prepared (B, N) host batch of the clips' own samples -> device -> process_batch   (clip-own dB, clip-edge padding)
  (c) build   : PyramidBank -> db_ref (upload, decimations, pads, the maxima launch), per second of audio

Device events for (a) / (b), a warm-up, then REPEATS timings with the two routes alternating in one process; (c) is wall time around a
synchronised build, REPEATS times.  Medians and the min .. max spread are printed as one JSON line per workload.  No threshold: the
numbers go into DESIGN.md 6e."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np      # noqa: E402
import torch            # noqa: E402

from amt_tools_amd.features import CQT, HCQT         # noqa: E402
from amt_tools_amd.synth import synth_clip           # noqa: E402
from amt_tools_amd.tracks import PyramidBank         # noqa: E402

HOP, SR = 512, 22050
WORKLOADS = {'tabcnn': (30, 200, lambda: CQT(SR, HOP, n_bins=192, bins_per_octave=24)),
             'config3': (8, 625, lambda: HCQT(SR, HOP, n_bins=72))}


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


def run(name, args, dev):
    B, T, make = WORKLOADS[name]
    N = (T - 1) * HOP + HOP - 1                                            # the samples of T frames
    mod = make()
    rng = np.random.default_rng(0)
    n_track = int(args.minutes * 60 * SR)
    tracks = []
    for i in range(args.tracks):
        seg = synth_clip(i)
        gains = rng.uniform(0.05, 1.0, size=n_track // seg.size + 1).astype(np.float32)
        tracks.append(np.concatenate([g * seg for g in gains])[:n_track - 1000 * i])
    seconds = sum(t.size for t in tracks) / SR

    def build():
        t0 = time.perf_counter()
        bank = PyramidBank(tracks, mod, dev)
        bank.db_ref
        torch.cuda.synchronize()
        return bank, (time.perf_counter() - t0) * 1e3
    bank, _ = build()                                                      # plan creation and first allocations outside the timings
    builds = [build()[1] for _ in range(args.repeats)]
    assert mod.get_expected_frames(np.zeros(N, dtype=np.float32)) == T
    draws = []
    for _ in range(args.warmup + args.repeats):
        ids = rng.integers(0, len(bank), size=B)
        firsts = np.array([rng.integers(0, bank.frame_counts[k] - T) for k in ids])       # the clip's N samples end inside the track
        host = np.stack([tracks[k][f * HOP:f * HOP + N] for k, f in zip(ids, firsts)])
        draws.append((ids, firsts, host))
    t = {'bank': [], 'upload': []}
    for i, d in enumerate(draws):
        row = {'bank': timed(lambda: mod.process_clips(bank.clips(d[0], d[1], T))),
               'upload': timed(lambda: mod.process_batch(torch.from_numpy(d[2]).to(dev)))}
        if i >= args.warmup:
            for k, v in row.items():
                t[k].append(v)
    pyramid_bytes, audio_bytes = bank.pyramid.numel() * 4, bank.audio.numel() * 4
    return {'bench': 'pyramid_clips', 'workload': name, 'clips': B, 'frames': T, 'tracks': len(bank), 'audio_seconds': round(seconds, 1),
            'repeats': args.repeats, 'audio_mib': round(audio_bytes / 2 ** 20, 2), 'pyramid_mib': round(pyramid_bytes / 2 ** 20, 2),
            'a_process_clips_from_bank': stats(t['bank']), 'b_upload_then_process_batch': stats(t['upload']),
            'c_bank_build': stats(builds), 'c_bank_build_ms_per_audio_second': round(float(np.median(builds)) / seconds, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tracks', type=int, default=4)
    ap.add_argument('--minutes', type=float, default=2.0, help='length of every synthetic track')
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--workloads', nargs='+', default=sorted(WORKLOADS), choices=sorted(WORKLOADS))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    for name in args.workloads:
        print(json.dumps(run(name, args, dev)), flush=True)


if __name__ == '__main__':
    main()
