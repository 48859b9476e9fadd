#!/usr/bin/env python3
"""
Golden vectors of the evaluators: tests/golden/evaluators.npz.  Like tools/gen_golden_tab.py (whose import stubs it reuses through
tools/gen_golden.py) this runs ONLY where the reference checkout is present; the test-suite reads the fixture, never the reference.

Recorded: what the REAL amt_tools.evaluate classes -- StackedMultipitchEvaluator, MultipitchEvaluator, TablatureEvaluator, SoftmaxAccuracy,
LossWrapper, ComboEvaluator -- and append_results / average_results over three tracks make of small seeded inputs: maps as float64,
tablatures as int64 (GuitarProfile(num_frets=19)).  Arrays and key names only: a results dictionary is stored as `<case>__keys` (its leaf
paths, '/'-joined, in the dictionary's order) and `<case>__values` (float64).

Cases: random maps of density 0.1 and random tablatures, an all-silent estimate, an all-silent reference, both silent, a perfect estimate,
and a tablature with two strings on one pitch in the same frame (string 0 fret 5 = string 1 fret 0 = A2), in estimate and reference.

mir_eval is not installed here.  TablatureEvaluator calls mir_eval.util.f_measure: the stand-in is its documented formula,
2 p r / (p + r) and 0 when both are 0.  The note evaluators are NOT recorded: their arithmetic is mir_eval's own.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden                                   # noqa: E402,F401  (installs the stubs, puts the reference on sys.path)
from gen_golden import OUT, rtools                  # noqa: E402

sys.modules['librosa'].note_to_midi = lambda note: np.asarray(gen_golden._note_to_midi(note))
sys.modules['mir_eval.util'].f_measure = lambda p, r: 0.0 if p == 0 and r == 0 else 2 * p * r / (p + r)
sys.modules['mir_eval'].util = sys.modules['mir_eval.util']
from amt_tools import evaluate as rev               # noqa: E402

rev.util = sys.modules['mir_eval.util']             # gen_golden imported the package (and bound the bare stub) before the line above

PROVENANCE = ('amt_tools.evaluate of the reference checkout; mir_eval absent: mir_eval.util.f_measure replaced by its documented formula '
              '2 p r / (p + r), 0 when p = r = 0 (TablatureEvaluator only); note evaluators not recorded (their arithmetic is mir_eval\'s)')
K, T, S = 88, 37, 3


def flatten(results, prefix=''):
    keys, values = [], []
    for k, v in results.items():
        if isinstance(v, dict):
            kk, vv = flatten(v, f'{prefix}{k}/')
            keys += kk
            values += vv
        else:
            keys.append(f'{prefix}{k}')
            values.append(float(v))
    return keys, values


def record(rec, case, results):
    keys, values = flatten(results)
    rec[f'{case}__keys'] = np.array(keys)
    rec[f'{case}__values'] = np.array(values, dtype=np.float64)


def maps(rng, kind, shape):
    est = (rng.random(shape) < 0.1).astype(np.float64)
    ref = (rng.random(shape) < 0.1).astype(np.float64)
    if kind == 'silent_est':
        est[:] = 0
    elif kind == 'silent_ref':
        ref[:] = 0
    elif kind == 'both_silent':
        est[:] = 0
        ref[:] = 0
    elif kind == 'perfect':
        est = ref.copy()
    return est, ref


def tabs(rng, kind):
    est = rng.integers(-1, 20, size=(6, T)).astype(np.int64)
    ref = np.where(rng.random((6, T)) < 0.6, est, rng.integers(-1, 20, size=(6, T))).astype(np.int64)
    if kind == 'silent_est':
        est[:] = -1
    elif kind == 'silent_ref':
        ref[:] = -1
    elif kind == 'both_silent':
        est[:] = -1
        ref[:] = -1
    elif kind == 'perfect':
        est = ref.copy()
    elif kind == 'duplicate_pitch':
        est[0, 3], est[1, 3] = 5, 0              # E2 + 5 = A2 + 0: one cell of the collapsed map
        ref[0, 3], ref[1, 3] = 5, 0
        est[0, 9], est[1, 9] = 5, 0              # the reference sounds that pitch on one string only
        ref[0, 9], ref[1, 9] = -1, 0
        est[2, 11], est[3, 11] = -1, 0           # and the other way round: D3 + 5 = G3 + 0
        ref[2, 11], ref[3, 11] = 5, 0
    return est, ref


def main():
    profile = rtools.GuitarProfile(num_frets=19)
    rec = {'provenance': np.array(PROVENANCE), 'kinds': np.array(['random', 'silent_est', 'silent_ref', 'both_silent', 'perfect', 'duplicate_pitch'])}
    rng = np.random.default_rng(2718)
    for kind in rec['kinds']:
        kind = str(kind)
        est, ref = maps(rng, kind, (S, K, T))
        rec[f'stacked_{kind}_est'], rec[f'stacked_{kind}_ref'] = est, ref
        record(rec, f'stacked_{kind}', rev.StackedMultipitchEvaluator().evaluate(est.copy(), ref.copy()))
        record(rec, f'stacked_avg_{kind}', rev.StackedMultipitchEvaluator(average_slices=True).evaluate(est.copy(), ref.copy()))
        record(rec, f'multipitch_{kind}', rev.MultipitchEvaluator().evaluate(est[0].copy(), ref[0].copy()))
        te, tr = tabs(rng, kind)
        rec[f'tab_{kind}_est'], rec[f'tab_{kind}_ref'] = te, tr
        record(rec, f'tablature_{kind}', rev.TablatureEvaluator(profile).evaluate(te.copy(), tr.copy()))
        record(rec, f'softmax_{kind}', rev.SoftmaxAccuracy().evaluate(te.copy(), tr.copy()))
    # LossWrapper + ComboEvaluator over three tracks: per-track results, the tracked (appended) results and their average
    combo = rev.ComboEvaluator([rev.LossWrapper(), rev.MultipitchEvaluator(), rev.StackedMultipitchEvaluator(results_key='per-slice'),
                                rev.TablatureEvaluator(profile), rev.SoftmaxAccuracy(results_key=rtools.KEY_TABLATURE)])
    tracked = dict()
    for n, kind in enumerate(('random', 'perfect', 'duplicate_pitch')):
        loss = {rtools.KEY_LOSS_TOTAL: np.float64(0.5 + n), rtools.KEY_LOSS_PITCH: np.float64(0.25 * n)}
        rec[f'combo_track{n}_loss'] = np.array([loss[rtools.KEY_LOSS_TOTAL], loss[rtools.KEY_LOSS_PITCH]])
        est = {rtools.KEY_LOSS: loss, rtools.KEY_MULTIPITCH: rec[f'stacked_{kind}_est'].copy(), rtools.KEY_TABLATURE: rec[f'tab_{kind}_est'].copy()}
        ref = {rtools.KEY_MULTIPITCH: rec[f'stacked_{kind}_ref'].copy(), rtools.KEY_TABLATURE: rec[f'tab_{kind}_ref'].copy()}
        # MultipitchEvaluator takes slice 0 through its own unpack key
        est['mp0'], ref['mp0'] = est[rtools.KEY_MULTIPITCH][0], ref[rtools.KEY_MULTIPITCH][0]
        combo.evaluators[1].unpack_key = 'mp0'
        results = combo.process_track(est, ref, f'track{n}')
        record(rec, f'combo_track{n}', results)
        tracked = rev.append_results(tracked, results)
    record(rec, 'combo_average', combo.average_results())
    keys, _ = flatten(rev.average_results(tracked))
    rec['appended__keys'] = np.array(keys)
    rec['appended__values'] = np.stack([np.atleast_1d(np.asarray(_get(tracked, k), dtype=np.float64)) for k in keys])
    record(rec, 'appended_average', rev.average_results(tracked))
    path = os.path.join(OUT, 'evaluators.npz')
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), 'bytes;', len(rec), 'arrays')


def _get(d, path):
    for k in path.split('/'):
        d = d[k] if k in d else d[int(k)]
    return d


if __name__ == '__main__':
    main()
