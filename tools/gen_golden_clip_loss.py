#!/usr/bin/env python3
"""
Golden vectors of the per-clip loss sums: tests/golden/clip_loss.npz.  Like tools/gen_golden_tab.py (it reuses the import stubs of
tools/gen_golden.py by importing it) this runs ONLY where the reference checkout is present; the test-suite reads the fixture, never
the reference.

Recorded: inputs, and what the REAL amt_tools output layers answer for them as float32 --
  LogisticBank.get_loss   logits (1, 12, 88), labels (1, 88, 12), without and with per-key weights
  SoftmaxGroups.get_loss  logits (1, 9, 126) = 6 groups x 21 classes, targets (1, 6, 9) in [-1, 20] (-1 and 20 both occur: the same
                          class), without and with per-(group, class) weights
-- on batches of ONE: the reference's loss of a clip, sum_k mean_t, which amt_tools_amd.cliploss restates as sums / T.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden                                   # noqa: E402,F401  (installs the stubs, puts the reference on sys.path)
from gen_golden import OUT                          # noqa: E402
from amt_tools.models.common import LogisticBank, SoftmaxGroups   # noqa: E402

T_BCE, KEYS = 12, 88
T_SM, GROUPS, CLASSES = 9, 6, 21


def main():
    rng = np.random.default_rng(20240)
    rec = {}
    x = (4.0 * rng.standard_normal((1, T_BCE, KEYS))).astype(np.float32)
    y = (rng.random((1, KEYS, T_BCE)) < 0.25).astype(np.float32)
    w = (0.5 + rng.random(KEYS)).astype(np.float32)
    rec['bce_logits'], rec['bce_labels'], rec['bce_weight'] = x, y, w
    for name, weights in (('bce_loss', None), ('bce_loss_weighted', w)):
        layer = LogisticBank(16, KEYS)
        if weights is not None:
            layer.set_weights(weights)              # (the constructor's own weighted branch reads self.weights before it is set)
        with torch.no_grad():
            loss = layer.get_loss(torch.from_numpy(x), torch.from_numpy(y))
        assert loss.dtype == torch.float32 and loss.dim() == 0
        rec[name] = loss.numpy()
    x = (4.0 * rng.standard_normal((1, T_SM, GROUPS * CLASSES))).astype(np.float32)
    t = rng.integers(-1, CLASSES, size=(1, GROUPS, T_SM)).astype(np.int64)
    t[0, 0, 0], t[0, 1, 0], t[0, 2, 1] = -1, CLASSES - 1, 0
    w = (0.5 + rng.random(GROUPS * CLASSES)).astype(np.float32)
    rec['sm_logits'], rec['sm_targets'], rec['sm_weight'] = x, t, w
    for name, weights in (('sm_loss', None), ('sm_loss_weighted', w)):
        layer = SoftmaxGroups(16, GROUPS, CLASSES)
        if weights is not None:
            layer.set_weights(weights)
        with torch.no_grad():
            loss = layer.get_loss(torch.from_numpy(x), torch.from_numpy(t))
        assert loss.dtype == torch.float32 and loss.dim() == 0
        rec[name] = loss.numpy()
    assert (t == -1).any() and (t == CLASSES - 1).any()
    path = os.path.join(OUT, 'clip_loss.npz')
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), 'bytes;', {k: float(v) for k, v in rec.items() if k.endswith(('loss', 'weighted'))})


if __name__ == '__main__':
    main()
