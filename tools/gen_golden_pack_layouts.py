#!/usr/bin/env python3
"""
Golden hashes of the packed weight layouts: tests/golden/pack_layouts.json, read by tests/test_pack_layouts.py (which imports
`record` from here).  Recorded on the commit BEFORE the layouts moved into csrc/amtx_pack_layouts.h, through the op-level host
packers of the built library (no GPU): the SHA-256 of every output buffer.

Inputs: standard_normal weights (float32) from numpy's default PCG64 generator seeded with [SEED, case number], the scale (where
the packer takes one) `random()` from the same generator behind the weights.  Cases, each with planes 1 and 2:
  amtx_conv3x3_pack      c_out 32, 64; scale None and random
  amtx_conv3x3g_pack     (48,48) (48,96) (64,64) (64,128) (80,80) (80,160): model_complexity 3, 4, 5, with and without a 16-channel
                         tail; scale None and random.  A pair the library does not build (amtx_conv3x3g_packed_elems 0) is listed
                         under "skipped"
  amtx_linear_pack       (7,5) (88,176) (88,256) (300,1000) (512,3648) (1024,512): ragged N and K, both pads, the engine's shapes
  amtx_bilstm_h_pack     hidden 128, 256, 384, 512; amtx_bilstm_pack (hidden 128) on the SAME weights: recorded under its own name, the
                         test also wants the two alike

    python tools/gen_golden_pack_layouts.py [path of libamtx.so]
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'pack_layouts.json')
SEED = 20261018
CONV3X3 = (32, 64)
CONV3X3G = ((48, 48), (48, 96), (64, 64), (64, 128), (80, 80), (80, 160))
LINEAR = ((7, 5), (88, 176), (88, 256), (300, 1000), (512, 3648), (1024, 512))
HIDDEN = (128, 256, 384, 512)


def record(L, P):
    """{'seed', 'skipped', 'hashes': {case: sha256}} of library `L` (ctypes, the signatures of amt_tools_amd._lib; P = its `ptr`)."""
    hashes, skipped, case = {}, [], [0]

    def rng():
        case[0] += 1
        return np.random.default_rng([SEED, case[0]])

    def put(name, rc, out):
        assert rc == 0, (name, rc, L.amtx_last_error())
        hashes[name] = hashlib.sha256(out.tobytes()).hexdigest()

    def conv(name, pack, elems, shape, args):
        g = rng()
        w = g.standard_normal(shape).astype(np.float32)
        sc = g.random(shape[0]).astype(np.float32)
        for planes in (1, 2):
            n = elems(planes)
            if n <= 0:
                skipped.append(f'{name} planes {planes}')
                continue
            for label, s in (('none', None), ('random', P(sc))):
                out = np.zeros(n, np.uint16)
                put(f'{name} planes {planes} scale {label}', pack(P(w), s, *args, planes, P(out)), out)

    for c_out in CONV3X3:
        conv(f'conv3x3 {c_out}', L.amtx_conv3x3_pack, lambda pl: L.amtx_conv3x3_packed_elems(c_out, pl), (c_out, 32, 3, 3), (c_out,))
    for c_in, c_out in CONV3X3G:
        conv(f'conv3x3g {c_in}->{c_out}', L.amtx_conv3x3g_pack, lambda pl: L.amtx_conv3x3g_packed_elems(c_in, c_out, pl), (c_out, c_in, 3, 3), (c_in, c_out))
    for n, k in LINEAR:
        w = rng().standard_normal((n, k)).astype(np.float32)
        for planes in (1, 2):
            out = np.zeros(L.amtx_linear_packed_elems(n, k, planes), np.uint16)
            put(f'linear {n}x{k} planes {planes}', L.amtx_linear_pack(P(w), n, k, planes, P(out)), out)
    for hid in HIDDEN:
        g = rng()
        wf = g.standard_normal((4 * hid, hid)).astype(np.float32)
        wb = g.standard_normal((4 * hid, hid)).astype(np.float32)
        for planes in (1, 2):
            out = np.zeros(L.amtx_bilstm_h_packed_elems(hid, planes), np.uint16)
            put(f'bilstm_h {hid} planes {planes}', L.amtx_bilstm_h_pack(P(wf), P(wb), hid, planes, P(out)), out)
            if hid == 128:
                out = np.zeros(L.amtx_bilstm_packed_elems(planes), np.uint16)
                put(f'bilstm 128 planes {planes}', L.amtx_bilstm_pack(P(wf), P(wb), planes, P(out)), out)
    return {'seed': SEED, 'skipped': skipped, 'hashes': hashes}


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    from amt_tools_amd import _lib
    if len(sys.argv) > 1:
        _lib.LIB_PATH = sys.argv[1]
    got = record(_lib.lib(), _lib.ptr)
    with open(OUT, 'w') as f:
        json.dump(got, f, indent=1)
        f.write('\n')
    print(OUT, len(got['hashes']), 'hashes,', len(got['skipped']), 'skipped')
