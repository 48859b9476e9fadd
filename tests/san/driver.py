"""Runs INSIDE the sanitizer process (LD_PRELOAD = clang's ASan runtime; started by tests/test_sanitized_host.py): drives the host halves
of the C ABI through tests/san/_build/libamtx_san.so -- weight packers at ragged sizes, amtx_of_model_create / set_tensor / finalize for
every engine configuration (their BatchNorm folding, fc1 permutation, fp64 head folding, fragment packing), the argument checks and
workspace carving of the forward entry points (the first kernel launch then reports "no device" through the shim: that is the expected
error), spectrogram and CQT plan builders.  numpy + ctypes only; any ASan / UBSan report aborts the process.

With a second argument it also writes, as JSON, what the engine DECIDES and PACKS: for each of the engine configurations below the hash of
the bytes amtx_of_model_finalize uploads (the shim's hipMemcpy sees them), and for those plus a grid of small models -- model_complexity
2 .. 5 x input channels x precision x offset head x each create-time A/B switch (thinned at model_complexity 4 and 5) -- the answers of the query entry points, the workspace
sizes and the device re-sync's support check.  tests/golden/of_conv_plan.json is that file as the commit before the ConvPlan refactor
wrote it; tests/test_sanitized_host.py requires every row of it back.

With a third argument it does none of that: it writes, as JSON, the LAUNCH TRACE -- the shim records every kernel launch (name, grid,
block, dynamic LDS bytes) instead of refusing it -- of a grid of GEMM problems through amtx_linear_fwd / amtx_linear_fwd_split and of whole
forward passes of the engine configurations.  The A/B switches of the launchers are sampled once per process: tests/san/launch_trace.py
runs this mode once per switch and tests/golden/launch_trace.json is what it recorded on the commit before gemm.hip's routing became
one function."""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_lib = _load('amtx_lib_san', os.path.join(ROOT, 'amt_tools_amd', '_lib.py'))          # the product's own binding table, without the package
synth = _load('amtx_synth_san', os.path.join(ROOT, 'amt_tools_amd', 'synth.py'))
_lib.LIB_PATH = sys.argv[1]
L = _lib.lib()
P = _lib.ptr
missing = [s for s in _lib.declared_symbols() if not hasattr(L, s)]
assert not missing, missing
rng = np.random.default_rng(0)
n_calls = 0
L.amtx_san_upload_hash_take.restype = C.c_uint64
L.amtx_san_upload_hash_take.argtypes = []
PLAN_BT = ((1, 1), (3, 17), (130, 47), (43, 140), (1024, 625))
PLAN_COLUMNS = ['dim_in', 'in_channels', 'model_complexity', 'offsets', 'precision', 'switch', 'fuses_db_scale', 'takes_feats16'] + \
               [f'conv_stack_fused_{B}x{T}' for B, T in PLAN_BT] + [f'workspace_bytes_{B}x{T}' for B, T in PLAN_BT] + ['finalize_device_rc', 'finalize_device_error']
PLAN_SWITCHES = ('', 'AMTX_NO_CONVG_MC2', 'AMTX_NO_CONV_FUSE', 'AMTX_X3_NO_SPLIT', 'AMTX_NO_CONVX12M')


def plan_row(h, cfg, switch):
    """What a finalized model decides, through the C ABI only.  The device re-sync is called with no device tensor set: it answers its support
    check, or the first missing tensor."""
    rc = L.amtx_of_model_finalize_device(h, None)
    err = L.amtx_last_error().decode()
    return [cfg['dim_in'], cfg['ch'], cfg['mc'], cfg['off'], cfg['prec'], switch, L.amtx_of_fuses_db_scale(h), L.amtx_of_takes_feats16(h)] + \
           [L.amtx_of_conv_stack_fused(h, B, T) for B, T in PLAN_BT] + [L.amtx_of_workspace_bytes(h, B, T) for B, T in PLAN_BT] + [rc, err]


# the engine configurations: (input bins, input channels, model_complexity, offset head, precision bf16 / x3 / f16)
configs = [dict(dim_in=229, ch=1, mc=2, off=0, prec=0), dict(dim_in=229, ch=1, mc=2, off=0, prec=1), dict(dim_in=229, ch=1, mc=2, off=0, prec=2),
           dict(dim_in=229, ch=1, mc=3, off=1, prec=0), dict(dim_in=229, ch=1, mc=3, off=0, prec=1), dict(dim_in=72, ch=6, mc=2, off=0, prec=0),
           dict(dim_in=72, ch=6, mc=3, off=1, prec=1), dict(dim_in=72, ch=6, mc=2, off=0, prec=2), dict(dim_in=229, ch=1, mc=3, off=1, prec=2), dict(dim_in=8, ch=1, mc=2, off=1, prec=0), dict(dim_in=40, ch=1, mc=2, off=0, prec=2),
           dict(dim_in=5, ch=1, mc=2, off=0, prec=0), dict(dim_in=192, ch=2, mc=2, off=0, prec=0)]


def make_model(cfg):
    """amtx_of_model_create + set_tensor with synthetic weights; the caller finalizes and destroys."""
    h = C.c_void_p()
    _lib.check(L.amtx_of_model_create(C.byref(h), cfg['dim_in'], cfg['ch'], cfg['mc'], 88, cfg['off'], cfg['prec']), 'create')
    sd = synth.synth_state_dict(3, dim_in=cfg['dim_in'], in_channels=cfg['ch'], model_complexity=cfg['mc'], offsets=bool(cfg['off']))
    for k, v in sd.items():
        a = np.ascontiguousarray(np.asarray(v), dtype=np.float32)
        if a.dtype.kind != 'f' or a.size == 0 or 'num_batches_tracked' in k:
            continue
        _lib.check(L.amtx_of_model_set_tensor(h, k.encode(), P(a), a.size), 'set_tensor')
    return h


# ---------------------------------------------------------------- launch trace (a third argument: instead of everything below)
GEMM_M = (1, 255, 256, 1023, 1024, 4096)
GEMM_N = (4, 88, 128, 256, 512, 1024, 2048)
GEMM_K = (8, 64, 128, 176, 192, 512, 1024, 1088, 3648)
TRACE_BT = ((2, 9), (3, 17), (130, 47), (43, 140))
TRACE_BIG = (1024, 625)          # configs[0] only: the fused stack, the 256-tile, ring and skinny GEMMs, planar A


def traced(call):
    """[return code, error text, launches] of one library call with the shim recording: nothing runs, every launch "succeeds"."""
    L.amtx_san_trace_begin()
    rc = call()
    return [rc, L.amtx_last_error().decode() if rc else '', L.amtx_san_trace_take().decode().splitlines()]


def reserve(nbytes):
    """Address space nothing may touch (the launches do not run): untouched pages of an anonymous mapping cost no memory."""
    import mmap
    mm = mmap.mmap(-1, nbytes + 256, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | getattr(mmap, 'MAP_NORESERVE', 0x4000))
    return mm, (C.addressof(C.c_char.from_buffer(mm)) + 255) // 256 * 256


def trace_gemm():
    """amtx_linear_fwd / amtx_linear_fwd_split over the whole M x N x K x lda x type grid (one call is microseconds: no thinning).  The
    pointers are one 16-byte aligned address: routing looks at alignment only."""
    buf = np.empty(64, np.uint8)
    p = C.c_void_p((buf.ctypes.data + 15) // 16 * 16)
    rows = []
    for m in GEMM_M:
        for n in GEMM_N:
            for k in GEMM_K:
                for lda in (k, k + 8):
                    for a_type in (0, 1, 2):
                        for c_type in (0, 1, 2):
                            for planes in (1, 2):
                                rows.append(traced(lambda: L.amtx_linear_fwd(p, lda, a_type, p, planes, p, p, n, c_type, m, n, k, None)))
                    for c_type in (0, 1, 2):
                        rows.append(traced(lambda: L.amtx_linear_fwd_split(p, lda, m * lda, p, p, p, n, c_type, m * n, m, n, k, None)))
    return rows


def trace_engine():
    """Every launch of amtx_of_forward (and _power / _feats16 where the model takes them), with all outputs and with the rolls only."""
    seqs = {}
    for cfg in configs:
        h = make_model(cfg)
        _lib.check(L.amtx_of_model_finalize(h), 'finalize')
        F, ch = cfg['dim_in'], cfg['ch']
        for B, T in TRACE_BT + ((TRACE_BIG,) if cfg is configs[0] else ()):
            need = L.amtx_of_workspace_bytes(h, B, T)
            fbytes, obytes = max(B * ch * T * F * 4, 2 * B * T * F * 8 * 2), B * 88 * T * 4
            big = (B, T) == TRACE_BIG
            if big:         # never touched: no output copies are asked for at this size
                keep, base = reserve(need + fbytes + 2 * obytes + 1024)
                ws, feats, outs = base, base + (need + 255) // 256 * 256, [base + (need + fbytes + 511) // 256 * 256 + i * obytes for i in range(2)]
            else:           # zeroed host memory: the logit copies of the shim are real, and instrumented
                keep = [np.zeros(need + 256, np.uint8), np.zeros(fbytes, np.uint8)] + [np.zeros(obytes, np.uint8) for _ in range(5)]
                ws, feats, outs = (keep[0].ctypes.data + 255) // 256 * 256, keep[1].ctypes.data, [a.ctypes.data for a in keep[2:]]
            ws, feats = C.c_void_p(ws), C.c_void_p(feats)
            for what in ('rolls',) if big else ('all', 'rolls'):
                o = [C.c_void_p(x) for x in outs] if what == 'all' else [C.c_void_p(x) for x in outs[:2]] + [None] * 3
                name = '%d/%d/%d/%d/%d %dx%d %s ' % (F, ch, cfg['mc'], cfg['off'], cfg['prec'], B, T, what)
                seqs[name + 'forward'] = traced(lambda: L.amtx_of_forward(h, feats, ch * T * F, T * F, F, 1, B, T, ws, need, *o, None))
                if L.amtx_of_fuses_db_scale(h):
                    seqs[name + 'power'] = traced(lambda: L.amtx_of_forward_power(h, feats, T * F, F, 1, feats, None, B, T, ws, need, *o, None))
                if L.amtx_of_takes_feats16(h):
                    seqs[name + 'feats16'] = traced(lambda: L.amtx_of_forward_feats16(h, feats, B, T, ws, need, *o, None))
            del keep
        _lib.check(L.amtx_of_model_destroy(h))
    return seqs


if len(sys.argv) > 3:
    L.amtx_san_trace_begin.restype, L.amtx_san_trace_begin.argtypes = None, []
    L.amtx_san_trace_take.restype, L.amtx_san_trace_take.argtypes = C.c_char_p, []
    with open(sys.argv[3], 'w') as f:
        json.dump({'gemm': trace_gemm(), 'engine': trace_engine()}, f)
    print('launch trace written')
    sys.exit(0)

plan_rows, upload_hashes = [], []

# ---------------------------------------------------------------- weight packers (op-level C ABI)
for planes in (1, 2):
    for c_out in (32, 64):
        w = rng.standard_normal((c_out, 32, 3, 3)).astype(np.float32)
        sc = rng.random(c_out).astype(np.float32)
        out = np.zeros(L.amtx_conv3x3_packed_elems(c_out, planes), np.uint16)
        _lib.check(L.amtx_conv3x3_pack(P(w), P(sc), c_out, planes, P(out)))
        _lib.check(L.amtx_conv3x3_pack(P(w), None, c_out, planes, P(out)))
        n_calls += 2
    for c_in, c_out in ((48, 48), (48, 96), (32, 32), (16, 16)):
        n = L.amtx_conv3x3g_packed_elems(c_in, c_out, planes)
        if n > 0:
            w = rng.standard_normal((c_out, c_in, 3, 3)).astype(np.float32)
            out = np.zeros(n, np.uint16)
            _lib.check(L.amtx_conv3x3g_pack(P(w), None, c_in, c_out, planes, P(out)))
            n_calls += 1
    for n_, k_ in ((88, 256), (1024, 512), (512, 3648), (1024, 176), (88, 3648), (7, 5), (300, 1000), (2048, 72)):
        w = rng.standard_normal((n_, k_)).astype(np.float32)
        out = np.zeros(L.amtx_linear_packed_elems(n_, k_, planes), np.uint16)
        _lib.check(L.amtx_linear_pack(P(w), n_, k_, planes, P(out)))
        n_calls += 1
    for hid in (128, 256):
        wf = rng.standard_normal((4 * hid, hid)).astype(np.float32)
        wb = rng.standard_normal((4 * hid, hid)).astype(np.float32)
        out = np.zeros(L.amtx_bilstm_h_packed_elems(hid, planes), np.uint16)
        _lib.check(L.amtx_bilstm_h_pack(P(wf), P(wb), hid, planes, P(out)))
        n_calls += 1
    out = np.zeros(L.amtx_bilstm_packed_elems(planes), np.uint16)
    wf = rng.standard_normal((512, 128)).astype(np.float32)      # named: a pointer taken from a temporary would dangle
    wb = rng.standard_normal((512, 128)).astype(np.float32)
    _lib.check(L.amtx_bilstm_pack(P(wf), P(wb), planes, P(out)))
    n_calls += 1

# ---------------------------------------------------------------- engine: create / set_tensor / finalize / workspace / argument checks
for cfg in configs:
    h = make_model(cfg)
    L.amtx_san_upload_hash_take()
    _lib.check(L.amtx_of_model_finalize(h), 'finalize')
    upload_hashes.append([cfg['dim_in'], cfg['ch'], cfg['mc'], cfg['off'], cfg['prec'], '%016x' % L.amtx_san_upload_hash_take()])
    plan_rows.append(plan_row(h, cfg, ''))
    for B, T in ((1, 1), (3, 17), (130, 47), (1024, 625)):
        need = L.amtx_of_workspace_bytes(h, B, T)
        assert need > 0
        L.amtx_of_conv_stack_fused(h, B, T)
    # forward: argument checks and workspace carving run on the host; the first kernel launch reports "no device" through the shim
    B, T = 2, 9
    need = L.amtx_of_workspace_bytes(h, B, T)
    ws = np.zeros(need + 256, np.uint8)
    base = (ws.ctypes.data + 255) // 256 * 256
    feats = rng.random((B, cfg['ch'], T, cfg['dim_in'])).astype(np.float32)
    on = np.zeros((B, 88, T), np.float32)
    mp = np.zeros((B, 88, T), np.float32)
    sb, sc_, st, sf = (s // 4 for s in feats.strides)
    rc = L.amtx_of_forward(h, P(feats), sb, sc_, st, sf, B, T, C.c_void_p(base), need, P(on), P(mp), None, None, None, None)
    assert rc != 0 and b'no device' in L.amtx_last_error(), (rc, L.amtx_last_error())
    rc = L.amtx_of_forward(h, P(feats), sb, sc_, st, sf, B, T, C.c_void_p(base), need - 1, P(on), P(mp), None, None, None, None)
    assert rc != 0 and b'workspace too small' in L.amtx_last_error()
    _lib.check(L.amtx_of_model_destroy(h))
    n_calls += 1
# an incomplete model must be refused by finalize, not read past a missing tensor
h = C.c_void_p()
_lib.check(L.amtx_of_model_create(C.byref(h), 229, 1, 2, 88, 0, 0))
assert L.amtx_of_model_finalize(h) != 0
_lib.check(L.amtx_of_model_destroy(h))

# ---------------------------------------------------------------- engine: the decision grid (small models: 20 bins, 4 keys; the weights do not matter)
if len(sys.argv) > 2:
    for mc in (2, 3, 4, 5):
        for ch in (1, 2, 3, 6, 8, 9):
            for off in (0, 1):
                sd = {k: np.full(shape, 0.5, np.float32) for k, shape in
                      synth.of_state_dict_shapes(dim_in=20, in_channels=ch, model_complexity=mc, dim_out=4, offsets=bool(off)).items() if 'num_batches_tracked' not in k}
                for prec in (0, 1, 2):
                    for switch in PLAN_SWITCHES:
                        # model_complexity 4 and 5 cost 0.2 .. 0.8 s each under ASan (their LSTMs) and decide alike whatever the switch: every
                        # channel count and precision without a switch and without offsets; offsets, and the switches (bf16, x3), at 1, 6, 9 channels
                        if mc >= 4 and (off or switch) and not (ch in (1, 6, 9) and (not switch or (not off and prec in (0, 1)))):
                            continue
                        cfg = dict(dim_in=20, ch=ch, mc=mc, off=off, prec=prec)
                        if switch:
                            os.environ[switch] = '1'
                        h = C.c_void_p()
                        _lib.check(L.amtx_of_model_create(C.byref(h), 20, ch, mc, 4, off, prec), 'create')
                        os.environ.pop(switch, None)
                        assert L.amtx_of_fuses_db_scale(h) == 0 and L.amtx_of_takes_feats16(h) == 0           # not finalized yet
                        for k, a in sd.items():
                            _lib.check(L.amtx_of_model_set_tensor(h, k.encode(), P(a), a.size), 'set_tensor')
                        _lib.check(L.amtx_of_model_finalize(h), 'finalize')
                        plan_rows.append(plan_row(h, cfg, switch))
                        _lib.check(L.amtx_of_model_destroy(h))
                        n_calls += 1
    with open(sys.argv[2], 'w') as f:
        f.write('{"plan_columns": %s,\n"plan_rows": [\n%s\n],\n"upload_hash_columns": ["dim_in", "in_channels", "model_complexity", "offsets", "precision", "fnv1a64"],\n'
                '"upload_hashes": [\n%s\n]}\n' % (json.dumps(PLAN_COLUMNS), ',\n'.join(json.dumps(r) for r in plan_rows), ',\n'.join(json.dumps(r) for r in upload_hashes)))

# ---------------------------------------------------------------- spectrogram and CQT plans (host-built tables, uploaded through the shim)
for sr, n_fft, hop, win, n_mels, htk, center, pad in ((22050, 2048, 512, 2048, 229, 0, 1, 0), (22050, 2048, 512, 2048, 229, 1, 1, 1), (16000, 1024, 160, 800, 80, 0, 0, 0),
                                                     (22050, 4096, 512, 4096, 512, 1, 1, 0), (22050, 128, 64, 128, 40, 0, 1, 0), (44100, 2048, 441, 2048, 0, 0, 1, 0)):
    pl = C.c_void_p()
    rc = L.amtx_spec_plan_create(C.byref(pl), sr, n_fft, hop, win, n_mels, htk, center, pad)
    if rc != 0:
        continue
    nb = L.amtx_spec_num_bins(pl)
    assert nb > 0 and L.amtx_spec_num_frames(pl, 22050) > 0
    if n_mels:
        fb = np.zeros((n_mels, n_fft // 2 + 1), np.float32)
        _lib.check(L.amtx_spec_filterbank(pl, P(fb)))
        assert np.isfinite(fb).all() and fb.max() > 0
    _lib.check(L.amtx_spec_plan_destroy(pl))
    n_calls += 1
    if n_mels:       # the slot matching of the mel gather (mel_assign_slots), host-only
        srow, sstart, rmax = np.full(512, -5, np.int32), np.zeros(512, np.int32), np.zeros(8, np.int32)
        rounds = L.amtx_spec_mel_layout(sr, n_fft, n_mels, htk, P(srow), P(sstart), P(rmax))
        assert rounds == (n_mels + 63) // 64 and sorted(srow[:64 * rounds][srow[:64 * rounds] >= 0].tolist()) == list(range(n_mels))
        n_calls += 1
for fmin, n_bins, bpo, harm in ((82.41, 192, 24, [1.0]), (32.70, 72, 12, [0.5, 1, 2, 3, 4, 5]), (27.5, 88, 12, [1.0])):
    pl = C.c_void_p()
    hv = (C.c_double * len(harm))(*harm)
    rc = L.amtx_cqt_plan_create(C.byref(pl), 22050, 512, fmin, n_bins, bpo, 0.0, hv, len(harm), 1, 0)
    if rc == 0:
        assert L.amtx_cqt_num_harmonics(pl) == len(harm) and L.amtx_cqt_num_frames(pl, 22050 * 4) > 0
        assert L.amtx_cqt_workspace_bytes(pl, 3, 22050 * 4) > 0
        _lib.check(L.amtx_cqt_plan_destroy(pl))
        n_calls += 1
print(f'sanitized host halves: {n_calls} packer / model / plan exercises, no report')
