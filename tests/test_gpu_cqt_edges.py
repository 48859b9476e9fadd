"""GPU parity of the CQT / VQT / HCQT front-end (csrc/cqt.hip, csrc/cqt_dec.hip) with the fp64 oracle (oracle/cqt_np.py) where
tests/test_gpu_cqt.py does not look: clips from one sample up, every size at which the route changes, plans that run cqt_basis_kernel<4>,
single-level plans, partial octaves, other rates, hops and harmonic sets, the GEMM fallback on its own, strided batches through the C ABI
with NaN around every row, maps below / across / above amin, the shortest clip the reflecting pad takes, and the 16-bit maps at T = 1.

Cases, inputs and bounds live in tests/cqt_ref.py; tests/test_cqt_ref.py shows on the CPU that an evaluation with the kernels' operand
roundings and exact accumulation stays within half of every bound on every case here, and that a one-plane operand, a dropped k-step or a
wrong pad misses TOL_LIN by a factor 10 or more.  Every test prints its figures (`CQTEDGE ...`) before it asserts.

Measured on the MI355X (cqt_ref.MEASURED holds the figures per family): linear 1.12e-5 at most (a clip of 3 samples; 6.2e-6 on whole
clips), dB on noise clips 3.10e-5, dB on tonal clips 3.98e-4 -- against TOL_LIN 4.5e-5, TOL_DB_BROADBAND 1e-4, TOL_DB_TONAL 1e-3.
Every route is the expected one.  Against a library whose windowed kernel drops its lo.hi product 56 of the 110 tests here fail (all 45
oracle comparisons on the windowed route, none on the GEMM route); with the decimator's second and third tap planes zeroed, 80.

Found by test_strided_batch_reads_nothing_outside_its_clips: the scaling kernels fused 10 log10(a) - offs into one fma, so the bin that is
the map's maximum came out as the rounding residue of offs -- 0.99999994 instead of 1.0 for a quiet clip (10 log10(max power) <= -64 dB).
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import cqt_ref as R                               # noqa: E402

CASES = R.cqt_cases()
BY_NAME = {c['name']: c for c in CASES}
DEV = 'cuda:0'


def _key(c):
    return tuple(sorted((k, v) for k, v in c.items()))


@functools.lru_cache(maxsize=None)
def _module_of(key):
    from amt_tools_amd import features as F
    c = dict(key)
    kw = dict(sample_rate=c['sr'], hop_length=c['hop'], fmin=c['fmin'], n_bins=c['n_bins'], bins_per_octave=c['bpo'], librosa_version=c['lv'])
    kind = R.is_module_kind(c)
    if kind == 'CQT':
        return F.CQT(**kw)
    if kind == 'VQT':
        return F.VQT(gamma=c['gamma'], **kw)
    if kind == 'HCQT':
        return F.HCQT(harmonics=list(c['harmonics']), **kw)
    return F.HVQT(harmonics=list(c['harmonics']), gamma=c['gamma'], **kw)


def module(c):
    """One features module (and one plan) per configuration, shared by every test of this file; `decibels` is an argument of the forward."""
    return _module_of(_key(c))


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(input, oracle linear map, oracle dB map) of a case: computed once."""
    case = BY_NAME[name]
    y = R.make_input(case)
    lin = R.oracle_mag(case['cfg'], y)
    for a in (y, lin):
        a.setflags(write=False)
    db = R.to_db(lin)
    db.setflags(write=False)
    return y, lin, db


def run(mod, y, decibels):
    mod.decibels = decibels
    try:
        return mod.process_audio(y)
    finally:
        mod.decibels = True


def db_bound(case):
    return R.TOL_DB_TONAL if case['input'] == 'tonal' else R.TOL_DB_BROADBAND


def check_against_oracle(tag, got_lin, got_db, ref_lin, ref_db, bound_db):
    assert got_lin.shape == got_db.shape == ref_lin.shape == ref_db.shape and got_lin.dtype == got_db.dtype == np.float32
    assert np.isfinite(got_lin).all() and np.isfinite(got_db).all()
    lin, db = R.lin_metric(got_lin, ref_lin), R.db_metric(got_db, ref_db)
    print(f'CQTEDGE {tag} shape {ref_lin.shape} lin {lin:.3e} db {db:.3e} (bounds {R.TOL_LIN:.1e} {bound_db:.1e})')
    assert lin < R.TOL_LIN, (tag, lin)
    assert db < bound_db, (tag, db)
    assert got_db.max() == 1.0 and got_db.min() >= 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# (a) lengths, (b) plans, (f) the shortest clip of the reflecting pad: every case of the table against the oracle
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c['name'] for c in CASES])
def test_case_matches_the_oracle(name):
    from amt_tools_amd import _lib
    case = BY_NAME[name]
    c = case['cfg']
    y, ref_lin, ref_db = _reference(name)
    mod = module(c)
    got_lin, got_db = run(mod, y, False), run(mod, y, True)
    frames = _lib.call('amtx_cqt_num_frames', mod._get_plan(DEV), len(y))
    assert got_lin.shape == (len(c['harmonics']), c['n_bins'], frames)
    if case['family'] == 'sweep' or len(c['harmonics']) > 1:         # the reference's own frame count: what HVQT truncates to, and what a CQT of whole octaves gives
        assert frames == mod.get_expected_frames(y)
    check_against_oracle(name, got_lin, got_db, ref_lin, ref_db, db_bound(case))


# ------------------------------------------------------------------------------------------------------------------------------
# (c) the route: which kernels ran
# ------------------------------------------------------------------------------------------------------------------------------
ROUTE_CASES = [c['name'] for c in CASES if c['route'] is not None and
               (c['family'] != 'sweep' or c['name'] in ('sweep-cqt84-n3', 'sweep-cqt84-n192', 'sweep-cqt84-n193', 'sweep-cqt84-n300', 'sweep-hcqt72-n2049'))]


def kernel_names(fn):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages()]


@pytest.mark.parametrize('name', ROUTE_CASES)
def test_route_is_the_expected_one(name):
    """cqt_forward_impl's decision, stated per case in cqt_ref (derived from the plan layout by hand): the windowed kernel
    (cqt_basis_kernel<4> for n_fft 128, <8> for 256) or the generic GEMM -- because of an n_fft, a hop, or a level shorter than 4 samples."""
    case = BY_NAME[name]
    y = _reference(name)[0]
    mod = module(case['cfg'])
    run(mod, y, True)                                                 # plan creation and workspace allocation stay out of the profile
    names = kernel_names(lambda: run(mod, y, True))
    assert any('cqt_scale_kernel' in k for k in names), names         # the profiler sees this library's kernels
    ran = sorted({k for k in (4, 8) if any(f'cqt_basis_kernel<{k}>' in n for n in names)})
    print(f'CQTEDGE route {name}: expected {case["route"]}, cqt_basis_kernel instantiations {ran}')
    want = {'windowed128': [4], 'windowed256': [8], 'windowed128+256': [4, 8]}.get(case['route'], [])
    assert case['route'].startswith('gemm:') or want
    assert ran == want, (name, case['route'], names)
    if not want:
        assert not any('cqt_basis_kernel' in n for n in names) and any('gemm' in n.lower() for n in names), names


def test_route_cases_cover_every_route():
    routes = {BY_NAME[n]['route'] for n in ROUTE_CASES}
    assert routes >= {'windowed128', 'windowed256', 'gemm:n_fft', 'gemm:hop', 'gemm:short'}, routes


# ------------------------------------------------------------------------------------------------------------------------------
# (d) strided batch through the C ABI, NaN everywhere a kernel must not look
# ------------------------------------------------------------------------------------------------------------------------------
ABI_N = R.ABI_N
ABI_FRONT = 515            # floats in front of the first row: the rows start at 4-byte, not 16-byte, boundaries


@functools.lru_cache(maxsize=None)
def _abi_clips():
    base = R.noise(ABI_N, 'abi-batch', draw=R.ABI_NOISE_DRAW)
    gains = dict(R.ABI_GAINS)
    clips = np.stack([base, np.zeros_like(base), base * np.float32(gains['quiet']), base * np.float32(gains['loud']),
                      R.tonal(ABI_N, R.ABI_TONAL_DRAW)]).astype(np.float32)
    clips.setflags(write=False)
    return clips


@functools.lru_cache(maxsize=None)
def _abi_reference(key):
    c = dict(key)
    lin = [R.oracle_mag(c, y) for y in _abi_clips()]
    return lin, [R.to_db(m) for m in lin]


@pytest.mark.parametrize('extra', [3, 1027])
@pytest.mark.parametrize('plan', ['cqt84', 'hcqt72', 'cqt84-lv09'])
def test_strided_batch_reads_nothing_outside_its_clips(plan, extra):
    """amtx_cqt_forward with audio_stride > num_samples: the level-0 basis product and the first decimation read the caller's buffer in place
    and must read zero outside every clip -- the gaps between the rows, the tail and a block in front of the first row hold NaN.  Every
    clip equals its own single-clip oracle; the silent clip's map is exactly 1.0 (linear: 0.0) between a loud and a quiet neighbour."""
    from amt_tools_amd import _lib
    c = dict(R.ABI_PLANS)[plan]
    clips = _abi_clips()
    B, n = clips.shape
    stride = n + extra
    host = np.full(ABI_FRONT + B * stride + 777, np.nan, dtype=np.float32)
    for b in range(B):
        host[ABI_FRONT + b * stride:ABI_FRONT + b * stride + n] = clips[b]
    buf = torch.from_numpy(host).to(DEV)
    view = buf[ABI_FRONT:]
    mod = module(c)
    handle = mod._get_plan(DEV)
    T, H = _lib.call('amtx_cqt_num_frames', handle, n), _lib.call('amtx_cqt_num_harmonics', handle)
    ws = _lib.alloc_workspace(_lib.call('amtx_cqt_workspace_bytes', handle, B, n), DEV)
    got = []
    for decibels in (0, 1):
        ws.fill_(0xff)                                                # NaN in the workspace as well
        out = torch.full((B, H, c['n_bins'], T), float('nan'), dtype=torch.float32, device=DEV)
        _lib.call('amtx_cqt_forward', handle, view, n, stride, B, decibels, ws, ws.numel(), out, device=DEV)
        got.append(out.cpu().numpy())
    assert torch.equal(torch.isnan(buf).cpu(), torch.from_numpy(np.isnan(host)))          # the caller's buffer is untouched
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
    ref_lin, ref_db = _abi_reference(_key(c))
    for b, kind in enumerate(('noise', 'silent', 'quiet', 'loud', 'tonal')):
        if kind == 'silent':
            np.testing.assert_array_equal(got[0][b], 0.0)
            np.testing.assert_array_equal(got[1][b], 1.0)
            continue
        check_against_oracle(f'abi-{plan}-stride+{extra}-{kind}', got[0][b], got[1][b], ref_lin[b], ref_db[b],
                             R.TOL_DB_TONAL if kind == 'tonal' else R.TOL_DB_BROADBAND)


# ------------------------------------------------------------------------------------------------------------------------------
# (e) amin
# ------------------------------------------------------------------------------------------------------------------------------
def test_maps_below_across_and_above_amin():
    """amplitude_to_db clamps magnitudes at amin = 1e-5.  Three gains of one noise clip, chosen with the oracle (and asserted on it): every
    magnitude below amin -- the map is all 1.0; the maximum above with three bins in ten below; everything above."""
    c = R.cfg(84, 12)
    mod = module(c)
    base = R.noise(6000, 'amin')
    unit = R.oracle_mag(c, base)
    gains = {'below': 0.5e-5 / unit.max(), 'across': 1e-5 / np.quantile(unit, 0.3), 'above': 2e-5 / unit.min()}
    for tag, gain in gains.items():
        y = (base * np.float32(gain)).astype(np.float32)
        ref_lin = R.oracle_mag(c, y)
        below = float((ref_lin < 1e-5).mean())
        print(f'CQTEDGE amin-{tag}: gain {gain:.3e}, oracle max {ref_lin.max():.3e} min {ref_lin.min():.3e}, below amin {below:.2f}')
        if tag == 'below':
            assert ref_lin.max() < 0.6e-5
        elif tag == 'across':
            assert ref_lin.max() > 2e-5 and 0.1 <= below <= 0.9
        else:
            assert ref_lin.min() > 1.5e-5
        got_lin, got_db = run(mod, y, False), run(mod, y, True)
        if tag == 'below':
            np.testing.assert_array_equal(got_db, np.ones_like(got_db))
            assert R.lin_metric(got_lin, ref_lin) < R.TOL_LIN
        else:
            check_against_oracle(f'amin-{tag}', got_lin, got_db, ref_lin, R.to_db(ref_lin), R.TOL_DB_BROADBAND)


# ------------------------------------------------------------------------------------------------------------------------------
# (f) the reflecting pad's refusal just below its shortest clip (the shortest clips themselves are cases of the table)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['reflect-cqt84-shortest', 'reflect-cqt192-shortest'])
def test_reflect_pad_refuses_a_shorter_clip_and_goes_on(name):
    from amt_tools_amd import _lib
    case = BY_NAME[name]
    c = case['cfg']
    y, ref_lin, ref_db = _reference(name)
    _, n_levels, pad = R.plan_layout(c)
    assert len(y) == pad * 2 ** (n_levels - 1) + 1 and R.level_lengths(len(y), n_levels)[-1] == pad + 1
    assert R.level_lengths(len(y) - 64, n_levels)[-1] == pad
    mod = module(c)
    with pytest.raises(_lib.AmtxError, match='reflect padding'):
        mod.process_audio(y[:len(y) - 64])
    with pytest.raises(_lib.AmtxError, match='reflect padding'):
        mod.process_audio(y[:len(y) - 1])
    check_against_oracle(name + '-after-refusal', run(mod, y, False), run(mod, y, True), ref_lin, ref_db, R.TOL_DB_BROADBAND)


# ------------------------------------------------------------------------------------------------------------------------------
# (g) the 16-bit maps at one frame and at one frame more than a 32-frame tile
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,T', [(300, 1), (16500, 33)])
@pytest.mark.parametrize('decibels', [True, False])
def test_16_bit_maps_at_one_frame_and_one_past_a_tile(n, T, decibels):
    """process_batch16 / split=True: the fp32 map rounded to bf16 (and the rounding's remainder), channels last, slots 6 .. 7 zero, bit for bit."""
    mod = module(R.cfg(72, 12, harmonics=R.HCQT_DEFAULT))
    audio = torch.from_numpy(np.stack([R.noise(n, f'feats16-{i}') for i in range(2)])).to(DEV)
    mod.decibels = decibels
    try:
        f32 = mod.process_batch(audio)                                # (B, 6, 72, T)
        one = mod.process_batch16(audio)
        two = mod.process_batch16(audio, split=True)
    finally:
        mod.decibels = True
    assert f32.shape == (2, 6, 72, T) and one.shape == (2, T, 72, 8) and two.shape == (2, 2, T, 72, 8)
    want = f32.permute(0, 3, 2, 1)
    hi = want.to(torch.bfloat16)
    lo = (want - hi.float()).to(torch.bfloat16)
    assert torch.equal(one[..., :6].view(torch.int16), hi.contiguous().view(torch.int16)) and torch.equal(two[0], one)
    assert torch.equal(two[1][..., :6].view(torch.int16), lo.contiguous().view(torch.int16))
    assert not one[..., 6:].view(torch.int16).any() and not two[..., 6:].view(torch.int16).any()
    ref = R.oracle_mag(R.cfg(72, 12, harmonics=R.HCQT_DEFAULT), audio[0].cpu().numpy())
    if decibels:
        assert R.db_metric(f32[0].cpu().numpy(), R.to_db(ref)) < R.TOL_DB_BROADBAND
    else:
        assert R.lin_metric(f32[0].cpu().numpy(), ref) < R.TOL_LIN
