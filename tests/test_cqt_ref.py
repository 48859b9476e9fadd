"""tests/cqt_ref.py without any kernel, on every case tests/test_gpu_cqt_edges.py runs:

* the time-domain fold-back the kernels rest on (sparsified FFT basis -> n_fft-tap complex kernel on strided windows of the decimated
  signal) IS the oracle's frequency-domain transform: 'exact' equals cq.vqt to 1e-10 of the map maximum (measured: 2.5e-14 at most);
* the kernels' operand roundings with exact accumulation ('ideal') stay within half of TOL_LIN and half of the case's dB bound -- so a
  bound a kernel misses is the kernel's doing, not the input's;
* every single-stage mutation (an operand of the basis product in one bf16 plane, decimator taps in one bf16 plane, one 32-deep k-step
  dropped, the reflecting pad one sample off, the decimator reading the reflecting pad) moves the linear metric by at least
  10 x TOL_LIN on every case that contains the stage -- so a kernel with such a bug cannot pass.

Figures over the 70 cases (python -m pytest tests/test_cqt_ref.py -s prints them per case):
    exact against the oracle          3e-16 .. 2.5e-14
    ideal, linear                     1.8e-6 .. 1.1e-5    (TOL_LIN / 2 = 2.25e-5; the largest on clips of 1 .. 3 samples, 6.4e-6 otherwise)
    ideal, dB, noise                  7e-7 .. 3.2e-5      (TOL_DB_BROADBAND / 2 = 5e-5)
    ideal, dB, tonal                  1.3e-4 .. 3.8e-4    (TOL_DB_TONAL / 2 = 5e-4; other synth_clips reach 3e-3 on HCQT maps: cqt_ref.DRAWS)
    weights in one plane              6.1e-4 .. 2.4e-3    signal in one plane      5.4e-4 .. 2.5e-3       (floor: 10 x TOL_LIN = 4.5e-4)
    one k-step dropped                6.7e-2 .. 1.0       taps in one plane        6.2e-4 .. 1.4e-2 (lowest octave, three levels or more)
    pad shifted (0.9)                 0.28 .. 0.61        decimator reads the pad  2.9e-3 .. 7.1e-2 (first and last two frames)
    two-plane decimator input         3.9e-6 -> 5.6e-6 on the 8-octave CQT: inside the ideal evaluation's own spread, recorded, not asserted
"""
import functools

import numpy as np
import pytest

import cqt_ref as R
from oracle import cqt_np as cq

CASES = R.cqt_cases()
BY_NAME = {c['name']: c for c in CASES}
NAMES = [c['name'] for c in CASES]


@functools.lru_cache(maxsize=None)
def _reference(name):
    case = BY_NAME[name]
    y = R.make_input(case)
    return y, R.oracle_mag(case['cfg'], y)


def _layout(c):
    levels, n_levels, pad = R.plan_layout(c)
    n_oct = -(-c['n_bins'] // c['bpo'])
    lowest = slice(0, c['n_bins'] - min(c['bpo'], c['n_bins']) * (n_oct - 1))
    return n_oct, lowest


@pytest.mark.parametrize('name', NAMES)
def test_exact_evaluation_is_the_oracle(name):
    case = BY_NAME[name]
    y, ref = _reference(name)
    got = R.ref_mag(case['cfg'], y, 'exact')
    assert got.shape == ref.shape
    err = R.lin_metric(got, ref)
    print(f'CQTREF {name} exact {err:.1e}')
    assert err < R.EXACT_TOL


@pytest.mark.parametrize('name', NAMES)
def test_ideal_evaluation_meets_half_of_every_bound(name):
    case = BY_NAME[name]
    y, ref = _reference(name)
    got = R.ref_mag(case['cfg'], y, 'ideal')
    lin, db = R.lin_metric(got, ref), R.db_metric(R.to_db(got), R.to_db(ref))
    bound = R.TOL_DB_TONAL if case['input'] == 'tonal' else R.TOL_DB_BROADBAND
    print(f'CQTREF {name} ideal lin {lin:.1e} db {db:.1e}')
    assert lin <= R.TOL_LIN / 2 and db <= bound / 2, (lin, db)


@pytest.mark.parametrize('name', NAMES)
def test_every_mutation_misses_the_linear_bound_tenfold(name):
    case = BY_NAME[name]
    c = case['cfg']
    y, ref = _reference(name)
    n_oct, lowest = _layout(c)
    T = ref.shape[-1]
    edge = sorted({0, 1, T - 2, T - 1} & set(range(T)))
    floor = R.MUTATION_FACTOR * R.TOL_LIN
    rows = []
    for m in ('weights_one_plane', 'signal_one_plane', 'drop_kstep'):
        rows.append((m, R.lin_metric(R.ref_mag(c, y, 'ideal', m), ref)))
    if n_oct >= 3:                                   # the lowest octave lies behind two decimations or more
        rows.append(('taps_one_plane', R.lin_metric(R.ref_mag(c, y, 'ideal', 'taps_one_plane'), ref, rows=lowest)))
    if c['lv'] == '0.9':
        rows.append(('pad_shift', R.lin_metric(R.ref_mag(c, y, 'ideal', 'pad_shift'), ref, frames=edge)))
        if n_oct >= 2:
            rows.append(('decim_reads_pad', R.lin_metric(R.ref_mag(c, y, 'ideal', 'decim_reads_pad'), ref, frames=edge)))
    print(f'CQTREF {name} ' + ' '.join(f'{k} {v:.1e}' for k, v in rows))
    for k, v in rows:
        assert v >= floor, (k, v, floor)


def test_two_plane_decimator_input_is_recorded_not_asserted():
    """The historical 1.07e-3 failure of the 8-octave CQT (a decimator whose input had two bf16 planes): emulated, it moves the linear
    metric no further from the oracle than the ideal evaluation already is -- nothing here could separate it.  Printed, never asserted."""
    case = BY_NAME['reflect-cqt192-shortest']
    y, ref = _reference(case['name'])
    a = R.lin_metric(R.ref_mag(case['cfg'], y, 'ideal'), ref)
    b = R.lin_metric(R.ref_mag(case['cfg'], y, 'ideal', 'decim_two_plane_input'), ref)
    print(f'CQTREF two-plane decimator input: ideal {a:.1e}, with it {b:.1e}')


def test_case_table_reaches_what_it_claims():
    """Routes, level layouts and sizes stated in cqt_ref's table, confirmed from the plan layout."""
    for case in CASES:
        if case['route'] is not None:
            assert R.expected_route(case['cfg'], case['n']) == case['route'], case['name']
    routes = {c['route'] for c in CASES}
    assert routes >= {'windowed128', 'windowed256', 'gemm:n_fft', 'gemm:hop', 'gemm:short'}
    plans = {name: c for name, c, _, _, _ in R.PLANS}
    lay = {name: R.plan_layout(c) for name, c in plans.items()}
    nfft = lambda name: [L['n_fft'] for _, L in sorted(lay[name][0].items())]                # noqa: E731
    assert nfft('k128') == [128] * 7 and nfft('single') == [256] and nfft('single-early') == [256] and lay['single-early'][1] == 2
    assert lay['single'][1] == 1 and nfft('partial-78') == [512] * 6 + [256] and lay['partial-78'][0][6]['ncols'] == 12
    assert nfft('partial-30-hop256') == [512, 512, 256] and nfft('sr16k') == [512] * 6 and nfft('bpo36') == [1024] * 3 and nfft('bpo48') == [1024] * 2
    assert [L['hop'] for _, L in sorted(lay['sr44k'][0].items())] == [512, 256, 128, 64, 32, 16, 8, 4]
    assert [L['hop'] for _, L in sorted(lay['hop384'][0].items())] == [192, 96, 48, 24, 12] and lay['hop1024'][0][0]['hop'] == 1024
    assert min(L['hop'] for L in lay['hop64'][0].values()) == 4 and min(L['hop'] for L in lay['hop128'][0].values()) == 4
    assert nfft('vqt-gamma5')[-1] == 64 and nfft('hvqt-123')[-2:] == [64, 32]
    assert max(L['ncols'] for L in lay['hcqt-8'][0].values()) == 168 and max(L['banks'] for L in lay['hcqt-8'][0].values()) == 7
    assert max(L['ncols'] for L in lay['hcqt-12'][0].values()) == 216 and max(L['banks'] for L in lay['hcqt-12'][0].values()) == 9
    # librosa 0.9: alpha = r - 1 shortens the filters; 78 / 12 is n_fft 256 throughout there
    assert {L['n_fft'] for L in R.plan_layout(dict(plans['partial-78'], lv='0.9'))[0].values()} == {256}
    # the reflecting pad's shortest clips: last level = pad + 1
    assert R.min_reflect_samples(R.cfg(84, 12, lv='0.9')) == 8193 and R.min_reflect_samples(R.cfg(192, 24, lv='0.9')) == 16385
    for case in CASES:
        if case['cfg']['lv'] == '0.9':
            assert case['n'] >= R.min_reflect_samples(case['cfg']), case['name']
    # CQT 84 / 12: seven levels, the deepest 3 samples long at n = 192 and 4 at 193
    assert R.level_lengths(192, 7)[-1] == 3 and R.level_lengths(193, 7)[-1] == 4 and R.level_lengths(300, 7)[-1] == 5
    # frames: one at 511, two at 512; the 16-bit tests' T = 1 and T = 33
    assert cq.vqt_expected_frames(511, 22050, 512, cq.C1_HZ, 84, 12, 0.0) == 1 and cq.vqt_expected_frames(512, 22050, 512, cq.C1_HZ, 84, 12, 0.0) == 2
    assert cq.vqt_expected_frames(300, 22050, 512, 0.5 * cq.C1_HZ, 72, 12, 0.0) == 1 and cq.vqt_expected_frames(16500, 22050, 512, 0.5 * cq.C1_HZ, 72, 12, 0.0) == 33


def test_rounding_helpers():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, -3.1415927, 1e-30, 0.0], dtype=np.float32)
    assert R.bf16(x).tolist()[:3] == [1.0, 1.0, 1.0 + 2.0 ** -6]                   # ties to even
    hi, lo = R.two_planes(x)
    assert np.all(np.abs(hi + lo - x.astype(np.float64)) <= 2.0 ** -16 * np.abs(x))
    assert np.array_equal(R.bf16(hi), hi) and np.array_equal(R.bf16(lo), lo)
