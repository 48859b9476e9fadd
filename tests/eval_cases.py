"""Note-matching cases shared by tests/test_evaluate_host.py and tests/test_gpu_evaluate.py, and the brute force both compare against: the
edge matrix by the rules the evaluators state (float64, distances rounded to N_DECIMALS, non-strict comparisons), written out here on its
own, and scipy's maximum bipartite matching for the cardinality.  Rows are [onset_s, offset_s, midi_pitch]."""
import functools

import numpy as np

D = 4                     # evaluate.N_DECIMALS, restated
UNIT = 10.0 ** -D         # one rounding unit
ONSET_TOL, OFFSET_MIN_TOL = 0.05, 0.05
RATIOS = (None, 0.2)


def brute_edges(est, ref, offset_ratio):
    """(num_ref, num_est) edges, integral pitches (50 cents = equal pitch)."""
    est, ref = np.asarray(est, dtype=np.float64).reshape(-1, 3), np.asarray(ref, dtype=np.float64).reshape(-1, 3)
    edges = np.zeros((len(ref), len(est)), dtype=bool)
    for i, (ron, roff, rp) in enumerate(ref):
        for j, (eon, eoff, ep) in enumerate(est):
            ok = rp == ep and np.around(abs(ron - eon), D) <= ONSET_TOL
            if ok and offset_ratio is not None:
                ok = np.around(abs(roff - eoff), D) <= max(OFFSET_MIN_TOL, offset_ratio * (roff - ron))
            edges[i, j] = ok
    return edges


def brute_matched(est, ref, offset_ratio):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    edges = brute_edges(est, ref, offset_ratio)
    if edges.size == 0:
        return 0
    return int((maximum_bipartite_matching(csr_matrix(edges), perm_type='column') >= 0).sum())


def greedy_matched(est, ref, offset_ratio):
    """Earliest-first greedy: estimated notes in onset order, each takes the earliest free reference note it may be matched with."""
    est, ref = np.asarray(est, dtype=np.float64).reshape(-1, 3), np.asarray(ref, dtype=np.float64).reshape(-1, 3)
    edges = brute_edges(est, ref, offset_ratio)
    taken, n = set(), 0
    for j in np.argsort(est[:, 0], kind='stable'):
        for i in np.argsort(ref[:, 0], kind='stable'):
            if edges[i, j] and i not in taken:
                taken.add(int(i))
                n += 1
                break
    return n


def _rows(*notes):
    return np.array(notes, dtype=np.float64).reshape(-1, 3)


def random_notes(seed, n, pitches=(60, 61, 62, 64), span=2.0):
    """n notes on a few pitches, onsets on a 10 ms grid plus jitter around the tolerances, so that several candidates compete."""
    rng = np.random.default_rng(seed)
    on = np.round(rng.uniform(0, span, n), 2) + rng.choice([0.0, UNIT, -UNIT, 0.4 * UNIT, 0.03], n)
    dur = rng.choice([0.05, 0.1, 0.25, 0.5, 1.0], n) + rng.choice([0.0, 0.02, 0.05], n)
    return np.stack([on, on + dur, rng.choice(np.array(pitches, dtype=np.float64), n)], axis=-1)


# Under the offset rule the candidates of a note are no contiguous run: earliest-first greedy is not maximum.
# A: E0 may take R0 or R1, E1 only R0; greedy gives R0 to E0.
GREEDY_A = (_rows((1.01, 1.95, 60), (1.03, 2.15, 60)), _rows((1.00, 2.00, 60), (1.02, 1.90, 60)))
# B: three short reference notes (offset tolerance 0.05 s each); E0 {R0, R1}, E1 {R1, R2}, E2 {R1}: greedy leaves E2 without a partner
GREEDY_B = (_rows((1.000, 1.23, 72), (1.005, 1.30, 72), (1.010, 1.26, 72)), _rows((1.00, 1.20, 72), (1.01, 1.26, 72), (1.02, 1.34, 72)))


def tolerance_edge_cases():
    """One estimated and one reference note per pitch: the onset (pitches 40 ..) and the offset distance (pitches 60 .., 80 ..) exactly at
    the tolerance, one rounding unit and a fraction of a unit either side of it."""
    deltas = [0.0, UNIT, -UNIT, 0.4 * UNIT, 0.6 * UNIT, -0.4 * UNIT, -0.6 * UNIT]
    est, ref = [], []
    for k, d in enumerate(deltas):
        ref.append((1.0, 2.0, 40 + k))
        est.append((1.0 + ONSET_TOL + d, 2.0, 40 + k))                       # late onset
        ref.append((3.0, 4.0, 50 + k))
        est.append((3.0 - ONSET_TOL - d, 4.0, 50 + k))                       # early onset
        ref.append((5.0, 6.0, 60 + k))                                       # duration 1 s: offset tolerance 0.2 s
        est.append((5.0, 6.0 + 0.2 + d, 60 + k))
        ref.append((7.0, 7.1, 80 + k))                                       # duration 0.1 s: the minimum tolerance, 0.05 s
        est.append((7.0, 7.1 - OFFSET_MIN_TOL - d, 80 + k))
    return _rows(*est), _rows(*ref)


def long_list(seed=5, n=90):
    """One pitch, n notes a millisecond apart on both sides: every window holds more than 64 and at most n candidates."""
    rng = np.random.default_rng(seed)
    on = 1.0 + np.arange(n) * 0.001
    est = np.stack([on + rng.choice([0.0, 0.0004], n), on + rng.choice([0.2, 0.3, 0.45], n), np.full(n, 69.0)], axis=-1)
    ref = np.stack([on, on + rng.choice([0.2, 0.3, 0.45], n), np.full(n, 69.0)], axis=-1)
    return est, ref


def beyond_the_bound(n=140):
    """n reference notes of one pitch inside the onset window of one estimated note (the kernel's bound is 128)."""
    ref = np.stack([1.0 + np.arange(n) * 0.0005, np.full(n, 2.0), np.full(n, 69.0)], axis=-1)
    return _rows((1.03, 2.0, 69), (1.031, 2.0, 69)), ref


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (est rows, ref rows)."""
    out = {'empty_est': (np.zeros((0, 3)), random_notes(1, 7)), 'empty_ref': (random_notes(2, 7), np.zeros((0, 3))),
           'both_empty': (np.zeros((0, 3)), np.zeros((0, 3))), 'greedy_a': GREEDY_A, 'greedy_b': GREEDY_B, 'tolerance_edges': tolerance_edge_cases(),
           'long_list': long_list()}
    for seed, (ne, nr) in enumerate([(5, 5), (12, 9), (30, 30), (40, 25), (1, 20), (64, 64)]):
        out[f'random_{seed}'] = (random_notes(100 + seed, ne), random_notes(200 + seed, nr))
    # an estimate that is the reference with jitter: dense matchings
    ref = random_notes(300, 50, pitches=(60, 61))
    est = ref + np.random.default_rng(301).choice([0.0, 0.02, -0.03, 0.0499, 0.06], size=(50, 1)) * np.array([1.0, 1.0, 0.0])
    out['jittered'] = (est, ref)
    return out


@functools.lru_cache(maxsize=None)
def expected(name, offset_ratio):
    est, ref = cases()[name]
    return brute_matched(est, ref, offset_ratio)
