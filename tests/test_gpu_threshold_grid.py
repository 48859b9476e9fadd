"""The two threshold-grid kernels (include/amtx_thrgrid.h, csrc/thrgrid.hip) against the kernels they restate, on rolls that
amtx_pianoroll_fwd cut at each threshold from the same logits: amtx_eval_multipitch_grid_counts against amtx_eval_multipitch_counts,
amtx_notes_decode_grid against amtx_notes_decode's `pairs` and `counts`.  Integers and bit patterns, no tolerance; outputs poisoned
(tests/poison.py) and zero-filled give the same results."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from amt_tools_amd import _lib, evaluate as ev, transcribe           # noqa: E402
from poison import PATTERNS, fill_storage                            # noqa: E402

DEV = 'cuda:0'
FRAMES, KEYS, BATCHES = (1, 63, 64, 65, 130), (3, 88), (1, 3)
GRID32 = np.concatenate([[0.0, 0.5, 1.0, 1.5], np.linspace(0.03, 0.97, 28)]).astype(np.float32)
# {onset, frame} pairs: the default, everything active, a high pair, above 1 (NaN alone), the default AGAIN, two mixed ones -- 7 pairs
PAIRS = np.array([[0.5, 0.5], [0.0, 0.0], [0.9, 0.9], [1.5, 1.5], [0.5, 0.5], [1.0, 0.25], [0.25, 1.0]], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _logits(B, T, K, seed):
    """(B, T, K) logits: a fifth exactly 0 (probability 0.5, ON the default threshold), +inf and -inf (probabilities 1 and 0, on the
    thresholds 1 and 0), one NaN; the first three cells are 3, 0 and NaN so that even 3 cells tell the pairs apart."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, T, K)) * 2.5).astype(np.float32)
    x[rng.random(x.shape) < 0.2] = 0.0
    x[rng.random(x.shape) < 0.03] = np.inf
    x[rng.random(x.shape) < 0.03] = -np.inf
    x.reshape(-1)[:3] = (3.0, 0.0, np.nan)
    if x.size >= 6:
        x.reshape(-1)[3:6] = (np.inf, -np.inf, 0.0)
    return torch.from_numpy(x).to(DEV)


def _roll(logits, thr, out=None):
    """amtx_pianoroll_fwd: (B, T, K) logits -> (B, K, T); thr < 0: probabilities."""
    B, T, K = logits.shape
    out = torch.empty((B, K, T), dtype=torch.float32, device=DEV) if out is None else out
    _lib.call('amtx_pianoroll_fwd', logits, K, 0, B, T, K, float(thr), out, device=DEV)
    return out


def _off_grid(t, phase):
    """A copy of `t` that starts `phase` floats behind a 256-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=DEV)
    view = buf[phase:phase + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * phase % 16
    return view


def _filled(shape, dtype, pattern):
    return fill_storage(torch.empty(shape, dtype=dtype, device=DEV), pattern)


# ------------------------------------------------------------------------------------------------------------------------------
# amtx_eval_multipitch_grid_counts
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('K', KEYS)
@pytest.mark.parametrize('T', FRAMES)
def test_grid_counts_equal_the_counts_of_every_thresholded_roll(T, K, B):
    logits = _logits(B, T, K, 7)
    prob = _roll(logits, -1.0)
    assert torch.isnan(prob).sum().item() == 1 and (B * T * K < 6 or ((prob == 0.5).any() and (prob == 1).any() and (prob == 0).any()))
    ref = (torch.rand((B, K, T), generator=torch.Generator().manual_seed(T + K + B)) < 0.4).float().to(DEV)
    want = torch.empty((B, 32, 3), dtype=torch.int64, device=DEV)
    one = torch.empty((B, 1, 3), dtype=torch.int64, device=DEV)
    for g, thr in enumerate(GRID32.tolist()):
        _lib.call('amtx_eval_multipitch_counts', _roll(logits, thr), ref, B, 1, K, T, one, device=DEV)
        want[:, g] = one[:, 0]
    want = want.cpu().numpy()
    assert (want[:, 0, 1] == K * T).all() and want[0, 3, 1] == 1                   # threshold 0: every cell; 1.5: the NaN alone
    # maps on the 16-byte grid, both one float off it (vector body behind a scalar head), and at different phases (scalar loop)
    for p_prob, p_ref in ((0, 0), (1, 1), (3, 2)):
        a, b = _off_grid(prob, p_prob), _off_grid(ref, p_ref)
        for G, thr in ((1, GRID32[1:2]), (32, GRID32)):
            thr_d = torch.from_numpy(np.ascontiguousarray(thr)).to(DEV)
            runs = []
            for pattern in (0x00,) + PATTERNS[1:]:
                counts = _filled((B, G, 3), torch.int64, pattern)
                _lib.call('amtx_eval_multipitch_grid_counts', a, b, B, K, T, thr_d, G, counts, device=DEV)
                runs.append(counts.cpu().numpy())
            assert np.array_equal(runs[0], want[:, 1:2] if G == 1 else want), (T, K, B, G, p_prob, p_ref)
            assert all(np.array_equal(r, runs[0]) for r in runs[1:]), 'stale output memory reached a count'
    # the Python primitive: one call, a device tensor
    got = ev.multipitch_grid_counts(prob, ref, GRID32)
    assert got.is_cuda and got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)


def test_grid_counts_refusals():
    prob = torch.zeros((1, 3, 8), device=DEV)
    thr = torch.zeros(33, device=DEV)
    counts = _filled((1, 33, 3), torch.int64, 0x7F)
    for G in (0, 33, -1):
        with pytest.raises(_lib.AmtxError, match='thresholds'):
            _lib.call('amtx_eval_multipitch_grid_counts', prob, prob, 1, 3, 8, thr, G, counts, device=DEV)
    with pytest.raises(_lib.AmtxError, match='null pointer'):
        _lib.call('amtx_eval_multipitch_grid_counts', prob, prob, 1, 3, 8, None, 1, counts, device=DEV)
    with pytest.raises(_lib.AmtxError, match='bad sizes'):
        _lib.call('amtx_eval_multipitch_grid_counts', prob, prob, 1, 0, 8, thr, 1, counts, device=DEV)
    torch.cuda.synchronize()
    assert (counts.view(torch.uint8).cpu().numpy() == 0x7F).all()


# ------------------------------------------------------------------------------------------------------------------------------
# amtx_notes_decode_grid
# ------------------------------------------------------------------------------------------------------------------------------
def _decode_reference(on_logits, mp_logits, pairs, cap):
    """amtx_notes_decode on the rolls of every pair: [(events (B * K, cap, 2), counts (B * K,))] on the host."""
    B, T, K = mp_logits.shape
    out = []
    for on_thr, mp_thr in pairs.tolist():
        events = torch.zeros((B * K, cap, 2), dtype=torch.int32, device=DEV)
        counts = torch.empty((B * K,), dtype=torch.int32, device=DEV)
        _lib.call('amtx_notes_decode', None if on_logits is None else _roll(on_logits, on_thr), _roll(mp_logits, mp_thr), B, K, T, cap, events, counts, device=DEV)
        out.append((events.cpu().numpy(), counts.cpu().numpy()))
    return out


def _decode_grid_checked(on_prob, mp_prob, pairs, cap, want, what):
    """The grid decoder into poisoned and zero-filled outputs: counts equal, the first min(count, cap) events of every row equal in
    order, and nothing else of the event buffer touched."""
    B, K, T = mp_prob.shape
    P = len(pairs)
    pairs_d = torch.from_numpy(pairs).to(DEV)
    for pattern in (0x00,) + PATTERNS[1:]:
        events = _filled((P * B * K, cap, 2), torch.int32, pattern)
        counts = _filled((P * B * K,), torch.int32, pattern)
        _lib.call('amtx_notes_decode_grid', on_prob, mp_prob, B, K, T, pairs_d, P, cap, events, counts, device=DEV)
        events, counts = events.cpu().numpy(), counts.cpu().numpy()
        fill = np.frombuffer(bytes([pattern]) * 4, dtype=np.int32)[0]
        for p in range(P):
            want_events, want_counts = want[p]
            rows = slice(p * B * K, (p + 1) * B * K)
            assert np.array_equal(counts[rows], want_counts), (what, p, hex(pattern))
            stored = np.arange(cap)[None, :] < np.minimum(want_counts, cap)[:, None]
            assert np.array_equal(events[rows][stored], want_events[stored]), (what, p, hex(pattern))
            assert (events[rows][~stored] == fill).all(), (what, p, hex(pattern), 'an event slot behind a row\'s count was written')


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('K', KEYS)
@pytest.mark.parametrize('T', FRAMES)
def test_grid_decode_equals_the_decoder_on_every_pair_of_rolls(T, K, B):
    on_logits, mp_logits = _logits(B, T, K, 11), _logits(B, T, K, 12)
    cap = T // 2 + 2
    want = _decode_reference(on_logits, mp_logits, PAIRS, cap)
    totals = [int(c.sum()) for _, c in want]
    assert len(set(totals)) >= 3 and totals[0] == totals[4], totals                # the pairs tell the maps apart; the repeated pair repeats
    assert max(int(c.max()) for _, c in want) <= cap                               # no pair overflows here
    _decode_grid_checked(_roll(on_logits, -1.0), _roll(mp_logits, -1.0), PAIRS, cap, want, (T, K, B))


@pytest.mark.parametrize('T,K,B', [(130, 88, 3), (65, 3, 1)])
def test_grid_decode_without_onsets_derives_them_from_the_frame_roll(T, K, B):
    mp_logits = _logits(B, T, K, 12)
    cap = T // 2 + 2
    want = _decode_reference(None, mp_logits, PAIRS, cap)
    assert len({int(c.sum()) for _, c in want}) >= 3
    # a pair's first entry is not read: NaN there changes nothing
    pairs = PAIRS.copy()
    pairs[:, 0] = np.nan
    _decode_grid_checked(None, _roll(mp_logits, -1.0), pairs, cap, want, (T, K, B, 'no onsets'))


def test_grid_decode_overflows_like_the_decoder_and_takes_views_off_the_16_byte_grid():
    B, T, K, cap = 3, 130, 88, 2
    on_logits, mp_logits = _logits(B, T, K, 11), _logits(B, T, K, 12)
    want = _decode_reference(on_logits, mp_logits, PAIRS, cap)
    assert max(int(c.max()) for _, c in want) > cap                                # rows with more events than slots
    on_prob, mp_prob = _roll(on_logits, -1.0), _roll(mp_logits, -1.0)
    _decode_grid_checked(on_prob, mp_prob, PAIRS, cap, want, 'overflow')
    _decode_grid_checked(_off_grid(on_prob, 1), _off_grid(mp_prob, 3), PAIRS, cap, want, 'off the 16-byte grid')
    # one pair, and as many pairs as two tiles and a half
    _decode_grid_checked(on_prob, mp_prob, PAIRS[2:3], cap, want[2:3], 'one pair')
    many = np.concatenate([PAIRS, PAIRS[::-1], PAIRS[:6]])
    _decode_grid_checked(on_prob, mp_prob, many, cap, want + want[::-1] + want[:6], 'twenty pairs')


def test_grid_decode_refusals():
    prob = torch.zeros((1, 3, 8), device=DEV)
    pairs = torch.zeros((2, 2), device=DEV)
    events, counts = _filled((6, 6, 2), torch.int32, 0x7F), _filled((6,), torch.int32, 0x7F)
    for args, text in (((prob, None, 1, 3, 8, pairs, 2, 6, events, counts), 'null pointer'), ((prob, prob, 1, 3, 8, None, 2, 6, events, counts), 'null pointer'),
                       ((prob, prob, 1, 3, 8, pairs, 0, 6, events, counts), 'bad sizes'), ((prob, prob, 1, 3, 8, pairs, 2, 0, events, counts), 'bad sizes'),
                       ((prob, prob, 1 << 20, 88, 8, pairs, 32, 6, events, counts), 'too many')):
        with pytest.raises(_lib.AmtxError, match=text):
            _lib.call('amtx_notes_decode_grid', *args, device=DEV)
    torch.cuda.synchronize()
    assert (events.view(torch.uint8).cpu().numpy() == 0x7F).all() and (counts.view(torch.uint8).cpu().numpy() == 0x7F).all()


# ------------------------------------------------------------------------------------------------------------------------------
# the Python primitive
# ------------------------------------------------------------------------------------------------------------------------------
def test_decode_notes_grid_equals_decode_notes_batch_per_pair_in_one_chunk_and_in_several():
    B, T, K = 3, 130, 88
    on_logits, mp_logits = _logits(B, T, K, 11), _logits(B, T, K, 12)
    on_prob, mp_prob = _roll(on_logits, -1.0), _roll(mp_logits, -1.0)
    times = np.arange(T) * 512 / 22050
    want = []
    for on_thr, mp_thr in PAIRS.tolist():
        want += transcribe.decode_notes_batch(_roll(on_logits, on_thr), _roll(mp_logits, mp_thr), times, 21)
    assert len({len(w) for w in want}) >= 3
    one = transcribe.decode_notes_grid_async(on_prob, mp_prob, times, PAIRS, 21)
    assert len(one.chunks) == 1
    # a budget of three pairs' events: chunks of 3, 3 and 1 pairs; a first buffer of 16 rows: every chunk decodes again
    several = transcribe.decode_notes_grid_async(on_prob, mp_prob, times, torch.from_numpy(PAIRS).to(DEV), 21, rows_capacity=16,
                                                 event_bytes=3 * B * K * (T // 2 + 2) * 8)
    assert [(p0, n) for p0, n, _ in several.chunks] == [(0, 3), (3, 3), (6, 1)]
    rows, offsets = several.device_rows()
    assert offsets.shape == (len(PAIRS) * B + 1,) and int(offsets[-1]) == rows.shape[0] == sum(len(w) for w in want)
    for got in (one.result(), several.result()):
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    # the host path on the same probabilities gives the same notes
    host = transcribe.decode_notes_grid(on_prob.cpu(), mp_prob.cpu(), times, PAIRS, 21)
    assert all(np.array_equal(a, b) for a, b in zip(host, want))
    with pytest.raises(ValueError, match='one .* time grid'):
        transcribe.decode_notes_grid_async(on_prob, mp_prob, np.tile(times, (B, 1)), PAIRS, 21)
