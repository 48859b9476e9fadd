"""Whole tracks from overlapped clips, the host side (amt_tools_amd/tracks.py: seam_clips, stitch_host, TrackMaps' bookkeeping,
NoteBank.host_whole) and the argument checks of the drivers that run before the library is entered.  No GPU here."""
import numpy as np
import pytest

from amt_tools_amd import _lib, evaluate as ev, inference, tools, tracks
from amt_tools_amd.tracks import NoteBank, TrackMaps, _note_order, seam_clips, stitch_host


def _seams(plan, track, length):
    """The seams of one track of a plan: the first kept frame of each of its clips, then the track's length."""
    return plan.kept[plan.track_ids == track, 0].tolist() + [length]


def test_every_frame_is_kept_exactly_once_at_least_margin_frames_from_a_clip_edge_that_is_no_track_edge():
    """Exhaustive: every num_frames < 40, every valid margin, every track length up to 4 * num_frames + 6."""
    plans = 0
    for num_frames in range(1, 40):
        for margin in range(0, (num_frames - 1) // 2 + 1):
            assert num_frames - 2 * margin >= 1
            lengths = np.arange(1, 4 * num_frames + 7)
            plan = seam_clips(lengths, num_frames, margin)
            assert plan.short.tolist() == list(range(num_frames - 1))                       # the tracks of 1 .. num_frames - 1 frames
            assert plan.kept.shape == (len(plan.track_ids), 3) and plan.first_frames.shape == plan.track_ids.shape
            assert (np.diff(plan.track_ids) >= 0).all()                                     # track order
            for t in range(num_frames - 1, len(lengths)):
                L = int(lengths[t])
                sel = slice(*np.searchsorted(plan.track_ids, [t, t + 1]))
                first, (dst, src, count) = plan.first_frames[sel], plan.kept[sel].T
                assert len(first) >= 1 and len(set(first.tolist())) == len(first)           # distinct clips
                assert (first >= 0).all() and (first + num_frames <= L).all()               # inside the track
                assert (count >= 1).all() and dst[0] == 0 and (dst[1:] == dst[:-1] + count[:-1]).all() and dst[-1] + count[-1] == L   # exactly once
                assert (dst - first == src).all() and (src >= 0).all() and (src + count <= num_frames).all()   # inside the clip
                left_is_track_edge, right_is_track_edge = first == 0, first + num_frames == L
                assert (left_is_track_edge | (src >= margin)).all()
                assert (right_is_track_edge | (num_frames - (src + count) >= margin)).all()
                assert (~left_is_track_edge | (src == 0)).sum() == len(first) and first[-1] + num_frames == L
                plans += 1
    assert plans > 30000


def test_literal_plans():
    plan = seam_clips([118, 59, 40, 23], 40, 6)
    assert plan.track_ids.tolist() == [0, 0, 0, 0, 1, 1, 2] and plan.first_frames.tolist() == [0, 28, 56, 78, 0, 19, 0]
    assert plan.short.tolist() == [3]
    assert _seams(plan, 0, 118) == [0, 34, 62, 87, 118] and _seams(plan, 1, 59) == [0, 29, 59] and _seams(plan, 2, 40) == [0, 40]
    assert plan.kept.tolist() == [[0, 0, 34], [34, 6, 28], [62, 6, 25], [87, 9, 31], [0, 0, 29], [29, 10, 30], [0, 0, 40]]
    assert all(a.dtype == np.int64 for a in plan)
    long = seam_clips([10000], 625, 64)
    assert len(long.track_ids) == 20 and long.first_frames[-1] == 9375 and long.kept[-1].tolist() == [9473, 98, 527]
    assert long.first_frames[:-1].tolist() == [497 * k for k in range(19)]
    # the order of the request, a track named twice, nothing but short tracks
    plan = seam_clips([118, 59, 40, 23], 40, 6, track_ids=[2, 3, 1, 2])
    assert plan.track_ids.tolist() == [2, 1, 1, 2] and plan.first_frames.tolist() == [0, 0, 19, 0] and plan.short.tolist() == [3]
    plan = seam_clips([5, 7], 40, 0)
    assert plan.track_ids.size == 0 and plan.kept.shape == (0, 3) and plan.short.tolist() == [0, 1]


def test_seam_clips_refuses():
    with pytest.raises(ValueError, match='margin=-1'):
        seam_clips([100], 40, -1)
    with pytest.raises(ValueError, match='num_frames=40 with margin=20'):
        seam_clips([100], 40, 20)
    with pytest.raises(ValueError, match='num_frames=0'):
        seam_clips([100], 0, 0)
    for bad in (1, -1):
        with pytest.raises(ValueError, match=f'unknown track {bad}: the bank holds 1 tracks'):
            seam_clips([100], 40, 6, track_ids=[0, bad])
    assert seam_clips([100], 40, 19).first_frames.tolist() == list(range(0, 60, 2)) + [60]      # stride 2 is fine


def _maps_and_tables(rows):
    """TrackMaps' bookkeeping for the 118- and the 59-frame track without a device: base, and the tables of the two tracks' clips."""
    torch = pytest.importorskip('torch')
    plan = seam_clips([118, 59], 40, 6)
    maps = TrackMaps([118, 59], 'cpu')
    maps.add('k', (rows,), torch.float32)
    assert maps.base['k'].tolist() == [0, 118 * rows] and maps.nbytes == 177 * rows * 4 and maps.track(1, 'k').shape == (1, rows, 59)
    return plan, maps, maps.descriptors('k', plan.track_ids, plan.kept)


def test_stitch_host_equals_plain_slicing_on_bit_patterns():
    rng = np.random.default_rng(3)
    rows = 5
    plan, _, desc = _maps_and_tables(rows)
    assert desc[:, 0].tolist() == [0] * 4 + [118 * rows] * 2 and desc[:, 1].tolist() == [118] * 4 + [59] * 2
    assert desc[:, 2:].tolist() == plan.kept.tolist()
    # float32 with NaN payloads and -0.0, compared as uint32
    bits = rng.integers(0, 2 ** 32, size=(6, rows, 40), dtype=np.uint64).astype(np.uint32)
    bits[0, 0, :4] = (0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000)                        # quiet / signalling NaNs with payloads, -0.0
    bits[5, 4, -1] = 0x80000000
    src = bits.view(np.float32)
    dst = np.full(177 * rows, np.float32(7.0))
    assert stitch_host(dst, src, desc) is dst
    want = [np.concatenate([bits[b, :, s:s + c] for b, (_, s, c) in enumerate(plan.kept) if plan.track_ids[b] == t], axis=1) for t in (0, 1)]
    assert np.array_equal(dst[:118 * rows].view(np.uint32).reshape(rows, 118), want[0])
    assert np.array_equal(dst[118 * rows:].view(np.uint32).reshape(rows, 59), want[1])
    assert (dst.view(np.uint32) == 0x7FC00001).sum() >= 1 and (dst.view(np.uint32) == 0x80000000).sum() >= 1
    # int64 with -1, a shape with two middle axes
    tab = rng.integers(-1, 20, size=(6, rows, 1, 40))
    tab[1, :, :, 6] = -1
    out = np.full(177 * rows, 99, dtype=np.int64)
    stitch_host(out, tab, desc)
    for t, (lo, L) in enumerate(((0, 118), (118 * rows, 59))):
        got = out[lo:lo + rows * L].reshape(rows, L)
        for b in np.flatnonzero(plan.track_ids == t):
            d, s, c = plan.kept[b]
            assert np.array_equal(got[:, d:d + c], tab[b, :, 0, s:s + c])
    assert (out != 99).all() and (out == -1).any()
    # one clip's share alone writes nothing else
    alone = np.full(177 * rows, 99, dtype=np.int64)
    stitch_host(alone, tab[2:3], desc[2:3])
    assert (alone != 99).sum() == rows * 25 and np.array_equal(alone[:118 * rows].reshape(rows, 118)[:, 62:87], tab[2, :, 0, 6:31])


def test_stitch_host_refuses_what_the_entry_point_refuses():
    src, dst = np.zeros((1, 2, 10), dtype=np.float32), np.zeros(60, dtype=np.float32)
    stitch_host(dst, src, [[0, 30, 20, 0, 10]])
    for row in ([0, 30, 21, 0, 10], [0, 30, 0, 1, 10], [1, 30, 0, 0, 10], [0, 31, 0, 0, 10], [0, 30, 0, 0, 11], [-1, 30, 0, 0, 1], [0, 30, 0, 0, -1],
                [0, 30, -1, 0, 1], [0, 30, 0, -1, 1]):
        with pytest.raises(ValueError, match='clip 0'):
            stitch_host(dst, src, [row])
    with pytest.raises(ValueError, match=r'\(1, 5\)'):
        stitch_host(dst, src, [[0, 30, 0, 0, 10]] * 2)
    with pytest.raises(TypeError, match='float32'):
        stitch_host(np.zeros(60, dtype=np.int64), src, [[0, 30, 0, 0, 10]])
    with pytest.raises(ValueError, match='flat'):
        stitch_host(np.zeros((2, 30), dtype=np.float32), src, [[0, 30, 0, 0, 10]])


def test_track_maps_bookkeeping_refuses_before_anything_is_allocated():
    with pytest.raises(ValueError, match='at least one track'):
        TrackMaps([], 'cpu')
    with pytest.raises(ValueError, match='at least one frame'):
        TrackMaps([5, 0], 'cpu')
    plan, maps, _ = _maps_and_tables(3)
    with pytest.raises(ValueError, match='one slot below 2'):
        maps.descriptors('k', [0, 2], plan.kept[:2])
    with pytest.raises(ValueError, match='one slot below 2'):
        maps.descriptors('k', [0], plan.kept[:2])
    torch = pytest.importorskip('torch')
    with pytest.raises(ValueError, match="already hold 'k'"):
        maps.add('k', (3,), torch.float32)
    with pytest.raises(TypeError, match='float32 or int64'):
        maps.add('j', (3,), torch.int32)
    with pytest.raises(ValueError, match=r"a batch of \(4,\) maps for maps of \(3,\)"):
        maps.stitch('k', torch.zeros(1, 4, 40), plan.kept[:1])


class _Frames(object):
    """What NoteBank reads of an audio bank."""
    frame_counts = np.array([50, 50, 50])
    device = 'cuda:0'
    module = None

    def __len__(self):
        return 3


def test_host_whole_is_the_constructors_input_in_note_order():
    rng = np.random.default_rng(5)
    given = []
    for n in (9, 0, 4):
        on = rng.integers(0, 40, n) * 0.01
        given.append(np.stack([on, on + rng.integers(0, 5, n) * 0.01, rng.integers(40, 44, n).astype(np.float64)], axis=1))
    given[0][0, :2] = 0.0                                                                   # a note with offset == 0 ...
    bank = NoteBank(given, bank=_Frames())
    groups = bank.host_whole([0, 1, 2])
    assert [g.shape for g in groups] == [(9, 3), (0, 3), (4, 3)]
    for got, want in zip(groups, given):
        assert np.array_equal(got.view(np.uint64), _note_order(want).view(np.uint64))
    # ... which the window route drops, whatever the window
    assert len(bank.host_window_clips([0], [[0.0, 100.0]])[0]) == 8 and (groups[0][:, 1] == 0).sum() == 1
    assert [len(g) for g in bank.host_whole([2, 0])] == [4, 9]
    groups[0][:] = -5                                                                        # a copy: the bank's table is not the caller's
    assert np.array_equal(bank.host_whole([0])[0], _note_order(given[0]))
    for bad in ([3], [-1], []):
        with pytest.raises(ValueError):
            bank.host_whole(bad)
    with pytest.raises(ValueError, match='unknown track 3'):
        bank.whole([0, 3])                                                                   # before any device state is made
    # stacked notes: one group per (track, string), keys in the dictionary's order
    stacked = [{s: (g[s::2, 2], g[s::2, :2]) for s in range(2)} for g in given]
    sbank = NoteBank(stacked)
    groups = sbank.host_whole([2, 0])
    assert len(groups) == 4 and sbank.slices == 2
    for got, (t, s) in zip(groups, ((2, 0), (2, 1), (0, 0), (0, 1))):
        assert np.array_equal(got, _note_order(given[t][s::2]))


class _Bank(object):
    frame_counts = np.array([118, 59, 40, 23])

    def __len__(self):
        return 4


class _CpuModel(object):
    device = 'cpu'


def test_the_drivers_refuse_before_the_library_is_entered(monkeypatch):
    def entered(*args, **kwargs):
        raise AssertionError('the library was entered')
    monkeypatch.setattr(_lib, 'call', entered)
    monkeypatch.setattr(_lib, 'lib', entered)
    bank = _Bank()
    for kwargs, text in ((dict(margin=-1), 'margin=-1'), (dict(margin=20), 'num_frames=40 with margin=20'),
                         (dict(margin=6, track_ids=[0, 4]), 'unknown track 4'), (dict(margin=6), 'the model has to be on a GPU')):
        with pytest.raises(ValueError, match=text):
            inference.run_tracks(bank, _CpuModel(), 40, **kwargs)
    labels = type('L', (), {'keys': [tools.KEY_ONSETS], '__len__': lambda self: 4})()
    batched = type('N', (), {'stacked': False, 'relative_times': False, '__len__': lambda self: 4})()
    cases = ((ev.MultipitchEvaluator(), None, None, 'validate_tracks needs a LabelBank'),
             (ev.MultipitchEvaluator(), labels, None, 'the LabelBank holds'),
             (ev.NoteEvaluator(), None, None, 'validate_tracks needs a NoteBank'),
             (ev.StackedNoteEvaluator(), None, batched, 'scores stacked notes, the NoteBank holds batched notes'),
             (ev.NoteEvaluator(), None, batched, 'validate_tracks scores device-resident tracks: the model has to be on a GPU'),
             (ev.NoteEvaluator(), None, type('N', (), {'stacked': False, '__len__': lambda self: 3})(), 'a bank of 4 tracks and a NoteBank of 3'))
    for evaluator, lab, nts, text in cases:
        with pytest.raises(ValueError, match=text):
            ev.validate_tracks(bank, lab, nts, _CpuModel(), evaluator, 40, 6)
    # the device wrapper: arrays, CPU tensors and other dtypes never reach the entry point
    torch = pytest.importorskip('torch')
    with pytest.raises(TypeError, match='device tensors'):
        tracks.stitch_clips(np.zeros(10, dtype=np.float32), np.zeros((1, 1, 10), dtype=np.float32), [[0, 10, 0, 0, 10]])
    with pytest.raises(ValueError, match='on one GPU'):
        tracks.stitch_clips(torch.zeros(10), torch.zeros(1, 1, 10), [[0, 10, 0, 0, 10]])
