"""The note ground truth of clips cut from resident tracks, off the GPU: tracks.NoteBank's host restatement of the reference's
slice_batched_notes against what the reference itself returned (tests/golden/note_clips.npz, tools/gen_golden_note_clips.py), the clips'
time windows against the reference's arithmetic, the boundary rules, cover_clips, and every refusal's text.  All comparisons are equality,
floating values on their uint64 view."""
import os
import pickle

import numpy as np
import pytest

from amt_tools_amd import evaluate as ev, tools
from amt_tools_amd.features import CQT, MelSpec
from amt_tools_amd.tracks import LabelBank, NoteBank, PyramidBank, TrackBank, clip_windows, cover_clips

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'note_clips.npz'))
HOP, SR = int(GOLDEN['hop_length']), int(GOLDEN['sample_rate'])


def bits(rows):
    """The uint64 view of note rows in _sort_rows order.  Rows of one pitch and onset are first put in offset order: _sort_rows is stable and
    leaves such ties as it finds them, and the bank has sorted once already where the reference has not."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    return np.ascontiguousarray(ev._sort_rows(rows[np.argsort(rows[:, 1], kind='stable')])).view(np.uint64)


def assert_same_rows(got, want, what):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), what


@pytest.mark.parametrize('relative', [False, True])
def test_host_clips_equal_what_the_reference_returned_for_batched_notes(relative):
    tracks = [GOLDEN[f'notes_T{i}'] for i in range(3)]
    assert [len(t) for t in tracks] == GOLDEN['sizes'].tolist() == [300, 65, 0]
    bank = NoteBank(tracks, relative_times=relative)
    assert bank.slices == 1 and bank.keys is None and not bank.stacked and bank.integral and len(bank) == 3
    windows = GOLDEN['windows']
    got = bank.host_window_clips(windows[:, 0].astype(np.int64), windows[:, 1:])
    want, off = GOLDEN[f'sliced_r{int(relative)}'], GOLDEN[f'sliced_r{int(relative)}_offsets']
    assert len(got) == len(windows) == len(off) - 1 and off[-1] == len(want) > 300
    for w in range(len(windows)):
        assert_same_rows(got[w], want[off[w]:off[w + 1]], (relative, w))
    assert np.array_equal(bank.count_clips(windows[:, 0].astype(np.int64), windows[:, 1:]), np.diff(off))
    # slicing keeps the order amtx_eval_notes_match reads
    for g in got:
        assert np.array_equal(g[:, [2, 0]], ev._sort_rows(g)[:, [2, 0]])


@pytest.mark.parametrize('relative', [False, True])
def test_host_clips_equal_what_the_reference_returned_for_stacked_notes(relative):
    stacks = [{s: (GOLDEN[f'stack_T{i}_S{s}'][:, 2], GOLDEN[f'stack_T{i}_S{s}'][:, :2]) for s in range(6)} for i in range(3)]
    bank = NoteBank(stacks, relative_times=relative)
    assert bank.slices == 6 and bank.keys == list(range(6)) and bank.stacked and len(bank) == 3
    windows = GOLDEN['windows']
    got = bank.host_window_clips(windows[:, 0].astype(np.int64), windows[:, 1:])
    want, off = GOLDEN[f'stacked_r{int(relative)}'], GOLDEN[f'stacked_r{int(relative)}_offsets']
    assert len(got) == 6 * len(windows) == len(off) - 1
    for g in range(len(got)):
        assert_same_rows(got[g], want[off[g]:off[g + 1]], (relative, g))
    assert np.array_equal(bank.count_clips(windows[:, 0].astype(np.int64), windows[:, 1:]), np.diff(off))


def test_windows_equal_the_reference_arithmetic_bit_for_bit():
    cases = GOLDEN['window_cases']
    assert len(cases) == 60
    modules = {'mel': lambda hop, sr: MelSpec(sample_rate=sr, hop_length=hop, n_mels=229, n_fft=2048),
               'cqt': lambda hop, sr: CQT(sample_rate=sr, hop_length=hop, n_bins=192, bins_per_octave=24),
               'cqt48': lambda hop, sr: CQT(sample_rate=sr, hop_length=hop, n_bins=48, bins_per_octave=12)}
    for name, make in modules.items():
        want = GOLDEN[f'sec_{name}']
        for c, (first, frames, hop, sr) in enumerate(cases.tolist()):
            module = make(hop, sr)
            assert int(max(module.get_sample_range(frames))) == int(GOLDEN[f'seq_{name}'][c])
            got = clip_windows(module, [first], frames)
            assert got.dtype == np.float64 and got.shape == (1, 2) and got.view(np.uint64).tolist() == want[c:c + 1].view(np.uint64).tolist(), (name, c)
    # what the reference stores for 625 frames at hop 512 is one sample short of num_frames * hop_length; an early-downsampling CQT, eight
    c = cases.tolist().index([0, 625, 512, 22050])
    assert GOLDEN['seq_mel'][c] == 319999 and GOLDEN['seq_cqt48'][c] == 319992
    several = clip_windows(modules['mel'](512, 22050), [0, 1, 7], 40)
    assert several.view(np.uint64).tolist() == np.concatenate([GOLDEN['sec_mel'][cases.tolist().index([f, 40, 512, 22050])][None] for f in (0, 1, 7)]).view(np.uint64).tolist()


def test_boundary_rules():
    t = lambda k: k * HOP / SR          # noqa: E731
    notes = np.array([[t(2), t(10), 60.0],       # offset == start_time: dropped
                      [t(30), t(35), 61.0],      # onset == stop_time: kept, zero length
                      [t(5), t(50), 62.0],       # spans the window: clipped at both ends
                      [t(12), t(14), 63.0],      # inside: as it is
                      [t(31), t(40), 64.0],      # onset after stop_time: dropped
                      [t(10), t(10), 65.0],      # zero length ON start_time: offset is not > start_time, dropped
                      [t(11), t(11), 66.0]])     # zero length inside: kept
    window = [(t(10), t(30))]
    absolute = NoteBank([notes], relative_times=False).host_window_clips([0], window)[0]
    want = np.array([[t(30), t(30), 61.0], [t(10), t(30), 62.0], [t(12), t(14), 63.0], [t(11), t(11), 66.0]])
    assert_same_rows(absolute, want, 'absolute')
    relative = NoteBank([notes], relative_times=True).host_window_clips([0], window)[0]
    want[:, :2] -= t(10)
    assert_same_rows(relative, want, 'relative')
    assert relative[:, :2].min() == 0.0 and not np.signbit(relative[:, :2]).any()
    assert NoteBank([notes]).count_clips([0], window).tolist() == [4]
    # a time of -0.0 is stored as 0.0
    assert not np.signbit(NoteBank([np.array([[-0.0, 0.5, 60.0]])]).rows).any()


def test_cover_clips_counts():
    n = 40
    counts = [0, 1, n - 1, n, n + 1, 3 * n]
    ids, firsts, left_out = cover_clips(counts, n)
    assert ids.dtype == firsts.dtype == np.int64
    assert ids.tolist() == [3, 4, 5, 5, 5] and firsts.tolist() == [0, 0, 0, n, 2 * n]
    assert left_out == 0 + 1 + (n - 1) + 0 + 1 + 0
    assert len(ids) * n + left_out == sum(counts)                    # nothing padded, nothing counted twice
    for count in counts:
        ids, firsts, left_out = cover_clips([count], n)
        assert len(ids) == count // n and left_out == count % n and firsts.tolist() == [k * n for k in range(count // n)]
    assert cover_clips([5, 7], 1)[0].tolist() == [0] * 5 + [1] * 7 and cover_clips([5, 7], 1)[2] == 0
    assert cover_clips([], n)[0].size == 0
    with pytest.raises(ValueError, match=r'a clip has at least one frame \(got 0\)'):
        cover_clips([5], 0)


class _Module(object):
    hop_length, sample_rate = 512, 16000

    def get_sample_range(self, num_frames):
        return np.arange(1, num_frames * 512)


class _Bank(object):
    """What NoteBank reads of the audio bank of the same tracks."""
    frame_counts = np.array([130, 64, 1, 94])
    device = 'cuda:0'
    module = _Module()

    def __len__(self):
        return 4


def _four(**kw):
    return NoteBank([np.zeros((0, 3)), np.array([[0.0, 1.0, 60.0]]), np.zeros((0, 3)), np.array([[0.5, 0.75, 61.5]])], bank=_Bank(), **kw)


def test_refusals_at_construction():
    good = np.array([[0.0, 1.0, 60.0], [0.5, 0.75, 61.0]])
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[1, 0] = bad_value
        with pytest.raises(ValueError, match=r'^track 1, row 1: a note time is NaN or infinite$'):
            NoteBank([good, bad])
    bad = good.copy()
    bad[0, 1] = -0.25
    with pytest.raises(ValueError, match=r'^track 2, row 0: offset -0\.25 < onset 0\.0$'):
        NoteBank([good, good, bad])
    stack = lambda rows: {'E': (rows[:, 2], rows[:, :2]), 'A': (rows[:1, 2], rows[:1, :2])}     # noqa: E731
    bad = good.copy()
    bad[1, 1] = np.nan
    with pytest.raises(ValueError, match=r"^track 1, 'E', row 1: a note time is NaN or infinite$"):
        NoteBank([stack(good), stack(bad)])
    with pytest.raises(ValueError, match=r"^track 1 carries the keys \['A', 'E'\], track 0 \['E', 'A'\]$"):
        NoteBank([stack(good), dict(reversed(list(stack(good).items())))])
    with pytest.raises(ValueError, match=r"^track 1 carries the keys \['E'\], track 0 \['E', 'A'\]$"):
        NoteBank([stack(good), {'E': stack(good)['E']}])
    with pytest.raises(ValueError, match=r'^track 1 holds batched notes, track 0 stacked notes$'):
        NoteBank([stack(good), good])
    with pytest.raises(ValueError, match=r'^notes of 3 tracks for a bank of 4$'):
        NoteBank([good, good, good], bank=_Bank())
    with pytest.raises(ValueError, match=r'^notes: at least one track$'):
        NoteBank([])
    with pytest.raises(ValueError, match=r'^track 0: batched notes are \(N, 3\) rows \[onset, offset, pitch\], not \(2, 2\)$'):
        NoteBank([good[:, :2]])


def test_integral_is_what_the_device_matcher_takes():
    assert NoteBank([np.array([[0.0, 1.0, 0.0], [0.0, 1.0, 127.0]])]).integral
    for pitch in (60.5, -1.0, 128.0):
        assert not NoteBank([np.array([[0.0, 1.0, 60.0], [0.0, 1.0, pitch]])]).integral
    assert not _four().integral and NoteBank([np.zeros((0, 3))]).integral


def test_request_errors_are_the_other_banks_texts():
    """One check for all banks: the texts tests/test_pyramid_clips.py holds TrackBank, PyramidBank and LabelBank to."""
    bank = _four()
    labels = LabelBank([{'multi_pitch': np.zeros((2, T))} for T in _Bank.frame_counts], bank=_Bank())
    requests = [(([0, 1], [0], 10), 'one first frame per track id, and at least one clip'),
                (([], [], 10), 'one first frame per track id, and at least one clip'),
                (([0], [0], 0), r'a clip has at least one frame \(got 0\)'),
                (([4], [0], 10), 'unknown track 4: the bank holds 4 tracks'),
                (([-1], [0], 10), 'unknown track -1: the bank holds 4 tracks'),
                (([0], [-3], 10), 'negative first frame -3'),
                (([0, 1], [0, 60], 10), r'clip 1: frames \[60, 70\) run past the 64 frames of track 1'),
                (([2], [0], 2), r'clip 0: frames \[0, 2\) run past the 1 frames of track 2')]
    for args, text in requests:
        for method in (bank.host_clips, bank.clips, labels.clips):
            with pytest.raises(ValueError, match='^' + text + '$'):
                method(*args)
    with pytest.raises(ValueError, match='a NoteBank built without a bank has no frame grid'):
        NoteBank([np.zeros((0, 3))]).host_clips([0], [0], 10)
    with pytest.raises(ValueError, match=r'^clip 0: the window \[1\.0, 0\.5\] is not 0 <= start_time <= stop_time, both finite$'):
        bank.host_window_clips([0], [(1.0, 0.5)])
    with pytest.raises(ValueError, match='^unknown track 4: the bank holds 4 tracks$'):
        bank.host_window_clips([4], [(0.0, 0.5)])
    # the windows of a clips() request are clip_windows of the bank's module
    got = bank.host_clips([3, 1], [0, 10], 40)
    want = bank.host_window_clips([3, 1], [(0.0, (40 * 512 - 1) / 16000), (10 * 512 / 16000, (50 * 512 - 1) / 16000)])
    assert [g.tobytes() for g in got] == [w.tobytes() for w in want] and [len(g) for g in got] == [1, 1]
    assert got[0].tolist() == [[0.5, 0.75, 61.5]] and got[1].tolist() == [[0.0, 1.0 - 0.32, 60.0]]


def test_a_bank_is_pickled_without_device_state():
    bank = _four()
    bank.__dict__['_dev'] = object()
    twin = pickle.loads(pickle.dumps(bank))
    assert '_dev' not in twin.__dict__ and twin.rows.tobytes() == bank.rows.tobytes() and twin.group_ptr.tolist() == bank.group_ptr.tolist() == [0, 0, 1, 1, 2]


def test_validate_clips_names_a_missing_bank_before_any_launch():
    bank = _Bank()
    labels = LabelBank([{tools.KEY_MULTIPITCH: np.zeros((2, T))} for T in _Bank.frame_counts], bank=bank)
    piano = ev.ComboEvaluator([ev.MultipitchEvaluator(), ev.NoteEvaluator()])
    args = (None, piano, [0], [0], 10)
    with pytest.raises(ValueError, match=r"^MultipitchEvaluator scores the label map 'multi_pitch': validate_clips needs a LabelBank for it$"):
        ev.validate_clips(bank, None, _four(), *args)
    with pytest.raises(ValueError, match=r'^NoteEvaluator scores notes: validate_clips needs a NoteBank for it$'):
        ev.validate_clips(bank, labels, None, *args)
    with pytest.raises(ValueError, match=r"^TablatureEvaluator scores the label map 'tablature', the LabelBank holds \['multi_pitch'\]$"):
        ev.validate_clips(bank, labels, None, None, ev.TablatureEvaluator(tools.GuitarProfile()), [0], [0], 10)
    with pytest.raises(ValueError, match=r'^StackedNoteEvaluator scores stacked notes, the NoteBank holds batched notes$'):
        ev.validate_clips(bank, None, _four(), None, ev.StackedNoteEvaluator(), [0], [0], 10)
    with pytest.raises(ValueError, match='relative_times=True'):
        ev.validate_clips(bank, None, _four(relative_times=False), None, ev.NoteEvaluator(), [0], [0], 10)
    with pytest.raises(ValueError, match=r'^clip 0: frames \[60, 70\) run past the 64 frames of track 1$'):
        ev.validate_clips(bank, labels, _four(), None, piano, [1], [60], 10)


def test_banks_are_exported():
    assert TrackBank and PyramidBank and {'NoteBank', 'NoteClips', 'cover_clips', 'clip_windows'} <= set(__import__('amt_tools_amd.tracks', fromlist=['x']).__all__)
    assert 'validate_clips' in ev.__all__
