"""Host side of label clips cut from resident tracks (amt_tools_amd/tracks.py LabelBank / ClipLoader, include/amtx_labels.h): the
run-length encoding round-trips every bit, the bank validates its maps, clips are drawn by the reference's rule, the loader hands the
same clips to both banks, and the header's entry point refuses bad arguments by name (its pinned table: tests/test_capi.py).  No GPU here."""
import pickle

import numpy as np
import pytest

from amt_tools_amd import _lib, cache, tools
from amt_tools_amd.tracks import ClipLoader, LabelBank, clip_descriptors, decode_rows, draw_clips, encode_rows

I32 = np.iinfo(np.int32)


def _float_maps():
    nan_payload = np.array([0x7FC00123], dtype=np.uint32).view(np.float32)[0]
    special = np.array([[0.25, 0.25, -0.0, 0.0, np.nan, np.nan, 1.0], [-0.0, -0.0, -0.0, nan_payload, np.nan, 0.25, 0.25]], dtype=np.float32)
    return {'zeros': np.zeros((3, 9)), 'constant': np.full((2, 9), 1.0), 'alternating': (np.arange(11) % 2)[None].astype(np.float64),
            'one_frame': np.array([[0.0], [1.0], [0.25]]), 'special': special, 'special64': special.astype(np.float64)}


def _int_maps():
    return {'tablature': np.array([[-1, -1, 20, 20, 20, 0], [I32.max, I32.max, I32.min, I32.min, -1, 20]], dtype=np.int64),
            'zeros': np.zeros((4, 5), dtype=np.int32), 'alternating': (np.arange(8) % 2)[None].astype(np.uint8),
            'one_frame': np.array([[I32.min], [I32.max]], dtype=np.int64), 'bool': np.array([[True, True, False, True]])}


@pytest.mark.parametrize('name', sorted(_float_maps()))
def test_float_maps_round_trip_bit_for_bit(name):
    m = _float_maps()[name]
    row_ptr, run_first, run_bits = encode_rows(m)
    assert (row_ptr.dtype, run_first.dtype, run_bits.dtype) == (np.int64, np.int32, np.int32) and row_ptr.shape == (m.shape[0] + 1,)
    back = decode_rows(row_ptr, run_first, run_bits, m.shape[1])
    assert back.dtype == np.float32 and back.shape == m.shape
    np.testing.assert_array_equal(back.view(np.uint32), m.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize('name', sorted(_int_maps()))
def test_integer_maps_round_trip(name):
    m = _int_maps()[name]
    back = decode_rows(*encode_rows(m), m.shape[1], dtype=np.int64)
    assert back.dtype == np.int64 and back.shape == m.shape
    np.testing.assert_array_equal(back, m.astype(np.int64))


def test_encoding_structure():
    for m in list(_float_maps().values()) + list(_int_maps().values()):
        row_ptr, run_first, run_bits = encode_rows(m)
        assert row_ptr[0] == 0 and row_ptr[-1] == len(run_first) == len(run_bits)
        for r in range(m.shape[0]):
            first = run_first[row_ptr[r]:row_ptr[r + 1]]
            assert len(first) >= 1 and first[0] == 0 and (np.diff(first) > 0).all() and first[-1] < m.shape[1]
    for T in (1, 2, 64, 65):
        row_ptr, run_first, _ = encode_rows((np.arange(T) % 2)[None].astype(np.float32))
        assert row_ptr.tolist() == [0, T] and run_first.tolist() == list(range(T))
    assert encode_rows(np.zeros((3, 100)))[0].tolist() == [0, 1, 2, 3]                  # a constant row is one run
    # split where the PATTERN changes, not where != says so: NaN next to the same NaN is one run, -0.0 next to 0.0 two
    assert encode_rows(np.array([[np.nan, np.nan, -0.0, 0.0]], dtype=np.float32))[1].tolist() == [0, 2, 3]


def test_values_the_patterns_cannot_hold_are_refused_by_row_and_frame():
    m = np.zeros((3, 5))
    m[2, 3] = 0.1                                                        # float64 0.1 is no float32 value
    with pytest.raises(ValueError, match='row 2, frame 3: float32 does not hold'):
        encode_rows(m)
    m[2, 3] = 1e300
    with pytest.raises(ValueError, match='row 2, frame 3'):
        encode_rows(m)
    encode_rows(np.array([[np.float64(np.float32(0.1)), np.inf, -np.inf, np.nan]]))
    for value in (2 ** 31, -2 ** 31 - 1):
        n = np.zeros((2, 4), dtype=np.int64)
        n[1, 2] = value
        with pytest.raises(ValueError, match=f'row 1, frame 2: {value} is outside int32'):
            encode_rows(n)
    with pytest.raises(ValueError, match='row 0, frame 1: 4294967295 is outside int32'):
        encode_rows(np.array([[0, 2 ** 32 - 1]], dtype=np.uint32))
    with pytest.raises(ValueError, match=r'\(rows, frames\)'):
        encode_rows(np.zeros(5))
    with pytest.raises(TypeError, match='floating, integer or bool'):
        encode_rows(np.zeros((2, 2), dtype=np.complex64))


class _Bank(object):
    """What LabelBank and ClipLoader read of a TrackBank / PyramidBank, without a device; clips() records its arguments."""

    def __init__(self, lengths, hop_length=512):
        import types
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.frame_counts = 1 + self.lengths // hop_length
        self.module = types.SimpleNamespace(hop_length=hop_length)
        self.device = 'cuda:0'
        self.calls = []

    def __len__(self):
        return len(self.lengths)

    def clips(self, track_ids, first_frames, num_frames):
        self.calls.append((np.array(track_ids), np.array(first_frames), num_frames))
        return ('clips', len(self.calls))


def _maps(widths, rng=None):
    rng = rng or np.random.default_rng(0)
    return [{tools.KEY_MULTIPITCH: (rng.random((5, T)) < 0.3).astype(np.float64), tools.KEY_TABLATURE: rng.integers(-1, 21, (3, T))} for T in widths]


def test_label_bank_tables_and_host_maps():
    maps = _maps((7, 1, 12))
    bank = LabelBank(maps)
    assert len(bank) == 3 and bank.rows_total == 8 and bank.keys == [tools.KEY_MULTIPITCH, tools.KEY_TABLATURE]
    assert bank.float_keys == [(tools.KEY_MULTIPITCH, 5)] and bank.int_keys == [(tools.KEY_TABLATURE, 3)]
    np.testing.assert_array_equal(bank.frame_counts, [7, 1, 12])
    assert bank.row_ptr.shape == (3 * 8 + 1,) and bank.row_ptr[-1] == len(bank.run_first) == len(bank.run_bits)
    assert bank.runs_per_track.sum() == len(bank.run_first) and bank.runs_per_track[1] == 8
    assert bank.nbytes == bank.row_ptr.nbytes + 8 * len(bank.run_first)
    for i, entry in enumerate(maps):
        np.testing.assert_array_equal(bank.host_map(i, tools.KEY_MULTIPITCH), entry[tools.KEY_MULTIPITCH].astype(np.float32))
        np.testing.assert_array_equal(bank.host_map(i, tools.KEY_TABLATURE), entry[tools.KEY_TABLATURE])
        assert bank.host_map(i, tools.KEY_MULTIPITCH).dtype == np.float32 and bank.host_map(i, tools.KEY_TABLATURE).dtype == np.int64
    # integer keys' rows come after the floating keys' whatever the dict's order
    swapped = LabelBank([{tools.KEY_TABLATURE: e[tools.KEY_TABLATURE], tools.KEY_MULTIPITCH: e[tools.KEY_MULTIPITCH]} for e in maps])
    for name in ('row_ptr', 'run_first', 'run_bits'):
        np.testing.assert_array_equal(getattr(swapped, name), getattr(bank, name))
    assert '_dev' not in bank.__dict__                                    # nothing touched a device


def test_label_bank_refusals_name_the_track():
    good = _maps((7, 9))
    with pytest.raises(ValueError, match="track 0, 'multi_pitch': row 1, frame 2: float32 does not hold"):
        bad = _maps((7,))
        bad[0][tools.KEY_MULTIPITCH][1, 2] = 0.3
        LabelBank(bad)
    with pytest.raises(ValueError, match="track 1, 'tablature': row 0, frame 0: 2147483648 is outside int32"):
        bad = _maps((7, 9))
        bad[1][tools.KEY_TABLATURE][0, 0] = 2 ** 31
        LabelBank(bad)
    with pytest.raises(ValueError, match='track 1 carries the keys'):
        LabelBank([good[0], {tools.KEY_MULTIPITCH: good[1][tools.KEY_MULTIPITCH]}])
    with pytest.raises(ValueError, match='track 1 carries the keys'):
        LabelBank([good[0], dict(good[1], **{tools.KEY_ONSETS: good[1][tools.KEY_MULTIPITCH]})])
    with pytest.raises(ValueError, match="track 1, 'multi_pitch': shape .4, 9., but track 0 has 5 rows"):
        LabelBank([good[0], dict(good[1], **{tools.KEY_MULTIPITCH: good[1][tools.KEY_MULTIPITCH][:4]})])
    with pytest.raises(ValueError, match="track 1, 'tablature': dtype float64, but track 0 holds integer"):
        LabelBank([good[0], dict(good[1], **{tools.KEY_TABLATURE: good[1][tools.KEY_TABLATURE].astype(np.float64)})])
    with pytest.raises(ValueError, match="track 1: 'tablature' has 8 frames, 'multi_pitch' has 9"):
        LabelBank([good[0], dict(good[1], **{tools.KEY_TABLATURE: good[1][tools.KEY_TABLATURE][:, :8]})])
    audio = _Bank([6 * 512 + 5, 9 * 512])                                  # 7 and 10 frames
    with pytest.raises(ValueError, match='track 1: its label maps have 9 frames, the bank has 10 frames'):
        LabelBank(good, bank=audio)
    with pytest.raises(ValueError, match='label maps of 1 tracks for a bank of 2'):
        LabelBank(good[:1], bank=audio)
    with pytest.raises(ValueError, match='track 2: its label maps have 7 frames, the bank has only 2 tracks'):
        LabelBank(_maps((7, 10, 7)), bank=audio)
    with pytest.raises(ValueError, match='at least one track'):
        LabelBank([])
    assert len(LabelBank(_maps((7, 10)), bank=audio)) == 2


@pytest.mark.parametrize('track_ids,first_frames,num_frames,match', [
    ([2], [0], 1, 'unknown track 2'),
    ([-1], [0], 1, 'unknown track -1'),
    ([0], [-1], 4, 'negative first frame'),
    ([0], [5], 3, 'clip 0: .* run past the 7 frames of track 0'),
    ([0, 1], [0, 7], 3, 'clip 1: .* run past the 9 frames'),
    ([0], [0], 0, 'at least one frame'),
    ([0, 1], [0], 2, 'one first frame per track id'),
])
def test_invalid_clip_requests_raise_before_any_device_is_touched(track_ids, first_frames, num_frames, match):
    bank = LabelBank(_maps((7, 9)))
    with pytest.raises(ValueError, match=match):
        bank.clips(track_ids, first_frames, num_frames)
    assert '_dev' not in bank.__dict__


def test_label_bank_pickles_without_device_state():
    bank = LabelBank(_maps((7, 9)))
    bank.__dict__['_dev'] = ('row_ptr', 'run_first', 'run_bits')            # stands for the device tensors
    again = pickle.loads(pickle.dumps(bank))
    assert '_dev' not in again.__dict__ and again.keys == bank.keys and again.rows_total == bank.rows_total
    for name in ('row_ptr', 'run_first', 'run_bits', 'frame_counts'):
        np.testing.assert_array_equal(getattr(again, name), getattr(bank, name))


@pytest.mark.parametrize('ambiguity', [None, 0.05])
def test_from_notes_holds_the_host_maps_of_the_same_notes(ambiguity):
    profile = tools.PianoProfile()
    rng = np.random.default_rng(3)
    notes, times = [], []
    for T in (300, 41):
        grid = np.arange(T) * 512 / 16000.0
        n = 40
        onsets = rng.uniform(-0.2, grid[-1] + 0.1, n)                      # some notes start before the grid or end past it
        notes.append((rng.integers(15, 115, n).astype(np.float64), np.stack([onsets, onsets + rng.uniform(0.01, 1.5, n)], axis=1)))
        times.append(grid)
    bank = LabelBank.from_notes(notes, times, profile, ambiguity=ambiguity)
    assert bank.keys == [tools.KEY_MULTIPITCH, tools.KEY_ONSETS, tools.KEY_OFFSETS] and not bank.int_keys and bank.rows_total == 3 * 88
    for i, ((pitches, intervals), grid) in enumerate(zip(notes, times)):
        want = {tools.KEY_MULTIPITCH: cache.notes_to_multi_pitch(pitches, intervals, grid, profile),
                tools.KEY_ONSETS: cache.notes_to_onsets(pitches, intervals, grid, profile, ambiguity),
                tools.KEY_OFFSETS: cache.notes_to_offsets(pitches, intervals, grid, profile, ambiguity)}
        assert want[tools.KEY_MULTIPITCH].sum() > 0 and want[tools.KEY_ONSETS].sum() > 0
        for key, ref in want.items():
            got = bank.host_map(i, key)
            assert got.dtype == np.float32 and got.shape == (88, len(grid))
            np.testing.assert_array_equal(got, ref)
    only = LabelBank.from_notes(notes, times, profile, keys=(tools.KEY_ONSETS,))
    np.testing.assert_array_equal(only.host_map(1, tools.KEY_ONSETS), cache.notes_to_onsets(*notes[1], times[1], profile))
    with pytest.raises(ValueError, match="no label map 'tablature' from notes"):
        LabelBank.from_notes(notes, times, profile, keys=(tools.KEY_TABLATURE,))


def test_draw_clips_is_the_reference_rule():
    """amt_tools/datasets/common.py:340-343, written out by hand for a fixed RandomState."""
    lengths, hop, num_frames = np.array([40000, 5000, 16001, 5120]), 512, 9
    ids = [2, 0, 0, 3, 1, 2]
    got = draw_clips(np.random.RandomState(11), lengths, hop, num_frames, ids)
    rng = np.random.RandomState(11)
    want = []
    for k in ids:
        seq_length = num_frames * hop
        sample_start = rng.randint(0, lengths[k] - seq_length)
        want.append(sample_start // hop)
    assert got.dtype == np.int64 and got.tolist() == want
    clip_descriptors(np.zeros(4), lengths, 1 + lengths // hop, ids, got, num_frames)          # every drawn clip exists
    many = draw_clips(np.random.RandomState(0), lengths, hop, num_frames, [1] * 200)           # 5000 - 4608 = 392 starts: frame 0 only
    assert set(many.tolist()) == {0}
    many = draw_clips(np.random.RandomState(0), lengths, hop, 1, [3] * 500)                    # the last frame of a track is reachable ...
    assert many.min() == 0 and many.max() == 8                                                 # ... up to (5120 - 512 - 1) // 512
    clip_descriptors(np.zeros(4), lengths, 1 + lengths // hop, [3] * 500, many, 1)
    with pytest.raises(ValueError, match='track 1 has 4608 samples: a clip of 9 frames needs more than 4608'):
        draw_clips(np.random.RandomState(0), [40000, 4608], hop, num_frames, [0, 1])           # length == seq_length
    draw_clips(np.random.RandomState(0), [40000, 4609], hop, num_frames, [0, 1])
    with pytest.raises(ValueError, match='unknown track 2'):
        draw_clips(np.random.RandomState(0), [40000, 4609], hop, num_frames, [2])


class _Labels(_Bank):
    def clips(self, track_ids, first_frames, num_frames):
        self.calls.append((np.array(track_ids), np.array(first_frames), num_frames))
        return {tools.KEY_ONSETS: ('onsets', len(self.calls)), tools.KEY_MULTIPITCH: ('multi_pitch', len(self.calls))}


@pytest.mark.parametrize('drop_last,batches', [(True, 2), (False, 3)])
def test_clip_loader_deals_an_epoch_and_asks_both_banks_for_the_same_clips(drop_last, batches):
    lengths = [40000, 9000, 16001, 30000, 12345, 8000, 20000]
    bank, labels = _Bank(lengths), _Labels(lengths)
    loader = ClipLoader(bank, labels, num_frames=9, batch_size=3, seed=5, drop_last=drop_last)
    assert len(loader) == batches
    for epoch in range(2):
        bank.calls.clear()
        labels.calls.clear()
        got = list(loader)
        assert len(got) == batches == len(bank.calls) == len(labels.calls)
        for n, batch in enumerate(got):
            assert sorted(batch) == sorted([tools.KEY_AUDIO, tools.KEY_ONSETS, tools.KEY_MULTIPITCH])
            assert batch[tools.KEY_AUDIO] == ('clips', n + 1) and batch[tools.KEY_ONSETS] == ('onsets', n + 1)
        seen = []
        for (ids, firsts, T), (lids, lfirsts, lT) in zip(bank.calls, labels.calls):
            np.testing.assert_array_equal(ids, lids)
            np.testing.assert_array_equal(firsts, lfirsts)
            assert T == lT == 9
            clip_descriptors(np.zeros(7), bank.lengths, bank.frame_counts, ids, firsts, T)
            seen += ids.tolist()
        assert [len(c[0]) for c in bank.calls] == ([3, 3] if drop_last else [3, 3, 1])
        assert len(set(seen)) == len(seen) and (sorted(seen) == list(range(7)) if not drop_last else len(seen) == 6)
        if epoch == 0:
            first_epoch = [c[0].tolist() + c[1].tolist() for c in bank.calls]
    # the same seed gives the same epochs; the loader's state moves on from epoch to epoch
    again = ClipLoader(_Bank(lengths), _Labels(lengths), 9, 3, seed=5, drop_last=drop_last)
    list(again)
    assert [c[0].tolist() + c[1].tolist() for c in again.bank.calls] == first_epoch
    # the permutation and the draws are the loader's RandomState's, in this order
    rng = np.random.RandomState(5)
    order = rng.permutation(7)
    assert first_epoch[0][:3] == order[:3].tolist()
    assert first_epoch[0][3:] == draw_clips(rng, lengths, 512, 9, order[:3]).tolist()
    with pytest.raises(ValueError, match='a bank of 7 tracks and labels of 2'):
        ClipLoader(bank, _Labels(lengths[:2]), 9, 3)
    with pytest.raises(ValueError, match='track 5 has 8000 samples'):
        list(ClipLoader(_Bank(lengths), _Labels(lengths), 16, 7, seed=0))


# ------------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
def test_an_undeclared_name_is_refused_with_every_header_named():
    with pytest.raises(_lib.AmtxError, match='amtx.h, amtx_tracks.h, amtx_pyramid.h, amtx_labels.h declare no function amtx_nothing'):
        _lib.call('amtx_nothing')


def _args(**change):
    """A complete, valid argument list of amtx_label_clips over host arrays (nothing is launched: every case below is refused first)."""
    host = np.zeros(8, dtype=np.int64)
    args = dict(row_ptr=host, run_first=host, run_bits=host, num_tracks=1, rows_total=8, row_lo=0, row_hi=8, key_rows=np.array([0, 5, 8]),
                num_keys=2, desc=host, batch=1, num_frames=4, out=host, out_kind=0, stream=None)
    assert not set(change) - set(args)
    args.update(change)
    return tuple(args.values())


@pytest.mark.parametrize('change,match', [
    (dict(row_ptr=None), 'amtx_label_clips: null'), (dict(run_first=None), 'amtx_label_clips: null'),
    (dict(run_bits=None), 'amtx_label_clips: null'), (dict(key_rows=None), 'amtx_label_clips: null'),
    (dict(desc=None), 'amtx_label_clips: null'), (dict(out=None), 'amtx_label_clips: null'),
    (dict(batch=0), 'amtx_label_clips: batch=0'), (dict(num_frames=0), 'amtx_label_clips: num_frames=0'),
    (dict(num_frames=2 ** 31), 'amtx_label_clips: num_frames=2147483648'),
    (dict(num_tracks=0), 'amtx_label_clips: num_tracks=0'), (dict(rows_total=0), 'amtx_label_clips: num_tracks=1, rows_total=0'),
    (dict(row_lo=8), 'amtx_label_clips: row_lo=8, row_hi=8: an empty row range'),
    (dict(row_hi=9), 'amtx_label_clips: row_lo=0, row_hi=9'), (dict(row_lo=-1), 'amtx_label_clips: row_lo=-1'),
    (dict(num_keys=0), 'amtx_label_clips: num_keys=0'), (dict(num_keys=17), 'amtx_label_clips: num_keys=17'),
    (dict(key_rows=np.array([0, 5, 5])), r'amtx_label_clips: key_rows\[2\]=5'),
    (dict(key_rows=np.array([1, 5, 8])), 'amtx_label_clips: key_rows must start at row_lo=0'),
    (dict(key_rows=np.array([0, 5, 7])), 'amtx_label_clips: key_rows must start at row_lo=0 and end at row_hi=8'),
    (dict(key_rows=np.array([0, 9, 8])), r'amtx_label_clips: key_rows\[1\]=9'),
    (dict(out_kind=2), 'amtx_label_clips: out_kind=2'),
])
def test_entry_point_refuses_bad_arguments_by_name(change, match):
    with pytest.raises(_lib.AmtxError, match=match):
        _lib.call('amtx_label_clips', *_args(**change))


def test_entry_point_counts_its_arguments():
    args = _args()
    with pytest.raises(TypeError, match='amtx_label_clips takes 15 arguments'):
        _lib.call('amtx_label_clips', *args[:-1])
    with pytest.raises(TypeError, match='amtx_label_clips takes 15 arguments'):
        _lib.call('amtx_label_clips', *args, None)
