"""Host side of CQT-family clips cut from resident pyramids (amt_tools_amd/tracks.py PyramidBank, include/amtx_pyramid.h): requests are
validated on the host -- by one check, with one text, for the three banks --, the bank's bookkeeping needs no device, and every entry
point of the header reports a null plan by name (the header's pinned table: tests/test_capi.py).  No GPU here."""
import pickle

import numpy as np
import pytest

from amt_tools_amd import _lib
from amt_tools_amd.features import CQT, HCQT, MelSpec
from amt_tools_amd.tracks import LabelBank, PyramidBank, PyramidClips, TrackBank, TrackClips, clip_descriptors

LENGTHS = (40000, 5001, 1500)


def _tracks():
    rng = np.random.default_rng(0)
    return [rng.standard_normal(n).astype(np.float32) for n in LENGTHS]


def test_bank_bookkeeping_needs_no_gpu_and_pickles_without_device_state():
    tracks = _tracks()
    mod = CQT(sample_rate=22050, hop_length=512, n_bins=192, bins_per_octave=24)
    bank = PyramidBank(tracks, mod)
    np.testing.assert_array_equal(bank.lengths, LENGTHS)
    np.testing.assert_array_equal(bank.starts, [0, 40000, 45004])                   # every track at a multiple of 4 elements
    np.testing.assert_array_equal(bank.frame_counts, [mod.get_expected_frames(t) for t in tracks])
    np.testing.assert_array_equal(bank.frame_counts, [79, 10, 3])
    assert len(bank) == 3 and '_dev' not in bank.__dict__                            # nothing touched a device
    for start, t in zip(bank.starts, tracks):
        np.testing.assert_array_equal(bank._host[start:start + t.size], t)
    again = pickle.loads(pickle.dumps(bank))
    np.testing.assert_array_equal(again._host, bank._host)
    np.testing.assert_array_equal(again.frame_counts, bank.frame_counts)
    bank.__dict__['_dev'] = ('audio', 'db_ref', 'pyramid', 'table')                  # stands for the device tensors
    assert '_dev' not in pickle.loads(pickle.dumps(bank)).__dict__
    # HCQT: the smallest count over its harmonics
    hmod = HCQT(sample_rate=22050, hop_length=512, n_bins=72)
    np.testing.assert_array_equal(PyramidBank(tracks, hmod).frame_counts, [hmod.get_expected_frames(t) for t in tracks])
    with pytest.raises(TypeError, match='a PyramidBank takes a CQT, VQT, HCQT or HVQT'):
        PyramidBank(tracks, MelSpec())
    with pytest.raises(ValueError, match='non-empty 1-D'):
        PyramidBank([np.zeros((2, 100), dtype=np.float32)], mod)


INVALID_REQUESTS = [
    ([3], [0], 1, 'unknown track 3'),
    ([-1], [0], 1, 'unknown track -1'),
    ([0], [-1], 4, 'negative first frame'),
    ([0], [77], 3, 'clip 0: .* run past the 79 frames of track 0'),               # one frame too far
    ([0, 1], [0, 8], 3, 'clip 1: .* run past the 10 frames'),
    ([2], [0], 4, 'run past the 3 frames of track 2'),                              # a track shorter than the clip
    ([0], [0], 0, 'at least one frame'),
    ([0, 1], [0], 2, 'one first frame per track id'),
]


@pytest.mark.parametrize('track_ids,first_frames,num_frames,match', INVALID_REQUESTS)
def test_invalid_requests_raise_before_any_device_is_touched(track_ids, first_frames, num_frames, match):
    bank = PyramidBank(_tracks(), CQT(sample_rate=22050, hop_length=512, n_bins=192, bins_per_octave=24))
    with pytest.raises(ValueError, match=match):
        bank.clips(track_ids, first_frames, num_frames)
    assert '_dev' not in bank.__dict__


class _Bank(object):
    """What LabelBank reads of the audio bank of the same tracks."""
    device = 'cuda:0'
    frame_counts = np.array([79, 10, 3])

    def __len__(self):
        return 3


def _bank(kind):
    if kind == 'track':
        return TrackBank(_tracks(), MelSpec(sample_rate=16000, hop_length=512))
    if kind == 'pyramid':
        return PyramidBank(_tracks(), CQT(sample_rate=22050, hop_length=512, n_bins=192, bins_per_octave=24))
    return LabelBank([{'multi_pitch': np.zeros((2, T))} for T in _Bank.frame_counts], bank=_Bank())


@pytest.mark.parametrize('kind', ['track', 'pyramid', 'label'])
def test_every_bank_refuses_the_same_requests_with_the_same_text(kind):
    """One request check for the three banks: every row of INVALID_REQUESTS raises from bank.clips the ValueError, word for word, that
    clip_descriptors raises for it over the same frame counts, and no device state has been created afterwards."""
    bank = _bank(kind)
    np.testing.assert_array_equal(bank.frame_counts, _Bank.frame_counts)
    for track_ids, first_frames, num_frames, match in INVALID_REQUESTS:
        with pytest.raises(ValueError, match=match) as want:
            clip_descriptors(np.zeros(3), bank.frame_counts, bank.frame_counts, track_ids, first_frames, num_frames)
        with pytest.raises(ValueError, match=match) as got:
            bank.clips(track_ids, first_frames, num_frames)
        assert str(got.value) == str(want.value)
        assert '_dev' not in bank.__dict__


def test_raw_audio_bank_and_foreign_arguments_still_have_no_clip_form():
    with pytest.raises(NotImplementedError, match='no clip form'):
        TrackBank(_tracks(), CQT())
    for arg in (None, object()):
        for call in (CQT().power_clips, CQT().process_clips, CQT().process_clips16, HCQT(n_bins=72).process_clips):
            with pytest.raises(NotImplementedError, match='no clip form'):
                call(arg)
    assert PyramidClips(None, np.array([[1, 5, 33]]), None, None).num_frames == 33
    assert TrackClips(None, np.array([[40000, 5001, 5, 33]]), None, None).num_frames == 33


def test_an_undeclared_name_is_refused_with_every_header_named():
    with pytest.raises(_lib.AmtxError, match='amtx.h, amtx_tracks.h, amtx_pyramid.h, amtx_labels.h declare no function amtx_nothing'):
        _lib.call('amtx_nothing')


NULL_CALLS = {
    'amtx_cqt_track_cols': (None,),
    'amtx_cqt_track_layout': (None, 1000, None, None, None, None),
    'amtx_cqt_pyramid_build': (None, None, 0, None, None, 1, None, 0, None, None),
    'amtx_cqt_power_clips': (None, None, None, None, None, 1, 1, None, None),
    'amtx_cqt_clips': (None, None, None, None, None, 1, 1, None, 1, None, 0, None, None),
    'amtx_cqt_clips16': (None, None, None, None, None, 1, 1, None, 1, None, 0, None, None),
    'amtx_cqt_clips16_split': (None, None, None, None, None, 1, 1, None, 1, None, 0, None, 8, None),
}


def test_every_new_entry_point_is_covered_below():
    assert sorted(list(NULL_CALLS) + ['amtx_cqt_clips_workspace_bytes']) == sorted(_lib.header_signatures()['amtx_pyramid.h'])


@pytest.mark.parametrize('name', sorted(NULL_CALLS))
def test_entry_point_reports_a_null_plan_by_name_and_counts_its_arguments(name):
    args = NULL_CALLS[name]
    with pytest.raises(_lib.AmtxError, match=name + ': null'):
        _lib.call(name, *args)
    with pytest.raises(TypeError, match=f'{name} takes {len(args)} arguments'):
        _lib.call(name, *args[:-1])


def test_workspace_query_answers_zero_for_a_null_plan():
    assert _lib.call('amtx_cqt_clips_workspace_bytes', None, 1, 1) == 0
    with pytest.raises(TypeError, match='amtx_cqt_clips_workspace_bytes takes 3 arguments'):
        _lib.call('amtx_cqt_clips_workspace_bytes', None, 1)
