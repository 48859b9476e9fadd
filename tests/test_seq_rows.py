"""Exact whole tracks on the CPU: the tables of the packed-row route (tracks.track_groups, sequence_table, gather_table) built from a
tracks.seam_clips plan, tracks.gather_rows_host against plain slicing, and every refusal of exact=True before anything is launched."""
import inspect

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from amt_tools_amd import _lib, evaluate as ev, inference, tools                       # noqa: E402
from amt_tools_amd.tracks import gather_rows_host, gather_table, seam_clips, sequence_table, track_groups   # noqa: E402

COUNTS = np.array([118, 59, 40, 23, 118, 300])


@pytest.mark.parametrize('num_frames,margin', [(40, 3), (24, 5), (40, 0), (7, 3)])
def test_tables_of_a_seam_plan_write_every_packed_row_once(num_frames, margin):
    row0, seqs = sequence_table(COUNTS)
    total = int(COUNTS.sum())
    assert row0.tolist() == np.concatenate(([0], np.cumsum(COUNTS)[:-1])).tolist() and seqs.dtype == np.int64 and seqs.shape == (6, 2)
    # longest first, ties in slot order; every sequence is its slot's rows
    assert seqs[:, 1].tolist() == [300, 118, 118, 59, 40, 23] and seqs[:, 0].tolist() == [row0[5], row0[0], row0[4], row0[1], row0[2], row0[3]]
    plan = seam_clips(COUNTS, num_frames, margin)
    passes = [(num_frames, plan.track_ids, plan.first_frames, plan.kept)]
    for t in plan.short.tolist():                                                          # a short track: one clip of its own length, all kept
        passes.append((int(COUNTS[t]), np.array([t]), np.array([0]), np.array([[0, 0, COUNTS[t]]])))
    written = np.zeros(total, dtype=np.int64)
    for frames, slots, firsts, kept in passes:
        table = gather_table(row0, slots, kept)
        assert table.dtype == np.int64 and table.shape == (len(slots), 3) and table.flags.c_contiguous
        for (src_first, count, dst_row), t, first in zip(table.tolist(), slots.tolist(), firsts.tolist()):
            written[dst_row:dst_row + count] += 1
            assert 0 <= src_first and src_first + count <= frames and row0[t] <= dst_row and dst_row + count <= row0[t] + COUNTS[t]
            assert dst_row - row0[t] == first + src_first                                 # the kept rows are the track's own frames
            # at least `margin` frames from a clip edge that is no track edge
            assert first == 0 or src_first >= margin
            assert first + frames == COUNTS[t] or frames - (src_first + count) >= margin
    assert (written == 1).all()
    assert plan.short.tolist() == [t for t, n in enumerate(COUNTS.tolist()) if n < num_frames]


def test_track_groups_take_tracks_in_request_order_up_to_max_rows():
    assert track_groups(COUNTS, 1 << 18) == [(0, 6)]
    assert track_groups(COUNTS, 177) == [(0, 2), (2, 4), (4, 5), (5, 6)]                   # 118 + 59 fits exactly; the 300-frame track runs alone
    assert track_groups(COUNTS, 100) == [(0, 1), (1, 3), (3, 4), (4, 5), (5, 6)]          # tracks longer than max_rows: alone, never split
    assert track_groups(COUNTS, 1) == [(j, j + 1) for j in range(6)]
    assert track_groups([5], 3) == [(0, 1)] and track_groups([], 3) == []
    for counts, max_rows in ((COUNTS, 177), (COUNTS, 100), (COUNTS, 400)):
        groups = track_groups(counts, max_rows)
        assert [lo for lo, _ in groups] == [0] + [hi for _, hi in groups[:-1]] and groups[-1][1] == len(counts)
        for (lo, hi), nxt in zip(groups, groups[1:] + [None]):
            assert hi - lo == 1 or counts[lo:hi].sum() <= max_rows
            assert nxt is None or counts[lo:hi].sum() + counts[nxt[0]] > max_rows          # greedy: the next track would not have fitted
    with pytest.raises(ValueError, match='max_rows=0'):
        track_groups(COUNTS, 0)
    for bad in ([], [3, 0]):
        with pytest.raises(ValueError, match='at least one'):
            sequence_table(bad)
    with pytest.raises(ValueError, match='one slot below 2'):
        gather_table([0, 5], [2], [[0, 0, 1]])


@pytest.mark.parametrize('dtype,width', [(np.uint16, (512,)), (np.float32, (88,)), (np.float32, ())])
def test_gather_rows_host_is_plain_slicing(dtype, width):
    rng = np.random.default_rng(3)
    src = rng.integers(0, 60000, size=(3, 10) + width).astype(dtype)
    table = np.array([[2, 5, 7], [9, 1, 0], [0, 10, 12]])                                  # a middle run, one row, a whole clip
    dst = np.full((25,) + width, 7, dtype=dtype)
    assert gather_rows_host(dst, src, table) is dst
    want = np.full((25,) + width, 7, dtype=dtype)
    want[7:12], want[0:1], want[12:22] = src[0, 2:7], src[1, 9:10], src[2]
    assert np.array_equal(dst, want) and (dst[1:7] == 7).all() and (dst[22:] == 7).all()
    for row in ([0, 11, 0], [5, 6, 0], [0, 10, 16], [-1, 1, 0], [0, -1, 0], [0, 1, -1]):
        with pytest.raises(ValueError, match='clip 2'):
            gather_rows_host(dst, src, np.array([table[0], table[1], row]))
    assert np.array_equal(dst, want)                                                       # checked before anything is written
    with pytest.raises(ValueError):
        gather_rows_host(dst, src, table[:2])
    with pytest.raises(ValueError):
        gather_rows_host(dst.astype(np.float64), src, table)


class _Bank(object):
    frame_counts = np.array([118, 59, 40, 23])

    def __len__(self):
        return 4

    def clips(self, *a):
        raise AssertionError('nothing may be cut from the bank')


def _refusals(monkeypatch):
    launched = []
    monkeypatch.setattr(_lib, 'call', lambda name, *a, **k: launched.append(name))
    return launched


def test_exact_refuses_before_anything_is_launched(monkeypatch):
    from amt_tools_amd.models import OnsetsFrames, OnsetsFrames2, TabCNN
    launched = _refusals(monkeypatch)
    bank = _Bank()
    piano = OnsetsFrames(229, tools.PianoProfile(), 1, 2, device='cpu', precision='bf16').eval()
    piano2 = OnsetsFrames2(229, tools.PianoProfile(), 1, 2, device='cpu', precision='x3').eval()
    tab = TabCNN(192, tools.GuitarProfile(num_frets=19), 1, 1, device='cpu').eval()
    loops = (lambda model, margin, **k: inference.run_tracks(bank, model, 40, margin, exact=True, **k),
             lambda model, margin, **k: ev.validate_tracks(bank, None, None, model, ev.MultipitchEvaluator(), 40, margin, exact=True, **k))
    for loop in loops:
        with pytest.raises(ValueError, match='margin 4 is already exact'):
            loop(tab, 4)
    with pytest.raises(ValueError, match='margin 4 is already exact'):
        inference._exact_tracks(bank, tab, 40, 4)
    for model in (piano, piano2):
        for margin in (0, 2):
            with pytest.raises(ValueError, match=f'margin={margin}: the convolutions of Onsets & Frames reach 3 frames'):
                inference.run_tracks(bank, model, 40, margin, exact=True)
            with pytest.raises(ValueError, match='reach 3 frames'):
                inference._exact_tracks(bank, model, 40, margin)
        with pytest.raises(ValueError, match='has to be on a GPU'):                        # the check _stitch_tracks makes
            inference.run_tracks(bank, model, 40, 3, exact=True)
        with pytest.raises(ValueError, match='unknown track 9'):                           # seam_clips', for the whole request
            inference.run_tracks(bank, model, 40, 3, track_ids=[0, 9], exact=True)
        with pytest.raises(ValueError, match='num_frames=6 with margin=3'):
            inference.run_tracks(bank, model, 6, 3, exact=True)
    with pytest.raises(ValueError, match='eval mode'):
        inference.run_tracks(bank, OnsetsFrames(229, tools.PianoProfile(), 1, 2, device='cpu').train(), 40, 3, exact=True)
    with pytest.raises(ValueError, match='OnsetsFrames / OnsetsFrames2, not int'):
        inference._exact_tracks(bank, 5, 40, 3)
    assert launched == []


def test_an_unsupported_recurrence_names_the_model_complexity(monkeypatch):
    """AMTX_ERR_UNSUPPORTED of the language phase becomes NotImplementedError naming the model_complexity; nothing else is swallowed."""
    from amt_tools_amd.models import _OFEngine
    eng = _OFEngine.__new__(_OFEngine)
    eng.handle, eng.n_out, eng.model_complexity, eng.language_workspace = None, 88, 4, torch.empty(64, dtype=torch.uint8)

    def call(name, *a, **k):
        if name == 'amtx_of_language_workspace_bytes':
            return 64
        raise _lib.AmtxError(f'{name} failed ({code}): bilstm_seq: unsupported hidden size 384')
    monkeypatch.setattr(_lib, 'call', call)
    args = (torch.empty(4, dtype=torch.uint8), torch.empty((2, 88)), np.array([[0, 2]]), torch.tensor([[0, 2]]), 2, {})
    code = _lib.ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match='model_complexity=4'):
        eng.language_rows(*args)
    code = -1
    with pytest.raises(_lib.AmtxError, match='failed'):
        eng.language_rows(*args)


def test_exact_is_a_keyword_of_both_drivers_and_off_by_default():
    """run_tracks: the last keyword.  validate_tracks: directly in front of `losses`, which stays the last keyword of all three validation
    loops (tests/test_clip_loss.py holds that)."""
    assert [p.name for p in inspect.signature(inference.run_tracks).parameters.values()][-1] == 'exact'
    assert [p.name for p in inspect.signature(ev.validate_tracks).parameters.values()][-2:] == ['exact', 'losses']
    for loop in (inference.run_tracks, ev.validate_tracks):
        assert inspect.signature(loop).parameters['exact'].default is False
    assert inspect.signature(inference._exact_tracks).parameters['max_rows'].default == 1 << 18
    assert 'amtx_ofseq.h' in _lib.HEADERS and {'amtx_bilstm_seq_fwd', 'amtx_rows_gather', 'amtx_of_acoustic_rows', 'amtx_of_language_rows',
                                               'amtx_of_language_workspace_bytes'} <= set(_lib.header_signatures()['amtx_ofseq.h'])
