"""Per-clip loss sums (amt_tools_amd/cliploss.py, include/amtx_cliploss.h) without a GPU: the float64 restatement against the reference's
own output layers (tests/golden/clip_loss.npz, tools/gen_golden_clip_loss.py), frame windows, the C ABI's refusals, tools.KEY_LOSS_FRAMES
on CPU models, and what the three validation loops refuse before anything is launched."""
import numpy as np
import pytest
import torch

from amt_tools_amd import _lib, cliploss, evaluate as ev, tools
from amt_tools_amd.models import OnsetsFrames, OnsetsFrames2, TabCNN, TranscriptionModel
from amt_tools_amd.synth import synth_state_dict, synth_tabcnn_state_dict

from conftest import load_golden

ERR_ARG = -1
GUITAR = tools.GuitarProfile(num_frets=19)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the restatement against the reference
# ------------------------------------------------------------------------------------------------------------------------------
def _within(got, want, n_terms):
    """The reference sums n_terms non-negative float32 terms: a relative error of at most n_terms * 2^-23 whatever its order."""
    assert abs(got - float(want)) <= n_terms * 2.0 ** -23 * abs(float(want)), (got, float(want), n_terms)


@pytest.mark.parametrize('weighted', [False, True])
def test_bce_sums_over_frames_is_the_references_loss_of_a_batch_of_one(weighted):
    g = load_golden('clip_loss.npz')
    x, y = g['bce_logits'], g['bce_labels']
    assert x.shape == (1, 12, 88) and y.shape == (1, 88, 12) and x.dtype == y.dtype == np.float32
    sums = cliploss.bce_sums(x, y, g['bce_weight'] if weighted else None)
    assert isinstance(sums, np.ndarray) and sums.dtype == np.float64 and sums.shape == (1,)
    _within(sums[0] / 12, g['bce_loss_weighted' if weighted else 'bce_loss'], 12 * 88)
    assert g['bce_loss'] != g['bce_loss_weighted']
    as_tensor = cliploss.bce_sums(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(g['bce_weight']) if weighted else None)
    assert torch.is_tensor(as_tensor) and as_tensor.dtype == torch.float64 and as_tensor.numpy().tobytes() == sums.tobytes()


@pytest.mark.parametrize('weighted', [False, True])
def test_softmax_groups_sums_over_frames_is_the_references_loss_of_a_batch_of_one(weighted):
    g = load_golden('clip_loss.npz')
    x, t = g['sm_logits'], g['sm_targets']
    assert x.shape == (1, 9, 126) and t.shape == (1, 6, 9) and t.dtype == np.int64 and (t == -1).any() and (t == 20).any()
    sums = cliploss.softmax_groups_sums(x, t, 6, 21, g['sm_weight'] if weighted else None)
    assert sums.dtype == np.float64 and sums.shape == (1,)
    _within(sums[0] / 9, g['sm_loss_weighted' if weighted else 'sm_loss'], 9 * 6)
    # -1 is the last class; padded rows (the TabCNN engine's 128) change nothing
    padded = np.concatenate([x, np.full((1, 9, 2), 1e30, dtype=np.float32)], axis=-1)
    again = cliploss.softmax_groups_sums(padded, np.where(t == -1, 20, t), 6, 21, g['sm_weight'] if weighted else None)
    assert again.tobytes() == sums.tobytes()


def test_a_target_outside_the_classes_makes_its_clip_nan_inside_the_window_only():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 5, 8)).astype(np.float32)
    t = rng.integers(-1, 4, size=(2, 2, 5))
    t[1, 0, 4] = 4
    sums = cliploss.softmax_groups_sums(x, t, 2, 4)
    assert np.isfinite(sums[0]) and np.isnan(sums[1])
    assert np.isfinite(cliploss.softmax_groups_sums(x, t, 2, 4, frames=[[0, 5], [0, 4]])).all()


# ------------------------------------------------------------------------------------------------------------------------------
# 2. windows
# ------------------------------------------------------------------------------------------------------------------------------
WINDOWS = [[0, 40], [6, 28], [39, 1], [0, 0], [17, 23]]


def test_sums_over_a_window_equal_the_sums_of_the_sliced_arrays_exactly():
    rng = np.random.default_rng(11)
    x = (4 * rng.standard_normal((5, 40, 88))).astype(np.float32)
    y = (rng.random((5, 88, 40)) < 0.1).astype(np.float32)
    w = (rng.random(88) + 0.5).astype(np.float32)
    got = cliploss.bce_sums(x, y, w, WINDOWS)
    for b, (first, count) in enumerate(WINDOWS):
        want = cliploss.bce_sums(x[b:b + 1, first:first + count], y[b:b + 1, :, first:first + count], w)[0] if count else 0.0
        assert got[b] == want and (got[b] > 0) == (count > 0), (b, got[b], want)
    assert got[3] == 0.0 and got[0] == cliploss.bce_sums(x, y, w)[0]
    lg = (4 * rng.standard_normal((5, 40, 128))).astype(np.float32)
    tg = rng.integers(-1, 21, size=(5, 6, 40))
    ww = (rng.random(126) + 0.5).astype(np.float32)
    for frames in (WINDOWS, np.array(WINDOWS, dtype=np.int32), torch.tensor(WINDOWS), cliploss.Windows(WINDOWS)):
        got = cliploss.softmax_groups_sums(lg, tg, 6, 21, ww, frames)
        for b, (first, count) in enumerate(WINDOWS):
            want = cliploss.softmax_groups_sums(lg[b:b + 1, first:first + count], tg[b:b + 1, :, first:first + count], 6, 21, ww)[0] if count else 0.0
            assert got[b] == want, (b, got[b], want)
    assert got[3] == 0.0


def test_window_tables_are_checked_on_the_host_and_the_error_names_the_clip():
    x, y = np.zeros((3, 8, 4), dtype=np.float32), np.zeros((3, 4, 8), dtype=np.float32)
    with pytest.raises(ValueError, match='clip 1: a negative entry'):
        cliploss.bce_sums(x, y, frames=[[0, 8], [-1, 2], [0, 0]])
    with pytest.raises(ValueError, match='clip 2: frames .3, 3 . 6. leave the clip\'s 8 frames'):
        cliploss.bce_sums(x, y, frames=[[0, 8], [1, 2], [3, 6]])
    with pytest.raises(ValueError, match=r'a \(3, 2\) table'):
        cliploss.bce_sums(x, y, frames=[[0, 8], [1, 2]])
    with pytest.raises(ValueError, match='integer table'):
        cliploss.bce_sums(x, y, frames=np.zeros((3, 2)))
    with pytest.raises(ValueError, match='labels'):
        cliploss.bce_sums(x, y.transpose(0, 2, 1))
    t = np.zeros((3, 2, 8), dtype=np.int64)
    with pytest.raises(ValueError, match='clip 0: frames'):
        cliploss.softmax_groups_sums(x, t, 2, 2, frames=[[8, 1], [0, 0], [0, 0]])
    with pytest.raises(ValueError, match='targets'):
        cliploss.softmax_groups_sums(x, t, 2, 3)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
def test_clip_loss_abi_refuses_bad_arguments_with_nothing_launched():
    L = _lib.lib()
    assert 'amtx_cliploss.h' in _lib.HEADERS and set(_lib.header_signatures()['amtx_cliploss.h']) == {
        'amtx_bce_clip_sums_workspace_bytes', 'amtx_bce_clip_sums', 'amtx_softmax_groups_clip_sums_workspace_bytes', 'amtx_softmax_groups_clip_sums'}
    buf, tg, sums = np.zeros(4096, dtype=np.float32), np.zeros(256, dtype=np.int64), np.zeros(4, dtype=np.float64)
    p, t, s = _lib.ptr(buf), _lib.ptr(tg), _lib.ptr(sums)
    good = np.array([[0, 8], [3, 5]], dtype=np.int32)
    g = _lib.ptr(good)
    need = int(L.amtx_bce_clip_sums_workspace_bytes(2, 8, 88))
    assert need == 2 * 1 * 3 * 8 and L.amtx_bce_clip_sums_workspace_bytes(0, 8, 88) == 0 and L.amtx_bce_clip_sums_workspace_bytes(2, 8, 0) == 0
    assert L.amtx_bce_clip_sums_workspace_bytes(2, 33, 88) == 2 * 2 * 3 * 8
    # null pointers
    assert L.amtx_bce_clip_sums(None, 88, p, None, None, None, 2, 8, 88, s, p, need, None) == ERR_ARG
    assert b'null' in L.amtx_last_error()
    assert L.amtx_bce_clip_sums(p, 88, None, None, None, None, 2, 8, 88, s, p, need, None) == ERR_ARG
    assert L.amtx_bce_clip_sums(p, 88, p, None, None, None, 2, 8, 88, None, p, need, None) == ERR_ARG
    assert L.amtx_bce_clip_sums(p, 88, p, None, None, None, 2, 8, 88, s, None, need, None) == ERR_ARG
    # ld < keys
    assert L.amtx_bce_clip_sums(p, 87, p, None, None, None, 2, 8, 88, s, p, need, None) == ERR_ARG
    assert b'ld' in L.amtx_last_error()
    # a bad row of the host table: the clip is named
    for row, text in (([3, 6], b'clip 1: frames [3, 3 + 6) leave the clip\'s 8 frames'), ([-1, 2], b'clip 1: a negative entry'), ([2, -2], b'clip 1: a negative entry'),
                      ([2147483647, 2147483647], b'clip 1: frames')):
        bad = np.array([[0, 8], row], dtype=np.int32)
        assert L.amtx_bce_clip_sums(p, 88, p, None, _lib.ptr(bad), g, 2, 8, 88, s, p, need, None) == ERR_ARG
        assert text in L.amtx_last_error(), L.amtx_last_error()
    # one table of the two
    assert L.amtx_bce_clip_sums(p, 88, p, None, g, None, 2, 8, 88, s, p, need, None) == ERR_ARG
    assert b'twice' in L.amtx_last_error()
    assert L.amtx_bce_clip_sums(p, 88, p, None, None, g, 2, 8, 88, s, p, need, None) == ERR_ARG
    # a workspace one byte short, batch == 0, misaligned sums
    assert L.amtx_bce_clip_sums(p, 88, p, None, None, None, 2, 8, 88, s, p, need - 1, None) == ERR_ARG
    assert b'workspace' in L.amtx_last_error()
    assert L.amtx_bce_clip_sums(p, 88, p, None, None, None, 0, 8, 88, s, p, need, None) == ERR_ARG
    assert L.amtx_bce_clip_sums(p, 88, p, None, None, None, 2, 0, 88, s, p, need, None) == ERR_ARG
    assert L.amtx_bce_clip_sums(p, 88, p, None, None, None, 2, 8, 88, _lib.ptr(buf[1:]), p, need, None) == ERR_ARG
    assert b'aligned' in L.amtx_last_error()
    # the grouped softmax
    need = int(L.amtx_softmax_groups_clip_sums_workspace_bytes(2, 8, 6, 21))
    assert need == 2 * 1 * 8 and L.amtx_softmax_groups_clip_sums_workspace_bytes(2, 33, 6, 21) == 2 * 2 * 8
    assert L.amtx_softmax_groups_clip_sums_workspace_bytes(2, 8, 6, 0) == 0 and L.amtx_softmax_groups_clip_sums_workspace_bytes(0, 8, 6, 21) == 0
    assert L.amtx_softmax_groups_clip_sums(None, 126, t, None, None, None, 2, 8, 6, 21, s, p, need, None) == ERR_ARG
    assert L.amtx_softmax_groups_clip_sums(p, 126, None, None, None, None, 2, 8, 6, 21, s, p, need, None) == ERR_ARG
    assert L.amtx_softmax_groups_clip_sums(p, 126, t, None, None, None, 2, 8, 6, 21, None, p, need, None) == ERR_ARG
    assert L.amtx_softmax_groups_clip_sums(p, 126, t, None, None, None, 2, 8, 6, 21, s, None, need, None) == ERR_ARG
    assert L.amtx_softmax_groups_clip_sums(p, 125, t, None, None, None, 2, 8, 6, 21, s, p, need, None) == ERR_ARG
    assert b'ld' in L.amtx_last_error()
    bad = np.array([[0, 8], [8, 1]], dtype=np.int32)
    assert L.amtx_softmax_groups_clip_sums(p, 126, t, None, _lib.ptr(bad), g, 2, 8, 6, 21, s, p, need, None) == ERR_ARG
    assert b'clip 1' in L.amtx_last_error()
    assert L.amtx_softmax_groups_clip_sums(p, 126, t, None, g, None, 2, 8, 6, 21, s, p, need, None) == ERR_ARG
    assert L.amtx_softmax_groups_clip_sums(p, 126, t, None, None, None, 2, 8, 6, 21, s, p, need - 1, None) == ERR_ARG
    assert L.amtx_softmax_groups_clip_sums(p, 126, t, None, None, None, 0, 8, 6, 21, s, p, need, None) == ERR_ARG
    assert L.amtx_softmax_groups_clip_sums(p, 126, t, None, None, None, 2, 8, 0, 21, s, p, need, None) == ERR_ARG
    assert L.amtx_softmax_groups_clip_sums(p, 1 << 20, t, None, None, None, 2, 8, 8193, 1, s, p, 1 << 20, None) == _lib.ERR_UNSUPPORTED
    assert not sums.any() and not buf.any()


# ------------------------------------------------------------------------------------------------------------------------------
# 4. CPU models
# ------------------------------------------------------------------------------------------------------------------------------
def _tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _piano_model(cls=OnsetsFrames, mc=2):
    model = cls(40, tools.PianoProfile(), 1, mc)
    model.load_state_dict(_tensors(synth_state_dict(2, dim_in=40, in_channels=1, model_complexity=mc, offsets=cls is OnsetsFrames2)))
    model.eval()
    return model


def _piano_batch(B, T, keys):
    rng = np.random.default_rng(B * T)
    batch = {tools.KEY_FEATS: torch.from_numpy(rng.random((B, 1, 40, T)).astype(np.float32))}
    for key, p in zip(keys, (0.08, 0.03, 0.03)):
        batch[key] = torch.from_numpy((rng.random((B, 88, T)) < p).astype(np.float32))
    return batch


def _close(a, b, rel):
    assert abs(float(a) - float(b)) <= rel * abs(float(b)), (float(a), float(b))


@pytest.mark.parametrize('cls,keys', [(OnsetsFrames, (tools.KEY_MULTIPITCH, tools.KEY_ONSETS)), (OnsetsFrames, (tools.KEY_MULTIPITCH,)),
                                      (OnsetsFrames2, (tools.KEY_MULTIPITCH, tools.KEY_ONSETS, tools.KEY_OFFSETS)), (OnsetsFrames2, (tools.KEY_MULTIPITCH,))])
def test_a_cpu_onsets_and_frames_model_returns_per_clip_sums_under_the_key(cls, keys):
    B, T = 3, 21
    model = _piano_model(cls)
    assert cls.loss_label_keys == (tools.KEY_MULTIPITCH, tools.KEY_ONSETS) + ((tools.KEY_OFFSETS,) if cls is OnsetsFrames2 else ())
    batch = _piano_batch(B, T, keys)
    with torch.no_grad():
        today = model.run_on_batch(batch)
        got = model.run_on_batch(dict(batch, **{tools.KEY_LOSS_FRAMES: None}))
    assert list(got) == list(today) and list(got[tools.KEY_LOSS]) == list(today[tools.KEY_LOSS])
    for key, sums in got[tools.KEY_LOSS].items():
        assert torch.is_tensor(sums) and sums.dtype == torch.float64 and tuple(sums.shape) == (B,), key
        _close((sums / T).mean(), today[tools.KEY_LOSS][key], 1e-5)
    others = [v for k, v in got[tools.KEY_LOSS].items() if k != tools.KEY_LOSS_TOTAL]
    assert len(others) == len(cls.loss_label_keys) and torch.allclose(got[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL], sum(others), rtol=1e-14, atol=0)
    for key in (tools.KEY_ONSETS, tools.KEY_MULTIPITCH):
        assert torch.equal(got[key], today[key])
    # a window per clip: the sums of the sliced logits; the table may be a tensor, and survives a float32 round trip with the audio
    frames = np.array([[0, T], [4, 9], [T - 1, 1]])
    with torch.no_grad():
        windowed = model.run_on_batch(dict(batch, **{tools.KEY_LOSS_FRAMES: frames}))[tools.KEY_LOSS]
        for table in (torch.from_numpy(frames), frames.astype(np.float32)):
            again = model.run_on_batch(dict(batch, **{tools.KEY_LOSS_FRAMES: table}))[tools.KEY_LOSS]
            assert all(torch.equal(again[k], windowed[k]) for k in windowed)
    assert all(windowed[k][0] == got[tools.KEY_LOSS][k][0] for k in windowed)
    assert all(0 < windowed[k][2] < windowed[k][1] < got[tools.KEY_LOSS][k][1] for k in windowed)
    # training mode: no gradient goes through the sums
    model.train()
    with pytest.raises(ValueError, match='eval mode only'):
        model.run_on_batch(dict(batch, **{tools.KEY_LOSS_FRAMES: None}))
    model.eval()
    # an unlabelled batch has no loss, with or without the key
    with torch.no_grad():
        assert tools.KEY_LOSS not in model.run_on_batch({tools.KEY_FEATS: batch[tools.KEY_FEATS], tools.KEY_LOSS_FRAMES: None})


@pytest.mark.parametrize('weighted', [False, True])
def test_a_cpu_tabcnn_returns_per_clip_sums_under_the_key(weighted):
    B, T = 3, 11
    model = TabCNN(40, GUITAR, 1, 1)
    model.load_state_dict(_tensors(synth_tabcnn_state_dict(5, dim_in=40, in_channels=1, model_complexity=1, num_groups=6, num_classes=21)))
    model.eval()
    assert TabCNN.loss_label_keys == (tools.KEY_TABLATURE,) and TranscriptionModel.loss_label_keys is None
    rng = np.random.default_rng(9)
    if weighted:
        model.dense[-1].set_weights(rng.random(126) + 0.5)
    batch = {tools.KEY_FEATS: torch.from_numpy(rng.random((B, 1, 40, T)).astype(np.float32)),
             tools.KEY_TABLATURE: torch.from_numpy(rng.integers(-1, 20, size=(B, 6, T)))}
    with torch.no_grad():
        today = model.run_on_batch(batch)
        got = model.run_on_batch(dict(batch, **{tools.KEY_LOSS_FRAMES: None}))
        half = model.run_on_batch(dict(batch, **{tools.KEY_LOSS_FRAMES: [[0, 5], [5, 6], [0, 0]]}))[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL]
    assert list(got[tools.KEY_LOSS]) == [tools.KEY_LOSS_TOTAL] and torch.equal(got[tools.KEY_TABLATURE], today[tools.KEY_TABLATURE])
    sums = got[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL]
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (B,)
    _close((sums / T).mean(), today[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL], 1e-5)
    assert 0 < half[0] < sums[0] and 0 < half[1] < sums[1] and half[2] == 0
    model.train()
    with pytest.raises(ValueError, match='eval mode only'):
        model.run_on_batch(dict(batch, **{tools.KEY_LOSS_FRAMES: None}))


def test_a_model_without_a_per_clip_loss_refuses_the_key():
    class Plain(TranscriptionModel):
        pass
    with pytest.raises(ValueError, match='Plain has no per-clip loss'):
        Plain(4, tools.PianoProfile()).eval().run_on_batch({tools.KEY_FEATS: torch.zeros(1, 1, 4, 3), tools.KEY_LOSS_FRAMES: None})


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the loops' refusals: before anything is launched (a CPU model and stand-ins for the banks)
# ------------------------------------------------------------------------------------------------------------------------------
class _Bank(object):
    """Three tracks; nothing of it is ever read on a device."""
    frame_counts = np.array([50, 60, 70])

    def __len__(self):
        return 3


class _Labels(_Bank):
    def __init__(self, *keys):
        self.keys = tuple(keys)


def test_the_three_loops_refuse_losses_before_anything_is_launched():
    model = _piano_model()
    bank = _Bank()
    combo = lambda: ev.ComboEvaluator([ev.MultipitchEvaluator(), ev.LossWrapper()])      # noqa: E731
    both = _Labels(tools.KEY_MULTIPITCH, tools.KEY_ONSETS)
    clips, refs = np.zeros((2, 1, 40, 8), dtype=np.float32), [{tools.KEY_MULTIPITCH: np.zeros((88, 8), dtype=np.float32)}] * 2

    def loops(evaluator, labels, m=model):
        return [lambda: ev.validate_batched(clips, refs, m, evaluator, losses=True),
                lambda: ev.validate_clips(bank, labels, None, m, evaluator, [0], [0], 8, losses=True),
                lambda: ev.validate_tracks(bank, labels, None, m, evaluator, 40, 6, losses=True)]

    # no LossWrapper among the evaluators
    for run in loops(ev.MultipitchEvaluator(), both) + loops(ev.ComboEvaluator([ev.MultipitchEvaluator()]), both):
        with pytest.raises(ValueError, match='losses=True scores the loss through a LossWrapper'):
            run()
    # a model without per-clip losses
    plain = _piano_model()
    plain.loss_label_keys = None
    for run in loops(combo(), both, plain):
        with pytest.raises(ValueError, match='OnsetsFrames has none'):
            run()
    # the bank loops: no LabelBank, a LabelBank that lacks one of the model's keys -- the error names it
    for run in loops(ev.LossWrapper(), None)[1:]:
        with pytest.raises(ValueError, match='losses=True needs a LabelBank'):
            run()
    for run in loops(combo(), _Labels(tools.KEY_MULTIPITCH))[1:]:
        with pytest.raises(ValueError, match=f'needs the label map \'{tools.KEY_ONSETS}\''):
            run()
    for run in loops(ev.LossWrapper(), _Labels(tools.KEY_ONSETS))[1:]:
        with pytest.raises(ValueError, match=f'needs the label map \'{tools.KEY_MULTIPITCH}\''):
            run()
    of2 = _piano_model(OnsetsFrames2)
    for run in loops(combo(), both, of2)[1:]:
        with pytest.raises(ValueError, match=f'needs the label map \'{tools.KEY_OFFSETS}\''):
            run()
    # validate_batched: a reference without the map that makes a batch labelled; the device loop only
    with pytest.raises(ValueError, match='the reference of clip 1 has none'):
        ev.validate_batched(clips, [refs[0], {tools.KEY_ONSETS: refs[0][tools.KEY_MULTIPITCH]}], model, combo(), losses=True)
    with pytest.raises(ValueError, match='the model has to be on a GPU'):
        ev.validate_batched(clips, refs, model, combo(), losses=True)
    # and the keyword is the last one of each loop, off by default
    import inspect
    for loop in (ev.validate_batched, ev.validate_clips, ev.validate_tracks):
        last = list(inspect.signature(loop).parameters.values())[-1]
        assert last.name == 'losses' and last.default is False
