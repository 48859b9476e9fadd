"""Per-clip loss sums on the device: amtx_bce_clip_sums / amtx_softmax_groups_clip_sums (include/amtx_cliploss.h, csrc/cliploss.hip) against
the float64 restatement of amt_tools_amd/cliploss.py, into poisoned memory; tools.KEY_LOSS_FRAMES on the GPU engines of OnsetsFrames,
OnsetsFrames2 and TabCNN; and losses=True in evaluate.validate_clips, validate_tracks and validate_batched.

TOLERANCE of a kernel sum against the restatement: 2e-6 * |ref| + 1e-7 * count, the project's tolerance for the same float32 arithmetic
(tests/test_gpu_train.py, BCE loss against torch), whose absolute term there is for a MEAN over frames and so scales with the number of
frames `count` a sum runs over."""
import contextlib
import functools
import warnings

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from amt_tools_amd import _lib, autograd, cliploss, evaluate as ev, tools               # noqa: E402
from amt_tools_amd.synth import synth_state_dict                                        # noqa: E402
from amt_tools_amd.tracks import LabelBank, seam_clips                                  # noqa: E402
from poison import PATTERNS, fill_storage                                               # noqa: E402
from test_gpu_run_tracks import DEV, GUITAR, MARGIN, T, piano_setup, tab_setup          # noqa: E402

REAL = {'bce_sums': cliploss.bce_sums, 'softmax_groups_sums': cliploss.softmax_groups_sums}      # the restatement is reached past any spy
GUARD = 32                                   # float64 elements in front of and behind `sums`; as many bytes x 8 behind the workspace


def close(got, ref, count, what=''):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bound = 2e-6 * np.abs(ref) + 1e-7 * np.asarray(count, dtype=np.float64)
    assert got.shape == ref.shape and (np.abs(got - ref) <= bound).all(), (what, got, ref, np.abs(got - ref), bound)


def counts_of(frames, B, T_):
    return np.full(B, T_) if frames is None else np.asarray(frames)[:, 1]


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the kernels
# ------------------------------------------------------------------------------------------------------------------------------
def launch(name, x, ld, labels, w, frames, sizes, pattern):
    """The entry point itself, `sums` between guard bands and the workspace in front of one, everything filled with `pattern` first."""
    B = sizes[0]
    arena = fill_storage(torch.empty(B + 2 * GUARD, dtype=torch.float64, device=DEV), pattern)
    need = int(_lib.call(name + '_workspace_bytes', *sizes))
    assert need > 0 and need % 8 == 0
    ws = fill_storage(torch.empty(need + 8 * GUARD, dtype=torch.uint8, device=DEV), pattern)
    table = None if frames is None else np.ascontiguousarray(frames, dtype=np.int32)
    table_dev = None if frames is None else torch.from_numpy(table).to(DEV)
    _lib.call(name, x, ld, labels, w, table, table_dev, *sizes, arena[GUARD:GUARD + B], ws, need, device=DEV)
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    around = np.concatenate([host[:GUARD], host[GUARD + B:]]).view(np.uint8)
    assert (around == pattern).all() and (ws[need:].cpu().numpy() == pattern).all(), (name, sizes, pattern)
    return host[GUARD:GUARD + B].copy()


def across_patterns(name, x, ld, labels, w, frames, sizes):
    runs = [launch(name, x, ld, labels, w, frames, sizes, pattern) for pattern in PATTERNS + PATTERNS[:1]]
    for other in runs[1:]:
        assert other.tobytes() == runs[0].tobytes(), (name, sizes, runs[0], other)        # the pattern does not matter; a second call: same bits
    return runs[0]


BCE_WINDOWS = [[0, 40], [6, 28], [39, 1], [0, 0], [17, 23]]
SM_WINDOWS = [[0, 37], [6, 25], [36, 1], [0, 0], [15, 22]]


@pytest.mark.parametrize('B,T_,K,ld,weighted,frames', [(1, 1, 4, 4, False, None), (3, 70, 88, 88, True, None), (2, 33, 120, 128, True, None),
                                                      (5, 40, 88, 88, False, BCE_WINDOWS)])
def test_bce_clip_sums_equal_the_float64_restatement(B, T_, K, ld, weighted, frames):
    g = torch.Generator().manual_seed(B * 1000 + T_)
    full = (torch.randn(B, T_, ld, generator=g) * 4).to(DEV)
    x = full[:, :, :K]
    y = (torch.rand(B, K, T_, generator=g) < 0.1).float().to(DEV)
    w = (torch.rand(K, generator=g) + 0.5).to(DEV) if weighted else None
    ref = cliploss.bce_sums(x.cpu().numpy(), y.cpu().numpy(), None if w is None else w.cpu().numpy(), frames)
    got = across_patterns('amtx_bce_clip_sums', full, ld, y, w, frames, (B, T_, K))
    close(got, ref, counts_of(frames, B, T_), ('bce', B, T_, K, ld))
    assert (ref > 0).sum() == (B if frames is None else B - 1)
    if frames is not None:
        assert got[3] == 0.0
    public = cliploss.bce_sums(x, y, w, frames)
    assert public.dtype == torch.float64 and public.device == x.device and public.cpu().numpy().tobytes() == got.tobytes()


@pytest.mark.parametrize('B,T_,G,Cn,ld,weighted,frames', [(1, 1, 1, 2, 2, False, None), (2, 8, 6, 21, 126, False, None), (5, 37, 6, 21, 128, True, SM_WINDOWS)])
def test_softmax_groups_clip_sums_equal_the_float64_restatement(B, T_, G, Cn, ld, weighted, frames):
    g = torch.Generator().manual_seed(B * 1000 + T_)
    full = (torch.randn(B, T_, ld, generator=g) * 4).to(DEV)
    y = torch.randint(-1, Cn, (B, G, T_), generator=g).to(DEV)
    assert Cn == 2 or ((y == -1).any() and (y == Cn - 1).any())
    w = (torch.rand(G * Cn, generator=g) + 0.5).to(DEV) if weighted else None
    ref = cliploss.softmax_groups_sums(full.cpu().numpy(), y.cpu().numpy(), G, Cn, None if w is None else w.cpu().numpy(), frames)
    got = across_patterns('amtx_softmax_groups_clip_sums', full, ld, y, w, frames, (B, T_, G, Cn))
    close(got, ref, counts_of(frames, B, T_), ('softmax', B, T_, G, Cn, ld))
    if frames is not None:
        assert got[3] == 0.0 and (got[[0, 1, 2, 4]] > 0).all()
    public = cliploss.softmax_groups_sums(full, y, G, Cn, w, frames)
    assert public.cpu().numpy().tobytes() == got.tobytes()


def test_a_target_outside_the_classes_is_nan_for_its_clip_inside_its_window():
    x = torch.randn(2, 5, 8, device=DEV)
    y = torch.randint(-1, 4, (2, 2, 5)).to(DEV)
    y[1, 0, 4] = 4
    sums = cliploss.softmax_groups_sums(x, y, 2, 4).cpu().numpy()
    assert np.isfinite(sums[0]) and np.isnan(sums[1])
    assert np.isfinite(cliploss.softmax_groups_sums(x, y, 2, 4, frames=[[0, 5], [0, 4]]).cpu().numpy()).all()


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the models
# ------------------------------------------------------------------------------------------------------------------------------
def spy(monkeypatch, module, name):
    """tests/test_gpu_evaluate.py's spy, keeping the arguments too: [(args, result)] of every call of module.name."""
    real, seen = getattr(module, name), []

    def wrapper(*args, **kwargs):
        assert not kwargs
        seen.append((args, real(*args)))
        return seen[-1][1]
    monkeypatch.setattr(module, name, wrapper)
    return seen


def table_of(frames):
    return frames.table if isinstance(frames, cliploss.Windows) else frames


def host_again(name, args):
    """The float64 restatement on the arguments a device call was recorded with."""
    host = [a.detach().cpu().numpy() if torch.is_tensor(a) else a for a in args]
    host[-1] = table_of(host[-1])
    return REAL[name](*host)


def check_calls(name, seen):
    """Every recorded device call agrees with the restatement on its own arguments."""
    for args, result in seen:
        logits = args[0]
        assert logits.is_cuda and result.is_cuda and result.dtype == torch.float64
        close(result.cpu().numpy(), host_again(name, args), counts_of(table_of(args[-1]), logits.shape[0], logits.shape[1]), name)


@functools.lru_cache(maxsize=None)
def of2_setup():
    """OnsetsFrames2 at the smallest complexity its engine takes, on piano_setup's tracks."""
    from amt_tools_amd.models import OnsetsFrames2
    model, bank = piano_setup()
    of2 = OnsetsFrames2(229, tools.PianoProfile(), 1, 2, device=DEV, precision='bf16')
    of2.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth_state_dict(1, dim_in=229, in_channels=1, model_complexity=2, offsets=True).items()})
    of2.frontend = model.frontend
    of2.change_device()
    of2.eval()
    return of2, bank


@functools.lru_cache(maxsize=None)
def piano_labels():
    """Random label maps of piano_setup's tracks under all three keys."""
    rng = np.random.default_rng(77)
    _, bank = piano_setup()
    maps = [{key: (rng.random((88, n)) < p).astype(np.float32) for key, p in ((tools.KEY_MULTIPITCH, 0.08), (tools.KEY_ONSETS, 0.03), (tools.KEY_OFFSETS, 0.03))}
            for n in bank.frame_counts.tolist()]
    return LabelBank(maps, bank=bank)


@functools.lru_cache(maxsize=None)
def tab_labels():
    rng = np.random.default_rng(78)
    _, bank = tab_setup()
    return LabelBank([{tools.KEY_TABLATURE: rng.integers(-1, 20, size=(6, n))} for n in bank.frame_counts.tolist()], bank=bank)


REQUEST = ([0, 0, 1, 2, 0], [0, 30, 19, 0, 78])
FRAMES = np.array([[0, 40], [6, 28], [39, 1], [0, 0], [17, 23]])


@pytest.mark.parametrize('which', ['OnsetsFrames', 'OnsetsFrames2', 'TabCNN'])
def test_models_return_per_clip_sums_from_the_engines_logits(monkeypatch, which):
    model, bank = {'OnsetsFrames': piano_setup, 'OnsetsFrames2': of2_setup, 'TabCNN': tab_setup}[which]()
    labels = tab_labels() if which == 'TabCNN' else piano_labels()
    bce, sm = spy(monkeypatch, cliploss, 'bce_sums'), spy(monkeypatch, cliploss, 'softmax_groups_sums')
    fallbacks = autograd.fallback_total()
    truth = {k: v for k, v in labels.clips(*REQUEST, T).items() if k in model.loss_label_keys}
    assert sorted(truth) == sorted(model.loss_label_keys)
    batch = dict(truth, **{tools.KEY_AUDIO: bank.clips(*REQUEST, T)})
    with torch.no_grad():
        today = model.run_on_batch(batch)
        assert not bce and not sm
        got = model.run_on_batch(dict(batch, **{tools.KEY_LOSS_FRAMES: None}))
        windowed = model.run_on_batch(dict(batch, **{tools.KEY_LOSS_FRAMES: FRAMES}))
    seen, name = (sm, 'softmax_groups_sums') if which == 'TabCNN' else (bce, 'bce_sums')
    heads = len(model.loss_label_keys)
    assert len(seen) == 2 * heads and not (bce if which == 'TabCNN' else sm)
    check_calls(name, seen)
    # the right labels for the right heads, the batch's own tensors; the windows as given
    head_keys = {'OnsetsFrames': (tools.KEY_MULTIPITCH, tools.KEY_ONSETS), 'OnsetsFrames2': (tools.KEY_MULTIPITCH, tools.KEY_ONSETS, tools.KEY_OFFSETS),
                 'TabCNN': (tools.KEY_TABLATURE,)}[which]
    loss_keys = {'OnsetsFrames': (tools.KEY_LOSS_PITCH, tools.KEY_LOSS_ONSETS), 'OnsetsFrames2': (tools.KEY_LOSS_PITCH, tools.KEY_LOSS_ONSETS, tools.KEY_LOSS_OFFSETS),
                 'TabCNN': (tools.KEY_LOSS_TOTAL,)}[which]
    for run, (out, frames) in enumerate(((got, None), (windowed, FRAMES))):
        assert list(out) == list(today) and list(out[tools.KEY_LOSS]) == list(today[tools.KEY_LOSS])
        for h, (label_key, loss_key) in enumerate(zip(head_keys, loss_keys)):
            args, result = seen[run * heads + h]
            assert args[1] is batch[label_key] and (args[-1] is None if frames is None else np.array_equal(table_of(args[-1]), frames))
            assert out[tools.KEY_LOSS][loss_key] is result and tuple(result.shape) == (5,)
        total = sum(out[tools.KEY_LOSS][k] for k in loss_keys)
        assert torch.equal(out[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL], total)
        for key in today:
            if key != tools.KEY_LOSS:
                assert torch.equal(out[key], today[key]), key
    # the mean over clips of sums / T is today's batch mean: float32 evaluation and a float32 mean over a few hundred terms lie well inside
    # 1e-5 relative, a wrong head pairing or a dropped clip far outside it
    for key, sums in got[tools.KEY_LOSS].items():
        mean, want = float((sums / T).mean()), float(today[tools.KEY_LOSS][key])
        assert want > 0 and abs(mean - want) <= 1e-5 * want, (key, mean, want)
    assert float(windowed[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL][3]) == 0.0
    assert autograd.fallback_total() == fallbacks
    model.train()
    try:
        with pytest.raises(ValueError, match='eval mode only'):
            model.run_on_batch(dict(batch, **{tools.KEY_LOSS_FRAMES: None}))
    finally:
        model.eval()


# ------------------------------------------------------------------------------------------------------------------------------
# 3. validate_clips
# ------------------------------------------------------------------------------------------------------------------------------
def per_head(seen, heads):
    """Recorded results per head, every head's batches joined in call order: [(sums (clips,), frames table or None per call)]."""
    return [np.concatenate([r.cpu().numpy() for _, r in seen[h::heads]]) for h in range(heads)]


@contextlib.contextmanager
def no_warnings():
    """A RuntimeWarning inside is an error: the LossWrapper's 'not found in estimates' among them."""
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        yield


CLIPS = ([0, 0, 0, 1, 2], [0, 39, 78, 19, 0])


@pytest.mark.parametrize('batch_size', [2, 256])
@pytest.mark.parametrize('which', ['OnsetsFrames', 'TabCNN'])
def test_validate_clips_tracks_every_clips_loss(monkeypatch, which, batch_size):
    model, bank = (tab_setup if which == 'TabCNN' else piano_setup)()
    labels = tab_labels() if which == 'TabCNN' else piano_labels()
    others = (lambda: [ev.TablatureEvaluator(GUITAR), ev.SoftmaxAccuracy(results_key='accuracy')]) if which == 'TabCNN' else \
        (lambda: [ev.MultipitchEvaluator(), ev.MultipitchEvaluator(unpack_key=tools.KEY_ONSETS, results_key='onsets')])
    seen = spy(monkeypatch, cliploss, 'softmax_groups_sums' if which == 'TabCNN' else 'bce_sums')
    plain = ev.ComboEvaluator(others())
    ev.validate_clips(bank, labels, None, model, plain, *CLIPS, T, batch_size=batch_size)
    assert not seen
    loss = ev.LossWrapper()
    combo = ev.ComboEvaluator([loss] + others())
    with no_warnings():
        average = ev.validate_clips(bank, labels, None, model, combo, *CLIPS, T, batch_size=batch_size, losses=True)
    loss_keys = (tools.KEY_LOSS_TOTAL,) if which == 'TabCNN' else (tools.KEY_LOSS_PITCH, tools.KEY_LOSS_ONSETS)
    heads = len(loss_keys)
    assert len(seen) == heads * -(-5 // batch_size) and all(args[-1] is None for args, _ in seen)
    check_calls('softmax_groups_sums' if which == 'TabCNN' else 'bce_sums', seen)
    sums = per_head(seen, heads)
    assert list(loss.results) == list(loss_keys) + ([tools.KEY_LOSS_TOTAL] if heads > 1 else [])
    for key, s in zip(loss_keys, sums):
        assert np.array_equal(np.asarray(loss.results[key]), s / T) and s.shape == (5,) and (s > 0).all(), key
    assert np.allclose(np.asarray(loss.results[tools.KEY_LOSS_TOTAL]), sum(sums) / T, rtol=1e-15, atol=0)
    assert average[tools.KEY_LOSS] == {k: float(np.mean(v)) for k, v in loss.results.items()}
    for got_e, want_e in zip(combo.evaluators[1:], plain.evaluators):
        assert list(got_e.results) == list(want_e.results)
        for k in want_e.results:
            assert np.array_equal(np.asarray(got_e.results[k]), np.asarray(want_e.results[k])) and len(got_e.results[k]) == 5, k


# ------------------------------------------------------------------------------------------------------------------------------
# 4. validate_tracks
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch_size', [3, 256])
@pytest.mark.parametrize('which', ['OnsetsFrames', 'TabCNN'])
def test_validate_tracks_adds_the_kept_frames_sums_up_per_track(monkeypatch, which, batch_size):
    model, bank = (tab_setup if which == 'TabCNN' else piano_setup)()
    labels = tab_labels() if which == 'TabCNN' else piano_labels()
    name = 'softmax_groups_sums' if which == 'TabCNN' else 'bce_sums'
    loss_keys = (tools.KEY_LOSS_TOTAL,) if which == 'TabCNN' else (tools.KEY_LOSS_PITCH, tools.KEY_LOSS_ONSETS)
    heads = len(loss_keys)
    counts = bank.frame_counts.tolist()
    assert counts == ([118, 59, 40, 34] if which == 'TabCNN' else [118, 59, 40, 23])
    plan = seam_clips(bank.frame_counts, T, MARGIN)
    assert plan.track_ids.tolist() == [0, 0, 0, 0, 1, 1, 2] and plan.short.tolist() == [3]
    other = (lambda: ev.TablatureEvaluator(GUITAR)) if which == 'TabCNN' else (lambda: ev.MultipitchEvaluator())
    plain = other()
    ev.validate_tracks(bank, labels, None, model, plain, T, MARGIN, batch_size=batch_size)
    # tracks 2 and 3 whole, as one clip each
    whole = {}
    with torch.no_grad():
        for t in (2, 3):
            truth = {k: v for k, v in labels.clips([t], [0], counts[t]).items() if k in model.loss_label_keys}
            out = model.run_on_batch(dict(truth, **{tools.KEY_AUDIO: bank.clips([t], [0], counts[t]), tools.KEY_LOSS_FRAMES: None}))
            whole[t] = {k: float(v[0]) / counts[t] for k, v in out[tools.KEY_LOSS].items()}
    seen = spy(monkeypatch, cliploss, name)
    loss = ev.LossWrapper()
    combo = ev.ComboEvaluator([other(), loss])
    with no_warnings():
        average = ev.validate_tracks(bank, labels, None, model, combo, T, MARGIN, batch_size=batch_size, losses=True)
    check_calls(name, seen)
    # the windows the model received: plan.kept[:, 1:3] in plan order, then the short track whole
    seam = [(args, r) for args, r in seen if args[0].shape[1] == T]
    short = [(args, r) for args, r in seen if args[0].shape[1] != T]
    assert len(seam) == heads * -(-7 // batch_size) and len(short) == heads
    for h in range(heads):
        tables = np.concatenate([table_of(args[-1]) for args, _ in seam[h::heads]])
        assert np.array_equal(tables, plan.kept[:, 1:3]) and all(isinstance(args[-1], cliploss.Windows) and args[-1].dev.is_cuda for args, _ in seam)
        assert table_of(short[h][0][-1]).tolist() == [[0, counts[3]]] and short[h][0][0].shape[:2] == (1, counts[3])
    # every track: the float64 sum of its clips' recorded sums over its length
    assert list(loss.results) == list(loss_keys) + ([tools.KEY_LOSS_TOTAL] if heads > 1 else [])
    per_track = {}
    for h, key in enumerate(loss_keys):
        clip_sums = np.concatenate([r.cpu().numpy() for _, r in seam[h::heads]])
        want = [sum(clip_sums[plan.track_ids == t].tolist()) / counts[t] for t in range(3)] + [float(short[h][1][0]) / counts[3]]
        per_track[key] = np.asarray(want)
        got = np.asarray(loss.results[key])
        assert got.shape == (4,) and (np.abs(got - want) <= 1e-12 * np.abs(want)).all() and (got > 0).all(), (key, got, want)
    total = np.asarray(loss.results[tools.KEY_LOSS_TOTAL])
    assert (np.abs(total - sum(per_track.values())) <= 1e-12 * total).all()
    assert average[tools.KEY_LOSS] == {k: float(np.mean(v)) for k, v in loss.results.items()}
    # a track that fits one clip: the loss of the track run whole, in whatever batch its clip ran (the engines' outputs of a clip do not
    # depend on the batch around it: tests/test_gpu_run_tracks.py holds that bit for bit)
    for t in (2, 3):
        for key in loss.results:
            got, want = float(np.asarray(loss.results[key])[t]), whole[t][key]
            print(f'{which} batch {batch_size} track {t} {key}: stitched {got!r} whole {want!r}')
            assert abs(got - want) <= 1e-12 * want, (t, key, got, want)
    # the other leaf scores as without the losses
    for k in plain.results:
        assert np.array_equal(np.asarray(combo.evaluators[0].results[k]), np.asarray(plain.results[k])), k


# ------------------------------------------------------------------------------------------------------------------------------
# 5. validate_batched
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch_size', [2, 256])
def test_validate_batched_tracks_every_clips_loss(monkeypatch, batch_size):
    from test_gpu_evaluate import of_setup
    model, clips, times, references, _ = of_setup()
    plain = ev.ComboEvaluator([ev.MultipitchEvaluator(), ev.NoteEvaluator()])
    ev.validate_batched(clips, references, model, plain, times=times, batch_size=batch_size)
    seen = spy(monkeypatch, cliploss, 'bce_sums')
    loss = ev.LossWrapper()
    combo = ev.ComboEvaluator([ev.MultipitchEvaluator(), loss, ev.NoteEvaluator()])
    with no_warnings():
        average = ev.validate_batched(clips, references, model, combo, times=times, batch_size=batch_size, losses=True)
    assert len(seen) == 2 * -(-5 // batch_size)
    check_calls('bce_sums', seen)
    # the labels the heads saw are the references' own maps
    for h, key in enumerate((tools.KEY_MULTIPITCH, tools.KEY_ONSETS)):
        given = np.concatenate([args[1].cpu().numpy() for args, _ in seen[h::2]])
        assert np.array_equal(given, np.stack([r[key] for r in references]).astype(np.float32)), key
    pitch, onsets = per_head(seen, 2)
    frames = references[0][tools.KEY_MULTIPITCH].shape[-1]
    assert list(loss.results) == [tools.KEY_LOSS_PITCH, tools.KEY_LOSS_ONSETS, tools.KEY_LOSS_TOTAL]
    assert np.array_equal(np.asarray(loss.results[tools.KEY_LOSS_PITCH]), pitch / frames) and pitch.shape == (5,) and (pitch > 0).all()
    assert np.array_equal(np.asarray(loss.results[tools.KEY_LOSS_ONSETS]), onsets / frames)
    assert np.allclose(np.asarray(loss.results[tools.KEY_LOSS_TOTAL]), (pitch + onsets) / frames, rtol=1e-15, atol=0)
    assert list(average) == [tools.KEY_MULTIPITCH, tools.KEY_LOSS, tools.KEY_NOTES]
    assert average[tools.KEY_LOSS] == {k: float(np.mean(v)) for k, v in loss.results.items()}
    for got_e, want_e in zip((combo.evaluators[0], combo.evaluators[2]), plain.evaluators):
        for k in want_e.results:
            assert np.array_equal(np.asarray(got_e.results[k]), np.asarray(want_e.results[k])), k
