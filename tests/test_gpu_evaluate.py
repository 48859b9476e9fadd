"""Evaluation on the device (csrc/eval.hip): the three counting / matching entries against NumPy and the brute-force matcher of
tests/eval_cases.py, each also with poisoned outputs and workspace, then validate_batched end to end against the host evaluators fed with
run_offline_batched's output.  Everything is compared for equality: counts are integers, and both paths end in results_from_counts."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from amt_tools_amd import _lib, evaluate as ev, tools, transcribe                     # noqa: E402
from amt_tools_amd.inference import run_offline_batched                               # noqa: E402
from poison import Poison                                                             # noqa: E402
import eval_cases as ec                                                               # noqa: E402
from test_gpu_tab_notes import random_tab                                             # noqa: E402

DEV = 'cuda:0'
PROFILE = tools.GuitarProfile(num_frets=19)
LENGTHS = (1, 63, 64, 65, 200, 1001)


# ------------------------------------------------------------------------------------------------------------------------------
# amtx_eval_multipitch_counts
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_maps(T, slices):
    rng = np.random.default_rng(40 + T + slices)
    shape = (5, slices, 88, T) if slices > 1 else (5, 88, T)
    est, ref = (rng.random(shape) < 0.1).astype(np.float32), (rng.random(shape) < 0.1).astype(np.float32)
    est[3] = 0                                   # clip 3: a silent estimate; clip 4: a perfect one; one slice of clip 2: both silent
    est[4] = ref[4]
    est[2, ..., :44, :] = 0
    ref[2, ..., :44, :] = 0
    for a in (est, ref):
        a.setflags(write=False)
    return est, ref


def numpy_map_counts(est, ref):
    e, r = est.reshape(est.shape[0], -1, 88 * est.shape[-1]) != 0, ref.reshape(ref.shape[0], -1, 88 * ref.shape[-1]) != 0
    return np.stack([(e & r).sum(-1), e.sum(-1), r.sum(-1)], axis=-1).astype(np.int64)


@pytest.mark.parametrize('pattern', [0x00, 0xFF])
@pytest.mark.parametrize('slices', [1, 6])
def test_multipitch_counts_equal_numpy(monkeypatch, slices, pattern):
    poison = Poison(monkeypatch, pattern)
    e = ev.StackedMultipitchEvaluator() if slices > 1 else ev.MultipitchEvaluator()
    for T in LENGTHS:
        est, ref = random_maps(T, slices)
        # batch 3 of the issue plus the silent / perfect clips.  88 * T is a multiple of 4, so every slice of these maps starts on the
        # 16-byte grid (the float4 body alone); once more with the two maps at DIFFERENT phases (the scalar loop throughout).  The scalar
        # head and tail are test_multipitch_counts_head_and_tail's
        est_d, ref_d = torch.from_numpy(np.array(est)).to(DEV), torch.from_numpy(np.array(ref)).to(DEV)
        before = poison.filled
        got = e.counts_batch(est_d, ref_d)
        assert poison.filled > before and got.dtype == torch.int64 and got.shape == (5, slices, 3)
        want = numpy_map_counts(est, ref)
        assert np.array_equal(got.cpu().numpy(), want), T
        flat = torch.zeros(est.size + 1, dtype=torch.float32, device=DEV)
        flat[1:] = est_d.reshape(-1)
        assert np.array_equal(e.counts_batch(flat[1:].reshape(est.shape), ref_d).cpu().numpy(), want), T
        for b in (0, 3, 4):
            host = e.evaluate(est[b].astype(np.float64), ref[b].astype(np.float64))
            assert e.results_from_counts(got[b].cpu().numpy()) == host


@pytest.mark.parametrize('keys', [88, 87, 1])
def test_multipitch_counts_head_and_tail(keys):
    """The scalar head and tail of the kernel: both maps at the SAME non-zero phase of a 16-byte line, as views 0 .. 3 floats into a
    larger buffer, and slices of keys * T floats with keys * T no multiple of 4 (87 keys or 1 key and an odd T), so that inside one call
    the slices start at every phase: head and tail both take every value in 0 .. 3, and with 1 key the head is longer than the slice
    (T = 1, 2).  The buffers hold ones around the views -- a cell read outside a view is counted -- and an all-ones pair of maps makes
    every cell of the view count: one cell missed or taken twice changes the result."""
    e = ev.StackedMultipitchEvaluator()
    rng = np.random.default_rng(keys)
    heads, tails = set(), set()
    for T in (1, 2, 3, 5, 63, 65, 201):
        shape = (3, 6, keys, T)
        n, size = keys * T, 3 * 6 * keys * T
        random = (rng.random(shape) < 0.3).astype(np.float32), (rng.random(shape) < 0.3).astype(np.float32)
        ones = np.ones(shape, dtype=np.float32), np.ones(shape, dtype=np.float32)
        for est, ref in (random, ones):
            flat_e, flat_r = (x.reshape(3, 6, n) != 0 for x in (est, ref))
            want = np.stack([(flat_e & flat_r).sum(-1), flat_e.sum(-1), flat_r.sum(-1)], axis=-1)
            for phase in range(4):
                bufs = []
                for x in (est, ref):
                    buf = torch.ones(size + 8, dtype=torch.float32, device=DEV)
                    buf[phase:phase + size] = torch.from_numpy(x).to(DEV).reshape(-1)
                    bufs.append(buf[phase:phase + size].reshape(shape))
                    assert bufs[-1].data_ptr() % 16 == 4 * phase and bufs[-1].is_contiguous()
                got = e.counts_batch(*bufs).cpu().numpy()
                assert np.array_equal(got, want), (T, phase, got.tolist(), want.tolist())
                for row in range(18):                       # what the kernel's three-part walk comes to for these slices
                    head = min(-(phase + row * n) % 4, n)
                    heads.add(head)
                    tails.add((n - head) % 4)
    assert (heads, tails) == ({0, 1, 2, 3}, {0, 1, 2, 3})


def test_multipitch_counts_refuse_bad_arguments():
    L = _lib.lib()
    x = torch.zeros((1, 1, 88, 8), dtype=torch.float32, device=DEV)
    out = torch.zeros(3, dtype=torch.int64, device=DEV)
    assert L.amtx_eval_multipitch_counts(_lib.ptr(x), None, 1, 1, 88, 8, _lib.ptr(out), None) == -1
    assert L.amtx_eval_multipitch_counts(_lib.ptr(x), _lib.ptr(x), 1, 0, 88, 8, _lib.ptr(out), None) == -1
    assert L.amtx_eval_multipitch_counts(_lib.ptr(x), _lib.ptr(x), 1, 1, 1 << 16, 1 << 16, _lib.ptr(out), None) == -1


# ------------------------------------------------------------------------------------------------------------------------------
# amtx_eval_tab_counts
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tab_pair(T):
    est = np.array(random_tab(T))
    ref = np.array(random_tab(T, 19))                           # another seed, classes 0 .. 18
    rng = np.random.default_rng(T)
    ref = np.where(rng.random(ref.shape) < 0.5, est, ref)
    t = T // 2
    est[0, 0, t], est[0, 1, t], ref[0, 0, t], ref[0, 1, t] = 5, 0, 5, 0          # two strings on A2 in one frame, on both sides
    est[1, 0, t], est[1, 1, t], ref[1, 0, t], ref[1, 1, t] = 5, 0, -1, 0         # ... on one side only
    est[2, 2, t], ref[2, 2, t] = 25, 25                                         # a stray class, equal on both sides
    est[2, 3, 0], ref[2, 3, 0] = -7, 3                                          # and a stray negative one
    return est, ref


def host_tab_counts(est, ref):
    """The five counts from tools' own maps, multiplied and summed (stray classes: silent for the maps, plain integers for [4])."""
    valid = lambda x: np.where((x >= 0) & (x < 20), x, -1)      # noqa: E731
    st_e, st_r = tools.tablature_to_stacked_multi_pitch(valid(est), PROFILE), tools.tablature_to_stacked_multi_pitch(valid(ref), PROFILE)
    co_e, co_r = st_e.max(axis=-3), st_r.max(axis=-3)
    flat = lambda x: x.reshape(x.shape[0], -1)                  # noqa: E731
    return np.stack([flat(st_e).sum(-1), flat(st_r).sum(-1), flat(st_e * st_r).sum(-1), flat(co_e * co_r).sum(-1), flat(est == ref).sum(-1),
                     np.full(est.shape[0], est.shape[1] * est.shape[2])], axis=-1).astype(np.int64)


@pytest.mark.parametrize('pattern', [0x00, 0xFF])
def test_tab_counts_equal_the_host_maps(monkeypatch, pattern):
    Poison(monkeypatch, pattern)
    for T in LENGTHS:
        est, ref = tab_pair(T)
        got = ev.TablatureEvaluator(PROFILE).counts_batch(torch.from_numpy(est).to(DEV), torch.from_numpy(ref).to(DEV)).cpu().numpy()
        want = host_tab_counts(est, ref)
        assert np.array_equal(got, want), (T, got, want)
        if T > 1:
            assert 0 < want[0, 2] < want[0, 0] and 0 < want[0, 3] < want[0, 0]                # the counts are not degenerate
        acc = ev.SoftmaxAccuracy().counts_batch(torch.from_numpy(est).to(DEV), torch.from_numpy(ref).to(DEV)).cpu().numpy()
        assert np.array_equal(acc[:, 4:], want[:, 4:])
        clean_e, clean_r = np.where((est[0] >= 0) & (est[0] < 20), est[0], -1), np.where((ref[0] >= 0) & (ref[0] < 20), ref[0], -1)
        assert ev.TablatureEvaluator(PROFILE).results_from_counts(got[0]) == ev.TablatureEvaluator(PROFILE).evaluate(clean_e, clean_r)
        assert ev.SoftmaxAccuracy().results_from_counts(acc[0]) == ev.SoftmaxAccuracy().evaluate(est[0], ref[0])


def test_tab_counts_refuse_more_than_16_strings():
    x = torch.zeros((1, 17, 8), dtype=torch.int64, device=DEV)
    out = torch.zeros(5, dtype=torch.int64, device=DEV)
    tuning = np.zeros(17, dtype=np.int32)
    assert _lib.lib().amtx_eval_tab_counts(_lib.ptr(x), _lib.ptr(x), 1, 17, 8, _lib.ptr(tuning), 20, _lib.ptr(out), None) == _lib.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------------------------
# amtx_eval_notes_match
# ------------------------------------------------------------------------------------------------------------------------------
def onset_order(rows):
    """What amtx_tab_notes writes for a string: ascending onset, pitches interleaved (rows of one pitch stay in onset order)."""
    return rows[np.argsort(rows[:, 0], kind='stable')]


def device_match(groups, ratio, est_order=None, wait=1):
    """(return code, matched (G,), status) of one call on a list of (est, ref) groups."""
    est = [g[0] if est_order is None else est_order(g[0]) for g in groups]
    er, eo, _ = ev._pack_groups(est) if est_order is None else (np.concatenate(est + [np.zeros((0, 3))]), None, None)
    if est_order is not None:
        eo = np.zeros(len(est) + 1, dtype=np.int32)
        eo[1:] = np.cumsum([len(g) for g in est])
        er = er if len(er) else np.zeros((1, 3))
    rr, ro, _ = ev._pack_groups([g[1] for g in groups])
    G = len(groups)
    L = _lib.lib()
    er_d, eo_d, rr_d, ro_d = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (er, eo, rr, ro))
    ws = _lib.alloc_workspace(int(L.amtx_eval_notes_match_workspace_bytes(er.shape[0], rr.shape[0])), DEV)
    matched = torch.empty(G, dtype=torch.int32, device=DEV)
    status = torch.empty(1, dtype=torch.int32, device=DEV)
    rc = L.amtx_eval_notes_match(_lib.ptr(er_d), _lib.ptr(eo_d), er.shape[0], _lib.ptr(rr_d), _lib.ptr(ro_d), rr.shape[0], G, ev.ONSET_TOLERANCE,
                                 -1.0 if ratio is None else ratio, ev.OFFSET_MIN_TOLERANCE, ev.N_DECIMALS, _lib.ptr(ws), ws.numel(), _lib.ptr(matched),
                                 _lib.ptr(status), wait, _lib.current_stream(DEV))
    torch.cuda.synchronize()
    assert _lib.guards_intact(ws)
    return rc, matched.cpu().numpy(), int(status.item())


NAMES = sorted(ec.cases())


@pytest.mark.parametrize('pattern', [0x00, 0xFF])
@pytest.mark.parametrize('ratio', ec.RATIOS)
def test_notes_match_equals_the_brute_force(monkeypatch, ratio, pattern):
    """Every host-test case as a group of its own call (1 group) and all of them in one call of 130 groups with empty groups at the start,
    in the middle and at the end; estimated rows in (pitch, onset) order and in plain onset order."""
    monkeypatch.setattr(_lib, 'GUARD_BYTES', 256)
    Poison(monkeypatch, pattern)
    empty = (np.zeros((0, 3)), np.zeros((0, 3)))
    groups, want = [empty], [0]
    for k in range(126):
        if k == 60:
            groups.append(empty)
            want.append(0)
        name = NAMES[k % len(NAMES)]
        groups.append(ec.cases()[name])
        want.append(ec.expected(name, ratio))
    groups += [empty, empty]
    want += [0, 0]
    assert len(groups) == 130
    for order in (None, onset_order):
        rc, matched, status = device_match(groups, ratio, order)
        assert rc == 0 and status == 0
        assert matched.tolist() == want, [(NAMES[(i - 1) % len(NAMES)], g, w) for i, (g, w) in enumerate(zip(matched.tolist(), want)) if g != w][:5]
    for name in ('greedy_a', 'greedy_b', 'long_list', 'tolerance_edges', 'empty_est'):
        rc, matched, status = device_match([ec.cases()[name]], ratio)
        assert (rc, status, matched.tolist()) == (0, 0, [ec.expected(name, ratio)]), name
    est, ref = ec.cases()['long_list']
    assert len(ref) > 64 and ec.brute_edges(est, ref, None).sum(axis=0).max() > 64      # more than a wave's worth of candidates


def test_notes_match_refuses_what_it_does_not_build(monkeypatch):
    monkeypatch.setattr(_lib, 'GUARD_BYTES', 256)
    Poison(monkeypatch, 0xFF)
    small = ec.cases()['random_1']
    # a window beyond the bound: that group alone answers AMTX_ERR_UNSUPPORTED, the call reports it, the guard bands hold
    for wait in (1, 0):
        rc, matched, status = device_match([small, ec.beyond_the_bound(), small], 0.2, wait=wait)
        assert rc == (_lib.ERR_UNSUPPORTED if wait else 0) and status == _lib.ERR_UNSUPPORTED
        assert matched.tolist() == [ec.expected('random_1', 0.2), _lib.ERR_UNSUPPORTED, ec.expected('random_1', 0.2)]
    # fractional and out-of-range pitches: AMTX_ERR_ARG
    frac = (np.array([[1.0, 2.0, 60.5]]), np.array([[1.0, 2.0, 60.0]]))
    high = (np.array([[1.0, 2.0, 60.0]]), np.array([[1.0, 2.0, 128.0]]))
    rc, matched, status = device_match([small, frac, high], None)
    assert rc == -1 and status == -1 and matched.tolist() == [ec.expected('random_1', None), -1, -1]
    # offsets that point past the arrays are clamped: nothing outside is read, the call itself succeeds
    L = _lib.lib()
    rows = torch.from_numpy(np.ascontiguousarray(small[0][np.lexsort((small[0][:, 0], small[0][:, 2]))])).to(DEV)
    off = torch.tensor([0, 1 << 30], dtype=torch.int32, device=DEV)
    ws = _lib.alloc_workspace(int(L.amtx_eval_notes_match_workspace_bytes(len(rows), len(rows))), DEV)
    out = torch.empty(2, dtype=torch.int32, device=DEV)
    rc = L.amtx_eval_notes_match(_lib.ptr(rows), _lib.ptr(off), len(rows), _lib.ptr(rows), _lib.ptr(off), len(rows), 1, 0.05, -1.0, 0.05, 4, _lib.ptr(ws),
                                 ws.numel(), _lib.ptr(out), _lib.ptr(out[1:]), 1, _lib.current_stream(DEV))
    assert rc == 0 and out.tolist() == [len(rows), 0] and _lib.guards_intact(ws)
    assert L.amtx_eval_notes_match(_lib.ptr(rows), _lib.ptr(off), len(rows), _lib.ptr(rows), _lib.ptr(off), len(rows), 1, 0.05, -1.0, 0.05, 4, _lib.ptr(ws),
                                   16, _lib.ptr(out), _lib.ptr(out[1:]), 1, None) == -1


def test_counts_batch_of_the_note_evaluators():
    groups = [ec.cases()[n] for n in ('random_2', 'greedy_b', 'empty_ref')]
    er, eo, _ = ev._pack_groups([g[0] for g in groups])
    rr, ro, _ = ev._pack_groups([g[1] for g in groups])
    to = lambda a: torch.from_numpy(a).to(DEV)               # noqa: E731
    e = ev.StackedNoteEvaluator(offset_ratio=0.2)
    counts = e.counts_batch((to(er), to(eo)), (to(rr), to(ro))).cpu().numpy()
    assert counts.tolist() == [[ec.expected(n, 0.2), len(ec.cases()[n][0]), len(ec.cases()[n][1])] for n in ('random_2', 'greedy_b', 'empty_ref')]
    host = e.evaluate({s: (g[0][:, 2], g[0][:, :2]) for s, g in enumerate(groups)}, {s: (g[1][:, 2], g[1][:, :2]) for s, g in enumerate(groups)})
    assert e.results_from_counts(counts) == host


# ------------------------------------------------------------------------------------------------------------------------------
# validate_batched end to end
# ------------------------------------------------------------------------------------------------------------------------------
def of_combo():
    return ev.ComboEvaluator([ev.MultipitchEvaluator(), ev.NoteEvaluator(), ev.NoteEvaluator(offset_ratio=0.2, results_key='notes-with-offsets')])


@functools.lru_cache(maxsize=None)
def of_setup():
    from amt_tools_amd.features import MelSpec
    from amt_tools_amd.models import OnsetsFrames
    from amt_tools_amd.synth import synth_batch, synth_labels, synth_state_dict
    T = 40
    model = OnsetsFrames(229, tools.PianoProfile(), 1, 2, device=DEV, precision='x3')
    sd = synth_state_dict(0, dim_in=229, in_channels=1, model_complexity=2)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model.frontend = torch.nn.Sequential(MelSpec(sample_rate=22050, hop_length=512, n_mels=229, n_fft=2048).frontend())
    model.change_device()
    model.eval()
    clips = synth_batch(0, 5, num_samples=512 * T - 1)
    times = np.arange(T) * 512 / 22050.0
    references = []
    for i in range(5):
        mp, on = synth_labels(i, num_frames=T)
        references.append({tools.KEY_MULTIPITCH: mp, tools.KEY_ONSETS: on, tools.KEY_NOTES: transcribe.multi_pitch_to_notes(mp, times, 21, on)})
    out = run_offline_batched(clips, model, times=times, batch_size=3, decode_notes=True)
    return model, clips, times, references, out


def host_scores(make, out, references, clips):
    combo, per_clip = make(), {}
    for i in clips:
        per_clip[i] = combo.process_track(out[i], references[i], i)
    return combo, per_clip


@pytest.mark.parametrize('batch_size', [2, 256])
def test_validate_batched_equals_the_host_evaluators_on_onsets_and_frames(batch_size, tmp_path):
    model, clips, times, references, out = of_setup()
    assert sum(len(out[i][tools.KEY_NOTES]) for i in range(5)) > 0
    want, per_clip = host_scores(of_combo, out, references, range(5))
    combo = of_combo()
    combo.set_save_dir(str(tmp_path))
    average = ev.validate_batched(clips, references, model, combo, times=times, batch_size=batch_size)
    assert average == want.average_results() and list(average) == [tools.KEY_MULTIPITCH, tools.KEY_NOTES, 'notes-with-offsets']
    for got_e, want_e in zip(combo.evaluators, want.evaluators):                     # per clip, in clip order
        assert list(got_e.results) == list(want_e.results)
        for k in want_e.results:
            assert np.array_equal(np.asarray(got_e.results[k]), np.asarray(want_e.results[k])) and len(got_e.results[k]) == 5, k
    assert sorted(p.name for p in tmp_path.iterdir()) == [f'{i}.txt' for i in range(5)]


def test_validate_batched_shards_by_rank():
    model, clips, times, references, out = of_setup()
    want, _ = host_scores(of_combo, out, references, (1, 3))
    combo = of_combo()
    average = ev.validate_batched(clips, references, model, combo, times=times, batch_size=256, rank=1, world=2)
    assert average == want.average_results()
    assert len(combo.evaluators[0].results[tools.KEY_F1]) == 2


def test_validate_batched_equals_the_host_evaluators_on_tabcnn():
    from amt_tools_amd.models import TabCNN
    from amt_tools_amd.synth import synth_batch, synth_tabcnn_state_dict
    model = TabCNN(192, PROFILE, 1, 1, device=DEV)
    sd = synth_tabcnn_state_dict(5, dim_in=192, in_channels=1, model_complexity=1, num_groups=6, num_classes=21)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model.change_device()
    model.eval()
    T = 40
    feats = np.random.default_rng(3).random((5, 1, 192, T)).astype(np.float32)
    times = np.arange(T) * 512 / 22050.0
    out = run_offline_batched(feats, model, times=times, batch_size=3, decode_notes=True, keep=(tools.KEY_TABLATURE,))
    references = []
    for i in range(5):
        # ground truth: the estimate with half of its cells redrawn, so that every count is well away from 0 and from the total
        rng = np.random.default_rng(50 + i)
        tab = np.where(rng.random((6, T)) < 0.5, out[i][tools.KEY_TABLATURE], np.repeat(rng.integers(-1, 20, size=(6, T // 4)), 4, axis=-1))
        references.append({tools.KEY_TABLATURE: tab, tools.KEY_NOTES: transcribe._tab_to_stacked_notes_host(tab, times, PROFILE)})
    make = lambda: ev.ComboEvaluator([ev.TablatureEvaluator(PROFILE), ev.SoftmaxAccuracy(results_key='accuracy'),   # noqa: E731
                                      ev.StackedNoteEvaluator(offset_ratio=0.2), ev.StackedNoteEvaluator(average_slices=True, results_key='notes-avg')])
    want, _ = host_scores(make, out, references, range(5))
    assert sum(len(p) for i in range(5) for p, _ in out[i][tools.KEY_NOTES].values()) > 0
    for batch_size in (2, 256):
        combo = make()
        average = ev.validate_batched(feats, references, model, combo, times=times, batch_size=batch_size)
        assert average == want.average_results()
        assert 0 < average[tools.KEY_TABLATURE][tools.KEY_F1] < 1 and list(average[tools.KEY_NOTES]) == list(range(6))


# ------------------------------------------------------------------------------------------------------------------------------
# validate_batched: the branches a batch takes only now and then
# ------------------------------------------------------------------------------------------------------------------------------
def assert_same_results(combo, want, clips=5):
    """Per clip, in clip order: what every leaf has tracked equals the host evaluators' record."""
    def same(got, want):
        assert list(got) == list(want)
        for k in want:
            if isinstance(want[k], dict):
                same(got[k], want[k])
            else:
                assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])) and len(got[k]) == clips, k
    for got_e, want_e in zip(combo.evaluators, want.evaluators):
        same(got_e.results, want_e.results)


def spy(monkeypatch, module, name, **forced):
    """Replace module.name by a wrapper that counts its calls, keeps what they returned and forces the given keyword arguments."""
    real, seen = getattr(module, name), []

    def wrapper(*args, **kwargs):
        seen.append(real(*args, **dict(kwargs, **forced)))
        return seen[-1]
    monkeypatch.setattr(module, name, wrapper)
    return seen


@functools.lru_cache(maxsize=None)
def tab_setup():
    """The model, clips and ground truth of test_validate_batched_equals_the_host_evaluators_on_tabcnn."""
    from amt_tools_amd.models import TabCNN
    from amt_tools_amd.synth import synth_tabcnn_state_dict
    model = TabCNN(192, PROFILE, 1, 1, device=DEV)
    sd = synth_tabcnn_state_dict(5, dim_in=192, in_channels=1, model_complexity=1, num_groups=6, num_classes=21)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model.change_device()
    model.eval()
    T = 40
    feats = np.random.default_rng(3).random((5, 1, 192, T)).astype(np.float32)
    times = np.arange(T) * 512 / 22050.0
    out = run_offline_batched(feats, model, times=times, batch_size=3, decode_notes=True, keep=(tools.KEY_TABLATURE,))
    references = []
    for i in range(5):
        rng = np.random.default_rng(50 + i)
        tab = np.where(rng.random((6, T)) < 0.5, out[i][tools.KEY_TABLATURE], np.repeat(rng.integers(-1, 20, size=(6, T // 4)), 4, axis=-1))
        references.append({tools.KEY_TABLATURE: tab, tools.KEY_NOTES: transcribe._tab_to_stacked_notes_host(tab, times, PROFILE)})
    return model, feats, times, references, out


def tab_combo():
    return ev.ComboEvaluator([ev.TablatureEvaluator(PROFILE), ev.SoftmaxAccuracy(results_key='accuracy'),
                              ev.StackedNoteEvaluator(offset_ratio=0.2), ev.StackedNoteEvaluator(average_slices=True, results_key='notes-avg')])


def test_validate_batched_takes_the_host_matcher_when_the_decoder_overflows(monkeypatch):
    """A first row buffer of ONE row: the device matcher runs on the truncated buffer (its group offsets are clamped to the buffer), the
    batch is decoded again into a buffer of the exact size, and the host matcher scores it -- every batch, both note evaluators."""
    model, clips, times, references, out = of_setup()
    want, _ = host_scores(of_combo, out, references, range(5))
    decoded = spy(monkeypatch, transcribe, 'decode_notes_batch_async', rows_capacity=1)
    on_host = spy(monkeypatch, ev, '_host_note_counts')
    combo = of_combo()
    average = ev.validate_batched(clips, references, model, combo, times=times, batch_size=2)
    assert len(decoded) == 3 and len(on_host) == 6
    assert average == want.average_results()
    assert_same_results(combo, want)


def test_validate_batched_takes_the_host_matcher_when_the_tablature_decoder_overflows(monkeypatch):
    model, feats, times, references, out = tab_setup()
    want, _ = host_scores(tab_combo, out, references, range(5))
    decoded = spy(monkeypatch, transcribe, 'decode_tab_notes_batch_async', rows_capacity=1)
    on_host = spy(monkeypatch, ev, '_host_note_counts')
    combo = tab_combo()
    average = ev.validate_batched(feats, references, model, combo, times=times, batch_size=2)
    assert len(decoded) == 3 and len(on_host) == 6 and all(isinstance(h, transcribe._PendingTabNotes) for h in decoded)
    assert average == want.average_results()
    assert_same_results(combo, want)


def test_validate_batched_takes_the_host_matcher_for_a_fractional_reference_pitch(monkeypatch):
    """One reference pitch of clip 1 moved by half a semitone: the device matcher takes integral pitches only, so the batch that holds
    the clip goes to the host matcher as a whole (both note evaluators: 2 calls), the other batches stay on the device."""
    model, clips, times, references, out = of_setup()
    references = [dict(r) for r in references]
    notes = np.array(references[1][tools.KEY_NOTES])
    assert len(notes) > 0
    notes[0, 2] += 0.5
    references[1][tools.KEY_NOTES] = notes
    want, _ = host_scores(of_combo, out, references, range(5))
    on_host = spy(monkeypatch, ev, '_host_note_counts')
    combo = of_combo()
    average = ev.validate_batched(clips, references, model, combo, times=times, batch_size=2)
    assert len(on_host) == 2
    assert average == want.average_results()
    assert_same_results(combo, want)


def test_validate_batched_with_the_cpu_tablature_decoder_under_a_gpu_model(monkeypatch):
    """No string count the kernel takes: the handle is the host classes' (no rows on the device), the note evaluators take the host
    matcher, and the results are those of the unpatched run."""
    model, feats, times, references, out = tab_setup()
    want, _ = host_scores(tab_combo, out, references, range(5))
    monkeypatch.setattr(transcribe, 'TAB_MAX_STRINGS', 0)
    decoded = spy(monkeypatch, transcribe, 'decode_tab_notes_batch_async')
    combo = tab_combo()
    average = ev.validate_batched(feats, references, model, combo, times=times, batch_size=2)
    assert len(decoded) == 3 and all(isinstance(h, transcribe._HostTabNotes) and h.device_rows() is None for h in decoded)
    assert average == want.average_results()
    assert_same_results(combo, want)


def test_validate_batched_with_a_loss_wrapper_in_the_combo():
    """The model's eval output has no loss: the LossWrapper leaf warns as its own unpack() does and tracks an empty dictionary per clip;
    the leaves around it score as without it."""
    import re
    model, clips, times, references, out = of_setup()
    make = lambda: ev.ComboEvaluator([ev.MultipitchEvaluator(), ev.NoteEvaluator()])                       # noqa: E731
    want, _ = host_scores(make, out, references, range(5))
    loss = ev.LossWrapper()
    combo = ev.ComboEvaluator([ev.MultipitchEvaluator(), loss, ev.NoteEvaluator()])
    with pytest.warns(RuntimeWarning, match=re.escape(f'Entry for key \'{tools.KEY_LOSS}\' not found in estimates.')):
        average = ev.validate_batched(clips, references, model, combo, times=times, batch_size=2)
    assert loss.results == {} and average == dict(want.average_results(), **{tools.KEY_LOSS: {}})
    assert list(average) == [tools.KEY_MULTIPITCH, tools.KEY_LOSS, tools.KEY_NOTES]
    combo.evaluators.remove(loss)
    assert_same_results(combo, want)
