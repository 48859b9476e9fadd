"""Exact whole-track Onsets & Frames on the device (include/amtx_ofseq.h): the packed-sequence BiLSTM against amtx_bilstm_h_fwd on every
sequence alone, bit for bit, into poisoned memory between guard bands; its refusals; amtx_rows_gather against tracks.gather_rows_host;
run_tracks / validate_tracks with exact=True against every track run whole as a batch of one."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from amt_tools_amd import _lib, cliploss, evaluate as ev, inference, tools               # noqa: E402
from amt_tools_amd.inference import KEY_LOGITS, run_tracks                              # noqa: E402
from amt_tools_amd.synth import synth_state_dict                                        # noqa: E402
from amt_tools_amd.tracks import gather_rows_host, seam_clips                           # noqa: E402
import lstm_ref                                                                          # noqa: E402
from poison import PATTERNS, fill_storage                                               # noqa: E402
from test_gpu_clip_loss import close, piano_labels                                      # noqa: E402
from test_gpu_run_tracks import (DEV, T, _host_scores, _piano_banks, _same_per_track, _tensors, piano_combo, piano_setup,   # noqa: E402
                                 piano_truth)

BF16, F32 = 0, 1
GUARD = 512
X3_LOGITS = 1.5e-4                           # DESIGN section 3's bound for x3 logits
BF16_LOGITS, BF16_CELLS = 6e-2, 3e-3         # the project's bf16 bounds: logits, share of piano-roll cells
LENGTHS = {'seven': (1, 2, 5, 19, 7, 96, 3), 'seventeen': (4, 31, 1, 9, 2, 17, 40, 3, 8, 1, 25, 6, 12, 2, 33, 5, 11)}
HIDDEN = (128, 256, 384, 512)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the recurrence
# ------------------------------------------------------------------------------------------------------------------------------
def _scattered(lengths, seed):
    """(S, 2) table {row0, len} in the order of `lengths`, the sequences packed without gaps in a shuffled order: row0 is not sorted."""
    order = np.random.default_rng(seed).permutation(len(lengths))
    row0 = np.zeros(len(lengths), dtype=np.int64)
    at = 0
    for s in order:
        row0[s] = at
        at += lengths[s]
    assert not (np.diff(row0) > 0).all()
    return np.stack([row0, np.asarray(lengths, dtype=np.int64)], axis=1)


@functools.lru_cache(maxsize=None)
def _case(H, groups, name):
    """Seeded inputs shared by both precisions: xproj [G][R][2][4H], W_hh of each group, the table."""
    lengths = LENGTHS[name]
    R = sum(lengths)
    g = torch.Generator().manual_seed(H * 100 + groups * 10 + len(lengths))
    xproj = torch.randn(groups, R, 2, 4 * H, generator=g)
    a = 0.15 if H == 128 else 0.1
    whh = [((torch.rand(4 * H, H, generator=g) * 2 - 1) * a, (torch.rand(4 * H, H, generator=g) * 2 - 1) * a) for _ in range(groups)]
    return xproj, whh, _scattered(lengths, H + groups)


def _packed_weights(whh, H, planes):
    L = _lib.lib()
    per = L.amtx_bilstm_h_packed_elems(H, planes)
    packed = np.zeros(per * len(whh), dtype=np.uint16)
    for g, (f, b) in enumerate(whh):
        _lib.check(L.amtx_bilstm_h_pack(_lib.ptr(f.numpy()), _lib.ptr(b.numpy()), H, planes, _lib.ptr(packed[g * per:])))
    return torch.from_numpy(packed.view(np.int16)).to(DEV), per


def _arena(nbytes, pattern):
    arena = fill_storage(torch.empty(2 * GUARD + nbytes, dtype=torch.uint8, device=DEV), pattern)
    return arena, arena[GUARD:GUARD + nbytes]


@pytest.mark.parametrize('name', list(LENGTHS))
@pytest.mark.parametrize('groups', [1, 2])
@pytest.mark.parametrize('planes', [1, 2])
@pytest.mark.parametrize('H', HIDDEN)
def test_every_packed_sequence_has_the_bits_of_the_sequence_alone(H, planes, groups, name):
    xproj, whh, seqs = _case(H, groups, name)
    R = int(seqs[:, 1].sum())
    dtype, et = (torch.bfloat16, BF16) if planes == 1 else (torch.float32, F32)
    x = xproj.to(DEV).to(dtype).contiguous()
    wp, per = _packed_weights(whh, H, planes)
    es = x.element_size()
    # every sequence alone: B = 1, T = len (computed once, shared by the patterns)
    alone = torch.zeros((groups, R, 2 * H), dtype=dtype, device=DEV)
    for g in range(groups):
        for row0, n in seqs.tolist():
            out = torch.empty((n, 2 * H), dtype=dtype, device=DEV)
            _lib.call('amtx_bilstm_h_fwd', x[g, row0:row0 + n], wp[g * per:], H, planes, et, out, 1, n, device=DEV)
            alone[g, row0:row0 + n] = out
    want = alone.view(torch.uint8).cpu().numpy().reshape(-1)
    seqs_dev = torch.from_numpy(seqs).to(DEV)
    for pattern in PATTERNS[1:]:
        arena, out = _arena(groups * R * 2 * H * es, pattern)
        _lib.call('amtx_bilstm_seq_fwd', x, wp, H, planes, et, out, seqs, seqs_dev, len(seqs), R, groups, device=DEV)
        got = arena.cpu().numpy()
        assert (got[:GUARD] == pattern).all() and (got[-GUARD:] == pattern).all(), (H, planes, groups, name, hex(pattern))
        same = got[GUARD:-GUARD] == want
        assert same.all(), (H, planes, groups, name, hex(pattern), 'first differing byte', int(np.argmin(same)), int((~same).sum()), 'of', same.size)
    # every row of [0, R) was written: no element of the result is the poison (0x7F7F.. is 3.39e38, no recurrence output)
    assert (alone.float().abs() <= 1).all()


@pytest.mark.parametrize('H,planes', [(128, 1), (128, 2), (256, 1), (256, 2)])
def test_packed_sequences_against_the_fp64_recurrence(H, planes):
    """One case per precision and kernel family, at the bound tests/test_gpu_ops.py holds amtx_bilstm_h_fwd to."""
    xproj, whh, seqs = _case(H, 1, 'seven')
    R = int(seqs[:, 1].sum())
    dtype, et = (torch.bfloat16, BF16) if planes == 1 else (torch.float32, F32)
    x = xproj.to(DEV).to(dtype).contiguous()
    wp, _ = _packed_weights(whh, H, planes)
    out = torch.empty((1, R, 2 * H), dtype=dtype, device=DEV)
    _lib.call('amtx_bilstm_seq_fwd', x, wp, H, planes, et, out, seqs, torch.from_numpy(seqs).to(DEV), len(seqs), R, 1, device=DEV)
    worst = 0.0
    for row0, n in seqs.tolist():
        ref = lstm_ref.forward(x[0, row0:row0 + n].float().cpu().unsqueeze(0), whh[0][0], whh[0][1])[0][0]
        worst = max(worst, float((out[0, row0:row0 + n].float().cpu().double() - ref).abs().max()))
    print(f'SEQ_FP64 hidden {H} planes {planes}: max abs err {worst:.3e}')
    assert worst < (3e-5 if planes == 2 else 3e-2), worst


# ------------------------------------------------------------------------------------------------------------------------------
# 2. bad tables
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,planes', [(128, 1), (256, 2)])
def test_a_bad_table_is_refused_naming_the_row_with_nothing_written(H, planes):
    R = 20
    dtype, et = (torch.bfloat16, BF16) if planes == 1 else (torch.float32, F32)
    x = torch.zeros((1, R, 2, 4 * H), dtype=dtype, device=DEV)
    wp = torch.zeros(_lib.lib().amtx_bilstm_h_packed_elems(H, planes), dtype=torch.int16, device=DEV)
    arena, out = _arena(R * 2 * H * x.element_size(), 0x7F)
    good = [[0, 8], [8, 12]]
    bad = (([[0, 8], [7, 12]], 'sequence 1: .* overlap sequence 0'), ([[12, 8], [0, 13]], 'sequence 1: .* overlap sequence 0'),
           ([[0, 8], [8, 0]], 'sequence 1: len=0'), ([[0, 8], [8, -3]], 'sequence 1: len=-3'), ([[0, 8], [8, 13]], r'sequence 1: rows \[8, 8 \+ 13\) leave the 20 packed rows'),
           ([[0, 8], [21, 1]], 'sequence 1: rows .* leave the 20'), ([[-1, 8], [8, 12]], 'sequence 0: row0=-1 is negative'),
           ([[0, 8], [2 ** 62, 2 ** 62]], 'sequence 1'))
    for table, text in bad:
        seqs = np.array(table, dtype=np.int64)
        with pytest.raises(_lib.AmtxError, match=text):
            _lib.call('amtx_bilstm_seq_fwd', x, wp, H, planes, et, out, seqs, torch.from_numpy(seqs).to(DEV), len(seqs), R, 1, device=DEV)
    seqs = np.array(good, dtype=np.int64)
    seqs_dev = torch.from_numpy(seqs).to(DEV)
    for args, text in (((x, wp, H, planes, et, out, seqs, seqs_dev, 0, R, 1), 'num_seqs=0'), ((x, wp, H, planes, et, out, None, seqs_dev, 2, R, 1), 'host copy .* is null'),
                       ((x, wp, H, planes, et, out, seqs, seqs_dev, 2, R, 0), 'groups=0'), ((x, wp, H, 3, et, out, seqs, seqs_dev, 2, R, 1), 'planes=3')):
        with pytest.raises(_lib.AmtxError, match=text):
            _lib.call('amtx_bilstm_seq_fwd', *args, device=DEV)
    # sizes and types that are not built: unsupported, not a bad argument -- and nothing written either
    for args in ((x, wp, 192, planes, et, out, seqs, seqs_dev, 2, R, 1), (x, wp, H, planes, 1 - et, out, seqs, seqs_dev, 2, R, 1)):
        with pytest.raises(_lib.AmtxError, match=rf'\({_lib.ERR_UNSUPPORTED}\)'):
            _lib.call('amtx_bilstm_seq_fwd', *args, device=DEV)
    torch.cuda.synchronize()
    assert (arena.cpu().numpy() == 0x7F).all()


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the row gather
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('planes', [1, 2])
@pytest.mark.parametrize('np_dtype,width', [(np.uint16, 512), (np.float32, 88)])
def test_rows_gather_equals_gather_rows_host_bit_for_bit(np_dtype, width, planes):
    B, frames, R = 4, 10, 37
    rng = np.random.default_rng(width + planes)
    bits = np.uint16 if np_dtype == np.uint16 else np.uint32
    src = rng.integers(0, np.iinfo(bits).max, size=(planes, B, frames, width), dtype=np.uint64).astype(bits)
    table = np.array([[2, 5, 7], [9, 1, 0], [0, 10, 12], [0, 0, 3]], dtype=np.int64)       # a middle run, one row, a whole clip, nothing
    row = width * src.itemsize
    src_dev = torch.from_numpy(src.view(np.int16 if bits == np.uint16 else np.int32)).to(DEV)
    for pattern in PATTERNS:
        arena, dst = _arena(planes * R * row, pattern)
        _lib.call('amtx_rows_gather', src_dev, B, frames, row, planes, B * frames * row, table, torch.from_numpy(table).to(DEV), dst, R, R * row, device=DEV)
        want = np.empty((planes, R, width), dtype=bits)
        want.view(np.uint8)[:] = pattern
        for p in range(planes):
            gather_rows_host(want[p], src[p], table)
        got = arena.cpu().numpy()
        assert np.array_equal(got[GUARD:-GUARD], want.view(np.uint8).reshape(-1)), (width, planes, hex(pattern))
        assert (got[:GUARD] == pattern).all() and (got[-GUARD:] == pattern).all()
    good = table[:3]
    arena, dst = _arena(planes * R * row, 0x7F)
    for last, text in (([0, 11, 0], 'clip 3: rows .* leave the clip'), ([5, 6, 0], 'clip 3: rows .* leave the clip'), ([0, 10, 28], 'clip 3: rows .* leave the 37 packed rows'),
                       ([-1, 1, 0], 'clip 3: a negative entry'), ([0, 1, -1], 'negative')):
        bad = np.concatenate([good, [last]]).astype(np.int64)
        with pytest.raises(_lib.AmtxError, match=text):
            _lib.call('amtx_rows_gather', src_dev, B, frames, row, planes, B * frames * row, bad, torch.from_numpy(bad).to(DEV), dst, R, R * row, device=DEV)
    with pytest.raises(_lib.AmtxError, match='16 bytes at a time'):
        _lib.call('amtx_rows_gather', src_dev, B, frames, row - 8, planes, B * frames * row, table, torch.from_numpy(table).to(DEV), dst, R, R * row, device=DEV)
    torch.cuda.synchronize()
    assert (arena.cpu().numpy() == 0x7F).all()


# ------------------------------------------------------------------------------------------------------------------------------
# 4. - 6. end to end
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def setup(which):
    """piano_setup's bank (tracks of 118, 59, 40 and 23 frames, MelSpec 229) with OnsetsFrames in bf16 (piano_setup's own model) or x3, or
    OnsetsFrames2 at model_complexity 3 in x3; synthetic weights."""
    from amt_tools_amd.models import OnsetsFrames, OnsetsFrames2
    model, bank = piano_setup()
    if which == 'of1-bf16':
        return model, bank
    cls, mc = (OnsetsFrames, 2) if which == 'of1-x3' else (OnsetsFrames2, 3)
    other = cls(229, tools.PianoProfile(), 1, mc, device=DEV, precision='x3')
    other.load_state_dict(_tensors(synth_state_dict(0, dim_in=229, in_channels=1, model_complexity=mc, offsets=cls is OnsetsFrames2)))
    other.frontend = model.frontend                                           # the bank's own MelSpec module
    other.change_device()
    other.eval()
    return other, bank


def _engine_on(model, bank, ids, firsts, frames):
    """The engine's logits and rolls of clips, their features staged as run_on_batch stages them: {key: (B, T, 88)}, {key: (B, 88, T)}."""
    with torch.no_grad():
        model.__dict__['_in_run_on_batch'] = True
        try:
            feats = model.pre_proc({tools.KEY_AUDIO: bank.clips(ids, firsts, frames)})[tools.KEY_FEATS]
            logits = {k: v.cpu().numpy().copy() for k, v in model(feats).items()}
        finally:
            model.__dict__.pop('_in_run_on_batch', None)
        _, _, on_bin, mp_bin, _ = model.__dict__.pop('_engine_out')
        rolls = {tools.KEY_ONSETS: on_bin.cpu().numpy().copy(), tools.KEY_MULTIPITCH: mp_bin.cpu().numpy().copy()}
        offsets = model.__dict__.pop('_engine_offsets', None)
        if offsets is not None:
            rolls[tools.KEY_OFFSETS] = offsets[1].cpu().numpy().copy()
    return logits, rolls


@functools.lru_cache(maxsize=None)
def whole(which):
    """(w): every track whole as a batch of one -- [(logits {key: (L, 88)}, rolls {key: (88, L)})], computed once and left unchanged."""
    model, bank = setup(which)
    out = []
    for t, n in enumerate(bank.frame_counts.tolist()):
        logits, rolls = _engine_on(model, bank, [t], [0], n)
        out.append(({k: v[0] for k, v in logits.items()}, {k: v[0] for k, v in rolls.items()}))
    return out


def _within(which, got_logits, got_rolls, want, what):
    """The exact route's result for one track against another whole-track result: -> how many logits differ in their bits."""
    x3 = which.endswith('x3')
    want_logits, want_rolls = want
    bits = 0
    for key, ref in want_logits.items():
        err = float(np.abs(got_logits[key] - ref).max())
        bits += int((got_logits[key].view(np.uint32) != ref.view(np.uint32)).sum())
        assert got_logits[key].shape == ref.shape and err <= (X3_LOGITS if x3 else BF16_LOGITS), (what, key, err)
    for key, ref in want_rolls.items():
        differ = got_rolls[key] != ref
        assert got_rolls[key].shape == ref.shape and got_rolls[key].dtype == ref.dtype
        if key == tools.KEY_OFFSETS:                                          # probabilities: the logits' bound through a sigmoid (slope <= 1 / 4)
            assert float(np.abs(got_rolls[key] - ref).max()) <= (X3_LOGITS if x3 else BF16_LOGITS) / 4 + 1e-6, (what, key)
        elif x3:                                                              # identical outside the band around 0 where the threshold may fall either way
            assert not (differ & (np.abs(want_logits[key].T) > X3_LOGITS)).any(), (what, key, int(differ.sum()))
        else:
            assert differ.mean() < BF16_CELLS, (what, key, float(differ.mean()))
    return bits


def _keep(model):
    return (tools.KEY_ONSETS, tools.KEY_MULTIPITCH, KEY_LOGITS) + ((tools.KEY_OFFSETS,) if model.has_offsets else ())


@pytest.mark.parametrize('batch_size', [3, 256])
@pytest.mark.parametrize('which', ['of1-x3', 'of1-bf16', 'of2-mc3-x3'])
def test_exact_run_tracks_is_every_track_run_whole(which, batch_size):
    model, bank = setup(which)
    counts = bank.frame_counts.tolist()
    got = run_tracks(bank, model, T, 3, batch_size=batch_size, keep=_keep(model), exact=True)
    assert list(got) == [0, 1, 2, 3]
    bits = total = 0
    for t in range(4):                                                        # the 40- and 23-frame tracks among them, whatever batch they ran in
        assert got[t][tools.KEY_ONSETS].shape == (88, counts[t]) and got[t][KEY_LOGITS][tools.KEY_MULTIPITCH].shape == (counts[t], 88)
        bits += _within(which, got[t][KEY_LOGITS], got[t], whole(which)[t], (which, batch_size, t))
        total += sum(v.size for v in got[t][KEY_LOGITS].values())
    print(f'EXACT {which} batch_size {batch_size}: {bits} of {total} logits differ from the whole tracks\' in their bits')
    # The case discriminates: the SEGMENT-WISE route on the same plan -- the plan's clips through the whole engine, kept frames by plain
    # slicing, what run_tracks(exact=False) stitches -- is more than ten times the x3 bound away from (w) on at least one track.
    plan = seam_clips(bank.frame_counts, T, 3)
    parts = [_engine_on(model, bank, plan.track_ids[lo:lo + batch_size], plan.first_frames[lo:lo + batch_size], T) for lo in range(0, len(plan.track_ids), batch_size)]
    logits, rolls = ({key: np.concatenate([part[i][key] for part in parts]) for key in (tools.KEY_ONSETS, tools.KEY_MULTIPITCH)} for i in (0, 1))
    segment = run_tracks(bank, model, T, 3, batch_size=batch_size, keep=(tools.KEY_ONSETS, tools.KEY_MULTIPITCH))
    worst = {}
    for j, (t, (d, s, c)) in enumerate(zip(plan.track_ids.tolist(), plan.kept.tolist())):
        for key in (tools.KEY_ONSETS, tools.KEY_MULTIPITCH):
            assert np.array_equal(segment[t][key][:, d:d + c], rolls[key][j][:, s:s + c])           # these ARE the segment-wise route's clips
            worst[t] = max(worst.get(t, 0.0), float(np.abs(logits[key][j][s:s + c] - whole(which)[t][0][key][d:d + c]).max()))
    print(f'SEGMENT-WISE {which}: max |logit - whole| per track {worst}')
    assert max(worst.values()) > 10 * X3_LOGITS, ('the case cannot tell the segment-wise route from the exact one', worst)
    # keep, the request's order and a rank's share, as for the segment-wise route
    some = run_tracks(bank, model, T, 3, track_ids=[3, 1, 0], batch_size=batch_size, keep=(tools.KEY_ONSETS,), decode_notes=True, rank=0, world=2, exact=True)
    assert list(some) == [3, 0] and all(sorted(v) == sorted([tools.KEY_ONSETS, tools.KEY_NOTES]) for v in some.values())
    for t in some:
        assert np.array_equal(some[t][tools.KEY_ONSETS], got[t][tools.KEY_ONSETS])
    assert run_tracks(bank, model, T, 3, track_ids=[1], rank=1, world=2, exact=True) == {}


@pytest.mark.parametrize('which', ['of1-x3', 'of1-bf16', 'of2-mc3-x3'])
def test_the_plan_does_not_matter(which):
    """Margin 3 with 40-frame clips, margin 5 with 24-frame clips, and max_rows small enough for two language passes ([118], [59, 40, 23]):
    each run is the whole tracks' result within the bounds, and the runs agree with one another within them."""
    model, bank = setup(which)
    runs = []
    for frames, margin, max_rows in ((T, 3, 1 << 18), (24, 5, 1 << 18), (T, 3, 130)):
        mine, maps, logits = inference._exact_tracks(bank, model, frames, margin, batch_size=5, want_logits=True, max_rows=max_rows)
        assert mine.tolist() == [0, 1, 2, 3]
        runs.append([({k: v[0].cpu().numpy() for k, v in logits[j].items()}, {k: maps.track(j, k)[0].cpu().numpy() for k in maps.keys}) for j in range(4)])
    for a, run in enumerate(runs):
        for t in range(4):
            _within(which, run[t][0], run[t][1], whole(which)[t], (which, a, t))
            for b in range(a):
                _within(which, run[t][0], run[t][1], runs[b][t], (which, a, b, t))


@pytest.mark.parametrize('batch_size', [3, 256])
def test_validate_tracks_exact_scores_its_own_predictions_and_the_whole_track_loss(batch_size):
    model, bank = setup('of1-bf16')
    labels, notes = piano_labels(), _piano_banks(bank, piano_truth())[1]
    predictions = run_tracks(bank, model, T, 3, batch_size=batch_size, decode_notes=True, keep=(tools.KEY_ONSETS, tools.KEY_MULTIPITCH, KEY_LOGITS), exact=True)
    track_logits = {t: p.pop(KEY_LOGITS) for t, p in predictions.items()}
    want = _host_scores(piano_combo, predictions, labels, notes, lambda groups: groups[0])
    combo = piano_combo()
    loss = ev.LossWrapper()
    average = ev.validate_tracks(bank, labels, notes, model, ev.ComboEvaluator(combo.evaluators + [loss]), T, 3, batch_size=batch_size, losses=True, exact=True)
    assert {k: v for k, v in average.items() if k != tools.KEY_LOSS} == want.average_results()
    _same_per_track(combo, want, 4)
    # each track's loss: cliploss' NumPy restatement on the track's own whole-track logits over all of its frames, over L_t
    assert list(loss.results) == [tools.KEY_LOSS_PITCH, tools.KEY_LOSS_ONSETS, tools.KEY_LOSS_TOTAL]
    counts = bank.frame_counts.tolist()
    for key, est, ref in ((tools.KEY_LOSS_PITCH, tools.KEY_MULTIPITCH, tools.KEY_MULTIPITCH), (tools.KEY_LOSS_ONSETS, tools.KEY_ONSETS, tools.KEY_ONSETS)):
        sums = [float(cliploss.bce_sums(track_logits[t][est][None], labels.host_map(t, ref)[None].astype(np.float32))[0]) for t in range(4)]
        close(np.asarray(loss.results[key]) * counts, sums, counts, key)
        assert (np.asarray(loss.results[key]) > 0).all()
    total = np.asarray(loss.results[tools.KEY_LOSS_TOTAL])
    assert (np.abs(total - (np.asarray(loss.results[tools.KEY_LOSS_PITCH]) + np.asarray(loss.results[tools.KEY_LOSS_ONSETS]))) <= 1e-12 * total).all()
    assert average[tools.KEY_LOSS] == {k: float(np.mean(v)) for k, v in loss.results.items()}
