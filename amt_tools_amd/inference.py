"""
Inference drivers.

* `run_offline(track_data, model, estimator=None)` -- same contract as amt_tools/inference.py:12-47: a dict of
  host arrays for ONE track -> float32 -> tensors -> batch of one -> `model.run_on_batch` -> host arrays ->
  optional estimator.  (Without the reference's four whole-dict deep copies.)
* `run_offline_batched(...)` -- new (BASELINE config 5): many equally long clips per launch, clips sharded
  over ranks round-robin (`i % world`), no collective on the data path; per-clip results equal `run_offline`'s.
* `_batched(...)` -- the loop under it, under `evaluate.validate_batched` and under `evaluate.validate_clips`: a partition through the
  model, batch by batch.  Its batches come from one of two sources: host clips that are uploaded, or `BankClips` -- clips named as
  (track, first frame) of a tracks.TrackBank / PyramidBank, whose model input the bank makes on the device.
* `run_tracks(...)` -- WHOLE resident tracks, one result per track, from equally long overlapped clips (tracks.seam_clips) through the same
  loop: behind every batch the kept columns of every output tensor are written into whole-track maps on the device (tracks.TrackMaps,
  amtx_stitch_clips); `_stitch_tracks` is that pass, shared with `evaluate.validate_tracks`.  Segment-wise inference: exact for TabCNN
  (margin >= 4) and for tracks that fit one clip, an approximation for the BiLSTMs of Onsets & Frames.
  With exact=True `_exact_tracks` runs instead: the acoustic half of the Onsets & Frames engine on the same clips, both recurrences once
  over whole tracks -- whole-track inference.  thresholds=(onset_thr, frame_thr) then cuts the rolls from the
  whole-track logits at that pair (`logits_to_map`); `evaluate.sweep_tracks` scores a grid of such pairs in one pass (section 6l).
"""

import numpy as np
import torch

from . import tools
from .dp import shard_indices

__all__ = ['run_offline', 'run_offline_batched', 'run_tracks']

KEY_LOGITS = 'logits'      # run_tracks(exact=True, keep=(..., KEY_LOGITS)): a track's raw logits


def run_offline(track_data, model, estimator=None):
    track_id = tools.unpack_dict(track_data, tools.KEY_TRACK)
    track_data = tools.dict_to_dtype(track_data, dtype=tools.FLOAT32)
    track_data = tools.dict_unsqueeze(tools.dict_to_tensor(track_data))
    predictions = tools.dict_squeeze(tools.dict_to_array(model.run_on_batch(track_data)), dim=0)
    if estimator is not None:
        predictions.update(estimator.process_track(predictions, track_id))
    return predictions


def _frame_times(model, num_frames):
    """Frame grid of the model's on-device front-end: frames * hop_length / sample_rate in float64 (FeatureModule.get_times,
    amt_tools/features/common.py:232-258).  Without a front-end module there is nothing to derive the grid from."""
    for m in getattr(model, 'frontend', []):
        mod = getattr(m, 'module', None)
        if mod is not None and hasattr(mod, 'get_hop_length') and hasattr(mod, 'get_sample_rate'):
            return (np.arange(num_frames) * mod.get_hop_length()).astype(np.float64) / float(mod.get_sample_rate())
    raise ValueError('decode_notes=True needs `times` when the model has no front-end module to take hop_length / sample_rate from')


def _model_device(model):
    """(the model's torch.device, whether the batched drivers take their GPU path for it)."""
    device = torch.device(f'cuda:{model.device}' if isinstance(model.device, int) else model.device)
    return device, device.type == 'cuda' and torch.cuda.is_available()


class BankClips(object):
    """A batch source of `_batched`: clip i is `num_frames` frames from first_frames[i] on of track track_ids[i] of `bank` (a
    tracks.TrackBank or PyramidBank).  The whole request is checked once, here, with the banks' own check and ValueError texts;
    `batch(idx)` is bank.clips of those clips -- the entry the models take under tools.KEY_AUDIO -- made on the current stream."""

    def __init__(self, bank, track_ids, first_frames, num_frames):
        from .tracks import _checked_request
        self.bank, self.num_frames = bank, int(num_frames)
        self.track_ids, self.first_frames = _checked_request(bank.frame_counts, track_ids, first_frames, num_frames)

    def __len__(self):
        return int(self.track_ids.size)

    def of(self, idx):
        """(track ids, first frames) of the clips `idx`."""
        idx = np.asarray(idx, dtype=np.int64)
        return self.track_ids[idx], self.first_frames[idx]

    def batch(self, idx):
        return self.bank.clips(*self.of(idx), self.num_frames)


@torch.no_grad()
def _batched(clips, model, batch_size, rank, world, enqueue, finish, stage_extra=None, model_extra=None):
    """The clips this rank owns through `model.run_on_batch`, `batch_size` at a time.  `clips` as for run_offline_batched, or a BankClips.
    Per batch, with idx the list of its clip indices:

      extra = stage_extra(idx)              (optional) while the batch is staged, BEFORE the batch before it runs
      pending = enqueue(idx, preds, extra)  right behind run_on_batch; anything but None
      finish(pending)                       after the NEXT batch's enqueue (the last batch: after the loop)

    model_extra(extra) (optional) -> a dictionary of further entries of the batch the model gets beside its audio or features, made from
    what stage_extra staged: ground truth for a labelled run.  Without it the model's batch is the one entry, as before.

    On a GPU model this is a three-stage pipeline: batch n+1 is uploaded on a copy stream (from pinned memory) while batch n's kernels
    run, and batch n-1 is finished on the host while the GPU is busy.  stage_extra runs inside the copy stream's context, before the
    event the model's stream waits for is recorded: what it uploads rides the same event (but has to be record_stream()ed by its reader).
    On a CPU model there are no streams; the calls come in the same order.

    A BankClips source has nothing to upload: its batch is made by the bank on the model's own stream (a descriptor table goes up, the
    audio is resident), so there is no pinned staging, no copy stream and no event for it, and stage_extra runs on the model's stream
    too.  The order of the calls is the same."""
    from_bank = isinstance(clips, BankClips)
    if not from_bank:
        clips = torch.as_tensor(np.asarray(clips) if not torch.is_tensor(clips) else clips)
    mine = shard_indices(len(clips) if from_bank else clips.shape[0], rank, world)
    key = tools.KEY_AUDIO if from_bank or clips.dim() == 2 else tools.KEY_FEATS
    # 16-bit PCM hand-over (round 6): int16 clips travel over PCIe as they are -- half the bytes of the float32 array the reference's loader makes
    # of the same file (amt_tools/tools/io.py:80-82: librosa / soundfile return sample / 32768 for 16-bit files) -- and become exactly that
    # float32 array on the device: sample * 2^-15 is exact.  Host-to-host transcription is bound by the upload (2 KB per frame as float32)
    pcm16 = not from_bank and key == tools.KEY_AUDIO and clips.dtype == torch.int16
    wire = torch.int16 if pcm16 else torch.float32
    device, on_gpu = _model_device(model)
    copy_stream = torch.cuda.Stream(device) if on_gpu and not from_bank else None
    staging = [None, None]            # pinned staging buffers (ring of two) + the event of the copy that last read them
    stage_count = [0]

    def stage(idx):
        if from_bank:
            return clips.batch(idx), (stage_extra(idx) if stage_extra else None), None
        lo, hi = int(idx[0]), int(idx[-1]) + 1
        contiguous = hi - lo == len(idx)
        if not on_gpu:
            sel = (clips[lo:hi] if contiguous else clips[torch.as_tensor(idx)]).float()
            return (sel * (1.0 / 32768.0) if pcm16 else sel), (stage_extra(idx) if stage_extra else None), None
        with torch.cuda.stream(copy_stream):
            zero_copy = contiguous and clips.is_pinned() and clips.dtype == wire
            if zero_copy:
                src = clips[lo:hi]                                # zero-copy: the caller's pinned memory is the DMA source
            else:
                slot = stage_count[0] % 2
                stage_count[0] += 1
                if staging[slot] is None:
                    staging[slot] = [torch.empty((batch_size,) + tuple(clips.shape[1:]), dtype=wire).pin_memory(), None]
                buf, last = staging[slot]
                if last is not None:
                    last.synchronize()                            # the copy that read this buffer two batches ago is done
                src = buf[:len(idx)]
                if contiguous:
                    src.copy_(clips[lo:hi])
                else:
                    torch.index_select(clips.to(wire) if clips.dtype != wire else clips, 0, torch.as_tensor(idx), out=src)
            dev = src.to(device, non_blocking=True)
            if pcm16:
                dev = dev.to(torch.float32).mul_(1.0 / 32768.0)   # on the copy stream, behind the DMA: the model's stream sees float32 audio
            extra = stage_extra(idx) if stage_extra else None
            ev = torch.cuda.Event()
            ev.record(copy_stream)
            if not zero_copy:
                staging[slot][1] = ev
        return dev, extra, ev

    batches = [mine[s:s + batch_size] for s in range(0, len(mine), batch_size)]
    nxt = stage(batches[0]) if batches else None
    pending = None
    for n, idx in enumerate(batches):
        data, extra, uploaded = nxt
        if uploaded is not None:
            main = torch.cuda.current_stream(device)
            main.wait_event(uploaded)
            # `data` was allocated from the copy stream's pool: tell the allocator that the main stream reads it, or the block
            # could be handed to the upload of batch n+2 (and overwritten by DMA) while this batch's first kernel still reads it
            data.record_stream(main)
        if n + 1 < len(batches):
            nxt = stage(batches[n + 1])
        now = enqueue(idx, model.run_on_batch({key: data, **model_extra(extra)} if model_extra else {key: data}), extra)
        if pending is not None:
            finish(pending)                                       # the GPU is busy with this batch meanwhile
        pending = now
    if pending is not None:
        finish(pending)


def run_offline_batched(clips, model, times=None, batch_size=256, rank=0, world=1, decode_notes=False, keep=None):
    """clips: (num_clips, N) float32 -- or int16 PCM -- array / CPU tensor of equally long clips (the model needs a front-end in
    `model.frontend`) or (num_clips, C, F, T) features.  Returns {clip index: predictions dict} for the clips
    this rank owns.  With decode_notes=True the note lists are decoded on the device (amtx_notes_decode; a model whose output is a
    tablature, TabCNN: stacked notes {string: (pitches, intervals)} from amtx_tab_notes, and `keep` may name KEY_MULTIPITCH for the
    collapsed pitch map of the tablature).
    `keep`: keys of the model output to bring back to the host (default: every array; () = notes only).

    The loop is `_batched`'s: on a GPU model batch i+1 is uploaded while batch i's kernels run, and batch i-1's results are brought to
    the host / assembled into note arrays while the GPU is busy."""
    out = {}

    def enqueue(idx, preds, _):
        if not decode_notes:
            return idx, preds, None
        from . import transcribe
        handle = transcribe.decode_notes_for(preds, model, times)
        if handle.strings is not None and keep is not None and tools.KEY_MULTIPITCH in keep:
            # a tablature model: the collapsed multi-pitch map only on request (amtx_tab_expand: 44 pitch rows per 6 tablature rows)
            tab = preds[tools.KEY_TABLATURE]
            if tab.is_cuda:
                preds[tools.KEY_MULTIPITCH] = tools.tab_expand(tab, model.profile, stacked=False, collapsed=True)[1]
            else:
                preds[tools.KEY_MULTIPITCH] = tools.stacked_multi_pitch_to_multi_pitch(tools.tablature_to_stacked_multi_pitch(tab, model.profile))
        return idx, preds, handle

    def finish(pending):
        idx, preds, handle = pending
        notes = handle.result() if handle is not None else None
        host = tools.dict_to_array({k: v for k, v in preds.items() if keep is None or k in keep})
        for j, i in enumerate(idx):
            out[i] = {k: v[j] for k, v in host.items() if isinstance(v, np.ndarray)}
            if notes is not None:
                out[i][tools.KEY_NOTES] = notes[j]

    _batched(clips, model, batch_size, rank, world, enqueue, finish)
    return out


def _stitch_tracks(bank, model, num_frames, margin, track_ids=None, batch_size=256, rank=0, world=1, wanted=None, model_entries=None, collect=None):
    """The stitching pass of run_tracks and evaluate.validate_tracks -> (the track ids this rank owns, in request order; the
    tracks.TrackMaps of their whole-track outputs, slot j = the j-th of those ids, or None when the rank owns no track).

    Ranks share TRACKS: position j of the request (default: every track of the bank) belongs to rank j % world.  The rank's tracks are
    covered by tracks.seam_clips(num_frames, margin); the clips run through `_batched` over a BankClips, unsharded, and the enqueue hook
    writes the kept columns of every output tensor (`wanted`: the keys to keep, default all) into the maps right behind run_on_batch, on
    the model's stream -- an output that lives in the engine's workspace is read before the next batch overwrites it.  Tracks shorter
    than a clip follow, each whole as one clip of its own length: one more pass per distinct length, through the same hook.

    The hook of a labelled pass (evaluate.validate_tracks with losses): model_entries(track ids, first frames, frames per clip, windows)
    -> further entries of the model's batch for the clips of one batch, `windows` being the (clips, 2) table {src_first, count} of the
    columns each clip keeps (seam clips: plan.kept[:, 1:3]; a short track: {0, L_t}); collect(slots, preds) is called behind every
    batch with the slot of each of its clips and the model's output.  Entries of the output that are no tensors are not stitched.

    ValueError before anything is launched: what seam_clips refuses (for the whole request, whichever rank owns the track) and a model
    that is not on a GPU."""
    from .tracks import TrackMaps, seam_clips
    seam_clips(bank.frame_counts, num_frames, margin, track_ids)                      # the whole request, checked once
    device, on_gpu = _model_device(model)
    if not on_gpu:
        raise ValueError('whole tracks are stitched from clips of device-resident tracks: the model has to be on a GPU')
    ids = np.arange(len(bank), dtype=np.int64) if track_ids is None else np.asarray(track_ids, dtype=np.int64).reshape(-1)
    mine = ids[shard_indices(len(ids), rank, world)]
    if mine.size == 0:
        return mine, None
    counts = np.asarray(bank.frame_counts, dtype=np.int64)[mine]
    plan = seam_clips(counts, num_frames, margin)                                      # over SLOTS: a track named twice has two maps
    maps = TrackMaps(counts, device)
    passes = [(int(num_frames), plan.track_ids, plan.first_frames, plan.kept)] if len(plan.track_ids) else []
    for length in sorted(set(counts[plan.short].tolist())):
        slots = plan.short[counts[plan.short] == length]
        passes.append((length, slots, np.zeros(len(slots), dtype=np.int64), np.tile(np.array([[0, 0, length]], dtype=np.int64), (len(slots), 1))))
    for frames, slots, firsts, kept in passes:
        tables = {}                        # rows of a map -> its descriptor table, on the host and on the device: uploaded once per pass

        def enqueue(idx, preds, _):
            lo, hi = int(idx[0]), int(idx[-1]) + 1                                     # unsharded: a batch is a run of clips
            for key, value in preds.items():
                if not torch.is_tensor(value) or (wanted is not None and key not in wanted):
                    continue
                if value.dim() < 2 or value.shape[0] != hi - lo or value.shape[-1] != frames:
                    raise ValueError(f"the model output '{key}' is no (batch, rows..., num_frames) map: {tuple(value.shape)} for {hi - lo} clips of {frames} frames")
                if key not in maps.keys:
                    maps.add(key, value.shape[1:-1], value.dtype)
                rows = maps.rows(key)
                if rows not in tables:
                    desc = maps.descriptors(key, slots, kept)
                    tables[rows] = desc, torch.from_numpy(desc).to(device)
                desc, desc_dev = tables[rows]
                maps.stitch(key, value, desc[lo:hi], desc_dev[lo:hi])
            if collect is not None:
                collect(slots[lo:hi], preds)
            return idx

        def stage_extra(idx):
            lo, hi = int(idx[0]), int(idx[-1]) + 1
            return model_entries(mine[slots[lo:hi]], firsts[lo:hi], frames, kept[lo:hi, 1:3])

        _batched(BankClips(bank, mine[slots], firsts, frames), model, batch_size, 0, 1, enqueue, lambda pending: None,
                 stage_extra if model_entries else None, (lambda entries: entries) if model_entries else None)
    return mine, maps


def _check_exact(model, margin):
    """What exact=True asks of the model and the margin: ValueError / NotImplementedError before anything is launched."""
    from .models import OnsetsFrames, TabCNN
    if isinstance(model, TabCNN):
        raise ValueError('exact=True is for the BiLSTMs of Onsets & Frames: TabCNN has no recurrence, margin 4 is already exact for it')
    if not isinstance(model, OnsetsFrames):
        raise ValueError(f'exact=True runs the two-phase Onsets & Frames engine: OnsetsFrames / OnsetsFrames2, not {type(model).__name__}')
    if model.training:
        raise ValueError('exact=True runs the inference engine: the model has to be in eval mode')
    if int(margin) < 3:
        raise ValueError(f'margin={int(margin)}: the convolutions of Onsets & Frames reach 3 frames, exact=True needs margin >= 3')


class _AcousticPhase(object):
    """What `_batched` takes for a model in the exact route: run_on_batch is the engine's acoustic phase on the batch, gathering into the
    packed buffers of the current language pass (`aim`)."""

    def __init__(self, model):
        self.model, self.device = model, model.device
        self.aim = None                      # (the pass's gather table on the host, on the device, total rows, rows_e, rows_pitch)
        self.at = 0                          # the pass's clips so far: _batched's batches are runs of clips

    def run_on_batch(self, batch):
        table, table_dev, total_rows, rows_e, rows_pitch = self.aim
        n = batch[tools.KEY_AUDIO].num_clips
        self.model.acoustic_rows_on_batch(batch, table[self.at:self.at + n], table_dev[self.at:self.at + n], total_rows, rows_e, rows_pitch)
        self.at += n
        return n


def _exact_tracks(bank, model, num_frames, margin, track_ids=None, batch_size=256, rank=0, world=1, want_logits=False, max_rows=1 << 18):
    """The pass of run_tracks(exact=True) and evaluate.validate_tracks(exact=True): _stitch_tracks' return contract, (the track ids this
    rank owns, in request order; the tracks.TrackMaps of their whole-track outputs) -- and, with want_logits, a third value: per slot
    {key: the track's (1, L_t, n_out) logits}.

    The plan is tracks.seam_clips, as for _stitch_tracks, and short tracks run as clips of their own length with the whole clip kept.  But
    the clips run only the engine's ACOUSTIC phase (convolutions, fc1, the pitch head), whose kept rows are gathered into packed rows; both
    BiLSTM recurrences then run once over the whole tracks of a LANGUAGE pass, which writes the piano rolls straight into the maps.  From
    margin 3 on the kept rows are the track's own, so this is whole-track inference.  A language pass holds tracks in request order until the
    next would bring it above `max_rows` rows (a memory knob); a longer track runs alone and is never split.

    ValueError before anything is launched: _check_exact's, what seam_clips refuses and a model that is not on a GPU."""
    from .tracks import TrackMaps, gather_table, seam_clips, sequence_table, track_groups
    _check_exact(model, margin)
    seam_clips(bank.frame_counts, num_frames, margin, track_ids)                      # the whole request, checked once
    device, on_gpu = _model_device(model)
    if not on_gpu:
        raise ValueError('whole tracks are run from clips of device-resident tracks: the model has to be on a GPU')
    ids = np.arange(len(bank), dtype=np.int64) if track_ids is None else np.asarray(track_ids, dtype=np.int64).reshape(-1)
    mine = ids[shard_indices(len(ids), rank, world)]
    if mine.size == 0:
        return (mine, None, None) if want_logits else (mine, None)
    counts = np.asarray(bank.frame_counts, dtype=np.int64)[mine]
    engine = model._get_engine(device)
    n_out = engine.n_out
    keys = [tools.KEY_ONSETS, tools.KEY_MULTIPITCH] + ([tools.KEY_OFFSETS] if model.has_offsets else [])
    maps = TrackMaps(counts, device)
    for key in keys:
        maps.add(key, (n_out,), torch.float32)
    phase = _AcousticPhase(model)
    logits = [None] * len(mine)
    for lo, hi in track_groups(counts, max_rows):
        row0, seqs = sequence_table(counts[lo:hi])
        total = int(counts[lo:hi].sum())
        rows_e = torch.empty(engine.rows_e_bytes(total), dtype=torch.uint8, device=device)
        rows_pitch = torch.empty((total, n_out), dtype=torch.float32, device=device)
        plan = seam_clips(counts[lo:hi], num_frames, margin)                           # over the SLOTS of this pass
        passes = [(int(num_frames), plan.track_ids, plan.first_frames, plan.kept)] if len(plan.track_ids) else []
        for length in sorted(set(counts[lo:hi][plan.short].tolist())):
            slots = plan.short[counts[lo:hi][plan.short] == length]
            passes.append((length, slots, np.zeros(len(slots), dtype=np.int64), np.tile(np.array([[0, 0, length]], dtype=np.int64), (len(slots), 1))))
        for frames, slots, firsts, kept in passes:
            table = gather_table(row0, slots, kept)
            phase.aim, phase.at = (table, torch.from_numpy(table).to(device), total, rows_e, rows_pitch), 0
            _batched(BankClips(bank, mine[lo + slots], firsts, frames), phase, batch_size, 0, 1, lambda idx, done, _: done, lambda pending: None)
        first = int(maps.base[keys[0]][lo])                                            # n_out * the rows in front of this pass
        out = {key: maps.flat(key)[first:first + n_out * total] for key in keys}
        packed = engine.language_rows(rows_e, rows_pitch, seqs, torch.from_numpy(seqs).to(device), total, out, want_logits=want_logits)
        if want_logits:
            for j in range(lo, hi):
                at, L = int(row0[j - lo]), int(counts[j])
                logits[j] = {key: rows[at:at + L].unsqueeze(0) for key, rows in packed.items()}
    return (mine, maps, logits) if want_logits else (mine, maps)


def _check_thresholds(values, what, limit=None):
    """Decision thresholds as a list of floats: ValueError for none, a non-finite or negative one (amtx_pianoroll_fwd reads a negative
    threshold as "no cut") and, with `limit`, more than that many."""
    values = [float(v) for v in np.asarray(values, dtype=np.float64).reshape(-1)]
    if not values:
        raise ValueError(f'{what}: at least one threshold')
    if not all(np.isfinite(v) and v >= 0 for v in values):
        raise ValueError(f'{what}: thresholds are finite and not negative, not {values}')
    if limit is not None and len(values) > limit:
        raise ValueError(f'{what}: {len(values)} thresholds, at most {limit}')
    return values


def logits_to_map(logits, threshold, out=None):
    """A track's (1, L, n_out) float32 logits -> its (1, n_out, L) map through amtx_pianoroll_fwd: sigmoid, transpose and
    `s < threshold ? 0 : 1` -- the expression behind every roll of the package; threshold < 0: the probabilities themselves.
    `out`: a contiguous (1, n_out, L) float32 tensor to write into."""
    from . import _lib
    assert logits.dim() == 3 and logits.is_cuda and logits.dtype == torch.float32 and logits.stride(2) == 1
    B, L, n_out = logits.shape
    assert B == 1 or logits.stride(0) == L * logits.stride(1)
    if out is None:
        out = torch.empty((B, n_out, L), dtype=torch.float32, device=logits.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == B * n_out * L
    _lib.call('amtx_pianoroll_fwd', logits, logits.stride(1), 0, B, L, n_out, float(threshold), out, device=logits.device)
    return out


@torch.no_grad()
def run_tracks(bank, model, num_frames, margin, track_ids=None, batch_size=256, keep=None, decode_notes=False, times=None, rank=0, world=1, thresholds=None,
               exact=False):
    """Transcribe WHOLE tracks of `bank` (a tracks.TrackBank / PyramidBank) from overlapped clips of `num_frames` frames: returns
    {track id: predictions} for the tracks this rank owns (position j of `track_ids`, default every track, belongs to rank j % world).
    A track's predictions are host arrays (rows..., L_t) per output key, L_t the track's own frame count, and with decode_notes=True its
    notes under tools.KEY_NOTES, decoded on the device from the track's stitched maps alone with the frame grid of its own length
    (`times`: None for the grid of the model's front-end, else indexed by track id: times[t] is the (L_t,) grid of track t).
    `keep` as for run_offline_batched (default: every array; () = notes only; KEY_MULTIPITCH of a tablature model on request).

    Of each clip only the frames at least `margin` frames from a clip edge that is not a track edge are kept (tracks.seam_clips), so this
    is SEGMENT-WISE inference.  For TabCNN, whose frames see 9 frames of features, margin >= 4 gives the whole-track result.  For
    Onsets & Frames the convolutions are exact from margin 3 on in exact arithmetic, but every BiLSTM starts anew at each clip edge and
    sees `margin` frames of context instead of the whole track: an approximation, measured in README; a track that fits one clip is run
    whole and is exact.  `margin` has no default.

    exact=True (OnsetsFrames / OnsetsFrames2 in eval mode on a GPU, margin >= 3): WHOLE-TRACK inference -- the clips run the engine's
    acoustic phase only, both BiLSTMs run once over every whole track (`_exact_tracks`).  `keep` may then also name 'logits': the
    track's raw logits {key: (L_t, n_out)} come back under that key.

    thresholds=(onset_thr, frame_thr) (exact=True only, else ValueError): `onsets` and `multi_pitch` are cut from the whole-track logits
    at these thresholds instead of 0.5 (logits_to_map), before notes are decoded -- the pair evaluate.sweep_tracks scores.  None: 0.5."""
    from . import transcribe
    decoder_keys = (tools.KEY_ONSETS, tools.KEY_MULTIPITCH, tools.KEY_TABLATURE)
    wanted = None if keep is None else set(keep) | (set(decoder_keys) if decode_notes else set())
    if keep is not None and tools.KEY_MULTIPITCH in keep:
        wanted.add(tools.KEY_TABLATURE)                        # a tablature model's pitch map is expanded from its stitched tablature
    logits = None
    if thresholds is not None:
        if not exact:
            raise ValueError('thresholds are applied to the whole-track logits of the exact route: exact=True')
        if np.size(thresholds) != 2:
            raise ValueError('thresholds: the pair (onset threshold, frame threshold)')
        thresholds = _check_thresholds(thresholds, 'run_tracks')
    if exact:
        want_logits = keep is not None and KEY_LOGITS in keep
        mine, maps, *rest = _exact_tracks(bank, model, num_frames, margin, track_ids, batch_size, rank, world, want_logits or thresholds is not None)
        if thresholds is not None and maps is not None:
            # the rolls again, from the same logits at the chosen thresholds, over the engine's own (cut at 0.5), before anything reads them
            for j in range(len(mine)):
                for key, thr in zip((tools.KEY_ONSETS, tools.KEY_MULTIPITCH), thresholds):
                    logits_to_map(rest[0][j][key], thr, out=maps.track(j, key))
        logits = rest[0] if want_logits else None
    else:
        mine, maps = _stitch_tracks(bank, model, num_frames, margin, track_ids, batch_size, rank, world, wanted)
    out = {}
    if maps is None:
        return out
    host = {key: maps.host(key) for key in maps.keys if keep is None or key in keep}
    want_pitch = keep is not None and tools.KEY_MULTIPITCH in keep and tools.KEY_MULTIPITCH not in maps.keys and tools.KEY_TABLATURE in maps.keys

    def collect(j, handle):
        out[int(mine[j])][tools.KEY_NOTES] = handle.result()[0]

    pending = None
    for j, t in enumerate(mine.tolist()):
        out[t] = {key: arrays[j] for key, arrays in host.items()}
        if logits is not None:
            out[t][KEY_LOGITS] = {key: value[0].cpu().numpy() for key, value in logits[j].items()}
        if want_pitch:                                         # the collapsed pitch map of a tablature (amtx_tab_expand), as run_offline_batched
            out[t][tools.KEY_MULTIPITCH] = tools.tab_expand(maps.track(j, tools.KEY_TABLATURE), model.profile, stacked=False, collapsed=True)[1][0].cpu().numpy()
        if decode_notes:
            preds = {key: maps.track(j, key) for key in maps.keys}
            handle = transcribe.decode_notes_for(preds, model, None if times is None else times[t])
            if pending is not None:
                collect(*pending)                              # the GPU decodes track j meanwhile
            pending = j, handle
    if pending is not None:
        collect(*pending)
    return out
