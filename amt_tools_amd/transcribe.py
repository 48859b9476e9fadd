"""
Note / pitch-list estimation for the hot path's output, mirroring the estimators of amt_tools/transcribe.py
that the paper scripts attach to Onsets & Frames (examples/papers/of_1.py:150-155):

* `NoteTranscriber.estimate(raw_output)`  -- amt_tools/transcribe.py:717-763 (+ StackedNoteTranscriber :420-481,
  tools.multi_pitch_to_notes tools/utils.py:369-471): binary (88,T) maps + times -> (K,3) rows
  [onset_s, offset_s, midi_pitch].  Bit-exact with the reference, including the row order among equal onsets
  (the reference argsorts by onset three times with NumPy's default, unstable sort; the same three passes run here).
  The per-event Python `while` walk is replaced by a vectorised next-stop scan (host arrays) or by the HIP kernel
  behind `amtx_notes_decode` (device tensors, whole batches: `decode_notes_batch`).
* `PitchListWrapper.estimate` -- amt_tools/transcribe.py:1038-1071, tools.multi_pitch_to_pitch_list utils.py:1023-1062.
* The guitar pipeline of examples/papers/tabcnn.py:90-91 -- `ComboEstimator` (transcribe.py:88-128), `TablatureWrapper` (:1097-1145),
  `StackedMultiPitchCollapser` (:1173-1201) -- and `StackedNoteTranscriber` (:373-481) for note lists per string.  On TabCNN's
  device output the maps come from `amtx_tab_expand` and the notes straight from the tablature (`decode_tab_notes_batch_async`,
  `amtx_tab_notes`: on one string a note is a run of one class), bit-exact with the host classes.

The reference's own estimators keep working on this package's model output unchanged; these classes exist so a
batched offline driver (BASELINE config 5) does not spend its time in per-note Python loops.
"""

import numpy as np

from . import _lib, tools

__all__ = ['NoteTranscriber', 'PitchListWrapper', 'multi_pitch_to_notes', 'decode_notes_batch', 'decode_notes_grid_async', 'decode_notes_grid',
           'cut_activations', 'estimate_hop_length', 'inhibit_activations',
           'ComboEstimator', 'TablatureWrapper', 'StackedMultiPitchCollapser', 'StackedNoteTranscriber', 'decode_tab_notes_batch_async',
           'decode_tab_notes_batch']


def estimate_hop_length(times):
    """Spacing of a (possibly gappy) frame grid: the median of those steps that equal their predecessor, i.e. steps inside a
    regular run (behaviour contract: amt_tools/tools/utils.py:3197-3229, including the 1e-8 absolute tolerance of np.isclose
    against zero and ValueError for grids that are empty or have no two equal consecutive steps)."""
    grid = np.sort(np.asarray(times).ravel())            # dtype kept: run_offline hands float32 grids over (inference.py:36)
    if grid.size == 0:
        raise ValueError('hop length of an empty time grid is undefined')
    steps = grid[1:] - grid[:-1]
    change = steps[1:] - steps[:-1]                      # == np.diff(grid, n=2)
    regular = steps[1:][np.abs(change) <= 1e-8]          # a step counts when it repeats the step before it
    if regular.size == 0:
        raise ValueError('time grid has no regularly spaced stretch to take a hop length from')
    return np.median(regular)


def _impulses(x):
    """Positive first difference along time, first frame counts (tools/utils.py:2381-2412), as booleans."""
    x = np.asarray(x)
    first = x[..., :1] > 0
    return np.concatenate([first, (x[..., 1:] - x[..., :-1]) > 0], axis=-1)


def _sort_by_onset(batched):
    return batched[np.argsort(batched[..., 0])]


def _extend_times(times):
    """The frame grid plus one more frame (tools/utils.py:441-442): offsets may point one past the last frame."""
    return np.append(times, times[-1] + estimate_hop_length(times))


def _events_to_notes(pitch_idcs, on_frames, off_frames, times, low, times_ext=None, min_duration=None, sorts=3):
    """(key, onset frame, offset frame) events in np.nonzero order -> (K,3) rows ordered like the reference.
    `times_ext` = _extend_times(times) when the caller already has it (one grid shared by a whole batch).
    `min_duration`: the reference's duration filter (transcribe.py:36-80), which sits between its first and second sort:
    notes shorter than the threshold go (threshold 0: zero-length notes go).
    `sorts`: how many of the reference's argsorts the caller's pipeline runs -- three for NoteTranscriber, two for
    StackedNoteTranscriber (multi_pitch_to_notes and notes_to_stacked_notes; no stacked_notes_to_notes)."""
    if times_ext is None:
        times_ext = _extend_times(times)
    if len(pitch_idcs) == 0:
        return np.empty([0, 3])
    # sort_notes in multi_pitch_to_notes (utils.py:469), notes_to_stacked_notes (:745), stacked_notes_to_notes (:531): three
    # successive argsorts by onset with NumPy's default (unstable) sort.  The same three argsorts run here on the 1-D onset
    # column only and their permutations are composed; the (K,3) rows are gathered once (same result as re-indexing the whole
    # array three times, 40 % less host time per clip -- the host assembly bounds the batched transcription driver).
    # float64 keys whatever the grid's dtype: the reference's sort runs on the (K, 3) array np.concatenate built from the float32 / float64
    # intervals and the int64 pitches, i.e. on float64 (utils.py:135-164) -- and NumPy's unstable sort orders ties differently per key width
    onset_t = times_ext[on_frames].astype(np.float64)
    perm = np.argsort(onset_t)
    if min_duration is not None:
        dur = times_ext[np.asarray(off_frames)[perm]] - onset_t[perm]
        perm = perm[dur >= min_duration] if min_duration else perm[dur > min_duration]
        if len(perm) == 0:
            return np.empty([0, 3])
    for _ in range(sorts - 1):
        perm = perm[np.argsort(onset_t[perm])]
    batched = np.empty((len(perm), 3))
    batched[:, 0] = onset_t[perm]
    batched[:, 1] = times_ext[np.asarray(off_frames)[perm]]
    batched[:, 2] = np.asarray(pitch_idcs)[perm] + low
    return batched


def inhibit_activations(activations, times, window_length):
    """Keep an activation only if no KEPT activation of the same row started less than `window_length` seconds before it
    (behaviour contract: amt_tools/tools/utils.py:2987-3038, which rescans the whole map once per kept activation).  Per row the
    non-zero frames are walked once: keep the first, jump with one binary search to the first frame at or past its time +
    window, keep the next non-zero from there on.  Returns a new {0,1} map of the input's dtype."""
    activations = np.asarray(activations)
    times = np.asarray(times)
    out = np.zeros_like(activations)
    rows, frames = np.nonzero(activations)
    bounds = np.searchsorted(rows, np.arange(activations.shape[0] + 1))
    for r in range(activations.shape[0]):
        fr = frames[bounds[r]:bounds[r + 1]]
        i = 0
        while i < len(fr):
            out[r, fr[i]] = 1
            release = np.searchsorted(times, times[fr[i]] + window_length, side='left')      # first frame outside the window
            i = np.searchsorted(fr, max(release, fr[i] + 1), side='left')
    return out


def multi_pitch_to_notes(multi_pitch, times, low=tools.DEFAULT_PIANO_LOWEST_PITCH, onsets=None, min_duration=None, sorts=3):
    """Vectorised tools.multi_pitch_to_notes for host arrays: returns (K,3) batched notes."""
    multi_pitch = np.asarray(multi_pitch)
    if onsets is None:
        imp = _impulses(multi_pitch)
        active = multi_pitch != 0
    else:
        onsets = np.asarray(onsets)
        imp = _impulses(onsets)
        active = np.logical_or(onsets, multi_pitch)
    T = multi_pitch.shape[-1]
    stop = np.logical_or(~active, imp)
    idx = np.where(stop, np.arange(T), T)
    nearest = np.minimum.accumulate(idx[..., ::-1], axis=-1)[..., ::-1]          # nearest stop at >= t
    after = np.concatenate([nearest[..., 1:], np.full(nearest.shape[:-1] + (1,), T)], axis=-1)   # strictly after t
    pitch_idcs, frame_idcs = imp.nonzero()
    return _events_to_notes(pitch_idcs, frame_idcs, after[pitch_idcs, frame_idcs], np.asarray(times), low, min_duration=min_duration,
                            sorts=sorts)


from ._order_pool import order_batch, reference_order as _reference_order     # noqa: E402  (the reference's three unstable argsorts)


_GRIDS = {}        # (grid dtype, shape, digest, device) -> the extended time grid / release table on the device
_RELEASE = {}      # (grid dtype, shape, digest, window) -> int32 release table of amtx_tab_notes
_D2H_STREAMS = {}  # device -> the stream note rows are copied to the host on


def _digest_cached(cache, array, extra, make):
    """cache[dtype, shape and digest of `array`, + extra], made by make(array) on a miss; at 16 entries the oldest ONE goes.  Keyed on a
    digest, not on the bytes themselves (a (B, T) grid is megabytes per batch)."""
    import hashlib
    array = np.ascontiguousarray(array)
    key = (array.dtype.str, array.shape, hashlib.blake2b(array.view(np.uint8).reshape(-1), digest_size=16).digest()) + extra
    value = cache.get(key)
    if value is None:
        if len(cache) >= 16:
            cache.pop(next(iter(cache)))
        value = cache[key] = make(array)
    return value


def _grid_on_device(ext, dev):
    """The extended time grid as a device tensor, uploaded once per distinct grid.  The upload is a copy from pageable memory on the
    current stream: it returns only when every kernel enqueued before it has finished, so one upload per batch made the batched driver wait
    for its own model forward before it could go on to the previous batch's host work (4 x 8 ms per 2048 clips; config 5's host-to-host
    rate went from 14 to 25 M frames/s with the grid cached)."""
    import torch
    t = _digest_cached(_GRIDS, ext, (str(dev),), lambda a: torch.from_numpy(a).to(dev))
    # the decoder's kernels read the grid on the caller's current stream, which need not be the stream it was allocated on: tell the
    # caching allocator, so that an evicted grid (its memory is only reused behind the streams recorded here) is not handed out again
    # while those kernels are still queued
    t.record_stream(torch.cuda.current_stream(t.device))
    return t


def _extended_grid(times, T):
    """One (T,) grid or a (B, T) array of grids -> (the grid(s) plus one more frame in float64, the row stride the kernels take: 0 = one
    grid shared by the batch).  float32 grids (run_offline) convert exactly, as in the reference's float64 rows."""
    times = np.asarray(times)
    ext = (_extend_times(times) if times.ndim == 1 else np.stack([_extend_times(t) for t in times])).astype(np.float64)
    assert ext.shape[-1] == T + 1
    return np.ascontiguousarray(ext), 0 if times.ndim == 1 else ext.shape[1]


def _side_stream(device):
    """The stream of `device` that results are copied to the host on, behind an event of the work they wait for: on the caller's stream
    the copies would queue behind whatever the caller has enqueued since (the batched drivers: the NEXT batch's whole forward pass)."""
    import torch
    side = _D2H_STREAMS.get(str(device))
    if side is None:
        side = _D2H_STREAMS[str(device)] = torch.cuda.Stream(device)
    return side


class _PendingRows(object):
    """Device half of a decoder already enqueued: one dense (E, 3) float64 array of note rows, the per-group offsets into it, for the
    piano decoder the rows' onset column.  Lets a caller enqueue the next batch's kernels before paying for this batch's host work.
    `strings`: note groups per clip of a tablature decoder, None for batched notes."""

    def __init__(self, rows, offsets, retry, onset_col=None, strings=None):
        self._rows, self._offsets, self._retry, self._onset, self.strings = rows, offsets, retry, onset_col, strings
        import torch
        self._done = torch.cuda.Event()
        self._done.record(torch.cuda.current_stream(rows.device))

    def device_rows(self):
        """(rows (E, 3) float64, offsets int32): the dense note rows and the offsets table as the decoder left them on the device, before
        result()'s host work.  offsets[-1] > len(rows) means the first buffer was too small: the rows beyond it were not written, and
        fetch() decodes once more into a buffer of the exact size."""
        return self._rows, self._offsets

    def fetch(self):
        """(rows (total, 3), offsets, onset column or None) on the host, copied on the side stream behind the decoder's event."""
        import torch
        side = _side_stream(self._rows.device)
        side.wait_event(self._done)
        with torch.cuda.stream(side):
            off = self._offsets.cpu().numpy()
            total = int(off[-1])
            if total > self._rows.shape[0]:             # more notes than the first buffer held: once more with the exact size
                again = self._retry(total)              # enqueued on this side stream, behind the decoder's event
                self._rows, self._offsets, self._onset, off = again._rows, again._offsets, again._onset, again._offsets.cpu().numpy()
            rows = self._rows[:total].cpu().numpy()
            onset = self._onset[:total].cpu().numpy() if self._onset is not None else None
        return rows, off, onset


class _PendingNotes(_PendingRows):
    """amtx_notes_decode + amtx_notes_rows: rows in np.nonzero order per clip; `result()` brings them to the host and applies the
    reference's row order clip by clip."""

    def result(self):
        rows, off, onset = self.fetch()
        # the reference's row order per clip: NumPy's own argsort, three times (amt_tools_amd/_order_pool.py: a few helper processes for
        # whole batches, in-process for small ones)
        return order_batch(rows, onset, off, len(off) - 1)


class _HostNotes(object):
    """The same handle for notes that are decoded on the host, `result()` does it all.  Here: piano rolls of a CPU model, clip by clip."""

    def __init__(self, *args, strings=None):
        self._args, self.strings = args, strings

    def device_rows(self):
        """None: this handle has no rows on the device."""
        return None

    def result(self):
        onsets, multi_pitch, t, low = self._args
        mp, on = multi_pitch.numpy(), onsets.numpy()
        return [multi_pitch_to_notes(mp[b], t if np.ndim(t) == 1 else t[b], low, on[b]) for b in range(mp.shape[0])]


def decode_notes_batch_async(onsets, multi_pitch, times, low=tools.DEFAULT_PIANO_LOWEST_PITCH, rows_capacity=None):
    """Enqueue the device decoder and return a handle; `handle.result()` -> list of B (K,3) float64 arrays.  (B,88,T) fp32 CUDA tensors
    (onsets may be None); `times` is one (T,) grid or a (B,T) array.  Two C-ABI calls: amtx_notes_decode (event walk per key) and
    amtx_notes_rows (compaction into the reference's batched-notes rows, frames -> seconds through the extended grid)."""
    import torch
    assert multi_pitch.is_cuda and multi_pitch.dim() == 3
    B, K, T = multi_pitch.shape
    dev = multi_pitch.device
    multi_pitch = multi_pitch.contiguous().float()
    if onsets is not None:
        onsets = onsets.contiguous().float()
    ext, stride = _extended_grid(times, T)
    ext_d = _grid_on_device(ext, dev)
    cap = T // 2 + 2
    pairs = torch.empty((B * K, cap, 2), dtype=torch.int32, device=dev)
    counts = torch.empty((B * K,), dtype=torch.int32, device=dev)
    _lib.call('amtx_notes_decode', onsets, multi_pitch, B, K, T, cap, pairs, counts, device=dev)
    # 1024 notes per clip on average covers any realistic transcription (the synthetic bench clips decode to ~400); a denser batch is
    # caught in result() through the total the device reports and decoded again into a buffer of the exact size
    return _rows_of_events(pairs, counts, B, K, cap, ext_d, stride, low, int(rows_capacity) if rows_capacity else max(B * 1024, 1 << 14))


def _rows_of_events(pairs, counts, groups, K, cap, ext_d, stride, low, capacity):
    """amtx_notes_rows on a decoder's event buffers (`groups` clips of K keys, `cap` events per row) -> the _PendingNotes of its rows; the
    handle's retry runs the same pass into a buffer of another capacity."""
    import torch
    dev = pairs.device

    def rows_pass(capacity):
        rows = torch.empty((capacity, 3), dtype=torch.float64, device=dev)
        onset_col = torch.empty((capacity,), dtype=torch.float64, device=dev)
        offsets = torch.empty((groups + 1,), dtype=torch.int32, device=dev)
        _lib.call('amtx_notes_rows', pairs, counts, groups, K, cap, ext_d, stride, int(low), rows, onset_col, capacity, offsets, device=dev)
        return _PendingNotes(rows, offsets, rows_pass, onset_col)

    return rows_pass(capacity)


def decode_notes_batch(onsets, multi_pitch, times, low=tools.DEFAULT_PIANO_LOWEST_PITCH):
    """Device path: (B,88,T) fp32 CUDA tensors (onsets may be None) -> list of B (K,3) float64 arrays.
    `times` is one (T,) grid shared by the batch or a (B,T) array."""
    return decode_notes_batch_async(onsets, multi_pitch, times, low).result()


def cut_activations(prob, threshold):
    """Host restatement of the device cut (`s < thr ? 0 : 1` on float32): a {0, 1} float32 map; equality and NaN are active."""
    return (~(np.asarray(prob, dtype=np.float32) < np.float32(threshold))).astype(np.float32)


def _threshold_pairs(pairs):
    pairs = np.ascontiguousarray(pairs, dtype=np.float32).reshape(-1, 2)
    if len(pairs) == 0:
        raise ValueError('at least one (onset threshold, frame threshold) pair')
    return pairs


class _HostGridNotes(object):
    """decode_notes_grid_async for host maps: multi_pitch_to_notes on every pair's cut rolls, clip by clip."""
    strings = None

    def __init__(self, on_prob, mp_prob, times, pairs, low):
        self._args = on_prob, mp_prob, times, pairs, low

    def device_rows(self):
        return None

    def result(self):
        on_prob, mp_prob, times, pairs, low = self._args
        out = []
        for on_thr, mp_thr in pairs:
            mp = cut_activations(mp_prob, mp_thr)
            on = cut_activations(on_prob, on_thr) if on_prob is not None else None
            out += [multi_pitch_to_notes(mp[b], times, low, None if on is None else on[b]) for b in range(mp.shape[0])]
        return out


class _PendingGridNotes(object):
    """The handle of decode_notes_grid_async on the device: `chunks` = [(first pair, number of pairs, _PendingNotes)], each chunk's groups
    being (pair - first pair) * B + clip.  One chunk unless the event buffer of all pairs would exceed the budget."""
    strings = None

    def __init__(self, chunks):
        self.chunks = chunks

    def device_rows(self):
        """_PendingRows.device_rows over all P * B groups.  One chunk: its own buffers, nothing waits.  Several: the chunks' rows are
        fetched (this waits for the decoder) and put behind one another."""
        import torch
        if len(self.chunks) == 1:
            return self.chunks[0][2].device_rows()
        rows, offsets, at = [], [], 0
        for _, _, handle in self.chunks:
            handle.fetch()                                   # decodes once more when the chunk's first buffer was too small
            r, off = handle.device_rows()
            total = int(off[-1])
            rows.append(r[:total])
            offsets.append(off[:-1] + at)
            at += total
        last = torch.full((1,), at, dtype=torch.int32, device=rows[0].device)
        return torch.cat(rows + ([rows[0].new_zeros((1, 3))] if at == 0 else [])), torch.cat(offsets + [last])

    def result(self):
        return [notes for _, _, handle in self.chunks for notes in handle.result()]


def decode_notes_grid_async(on_prob, mp_prob, times, pairs, low=tools.DEFAULT_PIANO_LOWEST_PITCH, rows_capacity=None, event_bytes=1 << 30):
    """decode_notes_batch_async for a table of threshold pairs: `on_prob` (or None) and `mp_prob` are (B, K, T) PROBABILITY maps, `pairs` a
    (P, 2) table of {onset threshold, frame threshold}; `handle.result()` -> list of P * B (N, 3) float64 arrays, entry p * B + b being
    what decode_notes_batch gives for clip b on the maps cut at pair p (`prob < thr ? 0 : 1`; without on_prob the onsets are derived
    from the frame roll and a pair's first entry is unused).  `times`: ONE (T,) grid shared by all clips; a (B, T) array is a ValueError.

    Device tensors: amtx_notes_decode_grid cuts and walks all pairs of a chunk in one launch, amtx_notes_rows takes its output with
    P_chunk * B clips.  The pairs are chunked so that the event buffer, P_chunk * B * K * capacity * 8 bytes, stays within `event_bytes`
    (at least one pair per chunk); `rows_capacity`: note rows of a chunk's first buffer.  Host arrays / CPU tensors: a loop over
    multi_pitch_to_notes."""
    import torch
    pairs_d = None
    if torch.is_tensor(pairs) and pairs.is_cuda:             # a table already on the device (a driver uploads it once)
        pairs_d = pairs.reshape(-1, 2).float().contiguous()
        if pairs_d.shape[0] == 0:
            raise ValueError('at least one (onset threshold, frame threshold) pair')
    else:
        pairs = _threshold_pairs(pairs.numpy() if torch.is_tensor(pairs) else pairs)
    if np.ndim(times) != 1:
        raise ValueError('decode_notes_grid takes one (T,) time grid for all clips')
    if not (torch.is_tensor(mp_prob) and mp_prob.is_cuda):
        host = lambda m: None if m is None else (m.numpy() if torch.is_tensor(m) else np.asarray(m))     # noqa: E731
        return _HostGridNotes(host(on_prob), host(mp_prob), np.asarray(times), pairs if pairs_d is None else pairs_d.cpu().numpy(), low)
    assert mp_prob.dim() == 3 and (on_prob is None or (on_prob.is_cuda and on_prob.shape == mp_prob.shape))
    B, K, T = mp_prob.shape
    dev = mp_prob.device
    mp_prob = mp_prob.contiguous().float()
    if on_prob is not None:
        on_prob = on_prob.contiguous().float()
    ext, stride = _extended_grid(times, T)
    ext_d = _grid_on_device(ext, dev)
    cap = T // 2 + 2
    per_chunk = max(1, int(event_bytes) // (B * K * cap * 8))
    if pairs_d is None:
        pairs_d = torch.from_numpy(pairs).to(dev)
    P = pairs_d.shape[0]
    chunks = []
    for p0 in range(0, P, per_chunk):
        n = min(per_chunk, P - p0)
        events = torch.empty((n * B * K, cap, 2), dtype=torch.int32, device=dev)
        counts = torch.empty((n * B * K,), dtype=torch.int32, device=dev)
        _lib.call('amtx_notes_decode_grid', on_prob, mp_prob, B, K, T, pairs_d[p0:p0 + n], n, cap, events, counts, device=dev)
        # the first buffer: T / 2 notes per (pair, clip) on average, at least the 1024 of decode_notes_batch_async -- a whole track is
        # longer than a clip, and a low threshold decodes to several times the notes of 0.5; 32 bytes per row, beside K * cap * 8 of events
        chunks.append((p0, n, _rows_of_events(events, counts, n * B, K, cap, ext_d, stride, low,
                                              int(rows_capacity) if rows_capacity else max(n * B * max(1024, T // 2), 1 << 14))))
    return _PendingGridNotes(chunks)


def decode_notes_grid(on_prob, mp_prob, times, pairs, low=tools.DEFAULT_PIANO_LOWEST_PITCH, rows_capacity=None, event_bytes=1 << 30):
    """decode_notes_grid_async(...).result()."""
    return decode_notes_grid_async(on_prob, mp_prob, times, pairs, low, rows_capacity, event_bytes).result()


class NoteTranscriber(object):
    """amt_tools.transcribe.NoteTranscriber (transcribe.py:717-785 over StackedNoteTranscriber :373-481), all constructor options:
    `inhibition_window` (seconds after a kept onset in which the same pitch cannot start again) acts -- exactly as in the
    reference, transcribe.py:463-468 -- only when the model supplies no onset map (the onsets are then the inhibited positive
    first difference of the multi-pitch map); `minimum_duration` drops shorter notes (0: zero-length notes)."""

    def __init__(self, profile, inhibition_window=None, minimum_duration=None, multi_pitch_key=None, onsets_key=None,
                 offsets_key=None, estimates_key=None, save_dir=None):
        self.inhibition_window = inhibition_window
        self.minimum_duration = minimum_duration
        self.profile = profile
        self.multi_pitch_key = tools.KEY_MULTIPITCH if multi_pitch_key is None else multi_pitch_key
        self.onsets_key = tools.KEY_ONSETS if onsets_key is None else onsets_key
        self.estimates_key = tools.KEY_NOTES if estimates_key is None else estimates_key
        self.save_dir = save_dir

    @staticmethod
    def get_default_key():
        return tools.KEY_NOTES

    def get_key(self):
        return self.estimates_key

    def estimate(self, raw_output):
        multi_pitch = tools.tensor_to_array(tools.unpack_dict(raw_output, self.multi_pitch_key))
        onsets = tools.tensor_to_array(tools.unpack_dict(raw_output, self.onsets_key))
        times = tools.tensor_to_array(tools.unpack_dict(raw_output, tools.KEY_TIMES))
        if self.inhibition_window is not None and onsets is None:
            derived = _impulses(multi_pitch).astype(np.asarray(multi_pitch).dtype)
            onsets = inhibit_activations(derived, times, self.inhibition_window)
        return multi_pitch_to_notes(multi_pitch, times, self.profile.low, onsets, self.minimum_duration)

    def process_track(self, raw_output, track=None):
        return {self.get_key(): self.estimate(raw_output)}


class PitchListWrapper(object):
    def __init__(self, profile, multi_pitch_key=None, estimates_key=None, save_dir=None):
        self.profile = profile
        self.multi_pitch_key = tools.KEY_MULTIPITCH if multi_pitch_key is None else multi_pitch_key
        self.estimates_key = tools.KEY_PITCHLIST if estimates_key is None else estimates_key

    def get_key(self):
        return self.estimates_key

    def estimate(self, raw_output):
        multi_pitch = tools.tensor_to_array(tools.unpack_dict(raw_output, self.multi_pitch_key))
        times = tools.tensor_to_array(tools.unpack_dict(raw_output, tools.KEY_TIMES))
        num_frames = multi_pitch.shape[-1]
        pitch_list = [np.empty(0)] * num_frames
        for i in np.where(np.sum(multi_pitch, axis=-2) > 0)[-1]:
            pitch_list[i] = (self.profile.low + np.where(multi_pitch[..., i])[-1]).astype('float')
        return times, pitch_list

    def process_track(self, raw_output, track=None):
        return {self.get_key(): self.estimate(raw_output)}


# ------------------------------------------------------------------------------------------------------------------------------
# Guitar: tablature -> stacked multi-pitch -> multi-pitch / stacked notes
# ------------------------------------------------------------------------------------------------------------------------------
class ComboEstimator(object):
    """Several estimators in succession, each fed the dict updated by the ones before it (amt_tools/transcribe.py:88-128)."""

    def __init__(self, estimators):
        self.estimators = estimators

    def process_track(self, raw_output, track=None):
        output = dict(raw_output)              # the caller's dict is not touched (the reference deep-copies; nothing here mutates an entry)
        for estimator in self.estimators:
            output.update(estimator.process_track(output, track))
        return output


class _Estimator(object):
    """What the estimators below share (amt_tools/transcribe.py:170-308).  `save_dir` is accepted; nothing is written."""

    def __init__(self, profile, estimates_key=None, save_dir=None):
        self.profile = profile
        self.estimates_key = self.get_default_key() if estimates_key is None else estimates_key
        self.save_dir = save_dir

    @staticmethod
    def get_default_key():
        return tools.KEY_MULTIPITCH

    def get_key(self):
        return self.estimates_key

    def process_track(self, raw_output, track=None):
        return {self.estimates_key: self.estimate(raw_output)}


class TablatureWrapper(_Estimator):
    """Tablature (S, T) -> stacked multi-pitch (S, P, T) (amt_tools/transcribe.py:1097-1145)."""

    def __init__(self, profile, tablature_key=None, estimates_key=None, save_dir=None):
        super().__init__(profile, estimates_key, save_dir)
        self.tablature_key = tools.KEY_TABLATURE if tablature_key is None else tablature_key

    def estimate(self, raw_output):
        return tools.tablature_to_stacked_multi_pitch(tools.unpack_dict(raw_output, self.tablature_key), self.profile)


class StackedMultiPitchCollapser(_Estimator):
    """Stacked multi-pitch (S, P, T) -> multi-pitch (P, T).  `stacked_key` defaults to the estimates key, so behind a TablatureWrapper the
    stacked map is replaced by its collapse (amt_tools/transcribe.py:1148-1201)."""

    def __init__(self, profile, stacked_key=None, estimates_key=None, save_dir=None):
        super().__init__(profile, estimates_key, save_dir)
        self.stacked_key = self.estimates_key if stacked_key is None else stacked_key

    def estimate(self, raw_output):
        return tools.stacked_multi_pitch_to_multi_pitch(tools.unpack_dict(raw_output, self.stacked_key))


class StackedNoteTranscriber(_Estimator):
    """Stacked multi-pitch (S, P, T) + times -> {slice: (pitches (N,), intervals (N, 2))} in float64 (amt_tools/transcribe.py:373-481):
    per slice NoteTranscriber's decoding with two of its three sorts by onset.  Options as in NoteTranscriber above."""

    def __init__(self, profile, inhibition_window=None, minimum_duration=None, multi_pitch_key=None, onsets_key=None,
                 offsets_key=None, estimates_key=None, save_dir=None):
        super().__init__(profile, estimates_key, save_dir)
        self.inhibition_window = inhibition_window
        self.minimum_duration = minimum_duration
        self.multi_pitch_key = tools.KEY_MULTIPITCH if multi_pitch_key is None else multi_pitch_key
        self.onsets_key = tools.KEY_ONSETS if onsets_key is None else onsets_key
        self.offsets_key = tools.KEY_OFFSETS if offsets_key is None else offsets_key

    @staticmethod
    def get_default_key():
        return tools.KEY_NOTES

    def estimate(self, raw_output):
        stacked = tools.tensor_to_array(tools.unpack_dict(raw_output, self.multi_pitch_key))
        stacked_onsets = tools.tensor_to_array(tools.unpack_dict(raw_output, self.onsets_key))
        times = tools.tensor_to_array(tools.unpack_dict(raw_output, tools.KEY_TIMES))
        stacked_notes = dict()
        for slc in range(stacked.shape[-3]):
            multi_pitch = np.asarray(stacked[slc])
            onsets = None if stacked_onsets is None else stacked_onsets[slc]
            if self.inhibition_window is not None and onsets is None:
                onsets = inhibit_activations(_impulses(multi_pitch).astype(multi_pitch.dtype), times, self.inhibition_window)
            rows = multi_pitch_to_notes(multi_pitch, times, self.profile.low, onsets, self.minimum_duration, sorts=2)
            stacked_notes[slc] = (rows[..., 2], rows[:, :2])
        return stacked_notes


def _tab_to_stacked_notes_host(tablature, times, profile, inhibition_window=None, minimum_duration=None):
    """One track on the host: (S, T) tablature -> stacked notes through the classes above."""
    raw = {tools.KEY_MULTIPITCH: tools.tablature_to_stacked_multi_pitch(np.asarray(tablature), profile), tools.KEY_TIMES: np.asarray(times)}
    return StackedNoteTranscriber(profile, inhibition_window, minimum_duration).estimate(raw)


def _release_table(times, window):
    """release[t] = first frame after t outside the inhibition window of an onset at frame t: the expression of inhibit_activations above,
    evaluated once per frame of the grid (NumPy scalars and all: the grid's dtype decides how `time + window` rounds), then the same
    max(release, t + 1).  Computed once per distinct (grid, window)."""
    one = lambda g: np.array([max(int(np.searchsorted(g, g[t] + window, side='left')), t + 1) for t in range(len(g))], dtype=np.int32)   # noqa: E731
    return _digest_cached(_RELEASE, times, (repr(window),), lambda grid: one(grid) if grid.ndim == 1 else np.stack([one(g) for g in grid]))


class _PendingTabNotes(_PendingRows):
    """amtx_tab_notes: rows dense over (clip, string); `result()` brings them to the host and slices them into stacked-notes dicts, one
    per clip.  No sort: onsets of one string are distinct and already ascending."""

    def result(self):
        rows, off, _ = self.fetch()
        S = self.strings
        return [{s: (rows[off[b * S + s]:off[b * S + s + 1], 2], rows[off[b * S + s]:off[b * S + s + 1], :2]) for s in range(S)}
                for b in range((len(off) - 1) // S)]


class _HostTabNotes(_HostNotes):
    """The same handle for what the kernel does not build (more than 64 classes under an inhibition window, more than 16 strings) and for
    CPU tablatures: the host classes, track by track."""

    def result(self):
        tablature, times, profile, window, min_dur = self._args
        tab = tools.tensor_to_array(tablature)
        times = np.asarray(times)
        return [_tab_to_stacked_notes_host(tab[b], times if times.ndim == 1 else times[b], profile, window, min_dur) for b in range(tab.shape[0])]


TAB_NOTES_MAX_CLASSES = 64     # amtx_tab_notes keeps the inhibition state of class k in lane k of a wave
TAB_MAX_STRINGS = 16


def decode_tab_notes_batch_async(tablature, times, profile, inhibition_window=None, minimum_duration=None, rows_capacity=None):
    """Enqueue the tablature decoder and return a handle; `handle.result()` -> list of B stacked-notes dicts {string: (pitches (N,),
    intervals (N, 2))}, float64, equal to StackedNoteTranscriber(profile, inhibition_window, minimum_duration) on the
    TablatureWrapper's map of each clip.  `tablature`: (B, S, T) int64 CUDA tensor, -1 = silent; `times`: one (T,) grid or (B, T)."""
    import torch
    assert tablature.dim() == 3
    B, S, T = tablature.shape
    num_classes = int(profile.num_pitches)
    tuning = np.ascontiguousarray(profile.get_midi_tuning(), dtype=np.int32)
    assert len(tuning) == S, (len(tuning), S)
    times = np.asarray(times)
    ext, stride = _extended_grid(times, T)
    if not tablature.is_cuda or S > TAB_MAX_STRINGS or (inhibition_window is not None and num_classes > TAB_NOTES_MAX_CLASSES):
        return _HostTabNotes(tablature, times, profile, inhibition_window, minimum_duration, strings=S)
    assert tablature.dtype == torch.int64
    dev = tablature.device
    tablature = tablature.contiguous()
    ext_d = _grid_on_device(ext, dev)
    rel_d, rel_stride = None, 0
    if inhibition_window is not None:
        rel_d = _grid_on_device(_release_table(times, inhibition_window), dev)
        rel_stride = 0 if times.ndim == 1 else T
    has_min = minimum_duration is not None

    def rows_pass(capacity):
        rows = torch.empty((capacity, 3), dtype=torch.float64, device=dev)
        offsets = torch.empty((B * S + 1,), dtype=torch.int32, device=dev)
        _lib.call('amtx_tab_notes', tablature, B, S, T, tuning, num_classes, ext_d, stride, rel_d, rel_stride, int(has_min),
                  float(minimum_duration) if has_min else 0.0, rows, capacity, offsets, device=dev)
        return _PendingTabNotes(rows, offsets, rows_pass, strings=S)

    # a string holds at most one note per frame; 128 notes per string on average is far above any real tablature (a denser batch is caught
    # in result() through the total the device reports and decoded again into a buffer of the exact size)
    return rows_pass(int(rows_capacity) if rows_capacity else max(1, min(B * S * T, max(B * S * 128, 1 << 14))))


def decode_tab_notes_batch(tablature, times, profile, inhibition_window=None, minimum_duration=None):
    return decode_tab_notes_batch_async(tablature, times, profile, inhibition_window, minimum_duration).result()


def decode_notes_for(preds, model, times=None):
    """The note decoder of one batch of `model`'s output, enqueued -- the offline drivers' one route.  Returns a handle:
    `result()` -> the batch's note lists on the host ((K, 3) batched notes per clip; a tablature model: stacked notes per clip),
    `device_rows()` -> _PendingRows.device_rows, or None when the notes are decoded on the host, `strings` -> note groups per clip of a
    tablature model, else None.  The grid is `times`, or the frame grid of the model's front-end when `times` is None."""
    from .inference import _frame_times
    tab_model = tools.KEY_MULTIPITCH not in preds and tools.KEY_TABLATURE in preds
    est = preds[tools.KEY_TABLATURE if tab_model else tools.KEY_MULTIPITCH]
    if times is None:
        times = _frame_times(model, est.shape[-1])
    if tab_model:
        return decode_tab_notes_batch_async(est, times, model.profile)
    if est.is_cuda:
        return decode_notes_batch_async(preds[tools.KEY_ONSETS], est, times, model.profile.low)
    return _HostNotes(preds[tools.KEY_ONSETS], est, times, model.profile.low)
