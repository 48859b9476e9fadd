"""
Training clips cut from device-resident tracks, with the reference's track-level semantics.

The reference computes a track's feature map ONCE and slices frames [frame_start, frame_start + num_frames) out of it, with
frame_start = sample_start // hop_length (amt_tools/datasets/common.py:325-327, 340-354, 392).  A clip's features are therefore
(1) scaled against the TRACK's maximum -- power_to_db(ref=np.max) and the 80 dB floor both see the whole map (features/mel.py:94,
features/common.py:199, 218-225; SURVEY finding F7) -- and (2) framed from the track's own samples at the clip's edges, not from padding.

`TrackBank` keeps whole tracks in one device buffer together with every track's power maximum; `bank.clips(...)` names frames of those
tracks, and `module.process_clips(clips)` (amt_tools_amd/features.py) returns exactly the slices of the track's own feature map, bit for
bit, without ever writing that map: amtx_spec_power_clips frames each clip out of its track (include/amtx_tracks.h).

`PyramidBank` is the same for the CQT family (CQT / VQT / HCQT / HVQT).  A clip of those cannot be decimated on its own -- seven 301-tap
half-band stages need context that doubles per level -- so the bank keeps every track's decimation pyramid resident beside its audio
(include/amtx_pyramid.h: about as many samples again) and a clip's features are basis products over windows of those resident signals.

A TrackBank of raw audio serves STFT / MelSpec modules only: the CQT family has no clip form there.

`LabelBank` is the ground truth of the same clips.  A clip's labels are an identity too: the columns [first_frame, first_frame + num_frames)
of the track's own label maps (the reference's slice_track, amt_tools/datasets/common.py:392).  The whole-track maps are made on the
host, where the reference's time-to-frame rule is pinned (amt_tools_amd/cache.py); their rows are piecewise constant, so the bank keeps
them run-length encoded -- integers only (encode_rows) -- and `labels.clips(...)` decodes the clips' columns on the device
(amtx_label_clips, include/amtx_labels.h) into the tensors the loss kernels take without a copy.  `ClipLoader` draws clips by the
reference's rule (draw_clips) and yields complete batches: features' clips under tools.KEY_AUDIO, label tensors under their keys.

`NoteBank` is the note ground truth of the same clips, for validation: the reference's slice_batched_notes of a clip's time window
(amt_tools/tools/utils.py:322-361), computed per (clip, slice) on the device (amtx_note_clips, include/amtx_noteclips.h) into the
(rows, offsets) pair the device note matcher reads.  `cover_clips` names the consecutive clips that cover whole tracks.

Whole tracks come from the same clips: `seam_clips` covers every track with equally long, overlapping clips and names the frames each
clip keeps, `TrackMaps` holds the whole-track outputs on the device, every track's map contiguous with its own width, and
amtx_stitch_clips (include/amtx_stitch.h; `stitch_host` is its NumPy restatement) writes a batch's kept columns into them.
`NoteBank.whole` is the unsliced note ground truth of whole tracks.  inference.run_tracks and evaluate.validate_tracks are the drivers.

What the banks share is written once: `_checked_request` validates a `clips(track_ids, first_frames, num_frames)` request against
a bank's frame counts, `_clip_table` lays the checked request out as the int64 table a clip kernel reads (clip_descriptors adds the
reflect rule and the 4-column form of amtx_spec_power_clips), `_Resident` is the lazy, never-pickled device state, and `_Clips` is the
batch entry that TrackClips and PyramidClips name -- the feature modules and models choose the kernel family by that type.
"""

from collections import namedtuple

import numpy as np

from . import _lib

__all__ = ['TrackBank', 'TrackClips', 'PyramidBank', 'PyramidClips', 'clip_descriptors', 'frame_start',
           'LabelBank', 'ClipLoader', 'encode_rows', 'decode_rows', 'draw_clips', 'NoteBank', 'NoteClips', 'cover_clips', 'clip_windows',
           'SeamPlan', 'seam_clips', 'stitch_host', 'stitch_clips', 'TrackMaps']


def frame_start(sample_start, hop_length):
    """First frame of a clip that starts at `sample_start`: the reference's rule (amt_tools/datasets/common.py:392)."""
    return int(sample_start) // int(hop_length)


def _checked_request(frame_counts, track_ids, first_frames, num_frames):
    """The one check of a clip request against a bank's frame counts: (track ids, first frames) as int64 1-D arrays.  ValueError for ids
    and first frames that do not pair up, no clip, fewer than one frame, an unknown track, a negative first frame and a clip that runs
    past its track's last frame (a track shorter than the clip included), in that order.  Pure host code."""
    frame_counts = np.asarray(frame_counts, dtype=np.int64).reshape(-1)
    ids = np.asarray(track_ids, dtype=np.int64).reshape(-1)
    firsts = np.asarray(first_frames, dtype=np.int64).reshape(-1)
    num_frames = int(num_frames)
    if ids.shape != firsts.shape or ids.size == 0:
        raise ValueError('one first frame per track id, and at least one clip')
    if num_frames < 1:
        raise ValueError(f'a clip has at least one frame (got {num_frames})')
    bad = (ids < 0) | (ids >= len(frame_counts))
    if bad.any():
        raise ValueError(f'unknown track {int(ids[bad][0])}: the bank holds {len(frame_counts)} tracks')
    if (firsts < 0).any():
        raise ValueError(f'negative first frame {int(firsts[firsts < 0][0])}')
    past = firsts + num_frames > frame_counts[ids]
    if past.any():
        b = int(np.argmax(past))
        raise ValueError(f'clip {b}: frames [{int(firsts[b])}, {int(firsts[b]) + num_frames}) run past the '
                         f'{int(frame_counts[ids[b]])} frames of track {int(ids[b])}')
    return ids, firsts


def _clip_table(*columns):
    """int64 (B, len(columns)) C-contiguous table of a checked request; a scalar column (the frames of every clip) is repeated."""
    desc = np.empty((columns[0].size, len(columns)), dtype=np.int64)
    for c, column in enumerate(columns):
        desc[:, c] = column
    return desc


def clip_descriptors(starts, lengths, frame_counts, track_ids, first_frames, num_frames, reflect_half=None):
    """The table amtx_spec_power_clips reads: int64 (B, 4) rows {track_start, track_len, first_frame, frames}, frames = num_frames, for the
    clips [first_frames[b], first_frames[b] + num_frames) of the tracks track_ids[b].  starts / lengths / frame_counts describe the bank
    (element offset, samples and frames of every track).  reflect_half: n_fft // 2 of a reflect-padded plan (librosa 0.9), else None.

    Pure host code.  ValueError for a request _checked_request refuses and for a reflect-padded plan over a track of n_fft / 2 samples or
    fewer."""
    starts, lengths, frame_counts = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (starts, lengths, frame_counts))
    if not (len(starts) == len(lengths) == len(frame_counts)):
        raise ValueError('starts, lengths and frame_counts describe the same tracks: one entry each')
    ids, firsts = _checked_request(frame_counts, track_ids, first_frames, num_frames)
    if reflect_half is not None:
        short = lengths[ids] <= int(reflect_half)
        if short.any():
            b = int(np.argmax(short))
            raise ValueError(f'track {int(ids[b])} has {int(lengths[ids[b]])} samples: reflect padding needs more than '
                             f'n_fft/2 = {int(reflect_half)}')
    return _clip_table(starts[ids], lengths[ids], firsts, int(num_frames))


def _reflect_half(module):
    return int(module.n_fft) // 2 if module._pad_mode() == 1 else None


class _Clips(object):
    """Clips of a bank, as a batch entry under tools.KEY_AUDIO or an argument of process_clips / power_clips: `bank`, `desc` (the host
    int64 table the clip kernels read, the clips' frame count in its last column), `desc_dev` (its device copy) and `db_ref` (device
    float32: the power maxima of the clips' tracks).  No tensor subclass: tools.dict_to_device passes it through as it is."""

    def __init__(self, bank, desc, desc_dev, db_ref):
        self.bank, self.desc, self.desc_dev, self.db_ref = bank, desc, desc_dev, db_ref

    @property
    def num_clips(self):
        return int(self.desc.shape[0])

    @property
    def num_frames(self):
        return int(self.desc[0, -1])

    @property
    def device(self):
        return self.desc_dev.device


class TrackClips(_Clips):
    """Clips of a TrackBank: desc (B, 4) = clip_descriptors, db_ref (B,)."""


class PyramidClips(_Clips):
    """Clips of a PyramidBank: desc (B, 3) rows {track, first_frame, frames}, db_ref (B, n_harm), per harmonic."""


class _Resident(object):
    """Device state that is created on first use, never at construction, and never pickled: `self.device` names the device, `_upload(device)`
    returns the tuple of device tensors, and `_device_state()` caches it under __dict__['_dev']."""

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('_dev', None)
        return state

    def _device_state(self):
        dev = self.__dict__.get('_dev')
        if dev is None:
            import torch
            from .features import _index_of
            dev = self.__dict__['_dev'] = self._upload(torch.device('cuda', _index_of(self.device)))
        return dev


class TrackBank(_Resident):
    """Whole tracks (1-D float32 arrays), back to back in ONE float32 device buffer, for the STFT / MelSpec `module` whose features the
    clips will be.  Keeps `starts` / `lengths` (samples) and `frame_counts` (module.get_expected_frames) per track on the host, and
    `db_ref`: every track's power maximum -- the reference of its dB scale -- from one amtx_spec_power_clips launch that writes no map.

    The device buffer and db_ref are created on first use, never at construction, and never pickled (a host copy of the tracks is kept
    and uploaded again): a bank can be built before DataLoader workers fork, like the feature modules."""

    def __init__(self, tracks, module, device=None):
        from .features import _SpecPlanOwner, _CqtPlanOwner
        if isinstance(module, _CqtPlanOwner):
            raise NotImplementedError(f'{type(module).__name__}: the decimation pyramid of the CQT family has no clip form over a bank of raw '
                                      f'audio (a PyramidBank keeps the pyramids resident)')
        if not isinstance(module, _SpecPlanOwner):
            raise TypeError(f'a TrackBank takes an STFT or MelSpec of this package, not {type(module).__name__}')
        self._take(tracks, module, device, align=1)
        # every track whole: the descriptors of the maxima launch (validated like any clip request)
        self._track_desc = np.concatenate([clip_descriptors(self.starts, self.lengths, self.frame_counts, [i], [0], n, _reflect_half(module))
                                           for i, n in enumerate(self.frame_counts)])

    def _take(self, tracks, module, device, align):
        """The host bookkeeping: lengths, starts (multiples of `align` elements), frame counts and one host buffer of all tracks."""
        tracks = [np.ascontiguousarray(t, dtype=np.float32) for t in tracks]
        if not tracks or any(t.ndim != 1 or t.size == 0 for t in tracks):
            raise ValueError('tracks: at least one, each a non-empty 1-D array of samples')
        self.module = module
        self.device = module.device if device is None else device
        self.lengths = np.array([t.size for t in tracks], dtype=np.int64)
        room = -(-self.lengths // align) * align
        self.starts = np.concatenate(([0], np.cumsum(room)[:-1])).astype(np.int64)
        self.frame_counts = np.array([module.get_expected_frames(t) for t in tracks], dtype=np.int64)
        if (self.frame_counts < 1).any():
            raise ValueError(f'track {int(np.argmin(self.frame_counts))} is too short for one frame')
        if align == 1:
            self._host = np.concatenate(tracks)
        else:
            self._host = np.zeros(int(self.starts[-1] + self.lengths[-1]), dtype=np.float32)
            for start, t in zip(self.starts, tracks):
                self._host[start:start + t.size] = t

    def __len__(self):
        return len(self.lengths)

    def _check_frames(self, i, frames):
        """The plan's frame count of track i must be the host bookkeeping's (module.get_expected_frames), or clips near the track's end
        would be framed from padding, or not exist (the reference's own count differs for a module that is not centred with
        win_length < n_fft: features/waveform.py:43-67)."""
        if frames != int(self.frame_counts[i]):
            raise ValueError(f'track {i} ({int(self.lengths[i])} samples): the module expects {int(self.frame_counts[i])} frames, '
                             f'its plan computes {frames}')

    def _upload(self, device):
        """(audio, db_ref) on the bank's device."""
        import torch
        plan = self.module._get_plan(device)
        for i, n in enumerate(self.lengths):                       # the kernel's contract counts frames as amtx_spec_num_frames does
            self._check_frames(i, int(_lib.call('amtx_spec_num_frames', plan, int(n))))
        audio = torch.from_numpy(self._host).to(device)
        desc = torch.from_numpy(self._track_desc).to(device)
        db_ref = torch.empty((len(self),), dtype=torch.float32, device=device)
        # power = NULL: maxima only; `frames` = each track's own count, rows per clip = the longest track's
        _lib.call('amtx_spec_power_clips', plan, audio, desc, len(self), int(self.frame_counts.max()), None, db_ref,
                  device=device)
        return audio, db_ref

    def _clips_of(self, kind, ids, desc):
        """The `kind` (TrackClips / PyramidClips) of a checked request: its table on the device and the maxima of the clips' tracks."""
        import torch
        audio, db_ref = self._device_state()[:2]
        return kind(self, desc, torch.from_numpy(desc).to(audio.device), db_ref[torch.from_numpy(ids).to(audio.device)])

    @property
    def audio(self):
        """The tracks back to back: 1-D float32 device tensor, track i at [starts[i], starts[i] + lengths[i])."""
        return self._device_state()[0]

    @property
    def db_ref(self):
        """(num_tracks,) float32 device tensor: every track's power maximum (bit for bit the clip_max of amtx_spec_power on that track)."""
        return self._device_state()[1]

    def clips(self, track_ids, first_frames, num_frames):
        """`num_frames` frames from first_frames[b] on of track track_ids[b], as a TrackClips.  first_frames follow the reference's rule
        (frame_start); the request is validated on the host (clip_descriptors)."""
        desc = clip_descriptors(self.starts, self.lengths, self.frame_counts, track_ids, first_frames, num_frames, _reflect_half(self.module))
        return self._clips_of(TrackClips, np.asarray(track_ids, dtype=np.int64).reshape(-1), desc)


class PyramidBank(TrackBank):
    """Whole tracks for a CQT / VQT / HCQT / HVQT `module`: the audio in one float32 device buffer (every track at a multiple of 4
    elements) and, beside it, every track's decimation pyramid as amtx_cqt_forward would lay it out for that track alone
    (amtx_cqt_pyramid_build), plus `db_ref`: per (track, harmonic) the maximum of the power map -- the reference of its dB scale -- from a
    launch that writes no map.  Host bookkeeping, lazy device state and pickling as TrackBank's."""

    def __init__(self, tracks, module, device=None):
        from .features import _CqtPlanOwner
        if not isinstance(module, _CqtPlanOwner):
            raise TypeError(f'a PyramidBank takes a CQT, VQT, HCQT or HVQT of this package, not {type(module).__name__}')
        self._take(tracks, module, device, align=4)

    def _upload(self, device):
        """(audio, db_ref, pyramid, track table) on the bank's device."""
        import ctypes as C
        import torch
        plan = self.module._get_plan(device)
        cols = int(_lib.call('amtx_cqt_track_cols', plan))
        n_harm = int(_lib.call('amtx_cqt_num_harmonics', plan))
        table = np.zeros((len(self), cols), dtype=np.int64)
        place = 0                                            # elements of the pyramid buffer handed out (strides are multiples of 4)
        for i, n in enumerate(self.lengths):
            level_len, level_stride, rows_h = ((C.c_int64 * 16)() for _ in range(3))
            frames = C.c_int64()
            # not through _lib.call: AMTX_ERR_UNSUPPORTED is an answer here (a plan the windowed basis kernel does not cover)
            rc = _lib.lib().amtx_cqt_track_layout(plan, int(n), level_len, level_stride, rows_h, C.byref(frames))
            if rc == _lib.ERR_UNSUPPORTED:
                raise NotImplementedError(f'{type(self.module).__name__}: {_lib.lib().amtx_last_error().decode()}')
            try:
                levels = _lib.check(rc, 'amtx_cqt_track_layout')
            except _lib.AmtxError as e:
                raise ValueError(f'track {i} ({int(n)} samples): {e}') from None
            self._check_frames(i, frames.value)
            rows = list(rows_h[:n_harm])
            table[i, :4] = (self.starts[i], n, max(rows), frames.value)
            for l in range(levels):
                table[i, 4 + 3 * l:7 + 3 * l] = (place, level_len[l], level_stride[l])
                place += level_stride[l]
            table[i, 4 + 3 * levels:] = rows
        audio = torch.from_numpy(self._host).to(device)
        pyramid = torch.empty((max(place, 4),), dtype=torch.float32, device=device)
        table_dev = torch.from_numpy(table).to(device)
        db_ref = torch.empty((len(self), n_harm), dtype=torch.float32, device=device)
        _lib.call('amtx_cqt_pyramid_build', plan, audio, audio.numel(), table, table_dev, len(self), pyramid, pyramid.numel(), db_ref,
                  device=device)
        return audio, db_ref, pyramid, table_dev

    @property
    def db_ref(self):
        """(num_tracks, n_harm) float32 device tensor: per harmonic, every track's power maximum over that harmonic's own frames (bit for
        bit the reference amtx_cqt_forward scales the whole track by)."""
        return self._device_state()[1]

    @property
    def pyramid(self):
        """The level signals of all tracks, 1-D float32 device tensor (include/amtx_pyramid.h)."""
        return self._device_state()[2]

    @property
    def table(self):
        """The track table, (num_tracks, cols) int64 device tensor (include/amtx_pyramid.h)."""
        return self._device_state()[3]

    def clips(self, track_ids, first_frames, num_frames):
        """`num_frames` frames from first_frames[b] on of track track_ids[b], as a PyramidClips; validated on the host (_checked_request:
        unknown track, negative first frame, a clip past its track's last frame, fewer than one frame)."""
        ids, firsts = _checked_request(self.frame_counts, track_ids, first_frames, num_frames)
        return self._clips_of(PyramidClips, ids, _clip_table(ids, firsts, int(num_frames)))


# ------------------------------------------------------------------------------------------------------------------------------
# ground truth: run-length encoded label rows, decoded per clip on the device
# ------------------------------------------------------------------------------------------------------------------------------
MAX_LABEL_KEYS = 16         # AMTX_LABEL_MAX_KEYS (include/amtx_labels.h): label maps of one dtype kind that one launch serves


def _is_float_map(a):
    kind = np.asarray(a).dtype.kind
    if kind not in 'fiub':
        raise TypeError(f'a label map holds floating, integer or bool values, not {np.asarray(a).dtype}')
    return kind == 'f'


def _row_patterns(label_map, what=''):
    """The (rows, T) int32 patterns of a label map: float32 bits of a floating map, int32 values of an integer or bool map."""
    a = np.asarray(label_map)
    is_float = _is_float_map(a)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f'{what}a label map is (rows, frames) with at least one of each, not {a.shape}')
    if is_float:
        with np.errstate(over='ignore', invalid='ignore'):
            f32 = a.astype(np.float32)
            bad = ~((f32.astype(a.dtype) == a) | (np.isnan(a) & np.isnan(f32)))
        if bad.any():
            r, t = (int(i) for i in np.argwhere(bad)[0])
            raise ValueError(f'{what}row {r}, frame {t}: float32 does not hold {a[r, t]!r} exactly')
        return np.ascontiguousarray(f32).view(np.int32)
    if a.dtype.kind == 'u':
        bad = a.astype(np.uint64) > np.uint64(2 ** 31 - 1)
    elif a.dtype.kind == 'i':
        wide = a.astype(np.int64)
        bad = (wide < -2 ** 31) | (wide > 2 ** 31 - 1)
    else:
        bad = np.zeros(a.shape, dtype=bool)
    if bad.any():
        r, t = (int(i) for i in np.argwhere(bad)[0])
        raise ValueError(f'{what}row {r}, frame {t}: {int(a[r, t])} is outside int32')
    return np.ascontiguousarray(a.astype(np.int32))


def encode_rows(label_map, what=''):
    """Run-length encoding of a (rows, T) label map: (row_ptr int64 (rows + 1,), run_first int32 (N,), run_bits int32 (N,)).  Run j of a
    row -- row_ptr[r] <= j < row_ptr[r + 1] -- holds the 32-bit pattern run_bits[j] from frame run_first[j] up to the next run's first
    frame, or to the track's end; every row's first run starts at frame 0.  Runs are split where the PATTERN changes: NaN and -0.0 survive.

    A floating map is stored as its float32 patterns, an integer or bool map as int32 values; ValueError, naming row and frame (after the
    prefix `what`), for a value float32 does not represent exactly or an integer outside int32.  Pure NumPy."""
    p = _row_patterns(label_map, what)
    starts = np.ones(p.shape, dtype=bool)
    starts[:, 1:] = p[:, 1:] != p[:, :-1]
    rows, frames = np.nonzero(starts)                     # row-major: ascending frames inside ascending rows
    row_ptr = np.concatenate(([0], np.cumsum(starts.sum(axis=1)))).astype(np.int64)
    return row_ptr, frames.astype(np.int32), p[rows, frames]


def decode_rows(row_ptr, run_first, run_bits, num_frames, dtype=np.float32):
    """The inverse of encode_rows for a track of `num_frames` frames: (rows, num_frames) float32 with the stored patterns (dtype float32)
    or the stored values as int64 (dtype int64) -- what amtx_label_clips writes for out_kind 0 / 1.  Pure NumPy: the CPU reference."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    run_first, run_bits = np.asarray(run_first, dtype=np.int32), np.asarray(run_bits, dtype=np.int32)
    stop = np.empty(run_first.shape, dtype=np.int64)
    stop[:-1] = run_first[1:]
    stop[row_ptr[1:] - 1 - row_ptr[0]] = int(num_frames)             # a row's last run ends with the track
    flat = np.repeat(run_bits, stop - run_first).reshape(len(row_ptr) - 1, int(num_frames))
    if np.dtype(dtype) == np.float32:
        return flat.view(np.float32)
    if np.dtype(dtype) == np.int64:
        return flat.astype(np.int64)
    raise TypeError(f'label clips are float32 or int64, not {np.dtype(dtype)}')


class LabelBank(_Resident):
    """The frame-aligned ground truth of whole tracks, run-length encoded (encode_rows), for clips cut on the device.

    maps: one dict {key: (rows_key, T_track) array} per track -- tools.KEY_MULTIPITCH, KEY_ONSETS, KEY_OFFSETS, KEY_TABLATURE or any other
    frame-aligned key -- consumed one track at a time (an iterator's maps can be dropped as soon as they are encoded).  All tracks carry
    the same keys with the same row count and dtype kind per key; all keys of a track have the same width, and with `bank` (the TrackBank /
    PyramidBank of the same tracks) that width is bank.frame_counts[i]: ValueError otherwise, naming the track.

    One row_ptr / run_first / run_bits for all tracks; the global row is track * rows_total + row, the floating keys' rows first, then the
    integer (and bool) keys'.  The device copies are created on first use, never at construction, and never pickled (the host encoding
    is kept): a bank can be built before DataLoader workers fork, like TrackBank."""

    def __init__(self, maps, bank=None, device=None):
        self.device = device if device is not None else (bank.device if bank is not None else 'cuda')
        self.float_keys, self.int_keys = [], []          # [(key, rows)] in the order of the first track's dict
        counts, ptrs, firsts, bits = [], [np.zeros(1, dtype=np.int64)], [], []
        kinds, order, runs = None, None, 0
        for i, entry in enumerate(maps):
            if kinds is None:
                if not len(entry):
                    raise ValueError('track 0 carries no label map')
                kinds = {key: (_is_float_map(a), int(np.shape(a)[0]) if np.ndim(a) == 2 else None) for key, a in entry.items()}
                self.float_keys = [(key, rows) for key, (is_float, rows) in kinds.items() if is_float]
                self.int_keys = [(key, rows) for key, (is_float, rows) in kinds.items() if not is_float]
                order = [key for key, _ in self.float_keys + self.int_keys]
                for group in (self.float_keys, self.int_keys):
                    if len(group) > MAX_LABEL_KEYS:
                        raise ValueError(f'{len(group)} label maps of one dtype kind: one launch serves {MAX_LABEL_KEYS}')
            if sorted(map(str, entry)) != sorted(map(str, kinds)):
                raise ValueError(f'track {i} carries the keys {sorted(map(str, entry))}, track 0 {sorted(map(str, kinds))}')
            width = None
            for key in order:
                a = np.asarray(entry[key])
                if _is_float_map(a) != kinds[key][0]:
                    raise ValueError(f"track {i}, '{key}': dtype {a.dtype}, but track 0 holds {'floating' if kinds[key][0] else 'integer'} values there")
                if a.ndim != 2:
                    raise ValueError(f"track {i}, '{key}': a label map is (rows, frames), not {a.shape}")
                if a.shape[0] != kinds[key][1]:
                    raise ValueError(f"track {i}, '{key}': shape {a.shape}, but track 0 has {kinds[key][1]} rows there")
                if width is None:
                    width = int(a.shape[1])
                elif a.shape[1] != width:
                    raise ValueError(f"track {i}: '{key}' has {a.shape[1]} frames, '{order[0]}' has {width}")
                row_ptr, run_first, run_bits = encode_rows(a, f"track {i}, '{key}': ")
                ptrs.append(row_ptr[1:] + runs)
                firsts.append(run_first)
                bits.append(run_bits)
                runs += int(row_ptr[-1])
            if bank is not None and (i >= len(bank) or width != int(bank.frame_counts[i])):
                have = f'{int(bank.frame_counts[i])} frames' if i < len(bank) else f'only {len(bank)} tracks'
                raise ValueError(f'track {i}: its label maps have {width} frames, the bank has {have}')
            counts.append(width)
        if kinds is None:
            raise ValueError('maps: at least one track')
        if bank is not None and len(counts) != len(bank):
            raise ValueError(f'label maps of {len(counts)} tracks for a bank of {len(bank)}')
        self.frame_counts = np.array(counts, dtype=np.int64)
        self.rows_total = sum(rows for _, rows in self.float_keys + self.int_keys)
        self.row_ptr = np.concatenate(ptrs)
        self.run_first = np.concatenate(firsts)
        self.run_bits = np.concatenate(bits)

    @classmethod
    def from_notes(cls, notes, times, profile, keys=None, ambiguity=None, bank=None, device=None):
        """The piano recipe: notes[i] = (pitches, intervals) and times[i] = the frame grid of track i; the whole-track maps come from
        cache.notes_to_multi_pitch / notes_to_onsets / notes_to_offsets on the host (`ambiguity` as there) and each track's maps are
        dropped once they are encoded.  keys: of tools.KEY_MULTIPITCH, KEY_ONSETS, KEY_OFFSETS (default: all three)."""
        from . import cache, tools
        makers = {tools.KEY_MULTIPITCH: lambda p, i, t: cache.notes_to_multi_pitch(p, i, t, profile),
                  tools.KEY_ONSETS: lambda p, i, t: cache.notes_to_onsets(p, i, t, profile, ambiguity),
                  tools.KEY_OFFSETS: lambda p, i, t: cache.notes_to_offsets(p, i, t, profile, ambiguity)}
        keys = tuple(makers) if keys is None else tuple(keys)
        for key in keys:
            if key not in makers:
                raise ValueError(f"no label map '{key}' from notes: {', '.join(makers)} (tablature and other maps go in as `maps`)")
        if len(notes) != len(times):
            raise ValueError(f'{len(notes)} note lists for {len(times)} frame grids')
        return cls(({key: makers[key](pitches, intervals, grid) for key in keys} for (pitches, intervals), grid in zip(notes, times)),
                   bank=bank, device=device)

    def __len__(self):
        return len(self.frame_counts)

    @property
    def keys(self):
        """Every label key, the floating ones first: the order of the rows inside a track."""
        return [key for key, _ in self.float_keys + self.int_keys]

    @property
    def runs_per_track(self):
        """(num_tracks,) runs of every track."""
        return np.diff(self.row_ptr[::self.rows_total])

    @property
    def nbytes(self):
        """Bytes of the three tables, on the host as on the device."""
        return int(self.row_ptr.nbytes + self.run_first.nbytes + self.run_bits.nbytes)

    def _rows_of(self, key):
        lo = 0
        for name, rows in self.float_keys + self.int_keys:
            if name == key:
                return lo, lo + rows
            lo += rows
        raise KeyError(key)

    def host_map(self, track, key):
        """The whole (rows_key, T_track) map of one track, decoded on the host (decode_rows): float32 or int64 as clips() gives it."""
        lo, hi = self._rows_of(key)
        g = int(track) * self.rows_total
        ptr = self.row_ptr[g + lo:g + hi + 1]
        dtype = np.float32 if key in dict(self.float_keys) else np.int64
        return decode_rows(ptr, self.run_first[ptr[0]:ptr[-1]], self.run_bits[ptr[0]:ptr[-1]], self.frame_counts[int(track)], dtype)

    def _upload(self, device):
        """(row_ptr, run_first, run_bits) on the bank's device."""
        import torch
        return tuple(torch.from_numpy(a).to(device) for a in (self.row_ptr, self.run_first, self.run_bits))

    def clips(self, track_ids, first_frames, num_frames):
        """{key: device tensor (B, rows_key, num_frames)} -- float32 for floating keys, int64 for integer and bool keys, each contiguous:
        the columns [first_frames[b], first_frames[b] + num_frames) of the maps of track track_ids[b].  Same signature and host validation
        as bank.clips (_checked_request against this bank's own frame counts).  One amtx_label_clips launch per dtype kind; the keys of a
        kind are views into one allocation, key-major."""
        import torch
        desc = _clip_table(*_checked_request(self.frame_counts, track_ids, first_frames, num_frames), int(num_frames))
        row_ptr, run_first, run_bits = self._device_state()
        device = row_ptr.device
        desc_dev = torch.from_numpy(desc).to(device)
        B, T = int(desc.shape[0]), int(num_frames)
        result, row_lo = {}, 0
        for group, dtype, kind in ((self.float_keys, torch.float32, 0), (self.int_keys, torch.int64, 1)):
            if not group:
                continue
            key_rows = np.cumsum([row_lo] + [rows for _, rows in group]).astype(np.int64)
            row_hi = int(key_rows[-1])
            flat = torch.empty(((row_hi - row_lo) * B * T,), dtype=dtype, device=device)
            _lib.call('amtx_label_clips', row_ptr, run_first, run_bits, len(self), self.rows_total, row_lo, row_hi, key_rows, len(group),
                      desc_dev, B, T, flat, kind, device=device)
            for (key, rows), lo in zip(group, key_rows):
                at = int(lo - row_lo) * B * T
                result[key] = flat[at:at + rows * B * T].view(B, rows, T)
            row_lo = row_hi
        return result


def draw_clips(rng, lengths, hop_length, num_frames, track_ids):
    """First frames of one random clip per entry of `track_ids`, by the reference's rule (amt_tools/datasets/common.py:340-343):
    seq_length = num_frames * hop_length, sample_start = rng.randint(0, length - seq_length), first frame = sample_start // hop_length --
    drawn in the order of track_ids from `rng` (a np.random.RandomState).  lengths: the samples of every track of the bank.  ValueError
    for an unknown track and for a track of seq_length samples or fewer (the reference pads those; the banks refuse them).  Pure host code."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    track_ids = np.asarray(track_ids, dtype=np.int64).reshape(-1)
    seq_length = int(num_frames) * int(hop_length)
    if int(num_frames) < 1 or int(hop_length) < 1:
        raise ValueError(f'a clip has at least one frame of at least one sample (got {num_frames} frames, hop {hop_length})')
    first_frames = np.empty(track_ids.shape, dtype=np.int64)
    for b, k in enumerate(track_ids):
        if k < 0 or k >= len(lengths):
            raise ValueError(f'unknown track {int(k)}: the bank holds {len(lengths)} tracks')
        if lengths[k] <= seq_length:
            raise ValueError(f'track {int(k)} has {int(lengths[k])} samples: a clip of {int(num_frames)} frames needs more than {seq_length}')
        first_frames[b] = frame_start(rng.randint(0, int(lengths[k]) - seq_length), hop_length)
    return first_frames


class ClipLoader(object):
    """Complete training batches from a TrackBank / PyramidBank and the LabelBank of the same tracks: an iterable with __len__ that takes
    the place of the DataLoader in the reference's train().  Every batch is {tools.KEY_AUDIO: bank.clips(...), **labels.clips(...)} with
    the same track ids and first frames for both: one clip of `num_frames` frames per track, drawn by draw_clips.

    An epoch is one permutation of the tracks from this loader's np.random.RandomState(seed), dealt into batches of `batch_size`; the
    last, smaller batch is dropped with drop_last.  The TRACK ORDER is this loader's own: the reference's comes from the shuffle of torch's
    DataLoader, which no NumPy generator reproduces.  The clip positions follow the reference's rule, from this loader's generator."""

    def __init__(self, bank, labels, num_frames, batch_size, seed=0, drop_last=True):
        if len(bank) != len(labels):
            raise ValueError(f'a bank of {len(bank)} tracks and labels of {len(labels)}')
        if int(batch_size) < 1 or int(num_frames) < 1:
            raise ValueError(f'batch_size and num_frames are at least 1 (got {batch_size}, {num_frames})')
        self.bank, self.labels = bank, labels
        self.num_frames, self.batch_size, self.drop_last = int(num_frames), int(batch_size), bool(drop_last)
        self.rng = np.random.RandomState(seed)

    def __len__(self):
        full, rest = divmod(len(self.bank), self.batch_size)
        return full + (1 if rest and not self.drop_last else 0)

    def __iter__(self):
        from . import tools
        order = self.rng.permutation(len(self.bank))
        for i in range(len(self)):
            ids = order[i * self.batch_size:(i + 1) * self.batch_size]
            firsts = draw_clips(self.rng, self.bank.lengths, self.bank.module.hop_length, self.num_frames, ids)
            batch = {tools.KEY_AUDIO: self.bank.clips(ids, firsts, self.num_frames)}
            batch.update(self.labels.clips(ids, firsts, self.num_frames))
            yield batch


# ------------------------------------------------------------------------------------------------------------------------------
# ground truth: the notes of a clip, sliced on the device
# ------------------------------------------------------------------------------------------------------------------------------
def cover_clips(frame_counts, num_frames):
    """(track_ids, first_frames, frames_left_out): consecutive, non-overlapping clips of `num_frames` frames that cover every track from
    frame 0 -- track i gives frame_counts[i] // num_frames clips -- and the number of frames no clip holds: every track's tail shorter
    than a clip, which is the whole of a track shorter than a clip.  Nothing is padded, nothing is counted twice.  Pure host code."""
    frame_counts = np.asarray(frame_counts, dtype=np.int64).reshape(-1)
    num_frames = int(num_frames)
    if num_frames < 1:
        raise ValueError(f'a clip has at least one frame (got {num_frames})')
    if (frame_counts < 0).any():
        raise ValueError(f'track {int(np.argmax(frame_counts < 0))} has a negative frame count')
    per_track = frame_counts // num_frames
    track_ids = np.repeat(np.arange(len(frame_counts), dtype=np.int64), per_track)
    first_frames = (np.arange(len(track_ids), dtype=np.int64) - np.repeat(np.cumsum(per_track) - per_track, per_track)) * num_frames
    return track_ids, first_frames, int((frame_counts - per_track * num_frames).sum())


def clip_windows(module, first_frames, num_frames):
    """(B, 2) float64 {sec_start, sec_stop} of the clips of `num_frames` frames that start at `first_frames`, by the reference's rule
    (amt_tools/datasets/common.py:343-358 with snap_to_frame): sample_start = first_frame * hop_length, seq_length =
    max(module.get_sample_range(num_frames)) (datasets/common.py:116: 319 999 samples for 625 frames at hop 512, not num_frames * hop_length),
    sec_start = sample_start / sample_rate, sec_stop = (sample_start + seq_length) / sample_rate -- Python floats, made here: the device
    never divides.  Pure host code."""
    hop, rate = int(module.hop_length), module.sample_rate
    seq_length = int(max(module.get_sample_range(int(num_frames))))
    windows = np.empty((len(first_frames), 2), dtype=np.float64)
    for b, first in enumerate(first_frames):
        sample_start = int(first) * hop
        windows[b] = sample_start / rate, (sample_start + seq_length) / rate
    return windows


def _note_order(rows):
    """Note rows in (pitch, onset) order: evaluate._sort_rows, the order amtx_eval_notes_match reads (a stable sort)."""
    return rows[np.lexsort((rows[:, 0], rows[:, 2]))]


class NoteClips(object):
    """What NoteBank.clips returns: `rows` (capacity, 3) float64 and `offsets` (batch * slices + 1,) int32 device tensors -- group
    clip * slices + slice owns rows[offsets[g]:offsets[g + 1]], the pair StackedNoteEvaluator.match_batch takes as `reference` --, `slices`
    (note groups per clip), `keys` (the stacked notes' keys; None for batched notes) and `total`: the rows of all groups as the host
    counted them (None when the caller set the capacity; offsets[-1] holds the kernel's total either way)."""

    def __init__(self, rows, offsets, slices, keys, total):
        self.rows, self.offsets, self.slices, self.keys, self.total = rows, offsets, slices, keys, total


class NoteBank(_Resident):
    """The note ground truth of whole tracks, for clips sliced on the device (amtx_note_clips, include/amtx_noteclips.h).

    notes[i]: the notes of track i, either a batched-notes array (N, 3) of rows [onset_s, offset_s, pitch] or a stacked-notes dictionary
    {key: (pitches, intervals)} (a tablature track: one entry per string).  All tracks are of one kind; stacked tracks carry the same keys
    in the same order (remembered as `keys`).  ValueError, naming track and row, for a NaN or infinite time and for offset < onset; with
    `bank` (the TrackBank / PyramidBank of the same tracks) for another track count.  `bank` also gives the clips their time windows
    (its module's hop length, sample rate and get_sample_range) and their frame counts; without it only window_clips / host_window_clips
    answer.

    One `rows` float64 (N, 3) table for all tracks and `group_ptr` int64 (num_tracks * slices + 1,): group track * slices + slice owns
    rows[group_ptr[g]:group_ptr[g + 1]], in (pitch, onset) order.  A time of -0.0 is stored as 0.0.  `integral`: every pitch is an integer
    in [0, 128), what the device matcher takes.  relative_times: whether a clip's times count from its own start (True: what a decoder
    whose grid starts at 0 needs) or stay absolute (False: what the reference's dataset returns).  The device copies are created on
    first use, never at construction, and never pickled."""

    def __init__(self, notes, bank=None, relative_times=True, device=None):
        self.device = device if device is not None else (bank.device if bank is not None else 'cuda')
        self.module = bank.module if bank is not None else None
        self.relative_times = bool(relative_times)
        self.keys, stacked, groups = None, None, []
        for i, entry in enumerate(notes):
            is_dict = isinstance(entry, dict)
            if stacked is None:
                stacked = is_dict
                self.keys = list(entry.keys()) if is_dict else None
                if is_dict and not self.keys:
                    raise ValueError('track 0 carries no stacked notes')
            if is_dict != stacked:
                raise ValueError(f'track {i} holds {"stacked" if is_dict else "batched"} notes, track 0 {"stacked" if stacked else "batched"} notes')
            if is_dict and list(entry.keys()) != self.keys:
                raise ValueError(f'track {i} carries the keys {list(entry.keys())}, track 0 {self.keys}')
            for key in (self.keys if is_dict else [None]):
                what = f'track {i}' + ('' if key is None else f', {key!r}')
                if is_dict:
                    pitches, intervals = entry[key]
                    pitches = np.asarray(pitches, dtype=np.float64).reshape(-1)
                    intervals = np.asarray(intervals, dtype=np.float64).reshape(-1, 2)
                    if len(pitches) != len(intervals):
                        raise ValueError(f'{what}: {len(pitches)} pitches for {len(intervals)} intervals')
                    rows = np.concatenate([intervals, pitches[:, None]], axis=-1)
                else:
                    rows = np.array(entry, dtype=np.float64)
                    if rows.size == 0:
                        rows = rows.reshape(0, 3)
                    if rows.ndim != 2 or rows.shape[1] != 3:
                        raise ValueError(f'{what}: batched notes are (N, 3) rows [onset, offset, pitch], not {rows.shape}')
                bad = ~np.isfinite(rows[:, :2]).all(axis=1)
                if bad.any():
                    raise ValueError(f'{what}, row {int(np.argmax(bad))}: a note time is NaN or infinite')
                bad = rows[:, 1] < rows[:, 0]
                if bad.any():
                    r = int(np.argmax(bad))
                    raise ValueError(f'{what}, row {r}: offset {float(rows[r, 1])!r} < onset {float(rows[r, 0])!r}')
                rows[:, :2] += 0.0                                 # -0.0 -> 0.0: max / min against a window then have one answer
                groups.append(_note_order(rows))
        if stacked is None:
            raise ValueError('notes: at least one track')
        self.slices = len(self.keys) if stacked else 1
        num_tracks = len(groups) // self.slices
        if bank is not None and num_tracks != len(bank):
            raise ValueError(f'notes of {num_tracks} tracks for a bank of {len(bank)}')
        self.frame_counts = None if bank is None else np.array(bank.frame_counts, dtype=np.int64)
        self.group_ptr = np.concatenate(([0], np.cumsum([len(g) for g in groups]))).astype(np.int64)
        self.rows = np.ascontiguousarray(np.concatenate(groups + [np.zeros((0, 3))], axis=0))
        pitch = self.rows[:, 2]
        self.integral = bool(np.all((pitch == np.floor(pitch)) & (pitch >= 0) & (pitch < 128)))
        # per group, its onsets and its offsets in ascending order: the host counts a clip's rows with two binary searches per group
        self._onsets = [np.sort(g[:, 0]) for g in groups]
        self._offsets = [np.sort(g[:, 1]) for g in groups]

    def __len__(self):
        return (len(self.group_ptr) - 1) // self.slices

    @property
    def stacked(self):
        return self.keys is not None

    @property
    def nbytes(self):
        """Bytes of the two tables, on the host as on the device."""
        return int(self.rows.nbytes + self.group_ptr.nbytes)

    def _upload(self, device):
        """(rows, group_ptr) on the bank's device; a bank without a note still uploads one (unread) row."""
        import torch
        rows = self.rows if len(self.rows) else np.zeros((1, 3))
        return torch.from_numpy(rows).to(device), torch.from_numpy(self.group_ptr).to(device)

    def _request(self, track_ids, first_frames, num_frames):
        """A checked clips(...) request -> (track ids, windows)."""
        if self.frame_counts is None:
            raise ValueError('a NoteBank built without a bank has no frame grid: name the clips by their windows (window_clips)')
        ids, firsts = _checked_request(self.frame_counts, track_ids, first_frames, num_frames)
        return ids, clip_windows(self.module, firsts, num_frames)

    def _checked_windows(self, track_ids, windows):
        ids = np.asarray(track_ids, dtype=np.int64).reshape(-1)
        windows = np.ascontiguousarray(windows, dtype=np.float64).reshape(-1, 2)
        if len(ids) != len(windows) or ids.size == 0:
            raise ValueError('one (start_time, stop_time) per track id, and at least one clip')
        bad = (ids < 0) | (ids >= len(self))
        if bad.any():
            raise ValueError(f'unknown track {int(ids[bad][0])}: the bank holds {len(self)} tracks')
        bad = ~(windows[:, 0] <= windows[:, 1]) | ~np.isfinite(windows).all(axis=1) | (windows[:, 0] < 0)
        if bad.any():
            b = int(np.argmax(bad))
            raise ValueError(f'clip {b}: the window [{float(windows[b, 0])!r}, {float(windows[b, 1])!r}] is not 0 <= start_time <= stop_time, both finite')
        return ids, windows + 0.0

    def count_clips(self, track_ids, windows):
        """(batch * slices,) int64: the rows every group of window_clips holds, from two binary searches per group.  A row is dropped for
        offset <= start_time or for onset > stop_time, never for both (onset <= offset, start_time <= stop_time).  Pure host code."""
        ids, windows = self._checked_windows(track_ids, windows)
        counts = np.empty(len(ids) * self.slices, dtype=np.int64)
        for b, (track, (start, stop)) in enumerate(zip(ids, windows)):
            for s in range(self.slices):
                g = int(track) * self.slices + s
                counts[b * self.slices + s] = np.searchsorted(self._onsets[g], stop, side='right') - np.searchsorted(self._offsets[g], start, side='right')
        return counts

    def host_window_clips(self, track_ids, windows):
        """window_clips answered with NumPy: one (n, 3) float64 array per group clip * slices + slice, the reference's slice_batched_notes
        (amt_tools/tools/utils.py:345-359) statement by statement.  The CPU restatement of the kernel."""
        ids, windows = self._checked_windows(track_ids, windows)
        out = []
        for track, (start, stop) in zip(ids, windows):
            for s in range(self.slices):
                g = int(track) * self.slices + s
                rows = self.rows[self.group_ptr[g]:self.group_ptr[g + 1]]
                rows = rows[rows[:, 1] > start]
                rows = rows[rows[:, 0] <= stop]
                rows[:, 0] = np.maximum(rows[:, 0], start)
                rows[:, 1] = np.minimum(rows[:, 1], stop)
                if self.relative_times:
                    rows[:, :2] -= start
                out.append(rows)
        return out

    def window_clips(self, track_ids, windows, rows_capacity=None):
        """The notes of the clips (track_ids[b], windows[b] = (start_time, stop_time)) as a NoteClips: one amtx_note_clips call.
        rows_capacity None: the buffer holds exactly the rows count_clips counts, so nothing is cut; a given capacity may be too
        small, and then offsets[-1] still holds the true total and the rows past the capacity are not written."""
        import torch
        ids, windows = self._checked_windows(track_ids, windows)
        total = int(self.count_clips(ids, windows).sum()) if rows_capacity is None else None
        capacity = max(total, 1) if rows_capacity is None else int(rows_capacity)
        rows, group_ptr = self._device_state()
        device = rows.device
        batch = len(ids)
        rows_out = torch.empty((capacity, 3), dtype=torch.float64, device=device)
        offsets = torch.empty((batch * self.slices + 1,), dtype=torch.int32, device=device)
        ws = _lib.alloc_workspace(int(_lib.call('amtx_note_clips_workspace_bytes', batch, self.slices)), device)
        _lib.call('amtx_note_clips', rows, group_ptr, len(self), self.slices, torch.from_numpy(ids).to(device),
                  torch.from_numpy(windows).to(device), batch, int(self.relative_times), rows_out, capacity, offsets, ws, ws.numel(), device=device)
        return NoteClips(rows_out, offsets, self.slices, self.keys, total)

    def clips(self, track_ids, first_frames, num_frames, rows_capacity=None):
        """The notes of the clips [first_frames[b], first_frames[b] + num_frames) of the tracks track_ids[b], as a NoteClips.  Same signature
        and host validation as bank.clips (_checked_request against the bank's frame counts); the windows are clip_windows'."""
        return self.window_clips(*self._request(track_ids, first_frames, num_frames), rows_capacity=rows_capacity)

    def host_clips(self, track_ids, first_frames, num_frames):
        """The same request answered with NumPy (host_window_clips): the fallback for pitches the device matcher does not take."""
        return self.host_window_clips(*self._request(track_ids, first_frames, num_frames))

    def _checked_tracks(self, track_ids):
        ids = np.asarray(track_ids, dtype=np.int64).reshape(-1)
        if ids.size == 0:
            raise ValueError('at least one track')
        bad = (ids < 0) | (ids >= len(self))
        if bad.any():
            raise ValueError(f'unknown track {int(ids[bad][0])}: the bank holds {len(self)} tracks')
        return ids

    def host_whole(self, track_ids):
        """The unsliced notes of whole tracks with NumPy: one (n, 3) float64 array per group track * slices + slice, in the bank's
        (pitch, onset) order, times as the constructor took them.  Nothing is clamped and nothing is dropped: a note with offset == 0,
        which every window that starts at 0 drops (offset <= start_time), is still there."""
        out = []
        for track in self._checked_tracks(track_ids):
            for g in range(int(track) * self.slices, (int(track) + 1) * self.slices):
                out.append(self.rows[self.group_ptr[g]:self.group_ptr[g + 1]].copy())
        return out

    def whole(self, track_ids):
        """The unsliced notes of whole tracks as a NoteClips -- host_whole on the device: `rows` and int32 `offsets` of the tracks' groups,
        taken from the resident table by index arithmetic.  Consecutive tracks give a view of the table, anything else one gather; no
        kernel of this library runs.  A whole track starts at time 0, so relative and absolute times are the same."""
        import torch
        ids = self._checked_tracks(track_ids)
        rows, _ = self._device_state()
        lo, hi = self.group_ptr[ids * self.slices], self.group_ptr[(ids + 1) * self.slices]
        # per group its size, in request order
        sizes = np.concatenate([np.diff(self.group_ptr[int(t) * self.slices:(int(t) + 1) * self.slices + 1]) for t in ids])
        offsets = np.concatenate(([0], np.cumsum(sizes)))
        total = int(offsets[-1])
        if total >= 2 ** 31:
            raise ValueError(f'{total} notes: the offsets of a NoteClips are int32')
        if total == 0:
            out = rows[:1]                                   # the (unread) row every NoteClips holds at least
        elif (np.diff(ids) == 1).all():
            out = rows[int(lo[0]):int(hi[-1])]
        else:
            index = np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in zip(lo, hi)])
            out = rows[torch.from_numpy(index).to(rows.device)]
        return NoteClips(out, torch.from_numpy(offsets.astype(np.int32)).to(rows.device), self.slices, self.keys, total)


# ------------------------------------------------------------------------------------------------------------------------------
# whole tracks from overlapped clips
# ------------------------------------------------------------------------------------------------------------------------------
# What seam_clips returns.  track_ids / first_frames: the clips, (n,) int64 each, in track order; kept: (n, 3) int64 rows
# {dst_first_frame, src_first_col, count} -- clip j keeps its columns [src_first_col, src_first_col + count), which are the frames
# [dst_first_frame, dst_first_frame + count) of its track; short: (m,) int64, the requested tracks shorter than a clip, in request order.
SeamPlan = namedtuple('SeamPlan', 'track_ids first_frames kept short')


def seam_clips(frame_counts, num_frames, margin, track_ids=None):
    """Equally long, overlapping clips that cover whole tracks, and the frames each clip keeps: a SeamPlan.  Of a clip only frames at
    least `margin` frames away from a clip edge that is not a track edge are kept.  With stride = num_frames - 2 * margin, a track of
    L >= num_frames frames gives the clips at 0, stride, 2 * stride, ... while first + num_frames < L, then one last clip at
    L - num_frames (its right edge is the track's own end).  The seams are 0, the middle first_{j+1} + (first_j + num_frames -
    first_{j+1}) // 2 of every overlap, and L; clip j keeps the track's frames [seam_j, seam_{j+1}).  Every frame is kept exactly once.

    track_ids: the tracks to cover, in this order (default: every track).  A track with L < num_frames gives no clip and is named in
    `short`: it fits one clip of its own length.  ValueError for margin < 0, num_frames - 2 * margin < 1 and an unknown track.
    Pure host code."""
    frame_counts = np.asarray(frame_counts, dtype=np.int64).reshape(-1)
    num_frames, margin = int(num_frames), int(margin)
    if margin < 0:
        raise ValueError(f'margin={margin}: the frames left out at a clip edge cannot be negative')
    stride = num_frames - 2 * margin
    if stride < 1:
        raise ValueError(f'num_frames={num_frames} with margin={margin}: a clip keeps num_frames - 2 * margin frames, at least one')
    ids = np.arange(len(frame_counts), dtype=np.int64) if track_ids is None else np.asarray(track_ids, dtype=np.int64).reshape(-1)
    bad = (ids < 0) | (ids >= len(frame_counts))
    if bad.any():
        raise ValueError(f'unknown track {int(ids[bad][0])}: the bank holds {len(frame_counts)} tracks')
    tracks, firsts, kept, short = [], [], [], []
    for t in ids.tolist():
        L = int(frame_counts[t])
        if L < num_frames:
            short.append(t)
            continue
        first = list(range(0, L - num_frames, stride)) + [L - num_frames]
        seams = [0] + [b + (a + num_frames - b) // 2 for a, b in zip(first[:-1], first[1:])] + [L]
        for j, f in enumerate(first):
            tracks.append(t)
            firsts.append(f)
            kept.append((seams[j], seams[j] - f, seams[j + 1] - seams[j]))
    return SeamPlan(np.array(tracks, dtype=np.int64), np.array(firsts, dtype=np.int64), np.array(kept, dtype=np.int64).reshape(-1, 3),
                    np.array(short, dtype=np.int64))


def _stitch_args(dst, src, desc, is_tensor):
    """What stitch_host and stitch_clips check alike -> (batch, rows, num_frames) of src."""
    if src.ndim < 2 or src.shape[0] < 1 or src.shape[-1] < 1 or int(np.prod(src.shape)) == 0:
        raise ValueError(f'src is (batch, rows..., num_frames) with at least one of each, not {tuple(src.shape)}')
    if dst.ndim != 1 or not (dst.is_contiguous() if is_tensor else dst.flags.c_contiguous):
        raise ValueError('dst is one flat, contiguous buffer')
    if src.dtype != dst.dtype:
        raise TypeError(f'src holds {src.dtype}, dst {dst.dtype}')
    if desc.ndim != 2 or desc.shape != (src.shape[0], 5):
        raise ValueError(f'one descriptor row {{base, L, dst_first, src_first, count}} per clip: ({src.shape[0]}, 5), not {desc.shape}')
    batch, num_frames = int(src.shape[0]), int(src.shape[-1])
    return batch, int(np.prod(src.shape)) // (batch * num_frames), num_frames


def stitch_host(dst, src, desc):
    """amtx_stitch_clips with NumPy (include/amtx_stitch.h): dst[base_b + r * L_b + dst_first_b + i] = src[b][r][src_first_b + i] for every
    row {base, L, dst_first, src_first, count} of `desc`, in place; returns dst.  src: (batch, rows..., num_frames); dst: a flat array of
    the same dtype.  ValueError for a row the entry point refuses.  The CPU restatement of the kernel."""
    src, desc = np.asarray(src), np.asarray(desc, dtype=np.int64)
    batch, rows, num_frames = _stitch_args(dst, src, desc, False)
    for b, (base, L, dst_first, src_first, count) in enumerate(desc.tolist()):
        if min(base, L, dst_first, src_first, count) < 0 or src_first + count > num_frames or dst_first + count > L or base + rows * L > dst.size:
            raise ValueError(f'clip {b}: the row {(base, L, dst_first, src_first, count)} leaves the clip, the track or dst')
    flat = src.reshape(batch, rows, num_frames)
    for b, (base, L, dst_first, src_first, count) in enumerate(desc.tolist()):
        dst[base:base + rows * L].reshape(rows, L)[:, dst_first:dst_first + count] = flat[b, :, src_first:src_first + count]
    return dst


STITCH_DTYPES = ('torch.float32', 'torch.int64')       # 4-byte maps (piano rolls, offset probabilities) and the 8-byte tablature


def stitch_clips(dst, src, desc, desc_dev=None):
    """One amtx_stitch_clips launch on the current stream: the kept columns of every clip of the device tensor `src` (batch, rows...,
    num_frames) into the flat device tensor `dst`, by the int64 (batch, 5) host table `desc` (stitch_host's).  desc_dev: its device copy,
    when the caller has uploaded it already.  float32 and int64 are taken, as bit patterns.  Shapes, dtypes and devices are checked
    here, before the library is entered; the rows of `desc` by the entry point, before anything is launched."""
    import torch
    if not (torch.is_tensor(src) and torch.is_tensor(dst)):
        raise TypeError('src and dst are device tensors (stitch_host takes arrays)')
    if not src.is_cuda or dst.device != src.device:
        raise ValueError(f'src ({src.device}) and dst ({dst.device}) are on one GPU')
    if str(src.dtype) not in STITCH_DTYPES:
        raise TypeError(f'a stitched map holds float32 or int64 elements, not {src.dtype}')
    desc = np.ascontiguousarray(desc, dtype=np.int64)
    batch, rows, num_frames = _stitch_args(dst, src, desc, True)
    if desc_dev is None:
        desc_dev = torch.from_numpy(desc).to(src.device)
    elif desc_dev.device != src.device or desc_dev.dtype != torch.int64 or tuple(desc_dev.shape) != desc.shape or not desc_dev.is_contiguous():
        raise ValueError('desc_dev is the contiguous int64 copy of desc on the GPU of src')
    _lib.call('amtx_stitch_clips', src.contiguous(), src.element_size(), batch, rows, num_frames, desc, desc_dev, dst, dst.numel(), device=src.device)
    return dst


class TrackMaps(object):
    """The whole-track outputs of a set of tracks on the device: per key ONE flat allocation that holds every track's (rows..., L_t) map
    back to back, each contiguous with its own width.  `frame_counts`: (n,) frames of the tracks, in the order of the slots 0 .. n - 1;
    `base[key]`: (n,) int64, the element at which every slot's map starts.  Nothing downstream sees padding: `track(j, key)` is the
    (1, rows..., L_j) view the decoders and evaluators take as a batch of one.

    A key is added with the shape and dtype of its maps (`add`); the drivers do that when the first batch shows them.  The memory is
    not initialised: a plan that keeps every frame exactly once (seam_clips) writes all of it."""

    def __init__(self, frame_counts, device):
        self.frame_counts = np.array(frame_counts, dtype=np.int64).reshape(-1)
        if self.frame_counts.size == 0 or (self.frame_counts < 1).any():
            raise ValueError('frame_counts: at least one track, at least one frame each')
        self.device = device
        self._first = np.concatenate(([0], np.cumsum(self.frame_counts)))         # frames in front of every slot, and of the end
        self.base, self._flat, self._shape = {}, {}, {}

    def __len__(self):
        return len(self.frame_counts)

    @property
    def keys(self):
        return list(self._flat)

    @property
    def nbytes(self):
        """Bytes of all allocations."""
        return int(sum(t.numel() * t.element_size() for t in self._flat.values()))

    def add(self, key, shape, dtype):
        """Allocate the maps under `key`: `shape` is a map's shape without its frame axis ((88,) for a piano roll, (6,) for a tablature),
        dtype torch.float32 or torch.int64."""
        import torch
        if key in self._flat:
            raise ValueError(f"the maps already hold '{key}'")
        if str(dtype) not in STITCH_DTYPES:
            raise TypeError(f"'{key}': a stitched map holds float32 or int64 elements, not {dtype}")
        shape = tuple(int(s) for s in shape)
        rows = int(np.prod(shape)) if shape else 1
        if rows < 1:
            raise ValueError(f"'{key}': a map has at least one row, not the shape {shape}")
        self._shape[key], self.base[key] = shape, self._first[:-1] * rows
        self._flat[key] = torch.empty((int(self._first[-1]) * rows,), dtype=dtype, device=self.device)

    def rows(self, key):
        return int(np.prod(self._shape[key])) if self._shape[key] else 1

    def flat(self, key):
        """The allocation under `key`: 1-D, slot j at [base[key][j], base[key][j] + rows * frame_counts[j])."""
        return self._flat[key]

    def track(self, j, key):
        """The map of slot j under `key` as a batch of one: a contiguous (1, rows..., L_j) view."""
        at, L = int(self.base[key][j]), int(self.frame_counts[j])
        return self._flat[key][at:at + self.rows(key) * L].view((1,) + self._shape[key] + (L,))

    def descriptors(self, key, slots, kept):
        """The (n, 5) int64 table {base, L, dst_first, src_first, count} of clips whose tracks are the slots `slots` and whose kept
        columns are the (n, 3) rows `kept` of a SeamPlan.  ValueError for an unknown slot."""
        slots, kept = np.asarray(slots, dtype=np.int64).reshape(-1), np.asarray(kept, dtype=np.int64).reshape(-1, 3)
        if len(slots) != len(kept) or ((slots < 0) | (slots >= len(self))).any():
            raise ValueError(f'one slot below {len(self)} per row of kept columns')
        return _clip_table(self.base[key][slots], self.frame_counts[slots], kept[:, 0], kept[:, 1], kept[:, 2])

    def stitch(self, key, src, desc, desc_dev=None):
        """stitch_clips of one batch tensor into the maps under `key`; its shape between batch and frames is the maps'."""
        if tuple(src.shape[1:-1]) != self._shape[key]:
            raise ValueError(f"'{key}': a batch of {tuple(src.shape[1:-1])} maps for maps of {self._shape[key]}")
        stitch_clips(self._flat[key], src, desc, desc_dev)

    def host(self, key):
        """Every slot's map on the host, (rows..., L_j) each: one copy of the allocation, sliced."""
        flat = self._flat[key].cpu().numpy()
        rows = self.rows(key)
        return [flat[int(at):int(at) + rows * int(L)].reshape(self._shape[key] + (int(L),)) for at, L in zip(self.base[key], self.frame_counts)]


# ------------------------------------------------------------------------------------------------------------------------------
# exact whole tracks: packed rows (include/amtx_ofseq.h, inference._exact_tracks)
# ------------------------------------------------------------------------------------------------------------------------------
def track_groups(frame_counts, max_rows):
    """The language passes of a request: [(lo, hi)] ranges of its slots, in request order.  Tracks are taken until the next would bring a
    pass above `max_rows` packed rows; a track longer than max_rows runs alone and is never split.  Pure host code."""
    counts = np.asarray(frame_counts, dtype=np.int64).reshape(-1)
    if int(max_rows) < 1:
        raise ValueError(f'max_rows={max_rows}: a language pass holds at least one row')
    groups, lo, rows = [], 0, 0
    for j, L in enumerate(counts.tolist()):
        if j > lo and rows + L > int(max_rows):
            groups.append((lo, j))
            lo, rows = j, 0
        rows += L
    if len(counts):
        groups.append((lo, len(counts)))
    return groups


def sequence_table(frame_counts):
    """(row0, table) of tracks whose rows are packed back to back in slot order: row0 (n,) int64, the packed row at which slot j starts,
    and the (n, 2) int64 sequence table {row0, len} the packed-sequence kernels take, listed LONGEST FIRST (ties in slot order) -- a
    block's slots are consecutive rows of the table, so they finish together.  Rows are addressed through row0: no data moves for it."""
    counts = np.asarray(frame_counts, dtype=np.int64).reshape(-1)
    if counts.size == 0 or (counts < 1).any():
        raise ValueError('frame_counts: at least one track, at least one frame each')
    row0 = np.concatenate(([0], np.cumsum(counts)[:-1])).astype(np.int64)
    order = np.argsort(-counts, kind='stable')
    return row0, _clip_table(row0[order], counts[order])


def gather_table(row0, slots, kept):
    """The (n, 3) int64 table {src_first, count, dst_row} of amtx_rows_gather for clips whose tracks are the slots `slots` and whose kept
    columns are the (n, 3) rows {dst_first_frame, src_first_col, count} of a SeamPlan: the kept rows of clip j land at packed row
    row0[slot_j] + dst_first_frame_j."""
    row0, slots, kept = np.asarray(row0, dtype=np.int64), np.asarray(slots, dtype=np.int64).reshape(-1), np.asarray(kept, dtype=np.int64).reshape(-1, 3)
    if len(slots) != len(kept) or ((slots < 0) | (slots >= len(row0))).any():
        raise ValueError(f'one slot below {len(row0)} per row of kept columns')
    return _clip_table(kept[:, 1], kept[:, 2], row0[slots] + kept[:, 0])


def gather_rows_host(dst, src, table):
    """amtx_rows_gather with NumPy: dst[dst_row_b + i] = src[b][src_first_b + i] for every row {src_first, count, dst_row} of `table` and
    i < count, in place; returns dst.  src: (batch, num_frames, width...), dst: (total_rows, width...) of the same dtype.  ValueError for a
    row the entry point refuses.  The CPU restatement of the kernel."""
    src, table = np.asarray(src), np.asarray(table, dtype=np.int64)
    if src.ndim < 2 or dst.ndim != src.ndim - 1 or dst.shape[1:] != src.shape[2:] or dst.dtype != src.dtype:
        raise ValueError(f'src is (batch, num_frames, width...), dst (total_rows, width...) of one dtype: {src.shape} {src.dtype}, {dst.shape} {dst.dtype}')
    if table.shape != (src.shape[0], 3):
        raise ValueError(f'one row {{src_first, count, dst_row}} per clip: ({src.shape[0]}, 3), not {table.shape}')
    for b, (first, count, row) in enumerate(table.tolist()):
        if min(first, count, row) < 0 or first + count > src.shape[1] or row + count > dst.shape[0]:
            raise ValueError(f'clip {b}: the row {(first, count, row)} leaves the clip or the packed rows')
    for b, (first, count, row) in enumerate(table.tolist()):
        dst[row:row + count] = src[b, first:first + count]
    return dst
