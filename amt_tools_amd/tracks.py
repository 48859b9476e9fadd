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

Features only: callers slice their label maps with the same first frames.  A TrackBank of raw audio serves STFT / MelSpec modules only:
the CQT family has no clip form there.
"""

import numpy as np

from . import _lib

__all__ = ['TrackBank', 'TrackClips', 'PyramidBank', 'PyramidClips', 'clip_descriptors', 'frame_start']


def frame_start(sample_start, hop_length):
    """First frame of a clip that starts at `sample_start`: the reference's rule (amt_tools/datasets/common.py:392)."""
    return int(sample_start) // int(hop_length)


def clip_descriptors(starts, lengths, frame_counts, track_ids, first_frames, num_frames, reflect_half=None):
    """The table amtx_spec_power_clips reads: int64 (B, 4) rows {track_start, track_len, first_frame, frames}, frames = num_frames, for the
    clips [first_frames[b], first_frames[b] + num_frames) of the tracks track_ids[b].  starts / lengths / frame_counts describe the bank
    (element offset, samples and frames of every track).  reflect_half: n_fft // 2 of a reflect-padded plan (librosa 0.9), else None.

    Pure host code.  ValueError for an unknown track, a negative first frame, a clip that runs past its track's last frame (a track shorter
    than the clip included) and for a reflect-padded plan over a track of n_fft / 2 samples or fewer."""
    starts, lengths, frame_counts = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (starts, lengths, frame_counts))
    track_ids = np.asarray(track_ids, dtype=np.int64).reshape(-1)
    first_frames = np.asarray(first_frames, dtype=np.int64).reshape(-1)
    num_frames = int(num_frames)
    if not (len(starts) == len(lengths) == len(frame_counts)):
        raise ValueError('starts, lengths and frame_counts describe the same tracks: one entry each')
    if track_ids.shape != first_frames.shape or track_ids.size == 0:
        raise ValueError('one first frame per track id, and at least one clip')
    if num_frames < 1:
        raise ValueError(f'a clip has at least one frame (got {num_frames})')
    bad = (track_ids < 0) | (track_ids >= len(starts))
    if bad.any():
        raise ValueError(f'unknown track {int(track_ids[bad][0])}: the bank holds {len(starts)} tracks')
    if (first_frames < 0).any():
        raise ValueError(f'negative first frame {int(first_frames[first_frames < 0][0])}')
    past = first_frames + num_frames > frame_counts[track_ids]
    if past.any():
        b = int(np.argmax(past))
        raise ValueError(f'clip {b}: frames [{int(first_frames[b])}, {int(first_frames[b]) + num_frames}) run past the '
                         f'{int(frame_counts[track_ids[b]])} frames of track {int(track_ids[b])}')
    if reflect_half is not None:
        short = lengths[track_ids] <= int(reflect_half)
        if short.any():
            b = int(np.argmax(short))
            raise ValueError(f'track {int(track_ids[b])} has {int(lengths[track_ids[b]])} samples: reflect padding needs more than '
                             f'n_fft/2 = {int(reflect_half)}')
    desc = np.empty((track_ids.size, 4), dtype=np.int64)
    desc[:, 0] = starts[track_ids]
    desc[:, 1] = lengths[track_ids]
    desc[:, 2] = first_frames
    desc[:, 3] = num_frames
    return desc


def _reflect_half(module):
    return int(module.n_fft) // 2 if module._pad_mode() == 1 else None


class TrackClips(object):
    """Clips of a TrackBank, as a batch entry under tools.KEY_AUDIO or an argument of process_clips / power_clips:
    `bank`, `desc` (host int64 (B, 4), clip_descriptors), `desc_dev` (its device copy) and `db_ref` ((B,) device float32: the power
    maxima of the clips' tracks).  No tensor subclass: tools.dict_to_device passes it through as it is."""

    def __init__(self, bank, desc, desc_dev, db_ref):
        self.bank, self.desc, self.desc_dev, self.db_ref = bank, desc, desc_dev, db_ref

    @property
    def num_clips(self):
        return int(self.desc.shape[0])

    @property
    def num_frames(self):
        return int(self.desc[0, 3])

    @property
    def device(self):
        return self.desc_dev.device


class TrackBank(object):
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

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('_dev', None)
        return state

    def _device_state(self):
        """(audio, db_ref) on the bank's device."""
        dev = self.__dict__.get('_dev')
        if dev is None:
            import torch
            from .features import _index_of
            device = torch.device('cuda', _index_of(self.device))
            plan = self.module._get_plan(device)
            # the kernel's contract counts frames as amtx_spec_num_frames does; the host bookkeeping (module.get_expected_frames) must agree,
            # or clips near a track's end would be framed from padding (the reference's own count differs for a module that is not
            # centred with win_length < n_fft: features/waveform.py:43-67)
            for i, n in enumerate(self.lengths):
                frames = int(_lib.call('amtx_spec_num_frames', plan, int(n)))
                if frames != int(self.frame_counts[i]):
                    raise ValueError(f'track {i} ({int(n)} samples): the module expects {int(self.frame_counts[i])} frames, its plan computes {frames}')
            audio = torch.from_numpy(self._host).to(device)
            desc = torch.from_numpy(self._track_desc).to(device)
            db_ref = torch.empty((len(self),), dtype=torch.float32, device=device)
            # power = NULL: maxima only; `frames` = each track's own count, rows per clip = the longest track's
            _lib.call('amtx_spec_power_clips', plan, audio, desc, len(self), int(self.frame_counts.max()), None, db_ref,
                      device=device)
            dev = self.__dict__['_dev'] = (audio, db_ref)
        return dev

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
        import torch
        desc = clip_descriptors(self.starts, self.lengths, self.frame_counts, track_ids, first_frames, num_frames, _reflect_half(self.module))
        audio, db_ref = self._device_state()
        ids = torch.from_numpy(np.asarray(track_ids, dtype=np.int64).reshape(-1)).to(audio.device)
        return TrackClips(self, desc, torch.from_numpy(desc).to(audio.device), db_ref[ids])


class PyramidClips(object):
    """Clips of a PyramidBank, as a batch entry under tools.KEY_AUDIO or an argument of a CQT-family module's process_clips / power_clips:
    `bank`, `desc` (host int64 (B, 3) rows {track, first_frame, frames}), `desc_dev` (its device copy) and `db_ref` ((B, n_harm) device
    float32: per harmonic, the power maxima of the clips' tracks)."""

    def __init__(self, bank, desc, desc_dev, db_ref):
        self.bank, self.desc, self.desc_dev, self.db_ref = bank, desc, desc_dev, db_ref

    @property
    def num_clips(self):
        return int(self.desc.shape[0])

    @property
    def num_frames(self):
        return int(self.desc[0, 2])

    @property
    def device(self):
        return self.desc_dev.device


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

    def _device_state(self):
        """(audio, db_ref, pyramid, track table) on the bank's device."""
        dev = self.__dict__.get('_dev')
        if dev is None:
            import ctypes as C
            import torch
            from .features import _index_of
            device = torch.device('cuda', _index_of(self.device))
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
                # the host bookkeeping (module.get_expected_frames) must agree with the plan, or clips near a track's end would not exist
                if frames.value != int(self.frame_counts[i]):
                    raise ValueError(f'track {i} ({int(n)} samples): the module expects {int(self.frame_counts[i])} frames, its plan computes {frames.value}')
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
            dev = self.__dict__['_dev'] = (audio, db_ref, pyramid, table_dev)
        return dev

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
        """`num_frames` frames from first_frames[b] on of track track_ids[b], as a PyramidClips; validated on the host as clip_descriptors
        does (unknown track, negative first frame, a clip past its track's last frame, fewer than one frame)."""
        import torch
        checked = clip_descriptors(self.starts, self.lengths, self.frame_counts, track_ids, first_frames, num_frames)
        ids = np.asarray(track_ids, dtype=np.int64).reshape(-1)
        desc = np.ascontiguousarray(np.stack((ids, checked[:, 2], checked[:, 3]), axis=1))
        audio, db_ref = self._device_state()[:2]
        return PyramidClips(self, desc, torch.from_numpy(desc).to(audio.device), db_ref[torch.from_numpy(ids).to(audio.device)])
