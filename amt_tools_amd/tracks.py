"""
Training clips cut from device-resident tracks, with the reference's track-level semantics.

The reference computes a track's feature map ONCE and slices frames [frame_start, frame_start + num_frames) out of it, with
frame_start = sample_start // hop_length (amt_tools/datasets/common.py:325-327, 340-354, 392).  A clip's features are therefore
(1) scaled against the TRACK's maximum -- power_to_db(ref=np.max) and the 80 dB floor both see the whole map (features/mel.py:94,
features/common.py:199, 218-225; SURVEY finding F7) -- and (2) framed from the track's own samples at the clip's edges, not from padding.

`TrackBank` keeps whole tracks in one device buffer together with every track's power maximum; `bank.clips(...)` names frames of those
tracks, and `module.process_clips(clips)` (amt_tools_amd/features.py) returns exactly the slices of the track's own feature map, bit for
bit, without ever writing that map: amtx_spec_power_clips frames each clip out of its track (include/amtx_tracks.h).

Features only: callers slice their label maps with the same first frames.  STFT / MelSpec modules only; the CQT family's decimation
pyramid has no clip form.
"""

import numpy as np

from . import _lib

__all__ = ['TrackBank', 'TrackClips', 'clip_descriptors', 'frame_start']


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
            raise NotImplementedError(f'{type(module).__name__}: the decimation pyramid of the CQT family has no clip form')
        if not isinstance(module, _SpecPlanOwner):
            raise TypeError(f'a TrackBank takes an STFT or MelSpec of this package, not {type(module).__name__}')
        tracks = [np.ascontiguousarray(t, dtype=np.float32) for t in tracks]
        if not tracks or any(t.ndim != 1 or t.size == 0 for t in tracks):
            raise ValueError('tracks: at least one, each a non-empty 1-D array of samples')
        self.module = module
        self.device = module.device if device is None else device
        self.lengths = np.array([t.size for t in tracks], dtype=np.int64)
        self.starts = np.concatenate(([0], np.cumsum(self.lengths)[:-1])).astype(np.int64)
        self.frame_counts = np.array([module.get_expected_frames(t) for t in tracks], dtype=np.int64)
        if (self.frame_counts < 1).any():
            raise ValueError(f'track {int(np.argmin(self.frame_counts))} is too short for one frame')
        self._host = np.concatenate(tracks)
        # every track whole: the descriptors of the maxima launch (validated like any clip request)
        self._track_desc = np.concatenate([clip_descriptors(self.starts, self.lengths, self.frame_counts, [i], [0], n, _reflect_half(module))
                                           for i, n in enumerate(self.frame_counts)])

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
