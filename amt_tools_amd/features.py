"""
Host-side mirror of amt-tools' FeatureModule plugin API (amt_tools/features/*.py) for the hot path's
spectral front-end, backed by the HIP kernels behind include/amtx.h.

Same class names, constructor keywords, method set and return conventions as the reference
(FeatureModule: features/common.py:15-321; WaveformWrapper bookkeeping: features/waveform.py:43-185;
STFT: features/stft.py; MelSpec: features/mel.py), so a `TranscriptionDataset`, `FeatureStream` or the
paper scripts can be handed these objects unchanged:

    process_audio(audio: np.ndarray (N,)) -> np.ndarray (C, F, T) float32      # seam S1

plus additions the reference does not have:

    process_batch(audio: torch.Tensor (B, N) on the GPU) -> torch.Tensor (B, C, F, T)   # batched, stays on device
    process_clips(clips: tracks.TrackClips) -> torch.Tensor (B, 1, F, T)                # frames cut from resident tracks, track-level dB
    process_clips(clips: tracks.PyramidClips) -> torch.Tensor (B, C, F, T)              # the same for the CQT family, from resident pyramids
    frontend()  -> nn.Module for `TranscriptionModel.frontend` (models/common.py:56-57,107-120): the
                   fused seam -- features are computed on the device inside `pre_proc`.

`librosa_version` selects the centre-padding convention of the librosa release the reference would
have resolved ('0.10': zeros, '0.9': reflect; SURVEY finding F12).

The GPU context is created lazily on first use (never at construction), so instances can be built
before DataLoader workers fork.  There is no CPU fallback: without the HIP extension or a GPU,
process_audio raises.
"""

import ctypes as C

import numpy as np

from . import _lib

__all__ = ['FeatureModule', 'WaveformWrapper', 'STFT', 'MelSpec', 'VQT', 'CQT', 'HVQT', 'HCQT']

FLOAT32 = 'float32'


class FeatureModule(object):
    """Generic feature-extraction module (features/common.py:15-321)."""

    def __init__(self, sample_rate, hop_length, num_channels, decibels=True):
        self.sample_rate = sample_rate
        self.hop_length = hop_length
        self.num_channels = num_channels
        self.decibels = decibels

    # ---- frame / sample bookkeeping (row A0) -------------------------------------------------
    def get_expected_frames(self, audio):
        num_frames = 0
        if audio.shape[-1] != 0:
            num_frames = 1 + len(audio) // self.hop_length
        return num_frames

    def get_sample_range(self, num_frames):
        sample_range = np.array([0])
        if num_frames > 0:
            max_samples = num_frames * self.hop_length - 1
            min_samples = max(1, max_samples - self.hop_length + 1)
            sample_range = np.arange(min_samples, max_samples + 1)
        return sample_range

    def get_num_samples_required(self):
        return self.get_sample_range(1)[-1]

    @staticmethod
    def divisor_pad(audio, divisor):
        pad_amt = divisor - (audio.shape[-1] % divisor)
        if pad_amt > 0 and pad_amt != divisor:
            audio = np.append(audio, np.zeros(pad_amt).astype(FLOAT32), axis=-1)
        return audio

    def frame_pad(self, audio):
        divisor = self.get_num_samples_required()
        if audio.shape[-1] > divisor:
            divisor = self.hop_length
        return self.divisor_pad(audio, divisor)

    def process_audio(self, audio):
        raise NotImplementedError

    # ---- host-array helpers kept for API parity (the device path fuses them into K2) --------
    def to_decibels(self, feats):
        """amplitude_to_db(ref=np.max) on a host array (features/common.py:181-201)."""
        mag = np.abs(np.asarray(feats))
        ref = mag.max() if mag.size else 1.0
        db = 10.0 * np.log10(np.maximum(1e-10, np.square(mag))) - 10.0 * np.log10(np.maximum(1e-10, ref ** 2))
        return np.maximum(db, db.max() - 80.0) if mag.size else db

    def post_proc(self, feats):
        if self.decibels:
            feats = self.to_decibels(feats)
            feats = feats / 80
            feats = feats + 1
        return np.expand_dims(feats, axis=0)

    def get_times(self, audio):
        frame_idcs = np.arange(self.get_expected_frames(audio))
        # librosa.frames_to_time: samples / sr in float64
        return (frame_idcs * self.hop_length).astype(np.float64) / float(self.sample_rate)

    def get_sample_rate(self):
        return self.sample_rate

    def get_hop_length(self):
        return self.hop_length

    def get_num_channels(self):
        return self.num_channels

    def get_feature_size(self):
        raise NotImplementedError

    @classmethod
    def features_name(cls):
        return cls.__name__


class WaveformWrapper(FeatureModule):
    """Frame bookkeeping of waveform-domain modules (features/waveform.py)."""

    def __init__(self, sample_rate=44100, hop_length=512, decibels=False, win_length=None, center=True):
        super().__init__(sample_rate=sample_rate, hop_length=hop_length, num_channels=1, decibels=decibels)
        if win_length is None:
            win_length = self.hop_length
        self.win_length = win_length
        self.center = center

    def get_expected_frames(self, audio):
        if self.center or audio.shape[-1] == 0:
            return super().get_expected_frames(audio)
        return 1 + ((max(0, (audio.shape[-1] - self.win_length)) - 1) // self.hop_length + 1)

    def get_sample_range(self, num_frames):
        if self.center or num_frames == 0:
            return super().get_sample_range(num_frames)
        if num_frames == 1:
            return np.arange(1, self.win_length + 1)
        return np.arange(1, self.hop_length + 1) + self.get_num_samples_required() + (num_frames - 2) * self.hop_length

    def center_pad(self, audio):
        half = int(self.win_length // 2)
        return np.pad(audio, [(half, half)], mode='constant')

    def process_audio(self, audio):
        """Raw framing (features/waveform.py:121-153): (win_length, T) strided frames, host only."""
        if audio.shape[-1] == 0:
            return np.zeros((self.win_length, 0))
        audio = self.center_pad(audio) if self.center else self.frame_pad(audio)
        n_frames = 1 + (audio.shape[-1] - self.win_length) // self.hop_length
        idx = np.arange(self.win_length)[:, None] + self.hop_length * np.arange(n_frames)[None, :]
        return audio[idx]

    def get_times(self, audio, at_start=False):
        times = super().get_times(audio)
        if self.center and at_start:
            times -= ((self.win_length // 2) / self.sample_rate)
        elif not self.center and not at_start:
            times += ((self.win_length // 2) / self.sample_rate)
        return times

    def get_feature_size(self):
        return self.win_length


def _index_of(device):
    """Device index of an int / str / torch.device ('cuda' without an index = the current device)."""
    import torch
    if isinstance(device, int):
        return device
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _lib.AmtxError(f'the HIP front-end runs on a GPU, not on {dev}')
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _bank_of(module, clips, what):
    """The bank of `clips`, which must belong to `module` itself or to a module of the same plan (_same_plan): `what` of the bank are
    those of its module's plan."""
    bank = clips.bank
    if bank.module is not module and not module._same_plan(bank.module):
        raise ValueError(f'the clips come from a bank of another module: its {what} are those of its own plan')
    return bank


class _PlanOwner(object):
    """Lazily created plans (device tables) of a feature module, one per device index.  A subclass names its ABI prefix (`<_ABI>_create` /
    `_destroy`), its "no GPU visible" text, what pickling drops, and states its plan ONCE: _plan_args()."""

    _ABI = None                 # 'amtx_spec_plan' / 'amtx_cqt_plan'
    _NO_GPU = None              # the text for a process that sees no GPU
    _TRANSIENT = ('_plans',)    # __dict__ keys that hold device pointers or tensors: never pickled (DataLoader workers, torch.save)

    def _plan_args(self):
        """The plan as a tuple of plain Python values: the arguments `<_ABI>_create` is called with (_create_args) AND the identity _same_plan
        compares -- one list, so a plan parameter cannot be in the one and not in the other."""
        raise NotImplementedError

    def _create_args(self):
        return self._plan_args()

    def _same_plan(self, other):
        """What lets the clips of `other`'s bank run under this module."""
        return type(other) is type(self) and other._plan_args() == self._plan_args()

    def _get_plan(self, device=None):
        """The plan (device tables) for `device` (a torch.device / index; default: the module's own device).  Plans are cached per
        device index and created under that device, so a module built with the default device='cuda:0' can be handed tensors that
        live on another GPU (one process per GPU under torchrun: rank k's tensors are on cuda:k) without its kernels
        dereferencing cuda:0 allocations."""
        import torch
        index = self._device_index() if device is None else _index_of(device)
        plans = self.__dict__.setdefault('_plans', {})
        plan = plans.get(index)
        if plan is None:
            if not torch.cuda.is_available():
                raise _lib.AmtxError(self._NO_GPU)
            handle = C.c_void_p()
            _lib.call(self._ABI + '_create', C.byref(handle), *self._create_args(), device=index)
            plan = plans[index] = handle
        return plan

    def _device_index(self):
        return _index_of(self.device)

    def change_device(self, device):
        """Follow the model to its device (TranscriptionModel.change_device propagates here through SpectralFrontend)."""
        self.device = device

    def __getstate__(self):
        state = dict(self.__dict__)
        for key in self._TRANSIENT:
            state.pop(key, None)
        return state

    def __del__(self):
        for plan in self.__dict__.get('_plans', {}).values():
            try:
                _lib.call(self._ABI + '_destroy', plan)
            except Exception:
                pass

    def _workspace_for(self, need, device):
        """The module's one kernel workspace: kept from call to call, replaced when it is too small or lives on another device."""
        ws = self.__dict__.get('_workspace')
        if ws is None or ws.numel() < need or ws.device != device:
            self.__dict__['_workspace'] = None
            ws = self.__dict__['_workspace'] = _lib.alloc_workspace(need, device)
        return ws

    def _process_host(self, audio):
        import torch
        dev = torch.device('cuda', self._device_index())
        x = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)).to(dev).unsqueeze(0)
        return self.process_batch(x)[0].cpu().numpy()

    def frontend(self):
        """nn.Module wrapper for `TranscriptionModel.frontend`: (B,1,N) audio -> (B,C,F,T) features."""
        from .models import SpectralFrontend
        return SpectralFrontend(self)


class _SpecPlanOwner(_PlanOwner):
    """The amtx_spec_plan shared by STFT / MelSpec instances."""

    _ABI = 'amtx_spec_plan'
    _NO_GPU = 'no GPU visible: the spectral front-end has no CPU fallback'
    _TRANSIENT = ('_plans', '_prof_events')

    # ---- device path -------------------------------------------------------------------------
    def power_batch(self, audio):
        """K1 on a (B, N) float32 CUDA tensor -> (power (B,T,F) fp32, clip_max (B,))."""
        import torch
        assert audio.is_cuda and audio.dtype == torch.float32 and audio.dim() == 2
        audio = audio.contiguous()
        B, N = audio.shape
        plan = self._get_plan(audio.device)
        T = _lib.call('amtx_spec_num_frames', plan, N)
        F = _lib.call('amtx_spec_num_bins', plan)
        power = torch.empty((B, T, F), dtype=torch.float32, device=audio.device)
        clip_max = torch.empty((B,), dtype=torch.float32, device=audio.device)
        with torch.cuda.device(audio.device):
            ev = self._prof_begin()
            _lib.call('amtx_spec_power', plan, audio, N, audio.stride(0) if B > 1 else N, B, power, clip_max, device=audio.device)
            self._prof_end('spec_power', ev)
        return power, clip_max

    # optional per-kernel timing (bench.py): events are recorded on the current stream, which is the stream
    # the kernels are launched on
    def _prof_begin(self):
        if self.__dict__.get('_prof_events') is None:
            return None
        import torch
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def _prof_end(self, name, ev):
        if ev is None:
            return
        import torch
        end = torch.cuda.Event(enable_timing=True)
        end.record()
        self._prof_events.append((name, ev, end))

    def scale_batch(self, power, clip_max, ref=None, model_layout=False):
        """K2: dB / scale + layout.  Returns (B,1,F,T) (reference layout) or (B,1,T,F) (model layout)."""
        import torch
        B, T, F = power.shape
        if self.decibels:
            transform = 0
        else:
            transform = 1 if self._linear_is_power else 2
        out = torch.empty((B, 1, T, F) if model_layout else (B, 1, F, T), dtype=torch.float32, device=power.device)
        with torch.cuda.device(power.device):
            ev = self._prof_begin()
            _lib.call('amtx_spec_scale', self._get_plan(power.device), power, clip_max, ref, B, T, transform, 1 if model_layout else 0, out,
                      device=power.device)
            self._prof_end('spec_scale', ev)
        return out

    def process_batch(self, audio, ref=None, model_layout=False):
        """Batched features on the device: (B, N) float32 CUDA tensor -> (B, 1, F, T) float32."""
        power, clip_max = self.power_batch(audio)
        return self.scale_batch(power, clip_max, ref, model_layout)

    # ---- clips cut from device-resident tracks (amt_tools_amd/tracks.py) -----------------------------------
    def power_clips(self, clips):
        """K1 on a TrackClips: (power (B,T,F) fp32, track_max (B,)).  Row t of clip b is frame first_frame[b] + t of its track, bit for
        bit the row amtx_spec_power gives for the whole track; track_max is the maximum of the clip's TRACK (TrackBank.db_ref).  The clips'
        OWN maxima, which the kernel also reduces (the ABI takes no null clip_max), are dropped on purpose: a bank exists for the track's."""
        import torch
        audio = _bank_of(self, clips, 'track maxima').audio
        B, T = clips.num_clips, clips.num_frames
        plan = self._get_plan(audio.device)
        F = _lib.call('amtx_spec_num_bins', plan)
        power = torch.empty((B, T, F), dtype=torch.float32, device=audio.device)
        own_max = torch.empty((B,), dtype=torch.float32, device=audio.device)     # written, never read (docstring)
        with torch.cuda.device(audio.device):
            ev = self._prof_begin()
            _lib.call('amtx_spec_power_clips', plan, audio, clips.desc_dev, B, T, power, own_max, device=audio.device)
            self._prof_end('spec_power', ev)
        return power, clips.db_ref

    def process_clips(self, clips, model_layout=False):
        """Features of a TrackClips on the device, (B, 1, F, T) float32 (model layout: (B, 1, T, F)): the slices
        [first_frame, first_frame + num_frames) of the tracks' own feature maps, bit for bit -- scaled against the track's maximum,
        the 80 dB floor below that same maximum, edge frames from the track's samples (SURVEY finding F7)."""
        power, track_max = self.power_clips(clips)
        return self.scale_batch(power, track_max, track_max, model_layout)

    def _process_host(self, audio, empty_rows):
        if audio.shape[-1] == 0:
            return np.zeros((1, empty_rows, 0))
        return super()._process_host(audio)


class STFT(WaveformWrapper, _SpecPlanOwner):
    """Magnitude spectrogram (features/stft.py) on the GPU."""
    _linear_is_power = False

    def __init__(self, sample_rate=16000, hop_length=512, decibels=True, win_length=None, center=True, n_fft=2048,
                 librosa_version='0.10', device='cuda:0'):
        self.n_fft = n_fft
        if win_length is None:
            win_length = self.n_fft
        WaveformWrapper.__init__(self, sample_rate=sample_rate, hop_length=hop_length, decibels=decibels,
                                 win_length=win_length, center=center)
        self.librosa_version = str(librosa_version)
        self.device = device

    def _pad_mode(self):
        return 1 if self.librosa_version.startswith('0.9') else 0

    def _plan_args(self):
        return (int(self.sample_rate), int(self.n_fft), int(self.hop_length), int(self.win_length), 0, 0,
                int(bool(self.center)), self._pad_mode())

    def process_audio(self, audio):
        # the reference reports n_fft rows for empty audio (features/stft.py:57-59)
        return self._process_host(audio, self.n_fft)

    def get_feature_size(self):
        return self.n_fft // 2 + 1


class MelSpec(STFT):
    """Mel spectrogram (features/mel.py): n_mels triangular Slaney-normalised filters on |STFT|^2,
    power_to_db(ref=max) -> /80 + 1."""
    _linear_is_power = True

    def __init__(self, sample_rate=16000, hop_length=512, decibels=True, n_mels=229, n_fft=2048, win_length=None,
                 center=True, htk=False, librosa_version='0.10', device='cuda:0'):
        super().__init__(sample_rate=sample_rate, hop_length=hop_length, decibels=decibels, win_length=win_length,
                         center=center, n_fft=n_fft, librosa_version=librosa_version, device=device)
        self.n_mels = n_mels
        self.htk = htk

    def _plan_args(self):
        return (int(self.sample_rate), int(self.n_fft), int(self.hop_length), int(self.win_length), int(self.n_mels),
                int(bool(self.htk)), int(bool(self.center)), self._pad_mode())

    def process_audio(self, audio):
        return self._process_host(audio, self.n_mels)

    def to_decibels(self, feats):
        """power_to_db(ref=np.max) on a host array (features/mel.py:78-96)."""
        S = np.asarray(feats)
        ref = S.max() if S.size else 1.0
        db = 10.0 * np.log10(np.maximum(1e-10, S)) - 10.0 * np.log10(np.maximum(1e-10, ref))
        return np.maximum(db, db.max() - 80.0) if S.size else db

    def get_feature_size(self):
        return self.n_mels

    def filterbank(self):
        """Dense (n_mels, n_fft//2+1) float32 copy of the plan's filterbank (for inspection/tests)."""
        out = np.zeros((self.n_mels, self.n_fft // 2 + 1), dtype=np.float32)
        _lib.call('amtx_spec_filterbank', self._get_plan(), out)
        return out


# ======================================================================================================
# CQT / VQT / HCQT / HVQT  (amt_tools/features/vqt.py, cqt.py, hvqt.py, hcqt.py)
# ======================================================================================================
C1_HZ = 32.70319566257483            # librosa.note_to_hz('C1')
_HANN_BANDWIDTH = 1.50018310546875   # librosa.filters.window_bandwidth('hann')


def _early_downsample_count(nyquist, filter_cutoff, hop_length, n_octaves):
    """librosa.core.constantq.__early_downsample_count, which the reference imports (features/vqt.py:7,95)."""
    c1 = max(0, int(np.ceil(np.log2(nyquist / filter_cutoff)) - 1) - 1)
    twos, h = 0, int(hop_length)
    while h > 0 and h % 2 == 0:
        twos, h = twos + 1, h // 2
    return min(c1, max(0, twos - n_octaves + 1))


class _CqtPlanOwner(_PlanOwner):
    """The amtx_cqt_plan shared by the VQT-family modules."""

    _ABI = 'amtx_cqt_plan'
    _NO_GPU = 'no GPU visible: the CQT front-end has no CPU fallback'
    _TRANSIENT = ('_plans', '_workspace')
    _truncate = False           # HVQT: the harmonics are truncated to the smallest frame count

    def _plan_args(self):
        return (int(self.sample_rate), int(self.hop_length), float(self.fmin), int(self.n_bins), int(self.bins_per_octave), float(self.gamma),
                tuple(float(h) for h in getattr(self, 'harmonics', (1.0,))), int(self._truncate), int(str(self.librosa_version).startswith('0.9')))

    def _create_args(self):
        args = self._plan_args()
        harmonics = args[6]                                  # the ABI takes them as (const double*, count)
        return args[:6] + ((C.c_double * len(harmonics))(*harmonics), len(harmonics)) + args[7:]

    def change_device(self, device):
        self.device = device
        for m in getattr(self, 'modules', []):              # HVQT / HCQT: the per-harmonic VQTs
            m.device = device

    def _audio_args(self, audio, max_harmonics=None):
        """Check the audio, get its device's plan, the sizes and the workspace: (plan, audio, N, row stride, B), T, H, workspace."""
        import torch
        assert audio.is_cuda and audio.dtype == torch.float32 and audio.dim() == 2
        audio = audio.contiguous()
        B, N = audio.shape
        plan = self._get_plan(audio.device)
        T = _lib.call('amtx_cqt_num_frames', plan, N)
        H = _lib.call('amtx_cqt_num_harmonics', plan)
        assert max_harmonics is None or H <= max_harmonics
        ws = self._workspace_for(_lib.call('amtx_cqt_workspace_bytes', plan, B, N), audio.device)
        return (plan, audio, N, audio.stride(0) if B > 1 else N, B), T, H, ws

    def _staged16(self, entry, args, B, T, split, device):
        """The (B, T, F, 8) bfloat16 map of `entry`(*args, out), or with `split` the two planes (2, B, T, F, 8) of `entry`_split."""
        import torch
        out = torch.empty(((2,) if split else ()) + (B, T, self.n_bins, 8), dtype=torch.bfloat16, device=device)
        if split:
            _lib.call(entry + '_split', *args, out, out[0].numel(), device=device)
        else:
            _lib.call(entry, *args, out, device=device)
        return out

    def process_batch(self, audio, model_layout=False):
        """(B, N) float32 CUDA tensor -> (B, C, F, T) float32 features on the device."""
        import torch
        args, T, H, ws = self._audio_args(audio)
        device = args[1].device
        out = torch.empty((args[-1], H, self.n_bins, T), dtype=torch.float32, device=device)
        _lib.call('amtx_cqt_forward', *args, int(bool(self.decibels)), ws, ws.numel(), out, device=device)
        return out

    def process_batch16(self, audio, split=False):
        """(B, N) float32 CUDA tensor -> (B, T, F, 8) bfloat16: the features of process_batch rounded to bf16 and laid out the way the
        Onsets & Frames engine's first conv kernel stages them (amtx_cqt_forward16: a position's harmonics in one 16-byte slot, slots
        C .. 7 zero) -- what OnsetsFrames.run_on_batch hands its engine when the model takes it (amtx_of_forward_feats16).
        split=True: (2, B, T, F, 8) -- plane 0 that map, plane 1 = bf16(feature - plane 0): the two planes the x3 engine multiplies with
        (amtx_cqt_forward16_split)."""
        args, T, _, ws = self._audio_args(audio, max_harmonics=8)
        return self._staged16('amtx_cqt_forward16', args + (int(bool(self.decibels)), ws, ws.numel()), args[-1], T, split, args[1].device)

    # ---- clips cut from the resident pyramids of whole tracks (amt_tools_amd/tracks.py, include/amtx_pyramid.h) ---------------
    def _clips_args(self, clips, max_harmonics=None, workspace=True):
        """(plan, audio, pyramid, track table, descriptors, B, T) of a PyramidClips of this module's plan, H and the workspace; anything
        else raises."""
        from .tracks import PyramidClips
        if not isinstance(clips, PyramidClips):
            raise NotImplementedError(f'{type(self).__name__}: the decimation pyramid has no clip form over raw audio (clips of the CQT family '
                                      f'come from a tracks.PyramidBank, those of a TrackBank from STFT / MelSpec)')
        bank = _bank_of(self, clips, 'pyramids and track maxima')
        audio = bank.audio
        plan, B, T = self._get_plan(audio.device), clips.num_clips, clips.num_frames
        H = _lib.call('amtx_cqt_num_harmonics', plan)
        assert max_harmonics is None or H <= max_harmonics
        ws = self._workspace_for(_lib.call('amtx_cqt_clips_workspace_bytes', plan, B, T), audio.device) if workspace else None
        return (plan, audio, bank.pyramid, bank.table, clips.desc_dev, B, T), H, ws

    def power_clips(self, clips):
        """A PyramidClips -> (power (B, H, F, T) fp32, db_ref (B, H)): column t of clip b is frame first_frame[b] + t of its track's power
        map, bit for bit; db_ref holds the maxima of the clips' TRACKS per harmonic (PyramidBank.db_ref)."""
        import torch
        args, H, _ = self._clips_args(clips, workspace=False)
        B, T, device = args[-2], args[-1], args[1].device
        power = torch.empty((B, H, self.n_bins, T), dtype=torch.float32, device=device)
        _lib.call('amtx_cqt_power_clips', *args, power, device=device)
        return power, clips.db_ref

    def process_clips(self, clips, model_layout=False):
        """Features of a PyramidClips on the device, (B, H, F, T) float32 (model layout: (B, H, T, F)): the slices
        [first_frame, first_frame + num_frames) of the tracks' own feature maps, bit for bit -- each harmonic scaled against its maximum
        over the whole track, edge frames from the track's samples (SURVEY finding F7)."""
        import torch
        args, H, ws = self._clips_args(clips)
        B, T, device = args[-2], args[-1], args[1].device
        out = torch.empty((B, H, self.n_bins, T), dtype=torch.float32, device=device)
        _lib.call('amtx_cqt_clips', *args, clips.db_ref, int(bool(self.decibels)), ws, ws.numel(), out, device=device)
        return out.transpose(-1, -2) if model_layout else out

    def process_clips16(self, clips, split=False):
        """A PyramidClips -> (B, T, F, 8) bfloat16, or (2, B, T, F, 8) with `split`: process_batch16 of the clips' tracks, sliced on T."""
        args, _, ws = self._clips_args(clips, max_harmonics=8)
        return self._staged16('amtx_cqt_clips16', args + (clips.db_ref, int(bool(self.decibels)), ws, ws.numel()), args[-2], args[-1], split,
                              args[1].device)


class VQT(FeatureModule, _CqtPlanOwner):
    """Variable-Q transform (features/vqt.py)."""

    def __init__(self, sample_rate=22050, hop_length=512, decibels=True, fmin=None, n_bins=84, bins_per_octave=12, gamma=None,
                 librosa_version='0.10', device='cuda:0'):
        FeatureModule.__init__(self, sample_rate, hop_length, 1, decibels)
        self.fmin = C1_HZ if fmin is None else fmin
        self.n_bins = n_bins
        self.bins_per_octave = bins_per_octave
        self.window = 'hann'
        # the reference keeps alpha in the librosa-0.9 convention and derives the default gamma from it (vqt.py:51-58)
        self.alpha = 2.0 ** (1.0 / self.bins_per_octave) - 1
        self.gamma = 24.7 * self.alpha / 0.108 if gamma is None else gamma
        self.n_octs = int(np.ceil(float(self.n_bins) / self.bins_per_octave))
        self.librosa_version = str(librosa_version)
        self.device = device

    def get_early_ds_count(self):
        fmax = self.fmin * 2.0 ** ((self.n_bins - 1) / self.bins_per_octave)
        cQ = 1.0 / (2.0 ** (1. / self.bins_per_octave) - 1)
        freq_cutoff = fmax * (1 + 0.5 * (_HANN_BANDWIDTH / cQ)) + 0.5 * self.gamma
        return _early_downsample_count(self.sample_rate / 2.0, freq_cutoff, self.hop_length, self.n_octs)

    def get_expected_frames(self, audio):
        early = self.get_early_ds_count()
        k = np.arange(early, early + self.n_octs)
        sig_lens = np.ceil(len(audio) / (2 ** k))
        hop_lens = self.hop_length // (2 ** k)
        return int(min(sig_lens // hop_lens + 1))

    def get_sample_range(self, num_frames):
        factor = 2 ** self.get_early_ds_count()
        max_samples = ((num_frames * self.hop_length // factor) - 1) * factor
        min_samples = max(1, max_samples - self.hop_length + 1)
        return np.arange(min_samples, max_samples + 1)

    def process_audio(self, audio):
        return self._process_host(audio)

    def get_times(self, audio, at_start=False):
        times = super().get_times(audio)
        if at_start:
            # intended behaviour of vqt.py:217-225 (the reference floor-divides the tuple wavelet_lengths returns)
            alpha = self.alpha
            longest = (1.0 / alpha) * self.sample_rate / (self.fmin + self.gamma / alpha)
            times -= ((longest // 2) / self.sample_rate)
        return times

    def get_feature_size(self):
        return self.n_bins


class CQT(VQT):
    """Constant-Q transform = VQT with gamma = 0 (features/cqt.py)."""

    def __init__(self, sample_rate=22050, hop_length=512, decibels=True, fmin=None, n_bins=84, bins_per_octave=12,
                 librosa_version='0.10', device='cuda:0'):
        super().__init__(sample_rate, hop_length, decibels, fmin, n_bins, bins_per_octave, gamma=0,
                         librosa_version=librosa_version, device=device)


class HVQT(FeatureModule, _CqtPlanOwner):
    """Harmonic VQT (features/hvqt.py): one VQT per harmonic h * fmin, each dB-normalised on its own, truncated to the
    smallest expected frame count, stacked on the channel axis.  All harmonics run in one device pass: harmonics that
    are octaves apart share pyramid levels (and GEMM launches)."""

    def __init__(self, sample_rate=22050, hop_length=512, decibels=True, fmin=None, harmonics=None, n_bins=84, bins_per_octave=12,
                 gamma=None, librosa_version='0.10', device='cuda:0'):
        self.fmin = C1_HZ if fmin is None else fmin
        if harmonics is None:
            harmonics = [0.5, 1, 2, 3, 4, 5]
        harmonics.sort()
        self.harmonics = harmonics
        FeatureModule.__init__(self, sample_rate, hop_length, len(self.harmonics), decibels)
        self.modules = [VQT(sample_rate=sample_rate, hop_length=hop_length, decibels=decibels, fmin=h * self.fmin, n_bins=n_bins,
                            bins_per_octave=bins_per_octave, gamma=gamma, librosa_version=librosa_version, device=device)
                        for h in self.harmonics]
        self.n_bins = n_bins
        self.bins_per_octave = bins_per_octave
        self.gamma = self.modules[0].gamma
        self.librosa_version = str(librosa_version)
        self.device = device

    _truncate = True

    def get_expected_frames(self, audio):
        return min(module.get_expected_frames(audio) for module in self.modules)

    def get_sample_range(self, num_frames):
        return self.modules[-1].get_sample_range(num_frames)

    def process_audio(self, audio):
        return self._process_host(audio)

    def get_times(self, audio, at_start=False):
        return self.modules[0].get_times(audio, at_start)[:self.get_expected_frames(audio)]

    def get_feature_size(self):
        return self.modules[0].get_feature_size()


class HCQT(HVQT):
    """Harmonic CQT (features/hcqt.py)."""

    def __init__(self, sample_rate=22050, hop_length=512, decibels=True, fmin=None, harmonics=None, n_bins=84, bins_per_octave=12,
                 librosa_version='0.10', device='cuda:0'):
        super().__init__(sample_rate, hop_length, decibels, fmin, harmonics, n_bins, bins_per_octave, gamma=0,
                         librosa_version=librosa_version, device=device)
