"""
Host-side contract pieces of amt_tools.tools that the hot path touches: dictionary keys
(amt_tools/tools/constants.py:46-69,118-137), the PianoProfile (amt_tools/tools/instrument.py:13-100),
dict plumbing with the reference's semantics (amt_tools/tools/utils.py:3505-3745) but without its
repeated whole-batch deep copies, activation helpers and RMS normalisation.
"""

import numpy as np

try:
    import torch
except Exception:   # pragma: no cover
    torch = None

# ---- dictionary keys / constants (values are the contract, amt_tools/tools/constants.py) ----------
KEY_TRACK = 'track'
KEY_AUDIO = 'audio'
KEY_FS = 'fs'
KEY_HOP = 'hop_length'
KEY_FEATS = 'features'
KEY_MULTIPITCH = 'multi_pitch'
KEY_PITCHLIST = 'pitch_list'
KEY_ONSETS = 'onsets'
KEY_OFFSETS = 'offsets'
KEY_TIMES = 'times'
KEY_TABLATURE = 'tablature'
KEY_NOTES = 'notes'
KEY_OUTPUT = 'model_output'
KEY_LOSS = 'loss'
KEY_LOSS_TOTAL = 'loss_total'
KEY_LOSS_ONSETS = 'loss_onsets'
KEY_LOSS_OFFSETS = 'loss_offsets'
KEY_LOSS_PITCH = 'loss_pitch'
KEY_LOSS_FRAMES = 'loss_frames'     # not the reference's: per-clip loss sums over a frame window of each clip (models.TranscriptionModel.run_on_batch)
KEY_ACCURACY = 'accuracy'
KEY_PRECISION = 'precision'
KEY_RECALL = 'recall'
KEY_F1 = 'f1-score'
KEY_TDR = 'tdr'
VAL = 'validation'
TXT_EXT = 'txt'
DEFAULT_PIANO_LOWEST_PITCH = 21
DEFAULT_PIANO_HIGHEST_PITCH = 108
DEFAULT_GUITAR_LABELS = ['E', 'A', 'D', 'G', 'B', 'e']
DEFAULT_GUITAR_TUNING = ['E2', 'A2', 'D3', 'G3', 'B3', 'E4']
DEFAULT_GUITAR_NUM_FRETS = 19
FLOAT32 = 'float32'
FLOAT64 = 'float64'
PYT_MODEL = 'model'
PYT_STATE = 'opt-state'
PYT_EXT = 'pt'


class InstrumentProfile(object):
    def __init__(self, low, high):
        self.low = low
        self.high = high

    def get_midi_range(self):
        return np.arange(self.low, self.high + 1)

    def get_range_len(self):
        return self.high - self.low + 1


class PianoProfile(InstrumentProfile):
    """88 keys, MIDI 21..108 (amt_tools/tools/instrument.py:65-100)."""

    def __init__(self, low=None, high=None):
        super().__init__(DEFAULT_PIANO_LOWEST_PITCH if low is None else low,
                         DEFAULT_PIANO_HIGHEST_PITCH if high is None else high)

    def get_num_dofs(self):
        return 1


def note_to_midi(note):
    """'E2' -> 40, 'A#3' / 'Bb3' -> 58 (scientific pitch notation, C4 = 60): what librosa.note_to_midi returns for the plain
    note names the instrument profiles use (amt_tools/tools/instrument.py:148-160)."""
    if isinstance(note, (list, tuple)):
        return [note_to_midi(n) for n in note]
    pc = {'C': 0, 'D': 2, 'E': 4, 'F': 5, 'G': 7, 'A': 9, 'B': 11}[note[0].upper()]
    i = 1
    while i < len(note) and note[i] in '#b':
        pc += 1 if note[i] == '#' else -1
        i += 1
    octave = int(note[i:]) if i < len(note) else 0
    return 12 * (octave + 1) + pc


class TablatureProfile(InstrumentProfile):
    """Instruments with several degrees of freedom, e.g. strings (amt_tools/tools/instrument.py:103-260)."""

    def __init__(self, tuning, num_pitches):
        self.tuning = tuning
        self.num_pitches = num_pitches
        midi_tuning = self.get_midi_tuning()
        super().__init__(midi_tuning[0], midi_tuning[-1] - 1 + self.num_pitches)

    def get_num_dofs(self):
        return len(self.tuning)

    def get_midi_tuning(self):
        return note_to_midi(list(self.tuning))

    def get_dof_midi_range(self):
        tuning = self.get_midi_tuning()
        return np.array([np.arange(tuning[i], tuning[i] + self.num_pitches) for i in range(self.get_num_dofs())])

    def get_fret(self, midi_pitch, string):
        return midi_pitch - self.get_midi_tuning()[string]

    def get_pitch(self, string, fret):
        return self.get_midi_tuning()[string] + fret


class GuitarProfile(TablatureProfile):
    """Six strings in standard tuning, 19 frets by default (amt_tools/tools/instrument.py:263-305)."""

    def __init__(self, tuning=None, num_frets=None):
        if tuning is None:
            tuning = DEFAULT_GUITAR_TUNING
        if num_frets is None:
            num_frets = DEFAULT_GUITAR_NUM_FRETS
        super().__init__(tuning, num_frets + 1)

    def get_num_frets(self):
        return self.num_pitches - 1


# ---- dict plumbing ---------------------------------------------------------------------------------
def unpack_dict(data, key):
    """Entry for `key`, or None (amt_tools/tools/utils.py:3823-3853)."""
    return data[key] if (isinstance(data, dict) and key in data) else None


def query_dict(dictionary, key):
    return isinstance(dictionary, dict) and key in dictionary.keys()


def get_tag(tag=None):
    """Name for a file that belongs to a track: the track's own name, or date and time when it has none (amt_tools/tools/utils.py:3881-3905)."""
    if tag is None:
        from datetime import datetime
        tag = datetime.now().strftime('%m_%d_%Y_%H_%M_%S')
    return tag


def _map_dict(track, fn):
    """New dict (recursively), every leaf passed through fn; the caller's dict is never mutated."""
    out = dict()
    for k, v in track.items():
        out[k] = _map_dict(v, fn) if isinstance(v, dict) else fn(v)
    return out


def dict_to_device(track, device):
    return _map_dict(track, lambda v: v.to(device) if torch is not None and isinstance(v, torch.Tensor) else v)


def dict_to_dtype(track, dtype):
    return _map_dict(track, lambda v: v.astype(dtype) if isinstance(v, np.ndarray) else v)


def dict_to_tensor(track):
    return _map_dict(track, lambda v: torch.from_numpy(v) if isinstance(v, np.ndarray) else v)


def array_to_tensor(data, device=None):
    """amt_tools/tools/utils.py:3438-3465."""
    if isinstance(data, np.ndarray):
        data = torch.from_numpy(data)
        if device is not None:
            data = data.to(device)
    return data


def framify_activations(activations, win_length, hop_length=1, pad=True):
    """Overlapping windows along the last axis: (..., T) -> (..., T', win_length), centre zero padding by win_length // 2 when
    `pad` (amt_tools/tools/utils.py:2922-2984; librosa.util.pad_center = symmetric zero padding, extra sample on the right)."""
    num_frames = activations.shape[-1]
    pad_length = win_length // 2
    num_frames_ = num_frames + 2 * pad_length if pad else max(win_length, num_frames)
    lpad = (num_frames_ - num_frames) // 2
    widths = [(0, 0)] * (activations.ndim - 1) + [(lpad, num_frames_ - num_frames - lpad)]
    activations = np.pad(activations, widths, mode='constant')
    num_hops = (num_frames_ - 2 * pad_length) // hop_length
    chunks = [np.expand_dims(activations[..., i: i + win_length], axis=-2) for i in np.arange(0, num_hops) * hop_length]
    return np.concatenate(chunks, axis=-2)


def tensor_to_array(data):
    if torch is not None and isinstance(data, torch.Tensor):
        data = data.cpu().detach().numpy()
    return data


def dict_to_array(track):
    return _map_dict(track, tensor_to_array)


def dict_unsqueeze(track, dim=0):
    def f(v):
        if torch is not None and isinstance(v, torch.Tensor):
            return v.unsqueeze(dim)
        if isinstance(v, np.ndarray):
            return np.expand_dims(v, axis=dim)
        return v
    return _map_dict(track, f)


def dict_squeeze(track, dim=None):
    def f(v):
        if (torch is not None and isinstance(v, torch.Tensor)) or isinstance(v, np.ndarray):
            if dim is None:
                return v.squeeze()
            if v.ndim > 0 and v.shape[dim] == 1:
                return v.squeeze(dim)
        return v
    out = dict()
    for k, v in track.items():
        # the reference recurses into nested dicts WITHOUT forwarding `dim` (utils.py:3681-3683)
        out[k] = dict_squeeze(v) if isinstance(v, dict) else f(v)
    return out


# ---- activation helpers ----------------------------------------------------------------------------
def threshold_activations(activations, threshold=0.5):
    """In place, like the reference (amt_tools/tools/utils.py:2896-2919): < thr -> 0, everything else -> 1."""
    activations[activations < threshold] = 0
    activations[activations != 0] = 1
    return activations


def multi_pitch_to_onsets(multi_pitch):
    """Positive first difference along time, first frame counts (amt_tools/tools/utils.py:2381-2412).
    Accepts ndarray or tensor; returns the same kind."""
    if torch is not None and isinstance(multi_pitch, torch.Tensor):
        onsets = torch.cat([multi_pitch[..., :1], multi_pitch[..., 1:] - multi_pitch[..., :-1]], dim=-1)
        return torch.clamp(onsets, min=0)
    onsets = np.concatenate([multi_pitch[..., :1], multi_pitch[..., 1:] - multi_pitch[..., :-1]], axis=-1)
    onsets[onsets <= 0] = 0
    return onsets


def multi_pitch_to_offsets(multi_pitch):
    """Where activity ceases; pitches active in the last frame count (amt_tools/tools/utils.py:2555-2589).
    Accepts ndarray or tensor; returns the same kind."""
    if torch is not None and isinstance(multi_pitch, torch.Tensor):
        offsets = torch.cat([multi_pitch[..., :-1] - multi_pitch[..., 1:], multi_pitch[..., -1:]], dim=-1)
        return torch.clamp(offsets, min=0)
    offsets = np.concatenate([multi_pitch[..., :-1] - multi_pitch[..., 1:], multi_pitch[..., -1:]], axis=-1)
    offsets[offsets <= 0] = 0
    return offsets


# ---- tablature -> pitch maps / stacked notes (the guitar estimators' arithmetic) --------------------
def _tab_geometry(profile):
    """(dof_start (S,), classes per string, pitch rows of the map) of a TablatureProfile (tools/utils.py:2013-2025)."""
    dof_start = np.asarray(profile.get_midi_tuning(), dtype=np.int64) - profile.low
    return dof_start, int(profile.num_pitches), int(profile.get_range_len())


def tab_expand(tablature, profile, stacked=True, collapsed=False):
    """Device path of the two functions below in ONE pass (amtx_tab_expand, csrc/tabnotes.hip): (..., S, T) int64 CUDA tablature ->
    (stacked (..., S, P, T) or None, collapsed (..., P, T) or None), fp32 like every other map the engines hand out.  Raises AmtxError
    when a class of the profile would land outside the map (or for more strings than the kernel is built for: no fallback here)."""
    from . import _lib
    assert tablature.is_cuda and tablature.dtype == torch.int64 and tablature.dim() >= 2 and (stacked or collapsed)
    dof_start, num_classes, P = _tab_geometry(profile)
    lead, (S, T) = tuple(tablature.shape[:-2]), tablature.shape[-2:]
    assert S == len(dof_start), (S, len(dof_start))
    B = int(np.prod(lead)) if lead else 1
    tab = tablature.contiguous()
    dev = tab.device
    st = torch.empty(lead + (S, P, T), dtype=torch.float32, device=dev) if stacked else None
    co = torch.empty(lead + (P, T), dtype=torch.float32, device=dev) if collapsed else None
    if B * S * T > 0:
        start = np.ascontiguousarray(dof_start, dtype=np.int32)
        _lib.call('amtx_tab_expand', tab, B, S, T, start, num_classes, P, st, co, device=dev)
    return st, co


def tablature_to_stacked_multi_pitch(tablature, profile):
    """(..., S, T) classes per string and frame, -1 = silent -> (..., S, P, T) one-hot pitch maps over the profile's whole range
    (amt_tools/tools/utils.py:1988-2059).  ndarray -> float64 ndarray, tensor -> tensor of the tablature's dtype, as in the reference;
    an int64 CUDA tablature (what TabCNN's engine returns) goes through the HIP kernel and comes back as fp32."""
    dof_start, _, P = _tab_geometry(profile)
    if torch is not None and isinstance(tablature, torch.Tensor):
        if tablature.is_cuda and tablature.dtype == torch.int64:
            return tab_expand(tablature, profile, stacked=True)[0]
        start = torch.as_tensor(dof_start, device=tablature.device).unsqueeze(-1)
        rows = torch.where(tablature >= 0, tablature.long() + start, torch.full_like(tablature, -1, dtype=torch.int64))
        hit = rows.unsqueeze(-2) == torch.arange(P, device=tablature.device).unsqueeze(-1)
        return hit.to(tablature.dtype)
    tablature = np.asarray(tablature)
    rows = np.where(tablature >= 0, tablature.astype(np.int64) + dof_start[:, None], -1)
    return (rows[..., None, :] == np.arange(P)[:, None]).astype(np.float64)


def stacked_multi_pitch_to_multi_pitch(stacked_multi_pitch):
    """(..., S, P, T) -> (..., P, T): the maximum over the strings (amt_tools/tools/utils.py:1787-1815)."""
    if torch is not None and isinstance(stacked_multi_pitch, torch.Tensor):
        return torch.max(stacked_multi_pitch, dim=-3)[0]
    return np.max(stacked_multi_pitch, axis=-3)


def notes_to_stacked_notes(pitches, intervals, key=0):
    """{key: (pitches (N,), intervals (N, 2))} sorted by onset the reference's way: through an (N, 3) float64 array and NumPy's default
    argsort (amt_tools/tools/utils.py:719-746, sort_notes :2713-2746); no notes -> shapes (0,) and (0, 2)."""
    batched = np.empty([0, 3])
    if len(pitches) > 0:
        batched = np.concatenate((intervals, np.expand_dims(pitches, axis=-1)), axis=-1)
    batched = batched[np.argsort(batched[..., 0])]
    return {key: (batched[..., 2], batched[:, :2])}


def rms_norm(audio):
    """Root-mean-square normalisation (amt_tools/tools/utils.py:2789-2814)."""
    rms = np.sqrt(np.mean(audio ** 2))
    if rms > 0:
        audio = audio / rms
    return audio


def rms_norm_batch(audio):
    """rms_norm for a (B, N) float32 CUDA tensor of clips, on the device (amtx_rms_norm)."""
    from . import _lib
    assert audio.is_cuda and audio.dim() == 2 and audio.dtype == torch.float32
    audio = audio.contiguous()
    B, N = audio.shape
    ws = _lib.alloc_workspace(int(_lib.call('amtx_rms_norm_workspace_bytes', B, N)), audio.device)
    out = torch.empty_like(audio)
    # a one-clip batch may carry any stride in its size-1 dimension (numpy's x[None] has 0): the rows are N apart by definition then
    _lib.call('amtx_rms_norm', audio, N, audio.stride(0) if B > 1 else N, B, out, out.stride(0) if B > 1 else N, ws, ws.numel(), device=audio.device)
    return out


def seed_everything(seed):
    import random
    random.seed(seed)
    np.random.seed(seed)
    if torch is not None:
        torch.manual_seed(seed)


def register_safe_globals():
    """amt_tools/train.py:106 resumes with `torch.load(model_path)` of a whole pickled module; torch >= 2.6 defaults to
    weights_only=True there, which rejects any class that is not allow-listed (the reference's own classes fail the same way).
    Call this once before `train(..., resume=True)`: it registers every class a pickled model of this package can contain
    (the package's modules, feature modules and profiles, and the stock torch.nn layers they are built from)."""
    from torch import nn
    from . import features, models
    classes = [getattr(models, n) for n in ('TranscriptionModel', 'OutputLayer', 'LogisticBank', 'SoftmaxGroups', 'AcousticModel',
                                            'LanguageModel', 'OnsetsFrames', 'OnsetsFrames2', 'TabCNN', 'SpectralFrontend')]
    classes += [getattr(features, n) for n in features.__all__]
    classes += [InstrumentProfile, PianoProfile, TablatureProfile, GuitarProfile]
    classes += [nn.Sequential, nn.Conv2d, nn.BatchNorm2d, nn.ReLU, nn.MaxPool2d, nn.Dropout, nn.Linear, nn.LSTM, nn.SyncBatchNorm]
    torch.serialization.add_safe_globals(classes)
    return classes
