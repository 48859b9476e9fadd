"""
Host-side mirror of amt-tools' TranscriptionModel plugin API (amt_tools/models/common.py,
amt_tools/models/onsetsframes.py) for the Onsets & Frames hot path.

Same class names, constructor arguments, attributes (`dim_in, profile, in_channels, model_complexity,
frame_width, device, iter, frontend`), methods (`change_device, pre_proc, forward, post_proc,
run_on_batch, model_name`) and -- because the sub-modules keep the reference's attribute names --
the same `state_dict()` keys, so reference checkpoints load and `amt_tools.train.train()` /
`amt_tools.inference.run_offline()` accept these objects unchanged (seam S2).

Execution paths
---------------
* eval mode on a CUDA (ROCm) device  -> the HIP inference engine behind include/amtx.h
  (`amtx_of_forward`): conv1 -> conv3x3+BN+ReLU+pool (MFMA) -> fc1 (MFMA GEMM) -> persistent BiLSTM ->
  LogisticBank heads -> piano roll.  No fallback: a missing extension raises.
* training mode on a GPU (autograd) -> hand-written HIP forward + backward kernels behind autograd.Functions
  (amt_tools_amd/autograd.py, which also decides per layer between them and a recorded ATen fallback: DESIGN.md 5.14).
* CPU devices -> stock torch ops on the same parameters (ATen; the reference's own arithmetic).

`precision` selects the inference engine's dense arithmetic.  `'x3'` (DEFAULT since round 6: split-bf16, three bf16 MFMAs per
product, fp32 accumulate) is the mode whose activations are inside north_star's 1e-4 of the fp32 CPU reference -- it is what a user
who swaps the reference classes for these gets.  `'bf16'` (bf16 MFMA operands, fp32 accumulate) is the throughput mode BASELINE
config 2 names: 2.8x the frames/s, sigmoid outputs within 7e-3, 1.4e-3 of the thresholded piano-roll cells differ (bench.py and
tests/test_gpu_model.py print both) -- opt in with `precision='bf16'`.  `'f16'` exists only in a library built with AMTX_BUILD_F16=1.
"""

import collections
import ctypes as C

import numpy as np
import os

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, tools
from . import autograd, cliploss

__all__ = ['TranscriptionModel', 'OutputLayer', 'LogisticBank', 'AcousticModel', 'LanguageModel', 'OnsetsFrames',
           'SpectralFrontend']


class TranscriptionModel(nn.Module):
    """Generic transcription model (amt_tools/models/common.py:19-199)."""

    def __init__(self, dim_in, profile, in_channels=1, model_complexity=1, frame_width=1, device='cpu'):
        nn.Module.__init__(self)
        self.dim_in = dim_in
        self.profile = profile
        self.in_channels = in_channels
        self.model_complexity = model_complexity
        self.frame_width = frame_width
        self.device = device
        self.iter = 0
        # hook for on-device front-ends (models/common.py:56-57); empty by default
        self.frontend = nn.Sequential()

    # ---- engine management (device handles never enter state_dict / pickles, SURVEY finding F11) ----
    _engine_class = None           # the subclass's _EngineBase
    _transient = ('_engine',)      # __dict__ keys that live only between calls on one device: subclasses extend, __getstate__ drops them
    _engine_stages = False         # the engine's first kernel can stage the features itself: the deferred forms of feature_route exist

    def __getstate__(self):
        state = dict(self.__dict__)
        for key in self._transient:
            state.pop(key, None)
        return state

    def _get_engine(self, device):
        eng = self.__dict__.get('_engine')
        if eng is None or eng.device != device:
            eng = self._engine_class(self, device)
            self.__dict__['_engine'] = eng
        eng.sync_weights(self)
        return eng

    def change_device(self, device=None):
        if device is None:
            device = self.device
        if isinstance(device, int):
            device = torch.device(f'cuda:{device}' if torch.cuda.is_available() else 'cpu')
        self.device = device
        self.to(self.device)
        if torch.device(self.device).type == 'cuda':
            # the training path's HIP convolutions / BatchNorm passes (amt_tools_amd/autograd.py) work on channels-last maps; keeping the
            # parameters in that memory format too means no layout copies around them.  Values, shapes and state_dict are unchanged
            self.to(memory_format=torch.channels_last)
        # an on-device front-end follows the model (its plans / tables are created per device on first use)
        for m in self.frontend:
            mod = getattr(m, 'module', None)
            if mod is not None and hasattr(mod, 'change_device'):
                mod.change_device(self.device)

    def pre_proc(self, batch):
        """To-device copy (the caller's dict is not modified) + optional front-end on the raw audio
        (models/common.py:83-122).  What is staged from the audio, and by which method of the front-end's module, is feature_route's answer
        (DESIGN.md 5.15); a deferred form (PendingFeatures) goes under KEY_FEATS as it is."""
        batch = tools.dict_to_device(batch, self.device)
        audio = tools.unpack_dict(batch, tools.KEY_AUDIO)
        feats = tools.unpack_dict(batch, tools.KEY_FEATS)
        route = self._feature_route(batch, audio)
        if route.source is not None:
            staged = self._stage_features(route, audio)
            feats = staged if feats is None else torch.cat((feats, staged), dim=1)
        batch[tools.KEY_FEATS] = feats
        return batch

    def _feature_route(self, batch, audio):
        """feature_route of this model and batch: the facts are gathered here, the rules are there.  The two switches are read per call."""
        from .tracks import _Clips, PyramidClips
        clips = isinstance(audio, _Clips)
        one = len(self.frontend) == 1 and isinstance(self.frontend[0], SpectralFrontend)
        return feature_route(
            training=self.training, inside=self._engine_stages and bool(self.__dict__.get('_in_run_on_batch')), n_frontends=len(self.frontend),
            module=self.frontend[0].module if one else None, defer_db_scale=os.environ.get('AMTX_DEFER_DB_SCALE', '1') != '0',
            cqt_feats16=os.environ.get('AMTX_CQT_FEATS16', '1') != '0',
            source=None if audio is None else 'audio' if not clips else 'pyramid_clips' if isinstance(audio, PyramidClips) else 'track_clips',
            audio_dims=audio.dim() if torch.is_tensor(audio) else None, has_feats=tools.query_dict(batch, tools.KEY_FEATS), device=self.device,
            clips_device=audio.device if clips else None, dim_in=self.dim_in, in_channels=self.in_channels,
            engine=lambda question: getattr(self._get_engine(audio.device), question)())

    def _stage_features(self, route, audio):
        """What `route` makes of `audio`: the (B,C,F,T) feature map, or the PendingFeatures of a deferred form."""
        source, form, module = route
        if (source, form) == ('audio', 'feats'):
            return self.frontend(audio.unsqueeze(-2))       # any nn.Sequential; a SpectralFrontend calls STAGING's process_batch
        stage = getattr(module, STAGING[source, form])
        if form == 'feats':
            # clips cut from device-resident tracks: the slices of the tracks' own feature maps (track-level dB scale)
            return stage(audio, model_layout=True).transpose(-1, -2)
        if source == 'audio':
            audio = audio.float()
        if form == 'power':
            # (clips: their own maximum = the reference = the TRACK's maximum)
            return PendingFeatures(module, *stage(audio))
        return PendingFeatures16(module, stage(audio, split=(form == 'feats16_split')), audio, source=source)

    def forward(self, feats):
        raise NotImplementedError

    def post_proc(self, batch):
        raise NotImplementedError

    # The label keys a per-clip loss needs (tools.KEY_LOSS_FRAMES below), the first one being the key that makes a batch labelled; None:
    # the model has no per-clip loss.
    loss_label_keys = None

    def _take_loss_frames(self, batch):
        """(the batch without tools.KEY_LOSS_FRAMES, whether it carried the key, its value as cliploss takes it).  The key is taken out
        before pre_proc -- a window table is no tensor to move to the model's device and nothing for a front-end -- and put back for
        post_proc.  ValueError for a model without a per-clip loss and in training mode: no gradient goes through the sums."""
        if not tools.query_dict(batch, tools.KEY_LOSS_FRAMES):
            return batch, False, None
        if self.loss_label_keys is None:
            raise ValueError(f'{type(self).__name__} has no per-clip loss: the batch may not carry \'{tools.KEY_LOSS_FRAMES}\'')
        if self.training:
            raise ValueError(f'\'{tools.KEY_LOSS_FRAMES}\' asks for per-clip loss sums, which carry no gradient: eval mode only')
        batch = dict(batch)
        frames = batch.pop(tools.KEY_LOSS_FRAMES)
        if frames is not None and not isinstance(frames, cliploss.Windows):
            frames = np.asarray(frames.detach().cpu() if torch.is_tensor(frames) else frames)
            if frames.dtype.kind == 'f' and np.array_equal(frames, np.rint(frames)):
                frames = frames.astype(np.int64)              # a table that went through a dict_to_dtype(float32) with the audio
        return batch, True, frames

    def run_on_batch(self, batch):
        """pre_proc -> forward -> post_proc.  In eval mode a labelled batch that carries tools.KEY_LOSS_FRAMES -- a (B, 2) integer table
        {first, count} per clip, or None for whole clips -- gets under tools.KEY_LOSS, instead of 0-d batch means, (B,) float64 SUMS per
        loss key: over the named frames of each clip, without the mean over frames (amt_tools_amd/cliploss.py).  sums / count is the
        loss of that clip as a batch of one."""
        batch, per_clip, frames = self._take_loss_frames(batch)
        batch = self.pre_proc(batch)
        if per_clip:
            batch[tools.KEY_LOSS_FRAMES] = frames
        batch[tools.KEY_OUTPUT] = self(batch[tools.KEY_FEATS])
        output = self.post_proc(batch)
        if tools.query_dict(batch, tools.KEY_TIMES):
            output[tools.KEY_TIMES] = batch[tools.KEY_TIMES]
        return output

    @classmethod
    def model_name(cls):
        return cls.__name__


class OutputLayer(nn.Module):
    def __init__(self, dim_in, dim_out, weights=None):
        super().__init__()
        self.dim_in = dim_in
        self.dim_out = dim_out
        self.weights = None
        if weights is not None:
            self.set_weights(np.asarray(weights).flatten())

    def set_weights(self, weights, device='cpu'):
        if isinstance(device, int):
            device = torch.device(f'cuda:{device}' if torch.cuda.is_available() else 'cpu')
        self.weights = torch.Tensor(weights).to(device)


class LogisticBank(OutputLayer):
    """Multi-label logistic output layer (amt_tools/models/common.py:486-620)."""

    def __init__(self, dim_in, dim_out, weights=None):
        super().__init__(dim_in, dim_out, weights)
        self.output_layer = nn.Linear(self.dim_in, self.dim_out)

    def forward(self, feats):
        if feats.is_cuda and torch.is_grad_enabled():     # training on a GPU: the HIP GEMMs, forward and backward
            return autograd.linear_layer('LogisticBank.output_layer', feats, self.output_layer.weight, self.output_layer.bias)
        return self.output_layer(feats)

    def get_loss(self, estimated, reference):
        """BCE with logits; mean over frames, sum over keys, mean over the batch (common.py:541-584).
        estimated (B,T,O) logits, reference (B,O,T)."""
        if autograd.bce_logits_loss_supported(estimated, reference):
            return autograd.bce_logits_loss(estimated, reference, self.weights)     # one HIP pass: loss + d loss / d logits
        if estimated.is_cuda and torch.is_grad_enabled() and estimated.requires_grad:
            # (a validation pass that computes a loss on logits of another dtype / layout is not a training step: nothing to record)
            autograd.note_fallback('LogisticBank.get_loss', f'logits {tuple(estimated.shape)} {estimated.dtype} vs labels {tuple(reference.shape)}')
        est = estimated.transpose(-2, -1)
        weight = self.weights.unsqueeze(-1) if self.weights is not None else None
        loss = F.binary_cross_entropy_with_logits(est.float(), reference.float(), weight=weight, reduction='none')
        return loss.mean(dim=-1).sum(dim=-1).mean()

    def get_loss_sums(self, estimated, reference, frames=None):
        """get_loss without its means: (B,) float64, per clip the sum over keys and over the frames `frames` names (cliploss.bce_sums)."""
        return cliploss.bce_sums(estimated, reference, self.weights, frames)

    def finalize_output(self, raw_output, threshold=None):
        """sigmoid -> (B,O,T) -> optional threshold (common.py:586-620)."""
        final = torch.sigmoid(raw_output.clone().detach()).transpose(-2, -1)
        if threshold is not None:
            final = tools.threshold_activations(final.contiguous(), threshold)
        return final


class AcousticModel(nn.Module):
    """Kelz-style acoustic model (amt_tools/models/onsetsframes.py:330-463); module layout kept for
    state_dict compatibility: layer{1,2,3}.0 = Conv2d, .1 = BatchNorm2d, fc1.0 = Linear."""

    def __init__(self, dim_in, dim_out, in_channels=1, model_complexity=2):
        super().__init__()
        nf1 = nf2 = 16 * model_complexity
        nf3 = 32 * model_complexity
        self.layer1 = nn.Sequential(nn.Conv2d(in_channels, nf1, (3, 3), padding=1), nn.BatchNorm2d(nf1), nn.ReLU())
        self.layer2 = nn.Sequential(nn.Conv2d(nf1, nf2, (3, 3), padding=1), nn.BatchNorm2d(nf2), nn.ReLU(),
                                    nn.MaxPool2d((1, 2)), nn.Dropout(0.25))
        self.layer3 = nn.Sequential(nn.Conv2d(nf2, nf3, (3, 3), padding=1), nn.BatchNorm2d(nf3), nn.ReLU(),
                                    nn.MaxPool2d((1, 2)), nn.Dropout(0.25))
        self.fc1 = nn.Sequential(nn.Linear(nf3 * (dim_in // 4), dim_out), nn.Dropout(0.50))

    use_hip_bn = True        # False: stock nn.BatchNorm2d / ReLU / MaxPool2d (ATen + MIOpen) also on the GPU in training mode

    def _stage(self, layer, x):
        """One conv stage.  Training on a GPU: the convolution is an implicit GEMM on the HIP kernels (autograd.conv3x3: forward,
        input and weight gradients), BatchNorm (batch statistics) + ReLU (+ MaxPool) run as the HIP passes of
        amt_tools_amd/autograd.py (bn_relu_pool); the Dropout behind them is the module's own.  Which side each step takes: DESIGN.md 5.14."""
        if not (self.training and x.is_cuda):
            return layer(x)
        mods = list(layer)
        conv, bn = mods[0], mods[1]
        if not self.use_hip_bn or isinstance(bn, nn.SyncBatchNorm):
            autograd.note_fallback('AcousticModel stage', 'use_hip_bn off' if not self.use_hip_bn else 'SyncBatchNorm (stock modules by design: its statistics are a collective)')
            return layer(x)
        if autograd.conv3x3_supported(x, conv):
            y = autograd.conv3x3(x, conv)
        else:
            autograd.note_fallback('AcousticModel conv', f'Conv2d {conv.in_channels} -> {conv.out_channels} on {x.dtype}')
            y = conv(x)
        done = 1                                   # modules of the stage that have run
        if autograd.bn_relu_pool_supported(y, bn):
            pool = len(mods) > 3 and isinstance(mods[3], nn.MaxPool2d)
            y = autograd.bn_relu_pool(y, bn, pool)
            done = 4 if pool else 3
        else:
            autograd.note_fallback('AcousticModel BatchNorm+ReLU+MaxPool', f'{y.shape[1]} channels, {y.dtype}, channels_last={y.is_contiguous(memory_format=torch.channels_last)}')
        for m in mods[done:]:
            y = m(y)
        return y

    def forward(self, in_feats):
        x = self._stage(self.layer3, self._stage(self.layer2, self._stage(self.layer1, in_feats)))
        if (self.training and x.is_cuda and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)
                and not x.is_contiguous()):
            # channels-last map: (B,T,F,C) is a free view, so the reference's (channel, freq) flatten order is applied to fc1's
            # weight columns (7.5 MB, differentiable permute) instead of transposing the activations (73 MB per head and step,
            # forward and backward)
            lin = self.fc1[0]
            B, C, T, F = x.shape
            w = lin.weight.view(lin.out_features, C, F).transpose(1, 2).reshape(lin.out_features, F * C)
            y = autograd.linear_layer('AcousticModel.fc1', x.permute(0, 2, 3, 1).reshape(B, T, F * C), w, lin.bias)
            for m in list(self.fc1)[1:]:
                y = m(y)
            return y
        if self.training and x.is_cuda:
            autograd.note_fallback('AcousticModel.fc1', 'conv map not in channels-last layout')
        x = x.transpose(-3, -2).flatten(-2)
        return self.fc1(x)


class LanguageModel(nn.Module):
    """BiLSTM language model (amt_tools/models/onsetsframes.py:466-575).  The reference processes eval
    inputs in `chunk_len`-frame chunks carrying the state; that is numerically the full-sequence
    result (SURVEY finding F9), which is what this module computes."""

    def __init__(self, dim_in, dim_out, chunk_len=512, bidirectional=True):
        super().__init__()
        self.dim_in = dim_in
        self.dim_out = dim_out
        self.chunk_len = chunk_len
        self.num_directions = int(bidirectional) + 1
        self.hidden_size = self.dim_out // self.num_directions
        self.mlm = nn.LSTM(input_size=self.dim_in, hidden_size=self.hidden_size, batch_first=True, bidirectional=bidirectional)
        self.use_hip_autograd = True      # False: stock nn.LSTM (ATen / MIOpen) also on the GPU

    def forward(self, in_feats):
        # differentiable path on a GPU (training, or eval outside the engine): both directions' recurrence is one persistent HIP
        # kernel forward and one backward (amt_tools_amd/autograd.py) instead of MIOpen's per-time-step LSTM
        if autograd.bilstm_supported(in_feats, self.mlm, self.use_hip_autograd):
            return autograd.bilstm(in_feats, self.mlm)
        if in_feats.is_cuda and torch.is_grad_enabled():
            autograd.note_fallback('LanguageModel', f'nn.LSTM hidden {self.hidden_size} x {self.num_directions} directions, {in_feats.dtype}, '
                                                    f'use_hip_autograd={self.use_hip_autograd}')
        return self.mlm(in_feats)[0]


class SpectralFrontend(nn.Module):
    """`TranscriptionModel.frontend` entry wrapping a GPU FeatureModule: (B,1,N) audio -> (B,C,F,T).
    The tensor is produced in the model's (T,F)-major memory order and returned as a transposed view, so
    the model's own transpose (onsetsframes.py:90) yields contiguous data without a copy."""

    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, audio):
        assert audio.dim() == 3 and audio.shape[1] == 1
        from .features import _SpecPlanOwner
        if isinstance(self.module, _SpecPlanOwner):
            feats = self.module.process_batch(audio[:, 0].float(), model_layout=True)    # (B,1,T,F)
            return feats.transpose(-1, -2)
        return self.module.process_batch(audio[:, 0].float())                            # CQT family: (B,C,F,T)


def _pick_side_stream(device, candidates=6, spins=20, spin_cycles=20000):
    """A side stream that really runs BESIDE the caller's current stream, for the training step's pitch head.  HIP multiplexes a process's
    streams onto GPU_MAX_HW_QUEUES (default 4) hardware queues in creation order, and two streams that land on the same queue execute one
    after the other.  Measured in round 6: as soon as the process holds an RCCL communicator -- whose own streams shift the order -- the
    first `torch.cuda.Stream()` sits on the null stream's queue, and the training step ran its two heads back to back: 11.4 instead of 9.5
    ms (GPU_MAX_HW_QUEUES=8 / 16: 9.5; =1: 11.3; the data-parallel step of BASELINE config 4 is exactly that case).  So the stream is chosen
    by a test: a chain of short one-block spin kernels (torch.cuda._sleep) on the current stream and on the candidate at once takes ~1.4 x
    one chain's time when the two overlap and ~1.9 x when they share a queue (tools/stream_queue_probe.py: the same verdicts as a chain of 40
    small GEMMs per stream; ONE long spin kernel is not a reliable probe against the null stream).  The first candidate below 1.7 x is
    kept; without one (or without _sleep) the first stream created.  Running BOTH heads on tested streams of their own costs 0.45 ms of
    extra cross-stream waits per step (measured 9.9 vs 9.45 ms), so the recurrent heads stay on the caller's stream."""
    import time
    sleep = getattr(torch.cuda, '_sleep', None)
    main = torch.cuda.current_stream(device)
    first = None
    try:
        with torch.cuda.device(device):
            def chains(streams):
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
                for st in streams:
                    with torch.cuda.stream(st):
                        for _ in range(spins):
                            sleep(spin_cycles)
                for st in streams:
                    st.synchronize()
                return time.perf_counter() - t0
            for _ in range(candidates):
                s = torch.cuda.Stream(device=device)
                first = first or s
                if sleep is None:
                    return s
                chains((main, s))                               # first use of the stream (and of the spin kernel)
                one = min(chains((main,)) for _ in range(2))
                if min(chains((main, s)) for _ in range(2)) < 1.7 * one:
                    return s
    except Exception:                                           # noqa: BLE001 -- a probe: any stream is a correct stream
        pass
    return first or torch.cuda.Stream(device=device)


FeatureRoute = collections.namedtuple('FeatureRoute', 'source form module')

# (source, form) -> the method of the front-end's module that stages it.  ('audio', 'feats') is reached through
# `model.frontend` itself, which may hold anything; the 'feats' rows are also what a deferred form materializes through.
STAGING = {('audio', 'feats'): 'process_batch', ('audio', 'power'): 'power_batch',
           ('audio', 'feats16'): 'process_batch16', ('audio', 'feats16_split'): 'process_batch16',
           ('track_clips', 'feats'): 'process_clips', ('track_clips', 'power'): 'power_clips',
           ('pyramid_clips', 'feats'): 'process_clips', ('pyramid_clips', 'feats16'): 'process_clips16', ('pyramid_clips', 'feats16_split'): 'process_clips16'}
# form -> the engine entry point that takes it (_OFEngine.forward)
ENTRY_POINTS = {'feats': 'amtx_of_forward', 'power': 'amtx_of_forward_power', 'feats16': 'amtx_of_forward_feats16', 'feats16_split': 'amtx_of_forward_feats16'}
# form -> the acoustic phase's entry point (_OFEngine.acoustic_rows)
ACOUSTIC_ROWS_ENTRY_POINTS = {'feats': 'amtx_of_acoustic_rows', 'power': 'amtx_of_acoustic_rows_power', 'feats16': 'amtx_of_acoustic_rows_feats16',
                              'feats16_split': 'amtx_of_acoustic_rows_feats16'}
_CLIPS_FAMILY = {'track_clips': 'spec', 'pyramid_clips': 'cqt'}
_CLIPS_NEED = {'track_clips': 'a TrackClips batch needs a model whose frontend is exactly one SpectralFrontend over an STFT / MelSpec module',
               'pyramid_clips': 'a TrackClips batch needs a model whose frontend is exactly one SpectralFrontend; clips of a PyramidBank need '
                                'one over a CQT / VQT / HCQT / HVQT module'}


def feature_route(*, training, inside, n_frontends, module, defer_db_scale, cqt_feats16, source, audio_dims, has_feats, device, clips_device,
                  dim_in, in_channels, engine):
    """How a batch's audio entry becomes the model's features: FeatureRoute(source, form, module).  A pure function of plain facts.
      training, inside       the model's mode; inside run_on_batch or not
      n_frontends, module    len(model.frontend); the module of its ONE SpectralFrontend, or None when it is anything else
      defer_db_scale, cqt_feats16   the switches AMTX_DEFER_DB_SCALE / AMTX_CQT_FEATS16 (False = set to 0)
      source, audio_dims     what the batch holds under KEY_AUDIO: 'audio' (audio_dims: dim() of a tensor, else None) | 'track_clips' |
                             'pyramid_clips' | None
      has_feats              KEY_FEATS is in the batch too
      device, clips_device   the model's device; the device the clips' bank lives on
      dim_in, in_channels    the model's
      engine                 engine('fuses_db_scale') / engine('takes_feats16'): asked only where a deferred form hangs on the answer, so the
                             engine is created exactly there.
    source: what is staged (None: nothing -- no audio, or a tensor and no front-end).  form: 'feats' = the ordinary (B,C,F,T) map;
    'power' = a dB-scaled STFT / MelSpec stops after its power kernel and the engine's first conv scales (PendingFeatures); 'feats16' /
    'feats16_split' = a CQT-family module writes the conv kernel's own staging format, one plane or the two of x3 (PendingFeatures16).
    The deferred forms exist inside run_on_batch in eval mode on a GPU, for audio alone, as a 2-D tensor or as clips of the module's family.
    Clips need the ONE SpectralFrontend over a module of their family, on the device their bank lives on: anything else raises -- clips are
    never silently skipped.  A PyramidClips is checked before the engine is asked, a TrackClips after: which error a wrong batch gets, and
    whether an engine exists by then, is part of the behaviour (tests/golden/feature_handoff.json)."""
    from .features import _SpecPlanOwner, _CqtPlanOwner, _index_of
    family = 'cqt' if isinstance(module, _CqtPlanOwner) else 'spec' if isinstance(module, _SpecPlanOwner) else None
    clips = source in _CLIPS_FAMILY
    on_gpu = torch.device(device).type == 'cuda'

    def check_clips():
        if family != _CLIPS_FAMILY[source]:
            raise TypeError(_CLIPS_NEED[source])
        if not on_gpu or _index_of(device) != clips_device.index:
            raise ValueError(f'the clips live on {clips_device}, the model on {device}')

    form = 'feats'
    if (inside and not training and defer_db_scale and not has_feats and on_gpu
            and (cqt_feats16 if family == 'cqt' else family == 'spec' and getattr(module, 'decibels', False))
            and (family == _CLIPS_FAMILY[source] if clips else audio_dims == 2)):
        if family == 'cqt':
            if clips:
                check_clips()
            planes = engine('takes_feats16')
            # amtx_of_forward_feats16 takes a bare (B,T,F,8) pointer and indexes it with the MODEL's dim_in / in_channels: a front-end of
            # another shape goes through the ordinary path, whose strides and shapes are explicit (and which raises on a mismatch)
            if planes and int(getattr(module, 'n_bins', -1)) == int(dim_in) and int(module.get_num_channels()) == int(in_channels):
                form = 'feats16_split' if planes == 2 else 'feats16'
        elif engine('fuses_db_scale'):
            form = 'power'
    if clips:
        check_clips()
    elif not n_frontends:
        source = None
    return FeatureRoute(source, form, module)


class PendingFeatures(object):
    """What pre_proc puts under KEY_FEATS for a deferred form of feature_route: its `form`, what the engine reads and the FeatureModule
    (`module`) that would finish it.  This class is form 'power' -- the dB scaling of the front-end is deferred into the engine's first conv
    kernel (amtx_of_forward_power): the raw power mel spectrogram (B,T,F), the clips' own maxima (B,) and, optionally, (B,) reference powers
    for the dB scale (track-level reference; None = each clip's own maximum).  `materialize()` is the ordinary feature tensor
    (B,1,T,F), bit-identical to what the conv kernel stages."""

    def __init__(self, module, power, clip_max, ref=None):
        self.module, self.form = module, 'power'
        self.power, self.clip_max, self.ref = power, clip_max, ref

    @property
    def device(self):
        return self.power.device

    def materialize(self):
        return self.module.scale_batch(self.power, self.clip_max, self.ref, model_layout=True)


class PendingFeatures16(PendingFeatures):
    """Forms 'feats16' / 'feats16_split': a CQT-family front-end has written its features in the first conv kernel's own staging format
    (process_batch16 / process_clips16 -> amtx_of_forward_feats16): (B,T,F,8) bfloat16, the harmonics of a position side by side, or the two
    planes (2,B,T,F,8) of the x3 engine.  `audio` is what they were computed from, a tensor or a PyramidClips (`source`); `materialize()` is
    the ordinary fp32 feature tensor as a (B,C,T,F) view, computed from it."""

    def __init__(self, module, feats16, audio, source='audio'):
        self.module, self.form = module, 'feats16_split' if feats16.dim() == 5 else 'feats16'
        self.feats16, self.audio, self.source = feats16, audio, source

    @property
    def device(self):
        return self.feats16.device

    def materialize(self):
        return getattr(self.module, STAGING[self.source, 'feats'])(self.audio).transpose(-1, -2)


class _EngineBase(object):
    """ctypes handle of a native model (ABI functions `<ABI>_create / _set_tensor / _finalize / _destroy`) + its workspace, bound to one device."""

    ABI = None

    def __init__(self, device, *create_args):
        self.device = device
        self.handle = C.c_void_p()
        _lib.call(self.ABI + '_create', C.byref(self.handle), *create_args, device=device)
        self.version = None
        self.workspace = None

    def sync_weights(self, model):
        items = [(k, v) for k, v in model.state_dict().items() if v.dtype.is_floating_point and not k.startswith('frontend.') and v.numel() > 0]
        version = tuple((k, v._version, v.data_ptr()) for k, v in items)
        if version == self.version:
            return
        if self.version is None or not self._resync_on_device(items):
            # ONE device-to-host copy of all parameters and buffers (a copy per tensor is ~60 synchronisations per re-sync); the library
            # packs from host memory
            flat = torch.cat([v.detach().reshape(-1).to(torch.float32) for _, v in items]).cpu().numpy()
            off = 0
            for k, v in items:
                n = v.numel()
                _lib.call(self.ABI + '_set_tensor', self.handle, k.encode(), flat[off:off + n], n)
                off += n
            _lib.call(self.ABI + '_finalize', self.handle, device=self.device)
        self.version = version

    def _resync_on_device(self, items):
        """A later weight version packed without leaving the GPU: True when done, False for the host path."""
        return False

    def _grow_workspace(self, need, device):
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = None
            self.workspace = _lib.alloc_workspace(need, device)

    def __del__(self):
        try:
            _lib.call(self.ABI + '_destroy', self.handle)
        except Exception:
            pass


class _OFEngine(_EngineBase):
    """The Onsets & Frames engine (amtx_of_model)."""

    ABI = 'amtx_of_model'

    def __init__(self, model, device):
        self.n_out = model.profile.get_range_len()
        super().__init__(device, int(model.dim_in), int(model.in_channels), int(model.model_complexity), int(self.n_out),
                         int(model.has_offsets), {'bf16': 0, 'x3': 1, 'f16': 2}[model.precision])
        self.device_sync = os.environ.get('AMTX_HOST_WEIGHT_SYNC') is None     # A/B switch: always pack on the host
        self.device_syncs = 0                            # re-syncs that stayed on the GPU (tests)
        self.model_complexity = int(model.model_complexity)
        self.language_workspace = None                   # the language phase's own (language_rows)

    def _resync_on_device(self, items):
        # A RE-sync (validate() inside train() pays one at every checkpoint) stays on the GPU where the library can pack there: the
        # tensors are handed over as device pointers and folded / packed by kernels -- the same bits as the host path.
        if not (self.device_sync and all(v.is_cuda and v.device == torch.device(self.device) and v.dtype == torch.float32 for _, v in items)):
            return False
        keep = []                                   # channels-last convolution weights (the GPU training layout) go through a dense device copy
        for k, v in items:
            t = v.detach()
            t = t if t.is_contiguous() else t.contiguous()
            keep.append(t)
            _lib.call('amtx_of_model_set_tensor_device', self.handle, k.encode(), t, t.numel())
        with torch.cuda.device(self.device):
            # not through _lib.call: AMTX_ERR_UNSUPPORTED is an answer here ("pack on the host"), every other error is raised below
            rc = _lib.lib().amtx_of_model_finalize_device(self.handle, _lib.current_stream(self.device))
            if keep and rc == 0:
                torch.cuda.current_stream(self.device).synchronize()     # the borrowed copies may go once the pack kernels have read them
        del keep
        if rc == 0:
            self.device_syncs += 1
            return True
        if rc != _lib.ERR_UNSUPPORTED:
            _lib.check(rc, 'amtx_of_model_finalize_device')
        self.device_sync = False                    # this configuration packs on the host
        return False

    def fuses_db_scale(self):
        return bool(_lib.call('amtx_of_fuses_db_scale', self.handle))

    def takes_feats16(self):
        """0: no; 1: (B,T,F,8) 16-bit channels-last features (one-plane engine); 2: the same as two planes (2,B,T,F,8) (x3 engine, round 6)."""
        return int(_lib.call('amtx_of_takes_feats16', self.handle))

    def conv_stack_fused(self, batch, num_frames):
        """True when a forward pass of this shape runs the three convolution layers as one kernel (csrc/convf.hip)."""
        return bool(_lib.call('amtx_of_conv_stack_fused', self.handle, int(batch), int(num_frames)))

    @staticmethod
    def _input(feats):
        """(form, the tensor whose device counts, the leading arguments of the form's entry point, B, T) of (B,C,T,F) fp32 features or a
        PendingFeatures: the form says where B and T are read and which strides go with the pointer."""
        form = feats.form if isinstance(feats, PendingFeatures) else 'feats'
        if form == 'feats':
            B, _, T, _ = feats.shape
            lead = (feats, *feats.stride(), B, T)
        elif form == 'power':
            clip_max, ref, feats = feats.clip_max, feats.ref, feats.power.unsqueeze(1)
            B, _, T, _ = feats.shape
            sb, _, st, sf = feats.stride()
            lead = (feats, sb, st, sf, clip_max, ref, B, T)
        else:
            feats = feats.feats16                           # (B,T,F,8) or two planes (2,B,T,F,8): a bare pointer, shape and device only
            B, T = feats.shape[-4], feats.shape[-3]
            lead = (feats, B, T)
        return form, feats, lead, B, T

    def forward(self, feats, want_logits=True):
        """feats: (B,C,T,F) fp32 CUDA tensor (any strides), or PendingFeatures.  Returns binary maps + raw logits.  The form says which entry
        point runs (ENTRY_POINTS)."""
        form, feats, lead, B, T = self._input(feats)
        self._grow_workspace(_lib.call('amtx_of_workspace_bytes', self.handle, B, T), feats.device)
        n_out = self.n_out
        opts = dict(dtype=torch.float32, device=feats.device)
        onsets = torch.empty((B, n_out, T), **opts)
        multi_pitch = torch.empty((B, n_out, T), **opts)
        lo = torch.empty((B, T, n_out), **opts) if want_logits else None
        lm = torch.empty((B, T, n_out), **opts) if want_logits else None
        lp = torch.empty((B, T, n_out), **opts) if want_logits else None
        ws = self.workspace
        _lib.call(ENTRY_POINTS[form], self.handle, *lead, ws, ws.numel(), onsets, multi_pitch, lo, lm, lp, device=feats.device)
        self._last = (B, T)
        return onsets, multi_pitch, lo, lm, lp

    # ---- the two phases of exact whole-track inference (include/amtx_ofseq.h, inference._exact_tracks) ----
    def rows_e_bytes(self, total_rows):
        return int(_lib.call('amtx_of_rows_e_bytes', self.handle, int(total_rows)))

    def acoustic_rows(self, feats, table, table_dev, total_rows, rows_e, rows_pitch):
        """The acoustic phase on a clip batch (`feats` as for forward): the rows the (B, 3) int64 gather table {src_first, count, dst_row}
        keeps -- `table` on the host, `table_dev` its device copy -- go into the packed buffers rows_e (rows_e_bytes(total_rows) bytes) and
        rows_pitch (total_rows, n_out) float32."""
        form, feats, lead, B, T = self._input(feats)
        table = np.ascontiguousarray(table, dtype=np.int64)
        if table.shape != (B, 3) or tuple(table_dev.shape) != (B, 3) or table_dev.dtype != torch.int64 or not table_dev.is_contiguous():
            raise ValueError(f'one gather row {{src_first, count, dst_row}} per clip, on the host and on the device: ({B}, 3) int64')
        self._grow_workspace(_lib.call('amtx_of_workspace_bytes', self.handle, B, T), feats.device)
        ws = self.workspace
        _lib.call(ACOUSTIC_ROWS_ENTRY_POINTS[form], self.handle, *lead, ws, ws.numel(), table, table_dev, int(total_rows), rows_e, rows_pitch, device=feats.device)

    def language_rows(self, rows_e, rows_pitch, seqs, seqs_dev, total_rows, out, want_logits=False):
        """The language phase on total_rows packed rows holding the whole tracks of the (S, 2) int64 sequence table {row0, len} (`seqs` on the
        host, `seqs_dev` its device copy).  `out`: {key: flat float32 tensor of n_out * total_rows elements} for KEY_ONSETS, KEY_MULTIPITCH and
        (offset head) KEY_OFFSETS -- track t's (n_out, L_t) map lands at element n_out * row0_t.  Returns {key: (total_rows, n_out) logits}
        with want_logits, else {}."""
        seqs = np.ascontiguousarray(seqs, dtype=np.int64)
        R, device = int(total_rows), rows_pitch.device
        need = _lib.call('amtx_of_language_workspace_bytes', self.handle, R)
        if self.language_workspace is None or self.language_workspace.numel() < need:
            self.language_workspace = None
            self.language_workspace = _lib.alloc_workspace(need, device)
        keys = (tools.KEY_ONSETS, tools.KEY_MULTIPITCH, tools.KEY_OFFSETS)
        logits = {k: torch.empty((R, self.n_out), dtype=torch.float32, device=device) for k in keys if want_logits and k in out}
        ws = self.language_workspace
        try:
            _lib.call('amtx_of_language_rows', self.handle, rows_e, rows_pitch, seqs, seqs_dev, len(seqs), R, ws, ws.numel(),
                      *(out.get(k) for k in keys), *(logits.get(k) for k in keys), device=device)
        except _lib.AmtxError as e:
            if f'({_lib.ERR_UNSUPPORTED})' in str(e):
                raise NotImplementedError(f'model_complexity={self.model_complexity}: no packed-sequence recurrence is built for this size and precision ({e})') from e
            raise
        return logits

    def offsets(self, device, want_logits=True):
        """OnsetsFrames2: offset probabilities (B,O,T) [+ raw logits (B,T,O)] of the last forward."""
        B, T = self._last
        opts = dict(dtype=torch.float32, device=device)
        prob = torch.empty((B, self.n_out, T), **opts)
        logits = torch.empty((B, T, self.n_out), **opts) if want_logits else None
        _lib.call('amtx_of_offsets', self.handle, self.workspace, self.workspace.numel(), B, T, prob, logits, device=device)
        return prob, logits


class OnsetsFrames(TranscriptionModel):
    """Onsets & Frames V1 (amt_tools/models/onsetsframes.py:17-196)."""

    has_offsets = False

    def __init__(self, dim_in, profile, in_channels=1, model_complexity=2, detach_heads=False, device='cpu',
                 precision='x3'):
        super().__init__(dim_in, profile, in_channels, model_complexity, 1, device)
        assert precision in ('bf16', 'x3', 'f16')
        self.detach_heads = detach_heads
        self.precision = precision
        self.dim_am = 256 * self.model_complexity
        self.dim_lm = 256 * (self.model_complexity - 1)
        dim_out = self.profile.get_range_len()
        self.onset_head = nn.Sequential(AcousticModel(self.dim_in, self.dim_am, self.in_channels, self.model_complexity),
                                        LanguageModel(self.dim_am, self.dim_lm), LogisticBank(self.dim_lm, dim_out))
        self.pitch_head = nn.Sequential(AcousticModel(self.dim_in, self.dim_am, self.in_channels, self.model_complexity),
                                        LogisticBank(self.dim_am, dim_out))
        self.dim_aj = 2 * dim_out
        self.adjoin = nn.Sequential(LanguageModel(self.dim_aj, self.dim_lm), LogisticBank(self.dim_lm, dim_out))

    _engine_class = _OFEngine
    _engine_stages = True
    loss_label_keys = (tools.KEY_MULTIPITCH, tools.KEY_ONSETS)
    _transient = TranscriptionModel._transient + ('_engine_out', '_engine_offsets', '_side_stream', '_overlap_armed', '_fb_last_forward',
                                                  '_overlap_latched_off')

    def pre_proc(self, batch):
        batch = super().pre_proc(batch)
        if not isinstance(batch[tools.KEY_FEATS], PendingFeatures):
            # frequency <-> time (onsetsframes.py:90); a view, the engine takes strides
            batch[tools.KEY_FEATS] = batch[tools.KEY_FEATS].transpose(-1, -2)
        return batch

    def run_on_batch(self, batch):
        # Without ground truth nothing downstream reads the raw logits (post_proc only thresholds them,
        # onsetsframes.py:186-194, and the engine has done that on the device): they stay in the engine's workspace
        # instead of being copied out into three (B,T,O) tensors.  forward() called on its own always returns logits.
        labelled = any(tools.query_dict(batch, k) for k in (tools.KEY_MULTIPITCH, tools.KEY_ONSETS, tools.KEY_OFFSETS))
        self.__dict__['_logits_wanted'] = labelled
        self.__dict__['_in_run_on_batch'] = True
        try:
            return super().run_on_batch(batch)
        finally:
            self.__dict__.pop('_logits_wanted', None)
            self.__dict__.pop('_in_run_on_batch', None)

    def acoustic_rows_on_batch(self, batch, table, table_dev, total_rows, rows_e, rows_pitch):
        """The engine's acoustic phase (_OFEngine.acoustic_rows) on a batch whose features are staged exactly as run_on_batch stages them in
        eval mode on a GPU (feature_route, deferred forms included).  inference._exact_tracks is the caller."""
        self.__dict__['_in_run_on_batch'] = True
        try:
            feats = self.pre_proc(batch)[tools.KEY_FEATS]
        finally:
            self.__dict__.pop('_in_run_on_batch', None)
        pending = isinstance(feats, PendingFeatures)
        if not pending and feats.dtype != torch.float32:
            feats = feats.float()
        self._get_engine(feats.device).acoustic_rows(feats if pending else feats.detach(), table, table_dev, total_rows, rows_e, rows_pitch)

    def forward(self, feats):
        """feats (B,C,T,F) -> dict of raw logits (B,T,O) under 'onsets' and 'multi_pitch'."""
        pending = isinstance(feats, PendingFeatures)
        if pending and self.training:
            feats, pending = feats.materialize(), False
        if pending or (feats.is_cuda and not self.training):
            eng = self._get_engine(feats.device)
            if not pending and feats.dtype != torch.float32:
                feats = feats.float()
            want = self.__dict__.get('_logits_wanted', True)
            onsets_bin, mp_bin, lo, lm, lp = eng.forward(feats if pending else feats.detach(), want_logits=want)
            if not want:
                # label-free run_on_batch: the entries are the final piano rolls already (post_proc passes them through)
                lo, lm = onsets_bin, mp_bin
            output = {tools.KEY_ONSETS: lo, tools.KEY_MULTIPITCH: lm}
            # piano rolls already thresholded on the device; post_proc picks them up for these logits
            self.__dict__['_engine_out'] = (lo, lm, onsets_bin, mp_bin, lp)
            if self.has_offsets:
                prob, logits = eng.offsets(feats.device, want_logits=want)
                output[tools.KEY_OFFSETS] = logits if want else prob
                self.__dict__['_engine_offsets'] = (output[tools.KEY_OFFSETS], prob)
            return output
        self.__dict__.pop('_engine_out', None)
        self.__dict__.pop('_engine_offsets', None)
        output = dict()
        fb0 = None
        if feats.is_cuda and self.training and torch.is_grad_enabled():
            fb0 = autograd.fallback_total()
        if self._overlap_heads(feats):
            # The detector heads only meet at the refinement stage (onsetsframes.py:118-134): the pitch head runs on a side stream beside the
            # recurrent heads -- acoustic model + a 625-step BiLSTM that keeps 4 of the 256 CUs busy at 8 clips; autograd replays
            # every op's backward on the stream of its forward, so the backward passes overlap the same way (11.0 -> 9.85 ms per step).
            # Tensors that cross streams are handed to the allocator with record_stream.  History: round 1 saw intermittent hangs with two
            # streams while the convolutions / Linear layers still ran on MIOpen / hipBLASLt; with the all-HIP step tools/two_stream_repro.py
            # and tests/test_gpu_rccl.py run thousands of steps clean (HISTORY.md "Measured (round 4)").  AMTX_TRAIN_OVERLAP=0 keeps one stream.
            main = torch.cuda.current_stream(feats.device)
            side = self.__dict__.get('_side_stream')
            if side is None or side.device != feats.device:
                side = _pick_side_stream(feats.device)       # tested to run beside the caller's stream
                self.__dict__['_side_stream'] = side
            side.wait_stream(main)
            feats.record_stream(side)
            with torch.cuda.stream(side):          # issued first, as in the reference (onsetsframes.py:121-124): same Dropout RNG order
                multi_pitch = self.pitch_head(feats)
            onsets, offsets = self._recurrent_heads(feats)
            main.wait_stream(side)
            multi_pitch.record_stream(main)
        else:
            multi_pitch = self.pitch_head(feats)
            onsets, offsets = self._recurrent_heads(feats)
        output[tools.KEY_ONSETS] = onsets
        heads = [onsets]
        if self.has_offsets:
            output[tools.KEY_OFFSETS] = offsets
            heads.append(offsets)
        if self.detach_heads:
            heads = [h.clone().detach() for h in heads]
        joint = torch.cat(heads + [multi_pitch], -1)
        output[tools.KEY_MULTIPITCH] = self.adjoin(joint)
        if fb0 is not None:
            self.__dict__['_fb_last_forward'] = autograd.fallback_total() - fb0    # 0: the next training forward may overlap its heads
            if self.__dict__['_fb_last_forward']:
                self.__dict__['_overlap_latched_off'] = True                   # sticky: see _overlap_heads
        return output

    def _overlap_heads(self, feats):
        """Training on a GPU: pitch head on a side stream beside the recurrent heads, unless AMTX_TRAIN_OVERLAP=0 (or the attribute
        `overlap_heads = False` on the model) -- and only while every dense layer of the step runs on this package's HIP kernels.
        tools/two_stream_repro.py narrowed the round-1 hang down to the vendor libraries: with BOTH MIOpen convolutions and hipBLASLt
        GEMMs in the two heads the side stream stops in the first head's fc1 GEMM within 2 - 90 steps (either library alone, or the
        all-HIP step: thousands of steps clean).  So the first training forward of a model runs on one stream, and the overlap is armed
        only if THIS model's previous training forward recorded no ATen fallback (bracketed with autograd.fallback_total() in forward():
        fallbacks of other models or of a validation pass do not count).  The side stream is picked by a concurrency test
        (_pick_side_stream): a stream that shares a hardware queue with the caller's does not overlap anything."""
        if not (feats.is_cuda and self.training and torch.is_grad_enabled()):
            return False
        if os.environ.get('AMTX_TRAIN_OVERLAP', '1') == '0' or not self.__dict__.get('overlap_heads', True):
            return False
        if not autograd.USE_HIP_DENSE:
            return False
        # Several ranks (round 6): on by default too.  Rounds 4 - 5 kept it off under a real process group "until an 8-GPU soak has run"; what
        # is known since: the round-1 hang needs MIOpen + hipBLASLt kernels on the two streams (none in this step); 300 steps with a one-rank
        # RCCL communicator and both streams run clean and bit-identical (tests/test_gpu_rccl.py); two rank processes with both streams each
        # run on one GPU (tests/test_gpu_multirank.py); and the gradient all-reduce is enqueued only after autograd has joined the side stream
        # back into the main one and the next forward forks only after the optimizer step -- RCCL's kernels never run beside the two-stream
        # phase.  AMTX_TRAIN_OVERLAP=0 is the switch back.
        # THIS model's previous training forward must have run without an ATen fallback (the count is bracketed per forward in forward():
        # other models, or a validation pass, do not switch the overlap off for the rest of the process).  The switch is STICKY per model:
        # one training forward of this model that recorded a fallback (an odd-shaped batch sent a layer to MIOpen / hipBLASLt) latches the
        # overlap off for the life of the object -- a vendor-library kernel under two streams is the hang tools/two_stream_repro.py found,
        # and a batch shape that fell back once can come by again at any step.  The bracket covers forward() only: LogisticBank.get_loss in
        # post_proc is not in it, and needs not be (its ATen branch is elementwise BCE on the main stream, after the streams have joined).
        if self.__dict__.get('_overlap_latched_off', False):
            return False
        if self.__dict__.get('_fb_last_forward', None) != 0:
            return False
        return True

    def _recurrent_heads(self, feats):
        """Onset (and offset) detector heads: (onsets, offsets or None)."""
        if self._grouped_recurrences(feats):
            # the onset and offset heads are independent: their two recurrences run as ONE grouped launch each way
            (am_on, lm_on, lb_on), (am_off, lm_off, lb_off) = self.onset_head, self.offset_head
            l_on, l_off = autograd.bilstm_multi([am_on(feats), am_off(feats)], [lm_on.mlm, lm_off.mlm])
            return lb_on(l_on), lb_off(l_off)
        onsets = self.onset_head(feats)
        offsets = self.offset_head(feats) if self.has_offsets else None
        return onsets, offsets

    def _grouped_recurrences(self, feats):
        """Training on a GPU with an offset head whose LSTM and the onset head's are both on the HIP autograd path."""
        if not (self.has_offsets and self.training):
            return False
        lms = (self.onset_head[1], self.offset_head[1])
        return all(isinstance(lm, LanguageModel) and autograd.bilstm_supported(feats, lm.mlm, lm.use_hip_autograd)
                   for lm in lms) and lms[0].hidden_size == lms[1].hidden_size

    def _loss_dict(self, output, batch):
        """The losses of the raw logits `output` against the ground truth of `batch` (onsetsframes.py:158-184): the label rules post_proc
        and loss_sums share.  With tools.KEY_LOSS_FRAMES in the batch, per-clip sums over a frame window (run_on_batch): get_loss_sums
        for get_loss."""
        onset_layer, pitch_layer = self.onset_head[-1], self.adjoin[-1]
        loss = dict()
        multi_pitch_ref = batch[tools.KEY_MULTIPITCH]
        if tools.KEY_LOSS_FRAMES in batch:
            frames = batch[tools.KEY_LOSS_FRAMES]
            get_loss = lambda layer, est, ref: layer.get_loss_sums(est, ref, frames)
        else:
            get_loss = lambda layer, est, ref: layer.get_loss(est, ref)
        loss[tools.KEY_LOSS_PITCH] = get_loss(pitch_layer, output[tools.KEY_MULTIPITCH], multi_pitch_ref)
        if tools.KEY_ONSETS in batch.keys():
            onsets_ref = batch[tools.KEY_ONSETS]
        else:
            # intended behaviour of onsetsframes.py:176-178 (the reference's NumPy helper fails on tensors)
            onsets_ref = tools.multi_pitch_to_onsets(multi_pitch_ref)
        loss[tools.KEY_LOSS_ONSETS] = get_loss(onset_layer, output[tools.KEY_ONSETS], onsets_ref)
        loss[tools.KEY_LOSS_TOTAL] = loss[tools.KEY_LOSS_PITCH] + loss[tools.KEY_LOSS_ONSETS]
        return loss

    def loss_sums(self, logits, labels, frames):
        """Per-clip loss sums of raw logits {key: (B, T, n_out)} against the label maps `labels` over the frame windows `frames` (what
        tools.KEY_LOSS_FRAMES carries): the get_loss_sums calls post_proc makes, without a forward pass."""
        return self._loss_dict(logits, {**labels, tools.KEY_LOSS_FRAMES: frames})

    def post_proc(self, batch):
        """Losses (when ground truth is present) + final piano rolls (onsetsframes.py:138-196)."""
        output = batch[tools.KEY_OUTPUT]
        onset_layer, pitch_layer = self.onset_head[-1], self.adjoin[-1]
        onsets_est, multi_pitch_est = output[tools.KEY_ONSETS], output[tools.KEY_MULTIPITCH]
        if tools.KEY_MULTIPITCH in batch.keys():
            output[tools.KEY_LOSS] = self._loss_dict(output, batch)
        cached = self.__dict__.pop('_engine_out', None)
        if cached is not None and cached[0] is onsets_est and cached[1] is multi_pitch_est:
            output[tools.KEY_ONSETS], output[tools.KEY_MULTIPITCH] = cached[2], cached[3]
        else:
            output[tools.KEY_ONSETS] = onset_layer.finalize_output(onsets_est, 0.5)
            output[tools.KEY_MULTIPITCH] = pitch_layer.finalize_output(multi_pitch_est, 0.5)
        return output

    def engine_logits(self, feats_bcft):
        """Raw logits of all three LogisticBanks from the HIP engine for features (B,C,F,T) on the GPU:
        dict with 'onsets', 'multi_pitch', 'pitch_head' (B,T,O) -- used by the parity tests."""
        feats = feats_bcft.transpose(-1, -2)
        eng = self._get_engine(feats.device)
        onsets_bin, mp_bin, lo, lm, lp = eng.forward(feats.float())
        return {'onsets': lo, 'multi_pitch': lm, 'pitch_head': lp, 'onsets_bin': onsets_bin, 'multi_pitch_bin': mp_bin}


class OnsetsFrames2(OnsetsFrames):
    """Onsets & Frames V2 (amt_tools/models/onsetsframes.py:199-327): adds an offset detector head whose logits join the
    refinement stage; `offsets` are returned as probabilities.  The HIP engine runs it at the model complexities
    `amtx_of_model_create` is built for (2, and 3 = the reference's default for this class); anything else raises there in eval
    mode on a GPU -- it never falls back."""

    has_offsets = True
    loss_label_keys = OnsetsFrames.loss_label_keys + (tools.KEY_OFFSETS,)

    def __init__(self, dim_in, profile, in_channels=1, model_complexity=3, detach_heads=True, device='cpu', precision='x3'):
        super().__init__(dim_in, profile, in_channels, model_complexity, detach_heads, device, precision)
        dim_out = self.profile.get_range_len()
        self.offset_head = nn.Sequential(AcousticModel(self.dim_in, self.dim_am, self.in_channels, self.model_complexity),
                                         LanguageModel(self.dim_am, self.dim_lm), LogisticBank(self.dim_lm, dim_out))
        self.dim_aj += dim_out
        self.adjoin[0] = LanguageModel(self.dim_aj, self.dim_lm)

    def _loss_dict(self, output, batch):
        loss = super()._loss_dict(output, batch)
        offset_layer, offsets_est = self.offset_head[-1], output[tools.KEY_OFFSETS]
        if tools.KEY_OFFSETS in batch.keys():
            offsets_ref = batch[tools.KEY_OFFSETS]
        else:
            offsets_ref = tools.multi_pitch_to_offsets(batch[tools.KEY_MULTIPITCH])
        if tools.KEY_LOSS_FRAMES in batch:
            offsets_loss = offset_layer.get_loss_sums(offsets_est, offsets_ref, batch[tools.KEY_LOSS_FRAMES])
        else:
            offsets_loss = offset_layer.get_loss(offsets_est, offsets_ref)
        loss[tools.KEY_LOSS_OFFSETS] = offsets_loss
        loss[tools.KEY_LOSS_TOTAL] += offsets_loss
        return loss

    def post_proc(self, batch):
        output = super().post_proc(batch)
        offset_layer = self.offset_head[-1]
        offsets_est = output[tools.KEY_OFFSETS]
        cached = self.__dict__.pop('_engine_offsets', None)
        if cached is not None and cached[0] is offsets_est:
            output[tools.KEY_OFFSETS] = cached[1]
        else:
            output[tools.KEY_OFFSETS] = offset_layer.finalize_output(offsets_est)
        return output

    def engine_logits(self, feats_bcft):
        out = super().engine_logits(feats_bcft)
        prob, logits = self._get_engine(feats_bcft.device).offsets(feats_bcft.device)
        out['offsets'], out['offsets_prob'] = logits, prob
        return out


class SoftmaxGroups(OutputLayer):
    """One categorical distribution per degree of freedom: `num_groups` x `num_classes` logits per frame, the LAST class meaning
    "inactive" (labelled -1 in ground truth and in the final output).  Behaviour contract: amt_tools/models/common.py:305-483."""

    def __init__(self, dim_in, num_groups, num_classes, weights=None):
        self.num_groups = num_groups
        self.num_classes = num_classes
        super().__init__(dim_in, num_groups * num_classes, weights)
        self.output_layer = nn.Linear(self.dim_in, self.dim_out)

    def forward(self, feats):
        return self.output_layer(feats)

    def _grouped(self, logits):
        """(B, T, G*C) -> (B, T, G, C)"""
        return logits.reshape(logits.shape[0], -1, self.num_groups, self.num_classes)

    def get_loss(self, estimated, reference):
        """Negative log-likelihood of the labelled class of every group: summed over groups, averaged over frames, then over the
        batch; optional per-(group, class) weights multiply each term (what F.cross_entropy(weight=..., reduction='none') does).
        estimated (B, T, G*C) logits, reference (B, G, T) class indices with -1 for the inactive class."""
        log_prob = torch.log_softmax(self._grouped(estimated).float(), dim=-1)                 # (B, T, G, C)
        target = reference.transpose(-2, -1).long()                                             # (B, T, G)
        target = torch.where(target < 0, torch.full_like(target, self.num_classes - 1), target)
        nll = -log_prob.gather(-1, target.unsqueeze(-1)).squeeze(-1)                            # (B, T, G)
        if self.weights is not None:
            per_class = self.weights.to(nll.device).reshape(self.num_groups, self.num_classes)
            group_idx = torch.arange(self.num_groups, device=nll.device).expand_as(target)
            nll = nll * per_class[group_idx, target]
        return nll.sum(dim=-1).mean(dim=-1).mean()

    def get_loss_sums(self, estimated, reference, frames=None):
        """get_loss without its means: (B,) float64, per clip the sum over groups and over the frames `frames` names
        (cliploss.softmax_groups_sums)."""
        return cliploss.softmax_groups_sums(estimated, reference, self.num_groups, self.num_classes, self.weights, frames)

    def finalize_output(self, raw_output, last_negative=True):
        """Most likely class per group and frame as (B, G, T) indices; the inactive class becomes -1 when `last_negative`."""
        winners = torch.softmax(self._grouped(raw_output.detach()), dim=-1).argmax(dim=-1)      # (B, T, G)
        if last_negative:
            winners = torch.where(winners == self.num_classes - 1, torch.full_like(winners, -1), winners)
        return winners.transpose(-2, -1)


def tab_window_view(feats, frame_width=9):
    """The shared sequence behind a TabCNN window tensor, or None.  `feats` is (B, T, C, F, W); TabCNN.pre_proc hands over an `unfold`
    view whose T and W strides are equal, so window t's column w is column t + w of ONE sequence of T + W - 1 columns that starts at the
    view's own first element.  Returns dict(offset=<storage offset in elements>, num_windows=T, num_cols=T + W - 1,
    strides=(b, c, f, t)) when that holds and the whole extent lies inside the tensor's storage; None for anything else (a contiguous
    copy of the windows, unequal strides, an as_strided view that reaches past its storage)."""
    if not torch.is_tensor(feats) or feats.dim() != 5 or feats.shape[-1] != frame_width or feats.dtype != torch.float32:
        return None
    B, T, Cc, Fd, W = feats.shape
    sb, st, sc, sf, sw = feats.stride()
    if st != sw or st <= 0 or min(sb, sc, sf) < 0 or min(B, T, Cc, Fd) <= 0:
        return None
    ncols = T + W - 1
    off = feats.storage_offset()
    last = off + (B - 1) * sb + (Cc - 1) * sc + (Fd - 1) * sf + (ncols - 1) * st
    if off < 0 or (last + 1) * feats.element_size() > feats.untyped_storage().nbytes():
        return None
    return dict(offset=off, num_windows=T, num_cols=ncols, strides=(sb, sc, sf, st))


class _TabEngine(_EngineBase):
    """The TabCNN engine (amtx_tab_model)."""

    ABI = 'amtx_tab_model'
    WORKSPACE_CAP = 1 << 30      # bytes: longer inputs run as several calls over independent chunks of windows (and of clips)

    def __init__(self, model, device):
        self.G = int(model.profile.get_num_dofs())
        self.C = int(model.profile.num_pitches + 1)
        super().__init__(device, int(model.dim_in), int(model.in_channels), int(model.model_complexity), self.G, self.C,
                         {'bf16': 0, 'x3': 1}[model.precision])
        self.forwards = 0                               # engine calls made (tests)

    def workspace_bytes(self, batch, num_windows):
        return int(_lib.call('amtx_tab_workspace_bytes', self.handle, int(batch), int(num_windows)))

    def _chunks(self, B, T):
        """[(b0, b1, t0, t1)] covering (B, T) with every chunk's workspace under WORKSPACE_CAP (one window of one clip at the least)."""
        cap = self.WORKSPACE_CAP
        if self.workspace_bytes(B, T) <= cap:
            return [(0, B, 0, T)]
        bc = B
        while bc > 1 and self.workspace_bytes(bc, 1) > cap:
            bc = (bc + 1) // 2
        lo, hi = 1, T                                    # the most windows per call at bc clips
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if self.workspace_bytes(bc, mid) <= cap:
                lo = mid
            else:
                hi = mid - 1
        return [(b0, min(B, b0 + bc), t0, min(T, t0 + lo)) for b0 in range(0, B, bc) for t0 in range(0, T, lo)]

    def forward(self, feats, view):
        """feats: the (B, T, C, F, 9) window view, `view` = tab_window_view(feats).  Returns logits (B, T, G*C) fp32 and tablature
        (B, G, T) int64."""
        B, T = feats.shape[:2]
        sb, sc, sf, st = view['strides']
        G, Cn = self.G, self.C
        logits = torch.empty((B, T, G * Cn), dtype=torch.float32, device=feats.device)
        tab = torch.empty((B, G, T), dtype=torch.int64, device=feats.device)
        chunks = self._chunks(B, T)
        self._grow_workspace(max(self.workspace_bytes(b1 - b0, t1 - t0) for b0, b1, t0, t1 in chunks), feats.device)
        base = feats.data_ptr()                          # element (0, 0, 0, 0, 0): column 0 of clip 0's sequence
        esz = feats.element_size()
        for b0, b1, t0, t1 in chunks:
            whole = len(chunks) == 1
            lg = logits if whole else torch.empty((b1 - b0, t1 - t0, G * Cn), dtype=torch.float32, device=feats.device)
            tb = tab if whole else torch.empty((b1 - b0, G, t1 - t0), dtype=torch.int64, device=feats.device)
            ptr = base + (b0 * sb + t0 * st) * esz               # windows are independent: a chunk starts at its first column
            _lib.call('amtx_tab_forward', self.handle, ptr, sb, sc, sf, st, b1 - b0, t1 - t0, self.workspace, self.workspace.numel(), lg, tb,
                      device=feats.device)
            if not whole:
                logits[b0:b1, t0:t1] = lg
                tab[b0:b1, :, t0:t1] = tb
        self.forwards += 1
        return logits, tab


class TabCNN(TranscriptionModel):
    """TabCNN, BASELINE config 1 (behaviour contract: amt_tools/models/tabcnn.py:17-221).  Module names and indices (`conv.{0,2,4}`,
    `dense.{0,3}`) are the reference's, so its checkpoints load; the 9-frame context windows are built on the model's device with a
    strided `unfold` view instead of the reference's device -> NumPy -> device round trip (tabcnn.py:122-127).

    Execution paths
    * inference on a CUDA (ROCm) device -- eval mode, fp32 input, nothing for autograd to record, model_complexity 1 -- with the window
      view pre_proc makes -> the HIP engine behind include/amtx.h (`amtx_tab_forward`, csrc/tab.hip): the convolutions run once per
      sequence instead of once per window (3.5x less arithmetic at dim_in 192), logits and tablature come out of the same call.
      `precision` 'x3' (default: split-bf16, fp32-class logits) or 'bf16' (the throughput mode).
    * training on a CUDA device with the window view pre_proc makes (`use_hip_train`, on by default) -> the same shared-window
      dataflow with gradients on the kernels of amt_tools_amd/autograd.py (_forward_hip_train).  A CUDA training
      forward that cannot take it (train_unsupported; the rules: DESIGN.md 5.14) is recorded under 'TabCNN.train' and runs stock.
    * everything else (CPU, eval with grad enabled, a contiguous copy of the windows in eval mode) -> stock torch ops, unchanged.  An
      inference call the engine would take but whose configuration it does not build is recorded by autograd.note_fallback."""

    CONTEXT = 9      # frames seen by one prediction (tabcnn.py:40)
    use_hip_train = True   # False: CUDA training forwards take the stock per-window path (MIOpen / hipBLASLt), on the record

    def __init__(self, dim_in, profile, in_channels=1, model_complexity=1, device='cpu', precision='x3'):
        super().__init__(dim_in, profile, in_channels, model_complexity, self.CONTEXT, device)
        assert precision in ('bf16', 'x3')
        self.precision = precision
        self.online = False
        widths = (32 * model_complexity, 64 * model_complexity, 64 * model_complexity)
        layers, c_prev = [], self.in_channels
        for c in widths:
            layers += [nn.Conv2d(c_prev, c, (3, 3)), nn.ReLU()]
            c_prev = c
        self.conv = nn.Sequential(*layers, nn.MaxPool2d((2, 2)), nn.Dropout(0.25))
        # three unpadded 3x3 convolutions shave 6 off both axes, the pooling halves them
        self.conv_embedding_size = widths[-1] * ((self.dim_in - 6) // 2) * ((self.frame_width - 6) // 2)
        self.fc_embedding_size = 128 * model_complexity
        self.dense = nn.Sequential(nn.Linear(self.conv_embedding_size, self.fc_embedding_size), nn.ReLU(), nn.Dropout(0.50),
                                   SoftmaxGroups(self.fc_embedding_size, self.profile.get_num_dofs(), self.profile.num_pitches + 1))

    _engine_class = _TabEngine
    _transient = TranscriptionModel._transient + ('_engine_tab',)
    loss_label_keys = (tools.KEY_TABLATURE,)

    def engine_unsupported(self):
        """Why the HIP engine does not build this configuration, or None when it does."""
        C_ = self.profile.num_pitches + 1
        G = self.profile.get_num_dofs()
        if self.model_complexity != 1:
            return f'model_complexity={self.model_complexity} (1 is built)'
        if not 1 <= self.in_channels <= 8:
            return f'in_channels={self.in_channels} (1 to 8 are built)'
        if not 9 <= self.dim_in <= 2048:
            return f'dim_in={self.dim_in} (9 to 2048 are built)'
        if C_ > 32 or G * C_ > 256:
            return f'num_classes={C_}, num_groups={G} (num_classes <= 32 and num_groups x num_classes <= 256 are built)'
        return None

    def _engine_view(self, feats):
        """The window view's geometry when this forward pass belongs to the HIP engine, else None."""
        if not (torch.is_tensor(feats) and feats.is_cuda and feats.dtype == torch.float32 and not self.training):
            return None
        if torch.is_grad_enabled() and (feats.requires_grad or any(p.requires_grad for p in self.parameters())):
            return None
        view = tab_window_view(feats, self.frame_width)
        if view is None or tuple(feats.shape[2:4]) != (self.in_channels, self.dim_in):
            return None
        why = self.engine_unsupported()
        if why is not None:
            autograd.note_fallback('TabCNN.forward', f'no HIP engine for {why}')
            return None
        return view

    def toggle_online(self):
        self.online = not self.online

    def pre_proc(self, batch):
        """Features (B, C, F, T) -> one context window per frame, (B, T', C, F, W).  Offline: T' = T, the sequence is zero-padded
        by W // 2 frames on both sides; online: no padding (the caller supplies exactly the frames of a window)."""
        batch = super().pre_proc(batch)
        feats = batch[tools.KEY_FEATS]
        W = self.frame_width
        if not self.online:
            feats = F.pad(feats, (W // 2, W // 2))
        elif feats.shape[-1] < W:
            feats = F.pad(feats, ((W - feats.shape[-1]) // 2, W - feats.shape[-1] - (W - feats.shape[-1]) // 2))
        windows = feats.unfold(-1, W, 1)                                  # (B, C, F, T', W) view
        batch[tools.KEY_FEATS] = windows.permute(0, 3, 1, 2, 4)           # (B, T', C, F, W)
        return batch

    def train_unsupported(self, feats):
        """Why a training forward on the CUDA tensor `feats` cannot take the shared-window HIP path, or None when it can."""
        if not self.use_hip_train:
            return 'TabCNN.use_hip_train is off'
        if not autograd.USE_HIP_DENSE:
            return 'autograd.USE_HIP_DENSE is off'
        if feats.dtype != torch.float32:
            return f'{feats.dtype} features'
        if tab_window_view(feats, self.frame_width) is None:
            return 'the windows are not a shared-window view (a contiguous copy?)'
        if tuple(feats.shape[2:4]) != (self.in_channels, self.dim_in):
            return f'feature shape {tuple(feats.shape[2:4])} is not ({self.in_channels}, {self.dim_in})'
        if self.dim_in < 8:
            return f'dim_in={self.dim_in}'
        for i, idx in enumerate((0, 2, 4)):
            if not autograd.tab_conv_supported(self.conv[idx], i > 0 or feats.requires_grad):
                return f'conv.{idx} ({self.conv[idx]})'
        if not isinstance(self.conv[6], nn.MaxPool2d) or self.conv[6].kernel_size not in (2, (2, 2)):
            return 'conv.6 is not MaxPool2d((2, 2))'
        fc, out = self.dense[0], self.dense[-1].output_layer
        # the output layer runs with its rows zero-padded to a multiple of 4 (_forward_hip_train): the rule is asked about that shape, so
        # only its input width can fail it; its dtype has never been looked at (the module is converted as a whole)
        n_out = out.out_features + (-out.out_features) % 4
        if not (autograd.linear_takes(fc.weight.dtype, fc.in_features, fc.out_features) and autograd.linear_takes(fc.weight.dtype, out.in_features, n_out)):
            return f'dense layers {fc.in_features} -> {fc.out_features} -> {out.out_features}'
        return None

    def _forward_hip_train(self, feats):
        """The training forward on shared-window sequences: returns the (B, T, G*C) logits."""
        view = tab_window_view(feats, self.frame_width)
        B, T = feats.shape[:2]
        sb, sc, sf, st = view['strides']
        # the sequence behind the windows, on the kernels' axes: (B, C, cols, F) -- cols as frames, frequency rows as bins
        seq = feats.as_strided((B, self.in_channels, view['num_cols'], self.dim_in), (sb, sc, st, sf), view['offset'])
        y = torch.relu(autograd.tab_conv3x3(seq, self.conv[0]))
        y = torch.relu(autograd.tab_conv3x3(y, self.conv[2]))
        y = autograd.tab_conv3x3(y, self.conv[4])               # conv3's ReLU is in the pool kernel
        x = self.conv[-1](autograd.tab_window_pool(y, T))       # (B*T, C3*H) in the reference's flatten order, then Dropout(0.25)
        fc = self.dense[0]
        x = self.dense[2](torch.relu(autograd.linear(x, fc.weight, fc.bias)))
        head = self.dense[-1].output_layer
        n = head.out_features
        pad = (-n) % 4                                          # G*C = 126 at 6 x 21: zero rows up to a multiple of 4
        w = F.pad(head.weight, (0, 0, 0, pad)) if pad else head.weight
        b = F.pad(head.bias, (0, pad)) if pad else head.bias
        logits = autograd.linear(x, w, b)[:, :n]
        return logits.reshape(B, T, n)

    def forward(self, feats):
        self.__dict__.pop('_engine_tab', None)
        if self.training and torch.is_tensor(feats) and feats.is_cuda:
            why = self.train_unsupported(feats)
            if why is None:
                return {tools.KEY_TABLATURE: self._forward_hip_train(feats)}
            autograd.note_fallback('TabCNN.train', why)
        view = self._engine_view(feats)
        if view is not None:
            logits, tab = self._get_engine(feats.device).forward(feats.detach(), view)
            self.__dict__['_engine_tab'] = (logits, tab)          # post_proc takes the tablature for these logits
            return {tools.KEY_TABLATURE: logits}
        B, T = feats.shape[:2]
        embeddings = self.conv(feats.reshape(B * T, self.in_channels, self.dim_in, self.frame_width))
        return {tools.KEY_TABLATURE: self.dense(embeddings.reshape(B, T, -1))}

    def post_proc(self, batch):
        output = batch[tools.KEY_OUTPUT]
        head = self.dense[-1]
        logits = output[tools.KEY_TABLATURE]
        if tools.KEY_TABLATURE in batch:
            labels = batch[tools.KEY_TABLATURE]
            if tools.KEY_LOSS_FRAMES in batch:
                loss = head.get_loss_sums(logits, labels, batch[tools.KEY_LOSS_FRAMES])      # per-clip sums (run_on_batch)
            elif self.training and self.use_hip_train and autograd.softmax_groups_loss_supported(logits, labels, head.num_groups):
                loss = autograd.softmax_groups_loss(logits, labels, head.num_groups, head.num_classes, head.weights)
            else:
                loss = head.get_loss(logits, labels)
            output[tools.KEY_LOSS] = {tools.KEY_LOSS_TOTAL: loss}
        engine = self.__dict__.pop('_engine_tab', None)
        if engine is not None and engine[0] is logits:
            output[tools.KEY_TABLATURE] = engine[1]
        else:
            output[tools.KEY_TABLATURE] = head.finalize_output(logits)
        return output
