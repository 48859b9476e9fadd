"""TEST INFRASTRUCTURE: how a batch's features reach the model -- which library entry points the Python side of the front-end and of the
engines calls for which batch, and with which arguments -- recorded on the CPU.

Under torch's FakeTensorMode a model (real parameters on the host, its `device` attribute naming a GPU) is handed batches of fake CUDA
tensors and real tracks.TrackClips / PyramidClips over a minimal stand-in bank (`module`, `audio`, `pyramid`, `table` as fake tensors, a NumPy
`desc`).  The REAL pre_proc, run_on_batch, forward, post_proc, PendingFeatures*.materialize, _OFEngine / _TabEngine.forward / offsets and the
real features.py methods run.  Stubbed are only
  - `_lib.call` (logs the name, every argument and the `device` keyword; answers `*_num_frames` as 1 + N // hop, `*_num_bins`,
    `*_num_harmonics`, `amtx_of_fuses_db_scale`, `amtx_of_takes_feats16` from the case's `hop`, `bins`, `harm`, `fuses`, `takes16`, the
    `*_workspace_bytes` by the formulas of _Lib.WORKSPACE, `*_create` by numbering the handle, everything else 0), `_lib.alloc_workspace`
    (logged; a fake uint8 tensor), `_lib.lib()` and `_lib.current_stream` (placeholders: nothing here reaches them);
  - `_EngineBase.sync_weights` (it copies the weights to the host);
  - `torch.cuda.device` as a null context and `torch.cuda.is_available` answering True to features.py alone (the case's `gpu_visible`; fake tensors
    ask it too and hear the truth): entering the one and the plan cache's "no GPU visible" check need a device.
`*_destroy` calls are not logged: they happen when the garbage collector says so -- possibly after the case, so every handle a case numbered is
set to null when it ends (the library's destroy functions take a null).  A training-mode model is driven through pre_proc alone
(`drive='pre_proc_inside'` sets the `_in_run_on_batch` flag by hand): its forward is the training step, which tests/train_dispatch_trace.py pins.

A row is [events, what run_on_batch / the last step returned as (key, shape, strides, dtype), autograd.fallbacks(), the exception as
'Type: text' or None].  Events, in order: ['call', name, arguments, device], ['alloc_workspace', bytes, device], ['feats', type name, ...]
for what pre_proc leaves under KEY_FEATS, ['forward', outputs], ['materialize', tensor], ['return', op, value] of a plan-owner method run
directly.  A tensor is [shape, strides, dtype]; a handle is its tag ('spec_plan#1'); the address a `*_create` writes to is 'out'.

`python tests/feature_handoff_trace.py OUT.json COMMIT` writes the golden; tests/golden/feature_handoff.json is the record of the commit
before models.py held one route and features.py one plan owner, made by this file, unmodified, with an export of that commit first on
sys.path; tests/test_feature_handoff.py requires every row back from the present code."""
import contextlib
import ctypes as C
import hashlib
import json
import logging
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)          # behind a tree that was named first (recording another commit)

# front-end name -> (class, constructor keywords, what its plan answers: bins, harmonics)
FRONTENDS = {
    'mel': ('MelSpec', dict(n_mels=32), 32, 1),
    'mel_lin': ('MelSpec', dict(n_mels=32, decibels=False), 32, 1),
    'mel_40': ('MelSpec', dict(n_mels=40), 40, 1),
    'stft': ('STFT', dict(n_fft=62), 32, 1),
    'stft_lin': ('STFT', dict(n_fft=62, decibels=False), 32, 1),
    'cqt': ('CQT', dict(n_bins=72), 72, 1),
    'hcqt': ('HCQT', dict(n_bins=72), 72, 6),
    'hcqt_60': ('HCQT', dict(n_bins=60), 60, 6),
    'hcqt_3': ('HCQT', dict(n_bins=72, harmonics=[1, 2, 3]), 72, 3),
}
AUDIO = dict(kind='tensor', shape=[2, 8000], dtype='float32', dev='cuda:0')


def _m(name, fe=('mel',), **kw):
    """A model case.  `fe`: the front-end entries -- a FRONTENDS name (wrapped in a SpectralFrontend), 'foreign' (an nn.Identity) or 'wrapped_foreign' /
    'wrapped_foreign_db' (a SpectralFrontend over a module that owns no plan, without / with `decibels`); the plan's answers are those of the first named one."""
    named = [f for f in fe if f in FRONTENDS]
    bins, harm = FRONTENDS[named[0]][2:] if named else (32, 1)
    c = dict(kind='model', cls='OnsetsFrames', precision='bf16', device='cuda:0', fe=list(fe), dim_in=72 if bins in (60, 72) else 32,
             ic=6 if harm > 1 else 1, audio=AUDIO, feats=None, train=False, drive='run_on_batch', labels=False, env={}, fuses=1, takes16=1,
             hop=512, bins=bins, harm=harm)
    c.update(kw)
    return [name, c]


def _tensor(b=2, n=8000, dtype='float32', dev='cuda:0', shape=None):
    return dict(kind='tensor', shape=shape or [b, n], dtype=dtype, dev=dev)


def _clips(kind, b=2, t=16, dev='cuda:0', bank='own'):
    """bank: 'own' = a bank of the model's module, 'equal' = of another module object of the same plan, or a FRONTENDS name = of that module."""
    return dict(kind=kind, B=b, T=t, dev=dev, bank=bank)


def _o(name, fe, ops, **kw):
    """A plan-owner case: `ops` are run in order on ONE module."""
    return [name, dict(dict(kind='owner', fe=fe, ops=ops, hop=512, bins=FRONTENDS[fe][2], harm=FRONTENDS[fe][3]), **kw)]


H9 = _tensor(2, 4097)           # 9 frames: less than one tile of anything
TRK, PYR = 'track_clips', 'pyramid_clips'


def cases():
    """[[name, settings]]: the one case list."""
    out = []
    # ---- an audio tensor into Onsets & Frames: log-mel / STFT ------------------------------------------------------------------------
    out += [_m('mel dB'), _m('mel dB, one clip', audio=_tensor(1)), _m('mel dB, engine does not fuse the dB scale', fuses=0),
            _m('mel dB, AMTX_DEFER_DB_SCALE=0', env={'AMTX_DEFER_DB_SCALE': '0'}), _m('mel dB, AMTX_CQT_FEATS16=0', env={'AMTX_CQT_FEATS16': '0'}),
            _m('mel decibels=False', fe=['mel_lin']), _m('stft dB', fe=['stft']), _m('stft dB, engine does not fuse', fe=['stft'], fuses=0),
            _m('mel dB, labelled', labels=True), _m('mel dB x3', precision='x3'),
            _m('of2 mel dB', cls='OnsetsFrames2'), _m('of2 mel dB, labelled', cls='OnsetsFrames2', labels=True),
            _m('mel dB, float64 audio', audio=_tensor(dtype='float64')), _m('mel dB, audio on the host', audio=_tensor(dev='cpu')),
            _m('mel dB, float64 audio, engine does not fuse', audio=_tensor(dtype='float64'), fuses=0),
            _m('mel dB, 3-D audio', audio=_tensor(shape=[2, 1, 8000])), _m('mel dB, 1-D audio', audio=_tensor(shape=[8000])),
            _m('mel dB, audio None', audio=dict(kind='none')), _m('mel dB, no audio, features given', audio=None, feats=[2, 1, 32, 16]),
            _m('mel dB, no audio, no features', audio=None), _m('mel dB, features beside audio', feats=[2, 1, 32, 16]),
            _m('mel dB, features beside audio, engine does not fuse', feats=[2, 1, 32, 16], fuses=0),
            _m('mel dB, training', train=True, drive='pre_proc_inside'), _m('mel dB, training, outside', train=True, drive='pre_proc'),
            _m('mel dB, outside run_on_batch', drive='pre_proc+forward'), _m('mel dB, model on the host', device='cpu'),
            _m('mel dB, model on the host, audio on the host', device='cpu', audio=_tensor(dev='cpu')),
            _m('two front-ends', fe=['mel', 'mel']), _m('a foreign module', fe=['foreign']), _m('a foreign module behind mel', fe=['mel', 'foreign']),
            _m('a SpectralFrontend over a foreign module', fe=['wrapped_foreign']),
            _m('a SpectralFrontend over a foreign module with decibels', fe=['wrapped_foreign_db']), _m('no front-end', fe=[]),
            _m('no front-end, features beside audio', fe=[], feats=[2, 1, 32, 16])]
    # ---- an audio tensor into Onsets & Frames: the CQT family -------------------------------------------------------------------------
    hc = dict(fe=['hcqt'], audio=H9)
    out += [_m('hcqt bf16', **hc), _m('hcqt bf16, one clip', fe=['hcqt'], audio=_tensor(1, 4097)), _m('hcqt x3', precision='x3', takes16=2, **hc),
            _m('hcqt, engine takes no feats16', takes16=0, **hc), _m('hcqt, AMTX_CQT_FEATS16=0', env={'AMTX_CQT_FEATS16': '0'}, **hc),
            _m('hcqt, AMTX_DEFER_DB_SCALE=0', env={'AMTX_DEFER_DB_SCALE': '0'}, **hc), _m('hcqt, engine fuses no dB scale', fuses=0, **hc),
            _m('hcqt 60 bins into dim_in 72', fe=['hcqt_60'], audio=H9), _m('hcqt 3 harmonics into 6 channels', fe=['hcqt_3'], audio=H9, ic=6),
            _m('hcqt 60 bins into dim_in 72 x3', fe=['hcqt_60'], audio=H9, precision='x3', takes16=2),
            _m('cqt', fe=['cqt'], audio=H9), _m('cqt x3', fe=['cqt'], audio=H9, precision='x3', takes16=2), _m('hcqt, labelled', labels=True, **hc),
            _m('of2 hcqt x3, labelled', cls='OnsetsFrames2', precision='x3', takes16=2, labels=True, **hc),
            _m('hcqt, float64 audio', fe=['hcqt'], audio=_tensor(2, 4097, 'float64')), _m('hcqt, audio on the host', fe=['hcqt'], audio=_tensor(2, 4097, dev='cpu')),
            _m('hcqt, 3-D audio', fe=['hcqt'], audio=_tensor(shape=[2, 1, 4097])), _m('hcqt, features beside audio', feats=[2, 6, 72, 9], **hc),
            _m('hcqt, training', train=True, drive='pre_proc_inside', **hc), _m('hcqt, outside run_on_batch', drive='pre_proc+forward', **hc),
            _m('hcqt, model on the host', device='cpu', **hc), _m('hcqt behind a foreign module', fe=['foreign', 'hcqt'], audio=H9, ic=6, dim_in=72)]
    # ---- TrackClips --------------------------------------------------------------------------------------------------------------------
    tc = _clips(TRK)
    out += [_m('track clips, mel dB', audio=tc), _m('track clips, mel dB, one clip', audio=_clips(TRK, b=1)),
            _m('track clips, engine does not fuse', audio=tc, fuses=0), _m('track clips, AMTX_DEFER_DB_SCALE=0', audio=tc, env={'AMTX_DEFER_DB_SCALE': '0'}),
            _m('track clips, mel decibels=False', fe=['mel_lin'], audio=tc), _m('track clips, stft dB', fe=['stft'], audio=tc),
            _m('track clips, labelled', audio=tc, labels=True), _m('of2 track clips', cls='OnsetsFrames2', audio=tc),
            _m('track clips of an equal plan', audio=_clips(TRK, bank='equal')), _m('track clips of an equal plan, engine does not fuse', audio=_clips(TRK, bank='equal'), fuses=0),
            _m('track clips of another plan', audio=_clips(TRK, bank='mel_40')), _m('track clips of another plan, engine does not fuse', audio=_clips(TRK, bank='mel_40'), fuses=0),
            _m('track clips of an stft bank into mel', audio=_clips(TRK, bank='stft')),
            _m('track clips on another device', audio=_clips(TRK, dev='cuda:1')), _m('track clips on another device, engine does not fuse', audio=_clips(TRK, dev='cuda:1'), fuses=0),
            _m('track clips, model on the host', audio=tc, device='cpu'), _m('track clips into hcqt', fe=['hcqt'], audio=tc),
            _m('track clips into hcqt on another device', fe=['hcqt'], audio=_clips(TRK, dev='cuda:1')),
            _m('track clips, a foreign module', fe=['foreign'], audio=tc), _m('track clips, a SpectralFrontend over a foreign module', fe=['wrapped_foreign'], audio=tc),
            _m('track clips, two front-ends', fe=['mel', 'mel'], audio=tc), _m('track clips, no front-end', fe=[], audio=tc),
            _m('track clips, training', audio=tc, train=True, drive='pre_proc_inside'), _m('track clips, outside run_on_batch', audio=tc, drive='pre_proc+forward'),
            _m('track clips, features beside them', audio=tc, feats=[2, 1, 32, 16]),
            _m('track clips, features beside them, engine does not fuse', audio=tc, feats=[2, 1, 32, 16], fuses=0)]
    # ---- PyramidClips ------------------------------------------------------------------------------------------------------------------
    pc = _clips(PYR, t=9)
    hp = dict(fe=['hcqt'], audio=pc)
    out += [_m('pyramid clips, hcqt bf16', **hp), _m('pyramid clips, one clip', fe=['hcqt'], audio=_clips(PYR, b=1, t=9)),
            _m('pyramid clips, hcqt x3', precision='x3', takes16=2, **hp), _m('pyramid clips, engine takes no feats16', takes16=0, **hp),
            _m('pyramid clips, AMTX_CQT_FEATS16=0', env={'AMTX_CQT_FEATS16': '0'}, **hp), _m('pyramid clips, AMTX_DEFER_DB_SCALE=0', env={'AMTX_DEFER_DB_SCALE': '0'}, **hp),
            _m('pyramid clips, 60 bins into dim_in 72', fe=['hcqt_60'], audio=pc), _m('pyramid clips, 3 harmonics into 6 channels', fe=['hcqt_3'], audio=pc, ic=6),
            _m('pyramid clips, cqt', fe=['cqt'], audio=pc), _m('pyramid clips, labelled', labels=True, **hp),
            _m('of2 pyramid clips x3', cls='OnsetsFrames2', precision='x3', takes16=2, **hp),
            _m('pyramid clips of an equal plan', fe=['hcqt'], audio=_clips(PYR, t=9, bank='equal')),
            _m('pyramid clips of an equal plan, engine takes no feats16', fe=['hcqt'], audio=_clips(PYR, t=9, bank='equal'), takes16=0),
            _m('pyramid clips of another plan', fe=['hcqt'], audio=_clips(PYR, t=9, bank='hcqt_3')),
            _m('pyramid clips of another plan, engine takes no feats16', fe=['hcqt'], audio=_clips(PYR, t=9, bank='hcqt_3'), takes16=0),
            _m('pyramid clips on another device', fe=['hcqt'], audio=_clips(PYR, t=9, dev='cuda:1')),
            _m('pyramid clips on another device, AMTX_CQT_FEATS16=0', fe=['hcqt'], audio=_clips(PYR, t=9, dev='cuda:1'), env={'AMTX_CQT_FEATS16': '0'}),
            _m('pyramid clips, model on the host', device='cpu', **hp), _m('pyramid clips into mel', audio=pc),
            _m('pyramid clips into mel on another device', audio=_clips(PYR, t=9, dev='cuda:1')),
            _m('pyramid clips, a foreign module', fe=['foreign'], audio=pc), _m('pyramid clips, two front-ends', fe=['hcqt', 'hcqt'], audio=pc),
            _m('pyramid clips, no front-end', fe=[], audio=pc), _m('pyramid clips, training', train=True, drive='pre_proc_inside', **hp),
            _m('pyramid clips, outside run_on_batch', drive='pre_proc+forward', **hp), _m('pyramid clips, features beside them', feats=[2, 6, 72, 9], **hp)]
    # ---- TabCNN: never a deferred form ---------------------------------------------------------------------------------------------------
    tab = dict(cls='TabCNN', precision='x3')
    out += [_m('tab, pyramid clips, cqt', fe=['cqt'], audio=pc, **tab), _m('tab, pyramid clips, hcqt', fe=['hcqt'], audio=pc, **tab),
            _m('tab, cqt', fe=['cqt'], audio=H9, **tab), _m('tab, mel dB', **tab), _m('tab, track clips, mel dB', audio=tc, **tab),
            _m('tab, track clips into cqt', fe=['cqt'], audio=tc, **tab), _m('tab, pyramid clips into mel', audio=pc, **tab),
            _m('tab, pyramid clips on another device', fe=['cqt'], audio=_clips(PYR, t=9, dev='cuda:1'), **tab),
            _m('tab, pyramid clips, model on the host', fe=['cqt'], audio=pc, device='cpu', **tab),
            _m('tab, pyramid clips, labelled', fe=['cqt'], audio=pc, labels=True, **tab), _m('tab, no front-end, features given', fe=[], audio=None, feats=[2, 1, 32, 16], **tab),
            _m('tab, pyramid clips, features beside them', fe=['cqt'], audio=pc, feats=[2, 1, 72, 9], **tab),
            _m('tab, pyramid clips, training', fe=['cqt'], audio=pc, train=True, drive='pre_proc', **tab),
            _m('tab, pyramid clips, the flag of run_on_batch set by hand', fe=['cqt'], audio=pc, drive='pre_proc_inside', **tab),
            _m('tab, mel dB, the flag of run_on_batch set by hand', drive='pre_proc_inside', **tab)]
    # ---- the plan owners' methods on their own -------------------------------------------------------------------------------------------
    a2, a1 = dict(B=2, N=8000), dict(B=1, N=8000)
    for fe in ('mel', 'mel_lin', 'stft', 'stft_lin'):
        out += [_o(fe + ': power_batch, scale_batch in both layouts', fe, [['power_batch', a2], ['scale_batch', dict(B=2, T=16, layout=False)],
                                                                          ['scale_batch', dict(B=2, T=16, layout=True, ref=True)]])]
    out += [_o('mel: process_batch, one clip, a view, another device', 'mel', [['process_batch', dict(a1, layout=True)], ['process_batch', dict(a2, view=True)],
                                                                               ['process_batch', dict(a2, dev='cuda:1')], ['process_batch', a2]]),
            _o('mel: audio that is not float32 / 2-D / on the device', 'mel', [['power_batch', dict(a2, dtype='float64')]]),
            _o('mel: 3-D audio', 'mel', [['power_batch', dict(B=2, N=8000, shape=[2, 1, 8000])]]),
            _o('mel: audio on the host', 'mel', [['power_batch', dict(a2, dev='cpu')]]),
            _o('mel: power_clips, process_clips', 'mel', [['power_clips', dict(B=2, T=16)], ['process_clips', dict(B=1, T=16)],
                                                          ['process_clips', dict(B=2, T=16, layout=True, bank='equal')], ['power_clips', dict(B=2, T=16, dev='cuda:1')]]),
            _o('mel: clips of another plan', 'mel', [['process_clips', dict(B=2, T=16, bank='mel_40')]]),
            _o('mel: pyramid clips', 'mel', [['process_clips', dict(B=2, T=9, clips=PYR, bank='hcqt')]]),
            _o('mel: pickled', 'mel', [['process_batch', a2], ['getstate', {}]]),
            _o('mel: module on the host', 'mel', [['get_plan', {}]], device='cpu'), _o('mel: no GPU visible', 'mel', [['get_plan', {}]], gpu_visible=False),
            _o('hcqt: no GPU visible', 'hcqt', [['get_plan', {}]], gpu_visible=False), _o('mel: module on device 1', 'mel', [['get_plan', {}], ['get_plan', dict(dev='cuda:0')], ['get_plan', {}]], device='cuda:1')]
    for fe in ('hcqt', 'cqt'):
        out += [_o(fe + ': process_batch and the workspace', fe, [['process_batch', dict(B=2, N=4097)], ['process_batch', dict(B=1, N=4097)], ['process_batch', dict(B=4, N=4097)],
                                                                  ['process_batch', dict(B=2, N=4097, dev='cuda:1')], ['process_batch', dict(B=2, N=4097, view=True)]]),
                _o(fe + ': process_batch16 with and without planes', fe, [['process_batch16', dict(B=2, N=4097)], ['process_batch16', dict(B=2, N=4097, split=True)],
                                                                          ['process_batch16', dict(B=1, N=4097, split=True)], ['process_batch16', dict(B=1, N=8000)],
                                                                          ['process_batch16', dict(B=2, N=4097, dev='cuda:1')]]),
                _o(fe + ': the clip methods and the workspace', fe, [['power_clips', dict(B=2, T=9)], ['process_clips', dict(B=2, T=9)], ['process_clips', dict(B=1, T=9, layout=True)],
                                                                     ['process_clips16', dict(B=4, T=9)], ['process_clips16', dict(B=2, T=9, split=True)],
                                                                     ['process_clips16', dict(B=2, T=9, dev='cuda:1')], ['process_clips', dict(B=2, T=9, bank='equal')],
                                                                     ['process_batch', dict(B=2, N=4097)], ['process_clips', dict(B=2, T=9)]])]
    out += [_o('hcqt: decibels=False', 'hcqt', [['process_batch', dict(B=2, N=4097)], ['process_clips', dict(B=2, T=9)], ['process_clips16', dict(B=2, T=9)]], decibels=False),
            _o('hcqt: float64 audio', 'hcqt', [['process_batch', dict(B=2, N=4097, dtype='float64')]]),
            _o('hcqt: float64 audio, feats16', 'hcqt', [['process_batch16', dict(B=2, N=4097, dtype='float64')]]),
            _o('hcqt: audio on the host, feats16', 'hcqt', [['process_batch16', dict(B=2, N=4097, dev='cpu')]]),
            _o('hcqt: 3-D audio', 'hcqt', [['process_batch', dict(B=2, N=4097, shape=[2, 1, 4097])]]),
            _o('hcqt: more than 8 harmonics, feats16', 'hcqt', [['process_batch16', dict(B=2, N=4097)]], harm=9),
            _o('hcqt: more than 8 harmonics, clips16', 'hcqt', [['process_clips16', dict(B=2, T=9)]], harm=9),
            _o('hcqt: track clips', 'hcqt', [['process_clips', dict(B=2, T=16, clips=TRK, bank='mel')]]),
            _o('hcqt: track clips, power_clips', 'hcqt', [['power_clips', dict(B=2, T=16, clips=TRK, bank='mel')]]),
            _o('hcqt: track clips, clips16', 'hcqt', [['process_clips16', dict(B=2, T=16, clips=TRK, bank='mel')]]),
            _o('hcqt: clips of another plan', 'hcqt', [['process_clips', dict(B=2, T=9, bank='hcqt_3')]]),
            _o('hcqt: clips of another plan, power_clips', 'hcqt', [['power_clips', dict(B=2, T=9, bank='hcqt_60')]]),
            _o('hcqt: clips of a cqt bank, clips16', 'hcqt', [['process_clips16', dict(B=2, T=9, bank='cqt')]]),
            _o('hcqt: pickled', 'hcqt', [['process_batch', dict(B=2, N=4097)], ['getstate', {}]]),
            _o('hcqt: module on the host', 'hcqt', [['get_plan', {}]], device='cpu'),
            _o('hcqt: module on device 1', 'hcqt', [['get_plan', {}], ['get_plan', dict(dev='cuda:0')], ['get_plan', {}], ['change_device', dict(dev='cuda:0')], ['get_plan', {}]], device='cuda:1'),
            _o('mel: change_device', 'mel', [['change_device', dict(dev='cuda:1')], ['get_plan', {}]])]
    # ---- the identity of a plan: one changed constructor argument at a time ---------------------------------------------------------------
    spec = dict(sample_rate=16000, hop_length=512, n_mels=32, n_fft=2048, win_length=2048, center=True, htk=False, librosa_version='0.10')
    out += [['same plan: MelSpec', dict(kind='same_plan', cls='MelSpec', kw=spec, others=[['MelSpec', spec]] + [['MelSpec', dict(spec, **{k: v})] for k, v in (
        ('sample_rate', 22050), ('hop_length', 256), ('n_mels', 40), ('n_fft', 1024), ('win_length', 1024), ('center', False), ('htk', True),
        ('librosa_version', '0.9.2'), ('decibels', False), ('device', 'cuda:1'))] + [['STFT', {k: v for k, v in spec.items() if k not in ('n_mels', 'htk')}], ['HCQT', {}]])]]
    stft = {k: v for k, v in spec.items() if k not in ('n_mels', 'htk')}
    out += [['same plan: STFT', dict(kind='same_plan', cls='STFT', kw=stft, others=[['STFT', stft], ['STFT', dict(stft, n_fft=4096, win_length=2048)], ['MelSpec', spec]])]]
    vqt = dict(sample_rate=22050, hop_length=512, fmin=32.7, n_bins=72, bins_per_octave=12, gamma=3.0, librosa_version='0.10')
    out += [['same plan: VQT', dict(kind='same_plan', cls='VQT', kw=vqt, others=[['VQT', vqt]] + [['VQT', dict(vqt, **{k: v})] for k, v in (
        ('sample_rate', 16000), ('hop_length', 256), ('fmin', 65.4), ('n_bins', 60), ('bins_per_octave', 24), ('gamma', 0.0), ('librosa_version', '0.9.2'),
        ('decibels', False), ('device', 'cuda:1'))] + [['HVQT', dict(vqt, harmonics=[1])], ['CQT', {k: v for k, v in vqt.items() if k != 'gamma'}], ['MelSpec', {}]])]]
    hv = dict(vqt, harmonics=[0.5, 1, 2])
    out += [['same plan: HVQT', dict(kind='same_plan', cls='HVQT', kw=hv, others=[['HVQT', hv], ['HVQT', dict(hv, harmonics=[0.5, 1, 3])], ['HVQT', dict(hv, harmonics=[0.5, 1])],
                                                                                  ['HVQT', dict(hv, harmonics=[2, 1, 0.5])], ['HVQT', dict(hv, gamma=0)], ['HCQT', {k: v for k, v in hv.items() if k != 'gamma'}]])]]
    return out


def cases_sha256():
    return hashlib.sha256(json.dumps(cases(), sort_keys=True).encode()).hexdigest()


class _Lib(object):
    """The stubs of amt_tools_amd._lib for one case, and the log."""

    WORKSPACE = {'amtx_cqt_workspace_bytes': lambda b, n: 1024 * b + n, 'amtx_cqt_clips_workspace_bytes': lambda b, t: 512 * b * t,
                 'amtx_of_workspace_bytes': lambda b, t: 4096 * b * t, 'amtx_tab_workspace_bytes': lambda b, t: 64 * b * t}

    def __init__(self, case):
        self.case, self.events, self.tags, self.handles = case, [], {}, []

    def desc(self, v):
        import torch
        if torch.is_tensor(v):
            return [list(v.shape), list(v.stride()), str(v.dtype)]
        if isinstance(v, C.c_void_p):
            return self.tags.get(v.value, 'pointer')
        if isinstance(v, C.Array):
            return [float(x) for x in v]
        if isinstance(v, bytes):
            return v.decode()
        if isinstance(v, (list, tuple)):
            return [self.desc(x) for x in v]
        if type(v).__module__ == 'numpy':
            return ['ndarray', list(v.shape), str(v.dtype)] if getattr(v, 'ndim', 0) else v.item()
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        return 'out' if type(v).__name__ == 'CArgObject' else type(v).__name__

    def call(self, name, *args, device=None):
        if name.endswith('_destroy'):
            return 0
        self.events.append(['call', name, [self.desc(a) for a in args], None if device is None else str(device)])
        c = self.case
        if name.endswith('_create'):
            handle = args[0]._obj
            handle.value = len(self.tags) + 1
            self.handles.append(handle)
            self.tags[handle.value] = '%s#%d' % (name[len('amtx_'):-len('_create')], handle.value)
            return 0
        if name in self.WORKSPACE:
            return self.WORKSPACE[name](int(args[1]), int(args[2]))
        if name.endswith('_num_frames'):
            return 1 + int(args[1]) // c['hop']
        if name.endswith('_num_bins'):
            return c['bins']
        if name.endswith('_num_harmonics'):
            return c['harm']
        if name == 'amtx_of_fuses_db_scale':
            return c['fuses']
        if name == 'amtx_of_takes_feats16':
            return c['takes16']
        return 0

    def alloc_workspace(self, nbytes, device):
        import torch
        self.events.append(['alloc_workspace', int(nbytes), str(device)])
        return torch.empty(int(nbytes), dtype=torch.uint8, device=device)

    @staticmethod
    def lib():
        raise AssertionError('nothing in a case reaches the library itself')

    @staticmethod
    def current_stream(device=None):
        return C.c_void_p(0)


@contextlib.contextmanager
def _patched(obj, **names):
    old = {k: getattr(obj, k) for k in names}
    for k, v in names.items():
        setattr(obj, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(obj, k, v)


def _flat(out, prefix=''):
    import torch
    rows = []
    for k, v in (out.items() if isinstance(out, dict) else []):
        if isinstance(v, dict):
            rows += _flat(v, prefix + str(k) + '.')
        elif torch.is_tensor(v):
            rows.append([prefix + str(k), list(v.shape), list(v.stride()), str(v.dtype)])
    return rows


def _module(name, device='cuda:0', **kw):
    from amt_tools_amd import features
    cls, ctor = FRONTENDS[name][:2]
    return getattr(features, cls)(**_copied(dict(ctor, device=device, **kw)))


class _Bank(object):
    """What the clip paths read of a tracks.TrackBank / PyramidBank."""

    def __init__(self, module, dev):
        import torch
        self.module = module
        self.audio = torch.empty(40000, dtype=torch.float32, device=dev)
        self.pyramid = torch.empty(30000, dtype=torch.float32, device=dev)
        self.table = torch.empty((3, 40), dtype=torch.int64, device=dev)


def _make_clips(spec, own, harm):
    """The real TrackClips / PyramidClips of a case, over a stand-in bank of `own` (the model's module), an equal one or another."""
    import numpy as np
    import torch
    from amt_tools_amd import tracks
    bank, b, t, dev = spec.get('bank', 'own'), spec['B'], spec['T'], spec.get('dev', 'cuda:0')
    if bank == 'own' and own is not None:
        module = own
    elif bank in ('own', 'equal'):
        module = type(own)(**_copied(own._ctor)) if own is not None else _module('mel')
    else:
        module = _module(bank)
    pyramid = spec.get('clips', spec.get('kind')) == PYR
    desc = np.zeros((b, 3 if pyramid else 4), dtype=np.int64)
    desc[:, -1] = t
    db_ref = torch.empty((b, harm) if pyramid else (b,), dtype=torch.float32, device=dev)
    return (tracks.PyramidClips if pyramid else tracks.TrackClips)(_Bank(module, dev), desc, torch.empty(desc.shape, dtype=torch.int64, device=dev), db_ref)


def _own_module(name, **kw):
    m = _module(name, **kw)
    m._ctor = dict(FRONTENDS[name][1], **kw)          # what an equal module is built from
    return m


def _build_model(c):
    """The case's model, on the host; its `device` names the case's device."""
    import torch
    from amt_tools_amd import features, models, tools
    if c['cls'] == 'TabCNN':
        model = models.TabCNN(c['dim_in'], tools.GuitarProfile(num_frets=19), c['ic'], 1, device=c['device'], precision=c['precision'])
    else:
        model = getattr(models, c['cls'])(c['dim_in'], tools.PianoProfile(), c['ic'], 2, device=c['device'], precision=c['precision'])
    entries = []
    for f in c['fe']:
        if f == 'foreign':
            entries.append(torch.nn.Identity())
        elif f in ('wrapped_foreign', 'wrapped_foreign_db'):
            entries.append(models.SpectralFrontend(features.WaveformWrapper(decibels=f.endswith('_db'))))
        else:
            entries.append(_own_module(f, device=c['device']).frontend())
    model.frontend = torch.nn.Sequential(*entries)
    return model.train(c['train'])


def _feats_event(model, feats):
    import torch
    own = [getattr(m, 'module', None) for m in model.frontend]
    if torch.is_tensor(feats):
        return ['feats', 'Tensor', list(feats.shape), list(feats.stride()), str(feats.dtype)]
    ev = ['feats', type(feats).__name__]
    names = {'PendingFeatures': ('power', 'clip_max', 'ref'), 'PendingFeatures16': ('feats16', 'audio')}.get(type(feats).__name__, ())
    for n in names:
        v = getattr(feats, n)
        ev.append([n, [list(v.shape), list(v.stride()), str(v.dtype)] if torch.is_tensor(v) else (None if v is None else type(v).__name__)])
    if names:
        ev.append(['module', type(feats.module).__name__, any(feats.module is m for m in own)])
    return ev


def _run_model(c, model, lib):
    """One model case: the dict its last step returned."""
    import torch
    from amt_tools_amd import models, tools
    module = next((m.module for m in model.frontend if isinstance(m, models.SpectralFrontend) and hasattr(m.module, '_ctor')), None)
    batch = {}
    a = c['audio']
    if a is not None:
        if a['kind'] == 'none':
            batch[tools.KEY_AUDIO] = None
        elif a['kind'] == 'tensor':
            batch[tools.KEY_AUDIO] = torch.empty(tuple(a['shape']), dtype=getattr(torch, a['dtype']), device=a['dev'])
        else:
            batch[tools.KEY_AUDIO] = _make_clips(a, module, c['harm'])
    if c['feats'] is not None:
        batch[tools.KEY_FEATS] = torch.empty(tuple(c['feats']), dtype=torch.float32, device='cuda:0' if c['device'] != 'cpu' else 'cpu')
    if c['labels']:
        n = c['feats'][-1] if a is None else (1 + a['shape'][-1] // c['hop'] if a['kind'] == 'tensor' else a['T'])
        dev = 'cuda:0' if c['device'] != 'cpu' else 'cpu'
        if c['cls'] == 'TabCNN':
            batch[tools.KEY_TABLATURE] = torch.zeros((a['B'], 6, n), dtype=torch.int64, device=dev)
        else:
            k = (a['shape'][0] if a['kind'] == 'tensor' else a['B'], 88, n)
            batch[tools.KEY_MULTIPITCH] = torch.zeros(k, device=dev)
            batch[tools.KEY_ONSETS] = torch.zeros(k, device=dev)
            if c['cls'] == 'OnsetsFrames2':
                batch[tools.KEY_OFFSETS] = torch.zeros(k, device=dev)
    pre_proc, forward = model.pre_proc, model.forward

    def logged_pre_proc(b):
        out = pre_proc(b)
        lib.events.append(_feats_event(model, out[tools.KEY_FEATS]))
        return out

    def logged_forward(feats):
        out = forward(feats)
        lib.events.append(['forward', _flat(out)])
        return out
    model.__dict__['pre_proc'], model.__dict__['forward'] = logged_pre_proc, logged_forward
    with torch.no_grad():
        if c['drive'] == 'run_on_batch':
            out = model.run_on_batch(batch)
        else:
            if c['drive'] == 'pre_proc_inside':
                model.__dict__['_in_run_on_batch'] = True
            out = model.pre_proc(batch)
            if c['drive'] == 'pre_proc+forward':
                out = model(out[tools.KEY_FEATS])
        feats = out.get(tools.KEY_FEATS) if c['drive'].startswith('pre_proc') and isinstance(out, dict) else None
        if isinstance(feats, models.PendingFeatures):          # what the deferred form stands for
            m = feats.materialize()
            lib.events.append(['materialize', list(m.shape), list(m.stride()), str(m.dtype)])
    return out


def _keywords(a):
    return {k: a[v] for k, v in (('model_layout', 'layout'), ('split', 'split')) if v in a}


def _copied(kw):
    return {k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()}          # HVQT sorts the list it is given


def _run_owner(c, lib):
    """One plan-owner case: every op's return value goes into the log."""
    import torch
    kw = {k: c[k] for k in ('device', 'decibels') if k in c}
    module = _own_module(c['fe'], **kw)
    for op, a in c['ops']:
        dev = a.get('dev', 'cuda:0')
        if op in ('power_batch', 'process_batch', 'process_batch16'):
            shape = tuple(a.get('shape', (a['B'], a['N'])))
            audio = torch.empty(shape, dtype=getattr(torch, a.get('dtype', 'float32')), device=dev)
            if a.get('view'):
                audio = torch.empty((a['B'], a['N'] + 24), dtype=torch.float32, device=dev)[:, 8:8 + a['N']]
            got = getattr(module, op)(audio, **_keywords(a))
        elif op == 'scale_batch':
            vec = lambda: torch.empty((a['B'],), dtype=torch.float32, device=dev)      # noqa: E731
            got = module.scale_batch(torch.empty((a['B'], a['T'], c['bins']), dtype=torch.float32, device=dev), vec(), vec() if a.get('ref') else None,
                                     model_layout=a['layout'])
        elif op in ('power_clips', 'process_clips', 'process_clips16'):
            clips = _make_clips(dict(a, kind=a.get('clips', TRK if c['fe'] in ('mel', 'mel_lin', 'stft', 'stft_lin') else PYR)), module, c['harm'])
            got = getattr(module, op)(clips, **_keywords(a))
        elif op == 'getstate':
            module.__dict__['_prof_events'] = []
            module.__dict__.setdefault('_workspace', None)
            got = sorted(k for k in module.__getstate__() if k.startswith('_') and k != '_ctor')
        elif op == 'change_device':
            module.change_device(a['dev'])
            got = [str(module.device)] + [str(m.device) for m in getattr(module, 'modules', [])]
        else:
            assert op == 'get_plan'
            got = module._get_plan(a.get('dev'))
            workspace = module.__dict__.get('_workspace')
            got = [lib.desc(got), sorted(module.__dict__.get('_plans', {})), None if workspace is None else str(workspace.device)]
        lib.events.append(['return', op, lib.desc(got)])


def _run_same_plan(c, lib):
    from amt_tools_amd import features
    mine = getattr(features, c['cls'])(**_copied(c['kw']))
    for i, (cls, kw) in enumerate(c['others']):
        lib.events.append(['same_plan', i, cls, bool(mine._same_plan(getattr(features, cls)(**_copied(kw))))])


def _one(c):
    """(events, outputs, fallbacks(), error) of one case."""
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from amt_tools_amd import _lib, models
    from amt_tools_amd import autograd as ag
    lib = _Lib(c)
    env = dict({'AMTX_DEFER_DB_SCALE': None, 'AMTX_CQT_FEATS16': None, 'AMTX_TRAIN_OVERLAP': '0'}, **c.get('env', {}))
    old_env = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    ag.reset_fallbacks()
    outputs, error = [], None
    with contextlib.ExitStack() as stack:
        stack.enter_context(warnings.catch_warnings())
        warnings.simplefilter('ignore')
        model = _build_model(c) if c['kind'] == 'model' else None
        stack.enter_context(_patched(logging.getLogger('torch._subclasses.fake_tensor'), disabled=True))
        stack.enter_context(_patched(_lib, call=lib.call, alloc_workspace=lib.alloc_workspace, lib=lib.lib, current_stream=lib.current_stream))
        stack.enter_context(_patched(models._EngineBase, sync_weights=lambda self, model: None))
        available = torch.cuda.is_available
        stack.enter_context(_patched(torch.cuda, device=lambda device: contextlib.nullcontext(), is_available=lambda: (
            c.get('gpu_visible', True) if sys._getframe(1).f_globals.get('__name__') == 'amt_tools_amd.features' else available())))
        stack.enter_context(FakeTensorMode(allow_non_fake_inputs=True))
        try:
            if c['kind'] == 'model':
                outputs = _flat(_run_model(c, model, lib))
            elif c['kind'] == 'owner':
                _run_owner(c, lib)
            else:
                _run_same_plan(c, lib)
        except Exception as e:      # noqa: BLE001 -- part of the record: the same text has to come back
            error = '%s: %s' % (type(e).__name__, e)
        taken = {k: list(v) for k, v in sorted(ag.fallbacks().items())}
        for handle in lib.handles:
            handle.value = None
    for k, v in old_env.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    ag.reset_fallbacks()
    return [lib.events, outputs, taken, error]


def record():
    """[row per case], in the order of cases()."""
    return [_one(c) for _, c in cases()]


def launches(events):
    """The names of a row's kernel-launching calls, in order: functions that take a stream, without the creation and weight calls."""
    from amt_tools_amd import _lib
    stream = {n for table in _lib.header_signatures().values() for n, (_, s) in table.items() if s}
    return [e[1] for e in events if e[0] == 'call' and e[1] in stream and not e[1].endswith(('_create', '_finalize', '_finalize_device', '_set_tensor_device'))]


def compact(rows, parent_commit):
    """Events and output lines repeat from case to case: they go into one table, a row names them by index."""
    table = {}

    def index(v):
        return table.setdefault(json.dumps(v), len(table))
    out = [[[index(e) for e in events], [index(o) for o in outputs], taken, error] for events, outputs, taken, error in rows]
    return dict(table=[json.loads(k) for k in table], cases_sha256=cases_sha256(), parent_commit=parent_commit, names=[n for n, _ in cases()], rows=out)


def expand(c):
    """The inverse of compact."""
    t = c['table']
    return [[[t[i] for i in events], [t[i] for i in outputs], taken, error] for events, outputs, taken, error in c['rows']]


def write(c, path):
    with open(path, 'w') as f:
        f.write('{"cases_sha256": "%s",\n"parent_commit": "%s",\n"names": %s,\n"table": [\n%s\n],\n"rows": [\n%s\n]}\n' % (
            c['cases_sha256'], c['parent_commit'], json.dumps(c['names']), ',\n'.join(json.dumps(v, separators=(',', ':')) for v in c['table']),
            ',\n'.join(json.dumps(v, separators=(',', ':')) for v in c['rows'])))


if __name__ == '__main__':
    got = compact(json.loads(json.dumps(record())), sys.argv[2])
    assert expand(got) == json.loads(json.dumps(record()))          # the record is a function of the code alone
    write(got, sys.argv[1])
    with open(sys.argv[1]) as fh:
        assert expand(json.load(fh)) == expand(got)
