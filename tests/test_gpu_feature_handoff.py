"""The entry points a real run_on_batch launches, against the rows of tests/golden/feature_handoff.json (recorded off the GPU on fake tensors:
tests/feature_handoff_trace.py), and its outputs against the same batch pushed through materialize() + the ordinary path.  Everything here
compares this package with itself: assert_array_equal."""
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from amt_tools_amd import _lib, tools                                                   # noqa: E402
from amt_tools_amd.synth import synth_clip, synth_state_dict, synth_tabcnn_state_dict   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
DEV = 'cuda:0'


def _tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _onsets_frames(module, dim_in, in_channels, precision):
    from amt_tools_amd.models import OnsetsFrames
    model = OnsetsFrames(dim_in, tools.PianoProfile(), in_channels, 2, device=DEV, precision=precision)
    model.load_state_dict(_tensors(synth_state_dict(7, dim_in=dim_in, in_channels=in_channels, model_complexity=2)))
    return model, module


def _mel(precision='bf16'):
    """MelSpec dB -> OnsetsFrames, 2 clips of 16 frames."""
    from amt_tools_amd.features import MelSpec
    model, module = _onsets_frames(MelSpec(sample_rate=16000, n_mels=229), 229, 1, precision)
    audio = torch.from_numpy(np.stack([synth_clip(i, num_samples=8000) for i in range(2)])).to(DEV)
    return model, module, audio, 16


def _hcqt(precision):
    """HCQT 6 x 72 -> OnsetsFrames mc 2, 2 clips of 4097 samples = 9 frames: less than one tile of anything."""
    from amt_tools_amd.features import HCQT
    model, module = _onsets_frames(HCQT(sample_rate=22050, hop_length=512, n_bins=72), 72, 6, precision)
    audio = torch.from_numpy(np.stack([synth_clip(20 + i, num_samples=4097) for i in range(2)])).to(DEV)
    return model, module, audio, 9


def _tab_clips():
    """2 PyramidClips of 9 frames -> TabCNN."""
    from amt_tools_amd.features import CQT
    from amt_tools_amd.models import TabCNN
    from amt_tools_amd.tracks import PyramidBank
    module = CQT(sample_rate=22050, hop_length=512, n_bins=192, bins_per_octave=24)
    model = TabCNN(192, tools.GuitarProfile(num_frets=19), 1, 1, device=DEV)
    model.load_state_dict(_tensors(synth_tabcnn_state_dict(5, dim_in=192, in_channels=1, model_complexity=1, num_groups=6, num_classes=21)))
    bank = PyramidBank([synth_clip(3, num_samples=30001), synth_clip(9, num_samples=17001)], module, DEV)
    return model, module, bank.clips([0, 1], [40, 3], 9), 9


# golden row -> (set-up, environment of the call, the launches the issue names for it)
ROWS = {'mel dB': (_mel, {}, ['amtx_spec_power', 'amtx_of_forward_power']),
        'mel dB, AMTX_DEFER_DB_SCALE=0': (_mel, {'AMTX_DEFER_DB_SCALE': '0'}, ['amtx_spec_power', 'amtx_spec_scale', 'amtx_of_forward']),
        'hcqt bf16': (lambda: _hcqt('bf16'), {}, ['amtx_cqt_forward16', 'amtx_of_forward_feats16']),
        'hcqt x3': (lambda: _hcqt('x3'), {}, ['amtx_cqt_forward16_split', 'amtx_of_forward_feats16']),
        'tab, pyramid clips, cqt': (_tab_clips, {}, ['amtx_cqt_clips', 'amtx_tab_forward'])}


@pytest.mark.parametrize('row', list(ROWS))
def test_run_on_batch_launches_the_recorded_entry_points(row, monkeypatch):
    """A real run_on_batch with `_lib.call` wrapped: the names of the launches it makes are those of the golden's row of the same batch kind
    (which are the ones the route table of DESIGN.md 5.15 names), and its outputs are the bits of the same batch's ordinary feature map --
    a deferred form's materialize(), else the module's own process_batch / process_clips -- handed over under KEY_FEATS."""
    import feature_handoff_trace as trace
    from amt_tools_amd.models import PendingFeatures
    from amt_tools_amd.tracks import PyramidClips
    with open(os.path.join(ROOT, 'tests', 'golden', 'feature_handoff.json')) as f:
        golden = json.load(f)
    setup, env, named = ROWS[row]
    want_names = trace.launches(trace.expand(golden)[golden['names'].index(row)][0])
    assert want_names == named
    model, module, audio, frames = setup()
    model.frontend = torch.nn.Sequential(module.frontend())
    model.change_device()
    model.eval()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    names, call = [], _lib.call

    def logged(name, *args, **kw):
        names.append(name)
        return call(name, *args, **kw)

    def outputs(batch):
        with torch.no_grad():
            return {k: v.cpu().numpy() for k, v in model.run_on_batch(batch).items() if torch.is_tensor(v)}
    outputs({tools.KEY_AUDIO: audio})                       # plans, engine and weights exist from here on
    monkeypatch.setattr(_lib, 'call', logged)
    got = outputs({tools.KEY_AUDIO: audio})
    monkeypatch.setattr(_lib, 'call', call)
    assert trace.launches([['call', n] for n in names]) == want_names
    with torch.no_grad():
        model.__dict__['_in_run_on_batch'] = True
        try:
            feats = model.pre_proc({tools.KEY_AUDIO: audio})[tools.KEY_FEATS]
        finally:
            model.__dict__.pop('_in_run_on_batch')
        assert isinstance(feats, PendingFeatures) == (named[-1] in ('amtx_of_forward_power', 'amtx_of_forward_feats16'))
        if isinstance(feats, PendingFeatures):
            plain = feats.materialize().transpose(-1, -2)            # (B, C, F, T), as a batch holds it
        else:
            plain = module.process_clips(audio) if isinstance(audio, PyramidClips) else module.process_batch(audio)
    assert plain.shape[0] == 2 and plain.shape[-1] == frames
    want = outputs({tools.KEY_FEATS: plain})
    assert sorted(got) == sorted(want) and got
    for key in got:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
