"""How a batch's features reach the model (models.feature_route and its callers, the plan owners of features.py: DESIGN.md 5.15) against the
trace recorded before models.py held one route and features.py one plan owner.  CPU only: the models run on fake CUDA tensors
(tests/feature_handoff_trace.py)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

# every error text of the parent's _clips_module, _bank_of and _clips_args, the plan cache's two and _index_of's: each has to be in a row
ERRORS = ('TypeError: a TrackClips batch needs a model whose frontend is exactly one SpectralFrontend over an STFT / MelSpec module',
          'TypeError: a TrackClips batch needs a model whose frontend is exactly one SpectralFrontend; clips of a PyramidBank need one over a CQT / VQT / HCQT / HVQT module',
          'ValueError: the clips live on cuda:1, the model on cuda:0', 'ValueError: the clips live on cuda:0, the model on cpu',
          'ValueError: the clips come from a bank of another module: its track maxima are those of its own plan',
          'ValueError: the clips come from a bank of another module: its pyramids and track maxima are those of its own plan',
          'NotImplementedError: HCQT: the decimation pyramid has no clip form over raw audio (clips of the CQT family come from a tracks.PyramidBank, those of a TrackBank from STFT / MelSpec)',
          'AmtxError: no GPU visible: the spectral front-end has no CPU fallback', 'AmtxError: no GPU visible: the CQT front-end has no CPU fallback',
          'AmtxError: the HIP front-end runs on a GPU, not on cpu')
ENTRY_POINTS = ('amtx_spec_power', 'amtx_spec_scale', 'amtx_spec_power_clips', 'amtx_cqt_forward', 'amtx_cqt_forward16', 'amtx_cqt_forward16_split', 'amtx_cqt_power_clips',
                'amtx_cqt_clips', 'amtx_cqt_clips16', 'amtx_cqt_clips16_split', 'amtx_of_forward', 'amtx_of_forward_power', 'amtx_of_forward_feats16', 'amtx_of_offsets',
                'amtx_tab_forward')


def test_every_batch_reaches_the_model_the_recorded_way():
    """tests/golden/feature_handoff.json was recorded by tests/feature_handoff_trace.py on commit e72ce58, BEFORE the rules moved into one place: per
    case every library call with its arguments (shape, strides, dtype of each tensor, every scalar, the handle, the device), every workspace
    allocation, what pre_proc leaves under KEY_FEATS, what forward and run_on_batch return, what a deferred form materializes to,
    autograd.fallbacks() and the exception's type and text, for
      - OnsetsFrames / OnsetsFrames2 / TabCNN with no front-end, MelSpec / STFT with and without decibels, CQT, HCQT with 6 harmonics, with
        bins that are not dim_in, with harmonics that are not in_channels, two front-ends, foreign modules;
      - audio as a 2-D float32 / float64 tensor on the device or the host, 3-D, 1-D, None, absent, TrackClips and PyramidClips of the module's
        own bank, of an equal plan under another module object, of another plan, on another device index; features beside the audio;
      - train / eval, inside / outside run_on_batch, the model on the host, the engine's fuses_db_scale 0 / 1 and takes_feats16 0 / 1 / 2,
        AMTX_DEFER_DB_SCALE=0, AMTX_CQT_FEATS16=0, with and without labels (want_logits), one clip and two;
      - the plan owners' methods on their own, both layouts, all three transforms, with and without planes, the workspace on first use, when it
        fits, when it is too small and on another device, what pickling drops, and _same_plan with one constructor argument changed at a time.
    Every row has to come back."""
    import feature_handoff_trace as trace
    with open(os.path.join(ROOT, 'tests', 'golden', 'feature_handoff.json')) as f:
        golden = json.load(f)
    names = [n for n, _ in trace.cases()]
    assert golden['cases_sha256'] == trace.cases_sha256() and golden['parent_commit'] == 'e72ce58' and golden['names'] == names and len(names) == 166
    want = trace.expand(golden)
    assert {row[3] for row in want} >= set(ERRORS), set(ERRORS) - {row[3] for row in want}
    called = {e[1] for row in want for e in row[0] if e[0] == 'call'}
    assert called >= set(ENTRY_POINTS), set(ENTRY_POINTS) - called
    got = json.loads(json.dumps(trace.record()))
    assert len(got) == len(want) == len(names)
    wrong = [(n, a, b) for n, a, b in zip(names, got, want) if json.dumps(a) != json.dumps(b)]
    assert not wrong, ('rows (case, got, want)', len(wrong), wrong[:2])
