"""The offline drivers off the GPU: validate_batched on a CPU model, and the order in which inference._batched calls its hooks."""
import numpy as np
import torch

from amt_tools_amd import evaluate as ev, tools
from amt_tools_amd.inference import run_offline_batched
from amt_tools_amd.models import OnsetsFrames
from amt_tools_amd.transcribe import multi_pitch_to_notes


def test_batched_driver_calls_its_hooks_one_batch_ahead_and_one_behind():
    """5 clips in batches of 2 through a model that only logs: batch n + 1 is staged before batch n runs, batch n - 1 is finished after
    batch n is enqueued, the last one after the loop.  The sequence is that of the loop run_offline_batched and validate_batched each
    wrote out before they shared this one (read off them: stage, wait, stage the next, run, enqueue / decode, finish the previous)."""
    from amt_tools_amd.inference import _batched
    log = []

    class Model(object):
        device = 'cpu'

        def run_on_batch(self, batch):
            log.append(('run', batch[tools.KEY_FEATS][:, 0, 0, 0].int().tolist()))
            return {'n': len(batch[tools.KEY_FEATS])}

    def stage_extra(idx):
        log.append(('stage_extra', list(idx)))
        return 'extra', list(idx)

    def enqueue(idx, preds, extra):
        log.append(('enqueue', list(idx)))
        assert preds == {'n': len(idx)} and extra in (None, ('extra', list(idx)))      # its own batch's predictions and extra
        return 'pending', list(idx)

    def finish(pending):
        log.append(('finish', pending[1]))

    clips = np.arange(5, dtype=np.float32).reshape(5, 1, 1, 1) * np.ones((1, 1, 3, 4), dtype=np.float32)
    _batched(clips, Model(), 2, 0, 1, enqueue, finish, stage_extra)
    b0, b1, b2 = [0, 1], [2, 3], [4]
    assert log == [('stage_extra', b0), ('stage_extra', b1), ('run', b0), ('enqueue', b0), ('stage_extra', b2), ('run', b1), ('enqueue', b1),
                   ('finish', b0), ('run', b2), ('enqueue', b2), ('finish', b1), ('finish', b2)]
    # a rank's share, not contiguous and without the optional hook: clips 1 and 3; and nothing at all for a rank without clips
    del log[:]
    _batched(clips, Model(), 2, 1, 2, enqueue, finish)
    assert log == [('run', [1, 3]), ('enqueue', [1, 3]), ('finish', [1, 3])]
    del log[:]
    _batched(clips[:1], Model(), 2, 1, 2, enqueue, finish)
    assert log == []


def test_validate_batched_on_a_cpu_model_equals_the_host_evaluators():
    """3 clips in batches of 2 through the model of test_model_cpu's frame-times test (40 bins, complexity 2, on the CPU): the batched
    loop scores what the host evaluators score on run_offline_batched's output, per clip and on average."""
    torch.manual_seed(0)
    model = OnsetsFrames(40, tools.PianoProfile(), 1, 2)
    model.eval()
    T = 12
    rng = np.random.default_rng(0)
    feats = (4 * rng.standard_normal((3, 1, 40, T))).astype(np.float32)
    times = np.arange(T) * 512 / 22050.0
    references = []
    for _ in range(3):
        mp = (rng.random((88, T)) < 0.3).astype(np.float32)
        references.append({tools.KEY_MULTIPITCH: mp, tools.KEY_NOTES: multi_pitch_to_notes(mp, times, 21)})
    make = lambda: ev.ComboEvaluator([ev.MultipitchEvaluator(), ev.NoteEvaluator(), ev.NoteEvaluator(offset_ratio=0.2, results_key='with-offsets')])  # noqa: E731
    out = run_offline_batched(feats, model, times=times, batch_size=2, decode_notes=True)
    assert sorted(out) == [0, 1, 2] and all(len(out[i][tools.KEY_NOTES]) > 0 for i in out)
    want = make()
    for i in range(3):
        want.process_track(out[i], references[i], i)
    combo = make()
    average = ev.validate_batched(feats, references, model, combo, times=times, batch_size=2)
    assert average == want.average_results() and 0 < average[tools.KEY_MULTIPITCH][tools.KEY_F1] < 1
    for got_e, want_e in zip(combo.evaluators, want.evaluators):
        assert list(got_e.results) == list(want_e.results)
        for k in want_e.results:
            assert np.array_equal(np.asarray(got_e.results[k]), np.asarray(want_e.results[k])) and len(got_e.results[k]) == 3, k
