"""Which backend every layer of a GPU training step takes (amt_tools_amd/autograd.py's rules, DESIGN.md 5.14, and their callers in
models.py) against the trace recorded before autograd.py held one statement of each rule.  CPU only: the models run on fake CUDA tensors
(tests/train_dispatch_trace.py)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SITES = ('LogisticBank.output_layer', 'LogisticBank.get_loss', 'AcousticModel conv', 'AcousticModel BatchNorm+ReLU+MaxPool', 'AcousticModel stage',
         'AcousticModel.fc1', 'LanguageModel', 'BiLSTM input projection', 'TabCNN.train')


def test_training_layers_take_the_recorded_backends():
    """tests/golden/train_dispatch.json was recorded by tests/train_dispatch_trace.py on commit ce1eae5, BEFORE the rules moved into one place:
    per case every autograd.Function call with its arguments (shape, strides, dtype, requires_grad of each tensor, every scalar), every
    note_fallback (site, reason) and stock nn.LSTM call in order, the input-projection decision BiLSTMFunction.forward hands its backward, the
    outputs' shapes, strides and dtypes, fallbacks(), the training_backend() line and the error under AMTX_STRICT_TRAINING=1, for
      - OnsetsFrames / OnsetsFrames2 training forwards with their losses: 1, 3, 4, 6 input channels (and features that need a gradient), 88 and
        87 keys, use_hip_bn / use_hip_autograd off per head, SyncBatchNorm, USE_HIP_DENSE off, fp64, a hidden size the recurrences are not
        built for, the BatchNorm variants, no_grad, detach_heads both ways, weighted / derived / missing / wrongly laid out labels;
      - AcousticModel, LanguageModel (input sizes 4 .. 512, both switch states), LogisticBank.forward and get_loss on their own in eval mode,
        under no_grad and in training mode;
      - TabCNN pre_proc -> forward -> post_proc: model_complexity 1 and 2, 1 / 3 / 8 channels, 126 logits, dim_in 7 / 8 / 192, a contiguous
        copy of the windows, use_hip_train / USE_HIP_DENSE off, fp64, integer / float / misshapen labels, eval mode.
    Every row has to come back."""
    import train_dispatch_trace as trace
    with open(os.path.join(ROOT, 'tests', 'golden', 'train_dispatch.json')) as f:
        golden = json.load(f)
    names = [n for n, _ in trace.cases()]
    assert golden['cases_sha256'] == trace.cases_sha256() and golden['parent_commit'] == 'ce1eae5' and golden['names'] == names and len(names) == 102
    want = trace.expand(golden)
    seen = {e[1] for row in want for e in row[0] if e[0] == 'fallback'}
    assert seen == set(SITES), seen ^ set(SITES)
    got = json.loads(json.dumps(trace.record()))
    assert len(got) == len(want) == len(names)
    wrong = [(n, a, b) for n, a, b in zip(names, got, want) if json.dumps(a) != json.dumps(b)]
    assert not wrong, ('rows (case, got, want)', len(wrong), wrong[:2])
