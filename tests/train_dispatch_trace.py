"""TEST INFRASTRUCTURE: which backend every layer of a GPU training step takes, recorded on the CPU.

Under torch's FakeTensorMode, inside `with torch.device('cuda')`, a model whose parameters are fake CUDA tensors (_fake_cuda) runs its
training forward on fake CUDA tensors: `is_cuda`, strides, `is_contiguous(memory_format=...)` and `requires_grad` answer as on a device, and
the stock ATen side (Conv2d, BatchNorm2d, Linear, BCE, log_softmax) runs as shape propagation.  `record()` runs every case of `cases()` that way with
  - `apply` of the seven autograd.Function classes replaced by stubs that log the class and every argument -- a tensor as (shape, strides,
    dtype, requires_grad), anything else as it is -- and return fresh fake tensors of the real Function's shape, dtype and memory format;
  - `autograd.note_fallback` wrapped (logged, then called) and `torch.nn.LSTM.forward` replaced (stock nn.LSTM needs a device);
  - the input-projection decision, which lies beneath BiLSTMFunction.apply: its stub runs the real BiLSTMFunction.forward on the fake
    tensors with `autograd._lib` and `autograd.matmul_f32` answering as placeholders, so the 'BiLSTM input projection' fallbacks land in the
    row where a device run records them, followed by a 'projection' event with what the backward is told (ctx.hip_mm).
A row is [events, outputs as (key, shape, strides, dtype), fallbacks() afterwards, the training_backend() line, the error text of the same
case under AMTX_STRICT_TRAINING=1 or 'none'].  A case whose stock side cannot run on fake tensors ends with an 'error' event.

`python tests/train_dispatch_trace.py OUT.json COMMIT` writes the golden; tests/golden/train_dispatch.json is the record of the commit before
autograd.py held one statement of each rule, made by this file, unmodified, with an export of that commit first on sys.path;
tests/test_train_dispatch.py requires every row back from the present code.  AMTX_TRAIN_OVERLAP=0: no stream is touched."""
import contextlib
import hashlib
import json
import logging
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)          # behind a tree that was named first (recording another commit)

B, T, DIM_IN = 2, 16, 32
FUNCTIONS = ('LinearFunction', 'Conv3x3Function', 'BiLSTMFunction', 'BNReLUPoolFunction', 'BCELogitsLossFunction', 'TabWindowPoolFunction',
             'SoftmaxGroupsLossFunction')


def _of(name, **kw):
    return [name, dict(dict(kind='of', cls='OnsetsFrames', mc=2, ic=1, dim_in=DIM_IN, keys=88, feats_grad=False, dtype='float32', bn_off=[],
                            sync_bn=False, lstm_off=[], dense=True, bn=None, no_grad=False, detach_heads=None, weights=False, labels='all',
                            label_layout='ok'), **kw)]


def _tab(name, **kw):
    return [name, dict(dict(kind='tab', mc=1, ic=1, dim_in=DIM_IN, frets=19, feats_grad=False, dtype='float32', copy=False, hip_train=True,
                            dense=True, labels='int64', train=True), **kw)]


def cases():
    """[[name, settings]]: the one case list."""
    out = [_of('of1'), _of('of2 mc2', cls='OnsetsFrames2'), _of('of2 mc3', cls='OnsetsFrames2', mc=3)]
    out += [_of('of1 in_channels %d' % c, ic=c) for c in (3, 4, 6)]
    out += [_of('of1 in_channels 1, feats need a gradient', feats_grad=True), _of('of1 in_channels 3, feats need a gradient', ic=3, feats_grad=True)]
    out += [_of('of1 87 keys', keys=87), _of('of2 mc3 87 keys', cls='OnsetsFrames2', mc=3, keys=87)]
    out += [_of('of1 use_hip_bn off on the pitch head', bn_off=['pitch_head']),
            _of('of2 mc2 use_hip_bn off on every head', cls='OnsetsFrames2', bn_off=['onset_head', 'pitch_head', 'offset_head']),
            _of('of1 SyncBatchNorm', sync_bn=True)]
    out += [_of('of2 mc2 stock LSTM on ' + ' and '.join(h), cls='OnsetsFrames2', lstm_off=h)
            for h in (['onset_head'], ['offset_head'], ['onset_head', 'offset_head'])]
    out += [_of('of1 stock LSTM on onset_head and adjoin', lstm_off=['onset_head', 'adjoin'])]
    out += [_of('of1 USE_HIP_DENSE off', dense=False), _of('of2 mc2 USE_HIP_DENSE off', cls='OnsetsFrames2', dense=False)]
    out += [_of('of1 fp64', dtype='float64'), _of('of2 mc2 fp64', cls='OnsetsFrames2', dtype='float64')]
    out += [_of('of1 mc6', mc=6), _of('of2 mc6', cls='OnsetsFrames2', mc=6)]
    out += [_of('of1 BatchNorm ' + v, bn=v) for v in ('track_running_stats=False', 'momentum=None', 'affine=False')]
    out += [_of('of1 no_grad', no_grad=True), _of('of2 mc2 no_grad', cls='OnsetsFrames2', no_grad=True)]
    out += [_of('of1 detach_heads', detach_heads=True), _of('of2 mc2 heads attached', cls='OnsetsFrames2', detach_heads=False)]
    out += [_of('of1 weighted loss', weights=True), _of('of1 onsets derived', labels='derived'), _of('of2 mc2 onsets and offsets derived', cls='OnsetsFrames2', labels='derived'),
            _of('of1 labels (B, T, K)', label_layout='wrong'), _of('of1 no labels', labels='none'), _of('of1 dim_in 229, 3 x 40 frames', dim_in=229, B=3, T=40)]
    # sub-modules on their own, outside a training step (the whole model would go to the engine)
    for mode in ('eval', 'no_grad', 'train'):
        out += [['AcousticModel ' + mode, dict(kind='am', mode=mode)], ['LanguageModel ' + mode, dict(kind='lm', mode=mode, I=512, hip=True, dense=True)],
                ['LanguageModel ' + mode + ' stock', dict(kind='lm', mode=mode, I=512, hip=False, dense=True)]]
    out += [['AcousticModel train USE_HIP_DENSE off', dict(kind='am', mode='train', dense=False)]]
    out += [['LanguageModel input size %d, USE_HIP_DENSE %s' % (i, d), dict(kind='lm', mode='train', I=i, hip=True, dense=d)]
            for i in (4, 174, 176, 264, 512) for d in (True, False)]
    out += [['LanguageModel one direction', dict(kind='lm', mode='train', I=512, hip=True, dense=True, bidirectional=False)],
            ['LanguageModel fp64', dict(kind='lm', mode='train', I=512, hip=True, dense=True, dtype='float64')]]
    for mode in ('eval', 'no_grad', 'train'):
        out += [['LogisticBank %s %d -> %d' % (mode, k, n), dict(kind='bank', mode=mode, K=k, N=n)] for k, n in ((256, 88), (256, 87), (174, 88))]
    out += [['LogisticBank train fp64', dict(kind='bank', mode='train', K=256, N=88, dtype='float64')],
            ['LogisticBank train USE_HIP_DENSE off', dict(kind='bank', mode='train', K=256, N=88, dense=False)]]
    for mode in ('no_grad', 'train'):
        out += [['get_loss %s %s' % (mode, v), dict(kind='loss', mode=mode, variant=v)]
                for v in ('plain', 'weighted', 'fp64 logits', 'labels (B, T, K)', 'detached logits', 'fp64 detached logits', 'uint8 labels')]
    out += [_tab('tab'), _tab('tab mc2', mc=2), _tab('tab in_channels 3', ic=3), _tab('tab in_channels 8', ic=8),
            _tab('tab feats need a gradient', feats_grad=True), _tab('tab in_channels 3, feats need a gradient', ic=3, feats_grad=True),
            _tab('tab 6 x 21 classes', frets=20), _tab('tab dim_in 7', dim_in=7), _tab('tab dim_in 8', dim_in=8), _tab('tab dim_in 192', dim_in=192),
            _tab('tab contiguous windows', copy=True), _tab('tab use_hip_train off', hip_train=False), _tab('tab USE_HIP_DENSE off', dense=False),
            _tab('tab fp64', dtype='float64'), _tab('tab float labels', labels='float32'), _tab('tab labels (B, T, G)', labels='wrong'),
            _tab('tab no labels', labels='none'), _tab('tab eval', train=False), _tab('tab 9 frames', T=9)]
    return out


def cases_sha256():
    return hashlib.sha256(json.dumps(cases(), sort_keys=True).encode()).hexdigest()


def _desc(v):
    import torch
    if torch.is_tensor(v):
        return [list(v.shape), list(v.stride()), str(v.dtype), bool(v.requires_grad)]
    return v if v is None or isinstance(v, (bool, int, float, str)) else repr(v)


class _Ctx(object):
    """What BiLSTMFunction.forward asks of its ctx."""

    def __init__(self, args):
        import torch
        self.needs_input_grad = tuple(torch.is_tensor(a) and a.requires_grad for a in args)

    def save_for_backward(self, *tensors):
        self.saved = tensors


class _Lib(object):
    """autograd._lib while the real BiLSTMFunction.forward runs on fake tensors: sizes answer 1, launches nothing."""

    @staticmethod
    def call(name, *args, **kw):
        return 1 if name.endswith('_elems') or name.endswith('_bytes') else None


class _Recorder(object):
    def __init__(self):
        self.events = []

    def fresh(self, shape, dtype, grad, channels_last=False):
        import torch
        y = torch.empty(tuple(shape), dtype=dtype, device='cuda', **(dict(memory_format=torch.channels_last) if channels_last else {}))
        return y.requires_grad_(True) if grad else y

    def stub(self, name, ag):
        import torch

        def apply(*args):
            self.events.append(['apply', name] + [_desc(a) for a in args])
            grad = torch.is_grad_enabled() and any(torch.is_tensor(a) and a.requires_grad for a in args)
            f32 = torch.float32
            if name == 'LinearFunction':
                x, w = args[:2]
                return self.fresh(tuple(x.shape[:-1]) + (w.shape[0],), f32, grad)
            if name == 'Conv3x3Function':
                x, w = args[:2]
                return self.fresh((x.shape[0], w.shape[0], x.shape[2], x.shape[3]), f32, grad, channels_last=True)
            if name == 'BNReLUPoolFunction':
                x, pool = args[0], args[7]
                return self.fresh((x.shape[0], x.shape[1], x.shape[2], x.shape[3] // 2 if pool else x.shape[3]), f32, grad, channels_last=True)
            if name in ('BCELogitsLossFunction', 'SoftmaxGroupsLossFunction'):
                return self.fresh((), f32, grad)
            if name == 'TabWindowPoolFunction':
                y3, t = args
                return self.fresh((y3.shape[0] * int(t), y3.shape[1] * ((y3.shape[3] - 6) // 2)), f32, grad)
            assert name == 'BiLSTMFunction'
            ctx = _Ctx(args)
            with torch.no_grad(), _patched(ag, _lib=_Lib, matmul_f32=lambda a, b, a_trans=False, b_trans=False, bias=None, out=None: out):
                outs = ag.BiLSTMFunction.forward(ctx, *args)
            self.events.append(['projection', [bool(v) for v in ctx.hip_mm]])
            return tuple(self.fresh(o.shape, o.dtype, grad) for o in outs)
        return apply

    def stock_lstm(self):
        import torch

        def forward(lstm, x, hx=None):
            self.events.append(['stock_lstm', _desc(x), lstm.hidden_size, bool(lstm.bidirectional)])
            grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in lstm.parameters()))
            return self.fresh(tuple(x.shape[:-1]) + (lstm.hidden_size * (2 if lstm.bidirectional else 1),), x.dtype, grad), None
        return forward


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
    for k, v in out.items():
        if isinstance(v, dict):
            rows += _flat(v, prefix + str(k) + '.')
        elif torch.is_tensor(v):
            rows.append([prefix + str(k), list(v.shape), list(v.stride()), str(v.dtype)])
    return rows


def _mode(mode):
    import torch
    return torch.no_grad() if mode == 'no_grad' else contextlib.nullcontext()


def _fake_cuda(module):
    """Module.to() cannot swap fake parameters: the module is built on the CPU in the layout change_device() gives it, then every parameter
    and buffer is replaced by a fake CUDA tensor of the same shape, strides, dtype and requires_grad."""
    import torch
    for m in module.modules():
        for k, p in m._parameters.items():
            if p is not None:
                m._parameters[k] = torch.nn.Parameter(torch.empty_strided(p.shape, p.stride(), dtype=p.dtype, device='cuda'), requires_grad=p.requires_grad)
        for k, v in m._buffers.items():
            if v is not None:
                m._buffers[k] = torch.empty_strided(v.shape, v.stride(), dtype=v.dtype, device='cuda')
    return module


def _build(c):
    """The case's module, on the CPU."""
    import torch
    from amt_tools_amd import models, tools
    dtype = getattr(torch, c.get('dtype', 'float32'))
    if c['kind'] == 'of':
        kw = {} if c['detach_heads'] is None else dict(detach_heads=c['detach_heads'])
        model = getattr(models, c['cls'])(c['dim_in'], tools.PianoProfile(high=108 - (88 - c['keys'])), c['ic'], c['mc'], device='cuda:0', **kw)
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d) and c['bn']:
                if c['bn'] == 'track_running_stats=False':
                    m.track_running_stats, m.running_mean, m.running_var, m.num_batches_tracked = False, None, None, None
                elif c['bn'] == 'momentum=None':
                    m.momentum = None
                else:
                    m.affine, m.weight, m.bias = False, None, None
        if c['sync_bn']:
            model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)
        for head in c['bn_off']:
            getattr(model, head)[0].use_hip_bn = False
        for head in c['lstm_off']:
            getattr(model, head)[0 if head == 'adjoin' else 1].use_hip_autograd = False
    elif c['kind'] == 'tab':
        model = models.TabCNN(c['dim_in'], tools.GuitarProfile(num_frets=c['frets']), c['ic'], c['mc'], device='cuda:0')
        model.use_hip_train = c['hip_train']
    elif c['kind'] == 'am':
        model = models.AcousticModel(DIM_IN, 512, 1, 2)
    elif c['kind'] == 'lm':
        model = models.LanguageModel(c['I'], 512 if c.get('bidirectional', True) else 256, bidirectional=c.get('bidirectional', True))
        model.use_hip_autograd = c['hip']
    else:
        model = models.LogisticBank(c.get('K', 256), c.get('N', 88))
    if dtype == torch.float64:
        model.double()
    return model.to(memory_format=torch.channels_last).train(c.get('train', c.get('mode', 'train') == 'train'))


def _run(c, model):
    """The case's forward on fake CUDA tensors: the dict it returns."""
    import torch
    from amt_tools_amd import models, tools
    dtype = getattr(torch, c.get('dtype', 'float32'))
    b, t = c.get('B', B), c.get('T', T)
    _fake_cuda(model)
    if c['kind'] == 'of':
        k = c['keys']
        if c['weights']:
            for m in model.modules():
                if isinstance(m, models.LogisticBank):
                    m.weights = torch.ones(k, device='cuda')
        lab = (b, t, k) if c['label_layout'] == 'wrong' else (b, k, t)
        batch = {tools.KEY_FEATS: torch.rand(b, c['ic'], c['dim_in'], t, dtype=dtype, device='cuda').requires_grad_(c['feats_grad'])}
        if c['labels'] != 'none':
            batch[tools.KEY_MULTIPITCH] = torch.zeros(lab, device='cuda')
        if c['labels'] == 'all':
            batch[tools.KEY_ONSETS] = torch.zeros(lab, device='cuda')
            if c['cls'] == 'OnsetsFrames2':
                batch[tools.KEY_OFFSETS] = torch.zeros(lab, device='cuda')
        with _mode('no_grad' if c['no_grad'] else 'train'):
            batch = model.pre_proc(batch)
            batch[tools.KEY_OUTPUT] = model(batch[tools.KEY_FEATS])
            return model.post_proc(batch)
    if c['kind'] == 'tab':
        g = 6
        batch = {tools.KEY_FEATS: torch.rand(b, c['ic'], c['dim_in'], t, dtype=dtype, device='cuda').requires_grad_(c['feats_grad'])}
        if c['labels'] == 'wrong':
            batch[tools.KEY_TABLATURE] = torch.zeros((b, t, g), dtype=torch.int64, device='cuda')
        elif c['labels'] != 'none':
            batch[tools.KEY_TABLATURE] = torch.zeros((b, g, t), dtype=getattr(torch, c['labels']), device='cuda')
        batch = model.pre_proc(batch)
        if c['copy']:
            batch[tools.KEY_FEATS] = batch[tools.KEY_FEATS].contiguous()
        batch[tools.KEY_OUTPUT] = model(batch[tools.KEY_FEATS])
        return model.post_proc(batch)
    with _mode(c['mode']):
        if c['kind'] == 'am':
            return {'out': model(torch.rand(b, 1, t, DIM_IN, device='cuda'))}
        if c['kind'] in ('lm', 'bank'):
            return {'out': model(torch.rand(b, t, c['I' if c['kind'] == 'lm' else 'K'], dtype=dtype, device='cuda'))}
        assert c['kind'] == 'loss'
        v, bank = c['variant'], model
        if v == 'weighted':
            bank.weights = torch.ones(88, device='cuda')
        logits = torch.rand(b, t, 88, dtype=torch.float64 if 'fp64' in v else torch.float32, device='cuda').requires_grad_('detached' not in v)
        labels = torch.zeros((b, t, 88) if v == 'labels (B, T, K)' else (b, 88, t), dtype=torch.uint8 if v == 'uint8 labels' else torch.float32, device='cuda')
        return {'loss': bank.get_loss(logits, labels)}


def _one(c, strict):
    """(events, outputs, fallbacks(), training_backend(), error text or None) of one run of a case."""
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from amt_tools_amd import autograd as ag
    rec = _Recorder()
    note = ag.note_fallback

    def note_fallback(site, reason):
        rec.events.append(['fallback', site, reason])
        note(site, reason)
    env = {'AMTX_TRAIN_OVERLAP': '0', 'AMTX_STRICT_TRAINING': '1' if strict else '0'}
    old_env = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    ag.reset_fallbacks()
    outputs, error = [], None
    with contextlib.ExitStack() as stack:
        stack.enter_context(warnings.catch_warnings())
        warnings.simplefilter('ignore')
        model = _build(c)
        stack.enter_context(_patched(logging.getLogger('torch._subclasses.fake_tensor'), disabled=True))     # it logs the errors the rows record
        for name in FUNCTIONS:
            stack.enter_context(_patched(getattr(ag, name), apply=rec.stub(name, ag)))
        stack.enter_context(_patched(ag, note_fallback=note_fallback, USE_HIP_DENSE=bool(c.get('dense', True))))
        stack.enter_context(_patched(torch.nn.LSTM, forward=rec.stock_lstm()))
        stack.enter_context(FakeTensorMode(allow_non_fake_inputs=True))
        stack.enter_context(torch.device('cuda'))
        try:
            outputs = _flat(_run(c, model))
        except Exception as e:      # noqa: BLE001 -- part of the record: the same text has to come back
            error = '%s: %s' % (type(e).__name__, e)
        backend, taken = ag.training_backend(), {k: list(v) for k, v in sorted(ag.fallbacks().items())}
    for k, v in old_env.items():
        os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    ag.reset_fallbacks()
    return rec.events, outputs, taken, backend, error


def record():
    """[row per case], in the order of cases()."""
    rows = []
    for name, c in cases():
        events, outputs, taken, backend, error = _one(c, strict=False)
        if error is not None:
            events = events + [['error', error]]
        rows.append([events, outputs, taken, backend, _one(c, strict=True)[4] or 'none'])
    return rows


def compact(rows, parent_commit):
    """Events and output lines repeat from case to case: they go into one table, a row names them by index."""
    table = {}

    def index(v):
        return table.setdefault(json.dumps(v), len(table))
    out = [[[index(e) for e in events], [index(o) for o in outputs], taken, index(backend), strict] for events, outputs, taken, backend, strict in rows]
    return dict(table=[json.loads(k) for k in table], cases_sha256=cases_sha256(), parent_commit=parent_commit, names=[n for n, _ in cases()], rows=out)


def expand(c):
    """The inverse of compact."""
    t = c['table']
    return [[[t[i] for i in events], [t[i] for i in outputs], taken, t[backend], strict] for events, outputs, taken, backend, strict in c['rows']]


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
