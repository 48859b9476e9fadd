"""Training path on the GPU: the HIP BiLSTM autograd function against torch's own LSTM (forward values and every gradient),
and one whole training step of the model against the reference's golden losses / gradients (tests/golden/of1_train.npz).
Tolerances: the recurrent mat-vecs use split-bf16 (fp32-class) products -> 2e-4 relative to the largest element."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from conftest import load_golden, golden_grad_slices                 # noqa: E402
from amt_tools_amd import tools                  # noqa: E402


def _rel(a, b):
    return (a - b).abs().max().item() / max(1e-12, b.abs().max().item())


@pytest.mark.parametrize('B,T,I,H', [(B, T, I, H) for H in (128, 256) for B, T, I in [(1, 1, 16), (3, 20, 64), (8, 37, 176), (5, 64, 512)]] +
                         [(B, T, I, H) for H in (384, 512) for B, T, I in [(3, 20, 64), (5, 64, 512)]])
def test_bilstm_autograd_matches_torch_lstm(B, T, I, H):
    """hidden 128: register-stationary kernels; hidden 256, 384, 512 (model_complexity 3, 4, 5): the streaming forward / backward kernels,
    one instantiation per hidden size.  The recurrences alone, against tighter lines: tests/test_gpu_bilstm_train.py."""
    from amt_tools_amd.autograd import bilstm
    torch.manual_seed(B * 1000 + T)
    ref = torch.nn.LSTM(I, H, batch_first=True, bidirectional=True).double()
    x = torch.randn(B, T, I, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(B, T, 2 * H, dtype=torch.float64)
    y_ref = ref(x)[0]
    y_ref.backward(gy)
    mine = torch.nn.LSTM(I, H, batch_first=True, bidirectional=True).cuda()
    mine.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    xc = x.detach().float().cuda().requires_grad_(True)
    y = bilstm(xc, mine)
    y.backward(gy.float().cuda())
    assert _rel(y.detach().cpu().double(), y_ref.detach()) < 2e-5
    assert _rel(xc.grad.cpu().double(), x.grad) < 2e-4
    for (n, p), (_, q) in zip(mine.named_parameters(), ref.named_parameters()):
        assert _rel(p.grad.cpu().double(), q.grad) < 2e-4, n


def test_training_step_on_gpu_matches_reference_golden():
    """The reference's training-mode losses and gradients (BatchNorm batch statistics, dropout off) with the model on the GPU: every
    layer on the HIP forward / backward kernels of amt_tools_amd/autograd.py (2 clips x 24 frames; the BASELINE-size step is
    test_full_size_training_step_matches_the_oracle below)."""
    from amt_tools_amd.models import OnsetsFrames
    from amt_tools_amd.synth import synth_state_dict
    g = load_golden('of1_train.npz')
    model = OnsetsFrames(229, tools.PianoProfile(), 1, int(g['model_complexity']), device='cuda:0')
    sd = synth_state_dict(int(g['seed']), dim_in=229, in_channels=1, model_complexity=int(g['model_complexity']))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model.change_device()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    model.train()
    batch = {tools.KEY_FEATS: torch.from_numpy(g['feats']), tools.KEY_MULTIPITCH: torch.from_numpy(g['multi_pitch']),
             tools.KEY_ONSETS: torch.from_numpy(g['onsets'])}
    out = model.run_on_batch(batch)
    loss = out[tools.KEY_LOSS]
    assert abs(loss[tools.KEY_LOSS_PITCH].item() - float(g['loss_pitch'])) < 2e-3
    assert abs(loss[tools.KEY_LOSS_ONSETS].item() - float(g['loss_onsets'])) < 2e-3
    loss[tools.KEY_LOSS_TOTAL].backward()
    named = dict(model.named_parameters())
    for i, k in enumerate(g['grad_keys']):
        ref = g[f'grad_{i}']
        got = named[str(k)].grad.cpu().numpy()
        assert np.abs(got - ref).max() / max(1e-6, np.abs(ref).max()) < 5e-3, k
    # the stock path gives the same numbers (switch kept for A/B)
    for mod in model.modules():
        if hasattr(mod, 'use_hip_autograd'):
            mod.use_hip_autograd = False
        if hasattr(mod, 'use_hip_bn'):
            mod.use_hip_bn = False
    model.zero_grad()
    out2 = model.run_on_batch(batch)
    assert abs(out2[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL].item() - loss[tools.KEY_LOSS_TOTAL].item()) < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize('B,T,K,weighted', [(8, 625, 88, False), (3, 70, 88, True), (1, 1, 4, False), (2, 33, 120, True)])
def test_bce_logits_loss_matches_torch(B, T, K, weighted):
    """amtx_bce_logits_loss = LogisticBank.get_loss (common.py:541-584) and its gradient, against torch in float64."""
    import torch.nn.functional as F
    from amt_tools_amd.autograd import bce_logits_loss
    g = torch.Generator().manual_seed(B * 1000 + T)
    x = (torch.randn(B, T, K, generator=g) * 4).cuda().requires_grad_(True)
    y = (torch.rand(B, K, T, generator=g) < 0.1).float().cuda()
    w = (torch.rand(K, generator=g) + 0.5).cuda() if weighted else None
    loss = bce_logits_loss(x, y, w)
    (loss * 3.0).backward()
    x64 = x.detach().double().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(x64.transpose(-2, -1), y.double(), weight=None if w is None else w.double().unsqueeze(-1),
                                             reduction='none').mean(dim=-1).sum(dim=-1).mean()
    (ref * 3.0).backward()
    assert abs(loss.item() - ref.item()) <= 2e-6 * abs(ref.item()) + 1e-7          # tolerance: fp32 terms, double reduction
    assert (x.grad.double() - x64.grad).abs().max().item() <= 1e-6 * x64.grad.abs().max().item() + 1e-9
    again = bce_logits_loss(x.detach(), y, w)
    assert again.item() == loss.item()                                             # deterministic


@pytest.mark.gpu
@pytest.mark.parametrize('B,C,T,F,pool', [(2, 32, 9, 229, False), (2, 32, 9, 229, True), (3, 64, 5, 114, True), (1, 48, 7, 18, True),
                                          (1, 96, 3, 2, True), (2, 4, 3, 5, False), (8, 32, 64, 229, True)])
def test_bn_relu_pool_training_matches_torch(B, C, T, F, pool):
    """amtx_bn_relu_pool_train_fwd / _bwd = nn.BatchNorm2d (training) -> ReLU -> [MaxPool2d((1,2))] against torch in float64:
    output, input gradient, gamma / beta gradients, running statistics, num_batches_tracked."""
    from amt_tools_amd.autograd import bn_relu_pool, bn_relu_pool_supported
    gen = torch.Generator().manual_seed(B * 100 + C + T + F)
    x = (torch.randn(B, C, T, F, generator=gen) * 1.5 + 0.3)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=gen) * 0.2)
        bn.running_mean.copy_(torch.randn(C, generator=gen) * 0.1)
        bn.running_var.copy_(torch.rand(C, generator=gen) + 0.5)
    import copy
    ref_bn = copy.deepcopy(bn).double()
    x64 = x.double().requires_grad_(True)
    y_ref = torch.relu(ref_bn(x64))
    if pool:
        y_ref = torch.nn.functional.max_pool2d(y_ref, (1, 2))
    gy = torch.randn(y_ref.shape, generator=gen)
    y_ref.backward(gy.double())

    bn = bn.cuda()
    xc = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    assert bn_relu_pool_supported(xc, bn)
    y = bn_relu_pool(xc, bn, pool)
    assert y.shape == y_ref.shape
    y.backward(gy.cuda())
    assert _rel(y.detach().cpu().double(), y_ref.detach()) < 2e-6
    assert _rel(xc.grad.cpu().double(), x64.grad) < 2e-5
    assert _rel(bn.weight.grad.cpu().double(), ref_bn.weight.grad) < 2e-5
    assert _rel(bn.bias.grad.cpu().double(), ref_bn.bias.grad) < 2e-5
    assert _rel(bn.running_mean.cpu().double(), ref_bn.running_mean) < 1e-6
    assert _rel(bn.running_var.cpu().double(), ref_bn.running_var) < 1e-6
    assert int(bn.num_batches_tracked) == 1
    # deterministic (no atomics)
    xc2 = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y2 = bn_relu_pool(xc2, bn, pool)
    y2.backward(gy.cuda())
    assert torch.equal(xc2.grad, xc.grad)


@pytest.mark.gpu
@pytest.mark.parametrize('mc', [2, 3])
def test_onsetsframes2_training_step_hip_vs_stock_path(mc):
    """OnsetsFrames2 (offset head; mc 3 = as shipped) in training mode: the HIP path (BatchNorm passes, onset + offset recurrences
    as one grouped launch each way, adjoin recurrence) against the stock ATen / MIOpen path on the same parameters and batch
    (dropout off): losses and gradients."""
    from amt_tools_amd.models import OnsetsFrames2, AcousticModel
    from amt_tools_amd.synth import synth_state_dict
    sd = synth_state_dict(31, dim_in=229, in_channels=1, model_complexity=mc, offsets=True)
    rng = np.random.default_rng(mc)
    B, T = 3, 24
    batch = {tools.KEY_FEATS: torch.from_numpy(rng.random((B, 1, 229, T)).astype(np.float32)),
             tools.KEY_MULTIPITCH: torch.from_numpy((rng.random((B, 88, T)) < 0.05).astype(np.float32)),
             tools.KEY_ONSETS: torch.from_numpy((rng.random((B, 88, T)) < 0.02).astype(np.float32)),
             tools.KEY_OFFSETS: torch.from_numpy((rng.random((B, 88, T)) < 0.02).astype(np.float32))}
    results = []
    for hip in (True, False):
        model = OnsetsFrames2(229, tools.PianoProfile(), 1, mc, device='cuda:0')
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        model.change_device()
        for mod in model.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
            if hasattr(mod, 'use_hip_autograd'):
                mod.use_hip_autograd = hip
            if isinstance(mod, AcousticModel):
                mod.use_hip_bn = hip
        model.train()
        out = model.run_on_batch(batch)
        loss = out[tools.KEY_LOSS]
        loss[tools.KEY_LOSS_TOTAL].backward()
        results.append(({k: float(v) for k, v in loss.items()}, {n: p.grad.detach().cpu() for n, p in model.named_parameters() if p.grad is not None}))
    (l_hip, g_hip), (l_ref, g_ref) = results
    assert set(l_hip) == set(l_ref) and 'loss_offsets' in l_hip
    for k in l_ref:
        assert abs(l_hip[k] - l_ref[k]) < 2e-3 * max(1.0, abs(l_ref[k])), k
    assert set(g_hip) == set(g_ref)
    rels = []
    for n in g_ref:
        if n.endswith('.0.bias') and '.layer' in n:
            # a convolution bias in front of a BatchNorm: the batch mean removes it, its gradient is rounding noise on both paths
            assert g_hip[n].abs().max().item() < 1e-4 and g_ref[n].abs().max().item() < 1e-4, n
            continue
        # ReLU / max-pool gradients are discontinuous: an element whose pre-activation sits within an ulp of zero moves one channel's
        # gradients by a per cent or two between two correct fp32 evaluations (seen on either path against a float64 CPU run,
        # depending on the input: notes in HISTORY.md).  Every tensor within 3e-2 in relative L2, the typical one within 1e-3.
        rels.append((g_hip[n] - g_ref[n]).norm().item() / max(1e-9, g_ref[n].norm().item()))
        assert rels[-1] < 3e-2, n
    assert float(np.median(rels)) < 1e-3


@pytest.mark.gpu
def test_bilstm_multi_equals_separate_launches():
    from amt_tools_amd.autograd import bilstm, bilstm_multi
    torch.manual_seed(7)
    B, T, H = 5, 19, 256
    lstms = [torch.nn.LSTM(I, H, batch_first=True, bidirectional=True).cuda() for I in (96, 64)]
    xs = [torch.randn(B, T, I, device='cuda', requires_grad=True) for I in (96, 64)]
    gys = [torch.randn(B, T, 2 * H, device='cuda') for _ in range(2)]
    ys = bilstm_multi(xs, [l for l in lstms])
    (ys[0] * gys[0]).sum().add((ys[1] * gys[1]).sum()).backward()
    got = [x.grad.clone() for x in xs] + [p.grad.clone() for l in lstms for p in l.parameters()]
    for x in xs:
        x.grad = None
    for l in lstms:
        l.zero_grad()
    ys2 = [bilstm(x, l) for x, l in zip(xs, lstms)]
    (ys2[0] * gys[0]).sum().add((ys2[1] * gys[1]).sum()).backward()
    ref = [x.grad for x in xs] + [p.grad for l in lstms for p in l.parameters()]
    for a, b in zip(ys, ys2):
        assert torch.equal(a, b)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize('mc', [4, 5])
def test_complexity_4_training_step_on_gpu_matches_reference_golden(mc):
    """The reference's training-mode losses and gradients at model_complexity 4 and 5 (tests/golden/of1_mc4_train.npz, of1_mc5_train.npz) with
    the model on the GPU: 64 / 64 / 128 (80 / 80 / 160)-channel convolution kernels, the streaming hidden-384 (512) recurrences forward and
    backward."""
    from amt_tools_amd.models import OnsetsFrames
    from amt_tools_amd.synth import synth_state_dict
    import amt_tools_amd.autograd as ag
    g = load_golden(f'of1_mc{mc}_train.npz')
    assert int(g['model_complexity']) == mc
    ag.reset_fallbacks()
    model = OnsetsFrames(229, tools.PianoProfile(), 1, mc, device='cuda:0')
    sd = synth_state_dict(int(g['seed']), dim_in=229, in_channels=1, model_complexity=mc)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model.change_device()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    model.train()
    batch = {tools.KEY_FEATS: torch.from_numpy(g['feats']), tools.KEY_MULTIPITCH: torch.from_numpy(g['multi_pitch']),
             tools.KEY_ONSETS: torch.from_numpy(g['onsets'])}
    loss = model.run_on_batch(batch)[tools.KEY_LOSS]
    assert abs(loss[tools.KEY_LOSS_PITCH].item() - float(g['loss_pitch'])) < 2e-3 * float(g['loss_pitch'])
    assert abs(loss[tools.KEY_LOSS_ONSETS].item() - float(g['loss_onsets'])) < 2e-3 * float(g['loss_onsets'])
    loss[tools.KEY_LOSS_TOTAL].backward()
    named = dict(model.named_parameters())
    rels = []
    for i, k in enumerate(g['grad_keys']):
        ref = torch.from_numpy(g[f'grad_{i}'])
        got = named[str(k)].grad.cpu()
        rels.append((got - ref).norm().item() / max(1e-9, ref.norm().item()))
        assert rels[-1] < 3e-2, (k, rels[-1])
    assert float(np.median(rels)) < 2e-3
    # rows of the recurrent matrices' gradients: the hidden-384 streaming forward (saved h) and backward (W_hh^T fragments) kernels
    slices = golden_grad_slices(g)
    assert len(slices) == (4 if mc == 4 else 5)
    for k, st, ref in slices:
        got = named[k].grad.cpu().numpy()[::st]
        rel = np.linalg.norm(got - ref) / max(1e-9, np.linalg.norm(ref))
        assert rel < 3e-3, (k, rel)
    assert ag.fallbacks() == {}, ag.fallbacks()          # every layer of the step on the HIP kernels


@pytest.mark.gpu
def test_onsetsframes2_training_step_on_gpu_matches_reference_golden():
    """The reference's own OnsetsFrames2 (model_complexity 3) training-mode losses and gradients (tests/golden/of2_train.npz) with the
    model on the GPU: ATen convolutions + HIP BatchNorm passes + the streaming hidden-256 recurrences (onset + offset grouped)."""
    from amt_tools_amd.models import OnsetsFrames2
    from amt_tools_amd.synth import synth_state_dict
    g = load_golden('of2_train.npz')
    mc = int(g['model_complexity'])
    model = OnsetsFrames2(int(g['dim_in']), tools.PianoProfile(), 1, mc, device='cuda:0')
    sd = synth_state_dict(int(g['seed']), dim_in=int(g['dim_in']), in_channels=1, model_complexity=mc, offsets=True)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model.change_device()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    model.train()
    batch = {tools.KEY_FEATS: torch.from_numpy(g['feats']), tools.KEY_MULTIPITCH: torch.from_numpy(g['multi_pitch']),
             tools.KEY_ONSETS: torch.from_numpy(g['onsets']), tools.KEY_OFFSETS: torch.from_numpy(g['offsets'])}
    loss = model.run_on_batch(batch)[tools.KEY_LOSS]
    for k, v in zip(g['loss_keys'], g['loss_values']):
        assert abs(loss[str(k)].item() - float(v)) < 2e-3 * max(1.0, abs(float(v))), k
    loss[tools.KEY_LOSS_TOTAL].backward()
    named = dict(model.named_parameters())
    rels = []
    for i, k in enumerate(g['grad_keys']):
        ref = torch.from_numpy(g[f'grad_{i}'])
        got = named[str(k)].grad.cpu()
        rels.append((got - ref).norm().item() / max(1e-9, ref.norm().item()))
        assert rels[-1] < 3e-2, (k, rels[-1])        # see test_onsetsframes2_training_step_hip_vs_stock_path for the metric
    assert float(np.median(rels)) < 2e-3


@pytest.mark.parametrize('M,N,K', [(1, 4, 4), (37, 88, 256), (625, 512, 3648), (5000, 88, 512), (130, 1024, 176), (4999, 132, 36)])
def test_linear_fwd_bwd_matches_float64(M, N, K):
    """autograd.linear (amtx_linear_train_fwd / amtx_linear_bwd: split-bf16 GEMMs, split contraction for the weight gradient) against
    torch's float64 linear: output, input gradient, weight gradient, bias gradient."""
    from amt_tools_amd.autograd import linear
    torch.manual_seed(M + N + K)
    x = torch.randn(M, K, dtype=torch.float64, requires_grad=True)
    w = torch.randn(N, K, dtype=torch.float64, requires_grad=True)
    b = torch.randn(N, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(M, N, dtype=torch.float64)
    y = torch.nn.functional.linear(x, w, b)
    y.backward(gy)
    xc, wc, bc = (t.detach().float().cuda().requires_grad_(True) for t in (x, w, b))
    yc = linear(xc, wc, bc)
    yc.backward(gy.float().cuda())
    assert _rel(yc.detach().cpu().double(), y.detach()) < 2e-5
    assert _rel(xc.grad.cpu().double(), x.grad) < 2e-5
    assert _rel(wc.grad.cpu().double(), w.grad) < 2e-5
    assert _rel(bc.grad.cpu().double(), b.grad) < 2e-5
    # 3-D input with a strided row view as nn.Linear sees them inside the model
    x3 = torch.randn(2, 5, 2 * K, device='cuda')[..., :K].requires_grad_(True)
    y3 = linear(x3, wc.detach(), bc.detach())
    ref3 = torch.nn.functional.linear(x3.detach().double().cpu(), w.detach(), b.detach())
    assert y3.shape == (2, 5, N) and _rel(y3.detach().cpu().double(), ref3) < 2e-5


@pytest.mark.parametrize('ci,co', [(1, 32), (32, 32), (32, 64), (48, 96), (16, 16)])
# (3, 64, 229) = 43 968 positions: more than the 24 576 that one xwgrad_kernel step per block covers (several steps per block, the per-step
# advance of the x / dy strips and the clip wrap inside the loop: ADVICE r02), several clips
@pytest.mark.parametrize('B,T,F', [(1, 1, 2), (2, 7, 13), (3, 20, 57), (1, 33, 229), (3, 64, 229)])
def test_conv3x3_fwd_bwd_matches_float64(ci, co, B, T, F):
    """autograd.conv3x3 (implicit GEMMs of csrc/train.hip) against torch's float64 Conv2d: output, input gradient (where the layer
    has one: not the one-channel first layer), weight and bias gradients; zero padding at clip boundaries in time and at the band
    edges, clips of a batch independent."""
    from amt_tools_amd.autograd import conv3x3
    torch.manual_seed(ci * 1000 + co + B + T + F)
    ref = torch.nn.Conv2d(ci, co, 3, padding=1).double()
    x = torch.randn(B, ci, T, F, dtype=torch.float64, requires_grad=ci > 1)
    gy = torch.randn(B, co, T, F, dtype=torch.float64)
    y = ref(x)
    y.backward(gy)
    mine = torch.nn.Conv2d(ci, co, 3, padding=1).cuda()
    mine.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    xc = x.detach().float().cuda().contiguous(memory_format=torch.channels_last).requires_grad_(ci > 1)
    yc = conv3x3(xc, mine)
    assert yc.is_contiguous(memory_format=torch.channels_last) or ci == 1 or F * T == 1
    yc.backward(gy.float().cuda())
    assert _rel(yc.detach().cpu().double(), y.detach()) < 2e-5
    if ci > 1:
        assert _rel(xc.grad.cpu().double(), x.grad) < 2e-5
    assert _rel(mine.weight.grad.cpu().double(), ref.weight.grad) < 2e-5
    assert _rel(mine.bias.grad.cpu().double(), ref.bias.grad) < 2e-5


def test_training_step_runs_without_vendor_gemm_or_conv_kernels():
    """With the HIP dense layers on (the default) a whole training step of OnsetsFrames must not launch a MIOpen / hipBLASLt /
    rocBLAS kernel: checked with torch's profiler on the kernel names of one step."""
    from amt_tools_amd.models import OnsetsFrames
    from amt_tools_amd.synth import synth_labels
    torch.manual_seed(0)
    model = OnsetsFrames(229, tools.PianoProfile(), 1, 2, device='cuda:0')
    model.change_device()
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=6e-4)
    B, T = 2, 64
    lab = [synth_labels(i, num_frames=T) for i in range(B)]
    batch = {tools.KEY_FEATS: torch.rand(B, 1, 229, T), tools.KEY_MULTIPITCH: torch.from_numpy(np.stack([l[0] for l in lab])),
             tools.KEY_ONSETS: torch.from_numpy(np.stack([l[1] for l in lab]))}

    def step():
        opt.zero_grad()
        model.run_on_batch(batch)[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL].backward()
        opt.step()

    step()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA or 'kernel' in e.key.lower()]
    vendor = [n for n in names if any(t in n.lower() for t in ('miopen', 'cijk_', 'rocblas', 'hipblas', 'igemm', 'gemv'))]
    assert not vendor, vendor
    assert any('xgemm_kernel' in n for n in names), names[:20]


@pytest.mark.parametrize('c_in,dim_in', [(6, 72), (3, 48)])
def test_multi_channel_first_conv_trains_on_the_hip_kernels(c_in, dim_in):
    """An HCQT-shaped model (6 harmonics x 72 bins, amt_tools/features/hvqt.py:107-133; also 3 channels) trains its FIRST convolution on
    the HIP implicit GEMMs too (zero-padded to a multiple of 4 channels) -- VERDICT r03: it went to MIOpen without a word.  Checked three
    ways: no vendor kernel in the step's trace, no recorded fallback, gradients equal to the stock ATen path's."""
    from amt_tools_amd import autograd as ag
    from amt_tools_amd.models import OnsetsFrames
    from amt_tools_amd.synth import synth_labels
    B, T = 2, 48
    lab = [synth_labels(i, num_frames=T) for i in range(B)]
    torch.manual_seed(1)
    batch = {tools.KEY_FEATS: torch.rand(B, c_in, dim_in, T), tools.KEY_MULTIPITCH: torch.from_numpy(np.stack([l[0] for l in lab])),
             tools.KEY_ONSETS: torch.from_numpy(np.stack([l[1] for l in lab]))}

    def make():
        torch.manual_seed(0)
        m = OnsetsFrames(dim_in, tools.PianoProfile(), c_in, 2, device='cuda:0')
        m.change_device()
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        m.train()
        return m

    ag.reset_fallbacks()
    model = make()
    model.run_on_batch(batch)[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL].backward()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        model.zero_grad()
        loss = model.run_on_batch(batch)[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL]
        loss.backward()
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    vendor = [n for n in names if any(t in n.lower() for t in ('miopen', 'cijk_', 'rocblas', 'hipblas', 'igemm', 'gemv'))]
    assert not vendor, vendor
    assert ag.fallbacks() == {}, ag.fallbacks()
    assert 'FALLBACKS' not in ag.training_backend()

    ref = make()
    ag.USE_HIP_DENSE = False
    try:
        for m in ref.modules():
            if hasattr(m, 'use_hip_bn'):
                m.use_hip_bn = False
        loss_ref = ref.run_on_batch(batch)[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL]
        loss_ref.backward()
    finally:
        ag.USE_HIP_DENSE = True
    assert 'AcousticModel stage' in ag.fallbacks()            # the stock path is on the record ...
    assert 'FALLBACKS TAKEN' in ag.training_backend()         # ... and in the line bench.py prints
    ag.reset_fallbacks()
    assert abs(loss.item() - loss_ref.item()) < 2e-3 * abs(loss_ref.item())
    rel = []
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        if '.layer' in n and n.endswith('.0.bias'):
            # a convolution bias in front of a training-mode BatchNorm: its gradient is exactly zero in real arithmetic (the batch mean
            # removes it), both paths return rounding noise
            assert float(p.grad.norm()) < 1e-3 and float(q.grad.norm()) < 1e-3, n
            continue
        rel.append(float((p.grad - q.grad).norm() / (q.grad.norm() + 1e-12)))
    w1 = dict(model.named_parameters())['onset_head.0.layer1.0.weight'].grad
    w1r = dict(ref.named_parameters())['onset_head.0.layer1.0.weight'].grad
    assert float((w1 - w1r).norm() / w1r.norm()) < 3e-2
    assert np.median(rel) < 1e-3 and max(rel) < 3e-2, (np.median(rel), max(rel))


@pytest.mark.timeout(900)
@pytest.mark.parametrize('of2', [False, True], ids=['OnsetsFrames_mc2', 'OnsetsFrames2_mc3'])
def test_full_size_training_step_matches_the_oracle(of2, capsys):
    """BASELINE config 4 at its real size: ONE training step of 8 clips x 625 frames -- audio -> HIP log-mel front-end
    (model.frontend) -> HIP forward / backward kernels (625-step BPTT in split-bf16) -> losses, EVERY parameter gradient (all tensors, the
    recurrent matrices `weight_hh_l0*` included), then one Adam step (lr 6e-4) -- against the CPU oracle: fp64 numpy front-end + the fp32
    torch restatement `oracle/model_ref.run_on_batch(training=True)` (BatchNorm batch statistics, dropout off; LSTM_IMPL='aten', pinned to the
    reference's goldens in tests/test_oracle_model.py).  Follows amt_tools/train.py:126-141 and models/common.py:541-584.
    Bounds: losses 2e-4 relative; per tensor max|g - g_ref| <= 5e-3 max|g_ref|; Conv2d biases in front of a batch-statistics BatchNorm have
    gradient exactly zero (compared as noise on the weight gradient's scale); after the Adam step |w - w_ref| <= 2 lr everywhere (Adam's first
    step is lr sign(g)) and <= 1e-6 + 1e-3 lr wherever the reference gradient is clear of the gradient tolerance."""
    from amt_tools_amd.features import MelSpec
    from amt_tools_amd.models import OnsetsFrames, OnsetsFrames2
    from amt_tools_amd.synth import synth_clip, synth_labels, synth_state_dict
    from oracle import frontend_np as fe, model_ref
    B, mc, lr = 8, (3 if of2 else 2), 6e-4
    sd_np = synth_state_dict(11, dim_in=229, in_channels=1, model_complexity=mc, offsets=of2)
    audio = np.stack([synth_clip(40 + i) for i in range(B)])
    lab = [synth_labels(40 + i) for i in range(B)]
    labels = {'multi_pitch': torch.from_numpy(np.stack([l[0] for l in lab])), 'onsets': torch.from_numpy(np.stack([l[1] for l in lab]))}
    if of2:
        labels['offsets'] = torch.from_numpy(np.stack([l[1][:, ::-1].copy() for l in lab]))

    # ---- the HIP path, through the product API (train.py:122-141)
    cls = OnsetsFrames2 if of2 else OnsetsFrames
    model = cls(229, tools.PianoProfile(), 1, mc, device='cuda:0')
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()})
    model.frontend = torch.nn.Sequential(MelSpec(sample_rate=22050, hop_length=512, n_mels=229, n_fft=2048, device='cuda:0').frontend())
    model.change_device()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    model.train()
    from amt_tools_amd import autograd as ag
    ag.reset_fallbacks()
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    batch = {tools.KEY_AUDIO: torch.from_numpy(audio), tools.KEY_MULTIPITCH: labels['multi_pitch'], tools.KEY_ONSETS: labels['onsets']}
    if of2:
        batch[tools.KEY_OFFSETS] = labels['offsets']
    opt.zero_grad()
    loss = model.run_on_batch(batch)[tools.KEY_LOSS]
    loss[tools.KEY_LOSS_TOTAL].backward()
    assert not ag.fallbacks(), ag.fallbacks()                  # every layer of the step ran on the HIP kernels
    got_loss = {k: float(v.detach()) for k, v in loss.items()}
    got_grad = {k: p.grad.detach().cpu().contiguous().numpy().copy() for k, p in model.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    got_w = {k: p.detach().cpu().contiguous().numpy().copy() for k, p in model.named_parameters()}

    # ---- the oracle
    old_impl, model_ref.LSTM_IMPL = model_ref.LSTM_IMPL, 'aten'
    try:
        feats = np.stack([fe.melspec_process_audio(a, 22050, 512, 229, 2048, dtype=np.float32) for a in audio]).astype(np.float32)
        sd = {k: torch.from_numpy(np.asarray(v)).clone() for k, v in sd_np.items()}
        leaves = {k: v.requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and 'running_' not in k}
        ref = model_ref.run_on_batch(torch.from_numpy(feats), sd, labels, training=True, detach_heads=of2)
        ref['loss']['loss_total'].backward()
    finally:
        model_ref.LSTM_IMPL = old_impl
    assert set(leaves) == set(got_grad), set(leaves) ^ set(got_grad)
    for k, v in ref['loss'].items():
        assert abs(got_loss[k] - float(v.detach())) <= 2e-4 * abs(float(v.detach())), (k, got_loss[k], float(v.detach()))
    ref_grad = {k: v.grad.numpy().copy() for k, v in leaves.items()}
    ropt = torch.optim.Adam(list(leaves.values()), lr=lr)
    ropt.step()
    worst, worst_k, n_tensors, flips, entries = 0.0, None, 0, 0, 0
    for k, g_ref in ref_grad.items():
        g = got_grad[k]
        assert g.shape == g_ref.shape, k
        if '.0.layer' in k and k.endswith('.0.bias'):          # exactly-zero gradient (bias in front of batch-statistics BatchNorm)
            scale = np.abs(ref_grad[k[:-4] + 'weight']).max()
            assert np.abs(g).max() <= 1e-2 * scale and np.abs(g_ref).max() <= 1e-2 * scale, k
            continue
        scale = max(1e-12, np.abs(g_ref).max())
        err = np.abs(g - g_ref).max() / scale
        n_tensors += 1
        if err > worst:
            worst, worst_k = err, k
        assert err <= 5e-3, (k, err)
        # one Adam step: lr sign(g) wherever |g| >> eps
        w, w_ref = got_w[k], leaves[k].detach().numpy()
        dw = np.abs(w - w_ref)
        assert dw.max() <= 2 * lr * 1.001 + 1e-7, (k, dw.max())
        clear = np.abs(g_ref) > 2 * 5e-3 * scale
        if clear.any():
            assert dw[clear].max() <= 1e-6 + 1e-3 * lr, (k, dw[clear].max())
        flips += int((dw > 0.5 * lr).sum())
        entries += dw.size
    with capsys.disabled():
        print(f'\n[config 4 full size, {"OnsetsFrames2 mc=3" if of2 else "OnsetsFrames mc=2"}] 8 clips x 625 frames: losses '
              f'{ {k: round(v, 4) for k, v in got_loss.items()} }; {n_tensors} gradient tensors, worst relative error {worst:.2e} ({worst_k}); '
              f'after one Adam step {flips} of {entries} weights moved the other way (|g_ref| inside the gradient tolerance)')


# (call, arguments): the smallest that reach each route of train.hip.  matmul: (m, n, k, what ldc has more than n);
# linear_db: amtx_linear_bwd's bias gradient alone at (m, n, k); conv_fwd / conv_bwd: (c_in, c_out) at rows 34, 17 frames a clip, 10 bins
TRAIN_ROUTES = [('matmul', (37, 32, 256, 0)), ('matmul', (37, 64, 256, 0)), ('matmul', (37, 88, 256, 0)),      # the three tile widths
                ('matmul', (88, 512, 5000, 0)), ('matmul', (88, 512, 5000, 4)),                              # split + reduce; a padded C: one launch
                ('linear_db', (1024, 64, 176)), ('linear_db', (5000, 88, 512)), ('linear_db', (511, 64, 176)),     # flat, row groups, direct
                ('conv_fwd', (32, 32)), ('conv_fwd', (32, 64)), ('conv_fwd', (64, 64)), ('conv_fwd', (48, 96)), ('conv_fwd', (1, 32)),   # strip x 2, generic x 2, conv1
                ('conv_bwd', (32, 64)), ('conv_bwd', (48, 96))]                                              # <32, 9> dgrad + xwgrad_kernel<4>; generic


@pytest.mark.parametrize('call,args', TRAIN_ROUTES, ids=lambda v: v if isinstance(v, str) else '-'.join(map(str, v)))
def test_train_entry_points_launch_the_recorded_kernels(call, args):
    """Each entry point launches the kernels -- instantiations and counts -- of the row that tests/golden/train_trace.json holds for the same
    arguments (tests/test_train_trace.py: recorded on the host, before train.hip took its decisions from routes), with a workspace of exactly
    the query's answer.  Operands are zeros: only the launches are looked at."""
    import collections
    import json
    import os
    import re
    import sys
    from amt_tools_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, 'san'))
    import train_trace
    L, dev, rows, t, f = _lib.lib(), 'cuda:0', 34, 17, 10
    stream = _lib.current_stream()

    def z(*shape):
        return torch.zeros(*shape, device=dev)

    def workspace(need):
        return torch.zeros(int(need), dtype=torch.uint8, device=dev)
    if call == 'matmul':
        m, n, k, pad = args
        case = train_trace.matmul_case(m, n, k, ldc_pad=pad)
        a, b, bias, c, ws = z(m, k), z(n, k), z(n), z(m, n + pad), workspace(L.amtx_matmul_workspace_bytes(m, n, k))
        run = lambda: _lib.check(L.amtx_matmul_f32(_lib.ptr(a), k, 0, _lib.ptr(b), k, 0, _lib.ptr(bias), _lib.ptr(c), n + pad, m, n, k,      # noqa: E731
                                                   _lib.ptr(ws), ws.numel(), stream), 'amtx_matmul_f32')
    elif call == 'linear_db':
        m, n, k = args
        case = train_trace.linear_bwd_case(m, n, k, 4)
        dy, db, ws = z(m, n), z(n), workspace(L.amtx_linear_bwd_workspace_bytes(m, n, k))
        run = lambda: _lib.check(L.amtx_linear_bwd(_lib.ptr(dy), n, None, k, None, k, None, k, None, _lib.ptr(db), m, n, k,                  # noqa: E731
                                                   _lib.ptr(ws), ws.numel(), stream), 'amtx_linear_bwd')
    else:
        ci, co = args
        x, w, bias, y, ws = z(rows, f, ci), z(co, ci, 3, 3), z(co), z(rows, f, co), workspace(L.amtx_conv3x3_train_workspace_bytes(rows, f, ci, co))
        if call == 'conv_fwd':
            case = train_trace.conv_fwd_case(rows, t, f, ci, co)
            run = lambda: _lib.check(L.amtx_conv3x3_train_fwd(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(y), rows, t, f, ci, co,     # noqa: E731
                                                              _lib.ptr(ws), ws.numel(), stream), 'amtx_conv3x3_train_fwd')
        else:
            case = train_trace.conv_bwd_case(rows, t, f, ci, co, 7)
            dx, dw = z(rows, f, ci), z(co, ci, 3, 3)
            run = lambda: _lib.check(L.amtx_conv3x3_bwd(_lib.ptr(y), _lib.ptr(x), _lib.ptr(w), _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(bias),   # noqa: E731
                                                        rows, t, f, ci, co, _lib.ptr(ws), ws.numel(), stream), 'amtx_conv3x3_bwd')
    with open(os.path.join(here, 'golden', 'train_trace.json')) as fh:
        golden = json.load(fh)
    assert golden['cases_sha256'] == train_trace.cases_sha256()
    rc, err, recorded = train_trace.expand(golden)[train_trace.cases().index(case)]
    assert rc == 0 and not err

    def kernel(text):
        m = re.search(r'\w+_kernel(<[^>]*>)?', text)
        return m and m.group(0)
    want = collections.Counter(kernel(line) for line in recorded if kernel(line))
    run()                                                             # the LDS grant and lazy module load stay out of the profile
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    ran = collections.Counter()
    for e in prof.key_averages():
        if kernel(e.key):
            ran[kernel(e.key)] += e.count
    print(f'TRAINROUTE {case!r}: {dict(ran)}')
    assert want and ran == want, (case, [e.key for e in prof.key_averages()])


@pytest.mark.parametrize('case', ['of1', 'of1 87 keys', 'of1 use_hip_bn off on the pitch head'])
def test_fallbacks_of_a_training_step_are_those_of_the_recorded_dispatch(case, monkeypatch):
    """tests/golden/train_dispatch.json is recorded on fake CUDA tensors (tests/train_dispatch_trace.py): here one real training step of the
    same three models (OnsetsFrames, dim_in 32, model_complexity 2, 2 clips x 16 frames; 87 keys; use_hip_bn off on the pitch head) on one
    stream has to record the (site, reason) sequence of the golden row of the same name, and give a finite loss."""
    import json
    import os
    import sys
    from amt_tools_amd import autograd as ag
    from amt_tools_amd.models import OnsetsFrames
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    import train_dispatch_trace as trace
    with open(os.path.join(here, 'golden', 'train_dispatch.json')) as fh:
        golden = json.load(fh)
    assert golden['cases_sha256'] == trace.cases_sha256()
    want = [tuple(e[1:]) for e in trace.expand(golden)[golden['names'].index(case)][0] if e[0] == 'fallback']
    assert bool(want) == (case != 'of1')
    monkeypatch.setenv('AMTX_TRAIN_OVERLAP', '0')
    seen, note = [], ag.note_fallback
    monkeypatch.setattr(ag, 'note_fallback', lambda site, reason: (seen.append((site, reason)), note(site, reason))[1])
    keys = 87 if '87' in case else 88
    torch.manual_seed(3)
    model = OnsetsFrames(32, tools.PianoProfile(high=107 if keys == 87 else None), 1, 2, device='cuda:0')
    model.change_device()
    model.train()
    if 'use_hip_bn' in case:
        model.pitch_head[0].use_hip_bn = False
    batch = {tools.KEY_FEATS: torch.rand(2, 1, 32, 16), tools.KEY_MULTIPITCH: (torch.rand(2, keys, 16) < 0.05).float(),
             tools.KEY_ONSETS: (torch.rand(2, keys, 16) < 0.02).float()}
    try:
        loss = model.run_on_batch(batch)[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL]
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ag.reset_fallbacks()
    print(f'DISPATCH {case!r}: {seen}')
    assert seen == want, (seen, want)
    assert bool(torch.isfinite(loss))
