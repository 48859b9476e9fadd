"""CPU-side checks of TabCNN training on shared-window sequences: the amtx_tab_pool_train_* /
amtx_softmax_groups_loss C ABI (exports, argument checks, workspace sizes -- no compute calls, no GPU needed), a float64 pure-torch
restatement of the dataflow the GPU path runs (padded convolutions over the whole sequence on the kernels' axes, pool read from the
interior) against the stock per-window path, and the reference golden against the stock CPU training path."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from amt_tools_amd import _lib, tools
from amt_tools_amd.models import TabCNN, tab_window_view
from amt_tools_amd.synth import synth_tabcnn_state_dict

from conftest import load_golden

NEW_FUNCS = ('amtx_tab_pool_train_fwd', 'amtx_tab_pool_train_bwd', 'amtx_softmax_groups_loss_workspace_bytes', 'amtx_softmax_groups_loss')
ERR_ARG = -1


def test_tab_train_abi_is_exported():
    L = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW_FUNCS:
        assert name in declared and name in _lib.signatures() and hasattr(L, name), name


def test_tab_train_argument_errors():
    L = _lib.lib()
    buf = np.zeros(4096, dtype=np.float32)
    rec = np.zeros(4096, dtype=np.uint8)
    tg = np.zeros(64, dtype=np.int64)
    p, r, t = _lib.ptr(buf), _lib.ptr(rec), _lib.ptr(tg)
    # pool forward: null pointers, too few bins, empty batch, negative stride
    assert L.amtx_tab_pool_train_fwd(None, 1, 1, 1, 1, 1, 4, 10, 2, p, r, None) == ERR_ARG
    assert b'null' in L.amtx_last_error()
    assert L.amtx_tab_pool_train_fwd(p, 1, 1, 1, 1, 1, 4, 10, 2, p, None, None) == ERR_ARG
    assert L.amtx_tab_pool_train_fwd(p, 1, 1, 1, 1, 1, 4, 7, 2, p, r, None) == ERR_ARG
    assert b'num_bins' in L.amtx_last_error()
    assert L.amtx_tab_pool_train_fwd(p, 1, 1, 1, 1, 0, 4, 10, 2, p, r, None) == ERR_ARG
    assert L.amtx_tab_pool_train_fwd(p, 1, 1, 1, 1, 1, 4, 10, 0, p, r, None) == ERR_ARG
    assert L.amtx_tab_pool_train_fwd(p, 1, -1, 1, 1, 1, 4, 10, 2, p, r, None) == ERR_ARG
    assert b'stride' in L.amtx_last_error()
    # pool backward
    assert L.amtx_tab_pool_train_bwd(None, r, 1, 4, 10, 2, p, None) == ERR_ARG
    assert L.amtx_tab_pool_train_bwd(p, None, 1, 4, 10, 2, p, None) == ERR_ARG
    assert L.amtx_tab_pool_train_bwd(p, r, 1, 4, 10, 2, None, None) == ERR_ARG
    assert L.amtx_tab_pool_train_bwd(p, r, 1, 0, 10, 2, p, None) == ERR_ARG
    assert L.amtx_tab_pool_train_bwd(p, r, 1, 4, 5, 2, p, None) == ERR_ARG
    # loss: null pointers, ld shorter than a row, empty sizes, workspace too small / missing
    need = int(L.amtx_softmax_groups_loss_workspace_bytes(2, 8, 6, 21))
    assert need > 0
    assert L.amtx_softmax_groups_loss(None, 126, t, None, 2, 8, 6, 21, p, p, p, need, None) == ERR_ARG
    assert L.amtx_softmax_groups_loss(p, 126, None, None, 2, 8, 6, 21, p, p, p, need, None) == ERR_ARG
    assert L.amtx_softmax_groups_loss(p, 126, t, None, 2, 8, 6, 21, None, p, p, need, None) == ERR_ARG
    assert L.amtx_softmax_groups_loss(p, 125, t, None, 2, 8, 6, 21, p, p, p, need, None) == ERR_ARG
    assert b'bad sizes' in L.amtx_last_error()
    assert L.amtx_softmax_groups_loss(p, 126, t, None, 0, 8, 6, 21, p, p, p, need, None) == ERR_ARG
    assert L.amtx_softmax_groups_loss(p, 126, t, None, 2, 8, 6, 0, p, p, p, need, None) == ERR_ARG
    assert L.amtx_softmax_groups_loss(p, 126, t, None, 2, 8, 6, 21, p, p, p, need - 1, None) == ERR_ARG
    assert b'workspace' in L.amtx_last_error()
    assert L.amtx_softmax_groups_loss(p, 126, t, None, 2, 8, 6, 21, p, p, None, need, None) == ERR_ARG


def test_softmax_groups_loss_workspace_is_monotone():
    L = _lib.lib()
    assert L.amtx_softmax_groups_loss_workspace_bytes(0, 8, 6, 21) == 0
    assert L.amtx_softmax_groups_loss_workspace_bytes(2, 8, 6, -1) == 0
    prev = 0
    for B, T in ((1, 1), (1, 30), (2, 30), (30, 200), (64, 200), (64, 1292)):
        n = int(L.amtx_softmax_groups_loss_workspace_bytes(B, T, 6, 21))
        assert n >= prev and n >= 4
        prev = n
    assert L.amtx_softmax_groups_loss_workspace_bytes(30, 200, 12, 21) >= L.amtx_softmax_groups_loss_workspace_bytes(30, 200, 6, 21)


# ------------------------------------------------------------------------------------------------------------------------------
# the dataflow of the GPU path, restated in float64 torch
# ------------------------------------------------------------------------------------------------------------------------------
def restated_logits(model, windows):
    """TabCNN's training forward (Dropout off) as the HIP path computes it: the sequence behind the window view on the kernels' axes
    (B, C, cols, F), three PADDED 3x3 convolutions with the weights' spatial axes swapped, ReLU between them, window t's 2x2 pool from
    rows {2h+3, 2h+4} x columns {t+3, t+4} of conv3's map, channel-major flatten, fc + ReLU, output layer."""
    view = tab_window_view(windows, model.frame_width) if windows.dtype == torch.float32 else _view64(windows, model.frame_width)
    assert view is not None
    B, T = windows.shape[:2]
    sb, sc, sf, st = view['strides']
    y = windows.as_strided((B, model.in_channels, view['num_cols'], model.dim_in), (sb, sc, st, sf), view['offset'])
    for i, idx in enumerate((0, 2, 4)):
        conv = model.conv[idx]
        y = F.conv2d(y, conv.weight.transpose(-1, -2), conv.bias, padding=1)
        if i < 2:
            y = torch.relu(y)
    H = (model.dim_in - 6) // 2
    r = 3 + 2 * torch.arange(H)
    c = 3 + torch.arange(T)
    quad = [y[:, :, c + dc][:, :, :, r + dr] for dr in (0, 1) for dc in (0, 1)]           # (B, C, T, H) each, row-major window order
    pooled = torch.relu(torch.stack(quad, 0).amax(0))
    x = pooled.permute(0, 2, 1, 3).reshape(B * T, -1)                                      # row b*T + t, column c*H + h
    x = torch.relu(model.dense[0](x))
    return model.dense[-1](x).reshape(B, T, -1)


def _view64(windows, W):
    # tab_window_view only answers for fp32; the float64 restatement needs the same geometry
    B, T, Cc, Fd, _ = windows.shape
    sb, st, sc, sf, sw = windows.stride()
    assert st == sw
    return dict(offset=windows.storage_offset(), num_windows=T, num_cols=T + W - 1, strides=(sb, sc, sf, st))


def _model(dim_in, in_channels=1, mc=1, seed=0, dtype=torch.float64, weighted=False):
    m = TabCNN(dim_in, tools.GuitarProfile(num_frets=19), in_channels, mc)
    sd = synth_tabcnn_state_dict(seed, dim_in=dim_in, in_channels=in_channels, model_complexity=mc, num_groups=6, num_classes=21)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    if weighted:
        m.dense[-1].set_weights(np.random.default_rng(seed).uniform(0.25, 2.0, 6 * 21))
    m.to(dtype)
    m.train()
    return m


def _grads(model, loss):
    model.zero_grad()
    loss.backward()
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize('T, dim_in, in_channels, mc, online', [(1, 192, 1, 1, False), (2, 10, 1, 1, False), (9, 9, 1, 1, False),
                                                                (37, 10, 6, 1, False), (9, 24, 1, 2, False), (37, 24, 1, 1, True),
                                                                (5, 16, 3, 1, True)])
def test_restated_shared_window_dataflow_matches_the_per_window_path(T, dim_in, in_channels, mc, online):
    """Same loss and the same gradient of every parameter (to 1e-10 of each tensor's max) as the stock per-window path: pins the index
    mapping (axis swap, interior offsets, pool rows / columns, flatten order) before any GPU run.  H = 1 at dim_in 9 and 10."""
    model = _model(dim_in, in_channels, mc, seed=T + dim_in)
    if online:
        model.toggle_online()
    g = torch.Generator().manual_seed(T)
    feats = torch.rand((2, in_channels, dim_in, T), generator=g, dtype=torch.float64) - 0.3
    labels = torch.randint(-1, 21, (2, 6, max(T - 8, 1) if online else T), generator=g)
    windows = model.pre_proc({tools.KEY_FEATS: feats})[tools.KEY_FEATS]
    assert windows.shape[1] == labels.shape[-1]
    stock = model(windows)[tools.KEY_TABLATURE]
    loss_s = model.dense[-1].get_loss(stock, labels)
    gs = _grads(model, loss_s)
    ours = restated_logits(model, windows)
    loss_o = model.dense[-1].get_loss(ours, labels)
    go = _grads(model, loss_o)
    assert abs(loss_s.item() - loss_o.item()) <= 1e-10 * abs(loss_s.item())
    assert (stock - ours).abs().max().item() <= 1e-10 * stock.abs().max().item()
    for k in gs:
        scale = max(gs[k].abs().max().item(), 1e-300)
        assert (gs[k] - go[k]).abs().max().item() <= 1e-10 * scale, k


# ------------------------------------------------------------------------------------------------------------------------------
# the reference golden
# ------------------------------------------------------------------------------------------------------------------------------
def test_tabcnn_train_golden_matches_the_cpu_stock_training_path():
    """tests/golden/tabcnn_train.npz (the reference TabCNN in train mode, Dropout p = 0; tools/gen_golden.py tabcnn_train) against this
    package's CPU training path in fp32: loss and all ten parameter gradients."""
    g = load_golden('tabcnn_train.npz')
    step = int(g['fc_row_step'])
    for i in range(int(g['num_cases'])):
        pre = f'c{i}_'
        dim_in, cin = int(g[pre + 'dim_in']), int(g[pre + 'in_channels'])
        model = _model(dim_in, cin, 1, seed=int(g[pre + 'seed']), dtype=torch.float32)
        if bool(g[pre + 'weighted']):
            model.dense[-1].set_weights(g[pre + 'weights'])
        out = model.run_on_batch({tools.KEY_FEATS: torch.from_numpy(g[pre + 'feats']), tools.KEY_TABLATURE: torch.from_numpy(g[pre + 'tablature'])})
        loss = out[tools.KEY_LOSS][tools.KEY_LOSS_TOTAL]
        grads = _grads(model, loss)
        assert [str(k) for k in g[pre + 'keys']] == list(grads)
        assert abs(loss.item() - float(g[pre + 'loss'])) <= 1e-5 * abs(float(g[pre + 'loss'])), (i, loss.item(), float(g[pre + 'loss']))
        for k, v in grads.items():
            got = v.numpy()[::step] if k == 'dense.0.weight' else v.numpy()
            ref = g[pre + 'grad_' + k]
            assert got.shape == ref.shape, k
            assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max(), (i, k, float(np.abs(got - ref).max()), float(np.abs(ref).max()))
