"""CPU-side checks of the TabCNN engine: the amtx_tab_* C ABI's argument checks (no compute calls, no GPU needed) and the window-view
detection that decides which forward passes the engine may take."""
import ctypes as C

import numpy as np
import pytest
import torch

from amt_tools_amd import _lib, tools
from amt_tools_amd.models import TabCNN, tab_window_view
from amt_tools_amd.synth import tabcnn_state_dict_shapes

TAB_FUNCS = ('amtx_tab_model_create', 'amtx_tab_model_destroy', 'amtx_tab_model_set_tensor', 'amtx_tab_model_finalize',
             'amtx_tab_workspace_bytes', 'amtx_tab_forward')


def _create(dim_in=192, in_channels=1, mc=1, groups=6, classes=21, precision=1):
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.amtx_tab_model_create(C.byref(h), dim_in, in_channels, mc, groups, classes, precision)
    return rc, h


def test_tab_abi_is_exported():
    L = _lib.lib()
    declared = _lib.declared_symbols()
    for name in TAB_FUNCS:
        assert name in declared and name in _lib.signatures() and hasattr(L, name), name


@pytest.mark.parametrize('kwargs, word', [(dict(mc=2), b'model_complexity'), (dict(classes=33), b'num_classes'),
                                          (dict(in_channels=9), b'in_channels'), (dict(groups=9, classes=32), b'num_groups'),
                                          (dict(dim_in=4096), b'dim_in')])
def test_tab_unsupported_configurations(kwargs, word):
    rc, h = _create(**kwargs)
    assert rc == _lib.ERR_UNSUPPORTED and not h.value
    assert word in _lib.lib().amtx_last_error()


def test_tab_argument_errors():
    L = _lib.lib()
    for kwargs, word in ((dict(dim_in=8), b'dim_in'), (dict(precision=2), b'precision'), (dict(groups=0), b'dims')):
        rc, h = _create(**kwargs)
        assert rc < 0 and rc != _lib.ERR_UNSUPPORTED and not h.value, kwargs
        assert word in L.amtx_last_error()
    rc, h = _create(dim_in=145, in_channels=6)
    assert rc == 0 and h.value
    try:
        shapes = tabcnn_state_dict_shapes(dim_in=145, in_channels=6)
        ok = np.zeros(int(np.prod(shapes['conv.0.weight'])), dtype=np.float32)
        assert L.amtx_tab_model_set_tensor(h, b'conv.0.weight', _lib.ptr(ok), ok.size) == 0
        rc = L.amtx_tab_model_set_tensor(h, b'conv.1.weight', _lib.ptr(ok), ok.size)            # not a state_dict key
        assert rc < 0 and b'conv.1.weight' in L.amtx_last_error()
        rc = L.amtx_tab_model_set_tensor(h, b'conv.0.weight', _lib.ptr(ok), ok.size - 1)        # wrong element count
        assert rc < 0 and b'conv.0.weight' in L.amtx_last_error()
        fc = np.zeros(64 * 69 * 128 + 64, dtype=np.float32)
        rc = L.amtx_tab_model_set_tensor(h, b'dense.0.weight', _lib.ptr(fc), fc.size)            # dim_in 192's fc on a dim_in 145 model
        assert rc < 0
        rc = L.amtx_tab_model_finalize(h)                                                         # nine tensors never set
        assert rc < 0 and b'never set' in L.amtx_last_error()
        with pytest.raises(_lib.AmtxError):
            _lib.check(rc, 'amtx_tab_model_finalize')
        # forward on a model that was never finalized: refused before anything reaches a device
        rc = L.amtx_tab_forward(h, C.c_void_p(256), 0, 0, 0, 1, 1, 1, C.c_void_p(256), 1 << 20, C.c_void_p(256), None, None)
        assert rc < 0 and b'finalized' in L.amtx_last_error()
    finally:
        assert L.amtx_tab_model_destroy(h) == 0


def test_tab_workspace_is_monotone():
    L = _lib.lib()
    rc, h = _create()
    assert rc == 0
    try:
        assert L.amtx_tab_workspace_bytes(h, 0, 10) == 0 and L.amtx_tab_workspace_bytes(h, 1, 0) == 0
        prev_b = 0
        for b in (1, 2, 3, 7, 30):
            prev_t = 0
            for t in (1, 2, 8, 9, 63, 64, 65, 200, 1292):
                n = L.amtx_tab_workspace_bytes(h, b, t)
                assert n > prev_t and n % 256 == 0, (b, t)
                assert n >= L.amtx_tab_workspace_bytes(h, max(1, b - 1), t)
                prev_t = n
            assert prev_t > prev_b
            prev_b = prev_t
    finally:
        L.amtx_tab_model_destroy(h)


def _model(**kw):
    return TabCNN(kw.pop('dim_in', 192), tools.GuitarProfile(num_frets=19), kw.pop('in_channels', 1), 1, **kw)


@pytest.mark.parametrize('B, Cc, Fd, T', [(2, 1, 192, 30), (1, 6, 145, 1), (3, 1, 20, 64)])
def test_window_view_of_offline_pre_proc(B, Cc, Fd, T):
    model = _model(dim_in=Fd, in_channels=Cc)
    feats = torch.randn(B, Cc, Fd, T)
    win = model.pre_proc({tools.KEY_FEATS: feats})[tools.KEY_FEATS]
    v = tab_window_view(win)
    assert v is not None and v['num_windows'] == T and v['num_cols'] == T + 8
    assert v['offset'] == win.storage_offset() == 0                       # the padded sequence's first column
    sb, sc, sf, st = v['strides']
    seq = torch.as_strided(win, (B, Cc, Fd, T + 8), (sb, sc, sf, st), v['offset'])
    assert torch.equal(seq[..., 4:4 + T], feats) and not seq[..., :4].any() and not seq[..., T + 4:].any()
    for t in (0, T - 1):
        assert torch.equal(win[:, t], seq[..., t:t + 9])


@pytest.mark.parametrize('T_in', [5, 9, 40])
def test_window_view_of_online_pre_proc(T_in):
    model = _model(dim_in=24)
    model.toggle_online()
    feats = torch.randn(2, 1, 24, T_in)
    win = model.pre_proc({tools.KEY_FEATS: feats})[tools.KEY_FEATS]
    v = tab_window_view(win)
    T = max(1, T_in - 8)
    assert v is not None and v['num_windows'] == T == win.shape[1] and v['num_cols'] == T + 8
    # a slice of windows of an online view: a base offset of its own, the same strides
    if T > 3:
        part = win[:, 2:]
        vp = tab_window_view(part)
        assert vp['offset'] == 2 * v['strides'][3] and vp['num_cols'] == T - 2 + 8


def test_window_view_rejects():
    model = _model(dim_in=20)
    win = model.pre_proc({tools.KEY_FEATS: torch.randn(2, 1, 20, 12)})[tools.KEY_FEATS]
    assert tab_window_view(win) is not None
    assert tab_window_view(win.contiguous()) is None                    # a copy of the windows: T stride 9*C*F, W stride 1
    assert tab_window_view(win.double()) is None
    seq = torch.randn(2, 1, 20, 40)
    uneq = seq.unfold(-1, 9, 2).permute(0, 3, 1, 2, 4)                  # hop 2: T stride 2, W stride 1
    assert tab_window_view(uneq) is None
    store = torch.randn(2 * 20 * 20)
    inside = torch.as_strided(store, (2, 12, 1, 20, 9), (400, 1, 400, 20, 1))          # 20 columns per row: exactly T + 8
    assert tab_window_view(inside) is not None
    tail = torch.as_strided(store, (1, 4, 1, 20, 9), (400, 1, 400, 20, 1), 408)        # columns 8 .. 19 of the second clip
    assert tab_window_view(tail)['offset'] == 408
    # a view whose T + 8 columns leave its storage (the storage shrank under it): never handed to the engine
    short = torch.randn(2, 1, 20, 20)
    win2 = torch.as_strided(short, (2, 12, 1, 20, 9), (400, 1, 400, 20, 1))
    assert tab_window_view(win2) is not None
    short.untyped_storage().resize_(4 * (2 * 400 - 1))
    assert tab_window_view(win2) is None


def test_cpu_path_unchanged_and_precision_keyword():
    profile = tools.GuitarProfile(num_frets=19)
    m = TabCNN(40, profile, 1, 1, 'cpu', 'bf16')                          # positional device, then the new keyword
    assert m.precision == 'bf16' and TabCNN(40, profile).precision == 'x3'
    with pytest.raises(AssertionError):
        TabCNN(40, profile, precision='f32')
    m.eval()
    with torch.no_grad():
        out = m.run_on_batch({tools.KEY_FEATS: torch.randn(1, 1, 40, 11)})
    assert out[tools.KEY_TABLATURE].shape == (1, 6, 11) and '_engine' not in m.__dict__
    assert TabCNN(40, profile, 1, 2).engine_unsupported().startswith('model_complexity')
    assert 'num_classes' in TabCNN(40, tools.GuitarProfile(num_frets=40)).engine_unsupported()
    assert TabCNN(40, tools.GuitarProfile(num_frets=22)).engine_unsupported() is None
