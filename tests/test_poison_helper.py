"""The poisoning helper of tests/test_gpu_poison.py on a machine without a GPU: the torch.empty wrapper (device filter lifted) fills whole
storages, is undone with its monkeypatch, and leaves the guard bands of _lib.alloc_workspace intact."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from amt_tools_amd import _lib                                   # noqa: E402
from poison import PATTERNS, Poison, assert_same, fill_storage, first_difference, refill, snapshot   # noqa: E402


def _bytes(t):
    st = t.untyped_storage()
    return torch.empty(0, dtype=torch.uint8).set_(st, 0, (st.nbytes(),)).numpy()


def test_patterns_mean_what_the_cases_rely_on():
    assert PATTERNS == (0x00, 0xFF, 0x7F)
    ff, sf = np.full(4, 0xFF, np.uint8), np.full(4, 0x7F, np.uint8)
    assert np.isnan(ff.view(np.float32)[0]) and np.isnan(ff.view(np.float16)).all() and ff.view(np.int32)[0] == -1
    assert torch.isnan(torch.from_numpy(ff.copy()).view(torch.bfloat16).float()).all()
    assert np.isfinite(sf.view(np.float32)[0]) and sf.view(np.float32)[0] > 3.3e38 and np.isnan(sf.view(np.float16)).all()
    assert sf.view(np.int32)[0] == 2139062143
    assert torch.isfinite(torch.from_numpy(sf.copy()).view(torch.bfloat16).float()).all()


@pytest.mark.parametrize('pattern', PATTERNS)
def test_wrapper_fills_whole_storages_and_is_undone(pattern):
    real_empty, real_empty_like = torch.empty, torch.empty_like
    mp = pytest.MonkeyPatch()
    try:
        poison = Poison(mp, pattern, on=lambda t: True)          # the device filter lifted: CPU tensors stand in for GPU ones
        assert torch.empty is not real_empty and torch.empty_like is not real_empty_like
        dense = torch.empty((3, 5, 7), dtype=torch.float32)
        assert (_bytes(dense) == pattern).all() and _bytes(dense).size == 3 * 5 * 7 * 4
        cl = torch.empty((2, 3, 4, 5), dtype=torch.float32, memory_format=torch.channels_last)
        assert cl.is_contiguous(memory_format=torch.channels_last) and (_bytes(cl) == pattern).all()
        like = torch.empty_like(torch.zeros(2, 3, 4, 5), memory_format=torch.channels_last)
        assert (_bytes(like) == pattern).all()
        base = torch.empty((6, 10), dtype=torch.int32)
        view = base[1:4, 2:5]                                    # a sliced view: its base's storage is filled, pad columns included
        assert (_bytes(view) == pattern).all() and _bytes(view).size == 6 * 10 * 4
        assert int(view[0, 0]) == {0x00: 0, 0xFF: -1, 0x7F: 2139062143}[pattern]
        half = torch.empty(8, dtype=torch.bfloat16, requires_grad=True)      # a leaf that wants a gradient is filled without an autograd error
        assert (_bytes(half) == pattern).all()
        assert poison.filled == 5
        poison.pattern = 0x11                                    # the pattern may change while the wrapper lives
        assert (_bytes(torch.empty(9, dtype=torch.uint8)) == 0x11).all()
    finally:
        mp.undo()
    assert torch.empty is real_empty and torch.empty_like is real_empty_like


def test_default_filter_leaves_cpu_and_pinned_tensors_alone(monkeypatch):
    poison = Poison(monkeypatch, 0xFF)
    t = torch.zeros(16)
    e = torch.empty_like(t)
    e.copy_(t)
    torch.empty(16)
    assert poison.filled == 0


@pytest.mark.parametrize('pattern', PATTERNS)
def test_guard_bands_survive_both_kinds_of_poisoning(monkeypatch, pattern):
    monkeypatch.setattr(_lib, 'GUARD_BYTES', 256)
    Poison(monkeypatch, pattern, on=lambda t: True)
    ws = _lib.alloc_workspace(1000, 'cpu')                       # allocation poisoned as a whole, the bands stamped after it
    assert ws._base is not None and ws.numel() == 1000 and (ws == pattern).all()
    assert _lib.guards_intact(ws)
    refill(ws, 0x7F if pattern != 0x7F else 0xFF)                # between calls: the view only
    assert _lib.guards_intact(ws) and (ws != pattern).all()
    fill_storage(ws, pattern)                                    # (the whole storage WOULD take the bands with it: refill is the tool for workspaces)
    assert not _lib.guards_intact(ws) or pattern == _lib._GUARD_PATTERN


def test_comparison_is_bitwise_and_rejects_non_finite_values():
    a = {'x': torch.tensor([1.0, -0.0, 3.0]), 'n': [np.arange(3), 2.5], 's': torch.tensor(1.5)}
    assert first_difference(snapshot(a), snapshot(a)) is None
    b = {'x': torch.tensor([1.0, 0.0, 3.0]), 'n': [np.arange(3), 2.5], 's': torch.tensor(1.5)}
    assert '(1,)' in first_difference(snapshot(a), snapshot(b))  # -0.0 == 0.0 numerically, not bit for bit
    c = {'x': torch.tensor([1.0, float('nan'), 3.0]), 'n': [np.arange(3), 2.5], 's': torch.tensor(1.5)}
    assert 'non-finite' in first_difference(snapshot(c), snapshot(c))
    with pytest.raises(AssertionError):
        assert_same(snapshot(b), snapshot(a), 'case')
    assert first_difference(snapshot({'s': torch.tensor(1.5)}), snapshot({'s': torch.tensor(2.5)})) is not None
