"""Poisoned memory for the GPU suite (tests/test_gpu_poison.py): what a kernel reads from memory nobody initialised must not reach a result.

Two mechanisms, both filling with ONE byte repeated:
* `Poison(monkeypatch, pattern)` wraps `torch.empty` / `torch.empty_like` for the length of a test: the real function runs, then the WHOLE
  storage of a tensor on a GPU is filled through `untyped_storage()` (so channels-last and strided results are covered too).  That reaches
  every kernel workspace (`_lib.alloc_workspace` allocates with torch.empty and stamps its guard bands AFTER the fill, so they stay intact),
  the per-call scratch buffers and every output tensor the package allocates.  CPU and pinned tensors are left alone.
* `refill(ws, pattern)` fills a persistent, grow-only workspace in place before the next call: the view only, never its guard bands.

PATTERNS: 0x00 is what a first allocation from the driver reads as (the baseline the suite has without this file); 0xFF is NaN as fp32 /
bf16 / f16, -1 as an integer, 255 in a pool winner record; 0x7F is 3.39e38 as fp32 / bf16 (finite, huge), NaN as f16 and 2139062143 as
int32 (fatal as a stale count or index)."""
import numpy as np
import torch

PATTERNS = (0x00, 0xFF, 0x7F)


_REAL_EMPTY = torch.empty          # bound at import: fill_storage must not go through a Poison wrapper


def fill_storage(t, pattern):
    """Every byte of `t`'s storage becomes `pattern` (not just the elements `t` views)."""
    st = t.untyped_storage()
    n = st.nbytes()
    if n:
        with torch.no_grad():
            _REAL_EMPTY(0, dtype=torch.uint8, device=t.device).set_(st, 0, (n,)).fill_(int(pattern))
    return t


def refill(ws, pattern):
    """A workspace from _lib.alloc_workspace (a view between two guard bands when GUARD_BYTES is set), filled in place."""
    if ws is not None and ws.numel():
        with torch.no_grad():
            ws.fill_(int(pattern))
    return ws


class Poison(object):
    """torch.empty / torch.empty_like return tensors whose storage holds `self.pattern` while the monkeypatch lives.  `on(tensor)` picks
    the tensors to fill (default: those on a GPU); `filled` counts them."""

    def __init__(self, monkeypatch, pattern=0x00, on=None):
        self.pattern = pattern
        self.filled = 0
        self.on = on if on is not None else (lambda t: t.is_cuda)
        real_empty, real_empty_like = torch.empty, torch.empty_like

        def _poisoned(t):
            if isinstance(t, torch.Tensor) and self.on(t) and t.untyped_storage().nbytes():
                fill_storage(t, self.pattern)
                self.filled += 1
            return t

        def empty(*args, **kwargs):
            return _poisoned(real_empty(*args, **kwargs))

        def empty_like(*args, **kwargs):
            return _poisoned(real_empty_like(*args, **kwargs))

        monkeypatch.setattr(torch, 'empty', empty)
        monkeypatch.setattr(torch, 'empty_like', empty_like)


def snapshot(obj):
    """What a public call returned, as host data that compares bit for bit: tensors -> numpy (NaN payloads kept), containers walked."""
    if isinstance(obj, torch.Tensor):
        return obj.detach().cpu().numpy().copy()
    if isinstance(obj, np.ndarray):
        return obj.copy()
    if isinstance(obj, dict):
        return {k: snapshot(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [snapshot(v) for v in obj]
    return obj


def first_difference(a, b, path=''):
    """None when two snapshots hold the same bits (shapes, dtypes, every byte) and no NaN / Inf; else a description of the first
    offending element -- the evidence a failing poison test starts from."""
    if isinstance(a, dict):
        if not isinstance(b, dict) or sorted(map(str, a)) != sorted(map(str, b)):
            return f'{path}: keys differ'
        for k in a:
            d = first_difference(a[k], b[k], f'{path}/{k}')
            if d:
                return d
        return None
    if isinstance(a, list):
        if not isinstance(b, list) or len(a) != len(b):
            return f'{path}: lengths differ'
        for i, (x, y) in enumerate(zip(a, b)):
            d = first_difference(x, y, f'{path}[{i}]')
            if d:
                return d
        return None
    if isinstance(a, np.ndarray):
        if not isinstance(b, np.ndarray) or a.shape != b.shape or a.dtype != b.dtype:
            return f'{path}: shape / dtype differ ({getattr(a, "shape", None)} {getattr(a, "dtype", None)} vs {getattr(b, "shape", None)} {getattr(b, "dtype", None)})'
        for name, arr in (('first', a), ('second', b)):
            if arr.dtype.kind == 'f' and not np.isfinite(arr).all():
                idx = np.argwhere(~np.isfinite(arr))[0]
                return f'{path}: {name} run holds {arr[tuple(idx)]} at {tuple(int(i) for i in idx)} ({int((~np.isfinite(arr)).sum())} of {arr.size} non-finite)'
        if a.tobytes() != b.tobytes():
            fa, fb = a.reshape(-1), b.reshape(-1)
            ne = fa.view(f'V{a.dtype.itemsize}') != fb.view(f'V{a.dtype.itemsize}') if a.size else np.zeros(0, bool)
            flat = int(np.argmax(ne))
            idx = np.unravel_index(flat, a.shape) if a.ndim else ()
            return (f'{path}: first difference at {tuple(int(i) for i in idx)}: {fa[flat]!r} vs {fb[flat]!r} '
                    f'({int(ne.sum())} of {a.size} elements differ)')
        return None
    return None if a == b or (a is None and b is None) else f'{path}: {a!r} vs {b!r}'


def assert_same(got, ref, what):
    d = first_difference(ref, got, '')
    assert d is None, f'{what}: {d}'
