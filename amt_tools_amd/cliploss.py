"""
Validation losses summed per clip, over a frame window of each clip (include/amtx_cliploss.h, csrc/cliploss.hip).

    bce_sums(logits, labels, weight=None, frames=None)                                      LogisticBank.get_loss without its means
    softmax_groups_sums(logits, targets, num_groups, num_classes, weight=None, frames=None)  SoftmaxGroups.get_loss without its means

Both return (B,) float64 SUMS: sums[b] / count_b is the reference's loss of clip b as a batch of one over its window's frames, and the sums
of the clips a track was cut into, over windows that keep every frame of the track once, add up to L_t times the loss of the segment-wise
logits of the whole track.  `frames`: a (B, 2) integer array-like {first, count} per clip, or None for whole clips.

Device tensors go to the kernels (no fallback: a missing library raises); host arrays and CPU tensors go to a float64 restatement of the
same sums in NumPy -- the oracle the kernels are tested against, and what a CPU model computes.  No gradient either way.  Models and
loops call the two functions by module attribute (`cliploss.bce_sums(...)`).
"""
import numpy as np

from . import _lib

__all__ = ['bce_sums', 'softmax_groups_sums', 'checked_frames', 'Windows']


class Windows(object):
    """A window table that travels with its device copy: `table`, the (B, 2) integer host array {first, count}, and `dev`, the same
    rows as an int32 tensor on the device the kernels run on (uploaded by whoever staged the batch: the validation loops put it on the
    way beside the batch's other uploads, so that no head's launch has to wait for a copy of its own).  Anything else handed over as
    `frames` is uploaded by the call that reads it."""

    def __init__(self, table, dev=None):
        self.table, self.dev = np.asarray(table), dev


def checked_frames(frames, batch, num_frames):
    """`frames` (an array-like, a tensor or a Windows) as a contiguous (batch, 2) int32 host array {first, count}, or None for None.
    ValueError, naming the clip, for a row with a negative entry or first + count > num_frames; for a wrong shape or a table that does
    not hold integers."""
    if frames is None:
        return None
    if isinstance(frames, Windows):
        frames = frames.table
    if hasattr(frames, 'detach'):
        frames = frames.detach().cpu().numpy()
    table = np.asarray(frames)
    if table.dtype.kind not in 'iu':
        raise ValueError(f'frames: an integer table, not {table.dtype}')
    if table.shape != (batch, 2):
        raise ValueError(f'frames: a ({batch}, 2) table of (first, count) for {batch} clips, not {tuple(table.shape)}')
    table = table.astype(np.int64)
    negative, beyond = (table < 0).any(axis=1), table.sum(axis=1) > num_frames
    if negative.any() or beyond.any():
        b = int(np.flatnonzero(negative | beyond)[0])
        first, count = table[b].tolist()
        if negative[b]:
            raise ValueError(f'frames: clip {b}: a negative entry in the window ({first}, {count})')
        raise ValueError(f'frames: clip {b}: frames [{first}, {first} + {count}) leave the clip\'s {num_frames} frames')
    return np.ascontiguousarray(table, dtype=np.int32)


def _is_device(t):
    return hasattr(t, 'is_cuda') and t.is_cuda


def _host(t, dtype):
    if t is None:
        return None
    if hasattr(t, 'detach'):
        t = t.detach().cpu().numpy()
    return np.asarray(t).astype(dtype)


def _like(sums, logits):
    """The restatement's answer in the kind of its input: a CPU tensor for a tensor, else the array."""
    if hasattr(logits, 'detach'):
        import torch
        return torch.from_numpy(sums)
    return sums


def _rows(logits, width):
    """A device (B, T, >= width) fp32 tensor as the kernels read it: unit column stride, clips B rows apart -> (tensor, ld)."""
    import torch
    if logits.dtype != torch.float32:
        logits = logits.float()
    B, T = logits.shape[:2]
    if logits.stride(2) != 1 or logits.stride(1) < width or (B > 1 and logits.stride(0) != T * logits.stride(1)):
        logits = logits.contiguous()
    return logits, logits.stride(1)


def _launch(name, logits, ld, labels, weight, frames, table, sizes):
    import torch
    device = logits.device
    B = logits.shape[0]
    if weight is not None:
        weight = torch.as_tensor(weight).detach().to(device=device, dtype=torch.float32).contiguous()
    table_dev = None
    if table is not None:
        staged = frames.dev if isinstance(frames, Windows) else None
        if staged is not None and staged.device == device and staged.dtype == torch.int32 and tuple(staged.shape) == table.shape and staged.is_contiguous():
            table_dev = staged
        else:
            table_dev = torch.from_numpy(table).to(device)
    sums = torch.empty((B,), dtype=torch.float64, device=device)
    ws = _lib.alloc_workspace(int(_lib.call(name + '_workspace_bytes', *sizes)), device)
    _lib.call(name, logits, ld, labels, weight, table, table_dev, *sizes, sums, ws, ws.numel(), device=device)
    return sums


def bce_sums(logits, labels, weight=None, frames=None):
    """sums[b] = sum_k weight[k] * sum_{t in window b} BCEWithLogits(logits[b, t, k], labels[b, k, t]) as (B,) float64, each term in the
    form max(x, 0) - x y + log1p(exp(-|x|)).  logits (B, T, K); labels (B, K, T); weight (K,) or None; frames: see the module."""
    if logits.ndim != 3 or labels.ndim != 3 or tuple(labels.shape) != (logits.shape[0], logits.shape[2], logits.shape[1]):
        raise ValueError(f'logits (B, T, K) against labels (B, K, T): {tuple(logits.shape)} against {tuple(labels.shape)}')
    B, T, K = (int(n) for n in logits.shape)
    if weight is not None and int(np.prod(tuple(weight.shape))) != K:
        raise ValueError(f'weight: one per key ({K}), not {tuple(weight.shape)}')
    table = checked_frames(frames, B, T)
    if _is_device(logits):
        if B == 0 or T == 0:
            raise ValueError(f'logits {tuple(logits.shape)}: at least one clip and one frame')
        import torch
        x, ld = _rows(logits.detach(), K)
        y = labels.detach().to(device=x.device, dtype=torch.float32).contiguous()
        return _launch('amtx_bce_clip_sums', x, ld, y, weight, frames, table, (B, T, K))
    x, y, w = _host(logits, np.float64), _host(labels, np.float64), _host(weight, np.float64)
    sums = np.zeros(B, dtype=np.float64)
    for b in range(B):
        first, count = (0, T) if table is None else (int(table[b, 0]), int(table[b, 1]))
        xs = np.ascontiguousarray(x[b, first:first + count])                       # (count, K)
        ys = np.ascontiguousarray(y[b][:, first:first + count].T)
        term = np.maximum(xs, 0.0) - xs * ys + np.log1p(np.exp(-np.abs(xs)))
        if w is not None:
            term = term * w.reshape(1, K)
        sums[b] = term.sum()
    return _like(sums, logits)


def softmax_groups_sums(logits, targets, num_groups, num_classes, weight=None, frames=None):
    """sums[b] = sum_{t in window b} sum_g w[g][y] * (logsumexp_c logits[b, t, g C + c] - logits[b, t, g C + y]), y = targets[b, g, t] with
    -1 for the last class, as (B,) float64.  logits (B, T, >= G C): columns beyond G C are ignored; targets (B, G, T) integers; weight
    (G C,) or None.  A target outside [-1, C) inside a clip's window makes that clip's sum NaN, as amtx_softmax_groups_loss does."""
    G, Cn = int(num_groups), int(num_classes)
    if logits.ndim != 3 or targets.ndim != 3 or logits.shape[2] < G * Cn or tuple(targets.shape) != (logits.shape[0], G, logits.shape[1]):
        raise ValueError(f'logits (B, T, >= {G} x {Cn}) against targets (B, {G}, T): {tuple(logits.shape)} against {tuple(targets.shape)}')
    B, T = int(logits.shape[0]), int(logits.shape[1])
    if weight is not None and int(np.prod(tuple(weight.shape))) != G * Cn:
        raise ValueError(f'weight: one per group and class ({G * Cn}), not {tuple(weight.shape)}')
    table = checked_frames(frames, B, T)
    if _is_device(logits):
        if B == 0 or T == 0:
            raise ValueError(f'logits {tuple(logits.shape)}: at least one clip and one frame')
        import torch
        x, ld = _rows(logits.detach(), G * Cn)
        y = targets.detach().to(device=x.device, dtype=torch.int64).contiguous()
        return _launch('amtx_softmax_groups_clip_sums', x, ld, y, weight, frames, table, (B, T, G, Cn))
    x, y, w = _host(logits, np.float64), _host(targets, np.int64), _host(weight, np.float64)
    sums = np.zeros(B, dtype=np.float64)
    for b in range(B):
        first, count = (0, T) if table is None else (int(table[b, 0]), int(table[b, 1]))
        xs = np.ascontiguousarray(x[b, first:first + count, :G * Cn]).reshape(count, G, Cn)
        ys = np.ascontiguousarray(y[b][:, first:first + count].T)                  # (count, G)
        ys = np.where(ys == -1, Cn - 1, ys)
        bad = (ys < 0) | (ys >= Cn)
        ys = np.where(bad, 0, ys)
        top = xs.max(axis=-1, keepdims=True) if count else xs[..., :1]
        nll = top[..., 0] + np.log(np.exp(xs - top).sum(axis=-1)) - np.take_along_axis(xs, ys[..., None], axis=-1)[..., 0]
        scale = np.ones((count, G)) if w is None else w.reshape(G, Cn)[np.arange(G)[None, :], ys]
        scale = np.where(bad, np.nan, scale)
        sums[b] = (scale * nll).sum()
    return _like(sums, logits)
