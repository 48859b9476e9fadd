"""
Evaluation: the evaluator classes of amt_tools/evaluate.py (constructor arguments, result-dictionary layout and keys; `train()` takes them
unchanged: process_track / average_results / reset_results / finalize(writer, step) / set_save_dir / set_patterns / set_verbose), and a
batched validation loop that scores a partition on the device: validate_batched for host clips and references, validate_clips for clips
of device-resident tracks (tracks.TrackBank / PyramidBank, LabelBank, NoteBank), validate_tracks for those tracks whole, one result per
track, stitched from overlapped clips; sweep_tracks for a grid of onset and frame thresholds over those tracks in one pass of the model.

Every evaluator is split in two:

* counting -- `counts(estimated, reference)` on host arrays (the reference's own float64 expressions, evaluate.py:815-829, :1246-1281,
  :1331-1334) or `counts_batch(estimated, reference)` on device tensors (ONE C-ABI call into csrc/eval.hip, a whole batch), and
* `results_from_counts(counts)` -- the arithmetic from those few numbers to precision / recall / f-measure / tdr / accuracy.  Both paths end
  in it, so they cannot disagree on the arithmetic.  (stage_batch / enqueue_batch / results_batch: its part in validate_batched.)

Note matching restates mir_eval.transcription.match_notes (mir_eval is not required): see `note_edges`.  UNPINNED: the rules -- non-strict
comparisons, 0.05 s onset tolerance, 50 cents, 0.05 s minimum offset tolerance, distances rounded to N_DECIMALS before they are compared --
are written down from the published behaviour, not checked against mir_eval's source; N_DECIMALS in particular.

Not here: PitchListEvaluator / StackedPitchListEvaluator (they rest on mir_eval.multipitch's resampling) and run_online.
"""
import json
import os
import sys
import warnings
from collections import namedtuple
from copy import deepcopy

import numpy as np

from . import tools
from .inference import run_offline

__all__ = ['validate', 'validate_batched', 'validate_clips', 'validate_tracks', 'sweep_tracks', 'multipitch_grid_counts', 'average_results', 'append_results', 'log_results', 'write_results', 'pattern_match',
           'Evaluator',
           'ComboEvaluator', 'LossWrapper', 'StackedMultipitchEvaluator', 'MultipitchEvaluator', 'StackedNoteEvaluator', 'NoteEvaluator',
           'TablatureEvaluator', 'SoftmaxAccuracy', 'note_edges', 'match_notes_count', 'N_DECIMALS']

EPSILON = sys.float_info.epsilon
N_DECIMALS = 4                 # decimals the note distances are rounded to before they meet a tolerance (UNPINNED, see above); the kernel takes it
ONSET_TOLERANCE = 0.05         # seconds
PITCH_TOLERANCE = 50.0         # cents
OFFSET_MIN_TOLERANCE = 0.05    # seconds


# ------------------------------------------------------------------------------------------------------------------------------
# the loops
# ------------------------------------------------------------------------------------------------------------------------------
def validate(model, dataset, evaluator, estimator=None, online=False):
    """One track at a time (amt_tools/evaluate.py:52-101): run_offline, then evaluator.process_track.  Returns the averaged results."""
    import torch
    if online:
        raise NotImplementedError('run_online is not part of this package')
    with torch.no_grad():
        for track_id in dataset.tracks:
            track_data = dataset.get_track_data(track_id)
            model.eval()                       # per track, as in the reference: a model may reset state there
            predictions = run_offline(track_data, model, estimator)
            evaluator.process_track(predictions, track_data, track_id)
    return evaluator.average_results()


# ------------------------------------------------------------------------------------------------------------------------------
# results dictionaries
# ------------------------------------------------------------------------------------------------------------------------------
def average_results(results):
    """A copy in which every ndarray / list leaf is its mean as a float (nested dictionaries walked, other leaves kept)."""
    out = deepcopy(results)
    for key, entry in out.items():
        if isinstance(entry, dict):
            out[key] = average_results(entry)
        elif isinstance(entry, (np.ndarray, list)):
            out[key] = float(np.mean(entry))
    return out


def append_results(tracked_results, new_results):
    """A copy of `tracked_results` with the leaves of `new_results` appended (np.append) under their keys; unknown keys are taken over."""
    out = deepcopy(tracked_results)
    for key, entry in new_results.items():
        if key not in out:
            out[key] = entry
        elif isinstance(entry, dict):
            out[key] = append_results(out[key], entry)
        else:
            out[key] = np.append(out[key], entry)
    return out


def pattern_match(query, patterns=None):
    """Whether some pattern is a substring of `query` (no patterns: False)."""
    return patterns is not None and any(p in query for p in patterns)


def log_results(results, writer, step=0, patterns=None, tag='', prnt=False):
    """writer.add_scalar(f'{tag}/{key}', value, global_step=step) for every leaf whose key matches (all when patterns is None); nested
    dictionaries extend the tag.  As in the reference, `prnt` is not handed down to nested dictionaries."""
    for key, entry in results.items():
        if isinstance(entry, dict):
            log_results(entry, writer, step, patterns, f'{tag}/{key}')
        elif patterns is None or pattern_match(key, patterns):
            writer.add_scalar(f'{tag}/{key}', entry, global_step=step)
            if prnt:
                print(json.dumps({'iter': step, f'{tag}/{key}': entry}))


def _write_line(file, text, verbose):
    file.write(text + '\n')
    if verbose:
        print(text)


def write_results(results, file, patterns=None, verbose=False):
    """Text form: '-----key-----' headers for nested dictionaries, ' key : value' lines, blank lines between blocks."""
    for key, entry in results.items():
        if isinstance(entry, dict):
            _write_line(file, f'-----{key}-----', verbose)
            write_results(entry, file, patterns, verbose)
            _write_line(file, '', verbose)
        elif patterns is None or pattern_match(key, patterns):
            _write_line(file, f' {key} : {entry}', verbose)
    _write_line(file, '', verbose)


def _f_measure(precision, recall):
    """mir_eval.util.f_measure with beta = 1: 2 p r / (p + r), 0 when both are 0."""
    if precision == 0 and recall == 0:
        return 0.0
    return 2 * precision * recall / (precision + recall)


def _hmean_f1(precision, recall):
    """hmean([p + EPSILON, r + EPSILON]) - EPSILON (evaluate.py:836): the harmonic mean of two numbers is 2 / (1 / a + 1 / b)."""
    return 2.0 / (1.0 / (precision + EPSILON) + 1.0 / (recall + EPSILON)) - EPSILON


# ------------------------------------------------------------------------------------------------------------------------------
# note matching (host)
# ------------------------------------------------------------------------------------------------------------------------------
def _midi_to_hz(pitches):
    return 440.0 * 2.0 ** ((np.asarray(pitches, dtype=np.float64) - 69.0) / 12.0)


def note_edges(est_pitches, est_intervals, ref_pitches, ref_intervals, offset_ratio=None, onset_tolerance=ONSET_TOLERANCE,
               pitch_tolerance=PITCH_TOLERANCE, offset_min_tolerance=OFFSET_MIN_TOLERANCE):
    """(num_ref, num_est) boolean matrix: which reference note may be matched with which estimated note.  In float64, every distance rounded
    with np.around(., N_DECIMALS) before the non-strict comparison:
      onsets   |on_ref - on_est| <= onset_tolerance
      pitches  |1200 (log2 f_ref - log2 f_est)| <= pitch_tolerance (MIDI pitches, converted to Hertz; integral pitches: equal pitch)
      offsets  (offset_ratio given) |off_ref - off_est| <= max(offset_min_tolerance, offset_ratio * (off_ref - on_ref))"""
    est_intervals = np.asarray(est_intervals, dtype=np.float64).reshape(-1, 2)
    ref_intervals = np.asarray(ref_intervals, dtype=np.float64).reshape(-1, 2)
    onset = np.around(np.abs(ref_intervals[:, None, 0] - est_intervals[None, :, 0]), N_DECIMALS) <= onset_tolerance
    cents = np.abs(1200.0 * (np.log2(_midi_to_hz(ref_pitches))[:, None] - np.log2(_midi_to_hz(est_pitches))[None, :]))
    edges = onset & (np.around(cents, N_DECIMALS) <= pitch_tolerance)
    if offset_ratio is not None:
        tol = np.maximum(offset_min_tolerance, offset_ratio * (ref_intervals[:, 1] - ref_intervals[:, 0]))
        edges &= np.around(np.abs(ref_intervals[:, None, 1] - est_intervals[None, :, 1]), N_DECIMALS) <= tol[:, None]
    return edges


def _max_matching(edges):
    """Size of a maximum matching of a boolean biadjacency matrix."""
    if edges.size == 0 or not edges.any():
        return 0
    try:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import maximum_bipartite_matching
        return int((maximum_bipartite_matching(csr_matrix(edges), perm_type='column') >= 0).sum())
    except ImportError:
        pass
    adj = [np.flatnonzero(row) for row in edges]
    owner = [-1] * edges.shape[1]                 # column -> row
    size = 0
    for root in range(len(adj)):
        seen, stack, cursor, via = set(), [root], {root: 0}, {}
        while stack:
            u = stack[-1]
            if cursor[u] == len(adj[u]):
                stack.pop()
                continue
            j = int(adj[u][cursor[u]])
            cursor[u] += 1
            if j in seen:
                continue
            seen.add(j)
            via[u] = j
            if owner[j] < 0:
                for w in stack:
                    owner[via[w]] = w
                size += 1
                break
            stack.append(owner[j])
            cursor[owner[j]] = 0
    return size


def match_notes_count(est_pitches, est_intervals, ref_pitches, ref_intervals, offset_ratio=None):
    """Size of a maximum matching of estimated to reference notes under note_edges' rules."""
    if len(est_pitches) == 0 or len(ref_pitches) == 0:
        return 0
    return _max_matching(note_edges(est_pitches, est_intervals, ref_pitches, ref_intervals, offset_ratio))


# ------------------------------------------------------------------------------------------------------------------------------
# evaluators
# ------------------------------------------------------------------------------------------------------------------------------
class Evaluator(object):
    """What all evaluators share (amt_tools/evaluate.py:288-533)."""

    def __init__(self, unpack_key=None, results_key=None, save_dir=None, patterns=None, verbose=False):
        self.unpack_key = self.get_default_key() if unpack_key is None else unpack_key
        self.results_key = self.get_default_key() if results_key is None else results_key
        self.save_dir = None
        self.set_save_dir(save_dir)
        self.patterns = None
        self.set_patterns(patterns)
        self.verbose = None
        self.set_verbose(verbose)
        self.results = None
        self.reset_results()

    def set_save_dir(self, save_dir):
        self.save_dir = save_dir
        if save_dir is not None:
            os.makedirs(save_dir, exist_ok=True)

    def set_patterns(self, patterns):
        self.patterns = patterns

    def set_verbose(self, verbose):
        self.verbose = verbose

    def reset_results(self):
        self.results = dict()

    def average_results(self):
        return average_results(self.results)

    @staticmethod
    def get_default_key():
        return NotImplementedError

    def unpack(self, estimated, reference):
        estimated = tools.unpack_dict(estimated, self.unpack_key)
        reference = tools.unpack_dict(reference, self.unpack_key)
        if estimated is None:
            warnings.warn(f'Entry for key \'{self.unpack_key}\' not found in estimates.', category=RuntimeWarning)
        if reference is None:
            warnings.warn(f'Entry for key \'{self.unpack_key}\' not found in ground-truth.', category=RuntimeWarning)
        return estimated, reference

    def evaluate(self, estimated, reference):
        return NotImplementedError

    def write(self, results, track=None):
        if self.save_dir is None:
            return
        tag = tools.get_tag(track)
        if self.verbose:
            print(f'Evaluating track: {tag}')
        path = os.path.join(self.save_dir, f'{tag}.{tools.TXT_EXT}')
        os.makedirs(os.path.dirname(path), exist_ok=True)       # a track name may contain directories
        with open(path, 'w') as f:
            write_results(results, f, self.patterns, self.verbose)

    def track_results(self, results, track=None):
        """Second half of process_track: append one track's results and write them.  validate_batched enters here."""
        self.results = append_results(self.results, results)
        self.write(results, track)
        return results

    def process_track(self, estimated, reference, track=None):
        return self.track_results(self.evaluate(*self.unpack(estimated, reference)), track)

    # The three moments of a batch in validate_batched (`batch`: its _Batch).  Here: what the map and tablature evaluators share
    reference_dtype = np.float32

    def stage_batch(self, refs, batch):
        """The clips' unpacked references on their way to the device; what comes back is handed to the other two as `staged`."""
        return batch.upload(np.stack([np.asarray(r) for r in refs]).astype(self.reference_dtype))

    def enqueue_batch(self, staged, batch):
        """Enqueue the counting on the model's stream -> tuple of device tensors to bring to the host."""
        raise NotImplementedError(f'{type(self).__name__} has no batched counting')

    def results_batch(self, staged, counts, batch):
        """What enqueue_batch returned, as host arrays -> one results dictionary per clip."""
        return [self.results_from_counts(c) for c in counts[0]]

    def finalize(self, writer, step=0):
        log_results(self.average_results(), writer, step, patterns=self.patterns, tag=tools.VAL)
        self.reset_results()


class ComboEvaluator(Evaluator):
    """Several evaluators as one (amt_tools/evaluate.py:535-662): each keeps its own results; one file per track for all of them."""

    def __init__(self, evaluators, save_dir=None, patterns=None, verbose=False):
        self.evaluators = evaluators
        super().__init__(None, None, save_dir, patterns, verbose)

    def reset_results(self):
        for evaluator in self.evaluators:
            evaluator.reset_results()

    @staticmethod
    def _merge(into, key, results):
        if tools.query_dict(into, key):
            into[key].update(results)
        else:
            into[key] = results

    def average_results(self):
        average = dict()
        for evaluator in self.evaluators:
            self._merge(average, evaluator.results_key, average_results(evaluator.results))
        return average

    def unpack(self, estimated, reference):
        return NotImplementedError

    def track_results(self, results, track=None):
        """`results`: one results dictionary per evaluator, in order."""
        merged = dict()
        for evaluator, new in zip(self.evaluators, results):
            self._merge(merged, evaluator.results_key, new)
            evaluator.results = append_results(evaluator.results, new)
        self.write(merged, track)
        return merged

    def process_track(self, estimated, reference, track=None):
        return self.track_results([e.evaluate(*e.unpack(estimated, reference)) for e in self.evaluators], track)


class LossWrapper(Evaluator):
    """Tracks the loss dictionary of the predictions (amt_tools/evaluate.py:665-725)."""

    @staticmethod
    def get_default_key():
        return tools.KEY_LOSS

    def unpack(self, estimated, reference=None):
        loss = tools.unpack_dict(estimated, self.unpack_key)
        if loss is None:
            warnings.warn(f'Entry for key \'{self.unpack_key}\' not found in estimates.', category=RuntimeWarning)
        return loss, None

    def evaluate(self, estimated, reference=None):
        return estimated

    # By default an eval-mode batch carries no loss: nothing to stage or count, unpack()'s warning and an empty dictionary per clip.
    # With losses=True the loops run the model labelled with tools.KEY_LOSS_FRAMES: its per-clip float64 sums (batch.preds) are the
    # "counts" that come back, and a clip's dictionary is {loss key: sum / frames} -- the loss of that clip as a batch of one.
    # validate_tracks adds the sums up per track itself and hands over finished dictionaries (batch.loss_results).
    def stage_batch(self, refs, batch):
        return None

    def enqueue_batch(self, staged, batch):
        if batch.loss_counts is None:
            return ()
        loss = tools.unpack_dict(batch.preds, self.unpack_key)
        if not isinstance(loss, dict):
            raise KeyError(f'the model output has no per-clip losses under \'{self.unpack_key}\'')
        batch.loss_keys = list(loss.keys())
        return tuple(loss.values())

    def results_batch(self, staged, counts, batch):
        if batch.loss_results is not None:
            return batch.loss_results
        if batch.loss_counts is None:
            warnings.warn(f'Entry for key \'{self.unpack_key}\' not found in estimates.', category=RuntimeWarning)
            return [dict() for _ in batch.idx]
        frames = np.asarray(batch.loss_counts, dtype=np.float64)
        return [{key: np.float64(sums[j]) / frames[j] for key, sums in zip(batch.loss_keys, counts)} for j in range(len(batch.idx))]


class StackedEvaluator(Evaluator):
    def __init__(self, average_slices=False, unpack_key=None, results_key=None, save_dir=None, patterns=None, verbose=False):
        super().__init__(unpack_key, results_key, save_dir, patterns, verbose)
        self.average_slices = average_slices

    @staticmethod
    def average_slice_results(_results):
        results = dict()
        for key in _results.keys():
            results = append_results(results, _results[key])
        return average_results(results)

    def _per_slice(self, keys, rows):
        results = dict(zip(keys, rows))
        return self.average_slice_results(results) if self.average_slices else results


class StackedMultipitchEvaluator(StackedEvaluator):
    """Frame-level precision / recall / f-measure per slice of a stacked multi-pitch map (amt_tools/evaluate.py:780-855)."""

    @staticmethod
    def get_default_key():
        return tools.KEY_MULTIPITCH

    @staticmethod
    def counts(estimated, reference):
        """(S, K, T) host maps -> (S, 3) float64: sum(est * ref), sum(est), sum(ref) over each slice."""
        shape = estimated.shape[:-2] + (-1,)
        est, ref = np.reshape(estimated, shape), np.reshape(reference, shape)
        return np.stack([np.sum(est * ref, axis=-1), np.sum(est, axis=-1), np.sum(ref, axis=-1)], axis=-1)

    def counts_batch(self, estimated, reference):
        """(B, S, K, T) or (B, K, T) fp32 device tensors holding 0 / 1 -> (B, S, 3) int64 device tensor (amtx_eval_multipitch_counts)."""
        import torch
        from . import _lib
        assert estimated.is_cuda and reference.is_cuda and estimated.shape == reference.shape and estimated.dim() in (3, 4)
        est, ref = estimated.contiguous().float(), reference.contiguous().float()
        B, S = est.shape[0], (est.shape[1] if est.dim() == 4 else 1)
        K, T = est.shape[-2:]
        counts = torch.empty((B, S, 3), dtype=torch.int64, device=est.device)
        _lib.call('amtx_eval_multipitch_counts', est, ref, B, S, K, T, counts, device=est.device)
        return counts

    def enqueue_batch(self, staged, batch):
        return (self.counts_batch(batch.est_map(self.unpack_key, stacked=staged.dim() == 4), staged),)

    def results_from_counts(self, counts):
        """(S, 3) counts of one clip -> its results dictionary."""
        counts = np.asarray(counts, dtype=np.float64)
        num_correct, num_predicted, num_ground_truth = counts[..., 0], counts[..., 1], counts[..., 2]
        precision = num_correct / (num_predicted + EPSILON)
        recall = num_correct / (num_ground_truth + EPSILON)
        f_measure = _hmean_f1(precision, recall)
        keys = list(range(len(f_measure)))
        return self._per_slice(keys, [{tools.KEY_PRECISION: precision[s], tools.KEY_RECALL: recall[s], tools.KEY_F1: f_measure[s]} for s in keys])

    def evaluate(self, estimated, reference):
        return self.results_from_counts(self.counts(np.asarray(estimated), np.asarray(reference)))


class MultipitchEvaluator(StackedMultipitchEvaluator):
    """The same for one (K, T) map: a stack of one slice, averaged away (amt_tools/evaluate.py:858-903)."""

    def __init__(self, unpack_key=None, results_key=None, save_dir=None, patterns=None, verbose=False):
        super().__init__(True, unpack_key, results_key, save_dir, patterns, verbose)

    def evaluate(self, estimated, reference):
        return super().evaluate(np.expand_dims(estimated, axis=-3), np.expand_dims(reference, axis=-3))


MAX_GRID_THRESHOLDS = 32       # thresholds per axis of a sweep (amtx_eval_multipitch_grid_counts)


def multipitch_grid_counts(prob, ref, thresholds):
    """(B, K, T) probability maps and reference maps, (G,) thresholds -> (B, G, 3) int64: per clip and threshold the cells active in
    both maps, in the estimate cut at the threshold (`prob < thr ? 0 : 1`: equality and NaN are active) and in the reference -- the
    three sums of MultipitchEvaluator on the roll cut at that threshold.  Device tensors: one call of amtx_eval_multipitch_grid_counts,
    one pass over the maps, a device tensor comes back.  Host arrays / CPU tensors: NumPy, an array comes back."""
    import torch
    if torch.is_tensor(prob) and prob.is_cuda:
        from . import _lib
        assert ref.is_cuda and prob.shape == ref.shape and prob.dim() == 3
        est, ref = prob.contiguous().float(), ref.contiguous().float()
        thr = torch.as_tensor(thresholds, dtype=torch.float32).reshape(-1).to(est.device)
        B, K, T = est.shape
        counts = torch.empty((B, thr.numel(), 3), dtype=torch.int64, device=est.device)
        _lib.call('amtx_eval_multipitch_grid_counts', est, ref, B, K, T, thr, thr.numel(), counts, device=est.device)
        return counts
    prob, ref = np.asarray(prob, dtype=np.float32), np.asarray(ref) != 0
    thr = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    assert prob.shape == ref.shape and prob.ndim == 3 and 1 <= len(thr) <= MAX_GRID_THRESHOLDS
    out = np.zeros((prob.shape[0], len(thr), 3), dtype=np.int64)
    for g, t in enumerate(thr):
        est = ~(prob < t)                          # not `prob >= t`: a NaN is active, as on the device
        out[:, g, 0], out[:, g, 1], out[:, g, 2] = (est & ref).sum(axis=(1, 2)), est.sum(axis=(1, 2)), ref.sum(axis=(1, 2))
    return out


def _sort_rows(rows):
    """Note rows in (pitch, onset) order."""
    return rows[np.lexsort((rows[:, 0], rows[:, 2]))] if len(rows) else rows.reshape(0, 3)


def _stacked_rows(stacked_notes):
    """{slice: (pitches, intervals)} -> list of (N, 3) float64 row arrays, one per slice in the dictionary's order."""
    return [np.concatenate([np.asarray(iv, dtype=np.float64).reshape(-1, 2), np.asarray(p, dtype=np.float64).reshape(-1, 1)], axis=-1)
            for p, iv in stacked_notes.values()]


class StackedNoteEvaluator(StackedEvaluator):
    """Note-level precision / recall / f-measure per slice of stacked notes (amt_tools/evaluate.py:906-987): a maximum matching under
    note_edges' rules; offset_ratio None = onsets only."""

    def __init__(self, offset_ratio=None, average_slices=False, unpack_key=None, results_key=None, save_dir=None, patterns=None, verbose=False):
        super().__init__(average_slices, unpack_key, results_key, save_dir, patterns, verbose)
        self.offset_ratio = offset_ratio

    @staticmethod
    def get_default_key():
        return tools.KEY_NOTES

    def counts(self, estimated, reference):
        """Stacked notes -> (S, 3) int64: matched, estimated, reference notes per slice (slices paired by position, as in the reference)."""
        est, ref = list(estimated.values()), list(reference.values())
        out = np.zeros((len(ref), 3), dtype=np.int64)
        for k in range(len(ref)):
            (pe, ie), (pr, ir) = est[k], ref[k]
            out[k] = match_notes_count(pe, ie, pr, ir, self.offset_ratio), len(pe), len(pr)
        return out

    def counts_batch(self, estimated, reference):
        """estimated, reference: (rows (N, 3) float64 device tensor, offsets (G + 1,) int32 device tensor), rows of one pitch in ascending
        onset order within a group -> (G, 3) int32 device tensor: matched, estimated, reference notes per group (amtx_eval_notes_match).
        matched < 0: the kernel refused the group (_lib.ERR_UNSUPPORTED: beyond its candidate window; -1: a fractional pitch)."""
        return self.match_batch(estimated, reference)[0]

    def match_batch(self, estimated, reference):
        """counts_batch with the call's status word: ((G, 3) counts, (1,) int32 device tensor: 0, or the first of -1 (a fractional pitch)
        and _lib.ERR_UNSUPPORTED that any group answered).  One int tells a caller whether any count has to be looked at."""
        import torch
        from . import _lib
        (er, eo), (rr, ro) = estimated, reference
        assert er.is_cuda and er.dtype == rr.dtype == torch.float64 and eo.dtype == ro.dtype == torch.int32 and eo.shape == ro.shape
        er, rr, eo, ro = er.contiguous(), rr.contiguous(), eo.contiguous(), ro.contiguous()
        dev, G = er.device, eo.shape[0] - 1
        ws = _lib.alloc_workspace(int(_lib.call('amtx_eval_notes_match_workspace_bytes', er.shape[0], rr.shape[0])), dev)
        counts = torch.empty((G, 3), dtype=torch.int32, device=dev)
        matched = torch.empty((G + 1,), dtype=torch.int32, device=dev)       # the last word: the call's status
        ratio = -1.0 if self.offset_ratio is None else float(self.offset_ratio)
        _lib.call('amtx_eval_notes_match', er, eo, er.shape[0], rr, ro, rr.shape[0], G, ONSET_TOLERANCE, ratio, OFFSET_MIN_TOLERANCE, N_DECIMALS,
                  ws, ws.numel(), matched, matched[G:], 0, device=dev)
        counts[:, 0] = matched[:G]
        counts[:, 1] = eo[1:] - eo[:-1]
        counts[:, 2] = ro[1:] - ro[:-1]
        return counts, matched[G:]

    def results_from_counts(self, counts, keys=None):
        """(S, 3) counts of one clip -> its results dictionary.  Either side empty: all zero, as mir_eval answers."""
        rows = []
        for matched, num_est, num_ref in np.asarray(counts).reshape(-1, 3).tolist():
            if num_est == 0 or num_ref == 0:
                p = r = f = 0.0
            else:
                p, r = float(matched) / num_est, float(matched) / num_ref
                f = _f_measure(p, r)
            rows.append({tools.KEY_PRECISION: p, tools.KEY_RECALL: r, tools.KEY_F1: f})
        return self._per_slice(list(range(len(rows))) if keys is None else keys, rows)

    def evaluate(self, estimated, reference):
        return self.results_from_counts(self.counts(estimated, reference), list(estimated.keys())[:len(reference)])

    stacked = True                 # the references are stacked notes (a tablature model's); NoteEvaluator: batched notes

    def stage_batch(self, refs, batch):
        """Notes as one (pitch, onset)-sorted row array plus offsets, a group per clip (stacked: per clip and slice); on the device only
        when every pitch is one the kernel takes."""
        groups = [g for r in refs for g in (_stacked_rows(r) if self.stacked else [r])]
        rows, offsets, ok = _pack_groups(groups)
        return _NoteRefs(rows, offsets, (batch.upload(rows), batch.upload(offsets)) if ok else None, len(groups) // max(len(refs), 1),
                         [list(r.keys()) for r in refs] if self.stacked else None)

    def enqueue_batch(self, staged, batch):
        assert self.stacked == (batch.notes.strings is not None), 'NoteEvaluator scores batched notes, StackedNoteEvaluator the stacked notes of a tablature model'
        assert staged.per_clip == (batch.notes.strings or 1), 'one reference note group per string'
        # the decoder's rows as they are on the device, before result()'s host ordering, which the matcher does not need
        return self.match_batch(batch.dev_rows, staged.dev) if staged.dev is not None and batch.dev_rows is not None else ()

    def results_batch(self, staged, counts, batch):
        from . import _lib
        counts, status = counts if counts else (None, None)
        if counts is not None and not batch.overflow and int(status[0]) == -1:
            raise _lib.AmtxError('amtx_eval_notes_match: an estimated note with a fractional pitch')
        # the host matcher takes the whole batch when the references' pitches are fractional, when the decoder overflowed (the
        # matcher ran on a truncated buffer; the batch is decoded again for the host) or when a group is beyond the window bound
        if counts is None or batch.overflow or int(status[0]) != 0:
            counts = _host_note_counts(self, *batch.est_rows_host(), staged.rows, staged.offsets)
        n = staged.per_clip
        return [self.results_from_counts(counts[j * n:(j + 1) * n], staged.keys[j] if staged.keys else None) for j in range(len(batch.idx))]


class NoteEvaluator(StackedNoteEvaluator):
    """The same for one list of batched notes (N, 3) (amt_tools/evaluate.py:990-1037)."""

    def __init__(self, offset_ratio=None, unpack_key=None, results_key=None, save_dir=None, patterns=None, verbose=False):
        super().__init__(offset_ratio, True, unpack_key, results_key, save_dir, patterns, verbose)

    stacked = False

    def evaluate(self, estimated, reference):
        estimated, reference = np.asarray(estimated), np.asarray(reference)
        return super().evaluate(tools.notes_to_stacked_notes(estimated[..., 2], estimated[:, :2]),
                                tools.notes_to_stacked_notes(reference[..., 2], reference[:, :2]))


class _TabCounts(object):
    """Counting shared by the two tablature evaluators: [0] sounding cells of the estimate, [1] of the reference, [2] cells where both sound
    the same class, [3] (pitch, frame) cells sounding in both collapsed maps, [4] cells with equal class (silence included), [5] cells."""

    @staticmethod
    def counts(estimated, reference, profile):
        estimated, reference = np.asarray(estimated), np.asarray(reference)
        out = np.zeros(6, dtype=np.float64)
        if profile is not None:
            st_est = tools.tablature_to_stacked_multi_pitch(estimated, profile)
            st_ref = tools.tablature_to_stacked_multi_pitch(reference, profile)
            out[0], out[1], out[2] = np.sum(st_est.flatten()), np.sum(st_ref.flatten()), np.sum(st_est.flatten() * st_ref.flatten())
            mp_est, mp_ref = tools.stacked_multi_pitch_to_multi_pitch(st_est), tools.stacked_multi_pitch_to_multi_pitch(st_ref)
            out[3] = np.sum(mp_est.flatten() * mp_ref.flatten())
        out[4], out[5] = np.sum(estimated == reference), reference.size
        return out

    @staticmethod
    def counts_batch(estimated, reference, profile):
        """(B, S, T) int64 device tablatures -> (B, 6) int64 device tensor (amtx_eval_tab_counts)."""
        import torch
        from . import _lib
        assert estimated.is_cuda and estimated.dtype == reference.dtype == torch.int64 and estimated.shape == reference.shape and estimated.dim() == 3
        est, ref = estimated.contiguous(), reference.contiguous()
        B, S, T = est.shape
        if profile is not None:
            tuning, classes = np.ascontiguousarray(profile.get_midi_tuning(), dtype=np.int32), int(profile.num_pitches)
            assert len(tuning) == S, (len(tuning), S)
        else:
            tuning, classes = np.zeros(S, dtype=np.int32), 1           # only count [4] is read then
        counts = torch.empty((B, 6), dtype=torch.int64, device=est.device)
        five = torch.empty((B, 5), dtype=torch.int64, device=est.device)
        _lib.call('amtx_eval_tab_counts', est, ref, B, S, T, tuning, classes, five, device=est.device)
        counts[:, :5] = five
        counts[:, 5] = S * T
        return counts


class TablatureEvaluator(Evaluator):
    """Precision / recall / f-measure of (string, fret) activations and the tablature disambiguation rate (amt_tools/evaluate.py:1195-1294)."""

    def __init__(self, profile, unpack_key=None, results_key=None, save_dir=None, patterns=None, verbose=False):
        super().__init__(unpack_key, results_key, save_dir, patterns, verbose)
        self.profile = profile

    @staticmethod
    def get_default_key():
        return tools.KEY_TABLATURE

    def counts(self, estimated, reference):
        return _TabCounts.counts(estimated, reference, self.profile)

    def counts_batch(self, estimated, reference):
        return _TabCounts.counts_batch(estimated, reference, self.profile)

    reference_dtype = np.int64

    def enqueue_batch(self, staged, batch):
        return (self.counts_batch(batch.preds[tools.KEY_TABLATURE].long(), staged),)

    def results_from_counts(self, counts):
        counts = np.asarray(counts, dtype=np.float64)
        num_predicted, num_ground_truth, num_correct_tablature, num_correct_multi_pitch = counts[0], counts[1], counts[2], counts[3]
        precision = num_correct_tablature / (num_predicted + EPSILON)
        recall = num_correct_tablature / (num_ground_truth + EPSILON)
        return {tools.KEY_PRECISION: precision, tools.KEY_RECALL: recall, tools.KEY_F1: _f_measure(precision, recall),
                tools.KEY_TDR: num_correct_tablature / (num_correct_multi_pitch + EPSILON)}

    def evaluate(self, estimated, reference):
        return self.results_from_counts(self.counts(estimated, reference))


class SoftmaxAccuracy(Evaluator):
    """Share of (group, frame) cells whose class is right (amt_tools/evaluate.py:1297-1345)."""

    @staticmethod
    def get_default_key():
        return tools.KEY_TABLATURE

    def counts(self, estimated, reference):
        return _TabCounts.counts(estimated, reference, None)

    def counts_batch(self, estimated, reference):
        return _TabCounts.counts_batch(estimated, reference, None)

    reference_dtype, enqueue_batch = np.int64, TablatureEvaluator.enqueue_batch

    def results_from_counts(self, counts):
        counts = np.asarray(counts)
        return {tools.KEY_ACCURACY: np.float64(counts[4]) / np.float64(counts[5])}

    def evaluate(self, estimated, reference):
        return self.results_from_counts(self.counts(estimated, reference))


# ------------------------------------------------------------------------------------------------------------------------------
# batched validation
# ------------------------------------------------------------------------------------------------------------------------------
def _leaves(evaluator):
    if isinstance(evaluator, ComboEvaluator):
        assert not any(isinstance(e, ComboEvaluator) for e in evaluator.evaluators), 'a ComboEvaluator inside a ComboEvaluator'
        return list(evaluator.evaluators)
    return [evaluator]


def _pack_groups(groups):
    """List of (N, 3) row arrays -> (rows (max(total, 1), 3) float64 in (pitch, onset) order per group, offsets (G + 1,) int32, whether
    every pitch is an integer the kernel takes)."""
    groups = [_sort_rows(np.asarray(g, dtype=np.float64).reshape(-1, 3)) for g in groups]
    offsets = np.zeros(len(groups) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(g) for g in groups])
    rows = np.concatenate(groups + [np.zeros((0, 3))], axis=0)
    ok = bool(np.all((rows[:, 2] == np.floor(rows[:, 2])) & (rows[:, 2] >= 0) & (rows[:, 2] < 128)))
    if len(rows) == 0:
        rows = np.zeros((1, 3))
    return np.ascontiguousarray(rows), offsets, ok


# a note evaluator's staged references: _pack_groups' host arrays, the pair on the device (None: a pitch the kernel does not take), groups
# per clip, and per clip the keys of its stacked notes (None: batched notes)
_NoteRefs = namedtuple('_NoteRefs', 'rows offsets dev per_clip keys')


def _host_note_counts(e, est_rows, est_off, ref_rows, ref_off):
    """The host matcher on packed groups: (G, 3) counts."""
    G = len(ref_off) - 1
    out = np.zeros((G, 3), dtype=np.int64)
    for g in range(G):
        a, b = est_rows[est_off[g]:est_off[g + 1]], ref_rows[ref_off[g]:ref_off[g + 1]]
        out[g] = match_notes_count(a[:, 2], a[:, :2], b[:, 2], b[:, :2], e.offset_ratio), len(a), len(b)
    return out


class _Batch(object):
    """One batch of validate_batched on its way through inference._batched: made while the batch is staged (idx, uploads, staged: what
    every leaf's stage_batch returned), filled behind the model (preds, notes: the decoder's handle or None, dev_rows: its
    device_rows(), work: what every leaf's enqueue_batch returned, done: the event behind all of it) and read when it is finished
    (overflow: the decoder's first buffer was too small)."""

    def __init__(self, idx, model, device):
        self.idx, self.model, self.device, self.uploads, self._est_host = idx, model, device, [], None
        # losses=True: model_entries, the ground truth (and tools.KEY_LOSS_FRAMES) the model's batch carries; loss_counts, the frames each
        # clip's sums run over; loss_results, finished loss dictionaries (validate_tracks).  All None: a LossWrapper warns as ever
        self.model_entries = self.loss_counts = self.loss_results = None

    def upload(self, array):
        """A host array of references to the device, from pinned memory on the current (copy) stream; enqueue record_stream()s them all."""
        import torch
        self.uploads.append(torch.from_numpy(array).pin_memory().to(self.device, non_blocking=True))
        return self.uploads[-1]

    def est_map(self, key, stacked):
        """The model's map under `key`; a tablature model's multi-pitch map is expanded from its tablature (amtx_tab_expand)."""
        est = self.preds.get(key)
        if est is None and key == tools.KEY_MULTIPITCH and tools.KEY_TABLATURE in self.preds:
            est = tools.tab_expand(self.preds[tools.KEY_TABLATURE], self.model.profile, stacked=stacked, collapsed=not stacked)[0 if stacked else 1]
        if est is None:
            raise KeyError(f'the model output has no entry \'{key}\'')
        return est

    def est_rows_host(self):
        """(rows, offsets) of the estimated notes on the host, fetched once: only a batch that takes the host matcher asks."""
        if self._est_host is None:
            if self.dev_rows is not None:
                self._est_host = self.notes.fetch()[:2]      # decodes once more when the first buffer was too small
            else:                                             # CPU tablature decoder
                self._est_host = _pack_groups([g for clip in self.notes.result() for g in _stacked_rows(clip)])[:2]
        return self._est_host


def _check_losses(who, leaves, model, labels=None, banks=False):
    """What losses=True needs, checked before anything is launched -> the model's loss_label_keys.  ValueError without a LossWrapper
    among the evaluators, for a model without a per-clip loss and, in the bank loops, without a LabelBank or for a LabelBank that lacks
    one of those keys: all of them, for a map derived at a clip's edge (onsets from multi_pitch) would differ from the track's."""
    if not any(isinstance(e, LossWrapper) for e in leaves):
        raise ValueError(f'{who}: losses=True scores the loss through a LossWrapper: the evaluator holds none')
    keys = getattr(model, 'loss_label_keys', None)
    if keys is None:
        raise ValueError(f'{who}: losses=True needs a model with per-clip losses (loss_label_keys): {type(model).__name__} has none')
    if banks:
        if labels is None:
            raise ValueError(f'{who}: losses=True needs a LabelBank with the label maps {tuple(keys)} of {type(model).__name__}')
        for key in keys:
            if key not in labels.keys:
                raise ValueError(f'{who}: losses=True needs the label map \'{key}\' of {type(model).__name__}, the LabelBank holds {labels.keys}')
    return tuple(keys)


def validate_batched(clips, references, model, evaluator, times=None, batch_size=256, rank=0, world=1, losses=False):
    """Score a partition without bringing a map to the host.  `clips` as for run_offline_batched; `references`: one ground-truth dictionary
    per clip with the keys the evaluators unpack (KEY_MULTIPITCH / KEY_ONSETS / KEY_OFFSETS maps, KEY_NOTES as batched notes -- stacked
    notes for tablature models --, KEY_TABLATURE).  The loop is run_offline_batched's (inference._batched), with every evaluator's
    stage_batch / enqueue_batch / results_batch as its hooks: a batch's references are uploaded beside its audio; behind the model, notes
    are decoded on the device when the evaluator tree holds a note evaluator and the decoder's row arrays go straight to
    amtx_eval_notes_match; only the count tensors (and the decoder's offsets table) come back, on transcribe's side stream, while the next
    batch runs.  Every clip's results are appended to the evaluator in clip order, exactly as process_track would have.  Returns
    evaluator.average_results() for the clips this rank owns.

    A LossWrapper among the evaluators warns and contributes an empty dictionary per clip -- an eval-mode batch carries no loss -- unless
    `losses` is set.  With losses=True (a GPU model) the references' own maps under the model's loss_label_keys are uploaded beside the
    audio (a key a map evaluator reads too goes up twice), the model runs labelled with tools.KEY_LOSS_FRAMES = None and returns per-clip
    float64 sums (amt_tools_amd/cliploss.py); the LossWrapper tracks {loss key: sum / frames} per clip, the reference's loss of that clip
    as a batch of one, so average_results()[KEY_LOSS] is the mean over clips; nothing warns, and only the sum tensors come back beside
    the counts.  ValueError before anything is launched: no LossWrapper, a model whose loss_label_keys is None, a model that is not on
    a GPU, a reference without the first of those keys (the others are derived by the model where its post_proc derives them)."""
    from .inference import _model_device, run_offline_batched
    assert len(references) == len(clips), (len(references), len(clips))
    leaves = _leaves(evaluator)
    loss_keys = _check_losses('validate_batched', leaves, model) if losses else None
    need_notes = any(isinstance(e, StackedNoteEvaluator) for e in leaves)
    device, on_gpu = _model_device(model)

    def track(results, i):
        evaluator.track_results(results if isinstance(evaluator, ComboEvaluator) else results[0], i)

    if losses:
        for i, ref in enumerate(references):
            if not tools.query_dict(ref, loss_keys[0]):
                raise ValueError(f'validate_batched: losses=True needs the label map \'{loss_keys[0]}\' of every clip: the reference of clip {i} has none')
        if not on_gpu:
            raise ValueError('validate_batched: losses=True is part of the device loop: the model has to be on a GPU')
    if not on_gpu:
        # a CPU model: the host evaluators on run_offline_batched's output, clip by clip
        out = run_offline_batched(clips, model, times=times, batch_size=batch_size, rank=rank, world=world, decode_notes=need_notes)
        for i, preds in out.items():
            track([e.evaluate(*e.unpack(preds, references[i])) for e in leaves], i)
        return evaluator.average_results()

    def stage(idx, batch):
        if losses:
            given = [k for k in loss_keys if all(tools.query_dict(references[i], k) for i in idx)]
            batch.model_entries = {k: batch.upload(np.stack([np.asarray(references[i][k]) for i in idx]).astype(np.int64 if k == tools.KEY_TABLATURE else np.float32))
                                   for k in given}
            batch.model_entries[tools.KEY_LOSS_FRAMES] = None
            batch.loss_counts = np.full(len(idx), batch.model_entries[loss_keys[0]].shape[-1], dtype=np.int64)
        return [e.stage_batch([tools.unpack_dict(references[i], e.unpack_key) for i in idx], batch) for e in leaves]

    _score_on_device(clips, stage, model, evaluator, times, batch_size, rank, world, losses)
    return evaluator.average_results()


class _BankNoteRefs(object):
    """_NoteRefs of a batch whose references a tracks.NoteBank sliced on the device: `dev` is its (rows, offsets) pair (None: the bank
    holds a pitch the device matcher does not take), and `rows` / `offsets` -- read only by a batch that takes the host matcher -- are
    notes.host_clips of the same request, packed when first asked for."""

    def __init__(self, notes, request, dev, whole=False):
        """request: (track ids, first frames, num_frames) of notes.clips; with `whole`, (track ids,) of notes.whole."""
        self.dev, self.per_clip = dev, notes.slices
        self.keys = [list(notes.keys)] * len(request[0]) if notes.stacked else None
        self._notes, self._request, self._host, self._whole = notes, request, None, whole

    def _packed(self):
        if self._host is None:
            groups = self._notes.host_whole(*self._request) if self._whole else self._notes.host_clips(*self._request)
            self._host = _pack_groups(groups)[:2]
        return self._host

    rows = property(lambda self: self._packed()[0])
    offsets = property(lambda self: self._packed()[1])


def _check_banks(who, leaves, bank, labels, notes, relative_times):
    """What validate_clips and validate_tracks refuse before anything is launched: an evaluator whose bank is missing or does not hold
    its key, stacked against batched notes, (relative_times: a NoteBank with absolute times,) and banks of different track counts."""
    for e in leaves:
        if isinstance(e, LossWrapper):
            continue
        if isinstance(e, StackedNoteEvaluator):
            if notes is None:
                raise ValueError(f'{type(e).__name__} scores notes: {who} needs a NoteBank for it')
            if e.stacked != notes.stacked:
                raise ValueError(f'{type(e).__name__} scores {"stacked" if e.stacked else "batched"} notes, the NoteBank holds '
                                 f'{"stacked" if notes.stacked else "batched"} notes')
            if relative_times and not notes.relative_times:
                raise ValueError('the NoteBank holds absolute times: a clip is decoded on a grid that starts at its own first frame (relative_times=True)')
        elif labels is None:
            raise ValueError(f'{type(e).__name__} scores the label map \'{e.unpack_key}\': {who} needs a LabelBank for it')
        elif e.unpack_key not in labels.keys:
            raise ValueError(f'{type(e).__name__} scores the label map \'{e.unpack_key}\', the LabelBank holds {labels.keys}')
    for other, what in ((labels, 'LabelBank'), (notes, 'NoteBank')):
        if other is not None and len(other) != len(bank):
            raise ValueError(f'a bank of {len(bank)} tracks and a {what} of {len(other)}')


def validate_clips(bank, labels, notes, model, evaluator, track_ids, first_frames, num_frames, times=None, batch_size=256, rank=0, world=1,
                   losses=False):
    """validate_batched for clips of resident tracks: clip i is `num_frames` frames from first_frames[i] on of track track_ids[i] (a request
    as bank.clips takes it; tracks.cover_clips names the clips that cover whole tracks).  `bank`: the tracks.TrackBank / PyramidBank the
    model's front-end reads; `labels`: the LabelBank of the same tracks, with every key a map or tablature evaluator unpacks (None: no
    such evaluator); `notes`: their NoteBank with relative_times (None: no note evaluator).  ValueError, before anything is launched,
    for an evaluator whose bank is missing or does not hold its key, and for a request the banks refuse.

    The loop is validate_batched's (inference._batched over an inference.BankClips): per batch the model gets
    {tools.KEY_AUDIO: bank.clips(...)}, the references are labels.clips(...) and notes.clips(...) -- device tensors in the layouts
    stage_batch would have uploaded -- and only clip descriptors go to the device and count tensors come back.  The host matcher runs
    on notes.host_clips(...) where results_batch falls back: the matcher's status word asks for it, the decoder overflowed, or
    notes.integral is false.  A LossWrapper warns and contributes an empty dictionary, as in validate_batched, unless `losses` is set.
    Every clip's results are appended in clip order; returns evaluator.average_results() for the clips this rank owns.

    losses=True: as in validate_batched, with labels.clips(...) of the batch's request as the model's ground truth -- made once per
    batch and shared with the map evaluators.  ValueError before anything is launched also for labels=None and for a LabelBank that
    lacks one of the model's loss_label_keys: all are required here, for a map derived at a clip's edge would differ from the track's."""
    from .inference import BankClips, _model_device
    leaves = _leaves(evaluator)
    _check_banks('validate_clips', leaves, bank, labels, notes, relative_times=True)
    loss_keys = _check_losses('validate_clips', leaves, model, labels, banks=True) if losses else None
    source = BankClips(bank, track_ids, first_frames, num_frames)
    if not _model_device(model)[1]:
        raise ValueError('validate_clips scores clips of device-resident tracks: the model has to be on a GPU')
    need_maps = any(not isinstance(e, (LossWrapper, StackedNoteEvaluator)) for e in leaves)
    need_notes = any(isinstance(e, StackedNoteEvaluator) for e in leaves)

    def stage(idx, batch):
        request = source.of(idx) + (source.num_frames,)
        maps = labels.clips(*request) if need_maps or losses else None
        if losses:
            batch.model_entries = {**{k: maps[k] for k in loss_keys}, tools.KEY_LOSS_FRAMES: None}
            batch.loss_counts = np.full(len(idx), source.num_frames, dtype=np.int64)
        refs = None
        if need_notes:
            sliced = notes.clips(*request) if notes.integral else None
            refs = _BankNoteRefs(notes, request, (sliced.rows, sliced.offsets) if sliced is not None else None)
        return [None if isinstance(e, LossWrapper) else refs if isinstance(e, StackedNoteEvaluator) else maps[e.unpack_key] for e in leaves]

    _score_on_device(source, stage, model, evaluator, times, batch_size, rank, world, losses)
    return evaluator.average_results()


def _batch_scorer(stage, model, evaluator, times):
    """The part of the device validation loops that scores ONE batch of predictions, as the three hooks inference._batched calls:
    (stage_extra, enqueue, finish).  stage(idx, batch) -> what each leaf gets as `staged`: the references of the clips idx on the device
    (or on their way there through batch.upload).  enqueue(idx, preds, batch) decodes the notes of `preds` when the evaluator tree holds a
    note evaluator (grid: `times`, None for the model's own grid of the maps' length) and enqueues every leaf's counting on the current
    stream; finish(batch) brings the counts back on transcribe's side stream and appends every clip's results under its index."""
    import torch
    from . import transcribe
    from .inference import _model_device
    leaves = _leaves(evaluator)
    need_notes = any(isinstance(e, StackedNoteEvaluator) for e in leaves)
    device = _model_device(model)[0]
    side = transcribe._side_stream(device)

    def track(results, i):
        evaluator.track_results(results if isinstance(evaluator, ComboEvaluator) else results[0], i)

    def stage_extra(idx):
        batch = _Batch(idx, model, device)
        batch.staged = stage(idx, batch)
        return batch

    def enqueue(idx, preds, batch):
        """Everything of one batch that runs on the device."""
        stream = torch.cuda.current_stream(device)
        for t in batch.uploads:
            t.record_stream(stream)
        batch.preds = preds
        batch.notes = transcribe.decode_notes_for(preds, model, times) if need_notes else None
        batch.dev_rows = batch.notes.device_rows() if need_notes else None      # None: the CPU tablature decoder
        batch.work = [e.enqueue_batch(staged, batch) for e, staged in zip(leaves, batch.staged)]
        batch.done = torch.cuda.Event()
        batch.done.record(stream)
        return batch

    def finish(batch):
        side.wait_event(batch.done)
        with torch.cuda.stream(side):
            host = [tuple(t.cpu().numpy() for t in work) for work in batch.work]
            est_off = batch.dev_rows[1].cpu().numpy() if batch.dev_rows is not None else None
        batch.overflow = est_off is not None and int(est_off[-1]) > batch.dev_rows[0].shape[0]
        per_eval = [e.results_batch(staged, counts, batch) for e, staged, counts in zip(leaves, batch.staged, host)]
        for j, i in enumerate(batch.idx):
            track([r[j] for r in per_eval], i)

    return stage_extra, enqueue, finish


def _score_on_device(clips, stage, model, evaluator, times, batch_size, rank, world, losses=False):
    """What validate_batched and validate_clips share on a GPU model: inference._batched over `clips` (host clips or a BankClips) with
    _batch_scorer's hooks.  With `losses` the model's batch also carries what stage left in batch.model_entries."""
    from .inference import _batched
    stage_extra, enqueue, finish = _batch_scorer(stage, model, evaluator, times)
    _batched(clips, model, batch_size, rank, world, enqueue, finish, stage_extra, (lambda batch: batch.model_entries) if losses else None)


def validate_tracks(bank, labels, notes, model, evaluator, num_frames, margin, track_ids=None, batch_size=256, rank=0, world=1, exact=False, losses=False):
    """Score WHOLE resident tracks, one result per track, as the reference's validate does -- from equally long overlapped clips.  The
    tracks (`track_ids`, default every track of `bank`; position j belongs to rank j % world) go through inference.run_tracks' stitching
    pass: clips of `num_frames` frames by tracks.seam_clips, of each only the frames at least `margin` frames from a clip edge that is
    not a track edge, written into whole-track maps on the device.  Then, track by track, the stitched views are the predictions of a
    batch of one, labels.clips([t], [0], L_t) and notes.whole([t]) its references, and both go through the hooks validate_clips scores a
    batch with: notes are decoded on the track's own grid, only count tensors come back, and the host matcher (on notes.host_whole)
    takes over where validate_clips falls back.  Every track's results are tracked under its id, in request order; returns
    evaluator.average_results() for the tracks this rank owns.

    Segment-wise inference (inference.run_tracks): exact for TabCNN from margin 4 on and for tracks that fit one clip, an approximation
    for the BiLSTMs of Onsets & Frames; `margin` has no default.  ValueError before anything is launched as in validate_clips (a missing
    bank or key, stacked against batched notes, a model that is not on a GPU), and for what tracks.seam_clips refuses.  A NoteBank with
    absolute times is as good as one with relative times: a whole track starts at time 0.  A LossWrapper warns and contributes an
    empty dictionary unless `losses` is set.

    losses=True: every clip of the stitching pass runs labelled -- labels.clips(...) of its request under the model's loss_label_keys --
    with tools.KEY_LOSS_FRAMES = the columns it keeps, {src_first, count} = plan.kept[:, 1:3] (a short track, run whole: {0, L_t}), so
    the model returns, per clip, float64 sums over exactly the frames that are stitched.  Every frame of a track is kept once, hence
        loss(track) = sum_k mean_t = (1 / L_t) * sum over the track's clips of their sums,
    added up in plan order in float64 on the host; the LossWrapper tracks that dictionary with the track's other results.  No logits are
    stitched.  This is the loss of the SEGMENT-WISE logits, the same approximation as the predictions: exact for tracks that fit one
    clip, for TabCNN from margin 4 on the whole track's loss, an approximation for Onsets & Frames.  ValueError as in validate_clips.

    exact=True: inference.run_tracks' exact route (inference._exact_tracks; OnsetsFrames / OnsetsFrames2 in eval mode, margin >= 3) makes
    the maps -- whole-track inference, scored as above.  With losses=True its language passes also return the packed logits, and a
    track's sums are model.loss_sums on the track's (1, L_t, n_out) logits against labels.clips([t], [0], L_t) over the frames [0, L_t):
    loss(track) = sums / L_t is the loss of the WHOLE-TRACK logits, what the model gives for the track as a batch of one."""
    import torch
    from . import cliploss
    from .inference import _check_exact, _exact_tracks, _model_device, _stitch_tracks
    if exact:
        _check_exact(model, margin)
    leaves = _leaves(evaluator)
    _check_banks('validate_tracks', leaves, bank, labels, notes, relative_times=False)
    loss_keys = _check_losses('validate_tracks', leaves, model, labels, banks=True) if losses else None
    if not _model_device(model)[1]:
        raise ValueError('validate_tracks scores device-resident tracks: the model has to be on a GPU')
    need_maps = any(not isinstance(e, (LossWrapper, StackedNoteEvaluator)) for e in leaves)
    need_notes = any(isinstance(e, StackedNoteEvaluator) for e in leaves)
    device = _model_device(model)[0]
    collected = []                         # per batch of the stitching pass: (the slot of each clip, the model's per-clip sums)

    def model_entries(ids, firsts, frames, windows):
        maps = labels.clips(ids, firsts, frames)
        table = np.ascontiguousarray(windows, dtype=np.int32)
        return {**{k: maps[k] for k in loss_keys}, tools.KEY_LOSS_FRAMES: cliploss.Windows(table, torch.from_numpy(table).to(device))}

    with torch.no_grad():
        track_losses = None
        if exact:
            mine, stitched, *rest = _exact_tracks(bank, model, num_frames, margin, track_ids, batch_size, rank, world, want_logits=losses)
            if losses and stitched is not None:
                sums = []
                for j, t in enumerate(mine.tolist()):
                    L = int(bank.frame_counts[t])
                    maps = labels.clips([t], [0], L)
                    table = np.array([[0, L]], dtype=np.int32)
                    sums.append(model.loss_sums(rest[0][j], {k: maps[k] for k in loss_keys}, cliploss.Windows(table, torch.from_numpy(table).to(device))))
                host = {key: torch.cat([d[key] for d in sums]).cpu().numpy() for key in sums[0]}       # the only transfer of the losses
                track_losses = [{key: host[key][j] / float(bank.frame_counts[t]) for key in host} for j, t in enumerate(mine.tolist())]
        elif losses:
            mine, stitched = _stitch_tracks(bank, model, num_frames, margin, track_ids, batch_size, rank, world, model_entries=model_entries,
                                            collect=lambda slots, preds: collected.append((np.asarray(slots), preds[tools.KEY_LOSS])))
        else:
            mine, stitched = _stitch_tracks(bank, model, num_frames, margin, track_ids, batch_size, rank, world)
        if collected:
            # the only transfer of the losses: the sum tensors.  np.add.at adds in index order: a track's clips in plan order
            slots = np.concatenate([s for s, _ in collected])
            lengths = np.asarray(bank.frame_counts, dtype=np.float64)[mine]
            totals = {}
            for key in collected[0][1]:
                totals[key] = np.zeros(len(mine), dtype=np.float64)
                np.add.at(totals[key], slots, torch.cat([sums[key] for _, sums in collected]).cpu().numpy())
            track_losses = [{key: total[j] / lengths[j] for key, total in totals.items()} for j in range(len(mine))]

        def stage(idx, batch):
            maps = labels.clips(idx, [0], int(bank.frame_counts[idx[0]])) if need_maps else None
            refs = None
            if need_notes:
                whole = notes.whole(idx) if notes.integral else None
                refs = _BankNoteRefs(notes, (idx,), (whole.rows, whole.offsets) if whole is not None else None, whole=True)
            return [None if isinstance(e, LossWrapper) else refs if isinstance(e, StackedNoteEvaluator) else maps[e.unpack_key] for e in leaves]

        stage_extra, enqueue, finish = _batch_scorer(stage, model, evaluator, None)
        pending = None
        for j, t in enumerate(mine.tolist()):
            batch = stage_extra([t])
            if track_losses is not None:
                batch.loss_results = [track_losses[j]]
            now = enqueue([t], {key: stitched.track(j, key) for key in stitched.keys}, batch)
            if pending is not None:
                finish(pending)                                   # the GPU scores track j meanwhile
            pending = now
        if pending is not None:
            finish(pending)
    return evaluator.average_results()


def sweep_tracks(bank, labels, notes, model, evaluator, num_frames, margin, onset_thresholds, frame_thresholds, track_ids=None, batch_size=256,
                 rank=0, world=1):
    """Score WHOLE resident tracks at every pair of a grid of onset and frame thresholds, from ONE run of the model: returns
    {(onset_thr, frame_thr): results}, `results` being what evaluator.average_results() would hold had validate_tracks(exact=True) scored
    the rank's tracks (position j of `track_ids` belongs to rank j % world) with rolls cut at that pair instead of 0.5.  The
    evaluator's own tracked results are not touched.

    The thresholds act behind the model, so inference._exact_tracks runs once with want_logits (the exact route only: OnsetsFrames /
    OnsetsFrames2 in eval mode on a GPU, margin >= 3).  Per track, amtx_pianoroll_fwd(threshold = -1) turns the onset and frame logits
    into probability maps; then
      * a MultipitchEvaluator (of tools.KEY_MULTIPITCH) takes its counts for all frame thresholds from ONE
        multipitch_grid_counts call against labels.clips([t], [0], L_t): its entry depends on the frame threshold only;
      * the notes of all len(onset_thresholds) * len(frame_thresholds) pairs are decoded by ONE transcribe.decode_notes_grid_async call
        (pair p = i_onset * len(frame_thresholds) + i_frame), and every NoteEvaluator scores them with one amtx_eval_notes_match of P
        groups against notes.whole([t]) repeated P times (offsets 0, N, 2N, ...).  A group the matcher refuses (unsupported, bad
        argument) and a NoteBank with fractional pitches take the host matcher on the same rows, as in validate_tracks; a chunk whose
        rows overflowed the decoder's first buffer is decoded again into one of the exact size and matched again on the device;
      * a LossWrapper is ignored: the loss does not depend on a threshold.
    Only count tensors come back.  Each leaf's results_from_counts makes a track's results, and they are appended and averaged with
    the evaluators' own functions, so the cell (0.5, 0.5) is bit-equal to validate_tracks(exact=True).

    ValueError before anything is launched: inference._check_exact's, validate_tracks' bank checks, a leaf other than
    MultipitchEvaluator (of KEY_MULTIPITCH), NoteEvaluator or LossWrapper, an axis with no, a non-finite, a negative or more than
    MAX_GRID_THRESHOLDS thresholds, and a model that is not on a GPU."""
    import torch
    from . import transcribe
    from .inference import _check_exact, _check_thresholds, _exact_tracks, _frame_times, _model_device, logits_to_map
    _check_exact(model, margin)
    leaves = _leaves(evaluator)
    for e in leaves:
        if not isinstance(e, (MultipitchEvaluator, NoteEvaluator, LossWrapper)):
            raise ValueError(f'sweep_tracks scores MultipitchEvaluator, NoteEvaluator and LossWrapper leaves, not {type(e).__name__}')
        if isinstance(e, MultipitchEvaluator) and e.unpack_key != tools.KEY_MULTIPITCH:
            raise ValueError(f'sweep_tracks: a MultipitchEvaluator scores \'{tools.KEY_MULTIPITCH}\' against the frame thresholds, not \'{e.unpack_key}\'')
    _check_banks('sweep_tracks', leaves, bank, labels, notes, relative_times=False)
    on_thr = _check_thresholds(onset_thresholds, 'sweep_tracks: onset_thresholds', MAX_GRID_THRESHOLDS)
    fr_thr = _check_thresholds(frame_thresholds, 'sweep_tracks: frame_thresholds', MAX_GRID_THRESHOLDS)
    device, on_gpu = _model_device(model)
    if not on_gpu:
        raise ValueError('sweep_tracks scores device-resident tracks: the model has to be on a GPU')
    scored = [e for e in leaves if not isinstance(e, LossWrapper)]
    map_leaves = [e for e in scored if isinstance(e, MultipitchEvaluator)]
    note_leaves = [e for e in scored if isinstance(e, NoteEvaluator)]
    F, P = len(fr_thr), len(on_thr) * len(fr_thr)
    side = transcribe._side_stream(device)

    def enqueue(t, logits, thr_d, pairs_d):
        """Everything of one track that runs on the device."""
        L = int(bank.frame_counts[t])
        mp_prob = logits_to_map(logits[tools.KEY_MULTIPITCH], -1.0)
        work = {'t': t, 'frame': None, 'chunks': []}
        if map_leaves:
            work['frame'] = multipitch_grid_counts(mp_prob, labels.clips([t], [0], L)[tools.KEY_MULTIPITCH], thr_d)
        if note_leaves:
            on_prob = logits_to_map(logits[tools.KEY_ONSETS], -1.0)
            handle = transcribe.decode_notes_grid_async(on_prob, mp_prob, _frame_times(model, L), pairs_d, model.profile.low)
            whole = notes.whole([t]) if notes.integral else None
            for p0, n, chunk in handle.chunks:
                rows, offsets = chunk.device_rows()
                ref = matches = None
                if whole is not None:
                    N = int(whole.total)
                    ref = (whole.rows[:max(N, 1)].repeat(n, 1), torch.arange(n + 1, dtype=torch.int32, device=device) * N)
                    matches = [e.match_batch((rows, offsets), ref) for e in note_leaves]
                work['chunks'].append((p0, n, chunk, rows.shape[0], offsets, matches, ref))
        work['done'] = torch.cuda.Event()
        work['done'].record(torch.cuda.current_stream(device))
        return work

    def finish(work):
        """A track's counts on the host: ((F, 3) frame counts or None, per note leaf its (P, 3) counts)."""
        side.wait_event(work['done'])
        with torch.cuda.stream(side):
            frame = work['frame'][0].cpu().numpy() if work['frame'] is not None else None
            host = [(off.cpu().numpy(), [c.cpu().numpy() for c, _ in matches] if matches is not None else None)
                    for _, _, _, _, off, matches, _ in work['chunks']]
        per_leaf = [np.zeros((P, 3), dtype=np.int64) for _ in note_leaves]
        ref_rows = None
        for (p0, n, chunk, capacity, _, _, ref), (off, counts) in zip(work['chunks'], host):
            if counts is not None and int(off[-1]) > capacity:
                # more notes than the chunk's first buffer held: the matcher saw a truncated buffer.  fetch() decodes once more into a
                # buffer of the exact size (and waits for it), and the matcher runs again on those rows
                chunk.fetch()
                counts = [c.cpu().numpy() for c, _ in (e.match_batch(chunk.device_rows(), ref) for e in note_leaves)]
            for i, e in enumerate(note_leaves):
                bad = np.ones(n, dtype=bool) if counts is None else counts[i][:, 0] < 0
                if counts is not None:
                    per_leaf[i][p0:p0 + n] = counts[i]
                if bad.any():
                    if ref_rows is None:
                        ref_rows = np.asarray(notes.host_whole([work['t']])[0], dtype=np.float64).reshape(-1, 3)
                    est_rows, est_off, _ = chunk.fetch()          # decodes once more when the first buffer was too small
                    for g in np.flatnonzero(bad):
                        a = est_rows[est_off[g]:est_off[g + 1]]
                        per_leaf[i][p0 + g] = match_notes_count(a[:, 2], a[:, :2], ref_rows[:, 2], ref_rows[:, :2], e.offset_ratio), len(a), len(ref_rows)
        return frame, per_leaf

    tracked = {(io, jf): [dict() for _ in scored] for io in range(len(on_thr)) for jf in range(F)}
    with torch.no_grad():
        mine, _, logits = _exact_tracks(bank, model, num_frames, margin, track_ids, batch_size, rank, world, want_logits=True)
        thr_d = torch.tensor(fr_thr, dtype=torch.float32).to(device)
        pairs_d = torch.tensor([[a, b] for a in on_thr for b in fr_thr], dtype=torch.float32).to(device)
        pending, results = None, []
        for j, t in enumerate(mine.tolist()):
            now = enqueue(t, logits[j], thr_d, pairs_d)
            if pending is not None:
                results.append(finish(pending))                   # the GPU scores track j meanwhile
            pending = now
        if pending is not None:
            results.append(finish(pending))
    for frame, per_leaf in results:
        for (io, jf), cell in tracked.items():
            for k, e in enumerate(scored):
                if isinstance(e, MultipitchEvaluator):
                    new = e.results_from_counts(frame[jf:jf + 1])
                else:
                    new = e.results_from_counts(per_leaf[note_leaves.index(e)][io * F + jf:io * F + jf + 1])
                cell[k] = append_results(cell[k], new)
    out = {}
    for (io, jf), cell in tracked.items():
        if isinstance(evaluator, ComboEvaluator):
            average = dict()
            for e, res in zip(scored, cell):
                ComboEvaluator._merge(average, e.results_key, average_results(res))
        else:
            average = average_results(cell[0]) if cell else dict()
        out[(on_thr[io], fr_thr[jf])] = average
    return out
