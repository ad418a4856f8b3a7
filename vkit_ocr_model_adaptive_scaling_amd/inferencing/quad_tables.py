"""Match-row tables on the host: what the five routes over match rows (inferencing/evaluation.py, nms.py, ranking.py,
lines.py, line_evaluation.py) do before and after their own rule, stated once.

* lists -> padded batch: ``quad_lists`` turns per-image quad arrays into (n, 4, 2) float64 and holds them to ``MAX_QUADS``;
  ``pad_quads``, ``pad_values`` and ``pad_rows`` lay them, their per-row values and their match rows out as (B, K, ...)
  with ``K = max(1, largest)`` and (B,) int32 counts;
* the checker of the tables the ``*_host`` oracles take, in the shape ``ops._quad_tables`` / ``ops._quad_table`` have on
  the device side: ``host_tables`` (two-sided), ``host_table`` (one-sided) and ``clamped`` for a count;
* the two ends of the device wrappers: ``require_gpu`` and the one capacity retry, ``with_capacity``.

The row layout, the clip and the don't-care pass are the rule's and live in inferencing/evaluation.py."""
from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import torch

ROW_WORDS = 16
MAX_QUADS = 8192  # per image and side: QM_MAX of csrc/quadmatch.hip


# ---- lists -> padded batch -----------------------------------------------------------------------------------------------

def quad_lists(quads: Sequence, gt: Optional[Sequence] = None):
    """One (n, 4, 2)-shaped array per image -> a list of (n, 4, 2) float64 arrays.  With ``gt`` the two-sided form: ``quads``
    are the predictions, both sides must hold as many images, and ``(pred, gt)`` come back.  More than ``MAX_QUADS`` quads in
    an image of either side raise."""
    sides = [[np.asarray(a, dtype=np.float64).reshape(-1, 4, 2) for a in s] for s in ([quads] if gt is None else [quads, gt])]
    if gt is not None and len(sides[0]) != len(sides[1]):
        raise ValueError(f'{len(sides[0])} images of predictions against {len(sides[1])} of annotations')
    most = [max([0] + [len(a) for a in s]) for s in sides]
    if max(most) > MAX_QUADS:
        got = f'{most[0]}' if gt is None else f'{most[1]} annotations / {most[0]} predictions'
        raise ValueError(f'at most {MAX_QUADS} quads per image and side, got {got}')
    return sides[0] if gt is None else (sides[0], sides[1])


def capacity(lists: Sequence) -> int:
    """K of a padded batch: the largest image's rows, at least 1"""
    return max([1] + [len(a) for a in lists])


def _pad(lists: Sequence, tail: Tuple[int, ...], dtype, out=None, count=None) -> Tuple[np.ndarray, np.ndarray]:
    """per-image (n,) + tail arrays -> ``((B, K) + tail, count (B,) int32)``, zero beyond an image's own rows; ``out`` and
    ``count`` are zeroed arrays (views of an upload buffer, say) to fill instead of new ones"""
    out = np.zeros((len(lists), capacity(lists)) + tail, dtype) if out is None else out
    count = np.zeros((len(lists),), np.int32) if count is None else count
    for b, a in enumerate(lists):
        out[b, :len(a)], count[b] = a, len(a)
    return out, count


def pad_quads(lists: Sequence, out=None, count=None) -> Tuple[np.ndarray, np.ndarray]:
    """``quad_lists`` of one side -> ``(quads (B, K, 4, 2) float64, count (B,) int32)``"""
    return _pad(lists, (4, 2), np.float64, out, count)


def pad_rows(tabs: Sequence) -> Tuple[np.ndarray, np.ndarray]:
    """per-image (n, 16) ``match_rows`` tables -> ``(rows (B, K, 16) int32, count (B,) int32)``"""
    return _pad(tabs, (ROW_WORDS,), np.int32)


def pad_values(lists: Sequence, values: Optional[Sequence], dtype, what: str) -> np.ndarray:
    """One value per quad beside ``pad_quads(lists)`` - probs as float32, care or valid flags as uint8 - -> (B, K) ``dtype``.
    ``values`` holds one (n,) array per image and must pair up with the quads image by image; None: 1 for every quad."""
    if values is None:
        out = np.zeros((len(lists), capacity(lists)), dtype)
        for b, a in enumerate(lists):
            out[b, :len(a)] = 1
        return out
    values = [np.asarray(v).reshape(-1) for v in values]
    if len(values) != len(lists):
        raise ValueError(f'{what} must have one entry per image, got {len(values)} for {len(lists)} images')
    if any(len(a) != len(v) for a, v in zip(lists, values)):
        raise ValueError(f'quads and {what} must pair up image by image')
    return _pad(values, (), dtype)[0]


def padded_sides(pred: Sequence, gt: Sequence, gt_care: Optional[Sequence] = None, pred_scores: Optional[Sequence] = None):
    """The two-sided batch of a route that builds its rows on the device -> ``(gt (B, M, 4, 2), gt_count, gt_care (B, M) uint8,
    pred (B, N, 4, 2), pred_count)``, and with ``pred_scores`` a sixth, ``probs (B, N) float32``.  ``gt_care`` holds one (m,)
    array per image, 0 = don't care, or is None: every annotation counts."""
    pq, gq = quad_lists(pred, gt)
    care = None if gt_care is None else [np.asarray(c).reshape(-1) != 0 for c in gt_care]
    out = (*pad_quads(gq), pad_values(gq, care, np.uint8, 'gt_care'), *pad_quads(pq))
    return out if pred_scores is None else out + (pad_values(pq, pred_scores, np.float32, 'pred_scores'),)


# ---- the tables of the host oracles --------------------------------------------------------------------------------------

def clamped(count, K: int) -> int:
    """a count as the device reads it: within [0, K]"""
    return min(max(int(count), 0), K)


def _row_table(side: str, rows, count) -> Tuple[np.ndarray, np.ndarray]:
    """one (B, K, 16) row table and its (B,) count; ``side`` is '', 'gt_' or 'pred_'"""
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    if rows.ndim != 3 or rows.shape[2] != ROW_WORDS:
        raise ValueError(f'{side}rows must be (B, K, {ROW_WORDS}), got {rows.shape}')
    count = np.asarray(count).reshape(-1)
    if len(count) != len(rows):
        raise ValueError(f'{side}count must be ({len(rows)},), got {count.shape}')
    return rows, count


def _row_values(name: str, t, shape, dtype) -> Optional[np.ndarray]:
    """an optional table with one value per row (``gt_care``, ``probs``)"""
    if t is None:
        return None
    t = np.ascontiguousarray(t, dtype=dtype)
    if t.shape != shape:
        raise ValueError(f'{name} must be {shape}, got {t.shape}')
    return t


def host_tables(gt_rows, gt_count, pred_rows, pred_count, gt_care=None, probs=None):
    """The tables of a two-sided oracle -> ``(gt_rows, gt_count, pred_rows, pred_count, gt_care, probs)``, ``B, M, N``: rows
    contiguous int32, ``gt_care`` (B, M) uint8 with None = all ones, ``probs`` (B, N) float32 (None stays None)."""
    gt_rows, gt_count = _row_table('gt_', gt_rows, gt_count)
    pred_rows, pred_count = _row_table('pred_', pred_rows, pred_count)
    (B, M), N = gt_rows.shape[:2], pred_rows.shape[1]
    if len(pred_rows) != B:
        raise ValueError(f'{B} images of annotations against {len(pred_rows)} of predictions')
    gt_care = np.ones((B, M), np.uint8) if gt_care is None else _row_values('gt_care', gt_care, (B, M), np.uint8)
    return (gt_rows, gt_count, pred_rows, pred_count, gt_care, _row_values('probs', probs, (B, N), np.float32)), B, M, N


def host_table(rows, count, probs=None):
    """The one-sided form -> ``(rows, count, probs)``, ``B, K``."""
    rows, count = _row_table('', rows, count)
    B, K = rows.shape[:2]
    return (rows, count, _row_values('probs', probs, (B, K), np.float32)), B, K


# ---- the ends of the device wrappers -------------------------------------------------------------------------------------

def require_gpu(who: str, device, host_route: str) -> torch.device:
    device = torch.device(device)
    if device.type != 'cuda':
        raise ValueError(f'{who} runs on the GPU, got device {device} (host route: {host_route})')
    return device


def with_capacity(who: str, call: Callable, read_stats: Callable, status, candidates):
    """The capacity retry of a device wrapper -> ``(outs, stats)``.  ``call(cap)`` runs the op with ``max_pairs=cap`` (None:
    its default); ``read_stats(outs)`` is the call's one stats read-back, as numpy; ``status`` and ``candidates`` index the
    two columns of it.  If an image reports status the call is repeated once with the largest reported candidate count; a
    second overflow raises."""
    outs = call(None)
    stats = read_stats(outs)
    if stats[status].any():
        outs = call(int(stats[candidates].max()))
        stats = read_stats(outs)
        if stats[status].any():
            raise RuntimeError(f'{who}: the retry with the reported capacity overflowed again')
    return outs, stats
