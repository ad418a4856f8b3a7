"""The device route of inferencing/strips.py: quadrilaterals of several images cut into upright strips in one launch
(``ops.quad_strips_u8``, csrc/strips.hip), and the step of ``infer`` / ``infer_batch`` that does so for the text lines of
their results.  And the device route of inferencing/spines.py: text lines cut along the spines through their characters
(``ops.spine_strips_u8``, csrc/spines.hip), with the same step."""
from typing import Sequence

import attrs
import numpy as np
import torch

from .evaluation import result_quads
from .spines import SpineStrips, check_spine_rows, spine_rows, spine_table
from .strips import QuadStrips, bucket_views, check_strip_rows, strip_rows, strip_table


def _arena(images, device):
    """``images`` as ``(arena, host source table, device source table)``: an ``(arena, sources)`` pair as
    ``ops.image_arena`` gives it (``sources`` the host table; or ``(arena, sources, device sources)``), (H, W, 3) uint8 device
    tensors (copied into one arena on the device) or numpy images (one upload)."""
    from .. import ops
    if isinstance(images, tuple) and len(images) in (2, 3) and isinstance(images[0], torch.Tensor) and images[0].dim() == 1:
        arena, sources = images[0], np.ascontiguousarray(np.asarray(images[1], dtype=np.int64).reshape(-1, 4))
        d_sources = images[2] if len(images) == 3 else torch.from_numpy(sources).to(arena.device, non_blocking=True)
        return arena, sources, d_sources
    if len(images) and all(isinstance(m, torch.Tensor) for m in images):
        sources = np.zeros((len(images), 4), np.int64)
        total = 0
        for i, m in enumerate(images):
            if m.dim() != 3 or m.shape[2] != 3 or m.dtype != torch.uint8 or not m.is_cuda:
                raise ValueError(f'image {i}: a device image is an (H, W, 3) uint8 tensor, got {m.dtype} {tuple(m.shape)}')
            sources[i] = (total, m.shape[0], m.shape[1], 0)
            total += -(-m.numel() // 16) * 16
        arena = torch.empty((total,), dtype=torch.uint8, device=images[0].device)
        for m, (offset, _, _, _) in zip(images, sources.tolist()):
            arena[offset:offset + m.numel()].copy_(m.reshape(-1))
        return arena, sources, torch.from_numpy(sources).to(arena.device, non_blocking=True)
    mats = [np.asarray(getattr(m, 'mat', m)) for m in images]
    for i, m in enumerate(mats):
        if m.ndim != 3 or m.shape[2] != 3:
            raise ValueError(f'image {i}: expected an (H, W, 3) image, got {m.shape}')
    return ops.image_arena(mats, device)


def _cut(cls, who: str, what: str, rule, check, table, launch, images, items_per_image: Sequence, height, width_max, width_step,
         margin, device):
    """The body of ``quad_strips`` and ``spine_strips``: the layout by ``rule``; then, unless it has no rows, the arena and
    its bounds, ``check(layout, sources, h)`` on the host (the launch needs no copy back), the one upload of ``table(layout,
    h)`` and ``launch(layout, h, arena, d_sources, d_table)``.  -> ``cls`` with device buckets."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise ValueError(f'{who} runs on the GPU, got device {device} (host route: {who}_host)')
    layout = rule(items_per_image, height, width_max, width_step, margin)
    h = int(height)
    if len(layout.rows):
        arena, sources, d_sources = _arena(images, device)
        if len(sources) != len(items_per_image):
            raise ValueError(f'{len(items_per_image)} {what} for {len(sources)} images')
        if ((sources[:, 0] < 0) | (sources[:, 0] + 3 * sources[:, 1] * sources[:, 2] > int(arena.numel()))).any():
            raise ValueError(f'{who}: a source leaves the arena of {int(arena.numel())} bytes')
        check(layout, sources, h)
        d_table = torch.from_numpy(table(layout, h)).to(arena.device, non_blocking=True)
        out = launch(layout, h, arena, d_sources, d_table)
    else:
        out = torch.empty((0,), dtype=torch.uint8, device=device)
    return cls.of(layout, bucket_views(out, layout.bucket_shapes), h)


def quad_strips(images, quads_per_image: Sequence, height: int = 32, width_max: int = 2048, width_step: int = 64,
                margin: float = 0.125, device='cuda') -> QuadStrips:
    """Cuts the quadrilaterals ``quads_per_image[s]`` ((n_s, 4, 2) ``(y, x)`` pixels) out of image s, turns them upright and
    brings them to ``height`` rows: one arena upload (none for an ``(arena, sources)`` pair or device images), one row
    upload, one launch, nothing read back - the per-quad arrays come from the host rule (``strip_rows``).  Equal to
    ``quad_strips_host`` byte for byte, with device buckets."""
    from .. import ops
    return _cut(QuadStrips, 'quad_strips', 'quad arrays', strip_rows,
                lambda l, sources, h: check_strip_rows(l.rows, sources, h, l.out_bytes), lambda l, h: strip_table(l.rows, h),
                lambda l, h, arena, d_sources, d_table: ops.quad_strips_u8(arena, d_sources, d_table, h, l.out_bytes, validate=False),
                images, quads_per_image, height, width_max, width_step, margin, device)


def spine_strips(images, lines_per_image: Sequence, height: int = 32, width_max: int = 2048, width_step: int = 64,
                 margin: float = 0.125, device='cuda') -> SpineStrips:
    """Cuts the text lines ``lines_per_image[s]`` - a list of (m, 4, 2) ``(y, x)`` arrays, the character quads of each line of
    image s in reading order - out of image s along their spines (inferencing/spines.py) and brings them to ``height`` rows:
    ``images`` as ``quad_strips`` takes them, one table upload, two launches, nothing read back - the per-line arrays and
    the knots come from the host rule (``spine_rows``).  Equal to ``spine_strips_host`` byte for byte, with device buckets."""
    from .. import ops
    return _cut(SpineStrips, 'spine_strips', 'line lists', spine_rows,
                lambda l, sources, h: check_spine_rows(l.rows, l.knots, sources, h, l.out_bytes, l.columns),
                lambda l, h: spine_table(l.rows, l.knots, h),
                lambda l, h, arena, d_sources, d_table: ops.spine_strips_u8(arena, d_sources, d_table, len(l.rows), len(l.knots), h,
                                                                            l.out_bytes, validate=False),
                images, lines_per_image, height, width_max, width_step, margin, device)


def result_lines(result) -> list:
    """The lines of a result as ``spine_strips`` takes them: per line the quads of its members in reading order."""
    quads = result_quads(result)[0]
    return [quads[np.asarray(members, dtype=np.int64)] for members in result.line_chars]


def spine_strips_for_results(results: Sequence, images_or_arena, height: int = 32, width_max: int = 2048,
                             width_step: int = 64, margin: float = 0.125, device='cuda'):
    """``strips_for_results`` along the spines: the lines of all results - result i reads image i - go through ONE
    ``spine_strips`` call.  -> the results with ``line_strip_ids`` and ``line_spines`` (per line the (K, 2, 2) centres and down
    vectors of ``SpineStrips.spine``; (0, 2, 2) for a line without a strip) filled, and the one shared ``SpineStrips``."""
    strips = spine_strips(images_or_arena, [result_lines(r) for r in results], height, width_max, width_step, margin, device)
    out, first = [], 0
    for r in results:
        n = len(r.line_chars)
        spines = [strips.spine(k) if strips.status[k] == 0 else np.zeros((0, 2, 2), np.float64) for k in range(first, first + n)]
        out.append(attrs.evolve(r, line_strip_ids=np.arange(first, first + n, dtype=np.int32), line_spines=spines))
        first += n
    return out, strips


def strips_for_results(results: Sequence, images_or_arena, height: int = 32, width_max: int = 2048, width_step: int = 64,
                       margin: float = 0.125, device='cuda'):
    """The step of ``infer`` / ``infer_batch``: the ``line_polygons`` of all results - result i reads image i - go through
    ONE ``strip_rows`` and one launch.  -> the results with ``line_strip_ids`` filled (for each line its index into the
    strips object) and the one shared ``QuadStrips``."""
    strips = quad_strips(images_or_arena, [r.line_polygons for r in results], height, width_max, width_step, margin, device)
    out, first = [], 0
    for r in results:
        n = len(r.line_polygons)
        out.append(attrs.evolve(r, line_strip_ids=np.arange(first, first + n, dtype=np.int32)))
        first += n
    return out, strips
