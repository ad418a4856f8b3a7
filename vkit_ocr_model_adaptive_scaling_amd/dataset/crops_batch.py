"""The batch side of dataset/crops.py: annotated pages -> a collated training batch whose two input images are warped on
the device.  ``adaptive_scaling_pages_collate_fn`` (host, worker-safe) -> ``PageCropWarper`` (main process, csrc/crops.hip) ->
``CharLabelRasterizer`` -> ``TwoPassStep``."""
from typing import Any, Dict, Iterable, Tuple

import numpy as np
import torch

from .blur import blur_row, crop_blur_host
from .crops import AnnotatedPage, CropConfig, crop_host, crop_quads, crop_row, _page_mat
from .labels import collate_quad_pass

_CROP_KEYS = ('crop_rows', 'crop_sources', 'crop_size', 'crop_blur')


def adaptive_scaling_pages_collate_fn(batch: Iterable[Tuple[AnnotatedPage, AnnotatedPage]], config: CropConfig, P: int,
                                      f: int = 2, margin: int = 10, rng_seed: int = 13371,
                                      draw: int = 0) -> Dict[str, Dict[str, Any]]:
    """``(rough page, precise page)`` pairs (the same page twice is fine) -> the batch of
    ``adaptive_scaling_quads_collate_fn`` with ``image`` replaced by ``crop_rows`` (B, 16) int64 - row b reads source b - and
    ``crop_sources``, the list of the B uint8 page arrays (not copied), and ``crop_size``, the crops' (H, W), which the
    warper needs and no other key holds.  Only when ``config.blur`` is set with ``prob > 0`` a pass also holds ``crop_blur``
    (B, 226) int32, the blur rows of its crops (dataset/blur.py).  The quads are carried into the crops
    (``crop_quads``) and go through the same ``quad_rows`` / ``label_points`` as there.  ``draw`` numbers the pass over the
    data: another draw, another crop of the same page.  ``config.core_margin`` must cover ``f * margin``, so that the anchor
    of a precise crop lies in the core box.  Host only."""
    pairs = list(batch)
    if not pairs:
        raise ValueError('empty batch')
    config.check()
    size = tuple(int(v) for v in config.size)
    if config.core_margin < f * margin:
        raise ValueError(f'config.core_margin {config.core_margin} must be at least f * margin = {f * margin}')

    def one_pass(pages, kind: str) -> Dict[str, Any]:
        mats = [_page_mat(p) for p in pages]
        rows = np.stack([crop_row(kind, p, config, rng_seed, draw, source=b) for b, p in enumerate(pages)])
        quads = [crop_quads(np.asarray(p.quads, dtype=np.float64).reshape(-1, 4, 2), r) for p, r in zip(pages, rows)]
        states = [{'seed': rng_seed, 'index': p.index, 'draw': draw} for p in pages]
        rest = collate_quad_pass(quads, [p.index for p in pages], states, size, kind == 'precise', P, f, margin, rng_seed)
        out = {'crop_rows': torch.from_numpy(rows), 'crop_sources': mats, 'crop_size': size}
        if config.blur is not None and config.blur.prob > 0:
            out['crop_blur'] = torch.from_numpy(np.stack([blur_row(kind, p, config, rng_seed, draw) for p in pages]))
        return {**out, **rest}

    return {'rough': one_pass([r for r, _ in pairs], 'rough'), 'precise': one_pass([p for _, p in pairs], 'precise')}


class PageCropWarper:
    """Called in the main process on a batch of ``adaptive_scaling_pages_collate_fn``: the pages of both passes go into one
    byte arena and one upload, one ``ops.crop_warp`` per pass - ``ops.crop_warp_blur`` for a pass that holds ``crop_blur`` -
    writes its (B, 3, H, W) float32 ``image`` on the device, and the batch comes back with ``image`` and without the crop
    keys - what ``CharLabelRasterizer`` takes."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError(f'PageCropWarper runs on the GPU, got device {self.device} (host route: crops_host)')

    def __call__(self, batch: Dict[str, Dict[str, Any]]) -> Dict[str, Dict[str, Any]]:
        from .. import ops
        names = ('rough', 'precise')
        mats, slot, remap = [], {}, {}
        for name in names:  # a page that serves both passes (the same array) is uploaded once
            for m in batch[name]['crop_sources']:
                if id(m) not in slot:
                    slot[id(m)] = len(mats)
                    mats.append(m)
            remap[name] = np.array([slot[id(m)] for m in batch[name]['crop_sources']], np.int64)
        arena, table, _ = ops.image_arena(mats, self.device)
        out = {}
        for name in names:
            part = batch[name]
            rows = part['crop_rows'].numpy().copy()
            rows[:, 0] = remap[name][rows[:, 0]]
            if 'crop_blur' in part:  # host tables: checked here, no copy back
                image = ops.crop_warp_blur(arena, table, rows, part['crop_blur'].numpy(), part['crop_size'])
            else:
                image = ops.crop_warp(arena, table, rows, part['crop_size'])
            out[name] = {'image': image, **{k: v for k, v in part.items() if k not in _CROP_KEYS}}
        return out


def crops_host(batch: Dict[str, Dict[str, Any]]) -> Dict[str, Dict[str, Any]]:
    """What ``PageCropWarper`` returns, through ``crop_host`` (``crop_blur_host`` for a pass that holds ``crop_blur``) and with
    host tensors: the slow route, for checks and for timing against."""
    out = {}
    for name in ('rough', 'precise'):
        part = batch[name]
        rows = part['crop_rows'].numpy()
        if 'crop_blur' in part:
            image = crop_blur_host(part['crop_sources'], rows, part['crop_blur'].numpy(), part['crop_size'])
        else:
            image = crop_host(part['crop_sources'], rows, part['crop_size'])
        image = torch.from_numpy(image)
        out[name] = {'image': image, **{k: v for k, v in part.items() if k not in _CROP_KEYS}}
    return out
