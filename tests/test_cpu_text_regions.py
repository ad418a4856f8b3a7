"""Text regions of the rough maps (inferencing/adaptive_scaling.py:190-279 restated on pixels; inferencing/regions.py,
csrc/regions.hip), host side: ``text_regions_host`` - the oracle of test_gpu_text_regions.py - against scipy's labelling
and np.median, the numbering rule on its own, ``region_scales`` on a hand-computed table, the new config defaults, and the
argument checks of the C ABI and of ops.text_regions, which run before anything touches the device.  The mask and height
builders here are shared with the GPU tests."""
import ctypes

import numpy as np
import pytest
import torch

RANDOM_KINDS = tuple(f'random{int(d * 10)}_{s}' for d in (0.3, 0.5, 0.6) for s in range(3))
KINDS = ('empty', 'full', 'checker', 'dots', 'serpentine', 'comb', 'u', 'diagonal', 'antidiagonal') + RANDOM_KINDS


def make_mask(kind: str, H: int, W: int) -> np.ndarray:
    """(H, W) uint8 masks that stress the labelling: see the GPU test's docstring for what each is there for."""
    y, x = np.mgrid[0:H, 0:W]
    if kind == 'empty':
        m = np.zeros((H, W), bool)
    elif kind == 'full':
        m = np.ones((H, W), bool)
    elif kind == 'checker':       # one region under 8-connectivity, H*W/2 under 4-connectivity
        m = (y + x) % 2 == 0
    elif kind == 'dots':          # ceil(H/2) * ceil(W/2) one-pixel regions: the maximum
        m = (y % 2 == 0) & (x % 2 == 0)
    elif kind == 'serpentine':    # one 1-pixel path over the whole map: even rows, joined at alternating ends
        m = (y % 2 == 0) | ((y % 2 == 1) & (x == np.where((y // 2) % 2 == 0, W - 1, 0)))
    elif kind == 'comb':          # teeth that meet only in the last row
        m = (x % 2 == 0) | (y == H - 1)
    elif kind == 'u':             # two arms that meet only in the last row
        m = (x == 0) | (x == W - 1) | (y == H - 1)
    elif kind == 'diagonal':      # lines through tile corners, 16 apart: (16, 64) lies on x - y = 48
        m = (x - y) % 16 == 0
    elif kind == 'antidiagonal':  # (15, 64) and (16, 63) lie on x + y = 79
        m = (x + y) % 16 == 15
    elif kind.startswith('random'):
        density, seed = kind[len('random'):].split('_')
        m = np.random.default_rng(1000 * int(density) + int(seed) + 7 * H + W).random((H, W)) < int(density) / 10
    else:
        raise KeyError(kind)
    return m.astype(np.uint8) * 255 if kind == 'full' else m.astype(np.uint8)  # any non-zero value is foreground


def make_height(H: int, W: int, seed: int) -> np.ndarray:
    """Heights in [3, 60] in steps of 0.5 (plenty of duplicates), 30 % zeros."""
    g = np.random.default_rng(seed)
    h = (np.floor(g.uniform(3, 60, (H, W)) * 2) / 2).astype(np.float32)
    h[g.random((H, W)) < 0.3] = 0
    return h


def first_pixels(labels: np.ndarray, n: int) -> np.ndarray:
    flat = labels.ravel()
    return np.array([np.flatnonzero(flat == r)[0] for r in range(1, n + 1)], dtype=np.int64)


@pytest.mark.parametrize('kind', KINDS)
def test_host_labelling_matches_scipy(kind):
    ndimage = pytest.importorskip('scipy.ndimage')
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import text_regions_host
    for H, W in ((1, 1), (7, 5), (33, 65), (40, 37)):
        mask = make_mask(kind, H, W)
        height = make_height(H, W, H + W)
        labels, boxes, areas, valid, medians = text_regions_host(mask, height)
        ref, n = ndimage.label(mask, structure=np.ones((3, 3)))
        assert labels.dtype == np.int32 and labels.shape == (H, W)
        assert len(boxes) == len(areas) == len(valid) == len(medians) == n == labels.max(initial=0)
        assert np.array_equal(labels != 0, mask != 0)
        # the same partition: the two labellings map one to one on every foreground pixel
        pairs = np.unique(np.stack([labels[mask != 0], ref[mask != 0]], axis=1), axis=0)
        assert len(pairs) == n and len(np.unique(pairs[:, 0])) == n and len(np.unique(pairs[:, 1])) == n
        # the numbering rule: first pixels strictly increase with the label
        assert (np.diff(first_pixels(labels, n)) > 0).all()
        for r in range(n):
            ys, xs = np.nonzero(labels == r + 1)
            assert tuple(boxes[r]) == (ys.min(), xs.min(), ys.max(), xs.max()) and areas[r] == len(ys)
            v = height[ys, xs]
            v = v[v > 0]
            assert valid[r] == len(v)
            want = np.median(v) if len(v) else np.float32(0)
            assert medians[r].tobytes() == np.float32(want).tobytes()


def test_expected_region_counts():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import text_regions_host
    H, W = 33, 65
    z = np.zeros((H, W), np.float32)
    count = lambda kind: len(text_regions_host(make_mask(kind, H, W), z)[1])
    assert count('empty') == 0 and count('full') == 1 and count('checker') == 1 and count('serpentine') == 1
    assert count('comb') == 1 and count('u') == 1 and count('dots') == 17 * 33
    hole = np.ones((7, 7), np.uint8)  # a ring with a dot in its hole: two regions, the hole itself none (no contour filling)
    hole[1:6, 1:6] = 0
    hole[3, 3] = 1
    labels, boxes, areas, _, _ = text_regions_host(hole, np.zeros((7, 7), np.float32))
    assert len(boxes) == 2 and areas.tolist() == [24, 1] and labels[3, 3] == 2 and labels[2, 2] == 0
    with pytest.raises(ValueError):
        text_regions_host(hole, np.zeros((7, 7), np.float64))
    with pytest.raises(ValueError):
        text_regions_host(hole, np.zeros((7, 8), np.float32))


@pytest.mark.parametrize('n', [0, 1, 2, 3, 4, 6, 100, 101, 1000])
def test_host_median_is_np_median_bit_for_bit(n):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import text_regions_host
    g = np.random.default_rng(n)
    for trial in range(20):
        vals = (g.uniform(0.01, 80, n) if trial % 2 else np.floor(g.uniform(3, 60, n) * 2) / 2).astype(np.float32)
        mask = np.ones((1, n + 3), np.uint8)
        height = np.zeros((1, n + 3), np.float32)
        height[0, g.permutation(n + 3)[:n]] = vals
        _, _, areas, valid, medians = text_regions_host(mask, height)
        assert areas.tolist() == [n + 3] and valid.tolist() == [n]
        want = np.float32(np.median(vals)) if n else np.float32(0)
        assert medians.dtype == np.float32 and medians[0].tobytes() == want.tobytes()


def test_region_scales_hand_computed():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import region_scales
    # a 200 x 300 page whose rough maps are valid on 100 x 150: heights count as predicted (200 / (100 * 2) = 1), a map
    # pixel is 2 x 2 page pixels; the side limit is round(35 * 0.25) = round(8.75) = 9
    boxes = np.array([(0, 0, 4, 19),     # 10 x 40 page pixels, median 7: scale 5, 50 x 200, kept
                      (9, 9, 30, 30),    # no valid height: dropped
                      (50, 3, 50, 4),    # 2 x 4, median 70: scale 0.5, 1 x 2, both sides below 9: dropped
                      (60, 0, 60, 9)],   # 2 x 20, median 70: 1 x 10, only the height is below 9: kept
                     np.int32)
    medians = np.array([7, 0, 70, 70], np.float32)
    scales, resized, keep = region_scales(boxes, medians, (200, 300), (100, 150), 35, 0.25)
    assert scales.dtype == np.float64 and resized.dtype == np.int64 and keep.dtype == bool
    assert scales.tolist() == [5.0, 0.0, 0.5, 0.5]
    assert resized.tolist() == [[50, 200], [0, 0], [1, 2], [1, 10]]
    assert keep.tolist() == [True, False, False, True]
    # a 400 x 300 page on the same maps: heights double (400 / 200), a map row is 4 page rows
    scales, resized, keep = region_scales(boxes[:1], medians[:1], (400, 300), (100, 150))
    assert scales.tolist() == [2.5] and resized.tolist() == [[50, 100]] and keep.tolist() == [True]
    # Python's round, as the reference: 2.5 -> 2
    # (one map row is 5 / 2 = 2.5 page rows; 28 * 5 / (2 * 2) = 35: scale 1)
    scales, resized, _ = region_scales(np.array([(0, 0, 0, 4)], np.int32), np.array([28], np.float32), (5, 5), (2, 5))
    assert scales.tolist() == [1.0] and resized.tolist() == [[2, 5]]
    s, r, k = region_scales(np.zeros((0, 4), np.int32), np.zeros((0,), np.float32), (10, 10), (5, 5))
    assert s.shape == (0,) and r.shape == (0, 2) and k.shape == (0,)
    with pytest.raises(ValueError):
        region_scales(boxes, medians[:2], (200, 300), (100, 150))


def test_config_defaults():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import AdaptiveScalingInferencingConfig
    c = AdaptiveScalingInferencingConfig()
    assert c.precise_flattened_text_region_resized_char_height_median == 35
    assert c.precise_flattened_text_region_resized_ratio_min == 0.25
    assert c.rough_text_regions_max == 4096


def test_c_entry_points_validate_before_launch():
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    L, P = _lib.lib, ctypes.c_void_p
    assert L.vkas_text_regions_workspace_bytes(2, 37, 53, 16) >= 3 * 2 * 37 * 53 * 4
    assert L.vkas_text_regions_workspace_bytes(1, 8, 8, 0) == -1 and b'max_regions 0' in L.vkas_last_error()
    assert L.vkas_text_regions_workspace_bytes(2, 1 << 15, 1 << 15, 5) == -1 and b'2^31' in L.vkas_last_error()
    for dims in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)):
        assert L.vkas_text_regions_workspace_bytes(*dims, 5) == -1 and b'bad dims' in L.vkas_last_error()
    a = lambda: P(256)  # any aligned non-null address: the checks run before anything is dereferenced or launched
    nb = L.vkas_text_regions_workspace_bytes(1, 8, 8, 5)

    def call(*, B=1, H=8, W=8, R=5, ws=None, nbytes=nb, null=None):
        ptrs = [a() for _ in range(9)]  # mask, height, workspace, count, labels, boxes, areas, valid, medians
        if ws is not None:
            ptrs[2] = ws
        if null is not None:
            ptrs[null] = None
        return L.vkas_text_regions(ptrs[0], ptrs[1], B, H, W, R, ptrs[2], nbytes, *ptrs[3:], None)

    for k in range(9):
        assert call(null=k) == -1 and b'null pointer' in L.vkas_last_error()
    assert call(R=0) == -1 and b'max_regions 0' in L.vkas_last_error()
    assert call(B=0) == -1 and b'bad dims' in L.vkas_last_error()
    assert call(H=0) == -1 and b'bad dims' in L.vkas_last_error()
    assert call(W=-3) == -1 and b'bad dims' in L.vkas_last_error()
    assert call(B=4, H=1 << 15, W=1 << 14) == -1 and b'2^31' in L.vkas_last_error()
    assert call(nbytes=nb - 1) == -1 and b'workspace' in L.vkas_last_error()
    assert call(ws=P(264)) == -1 and b'aligned' in L.vkas_last_error()


def test_ops_text_regions_validates_before_launch():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    m = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    h = lambda *s: torch.zeros(*s, dtype=torch.float32)
    with pytest.raises(ValueError, match='mask must be'):
        ops.text_regions(m(5, 7), h(5, 7), 8)
    with pytest.raises(ValueError, match='height must be'):
        ops.text_regions(m(2, 5, 7), h(2, 5, 6), 8)
    with pytest.raises(ValueError, match='uint8'):
        ops.text_regions(m(2, 5, 7).bool(), h(2, 5, 7), 8)
    with pytest.raises(ValueError, match='float32'):
        ops.text_regions(m(2, 5, 7), h(2, 5, 7).double(), 8)
    for shape in ((0, 5, 7), (2, 0, 7), (2, 5, 0)):
        with pytest.raises(ValueError, match='empty'):
            ops.text_regions(m(*shape), h(*shape), 8)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match='max_regions'):
            ops.text_regions(m(2, 5, 7), h(2, 5, 7), bad)
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.text_regions(m(2, 5, 7), h(2, 5, 7), 8)  # valid arguments: no CPU fallback
