"""Character quadrilaterals from the precise maps (inferencing/adaptive_scaling.py:399-465,481-491; csrc/charpoly.hip), host
side: a numpy restatement of the reference's peak finding and polygon building - the oracle that the GPU tests
(test_gpu_char_polygons.py) compare against - checked against scipy, a hand-computed quadrilateral, and the argument checks
of the C ABI and of ops.char_polygons, which run before anything touches the device."""
import ctypes

import numpy as np
import pytest
import torch

TWO_PI = 2 * np.pi  # a Python float, as in the reference: numpy 2 applies it to float32 operands in float32


def window_max(mat: np.ndarray, size) -> np.ndarray:
    """scipy.ndimage.maximum_filter(mat, size=size) (mode 'reflect'): the max over rows [y - s//2, y + s - 1 - s//2] and
    the same columns, clamped to the map; a float size truncates to int(size)."""
    s = int(size)
    H, W = mat.shape
    rows = np.empty_like(mat)
    for x in range(W):
        rows[:, x] = mat[:, max(0, x - s // 2):min(W, x + s - s // 2)].max(axis=1)
    out = np.empty_like(mat)
    for y in range(H):
        out[y] = rows[max(0, y - s // 2):min(H, y + s - s // 2)].max(axis=0)
    return out


def peaks(prob: np.ndarray, thr: float, size) -> np.ndarray:
    """:481-491 on one (H, W) float32 map: (N, 2) (y, x) in np.nonzero order."""
    mask = window_max(prob, size) == prob
    mask[prob < thr] = 0  # float32 against a Python float: compared in float32
    return np.stack(np.nonzero(mask), axis=1)


def quads(offset: np.ndarray, angle: np.ndarray, dist: np.ndarray, ys, xs, scale_y: float, scale_x: float) -> np.ndarray:
    """precise_build_polygon (:399-465) for the points (ys, xs) of one page, in float32: (N, 4, 2) (y, x) corners up-left,
    up-right, down-right, down-left.  The point is scaled to the padded image by (scale_y, scale_x)."""
    py = np.asarray(ys).astype(np.float32) * np.float32(scale_y)
    px = np.asarray(xs).astype(np.float32) * np.float32(scale_x)
    oy, ox = offset[ys, xs, 0], offset[ys, xs, 1]
    corners = [(py + oy, px + ox)]
    theta = np.arctan2(oy, ox) % TWO_PI
    for k in range(3):
        theta = (theta + angle[ys, xs, k] * TWO_PI) % TWO_PI
        d = dist[ys, xs, k + 1]
        corners.append((py + np.sin(theta) * d, px + np.cos(theta) * d))
    return np.stack([np.stack(c, axis=-1) for c in corners], axis=1).astype(np.float32)


def char_polygons(prob, offset, angle, dist, thr, size, scale_y, scale_x):
    """The whole step on (B, H, W[, C]) maps: points (N, 3) (b, y, x), probs (N,), quads (N, 4, 2), in (b, y, x) order."""
    pts, prs, qds = [], [], []
    for b in range(prob.shape[0]):
        yx = peaks(prob[b], thr, size)
        ys, xs = yx[:, 0], yx[:, 1]
        pts.append(np.concatenate([np.full((len(yx), 1), b), yx], axis=1))
        prs.append(prob[b][ys, xs])
        qds.append(quads(offset[b], angle[b], dist[b], ys, xs, scale_y, scale_x))
    return (np.concatenate(pts).astype(np.int32).reshape(-1, 3), np.concatenate(prs).astype(np.float32),
            np.concatenate(qds).reshape(-1, 4, 2))


@pytest.mark.parametrize('size', [1, 3, 4, 5, 5.0, 5.5, 9])
def test_window_max_matches_scipy(size):
    ndimage = pytest.importorskip('scipy.ndimage')
    g = np.random.default_rng(11)
    for shape in ((1, 1), (1, 9), (7, 1), (6, 6), (40, 33)):
        mat = (np.floor(g.random(shape) * 16) / 16).astype(np.float32)  # ties and plateaus
        assert np.array_equal(window_max(mat, size), ndimage.maximum_filter(mat, size=size)), (shape, size)
        # the peak rule itself, as the reference writes it
        ref = ndimage.maximum_filter(mat, size=size) == mat
        ref[mat < 0.7] = 0
        assert np.array_equal(peaks(mat, 0.7, size), np.stack(np.nonzero(ref), axis=1))


def test_threshold_is_compared_in_float32():
    at = np.full((3, 3), np.float32(0.7), dtype=np.float32)  # (float)0.7 < 0.7 in double: still a peak
    assert float(np.float32(0.7)) < 0.7 and len(peaks(at, 0.7, 3)) == 9


def test_hand_computed_square():
    """Up-left offset (-3, -3) from the point and the angle split in four quarter turns: an axis-aligned 6 x 6 square."""
    offset = np.zeros((4, 5, 2), np.float32)
    angle = np.full((4, 5, 4), 0.25, np.float32)
    dist = np.zeros((4, 5, 4), np.float32)
    offset[2, 3] = (-3, -3)
    dist[2, 3] = (99, 3 * np.sqrt(2), 3 * np.sqrt(2), 3 * np.sqrt(2))  # dist[..., 0] is not used
    q = quads(offset, angle, dist, np.array([2]), np.array([3]), 2.0, 2.0)[0]
    p = np.array([4.0, 6.0])
    expect = p + np.array([(-3, -3), (-3, 3), (3, 3), (3, -3)], np.float64)
    assert q.dtype == np.float32 and np.allclose(q, expect, atol=1e-5)


def test_config_defaults():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import AdaptiveScalingInferencingConfig
    c = AdaptiveScalingInferencingConfig()
    assert c.precise_build_polygons_positive_char_prob_thr == 0.7
    assert c.precise_build_polygons_maximum_filter_size == 5


def test_c_entry_points_validate_before_launch():
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    L, P = _lib.lib, ctypes.c_void_p
    assert L.vkas_char_polygons_workspace_bytes(2, 37, 53, 5) > 2 * 37 * 53 * 4
    assert L.vkas_char_polygons_workspace_bytes(1, 8, 8, 0) == -1 and b'size 0' in L.vkas_last_error()
    assert L.vkas_char_polygons_workspace_bytes(2, 1 << 15, 1 << 15, 5) == -1 and b'2^31' in L.vkas_last_error()
    assert L.vkas_char_polygons_workspace_bytes(1, 0, 8, 5) == -1 and b'bad dims' in L.vkas_last_error()
    a = lambda: P(256)  # any aligned non-null address: the checks run before anything is dereferenced or launched
    nb = L.vkas_char_polygons_workspace_bytes(1, 8, 8, 5)

    def call(*, prob=None, ws=None, nbytes=nb, B=1, H=8, W=8, size=5, quads=None):
        return L.vkas_char_polygons(prob or a(), a(), a(), a(), B, H, W, size, 0.7, 2.0, 2.0, ws or a(), nbytes, a(), a(),
                                    a(), quads or a(), None)

    assert L.vkas_char_polygons(None, a(), a(), a(), 1, 8, 8, 5, 0.7, 2.0, 2.0, a(), nb, a(), a(), a(), a(), None) == -1
    assert b'null pointer' in L.vkas_last_error()
    assert call(size=0) == -1 and b'size 0' in L.vkas_last_error()
    assert call(B=-1) == -1 and b'bad dims' in L.vkas_last_error()
    assert call(B=4, H=1 << 15, W=1 << 14) == -1 and b'2^31' in L.vkas_last_error()
    assert call(nbytes=nb - 1) == -1 and b'workspace' in L.vkas_last_error()
    assert call(quads=P(260)) == -1 and b'aligned' in L.vkas_last_error()
    assert call(ws=P(264)) == -1 and b'aligned' in L.vkas_last_error()


def test_ops_char_polygons_validates_before_launch():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    z = torch.zeros
    maps = lambda B=2, H=5, W=7: (z(B, H, W), z(B, H, W, 2), z(B, H, W, 4), z(B, H, W, 4))
    with pytest.raises(ValueError, match='prob'):
        ops.char_polygons(z(5, 7), *maps()[1:], 0.7, 5, 2.0, 2.0)
    for k, bad in ((1, z(2, 5, 7, 3)), (2, z(2, 5, 6, 4)), (3, z(1, 5, 7, 4))):
        args = list(maps())
        args[k] = bad
        with pytest.raises(ValueError, match=('offset', 'angle', 'dist')[k - 1]):
            ops.char_polygons(*args, 0.7, 5, 2.0, 2.0)
    with pytest.raises(ValueError, match='float32'):
        ops.char_polygons(maps()[0].double(), *maps()[1:], 0.7, 5, 2.0, 2.0)
    with pytest.raises(ValueError, match='empty map'):
        ops.char_polygons(*maps(H=0), 0.7, 5, 2.0, 2.0)
    for size in (0, 0.5, -3):
        with pytest.raises(ValueError, match='size'):
            ops.char_polygons(*maps(), 0.7, size, 2.0, 2.0)
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.char_polygons(*maps(), 0.7, 5.5, 2.0, 2.0)  # valid arguments: no CPU fallback


def test_group_char_polygons_splits_in_order():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import (AdaptiveScalingInferencingPreciseCharPolygons,
                                                                 precise_group_char_polygons)
    g = np.random.default_rng(3)
    pts = np.stack(np.nonzero(g.random((16, 24)) < 0.3), axis=1).astype(np.int32)
    n = len(pts)
    r = AdaptiveScalingInferencingPreciseCharPolygons(
        padded_image=np.zeros((32, 48, 3), np.uint8), points=pts, probs=g.random(n).astype(np.float32),
        polygons=g.random((n, 4, 2)).astype(np.float32))
    labels = np.zeros((16, 24), np.int64)
    labels[2:9, 3:20] = 1
    labels[10:15, 1:8] = 3  # label 2 has no pixel: an empty group
    groups = precise_group_char_polygons(r, labels)
    assert len(groups) == 3 and len(groups[1].points) == 0
    for lab, grp in zip((1, 2, 3), groups):
        expect = np.stack(np.nonzero(labels == lab), axis=1)
        keep = [i for i, (y, x) in enumerate(pts) if labels[y, x] == lab]
        assert np.array_equal(grp.points.reshape(-1, 2), pts[keep])
        assert set(map(tuple, grp.points)) <= set(map(tuple, expect))
        assert np.array_equal(grp.probs, r.probs[keep]) and np.array_equal(grp.polygons, r.polygons[keep])
    with pytest.raises(ValueError):
        precise_group_char_polygons(r, labels[:, :20])  # not the map resolution
    with pytest.raises(ValueError):
        precise_group_char_polygons(r, labels.astype(np.float32))
