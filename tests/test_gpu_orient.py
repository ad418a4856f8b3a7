"""Region moments and extents on the MI355X (csrc/orient.hip, ops.region_moments / ops.region_extents) against the host
oracles of inferencing/orient.py (checked on their own in test_cpu_orient.py): exact equality.  The kernel folds equal-label
runs in a thread's quad, then across the wave, then with integer atomics, so the seams are: label changes inside a quad,
several labels in one wave, rows that are no multiple of four (scalar loads), one region across many blocks (contention on
one row of the table), sums beyond 32 bits, labels above the table and directions of both signs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def blobs(seed, B, H, W, n):
    """Random rectangles and diagonals painted over each other: labels 0..n in ragged, interleaved runs."""
    g = np.random.default_rng(seed)
    lab = np.zeros((B, H, W), np.int32)
    for b in range(B):
        for r in range(1, n + 1):
            y, x = int(g.integers(0, H)), int(g.integers(0, W))
            h, w = int(g.integers(1, H // 2)), int(g.integers(1, W // 2))
            lab[b, y:y + h, x:x + w] = r
        noise = g.random((H, W)) < 0.1
        lab[b][noise] = g.integers(0, n + 1, int(noise.sum()))
    return lab


def diagonals(H, W):
    lab = np.zeros((1, H, W), np.int32)
    ys, xs = np.mgrid[0:H, 0:W]
    lab[0][(ys == xs)] = 1
    lab[0][(ys + xs == W - 1)] = 2
    lab[0][(ys == 2 * xs + 3)] = 3
    return lab


def corners(H, W):
    lab = np.zeros((1, H, W), np.int32)
    lab[0, 0, 0], lab[0, 0, W - 1], lab[0, H - 1, 0], lab[0, H - 1, W - 1] = 1, 2, 3, 4
    return lab


def random_dirs(seed, B, R):
    g = np.random.default_rng(seed)
    theta = g.uniform(-np.pi, np.pi, (B, R))  # c and s of both signs, up to the full 2^14
    d = np.stack([np.round(np.cos(theta) * 16384), np.round(np.sin(theta) * 16384)], axis=-1).astype(np.int32)
    d[:, 0] = (16384, 0)
    if R > 1:
        d[:, 1] = (-16384, 16384)
    return d


CASES = {
    'blobs': (lambda: blobs(1, 2, 37, 53, 9), 9),
    'blobs_w4': (lambda: blobs(2, 2, 33, 52, 6), 6),          # rows of whole quads: the 16-byte loads
    'diagonals': (lambda: diagonals(41, 47), 3),
    'corners': (lambda: corners(19, 23), 4),
    'small_table': (lambda: blobs(3, 2, 37, 53, 9), 4),       # labels above R are ignored
    'large_table': (lambda: blobs(4, 1, 37, 53, 5), 11),      # rows without pixels
    'one_region': (lambda: np.ones((1, 96, 200), np.int32), 1),
    'long_row': (lambda: np.ones((1, 1, 32768), np.int32), 2),
}


def check_case(name):
    from vkit_ocr_model_adaptive_scaling_amd import ops
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import orient as O
    make, R = CASES[name]
    lab = make()
    d_lab = torch.from_numpy(lab).cuda()
    want = O.region_moments_host(lab, R)
    got = ops.region_moments(d_lab, R)
    assert got.dtype == torch.int64 and tuple(got.shape) == (lab.shape[0], R, 6)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    assert ops.region_moments(d_lab, R).cpu().numpy().tobytes() == got.tobytes(), 'two calls, equal bytes'
    dirs = random_dirs(7, lab.shape[0], R)
    want_e = O.region_extents_host(lab, dirs)
    got_e = ops.region_extents(d_lab, dirs)
    assert got_e.dtype == torch.int32 and tuple(got_e.shape) == (lab.shape[0], R, 4)
    got_e = got_e.cpu().numpy()
    assert np.array_equal(got_e, want_e), np.argwhere(got_e != want_e)[:5].tolist()
    assert ops.region_extents(d_lab, torch.from_numpy(dirs).cuda(), validate=False).cpu().numpy().tobytes() == got_e.tobytes()
    return want, want_e


@pytest.mark.parametrize('name', list(CASES))
def test_moments_and_extents_match_host(name):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing.orient import EMPTY_EXTENT
    want, want_e = check_case(name)
    if name == 'long_row':
        assert want[0, 0, 4] == sum(x * x for x in range(32768)) > 1 << 43, 'a sum beyond 32 bits'
        assert not want[0, 1].any() and tuple(want_e[0, 1].tolist()) == EMPTY_EXTENT
    if name == 'one_region':
        assert want[0, 0, 0] == 96 * 200
    if name == 'large_table':
        assert (want[0, :, 0] == 0).any()


def test_argument_checks():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    lab = torch.zeros((1, 8, 8), dtype=torch.int32)
    dirs = np.zeros((1, 3, 2), np.int32)
    with pytest.raises(RuntimeError):
        ops.region_moments(lab, 3)
    with pytest.raises(RuntimeError):
        ops.region_extents(lab, dirs)
    d = lab.cuda()
    for bad in (lambda: ops.region_moments(d[0], 3), lambda: ops.region_moments(d.long(), 3), lambda: ops.region_moments(d, 0),
                lambda: ops.region_extents(d, dirs[0]), lambda: ops.region_extents(d, dirs.astype(np.int64)),
                lambda: ops.region_extents(d, np.full((1, 3, 2), 16385, np.int32)),
                lambda: ops.region_extents(d, np.zeros((2, 3, 2), np.int32))):
        with pytest.raises(ValueError):
            bad()
