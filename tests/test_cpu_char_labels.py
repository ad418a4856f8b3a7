"""Training labels from character quadrilaterals, host side (dataset/labels.py): the quad rows on hand-computed cases, the
validity rule, the host oracle ``char_label_maps_host`` - what tests/test_gpu_char_labels.py holds the kernel to - against
an independent float64 fill, the owner rule, the round trip of ``label_points`` through a float64 restatement of
precise_build_polygon (inferencing/adaptive_scaling.py:399-465, csrc/charpoly.hip), row counts and reproducibility, the
collated batch against the schema of ``adaptive_scaling_dataset_collate_fn``, "labels meet inference" on the host oracles
alone, and the argument checks of the C ABI and of ops.char_label_maps, which run before anything touches the device."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import char_label_cases as C
from tests.test_cpu_char_polygons import peaks
from vkit_ocr_model_adaptive_scaling_amd.dataset import (QuadSample, adaptive_scaling_quads_collate_fn, char_labels_host,
                                                         quad_rows, char_label_maps_host, label_points,
                                                         SyntheticAdaptiveScalingIterableDataset,
                                                         adaptive_scaling_dataset_collate_fn)
from vkit_ocr_model_adaptive_scaling_amd.utils import portable_rng as prng

TWO_PI = 2.0 * math.pi


def f32(rows):
    return rows.view(np.float32)


# ------------------------------------------------------------------------------------------------------------- quad rows
@pytest.mark.parametrize('f,corners,box,centre,frame', [
    (2, [32, 48, 32, 176, 96, 176, 96, 48], [2, 3, 6, 11], [4.0, 7.0], [0.0, 0.25, 0.5, 0.0]),
    (1, [64, 96, 64, 352, 192, 352, 192, 96], [4, 6, 12, 22], [8.0, 14.0], [0.0, 0.125, 0.25, 0.0])], ids=['f2', 'f1'])
def test_row_of_an_axis_aligned_8x4_box(f, corners, box, centre, frame):
    """(y, x) image corners (4, 6) (4, 22) (12, 22) (12, 6): 16 x 8 image pixels, 8 x 4 map pixels at f = 2.  The frame is
    a = (0, 4), b = (2, 0) map pixels at f = 2, so s = dx / 4 and t = dy / 2."""
    quad = np.array(C.rect(4, 6, 12, 22), dtype=np.float64)
    rows, ok = quad_rows(quad[None], 64, 64, f)
    assert ok.tolist() == [True] and rows.shape == (1, 20) and rows.dtype == np.int32
    r = rows[0]
    assert r[:8].tolist() == corners and r[8:12].tolist() == box
    assert f32(r)[12:14].tolist() == centre and f32(r)[14:18].tolist() == frame
    assert f32(r)[18] == 8.0 and r[19] == 1
    # the box is clipped to the map, and may come out empty
    assert quad_rows(quad[None], 5, 9, 2)[0][0, 8:12].tolist() == [2, 3, 4, 8]
    assert quad_rows(quad[None], 2, 64, 2)[0][0, 8:12].tolist() == [2, 3, 1, 11]


def test_row_of_a_box_turned_by_30_degrees():
    """half sides 8 x 3 map pixels about (20.5, 30.25), f = 2: the corners are rint(c * 8), the centre their mean, and M maps
    the side mid-points (of the ROUNDED corners) to (+-1, 0) and (0, +-1)"""
    quad = np.array(C.rot(20.5, 30.25, 8, 3, 30)) * 2
    s30, c30 = 0.5, math.sqrt(3) / 2
    ul = (20.5 - 8 * s30 - 3 * c30, 30.25 - 8 * c30 + 3 * s30)
    assert np.allclose(quad[0] / 2, ul, atol=1e-12)
    rows, ok = quad_rows(quad[None], 48, 64, 2)
    r = rows[0]
    assert ok[0] and r[:8].tolist() == np.rint(quad * 8).astype(int).reshape(-1).tolist()
    q = r[:8].reshape(4, 2) / 16.0
    assert r[8:12].tolist() == [int(q[:, 0].min()), int(q[:, 1].min()), int(q[:, 0].max()), int(q[:, 1].max())]
    c = f32(r)[12:14].astype(np.float64)
    assert np.abs(c - q.mean(0)).max() < 4e-6 and np.abs(c - (20.5, 30.25)).max() < 0.05
    M = f32(r)[14:18].astype(np.float64).reshape(2, 2)
    mids = [(q[1] + q[2]) / 2, (q[2] + q[3]) / 2, (q[3] + q[0]) / 2, (q[0] + q[1]) / 2]  # right, bottom, left, top
    st = np.array([M @ (m - q.mean(0)) for m in mids])
    assert np.abs(st - [(1, 0), (0, 1), (-1, 0), (0, -1)]).max() < 1e-6
    assert abs(float(f32(r)[18]) - 12.0) < 1e-5  # 2 * 3 map pixels = 12 image pixels high


def test_invalid_quads_are_reported_and_not_altered():
    good = C.rect(4, 6, 12, 22)
    bad = {'counter_clockwise': good[::-1], 'bow_tie': [good[0], good[2], good[1], good[3]],
           'zero_area': [(5, 5)] * 4, 'collinear': [(5, 5), (5, 9), (5, 13), (5, 7)],
           'nan': [good[0], (float('nan'), 3.0), good[2], good[3]], 'inf': [good[0], good[1], (float('inf'), 1.0), good[3]],
           'out_of_range': [(4, 6), (4, 2.0e6), (12, 2.0e6), (12, 6)],
           'beyond_int32': [(4, 6), (4, 1.0e12), (12, 1.0e12), (12, 6)]}
    quads = np.array([good] + list(bad.values()) + [good], dtype=np.float64)
    before = quads.copy()
    rows, ok = quad_rows(quads, 64, 64, 2)
    assert np.array_equal(quads, before, equal_nan=True)
    assert ok.tolist() == [True] + [False] * len(bad) + [True]
    assert not rows[1:-1].any() and np.array_equal(rows[0], rows[-1]) and rows[0, 19] == 1
    # +-2^19 itself is in range
    edge = np.array(C.rect(-32768, -32768, 32768, 32768), dtype=np.float64)
    assert quad_rows(edge[None], 64, 64, 1)[1][0] and not quad_rows(edge[None] * 1.0001, 64, 64, 1)[1][0]
    # the oracle skips them
    o, m, hh, s = char_label_maps_host(rows[None, 1:-1], [len(bad)], 64, 64, (0, 63, 0, 63))
    assert not o.any() and not m.any() and not hh.any() and not s.any()


# --------------------------------------------------------------------------------------------------------------- oracle
def independent_fill(quads_map, h, w, sigma=0.5):
    """float64, from the corners themselves (exact in Q4): pixel centres inside by the signs of the cross products, the
    smallest k |F^-1 (p - c)|^2 wins"""
    yy, xx = np.mgrid[0:h, 0:w] + 0.5
    best = np.full((h, w), np.inf)
    owner = np.zeros((h, w), dtype=np.int32)
    for i, q in enumerate(np.asarray(quads_map, dtype=np.float64)):
        inside = np.ones((h, w), dtype=bool)
        for j in range(4):
            e, d = q[(j + 1) % 4] - q[j], np.stack([yy - q[j, 0], xx - q[j, 1]])
            inside &= e[1] * d[0] - e[0] * d[1] >= 0
        F = np.stack([(q[1] + q[2] - q[0] - q[3]) / 4, (q[2] + q[3] - q[0] - q[1]) / 4], axis=1)
        st = np.einsum('ij,jhw->ihw', np.linalg.inv(F), np.stack([yy - q[:, 0].mean(), xx - q[:, 1].mean()]))
        a = (st ** 2).sum(0) / (2 * sigma * sigma)
        take = inside & (a < best)
        best[take], owner[take] = a[take], i + 1
    return owner, np.where(owner > 0, np.exp(-best), 0.0)


def test_oracle_matches_an_independent_fill():
    """corners on the 1/16 grid, no two quads equidistant from a pixel centre"""
    h, w = 40, 72
    g = lambda q: np.rint(np.asarray(q) * 16) / 16
    quads = np.array([g(C.rect(2.5, 3.5, 9.5, 15.5)), g(C.rot(20, 20, 9, 4, 30)), g(C.rot(18, 50, 8, 3, 80)),
                      g(C.rot(22, 24.3, 7, 5, -20)), g(C.rect(-3, 60.25, 6.75, 80)), g(C.rect(30.0625, 5, 30.9375, 30)),
                      g([(30, 40), (31, 58), (38.5, 60), (36, 38.25)])])
    for f in (1, 2):
        rows, ok = quad_rows(quads * f, h, w, f)
        assert ok.all()
        owner, mask, height, score = char_label_maps_host(rows[None], [len(rows)], h, w, (0, h - 1, 0, w - 1))
        ref_owner, ref_score = independent_fill(quads, h, w)
        assert np.array_equal(owner[0], ref_owner)
        assert np.array_equal(mask[0], (ref_owner > 0).astype(np.float32))
        assert np.abs(score[0] - ref_score).max() < 2e-6  # float32 a: a few ulp of values up to ~4
        hq = 0.5 * (np.linalg.norm(quads[:, 3] - quads[:, 0], axis=1) + np.linalg.norm(quads[:, 2] - quads[:, 1], axis=1)) * f
        assert np.array_equal(height[0], np.concatenate([[0.0], hq]).astype(np.float32)[ref_owner])
        # the crop is a window of the full maps
        box = (3, 34, 5, 68)
        crop = char_label_maps_host(rows[None], [len(rows)], h, w, box)
        for full, part in zip((owner, mask, height, score), crop):
            assert np.array_equal(part, full[:, 3:35, 5:69])


def test_owner_rule_and_edge_cases_of_the_scenes():
    c = C.case('one_tile')
    owner, mask, height, score = (a[0] for a in c['ref'])
    assert set(np.unique(owner)) == {0, 1, 3, 4, 5, 8, 9, 13, 14}  # 2 = the twin of 1; 6, 7 thin; 10, 11, 12 outside
    assert (owner[2:8, 2:11] == 1).all()
    assert owner[12, 8] == 3 and owner[12, 7] == 3 and owner[12, 9] == 4  # column 8 is equidistant: the lower index
    assert (owner[[2, 2, 6, 6], [20, 27, 20, 27]] == 5).all() and owner[1, 20] == 0 and owner[2, 19] == 0
    assert not owner[10, 20:30].any() and not owner[8:14, 30].any()  # thinner than a pixel, no centre inside
    assert owner[0, 40] == 8 and owner[15, 60] == 9  # partly outside the map
    assert np.array_equal(mask, (owner > 0).astype(np.float32)) and ((score > 0) == (owner > 0)).all()
    # two identical quads with different heights: the first one's height everywhere
    rows = c['rows'][:, :2].copy()
    f32(rows)[0, 1, 18] = 99.0
    o, _, hh, _ = char_label_maps_host(rows, [2], 16, 64, (0, 15, 0, 63))
    assert set(np.unique(o)) == {0, 1} and set(np.unique(hh)) == {0.0, 6.0}
    rows[0, 0, 19] = 0  # ... until it is marked invalid
    o, _, hh, _ = char_label_maps_host(rows, [2], 16, 64, (0, 15, 0, 63))
    assert set(np.unique(o)) == {0, 2} and set(np.unique(hh)) == {0.0, 99.0}
    # a quad of the second table chunk beats one of the first on a pixel both contain
    t = C.case('two_chunks')
    assert t['ref'][0][0, 5, 7] == 281
    assert char_label_maps_host(t['rows'][:, :1], [1], t['h'], t['w'], t['box'])[0][0, 5, 7] == 1
    # count is clamped, and an empty image gives zero maps
    b = C.case('batch3')
    assert not b['ref'][0][1].any() and b['ref'][0][0].any() and b['ref'][0][2].any()
    over = char_label_maps_host(b['rows'], [99, -4, 14], b['h'], b['w'], b['box'])
    assert np.array_equal(over[0][0], char_label_maps_host(b['rows'], [14, 0, 14], b['h'], b['w'], b['box'])[0][0])
    assert not over[0][1].any()


# --------------------------------------------------------------------------------------------------------- label points
def build_polygon(p, offsets, angles, distances):
    """precise_build_polygon (:399-465) in float64 on one label row: (4, 2) up-left, up-right, down-right, down-left"""
    out = [p + offsets]
    theta = np.mod(np.arctan2(offsets[0], offsets[1]), TWO_PI)
    for k in range(3):
        theta = np.mod(theta + angles[k] * TWO_PI, TWO_PI)
        out.append(p + np.array([np.sin(theta), np.cos(theta)]) * distances[k])
    return np.array(out)


def seeded_quads(n, seed=5):
    """convex quads about (60, 80) map pixels: turned boxes of half sides 8..30 x 8..20 with every corner moved by up to a
    tenth of the smaller half side"""
    u = prng.uniform(seed, 0, n * 13).reshape(n, 13)
    quads = []
    for r in u:
        hw, hh = 8 + 22 * r[0], 8 + 12 * r[1]
        q = np.array(C.rot(60 + 10 * (r[2] - 0.5), 80 + 10 * (r[3] - 0.5), hw, hh, 160 * (r[4] - 0.5)))
        quads.append(q + (r[5:13].reshape(4, 2) - 0.5) * 0.2 * min(hw, hh))
    return np.array(quads)


def test_label_points_round_trip_on_200_quads():
    h, w, f, box, P = 120, 160, 2, (10, 109, 10, 149), 3
    worst = 0.0
    for i, q in enumerate(seeded_quads(200)):
        rows, ok = quad_rows(q[None] * f, h, w, f)
        assert ok[0], i
        lp = label_points(q[None] * f, ok, h, w, f, box, P, rng_seed=11, rng_stream=i)
        for j in range(P):
            p = np.array([lp['downsampled_label_point_y'][j], lp['downsampled_label_point_x'][j]], dtype=np.float64) * f
            got = build_polygon(p, lp['up_left_offsets'][j].astype(np.float64), lp['corner_angles'][j],
                                lp['corner_distances'][j])
            want = q * f
            assert np.abs(got[0] - want[0]).max() < 1.0, (i, j)
            for k in (1, 2, 3):
                d = lp['corner_distances'][j][k - 1]
                err = np.abs(got[k] - want[k]).max()
                worst = max(worst, err / (1 + d))
                assert err <= 1e-6 * (1 + d), (i, j, k, err)
            assert abs(lp['corner_angles'][j].sum() - 1.0) < 1e-6, (i, j)
            assert (lp['corner_angles'][j] > 0).all()
    assert worst < 1e-6


def _scene_quads():
    """12 boxes on a 64 x 128 map (f = 2), three of them without a usable centroid point: outside the core box, invalid,
    and far outside the map"""
    quads = [C.rect(12 + 14 * (i // 4), 14 + 26 * (i % 4), 22 + 14 * (i // 4), 34 + 26 * (i % 4)) for i in range(9)]
    quads += [C.rect(1, 1, 9, 12), C.rect(30, 30, 40, 50)[::-1], C.rect(200, 200, 210, 220)]
    return np.array(quads, dtype=np.float64) * 2


def test_label_point_counts_and_reproducibility():
    h, w, f, box = 64, 128, 2, (10, 53, 10, 117)
    quads = _scene_quads()
    rows, ok = quad_rows(quads, h, w, f)
    assert ok.tolist() == [True] * 10 + [False, True]
    for P in (4, 9, 30):  # u = 9: fewer, as many, more
        a = label_points(quads, ok, h, w, f, box, P, rng_seed=3)
        b = label_points(quads, ok, h, w, f, box, P, rng_seed=3)
        assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
        assert all(len(v) == P for v in a.values())
        assert a['up_left_offsets'].dtype == np.int64 and a['downsampled_label_point_y'].dtype == np.int64
        qi = a['quad_index']
        assert set(qi) <= set(range(9)) and len(set(qi[:9])) == min(P, 9)  # a permutation of the usable quads, cycled
        if P > 9:
            assert np.array_equal(qi, qi[:9][np.arange(P) % 9])
        ys, xs = a['downsampled_label_point_y'], a['downsampled_label_point_x']
        assert (ys >= box[0]).all() and (ys <= box[1]).all() and (xs >= box[2]).all() and (xs <= box[3]).all()
        centres = np.floor(quads[qi].mean(1) / f).astype(np.int64)
        assert np.array_equal(np.stack([ys, xs], 1)[:9], centres[:9])  # the first pass takes the centroid points
        for j in range(P):  # every origin lies strictly inside its quad
            q, py, px = quads[qi[j]], ys[j] * f, xs[j] * f
            assert q[0, 0] < py < q[2, 0] and q[0, 1] < px < q[2, 1]
    far = label_points(quads, ok, h, w, f, box, 30, rng_seed=3)
    assert len(set(zip(far['downsampled_label_point_y'][9:], far['downsampled_label_point_x'][9:]))) > 9  # deviated
    other = label_points(quads, ok, h, w, f, box, 30, rng_seed=4)
    assert not np.array_equal(other['downsampled_label_point_x'], far['downsampled_label_point_x'])
    with pytest.raises(ValueError):
        label_points(quads[9:], ok[9:], h, w, f, box, 4, rng_seed=3)
    with pytest.raises(ValueError):
        label_points(np.zeros((0, 4, 2)), np.zeros((0,), bool), h, w, f, box, 4, rng_seed=3)


# -------------------------------------------------------------------------------------------------------------- collate
def quad_pairs(B=3, H=96, W=128):
    quads = (np.array([C.rect(14, 14, 22, 30), C.rot(30, 40, 8, 4, 25), C.rect(12, 42, 20, 52)], dtype=np.float64) * 2)
    img = lambda i: prng.integers(9, i, H * W * 3, 0, 256).reshape(H, W, 3).astype(np.uint8)
    return [(QuadSample(img(2 * i), quads[:i], index=i, rng_state={'i': i}),
             QuadSample(img(2 * i + 1), quads[:i + 1], index=i, rng_state={'i': i})) for i in range(B)]


def test_collated_batch_has_the_schema_of_the_synthetic_source():
    B, P = 3, 7
    ds = SyntheticAdaptiveScalingIterableDataset(B, (96, 128), num_label_points=P)
    want = adaptive_scaling_dataset_collate_fn(ds.sample(i) for i in range(B))
    batch = adaptive_scaling_quads_collate_fn(quad_pairs(B), P=P, f=2, margin=10, rng_seed=5)
    for part in ('rough', 'precise'):
        t = batch[part]
        assert t['char_quad_rows'].dtype == torch.int32 and t['char_quad_count'].dtype == torch.int32
        assert t['char_quad_rows'].shape == (B, 2 if part == 'rough' else 3, 20)
        assert t['char_quad_count'].tolist() == ([0, 1, 2] if part == 'rough' else [1, 2, 3])
        assert set(t) == (set(want[part]) - {'downsampled_mask', 'downsampled_score_map'}) | {'char_quad_rows',
                                                                                             'char_quad_count'}
    got = char_labels_host(batch)
    assert set(got) == set(want)
    for part in ('rough', 'precise'):
        assert list(got[part]) != [] and set(got[part]) == set(want[part])
        for k, v in want[part].items():
            g = got[part][k]
            if torch.is_tensor(v):
                assert torch.is_tensor(g) and g.dtype == v.dtype and g.shape == v.shape, (part, k)
            else:
                assert type(g) is type(v), (part, k)
        assert got[part]['downsampled_shape'] == want[part]['downsampled_shape']
        assert got[part]['downsampled_core_box'] == want[part]['downsampled_core_box']
        assert got[part]['rng_states'] == [{'i': i} for i in range(B)]
    r, p = got['rough'], got['precise']
    assert not r['downsampled_mask'][0].any() and r['downsampled_mask'][1].any()  # a rough sample without characters
    assert set(np.unique(r['downsampled_score_map'].numpy())) == {0.0, 16.0}  # heights in image pixels: 8 map pixels
    assert float(p['downsampled_score_map'].max()) <= 1.0 and float(p['downsampled_score_map'].max()) > 0.9
    assert torch.equal(p['image'][1], torch.from_numpy(quad_pairs(B)[1][1].image.transpose(2, 0, 1).astype(np.float32)))
    again = adaptive_scaling_quads_collate_fn(quad_pairs(B), P=P, f=2, margin=10, rng_seed=5)
    assert all(torch.equal(again['precise'][k], batch['precise'][k]) for k in batch['precise'] if torch.is_tensor(batch['precise'][k]))
    with pytest.raises(ValueError):  # a precise sample without a usable quad
        adaptive_scaling_quads_collate_fn([(quad_pairs(1)[0][0], quad_pairs(1)[0][0])], P=P)


# ------------------------------------------------------------------------------------------------ labels meet inference
def test_score_map_of_separated_quads_has_one_peak_per_quad_at_its_centroid():
    """the config defaults of precise_infer_char_polygons: threshold 0.7, maximum filter 5"""
    m = C.MEET
    quads = np.array(m['quads'], dtype=np.float64) * m['f']
    rows, ok = quad_rows(quads, m['h'], m['w'], m['f'])
    assert ok.all()
    _, _, _, score = char_label_maps_host(rows[None], [len(rows)], m['h'], m['w'], m['box'])
    want = np.floor(quads.mean(1) / m['f']).astype(np.int64) - (m['box'][0], m['box'][2])
    got = peaks(score[0], 0.7, 5)
    assert sorted(map(tuple, got)) == sorted(map(tuple, want))


# ------------------------------------------------------------------------------------------------------ argument checks
def test_c_entry_point_validates_before_launch():
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    lib = _lib.lib
    rows = np.zeros((1, 1, 20), dtype=np.int32)
    count = np.zeros((1,), dtype=np.int32)
    out = np.zeros((16,), dtype=np.float32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)

    def call(B=1, K=1, h=4, w=4, up=0, left=0, CH=4, CW=4, k=2.0, outs=(None, P(out), None, None)):
        return lib.vkas_char_label_maps(P(rows), P(count), B, K, h, w, up, left, CH, CW, k, *outs, None)
    for bad in (dict(K=-1), dict(B=-1), dict(B=70000, h=1, w=1, CH=1, CW=1), dict(B=8, h=16384, w=16384),
                dict(h=0), dict(up=1), dict(left=-1), dict(CH=5), dict(CW=0), dict(up=2, CH=3), dict(k=0.0),
                dict(k=float('nan')), dict(k=float('inf')), dict(outs=(None, None, None, None))):
        assert call(**bad) == -1, bad  # VKAS_E_ARG
        assert lib.vkas_last_error()


def test_ops_char_label_maps_validates_before_launch():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    rows, count = torch.zeros((2, 3, 20), dtype=torch.int32), torch.zeros((2,), dtype=torch.int32)
    box = (0, 3, 0, 3)
    for args in ((rows[:, :, :19], count, 4, 4, box), (rows[0], count, 4, 4, box), (rows, count[:1], 4, 4, box),
                 (rows.long(), count, 4, 4, box), (rows, count.long(), 4, 4, box), (rows, count, 4, 4, (0, 4, 0, 3)),
                 (rows, count, 4, 4, (2, 1, 0, 3)), (rows, count, 0, 4, box), (rows, count, 1 << 15, 1 << 15, box)):
        with pytest.raises(ValueError):
            ops.char_label_maps(*args)
    with pytest.raises(ValueError):
        ops.char_label_maps(rows, count, 4, 4, box, sigma=0.0)
    with pytest.raises(RuntimeError):  # host tensors: no CPU fallback
        ops.char_label_maps(rows, count, 4, 4, box)
