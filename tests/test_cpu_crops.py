"""dataset/crops.py on the host: the crop rows (reproducible, in bounds, the precise scale, the round trip), ``crop_host``
against ``warp_host`` and against hand-made cases, the photometric rule, labels meeting pixels through a crop, the collated
schema and the argument errors.  The device kernel is held to ``crop_host`` in tests/test_gpu_crops.py."""
import math

import numpy as np
import pytest
import torch

from tests import crop_cases as C
from vkit_ocr_model_adaptive_scaling_amd.dataset import (AnnotatedPage, CropConfig, QuadSample, adaptive_scaling_pages_collate_fn,
                                                         adaptive_scaling_quads_collate_fn, affine_row, check_crop_rows,
                                                         crop_draw, crop_host, crop_quads, crop_row, crops_host, label_points,
                                                         quad_rows)
from vkit_ocr_model_adaptive_scaling_amd.dataset.crops import noise_unit, page_positions
from vkit_ocr_model_adaptive_scaling_amd.inferencing.orient import warp_log2n
from vkit_ocr_model_adaptive_scaling_amd.inferencing.packing import remap_polygons_affine, warp_host


def seeded_page(i):
    """page i of the 200: its size, character height and count vary; the image is not looked at"""
    rng = np.random.default_rng([11, i])
    h, w = int(rng.integers(60, 4000)), int(rng.integers(60, 4000))
    n = int(rng.integers(1, 6))
    ch = float(np.exp(rng.uniform(np.log(2.0), np.log(600.0))))  # 2 .. 600 px: both clamps act somewhere
    quads = [C.parallelogram(rng.uniform(0, h), rng.uniform(0, w), 0.4 * ch * rng.uniform(0.5, 1.5), ch / 2,
                             rng.uniform(-20, 20), rng.uniform(-0.3, 0.3)) for _ in range(n)]
    return AnnotatedPage(np.zeros((h, w, 3), np.uint8), np.array(quads), i)


def quad_height(q):
    return 0.5 * (np.hypot(*(q[3] - q[0])) + np.hypot(*(q[2] - q[1])))


def test_rows_are_reproducible_and_in_bounds():
    cfg = CropConfig()
    lo, hi = 65536 / 8 - 1, 65536 * 8 + 1
    for i in range(200):
        page = seeded_page(i)
        for kind in ('rough', 'precise'):
            row = crop_row(kind, page, cfg, 5, draw=2)
            assert row.dtype == np.int64 and row.shape == (16,)
            assert np.array_equal(row, crop_row(kind, seeded_page(i), cfg, 5, draw=2))
            assert not np.array_equal(row[:7], crop_row(kind, page, cfg, 5, draw=3)[:7])
            check_crop_rows(row[None], [page.image.shape[:2]])
            d = crop_draw(kind, page, cfg, 5, draw=2)
            assert row[7] == warp_log2n(d['scale']) and cfg.scale_min <= d['scale'] <= cfg.scale_max
            assert abs(d['theta']) <= math.radians(cfg.rotate_max_deg)
            # R(theta) / s: the diagonal within the bounds, the off-diagonal below sin(5 degrees) of them
            assert lo * math.cos(math.radians(5)) - 1 <= row[3] <= hi and row[3] == row[6] and row[4] == -row[5]
            assert lo <= math.hypot(row[3], row[4]) <= hi
    rough, precise = (crop_row(k, seeded_page(0), cfg, 5) for k in ('rough', 'precise'))
    assert not np.array_equal(rough[8:], precise[8:])  # the kinds draw from different streams


def test_precise_scale_anchor_and_label_points():
    cfg = CropConfig(size=(256, 320))
    H, W = cfg.size
    f, margin = 2, 10
    jl, jh = cfg.scale_jitter
    clamped = free = 0
    for i in range(200):
        page = seeded_page(i)
        d = crop_draw('precise', page, cfg, 9)
        row = crop_row('precise', page, cfg, 9)
        moved = crop_quads(page.quads, row)
        a = d['anchor']
        before, after = quad_height(page.quads[a]), quad_height(moved[a])
        if d['clamped']:
            clamped += 1
            assert d['scale'] in (cfg.scale_min, cfg.scale_max)
            assert abs(after / before - d['scale']) <= 1e-3 * d['scale']
        else:
            free += 1
            assert cfg.precise_char_height * jl * (1 - 1e-3) <= after <= cfg.precise_char_height * jh * (1 + 1e-3)
        c = moved[a].mean(axis=0)
        cy, cx = math.floor(c[0] / f), math.floor(c[1] / f)
        assert margin <= cy <= H // f - margin - 1 and margin <= cx <= W // f - margin - 1
        width = 0.5 * (np.hypot(*(moved[a][1] - moved[a][0])) + np.hypot(*(moved[a][2] - moved[a][3])))
        if min(after, width) >= 10:  # the centroid pixel's origin, under 3 px from the centroid, lies strictly inside
            _, ok = quad_rows(moved, H // f, W // f, f)
            assert ok[a]
            pts = label_points(moved, ok, H // f, W // f, f, (margin, H // f - margin - 1, margin, W // f - margin - 1), 6, 9)
            assert len(pts['quad_index']) == 6
    assert clamped >= 10 and free >= 100


def test_round_trip_through_the_integer_map():
    cfg = CropConfig(size=(512, 512))
    for i in range(0, 200, 4):
        page = seeded_page(i)
        for kind in ('rough', 'precise'):
            row = crop_row(kind, page, cfg, 3)
            moved = crop_quads(page.quads, row)
            warp = np.array([0, 0, 512, 512, *row[1:7].tolist(), row[7], 0], np.int64)
            assert np.abs(remap_polygons_affine(moved, warp) - page.quads).max() <= 1e-6
            assert np.array_equal(remap_polygons_affine(moved, warp), page_positions(moved, row))
    # the centre of the crop is the drawn centre, to the rounding of the anchor words (2^-17)
    d, row = crop_draw('rough', page, cfg, 3), crop_row('rough', page, cfg, 3)
    assert np.abs(page_positions(np.array([256.0, 256.0]), row) - d['centre']).max() <= 2.0 ** -16


def test_identity_row_returns_the_source_crop():
    src = C.image(7, 40, 50)
    row = affine_row((32, 64), 1.0, 0.0, (16 + 5, 32 + 7))       # the crop's up-left corner at page position (5, 7)
    assert row[1:8].tolist() == [5 * 65536, 7 * 65536, 65536, 0, 0, 65536, 0]
    out = crop_host([src], row[None], (32, 64))
    want = np.zeros((3, 32, 64), np.float32)
    want[:, :32, :43] = src[5:37, 7:50].transpose(2, 0, 1)
    assert out.dtype == np.float32 and np.array_equal(out[0], want)
    row = affine_row((32, 64), 1.0, 0.0, (16 - 3, 32 - 60))      # up-left at (-3, -60): zeros above and to the left
    want = np.zeros((3, 32, 64), np.float32)
    want[:, 3:, 60:] = src[:29, :4].transpose(2, 0, 1)
    assert np.array_equal(crop_host([src], row[None], (32, 64))[0], want)


@pytest.mark.parametrize('name', C.CASES)
def test_geometry_is_warp_host(name):
    c = C.case(name)
    H, W = c['size']
    seen = set()
    for b, row in enumerate(c['rows']):
        off = row.copy()
        off[8:11], off[11:15] = 0x3F800000, 0                     # gains 1, bias and amplitude 0
        got = crop_host(c['sources'], off[None], c['size'])[0]
        warp = np.array([[0, 0, H, W, *row[1:7].tolist(), row[7], 0]], np.int64)
        want = warp_host(c['sources'][int(row[0])], warp, np.zeros((H, W, 3), np.uint8))
        assert np.array_equal(got, want.transpose(2, 0, 1).astype(np.float32)), (name, b)
        seen.add(int(row[7]))
    if name == 'one_tile':
        assert seen == {0, 1, 2, 3}


def test_photometric_rule():
    src = C.image(8, 64, 64)
    size = (64, 64)
    geo = affine_row(size, 1.0, 0.0, (32.0, 32.0))
    v = crop_host([src], geo[None], size)[0]
    assert np.array_equal(v, src.transpose(2, 0, 1).astype(np.float32))
    key = 0x0123456789ABCDEF
    r = noise_unit(key, (3, 64, 64))
    assert r.dtype == np.float32 and r.min() >= -1.0 and r.max() < 1.0
    assert np.array_equal(r * 2.0 ** 23, np.round(r * 2.0 ** 23))
    for amp in (1.0, 8.0):
        for c in range(3):  # uniform in [-1, 1): variance 1/3; four standard errors of the mean of 4096 samples
            assert abs(float((np.float32(amp) * r[c]).mean(dtype=np.float64))) <= 4 * amp / math.sqrt(3 * 4096)
    assert not np.array_equal(r, noise_unit(key + 1, (3, 64, 64)))
    # gain 0: clamp(bias + amp * r), whatever the pixels
    row = affine_row(size, 1.0, 0.0, (32.0, 32.0), gain=(0, 0, 0), bias=(4.0, 128.0, 252.0), noise_amp=8.0, noise_key=key)
    out = crop_host([src], row[None], size)[0]
    bias = np.array([4.0, 128.0, 252.0], np.float32)[:, None, None]
    want = np.clip(bias + np.float32(8.0) * r, np.float32(0), np.float32(255))
    assert np.array_equal(out, want)
    assert (out[0] == 0).any() and (out[2] == 255).any() and 0 < out[1].min() and out[1].max() < 255
    # the order of the operations: (gain * v + bias) + amp * r, each step rounded to float32
    g, b, amp = np.float32(1.1), np.float32(-12.5), np.float32(6.5)
    row = affine_row(size, 1.0, 0.0, (32.0, 32.0), gain=(g, g, g), bias=(b, b, b), noise_amp=amp, noise_key=key)
    t = ((g * v).astype(np.float32) + b).astype(np.float32) + (amp * r).astype(np.float32)
    assert np.array_equal(crop_host([src], row[None], size)[0], np.clip(t, np.float32(0), np.float32(255)))
    # photometric off in the config: gains 1, bias and amplitude 0
    page = AnnotatedPage(src, np.zeros((0, 4, 2)), 0)
    off = crop_row('rough', page, CropConfig(size=size, photometric=False), 1)
    assert off[8:15].tolist() == [0x3F800000] * 3 + [0] * 4
    on = crop_row('rough', page, CropConfig(size=size), 1)
    assert np.array_equal(on[:8], off[:8]) and not np.array_equal(on[8:15], off[8:15])


@pytest.mark.parametrize('scale', [0.5, 1.0, 2.0])
@pytest.mark.parametrize('deg', [-5.0, 5.0])
def test_labels_meet_pixels(scale, deg):
    """an inverted or transposed map would paint the dark characters somewhere else than the transformed quads"""
    quads = np.array([C.parallelogram(60, 50, 14, 20, 10, 0.2), C.parallelogram(70, 120, 10, 24, -15, -0.1),
                      C.parallelogram(140, 60, 30, 12, 5, 0.3), C.parallelogram(150, 150, 16, 16, 40, 0.0)])
    page = C.painted_page(200, 220, quads)
    size = (128, 160)
    row = affine_row(size, scale, math.radians(deg), (100.0, 90.0))
    out = crop_host([page], row[None], size)[0]
    moved = crop_quads(quads, row)
    py, px = np.mgrid[0:size[0], 0:size[1]] + 0.5
    core = np.zeros(size, bool)
    near = np.zeros(size, bool)
    for q in moved:
        core |= C.inside(q, py, px, -2.0)
        near |= C.inside(q, py, px, 2.0)
    src_pos = page_positions(np.stack([py, px], axis=-1), row)
    m = 1.0 + 1.0 / scale  # page pixels a crop pixel reaches from its centre: its sub-samples (under 1 / scale) and a tap
    on_page = ((src_pos[..., 0] >= m) & (src_pos[..., 0] <= 200 - m) & (src_pos[..., 1] >= m) & (src_pos[..., 1] <= 220 - m))
    off_page = ((src_pos[..., 0] < -m) | (src_pos[..., 0] > 200 + m) | (src_pos[..., 1] < -m) | (src_pos[..., 1] > 220 + m))
    assert core.sum() > 200 and (~near & on_page).sum() > 1000
    assert (out[:, core] < 64).all()
    assert (out[:, ~near & on_page] > 192).all()
    assert (out[:, off_page] == 0).all()


def test_collated_schema():
    pages = [C.synthetic_page(i, 150 + 90 * i, 220 + 60 * i, 14 + 8 * i, i) for i in range(3)]
    cfg = CropConfig(size=(128, 160), core_margin=8)
    P = 5
    got = adaptive_scaling_pages_collate_fn([(p, p) for p in pages], cfg, P=P, f=2, margin=4, rng_seed=21)
    samples = [QuadSample(np.zeros((128, 160, 3), np.uint8), crop_quads(p.quads, r.numpy()), p.index)
               for p, r in zip(pages, got['precise']['crop_rows'])]
    want = adaptive_scaling_quads_collate_fn([(s, s) for s in samples], P=P, f=2, margin=4, rng_seed=21)
    for part in ('rough', 'precise'):
        assert set(got[part]) == (set(want[part]) - {'image'}) | {'crop_rows', 'crop_sources', 'crop_size'}
        for k, v in want[part].items():
            if k == 'image':
                continue
            if torch.is_tensor(v):
                assert got[part][k].dtype == v.dtype and got[part][k].shape[0] == 3 and got[part][k].shape[2:] == v.shape[2:], k
        assert got[part]['crop_rows'].dtype == torch.int64 and tuple(got[part]['crop_rows'].shape) == (3, 16)
        assert got[part]['crop_rows'][:, 0].tolist() == [0, 1, 2] and got[part]['crop_size'] == (128, 160)
        assert all(a is p.image for a, p in zip(got[part]['crop_sources'], pages))
        assert got[part]['downsampled_shape'] == (64, 80)
    # the precise pass of the pages collate IS the quads collate on the transformed quads
    for k, v in want['precise'].items():
        if torch.is_tensor(v) and k != 'image':
            assert torch.equal(got['precise'][k], v), k
    # the host route: the schema TwoPassStep takes once the maps are rasterised, images equal to crop_host's
    host = crops_host(got)
    for part in ('rough', 'precise'):
        assert set(host[part]) == set(want[part])
        assert host[part]['image'].dtype == torch.float32 and tuple(host[part]['image'].shape) == (3, 3, 128, 160)
    ref = crop_host([p.image for p in pages], got['rough']['crop_rows'].numpy(), (128, 160))
    assert np.array_equal(host['rough']['image'].numpy(), ref)
    again = adaptive_scaling_pages_collate_fn([(p, p) for p in pages], cfg, P=P, f=2, margin=4, rng_seed=21, draw=1)
    assert not torch.equal(again['rough']['crop_rows'], got['rough']['crop_rows'])


def test_argument_errors():
    page = C.synthetic_page(0, 120, 160, 16, 0)
    row = crop_row('rough', page, CropConfig(size=(64, 64)), 1)
    shapes = [(120, 160)]
    check_crop_rows(row[None], shapes)

    def bad(word, value):
        r = row.copy()[None]
        r[0, word] = value
        return r
    for word, value in ((0, -1), (0, 1), (3, (1 << 22) + 1), (6, -(1 << 22) - 1), (1, 1 << 40), (2, -(1 << 40)), (7, 4), (7, -1),
                        (8, 0x7F800000), (12, 0x7FC00000), (14, 0xFF800000), (9, 1 << 32), (13, -1)):
        with pytest.raises(ValueError):
            check_crop_rows(bad(word, value), shapes)
    with pytest.raises(ValueError):
        check_crop_rows(row[None, :15], shapes)
    with pytest.raises(ValueError):
        check_crop_rows(row[None].astype(np.float64), shapes)
    with pytest.raises(ValueError):
        check_crop_rows(row[None], [(120, 8193)])
    with pytest.raises(ValueError):
        crop_host([page.image], bad(7, 5), (64, 64))
    assert not crop_host([page.image], bad(0, 3), (64, 64), strict=False).any()   # as the device takes an unchecked table
    empty = AnnotatedPage(page.image, np.zeros((0, 4, 2)), 0)
    flipped = AnnotatedPage(page.image, page.quads[:, ::-1], 0)                   # counter-clockwise: every quad invalid
    for p in (empty, flipped):
        crop_row('rough', p, CropConfig(size=(64, 64)), 1)
        with pytest.raises(ValueError, match='valid quad'):
            crop_row('precise', p, CropConfig(size=(64, 64)), 1)
        with pytest.raises(ValueError):
            adaptive_scaling_pages_collate_fn([(page, p)], CropConfig(size=(64, 64), core_margin=8), P=3, margin=4)
    for size in ((100, 64), (64, 65), (0, 64)):
        with pytest.raises(ValueError, match='multiples of 32'):
            crop_row('rough', page, CropConfig(size=size), 1)
    with pytest.raises(ValueError, match='core_margin'):
        adaptive_scaling_pages_collate_fn([(page, page)], CropConfig(size=(64, 64), core_margin=4), P=3, margin=4)
    with pytest.raises(ValueError):
        crop_row('other', page, CropConfig(size=(64, 64)), 1)
    with pytest.raises(ValueError):
        adaptive_scaling_pages_collate_fn([], CropConfig(size=(64, 64)), P=3)
