"""dataset/blur.py on the host: the table builders (valid, symmetric, the motion stroke's centroid and axis), the rule of
``crop_blur_host`` (R = 0 is ``crop_host``, constants stay, the impulse response, the halo continues the map), what an
unchecked table gives, the draws (reproducible, off by default, the crop rows untouched, the drawn share), the collated schema
and the argument errors.  The device kernels are held to ``crop_blur_host`` in tests/test_gpu_crop_blur.py."""
import math

import numpy as np
import pytest
import torch

from tests import blur_cases as BC
from tests import crop_cases as C
from tests.test_cpu_crops import seeded_page
from vkit_ocr_model_adaptive_scaling_amd.dataset import (AnnotatedPage, BlurConfig, CropConfig, adaptive_scaling_pages_collate_fn,
                                                         affine_row, blur_draw, blur_row, check_blur_rows, crop_blur_host,
                                                         crop_host, crop_row, crops_host, defocus_blur_row, gaussian_blur_row,
                                                         identity_blur_row, motion_blur_row)

OFFSETS = np.arange(15) - 7


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def table(row):
    return row[1:].astype(np.int64).reshape(15, 15)


def assert_valid(row):
    assert row.dtype == np.int32 and row.shape == (226,)
    r, w = int(row[0]), table(row)
    assert 0 <= r <= 7 and w.min() >= 0 and w.max() <= 65536 and int(w.sum()) == 65536
    far = np.maximum(np.abs(OFFSETS)[:, None], np.abs(OFFSETS)[None, :]) > r
    assert not w[far].any()
    check_blur_rows(row[None])


def test_every_builder_validates_over_its_range():
    assert_valid(identity_blur_row())
    assert int(identity_blur_row()[0]) == 0 and table(identity_blur_row())[7, 7] == 65536
    for sigma in np.linspace(0.5, 2.3, 19).tolist() + [0.1, 7.0 / 3]:
        row = gaussian_blur_row(sigma)
        assert_valid(row)
        assert int(row[0]) == min(7, math.ceil(3 * sigma))
    for rho in np.linspace(1.0, 6.5, 23).tolist() + [0.125, 7.5]:
        row = defocus_blur_row(rho)
        assert_valid(row)
        nz = np.nonzero(table(row))
        assert int(row[0]) == max(np.abs(nz[0] - 7).max(), np.abs(nz[1] - 7).max())  # the smallest radius that holds it
    assert int(defocus_blur_row(7.5)[0]) == 7 and int(defocus_blur_row(1.0)[0]) == 1
    for length in np.linspace(3.0, 15.0, 13).tolist() + [1.0]:
        for angle in np.linspace(0.0, math.pi, 17)[:-1]:
            assert_valid(motion_blur_row(length, angle))
    assert np.array_equal(motion_blur_row(1.0, 0.3), identity_blur_row())


def test_gaussian_and_defocus_tables_have_the_symmetries_of_the_square():
    for row in [gaussian_blur_row(s) for s in (0.5, 1.0, 1.7, 2.3)] + [defocus_blur_row(r) for r in (1.0, 2.6, 4.05, 6.5)]:
        w = table(row)
        assert np.array_equal(w, w.T) and np.array_equal(w, w[::-1]) and np.array_equal(w, w[:, ::-1])  # these generate all 8


def test_motion_table_centroid_axis_and_single_row():
    """The stroke is 256 points, symmetric about the centre, splatted bilinearly.  Its covariance is that of the segment,
    ``(l^2 / 12) u u^T`` with ``l = length - 1``, plus what the splat adds - ``diag(f (1 - f))`` averaged, each entry in
    [0, 1/4], i.e. an isotropic part and a deviation of norm at most 1/8 - plus what the quantisation moves to the centre:
    under 2^-16 of weight per non-zero cell, at most 45 cells at a squared distance of at most 98, a norm below 0.07.  A
    symmetric perturbation of norm e turns the principal axis of a matrix with eigenvalue gap g by at most
    ``asin(2 e / g) / 2`` (Davis-Kahan): the bound used below with e = 0.2."""
    for length in (7.0, 11.0, 15.0):
        for angle in (0.0, 0.3, math.pi / 4, 1.2, math.pi / 2, 2.0, 2.9):
            w = table(motion_blur_row(length, angle)) / 65536.0
            cy, cx = float((w.sum(axis=1) * OFFSETS).sum()), float((w.sum(axis=0) * OFFSETS).sum())
            assert abs(cy) <= 1e-3 and abs(cx) <= 1e-3
            dy, dx = OFFSETS[:, None] - cy, OFFSETS[None, :] - cx
            cov = np.array([[(w * dy * dy).sum(), (w * dy * dx).sum()], [(w * dy * dx).sum(), (w * dx * dx).sum()]])
            vals, vecs = np.linalg.eigh(cov)
            axis = math.atan2(vecs[0, 1], vecs[1, 1]) % math.pi      # the eigenvector of the larger eigenvalue, as (y, x)
            off = abs(axis - angle % math.pi)
            gap = (length - 1.0) ** 2 / 12
            assert min(off, math.pi - off) <= 0.5 * math.asin(min(1.0, 2 * 0.2 / gap)), (length, angle)
    for length in (3, 8, 15):
        w = table(motion_blur_row(float(length), 0.0))
        assert not w[np.arange(15) != 7].any() and np.array_equal(np.nonzero(w[7])[0], np.arange(15)[np.abs(OFFSETS) <= length // 2])


@pytest.mark.parametrize('name', C.CASES)
def test_radius_zero_is_crop_host(name):
    c = C.case(name)
    blur = np.stack([identity_blur_row()] * len(c['rows']))
    assert np.array_equal(bits(crop_blur_host(c['sources'], c['rows'], blur, c['size'])), bits(c['ref']))


def test_a_constant_seen_wholly_inside_stays_constant():
    page = np.empty((120, 220, 3), np.uint8)
    page[:] = (137, 5, 255)
    size = (16, 64)   # at scale 1/2 and 5 degrees the cells -7 .. 70 reach 80 + 7 page pixels from the centre: inside
    rows = np.stack([affine_row(size, 1.0, math.radians(5), (60.0, 110.0), **C.PHOTO['off']),
                     affine_row(size, 0.5, math.radians(-5), (60.0, 110.0), **C.PHOTO['noise'])])
    for blur in (gaussian_blur_row(2.3), defocus_blur_row(7.0), motion_blur_row(15.0, 0.4), BC.radius_row(7, 9)):
        out = crop_blur_host([page], rows, np.stack([blur, blur]), size)
        assert np.array_equal(out[0], np.broadcast_to(np.array([137, 5, 255], np.float32)[:, None, None], (3,) + size))
        assert np.array_equal(bits(out), bits(crop_host([page], rows, size)))      # the jitter sees the same exact value


def test_the_impulse_reproduces_the_mirrored_table():
    page = np.zeros((40, 50, 3), np.uint8)
    page[20, 30] = 255
    size = (40, 50)
    row = affine_row(size, 1.0, 0.0, (20.0, 25.0))
    assert row[1:8].tolist() == [0, 0, 65536, 0, 0, 65536, 0]
    for blur in (BC.radius_row(7, 11), motion_blur_row(9.0, 0.5), BC.radius_row(3, 12)):
        out = crop_blur_host([page], row[None], blur[None], size)[0]
        want = np.zeros(size, np.float32)
        want[13:28, 23:38] = (255 * table(blur)[::-1, ::-1]).astype(np.float32) * np.float32(2.0 ** -16)
        for c in range(3):
            assert np.array_equal(out[c], want)


def test_the_halo_continues_the_map():
    """a crop whose windows reach past its edge over the page equals the centre of a larger crop of the same map: the values
    beyond the edge are the page's, neither a clamp nor zeros"""
    src = C.image(21, 80, 120)
    size, big = (16, 64), (30, 78)
    blur = BC.radius_row(7, 13)
    for theta, centre in ((0.0, (40.0, 60.0)), (math.radians(5), (38.5, 61.25)), (math.radians(90), (40.0, 60.0))):
        small = affine_row(size, 0.8, theta, centre)
        large = small.copy()                  # the same map, the origin moved by (-7, -7) cells
        large[1] -= 7 * small[3] + 7 * small[4]
        large[2] -= 7 * small[5] + 7 * small[6]
        got = crop_blur_host([src], small[None], blur[None], size)[0]
        assert np.array_equal(got, crop_blur_host([src], large[None], blur[None], big)[0][:, 7:23, 7:71])
        v = crop_host([src], large[None], big)[0].astype(np.int64)     # the geometric values of the cells -7 .. H + 6, W + 6
        w = table(blur)

        def blurred(v):
            acc = sum(w[7 + a, 7 + b] * v[:, 7 + a:23 + a, 7 + b:71 + b] for a in range(-7, 8) for b in range(-7, 8))
            return acc.astype(np.float32) * np.float32(2.0 ** -16)
        assert np.array_equal(got, blurred(v))
        border = np.zeros_like(v)
        border[:, 7:23, 7:71] = v[:, 7:23, 7:71]
        assert np.abs(got - blurred(border)).max() > 20                # a zero border of the crop would darken its rim


def invalid_rows():
    good = BC.radius_row(3, 14)

    def edit(word, value, fix=None):
        r = good.copy()
        r[word] = value
        if fix is not None:
            r[fix] -= value - good[word]      # the sum stays 65536
        return r
    centre = 1 + 7 * 15 + 7
    return {'radius 9': edit(0, 9), 'radius -1': edit(0, -1), 'radius 8': edit(0, 8), 'sum + 1': edit(centre, good[centre] + 1),
            'sum - 1': edit(centre, good[centre] - 1), 'weight 65537': edit(centre, 65537, centre + 1),
            'weight -1': edit(centre + 1, -1, centre), 'outside the square': edit(1 + 7 * 15 + 11, 5, centre),
            'corner': edit(1, 1, centre)}


def test_an_unchecked_invalid_row_gives_a_zero_image():
    c = BC.case('one_tile')
    good = BC.radius_row(3, 14)
    assert_valid(good)
    for what, bad in invalid_rows().items():
        blur = np.stack([good, bad, good])
        with pytest.raises(ValueError):
            check_blur_rows(blur)
        with pytest.raises(ValueError):
            crop_blur_host(c['sources'], c['rows'][:3], blur, c['size'])
        out = crop_blur_host(c['sources'], c['rows'][:3], blur, c['size'], strict=False)
        assert not out[1].any() and out[0].any() and out[2].any(), what
    rows = np.array(c['rows'][:2])
    rows[1, 0] = 4                                      # a bad crop row, as crop_host takes it
    out = crop_blur_host(c['sources'], rows, np.stack([good, good]), c['size'], strict=False)
    assert out[0].any() and not out[1].any()


def test_draws():
    blur = BlurConfig(prob=0.3)
    on, off, zero = CropConfig(blur=blur), CropConfig(), CropConfig(blur=BlurConfig())
    assert CropConfig().blur is None and BlurConfig().prob == 0.0
    drawn = 0
    for i in range(200):
        page = seeded_page(i)
        for kind in ('rough', 'precise'):
            assert np.array_equal(crop_row(kind, page, on, 5, draw=2), crop_row(kind, page, off, 5, draw=2))  # the first 13
            row = blur_row(kind, page, on, 5, draw=2)
            assert_valid(row)
            assert np.array_equal(row, blur_row(kind, seeded_page(i), on, 5, draw=2))
            d = blur_draw(kind, page, on, 5, draw=2)
            assert d == blur_draw(kind, page, on, 5, draw=2) and 0.0 <= d['angle'] < math.pi
            lo, hi = {'gaussian': blur.gaussian_sigma, 'defocus': blur.defocus_radius, 'motion': blur.motion_length}[d['kind']]
            assert lo <= d['size'] <= hi
            assert d['blur'] == (not np.array_equal(row, identity_blur_row()))
            drawn += d['blur']
            for cfg in (off, zero):
                assert np.array_equal(blur_row(kind, page, cfg, 5, draw=2), identity_blur_row())
    assert drawn > 60
    rough, precise = (blur_draw(k, seeded_page(0), on, 5) for k in ('rough', 'precise'))
    assert rough != precise and rough != blur_draw('rough', seeded_page(0), on, 5, draw=1)


def test_the_drawn_share_and_the_kinds():
    n, prob = 2000, 0.3
    cfg = CropConfig(blur=BlurConfig(prob=prob))
    page = AnnotatedPage(np.zeros((8, 8, 3), np.uint8), np.zeros((0, 4, 2)), 0)
    draws = []
    for i in range(n):
        page.index = i
        draws.append(blur_draw('rough', page, cfg, 77))
    count = sum(d['blur'] for d in draws)
    assert abs(count - n * prob) <= 3 * math.sqrt(n * prob * (1 - prob))
    kinds = [d['kind'] for d in draws]
    for k in ('gaussian', 'defocus', 'motion'):       # equal weights: a third each, within 3 binomial sigma
        assert abs(kinds.count(k) - n / 3) <= 3 * math.sqrt(n * (1 / 3) * (2 / 3))
    only = CropConfig(blur=BlurConfig(prob=1.0, kind_weights=(0.0, 1.0, 0.0)))
    assert {blur_draw('rough', AnnotatedPage(page.image, page.quads, i), only, 3)['kind'] for i in range(50)} == {'defocus'}


def test_collated_schema_with_and_without_blur():
    pages = [C.synthetic_page(i, 150 + 90 * i, 220 + 60 * i, 14 + 8 * i, i) for i in range(3)]
    args = dict(P=5, f=2, margin=4, rng_seed=21)
    plain = adaptive_scaling_pages_collate_fn([(p, p) for p in pages], CropConfig(size=(128, 160), core_margin=8), **args)
    zero = adaptive_scaling_pages_collate_fn([(p, p) for p in pages],
                                             CropConfig(size=(128, 160), core_margin=8, blur=BlurConfig(prob=0.0)), **args)
    cfg = CropConfig(size=(128, 160), core_margin=8, blur=BlurConfig(prob=1.0))
    got = adaptive_scaling_pages_collate_fn([(p, p) for p in pages], cfg, **args)
    for part in ('rough', 'precise'):
        assert set(zero[part]) == set(plain[part]) and 'crop_blur' not in plain[part]
        assert set(got[part]) == set(plain[part]) | {'crop_blur'}
        b = got[part]['crop_blur']
        assert b.dtype == torch.int32 and tuple(b.shape) == (3, 226)
        want = np.stack([blur_row(part, p, cfg, 21) for p in pages])
        assert np.array_equal(b.numpy(), want) and (b[:, 0] > 0).all()
        check_blur_rows(b.numpy())
        for k, v in plain[part].items():       # everything else is what it is without blur
            if torch.is_tensor(v):
                assert torch.equal(got[part][k], v), (part, k)
    host, host_plain = crops_host(got), crops_host(plain)
    for part in ('rough', 'precise'):
        assert set(host[part]) == set(host_plain[part]) and 'crop_blur' not in host[part]
        ref = crop_blur_host([p.image for p in pages], got[part]['crop_rows'].numpy(), got[part]['crop_blur'].numpy(), (128, 160))
        assert np.array_equal(bits(host[part]['image'].numpy()), bits(ref))
        assert not np.array_equal(host[part]['image'].numpy(), host_plain[part]['image'].numpy())


def test_argument_errors():
    good = BC.radius_row(2, 15)
    for bad in (good[None, :225], good[None].astype(np.float64), good, np.stack([good, good]).astype(np.int64) + (1 << 40)):
        with pytest.raises(ValueError):
            check_blur_rows(bad)
    assert check_blur_rows(good[None].astype(np.int64)).dtype == np.int32
    for call in (lambda: gaussian_blur_row(0.0), lambda: gaussian_blur_row(float('nan')), lambda: defocus_blur_row(0.05),
                 lambda: defocus_blur_row(7.6), lambda: motion_blur_row(15.5, 0.0), lambda: motion_blur_row(0.5, 0.0),
                 lambda: BlurConfig(prob=1.5).check(), lambda: BlurConfig(prob=-0.1).check(),
                 lambda: BlurConfig(kind_weights=(0.0, 0.0, 0.0)).check(), lambda: BlurConfig(kind_weights=(1.0, -1.0, 1.0)).check(),
                 lambda: BlurConfig(gaussian_sigma=(0.5, 2.5)).check(), lambda: BlurConfig(defocus_radius=(1.0, 8.0)).check(),
                 lambda: BlurConfig(motion_length=(3.0, 16.0)).check(), lambda: BlurConfig(motion_length=(5.0, 3.0)).check(),
                 lambda: CropConfig(blur=BlurConfig(prob=2.0)).check()):
        with pytest.raises(ValueError):
            call()
    c = BC.case('one_tile')
    with pytest.raises(ValueError):
        crop_blur_host(c['sources'], c['rows'], c['blur'][:4], c['size'])
    with pytest.raises(ValueError):
        crop_blur_host(c['sources'], c['rows'], c['blur'], (0, 64))
    page = C.synthetic_page(0, 120, 160, 16, 0)
    with pytest.raises(ValueError):
        blur_draw('other', page, CropConfig(blur=BlurConfig(prob=1.0)), 1)
    with pytest.raises(ValueError):
        blur_draw('rough', page, CropConfig(blur=BlurConfig(prob=1.0)), 1, draw=-1)


def test_op_argument_errors_come_before_the_device():
    """ops.crop_warp_blur checks its arguments before anything touches the device: on a machine without one the bad calls
    raise ValueError and only a good call reaches the refusal to run on the host."""
    from vkit_ocr_model_adaptive_scaling_amd import ops
    c = BC.case('one_tile')
    m = c['sources'][0]
    arena = torch.from_numpy(np.ascontiguousarray(m).reshape(-1).copy())
    sources = np.array([[0, m.shape[0], m.shape[1], 0]], np.int64)
    rows, blur, size = np.array(c['rows']), np.array(c['blur']), c['size']
    B = len(rows)
    assert ops.crop_blur_work_bytes(B, size, 7) == B * 3 * 30 * 80 and ops.crop_blur_work_bytes(B, size, 0) == B * 3 * 16 * 64
    bad_sum = blur.copy()
    bad_sum[1, 1 + 7 * 15 + 7] += 1
    small = torch.zeros((ops.crop_blur_work_bytes(B, size, 3) - 1,), dtype=torch.uint8)
    calls = [lambda: ops.crop_warp_blur(arena, sources, rows, blur[:4], size),
             lambda: ops.crop_warp_blur(arena, sources, rows, blur[:, :225], size),
             lambda: ops.crop_warp_blur(arena, sources, rows, blur.astype(np.int64), size),
             lambda: ops.crop_warp_blur(arena, sources, rows, bad_sum, size),
             lambda: ops.crop_warp_blur(arena, sources, rows, blur, size, radius_max=8),
             lambda: ops.crop_warp_blur(arena, sources, rows, blur, size, radius_max=-1),
             lambda: ops.crop_warp_blur(arena, sources, rows, blur, size, radius_max=2.5),
             lambda: ops.crop_warp_blur(arena, sources, rows, blur, size, radius_max=2),       # the table holds a radius 3
             lambda: ops.crop_warp_blur(arena, sources, rows, blur, size, work=small),
             lambda: ops.crop_warp_blur(arena, sources, rows, blur, size, work=torch.zeros((1 << 20,), dtype=torch.int8)),
             lambda: ops.crop_warp_blur(arena, sources, rows[:, :12], blur, size),
             lambda: ops.crop_warp_blur(arena, sources, rows, blur, (16, 8193)),
             lambda: ops.crop_warp_blur(arena.view(1, -1), sources, rows, blur, size)]
    for k, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f'call {k} did not raise')
    assert int(blur[:, 0].max()) == 3
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.crop_warp_blur(arena, sources, rows, blur, size)
    with pytest.raises(RuntimeError, match='MI355X'):   # all radii 0 on the host: crop_warp's refusal, the same words
        ops.crop_warp_blur(arena, sources, rows, np.stack([identity_blur_row()] * B), size)
