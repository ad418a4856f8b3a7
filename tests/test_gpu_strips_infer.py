"""The line strips inside ``infer`` / ``infer_batch`` on the MI355X, on the small untrained model and the three images of
tests/test_gpu_quad_lines_infer.py.

Off (the default) the results equal those of a config that never heard of the feature, field for field, with the new fields
at their defaults.  On without ``precise_char_lines`` raises.  On, every strip equals the host oracle (``quad_strips_host``)
on the result's own ``line_polygons``, ``line_strip_ids`` count through the lines of the images, every other field is what it
is with the switch off, and a batch of one equals ``infer``.  The untrained model's lines are single characters, so lines
of several characters go through ``strips_for_results`` on a hand-made layout, as the lines tests do."""
import attrs
import numpy as np
import pytest
import torch

from tests import quad_line_cases as Q
from tests.test_gpu_infer_oriented import configure
from tests.test_gpu_inferencing import build
from tests.test_gpu_infer_batch import assert_results_equal
from tests.test_gpu_quad_lines_infer import LINE_FIELDS, assert_same_fields, images, same

pytestmark = pytest.mark.gpu

STRIP_FIELDS = ('line_strip_ids', 'line_strips')


def assert_strips_are_the_oracles(strips, imgs, results, what, **kw):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import quad_strips_host
    want = quad_strips_host(imgs, [r.line_polygons for r in results], **kw)
    assert strips.height == want.height and len(strips.buckets) == len(want.buckets), what
    for name in ('image', 'status', 'squeezed', 'widths', 'bucket', 'index', 'rows'):
        assert same(getattr(strips, name), getattr(want, name)), (what, name)
    for a, b in zip(strips.buckets, want.buckets):
        assert a.is_cuda and same(a.cpu().numpy(), b), what
    first = 0
    for k, r in enumerate(results):
        L = len(r.line_polygons)
        assert r.line_strip_ids.dtype == np.int32 and r.line_strip_ids.tolist() == list(range(first, first + L)), (what, k)
        assert (strips.image[first:first + L] == k).all(), (what, k)
        for l, s in enumerate(r.line_strip_ids.tolist()):
            if want.status[s] == 0:
                assert same(strips.strip(s).cpu().numpy(), np.ascontiguousarray(want.strip(s))), (what, k, l)
        first += L
    assert first == len(strips.status), what
    return want


def test_off_is_the_result_without_the_feature_and_on_adds_the_oracles_strips():
    inf, _ = build(torch.float16)
    configure(inf, False)
    imgs = images()
    c = inf.config
    assert (c.precise_line_strips, c.precise_line_strip_height, c.precise_line_strip_width_max, c.precise_line_strip_width_step,
            c.precise_line_strip_margin) == (False, 32, 2048, 64, 0.125)
    c.precise_char_lines = True
    base = [inf.infer(img) for img in imgs]          # the config as it comes: the new fields never touched
    base_batch = inf.infer_batch(imgs)
    assert sum(len(r.line_polygons) for r in base) > 0 and base_batch.line_strips is None
    for r in base + list(base_batch.results):
        assert r.line_strips is None and r.line_strip_ids.shape == (0,) and r.line_strip_ids.dtype == np.int32
    # off: the parameters are not read
    c.precise_line_strip_height, c.precise_line_strip_width_max, c.precise_line_strip_width_step, c.precise_line_strip_margin = \
        0, -1, 0, 7.0
    for k, img in enumerate(imgs):
        assert_same_fields(inf.infer(img), base[k], ('off', k))
    off_batch = inf.infer_batch(imgs)
    for k, r in enumerate(off_batch.results):
        assert_same_fields(r, base_batch.results[k], ('off, batch', k))
    assert off_batch.line_strips is None
    for kw in (dict(height=32, width_max=2048, width_step=64, margin=0.125), dict(height=12, width_max=40, width_step=8, margin=0.5)):
        c.precise_line_strips = True
        c.precise_line_strip_height, c.precise_line_strip_width_max, c.precise_line_strip_width_step, \
            c.precise_line_strip_margin = kw['height'], kw['width_max'], kw['width_step'], kw['margin']
        on = [inf.infer(img) for img in imgs]
        on_batch = inf.infer_batch(imgs)
        assert all(r.line_strips is None for r in on_batch.results)
        assert_strips_are_the_oracles(on_batch.line_strips, imgs, on_batch.results, ('infer_batch', kw), **kw)
        for k, (a, b) in enumerate(zip(on, on_batch.results)):
            assert_same_fields(a, base[k], ('on', k), skip=STRIP_FIELDS)
            assert_same_fields(b, base_batch.results[k], ('on, batch', k), skip=STRIP_FIELDS)
            want = assert_strips_are_the_oracles(a.line_strips, [imgs[k]], [a], ('infer', k, kw), **kw)
            one = inf.infer_batch([imgs[k]])
            assert_results_equal(a, one.results[0], ('a batch of one against infer', k))
            for name in LINE_FIELDS + ('line_strip_ids',):
                assert same(getattr(a, name), getattr(one.results[0], name)), ('a batch of one against infer', k, name)
            assert same(one.line_strips, a.line_strips), ('a batch of one against infer', k)
            print(f'{kw}, image {k}: {len(want.status)} lines, {int((want.status == 0).sum())} strips, widths '
                  f'{sorted(set(want.widths.tolist()))}, {int(want.squeezed.sum())} squeezed')
    c.precise_line_strips = False
    assert_same_fields(inf.infer(imgs[0]), base[0], 'off again')


def test_on_without_lines_raises():
    inf, _ = build(torch.float16)
    configure(inf, False)
    inf.config.precise_line_strips = True
    img = images()[0]
    with pytest.raises(ValueError, match='precise_char_lines'):
        inf.infer(img)
    with pytest.raises(ValueError, match='precise_char_lines'):
        inf.infer_batch([img])


def test_a_hand_made_layout_in_a_result():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import group_results, strips_for_results
    inf, _ = build(torch.float16)
    configure(inf, False)
    imgs = [np.random.default_rng(8).integers(0, 256, (420, 640, 3), dtype=np.uint8), images()[1]]
    base = inf.infer(images()[0])
    sizes = [len(p) for p in base.probs]
    n = sum(sizes)
    assert n >= 45
    # the result keeps its regions; its characters become three lines of n // 3 in scrambled order (and up to two single
    # ones), as in tests/test_gpu_quad_lines_infer.py, here inside the first image (a long line may leave it: zeros)
    quads, truth = Q.layout(3, n // 3, **Q.LATIN, word_space=10.0, angle=0.35, seed=9)
    quads = quads - quads.reshape(-1, 2).min(axis=0) + 20.0
    spare = np.array([Q.SQ(330 + 40 * k, 500, 30, 16) for k in range(n - len(quads))], np.float64).reshape(-1, 4, 2)
    truth = truth + [[len(quads) + k] for k in range(len(spare))]
    quads = np.concatenate([quads, spare])
    cuts = np.cumsum([0] + sizes)
    made = attrs.evolve(base, polygons=[quads[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    empty = attrs.evolve(made, polygons=[q[:0] for q in made.polygons], probs=[p[:0] for p in made.probs],
                         points=[p[:0] for p in made.points])
    grouped = group_results([made, empty])
    assert [m.tolist() for m in grouped[0].line_chars] == truth and len(grouped[1].line_polygons) == 0
    out, strips = strips_for_results(grouped, imgs)
    for a, b in zip(out, grouped):
        assert_same_fields(a, b, 'the step changes line_strip_ids only', skip=('line_strip_ids',))
    want = assert_strips_are_the_oracles(strips, imgs, out, 'hand-made layout')
    assert out[0].line_strip_ids.tolist() == list(range(len(truth))) and out[1].line_strip_ids.shape == (0,)
    assert out[0].line_strips is None and (want.status == 0).all() and (want.widths[:3] > 3 * 32).all(), 'lines of several characters'
    # the strip's frame maps back onto the line's rectangle grown by the margin
    for s in range(3):
        h, w = 32, int(want.widths[s])
        P = out[0].line_polygons[s]
        A, D = ((P[1] - P[0]) + (P[2] - P[3])) / 2, ((P[3] - P[0]) + (P[2] - P[1])) / 2
        ld = np.hypot(*D)
        along, down = np.array([[-1.0], [1.0], [1.0], [-1.0]]), np.array([[-1.0], [-1.0], [1.0], [1.0]])
        grown = P + 0.125 * ld * along * (A / np.hypot(*A)) + 0.125 * down * D
        back = strips.remap(s, np.array([[0, 0], [0, w], [h, w], [h, 0]], np.float64))
        assert np.abs(back - grown).max() <= (w + h) * 2.0 ** -17 + 2.0 ** -16
    other, small = strips_for_results(grouped, imgs, height=16, width_max=64, width_step=16, margin=0.0)
    assert_strips_are_the_oracles(small, imgs, other, 'other parameters', height=16, width_max=64, width_step=16, margin=0.0)
    assert small.squeezed[:3].all() and tuple(small.buckets[-1].shape)[1:] == (16, 64, 3)
