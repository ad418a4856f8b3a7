"""The curved line strips inside ``infer`` / ``infer_batch`` on the MI355X, on the small untrained model and the three images
of tests/test_gpu_quad_lines_infer.py.

Off (the default) the results equal those of a config that never heard of the feature, field for field, with the new field
at its default.  On without ``precise_line_strips`` raises.  On, ``line_strips`` is a ``SpineStrips`` that equals the host
oracle (``spine_strips_host``) on the result's own lines, ``line_spines`` are its spines, every other field is what it is with
the switch off (``line_polygons`` included), also after the suppression, and a batch of one equals ``infer``.  The untrained
model's lines are single characters, so a hand-made arc goes through ``group_results`` and ``spine_strips_for_results`` in
a result, as the lines tests do."""
import attrs
import numpy as np
import pytest
import torch

from tests import spine_cases as P
from tests.test_gpu_infer_oriented import configure
from tests.test_gpu_inferencing import build
from tests.test_gpu_infer_batch import assert_results_equal
from tests.test_gpu_quad_lines_infer import LINE_FIELDS, assert_same_fields, images, same

pytestmark = pytest.mark.gpu

SPINE_FIELDS = ('line_strip_ids', 'line_strips', 'line_spines')


def assert_spines_are_the_oracles(strips, imgs, results, what, **kw):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import SpineStrips, result_lines, spine_strips_host
    want = spine_strips_host(imgs, [result_lines(r) for r in results], **kw)
    assert isinstance(strips, SpineStrips) and strips.height == want.height and len(strips.buckets) == len(want.buckets), what
    for name in ('image', 'status', 'squeezed', 'widths', 'bucket', 'index', 'rows', 'knots'):
        assert same(getattr(strips, name), getattr(want, name)), (what, name)
    for a, b in zip(strips.buckets, want.buckets):
        assert a.is_cuda and same(a.cpu().numpy(), b), what
    first = 0
    for k, r in enumerate(results):
        L = len(r.line_chars)
        assert L == len(r.line_polygons) == len(r.line_spines), (what, k)
        assert r.line_strip_ids.dtype == np.int32 and r.line_strip_ids.tolist() == list(range(first, first + L)), (what, k)
        assert (strips.image[first:first + L] == k).all(), (what, k)
        for l, s in enumerate(r.line_strip_ids.tolist()):
            if want.status[s] == 0:
                assert same(strips.strip(s).cpu().numpy(), np.ascontiguousarray(want.strip(s))), (what, k, l)
                assert same(r.line_spines[l], want.spine(s)) and r.line_spines[l].shape[1:] == (2, 2), (what, k, l)
            else:
                assert r.line_spines[l].shape == (0, 2, 2), (what, k, l)
        first += L
    assert first == len(strips.status), what
    return want


def test_off_is_the_result_without_the_feature_and_on_adds_the_oracles_strips():
    inf, _ = build(torch.float16)
    configure(inf, False)
    imgs = images()
    c = inf.config
    assert c.precise_line_strip_curved is False
    c.precise_char_lines = c.precise_line_strips = True
    base = [inf.infer(img) for img in imgs]          # the config as it comes: the new field never touched
    base_batch = inf.infer_batch(imgs)
    assert sum(len(r.line_polygons) for r in base) > 0
    for r in base + list(base_batch.results):
        assert r.line_spines == []
    kw = dict(height=32, width_max=2048, width_step=64, margin=0.125)
    for kw in (kw, dict(height=12, width_max=40, width_step=8, margin=0.5)):
        c.precise_line_strip_curved = False
        c.precise_line_strip_height, c.precise_line_strip_width_max, c.precise_line_strip_width_step, \
            c.precise_line_strip_margin = kw['height'], kw['width_max'], kw['width_step'], kw['margin']
        off = [inf.infer(img) for img in imgs]
        off_batch = inf.infer_batch(imgs)
        if kw['height'] == 32:
            for k in range(len(imgs)):
                assert_same_fields(off[k], base[k], ('off', k))
                assert_same_fields(off_batch.results[k], base_batch.results[k], ('off, batch', k))
            assert same(off_batch.line_strips, base_batch.line_strips)
        c.precise_line_strip_curved = True
        on = [inf.infer(img) for img in imgs]
        on_batch = inf.infer_batch(imgs)
        assert all(r.line_strips is None for r in on_batch.results)
        assert_spines_are_the_oracles(on_batch.line_strips, imgs, on_batch.results, ('infer_batch', kw), **kw)
        for k, (a, b) in enumerate(zip(on, on_batch.results)):
            assert_same_fields(a, off[k], ('on', k), skip=SPINE_FIELDS)
            assert_same_fields(b, off_batch.results[k], ('on, batch', k), skip=SPINE_FIELDS)
            assert same(a.line_strip_ids, off[k].line_strip_ids)
            want = assert_spines_are_the_oracles(a.line_strips, [imgs[k]], [a], ('infer', k, kw), **kw)
            one = inf.infer_batch([imgs[k]])
            assert_results_equal(a, one.results[0], ('a batch of one against infer', k))
            for name in LINE_FIELDS + ('line_strip_ids', 'line_spines'):
                assert same(getattr(a, name), getattr(one.results[0], name)), ('a batch of one against infer', k, name)
            assert same(one.line_strips, a.line_strips), ('a batch of one against infer', k)
            print(f'{kw}, image {k}: {len(want.status)} lines, {int((want.status == 0).sum())} strips, widths '
                  f'{sorted(set(want.widths.tolist()))}, {int(want.squeezed.sum())} squeezed, {len(want.knots)} knots')
    c.precise_line_strip_curved = False
    c.precise_line_strip_height, c.precise_line_strip_width_max, c.precise_line_strip_width_step, c.precise_line_strip_margin = \
        32, 2048, 64, 0.125
    assert_same_fields(inf.infer(imgs[0]), base[0], 'off again')


def test_on_without_line_strips_raises_and_on_follows_the_suppression():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import result_quads
    inf, _ = build(torch.float16)
    configure(inf, False)
    img = images()[0]
    c = inf.config
    c.precise_char_lines = c.precise_line_strip_curved = True
    with pytest.raises(ValueError, match='precise_line_strips'):
        inf.infer(img)
    with pytest.raises(ValueError, match='precise_line_strips'):
        inf.infer_batch([img])
    c.precise_char_lines = False
    with pytest.raises(ValueError):
        inf.infer(img)
    c.precise_char_lines = c.precise_line_strips = True
    c.precise_line_strip_curved = False
    c.precise_char_nms_iou_thr = 0.05
    straight = inf.infer(img)
    c.precise_line_strip_curved = True
    both = inf.infer(img)
    assert len(straight.line_chars) > 0 and len(straight.char_lines) == len(result_quads(straight)[0])
    assert_same_fields(both, straight, 'after the suppression', skip=SPINE_FIELDS)
    assert_spines_are_the_oracles(both.line_strips, [img], [both], 'after the suppression')


def test_a_hand_made_arc_in_a_result():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import (group_results, quad_strips_host, result_quads,
                                                                  spine_strips_for_results, strips_for_results)
    inf, _ = build(torch.float16)
    configure(inf, False)
    centre, R = (20.0, 20.0), 200.0
    imgs = [P.radial_image((256, 256), centre, R), images()[1]]
    base = inf.infer(images()[0])
    sizes = [len(p) for p in base.probs]
    n = sum(sizes)
    assert n >= 45 and sum(k > 0 for k in sizes) >= 2
    # the result keeps its regions; its characters become the quarter circle of tests/test_cpu_spines.py in scrambled order,
    # spread over the regions' lists, and single characters far from it
    arc = P.arc(centre, R)
    order = np.random.default_rng(9).permutation(len(arc))
    spare = np.array([[[240.0 - 3 * k, 2.0], [240.0 - 3 * k, 4.0], [242.0 - 3 * k, 4.0], [242.0 - 3 * k, 2.0]]
                      for k in range(n - len(arc))]).reshape(-1, 4, 2)
    quads = np.concatenate([arc[order], spare])
    cuts = np.cumsum([0] + sizes)
    made = attrs.evolve(base, polygons=[quads[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    empty = attrs.evolve(made, polygons=[q[:0] for q in made.polygons], probs=[p[:0] for p in made.probs],
                         points=[p[:0] for p in made.points])
    grouped = group_results([made, empty])
    assert np.argsort(order).tolist() in [m.tolist() for m in grouped[0].line_chars], 'the arc is one line in reading order'
    assert len(grouped[1].line_polygons) == 0
    out, strips = spine_strips_for_results(grouped, imgs)
    for a, b in zip(out, grouped):
        assert_same_fields(a, b, 'the step changes line_strip_ids and line_spines only', skip=('line_strip_ids', 'line_spines'))
    want = assert_spines_are_the_oracles(strips, imgs, out, 'hand-made arc')
    assert out[0].line_strips is None and out[1].line_strip_ids.shape == (0,) and out[1].line_spines == []
    s = [m.tolist() for m in out[0].line_chars].index(np.argsort(order).tolist())
    assert want.status[s] == 0 and len(out[0].line_spines[s]) == 22 and np.array_equal(result_quads(out[0])[0][out[0].line_chars[s]], arc)
    # the strip is level along the circle, the straight route's strip of the same line is not
    level = lambda strip: int(np.abs(strip[:, :, 0].astype(np.int64) - np.median(strip[:, :, 0], axis=1, keepdims=True)).max())
    assert level(strips.strip(s).cpu().numpy()) <= 2
    _, chord = strips_for_results(grouped, imgs)
    assert level(chord.strip(s).cpu().numpy()) > 2
    assert np.array_equal(chord.strip(s).cpu().numpy(), quad_strips_host(imgs, [r.line_polygons for r in grouped]).strip(s))
    other, small = spine_strips_for_results(grouped, imgs, height=16, width_max=64, width_step=16, margin=0.0)
    assert_spines_are_the_oracles(small, imgs, other, 'other parameters', height=16, width_max=64, width_step=16, margin=0.0)
    assert small.squeezed[s] and tuple(small.buckets[-1].shape)[1:] == (16, 64, 3)
