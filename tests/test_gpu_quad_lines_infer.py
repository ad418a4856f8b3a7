"""The text lines inside ``infer`` / ``infer_batch`` on the MI355X, on the small untrained model and the images of
tests/test_gpu_infer_batch.py.

Off (the default), the results equal those of a config that never heard of the feature, field for field, with the new
fields at their defaults.  On, ``char_lines``, ``line_chars`` and ``line_polygons`` equal the host oracle
(``quad_lines_lists_host``) on the result's own quads, every other field is what it is with the switch off, and
``infer_batch`` of one image equals ``infer`` of it.  The untrained model's characters are small and apart from one another, so
what the oracle groups on its output is printed, not asserted; lines of several characters are covered HERE BY THE SECOND
ROUTE: the step of ``infer`` on a result whose polygons are a hand-made layout spread over its regions
(``test_a_hand_made_layout_in_a_result``), where the layout's truth is asserted."""
import attrs
import numpy as np
import pytest
import torch

from tests import quad_line_cases as Q
from tests.test_gpu_infer_batch import assert_results_equal, picture
from tests.test_gpu_inferencing import build
from tests.test_gpu_infer_oriented import configure

pytestmark = pytest.mark.gpu

LINE_FIELDS = ('char_lines', 'line_chars', 'line_polygons', 'lines_status')


def same(u, v):
    if isinstance(u, np.ndarray) or isinstance(v, np.ndarray):
        return isinstance(u, np.ndarray) and isinstance(v, np.ndarray) and u.dtype == v.dtype and u.shape == v.shape and \
            u.tobytes() == v.tobytes()
    if isinstance(u, torch.Tensor):
        return isinstance(v, torch.Tensor) and same(u.cpu().numpy(), v.cpu().numpy())
    if isinstance(u, (list, tuple)):
        return type(u) is type(v) and len(u) == len(v) and all(same(x, y) for x, y in zip(u, v))
    if attrs.has(type(u)):
        return type(u) is type(v) and all(same(getattr(u, f.name), getattr(v, f.name)) for f in attrs.fields(type(u)))
    return type(u) is type(v) and u == v


def assert_same_fields(a, b, what, skip=()):
    for f in attrs.fields(type(a)):
        if f.name not in skip:
            assert same(getattr(a, f.name), getattr(b, f.name)), (what, f.name)


def assert_lines_are_the_oracles(result, what, **kw):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import quad_lines_lists_host, result_quads
    quads, _ = result_quads(result)
    ref, stats = quad_lines_lists_host([quads], **kw)
    ref = ref[0]
    assert result.lines_status == 0 and same(result.char_lines, ref.line) and result.char_lines.shape == (len(quads),), what
    assert same(list(result.line_chars), list(ref.lines)) and same(result.line_polygons, ref.polygons), what
    return stats


def images():
    return [np.random.default_rng(5).integers(0, 256, (100, 150, 3), dtype=np.uint8), picture((120, 90), 3), picture((64, 200), 4)]


def test_off_is_the_result_without_the_feature_and_on_adds_the_oracles_lines():
    inf, _ = build(torch.float16)
    configure(inf, False)
    imgs = images()
    c = inf.config
    assert (c.precise_char_lines, c.precise_char_line_gap, c.precise_char_line_cross, c.precise_char_line_height_ratio) == \
        (False, 1.5, 0.5, 2.0)
    base = [inf.infer(img) for img in imgs]          # the config as it comes: the new fields never touched
    base_batch = inf.infer_batch(imgs).results
    assert sum(len(p) for p in base[0].probs) > 0
    for r in base + list(base_batch):
        assert r.char_lines.shape == (0,) and r.char_lines.dtype == np.int32 and r.line_chars == [] and r.lines_status == 0
        assert r.line_polygons.shape == (0, 4, 2) and r.line_polygons.dtype == np.float64
    c.precise_char_line_gap, c.precise_char_line_cross, c.precise_char_line_height_ratio = 3.0, 1.0, 4.0  # off: not read
    for k, img in enumerate(imgs):
        assert_same_fields(inf.infer(img), base[k], ('off', k))
    for k, r in enumerate(inf.infer_batch(imgs).results):
        assert_same_fields(r, base_batch[k], ('off, batch', k))
    for kw in (dict(gap=1.5, cross=0.5, height_ratio=2.0), dict(gap=3.0, cross=1.0, height_ratio=4.0)):
        c.precise_char_lines = True
        c.precise_char_line_gap, c.precise_char_line_cross, c.precise_char_line_height_ratio = kw['gap'], kw['cross'], kw['height_ratio']
        on = [inf.infer(img) for img in imgs]
        on_batch = inf.infer_batch(imgs).results
        for k, (a, b) in enumerate(zip(on, on_batch)):
            assert_same_fields(a, base[k], ('on', k), skip=LINE_FIELDS)
            assert_same_fields(b, base_batch[k], ('on, batch', k), skip=LINE_FIELDS)
            stats = assert_lines_are_the_oracles(a, ('infer', k), **kw)
            assert_lines_are_the_oracles(b, ('infer_batch', k), **kw)
            # a batch shares its pages among the images, so its characters are not those of infer; a batch of one is infer
            one = inf.infer_batch([imgs[k]]).results[0]
            assert_results_equal(a, one, ('a batch of one against infer', k))
            for name in LINE_FIELDS:
                assert same(getattr(a, name), getattr(one, name)), ('a batch of one against infer', k, name)
            print(f'{kw}, image {k}: {stats[0]} characters, {stats[1]} take part, {stats[2]} links, {stats[3]} lines')
    c.precise_char_lines = False
    assert_same_fields(inf.infer(imgs[0]), base[0], 'off again')


def test_lines_follow_the_suppression():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import result_quads
    inf, _ = build(torch.float16)
    configure(inf, False)
    img = images()[0]
    inf.config.precise_char_nms_iou_thr = 0.05
    suppressed = inf.infer(img)
    inf.config.precise_char_lines = True
    both = inf.infer(img)
    assert_same_fields(both, suppressed, 'after the suppression', skip=LINE_FIELDS)
    assert_lines_are_the_oracles(both, 'after the suppression')
    assert len(both.char_lines) == len(result_quads(suppressed)[0])


def test_a_hand_made_layout_in_a_result():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import group_results, result_quads
    inf, _ = build(torch.float16)
    configure(inf, False)
    base = inf.infer(images()[0])
    sizes = [len(p) for p in base.probs]
    n = sum(sizes)
    assert n >= 45 and sum(k > 0 for k in sizes) >= 2
    # the result keeps its regions, points and probs; its characters become three lines of n // 3 in scrambled order, so
    # every line runs through several regions' lists
    quads, truth = Q.layout(3, n // 3, **Q.LATIN, word_space=10.0, angle=0.35, seed=9)
    quads = quads + 400.0
    spare = np.array([Q.SQ(900 + 60 * k, 900, 30, 16) for k in range(n - len(quads))], np.float64).reshape(-1, 4, 2)
    quads = np.concatenate([quads, spare])
    cuts = np.cumsum([0] + sizes)
    made = attrs.evolve(base, polygons=[quads[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    assert np.array_equal(result_quads(made)[0], quads)
    out = group_results([made, attrs.evolve(made, polygons=[q[:0] for q in made.polygons], probs=[p[:0] for p in made.probs],
                                            points=[p[:0] for p in made.points])])
    assert_same_fields(out[0], made, 'the step changes the line fields only', skip=LINE_FIELDS)
    assert_lines_are_the_oracles(out[0], 'hand-made layout')
    want = truth + [[len(quads) - len(spare) + k] for k in range(len(spare))]
    assert [m.tolist() for m in out[0].line_chars] == want and out[0].line_polygons.shape == (len(want), 4, 2)
    assert out[1].lines_status == 0 and out[1].line_chars == [] and out[1].char_lines.shape == (0,)
    made_other = group_results([made], gap=1.0)[0]
    assert_lines_are_the_oracles(made_other, 'gap 1.0', gap=1.0)
    assert len(made_other.line_chars) > len(want)


def test_an_image_with_too_many_characters_gets_no_lines():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import AdaptiveScalingInferencingResult, group_results
    n = 8193
    sq = np.array([[0, 0], [0, 4], [4, 4], [4, 0]], np.float64)
    big = AdaptiveScalingInferencingResult(
        image_shape=(10, 10), regions=None, packed=np.ones((1,), bool), too_large=np.zeros((1,), bool),
        placements=np.zeros((1, 8), np.int32), placement_regions=np.ones((1,), np.int32), page_shape=(256, 256), page=None,
        region_labels=None, points=[np.zeros((n, 2), np.int32)], probs=[np.full((n,), 0.9, np.float32)],
        polygons=[np.broadcast_to(sq, (n, 4, 2)).copy()])
    small = attrs.evolve(big, points=[big.points[0][:3]], probs=[big.probs[0][:3]], polygons=[big.polygons[0][:3]])
    out = group_results([big, small])
    assert out[0].lines_status == 2 and out[0].line_chars == [] and out[0].char_lines.shape == (0,)
    assert out[0].line_polygons.shape == (0, 4, 2) and len(out[0].probs[0]) == n
    assert out[1].lines_status == 0 and out[1].char_lines.tolist() == [0, 0, 0] and [m.tolist() for m in out[1].line_chars] == [[0, 1, 2]]
