"""``infer`` with oriented text regions (config.precise_text_region_orient) on the MI355X: equal, bit for bit, to the
composition of the public pieces and the host oracles - ``rough_infer_text_regions``, the moment and extent oracles, the
rule of inferencing/orient.py, ``stack_regions``, ``resample_host`` + ``warp_host``, both label oracles,
``precise_infer_char_polygons``, grouping and both remaps -, eager and replayed; and with the flag off, what it was before
the flag existed (tests/test_gpu_region_packing.py states that path), with the same graph keys."""
import numpy as np
import pytest
import torch

from tests.test_gpu_inferencing import build
from tests.test_gpu_region_packing import compose as compose_straight

pytestmark = pytest.mark.gpu


def configure(inf, orient):
    # as tests/test_gpu_region_packing.py: the untrained model predicts heights near 0.9 and probabilities near 0.5
    c = inf.config
    c.rough_valid_char_height_min = 0.85
    c.precise_flattened_text_region_resized_char_height_median = 4
    c.precise_build_polygons_positive_char_prob_thr = 0.5
    c.precise_text_region_orient = orient
    # the untrained model's regions are blobs, not lines: any blob that is slanted and packs smaller than its box qualifies
    c.precise_text_region_flattener_typical_long_side_ratio_min = 1.0


def compose(inf, img, resize_fn):
    """infer() with oriented regions restated with the public pieces and the host oracles."""
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import (
        check_warps, orient_regions, pack_region_labels_host, precise_group_char_polygons, region_crops, region_directions,
        region_extents_host, region_moments_host, remap_polygons, remap_polygons_affine, resample_host, stack_regions,
        warp_host, warp_region_labels_host, warp_row)
    c = inf.config
    r = inf.rough_infer_text_regions(img, resize_fn=resize_fn)
    n = len(r.boxes)
    shape = img.shape[:2]
    _, dirs = region_directions(region_moments_host(r.labels, n)[0])
    extents = region_extents_host(r.labels, dirs[None])[0]
    oriented, rects, shapes, keep = orient_regions(
        dirs, extents, r.scales, r.resized_shapes, r.keep, shape, r.resized_shape,
        c.precise_text_region_flattener_typical_long_side_ratio_min, c.precise_flattened_text_region_resized_char_height_median,
        c.precise_flattened_text_region_resized_ratio_min)
    crops = region_crops(r.boxes, shape, r.resized_shape)
    page_shape, boxes, packed, too_large = stack_regions(
        shapes, c.precise_stack_flattened_text_regions_page_pad, c.precise_stack_flattened_text_regions_pad,
        c.precise_page_width_max, c.precise_page_height_step, keep=keep)
    straight = packed & ~oriented
    placements = np.concatenate([crops[straight], boxes[straight]], axis=1).astype(np.int32)
    ids = (np.flatnonzero(straight) + 1).astype(np.int32)
    warp_ids = (np.flatnonzero(packed & oriented) + 1).astype(np.int32)
    warps = np.array([warp_row(dirs[k - 1], rects[k - 1], shape, r.resized_shape, boxes[k - 1], r.scales[k - 1])
                      for k in warp_ids.tolist()], np.int64).reshape(-1, 12)
    check_warps(warps, page_shape, placements)
    page = warp_host(img, warps, resample_host(img, placements, page_shape))
    chars = inf.precise_infer_char_polygons(page)
    labels = pack_region_labels_host(r.labels, r.resized_shape, shape, placements, ids,
                                     (page_shape[0] // 2, page_shape[1] // 2), 2)
    labels = warp_region_labels_host(r.labels, r.resized_shape, shape, warps, warp_ids, labels, 2)
    groups = precise_group_char_polygons(chars, labels)
    points = [np.zeros((0, 2), np.int32)] * n
    probs = [np.zeros((0,), np.float32)] * n
    polygons = [np.zeros((0, 4, 2), np.float64)] * n
    for table, table_ids, remap in ((placements, ids, remap_polygons), (warps, warp_ids, remap_polygons_affine)):
        for k, rid in enumerate(table_ids.tolist()):
            if rid <= len(groups):
                points[rid - 1], probs[rid - 1] = groups[rid - 1].points, groups[rid - 1].probs
                polygons[rid - 1] = remap(groups[rid - 1].polygons, table[k])
    return dict(r=r, oriented=oriented, shapes=shapes, keep=keep, packed=packed, too_large=too_large, placements=placements,
                ids=ids, warps=warps, warp_ids=warp_ids, page=page, labels=labels, points=points, probs=probs,
                polygons=polygons)


def test_oriented_infer_equals_the_composition_of_public_pieces():
    inf, _ = build(torch.float16)
    configure(inf, True)
    shape = (100, 150)
    # blobs rarely pack smaller along their axis than by their box: this page has two that do (the conditions below)
    img = np.random.default_rng(7).integers(0, 256, shape + (3,), dtype=np.uint8)
    first = inf.infer(img, return_page=True, return_labels=True)  # every graph signature's first call: eager
    replays = inf.graphs.replays
    w = compose(inf, img, None)
    r, points = w['r'], w['points']
    with_chars = np.array([len(p) > 0 for p in points])
    turned, straight = w['packed'] & w['oriented'], w['packed'] & ~w['oriented']
    print(f'{r.num_regions} regions, {int(w["keep"].sum())} kept, {int(turned.sum())} oriented and {int(straight.sum())} '
          f'axis-aligned on a {w["page"].shape} page, characters in {int((with_chars & turned).sum())} and '
          f'{int((with_chars & straight).sum())} of them; the box path packs {int(r.resized_shapes[w["packed"]].prod(axis=1).sum())} px2, '
          f'this one {int(w["shapes"][w["packed"]].prod(axis=1).sum())} px2')
    assert turned.sum() >= 2 and straight.sum() >= 1, 'the page must hold oriented and axis-aligned regions'
    assert (with_chars & turned).any() and (with_chars & straight).any(), 'characters in at least one region of each kind'
    assert w['shapes'][w['packed']].prod(axis=1).sum() < r.resized_shapes[w['packed']].prod(axis=1).sum()
    after_compose = inf.graphs.replays
    later = [inf.infer(img, return_page=True, return_labels=True)]
    before_last = inf.graphs.replays
    later.append(inf.infer(img))
    print(f'replays: {replays} after the first call, {after_compose} after compose, {before_last} after the second call, '
          f'{inf.graphs.replays} after the third; {inf.graphs.captures} captures; keys {[k[0] for k in inf.graphs.entries]}; pages '
          f'{[res.page_shape for res in [first] + later]}, oriented {[int(res.oriented.sum()) for res in [first] + later]}')
    for k, res in enumerate([first] + later):
        assert res.image_shape == shape and res.page_shape == w['page'].shape[:2] and res.regions.num_regions == r.num_regions
        assert np.array_equal(res.regions.boxes, r.boxes) and np.array_equal(res.regions.scales, r.scales)
        assert res.regions.char_height_medians.tobytes() == r.char_height_medians.tobytes()
        assert np.array_equal(res.regions.keep, w['keep']) and np.array_equal(res.regions.resized_shapes, w['shapes'])
        assert res.oriented.dtype == bool and np.array_equal(res.oriented, w['oriented'])
        assert np.array_equal(res.packed, w['packed']) and np.array_equal(res.too_large, w['too_large'])
        assert res.placements.dtype == np.int32 and np.array_equal(res.placements, w['placements'])
        assert np.array_equal(res.placement_regions, w['ids'])
        assert res.warps.dtype == np.int64 and np.array_equal(res.warps, w['warps'])
        assert res.warp_regions.dtype == np.int32 and np.array_equal(res.warp_regions, w['warp_ids'])
        if k < 2:
            assert np.array_equal(res.page, w['page']) and np.array_equal(res.region_labels, w['labels'])
            assert np.array_equal(res.regions.labels, r.labels)
        else:
            assert res.page is None and res.region_labels is None and res.regions.labels is None
        assert len(res.points) == len(res.probs) == len(res.polygons) == len(r.boxes)
        for a, b, name in ((res.points, points, 'points'), (res.probs, w['probs'], 'probs'), (res.polygons, w['polygons'], 'polygons')):
            for u, v in zip(a, b):
                assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (k, name)
    # by its third call each of the two graphs of infer is captured (the first call of a signature runs eagerly)
    assert inf.graphs.replays >= before_last + 2, 'the third call replays both graphs'
    captured = [k[0][0] for k, e in inf.graphs.entries.items() if e.graph is not None]
    assert 'rough_text_regions_moments' in captured and 'precise_char_polygons' in captured, captured
    # the way back is the way in: the label cell under a character of an oriented region, taken through
    # remap_polygons_affine, lies in the image on a rough-map pixel that is the region's own or background
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import remap_polygons_affine
    vh, vw = r.resized_shape
    for k, rid in enumerate(w['warp_ids'].tolist()):
        if len(points[rid - 1]):
            at = np.floor(remap_polygons_affine(points[rid - 1] * 2.0 + 1.0, w['warps'][k])).astype(np.int64)
            assert (at >= 0).all() and (at[:, 0] < shape[0]).all() and (at[:, 1] < shape[1]).all()
            my = np.minimum(vh - 1, ((2 * at[:, 0] + 1) * vh) // (2 * shape[0]))
            mx = np.minimum(vw - 1, ((2 * at[:, 1] + 1) * vw) // (2 * shape[1]))
            assert np.isin(r.labels[my, mx], (0, rid)).all()


def test_flag_off_is_the_path_without_the_feature():
    inf, _ = build(torch.float16)
    configure(inf, False)
    img = np.random.default_rng(5).integers(0, 256, (100, 150, 3), dtype=np.uint8)
    results = [inf.infer(img, return_page=True, return_labels=True) for _ in range(2)]
    keys = sorted(str(k[0]) for k in inf.graphs.entries)
    r, packed, too_large, placements, ids, page, labels, points, probs, polygons = compose_straight(inf, img, None)
    for res in results:
        assert res.oriented.shape == (0,) and res.oriented.dtype == bool
        assert res.warps.shape == (0, 12) and res.warps.dtype == np.int64
        assert res.warp_regions.shape == (0,) and res.warp_regions.dtype == np.int32
        assert np.array_equal(res.regions.keep, r.keep) and np.array_equal(res.regions.resized_shapes, r.resized_shapes)
        assert np.array_equal(res.packed, packed) and np.array_equal(res.too_large, too_large)
        assert np.array_equal(res.placements, placements) and np.array_equal(res.placement_regions, ids)
        assert np.array_equal(res.page, page) and np.array_equal(res.region_labels, labels)
        for a, b in ((res.points, points), (res.probs, probs), (res.polygons, polygons)):
            for u, v in zip(a, b):
                assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()
    c = inf.config
    thr, hmin, cap = float(c.rough_char_mask_positive_thr), float(c.rough_valid_char_height_min), int(c.rough_text_regions_max)
    peak, size = float(c.precise_build_polygons_positive_char_prob_thr), c.precise_build_polygons_maximum_filter_size
    assert keys == sorted(str(k) for k in (('rough_text_regions', thr, hmin, cap), ('precise_char_polygons', peak, size)))
