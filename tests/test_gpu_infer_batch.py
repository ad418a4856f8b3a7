"""``infer_batch`` on the MI355X: for one image it equals ``infer`` field by field, bit for bit; for a batch whose regions
need several shared pages it equals, bit for bit, the composition of the public pieces and the host oracles -
``rough_infer_text_regions_batch``, ``region_crops``, ``stack_regions_pages``, ``resample_pack_multi_host`` +
``pack_region_labels_multi_host``, ``precise_infer_char_polygons_batch``, ``precise_group_char_polygons`` per page,
``remap_polygons`` -, eager and replayed; then the orient flag, the empty list and an image without regions."""
import attrs
import numpy as np
import pytest
import torch

from tests.test_gpu_inferencing import build
from tests.test_gpu_infer_oriented import configure

pytestmark = pytest.mark.gpu


def picture(shape, seed):
    """Seeded noise with drawn bars: text-line-like dark bars on the noise."""
    g = np.random.default_rng(seed)
    img = g.integers(0, 256, tuple(shape) + (3,), dtype=np.uint8)
    for k in range(int(g.integers(2, 5))):
        y, x = int(g.integers(0, shape[0] - 12)), int(g.integers(0, shape[1] // 2))
        img[y:y + int(g.integers(4, 12)), x:x + int(g.integers(shape[1] // 4, shape[1] // 2))] //= 8
    return img


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_regions_equal(a, b, what):
    assert a.resized_shape == b.resized_shape and a.num_regions == b.num_regions, what
    for name in ('boxes', 'areas', 'valid', 'char_height_medians', 'scales', 'resized_shapes', 'keep'):
        assert same(getattr(a, name), getattr(b, name)), (what, name)
    for name in ('labels', 'padded_image'):
        u, v = getattr(a, name), getattr(b, name)
        assert (u is None and v is None) or same(u, v), (what, name)


def assert_results_equal(a, b, what):
    assert a.image_shape == b.image_shape and tuple(a.page_shape) == tuple(b.page_shape), what
    assert_regions_equal(a.regions, b.regions, what)
    for name in ('packed', 'too_large', 'placements', 'placement_regions'):
        assert same(getattr(a, name), getattr(b, name)), (what, name)
    for name in ('page', 'region_labels'):
        u, v = getattr(a, name), getattr(b, name)
        assert (u is None and v is None) or same(u, v), (what, name)
    for name in ('points', 'probs', 'polygons'):
        u, v = getattr(a, name), getattr(b, name)
        assert len(u) == len(v) == len(a.regions.boxes), (what, name)
        for k, (x, y) in enumerate(zip(u, v)):
            assert same(x, y), (what, name, k)


@pytest.mark.parametrize('shape', [(100, 150), (800, 1000)], ids=['100x150', '800x1000'])
def test_a_batch_of_one_equals_infer(shape):
    inf, _ = build(torch.float16)
    configure(inf, False)
    img = np.random.default_rng(5).integers(0, 256, shape + (3,), dtype=np.uint8)
    for k in range(3):  # the first call of a graph signature is eager, the later ones replay
        full = k < 2
        one = inf.infer(img, return_page=full, return_labels=full)
        batch = inf.infer_batch([img], return_pages=full, return_labels=full)
        res = batch.results[0]
        if k == 0:
            chars = sum(len(p) for p in one.points)
            print(f'{shape}: {one.regions.num_regions} regions, {int(one.packed.sum())} packed on a {one.page_shape} page, '
                  f'{chars} characters')
            assert one.packed.sum() >= 2 and chars > 0 and one.page_shape[0] <= inf.config.precise_page_height_max
        assert len(batch.results) == 1 and batch.page_shapes == [one.page_shape]
        assert_results_equal(res, one, (shape, k))
        assert one.placement_pages.shape == (0,) and one.placement_pages.dtype == np.int32
        assert res.placement_pages.dtype == np.int32 and res.placement_pages.tolist() == [0] * len(one.placements)
        assert batch.rows.dtype == np.int32 and np.array_equal(batch.rows[:, 2:10], one.placements)
        assert np.array_equal(batch.rows[:, 10], one.placement_regions) and np.array_equal(batch.rows[:, 11], one.placement_regions)
        if full:
            assert len(batch.pages) == len(batch.region_labels) == 1
            assert same(batch.pages[0], one.page) and same(batch.region_labels[0], one.region_labels)
        else:
            assert batch.pages is None and batch.region_labels is None and res.page is None and res.regions.labels is None
    # the batch ran the graphs of infer: no key of its own, no further shape
    c = inf.config
    thr, hmin, cap = float(c.rough_char_mask_positive_thr), float(c.rough_valid_char_height_min), int(c.rough_text_regions_max)
    peak, size = float(c.precise_build_polygons_positive_char_prob_thr), c.precise_build_polygons_maximum_filter_size
    assert sorted(str(k[0]) for k in inf.graphs.entries) == sorted(
        str(k) for k in (('rough_text_regions', thr, hmin, cap), ('precise_char_polygons', peak, size)))
    # and the rough half alone equals rough_infer_text_regions
    assert_regions_equal(inf.rough_infer_text_regions_batch([img])[0], inf.rough_infer_text_regions(img, resize_fn='device'), shape)


def compose(inf, imgs):
    """infer_batch() restated with the public pieces and the host oracles."""
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import (
        pack_region_labels_multi_host, precise_group_char_polygons, region_crops, remap_polygons, resample_pack_multi_host,
        stack_regions_pages)
    c = inf.config
    rough = inf.rough_infer_text_regions_batch(imgs)
    shapes = [img.shape[:2] for img in imgs]
    crops = np.concatenate([region_crops(r.boxes, shape, r.resized_shape) for r, shape in zip(rough, shapes)])
    image_of = np.concatenate([np.full(len(r.boxes), i) for i, r in enumerate(rough)])
    local = np.concatenate([np.arange(1, len(r.boxes) + 1) for r in rough])
    page_shapes, boxes, page_of, packed, too_large = stack_regions_pages(
        np.concatenate([r.resized_shapes for r in rough]), c.precise_stack_flattened_text_regions_page_pad,
        c.precise_stack_flattened_text_regions_pad, c.precise_page_width_max, c.precise_page_height_step,
        c.precise_page_height_max, keep=np.concatenate([r.keep for r in rough]))
    rows = []
    for g in np.flatnonzero(packed).tolist():
        rows.append([image_of[g], page_of[g], *crops[g], *boxes[g], local[g], g + 1])
    rows = np.array(rows, np.int32).reshape(-1, 12)
    rows = rows[np.argsort(rows[:, 1], kind='stable')]
    pages, labels = [], []
    for q, shape in enumerate(page_shapes):  # a page at a time: the definition does not care about batches
        mine = rows[rows[:, 1] == q].copy()
        mine[:, 1] = 0
        pages.append(resample_pack_multi_host(imgs, mine, shape, 1)[0])
        labels.append(pack_region_labels_multi_host([r.labels for r in rough], [r.resized_shape for r in rough], shapes, mine,
                                                    (shape[0] // 2, shape[1] // 2), 2, 1)[0])
    chars = inf.precise_infer_char_polygons_batch(pages)
    results = []
    for i, r in enumerate(rough):
        n = len(r.boxes)
        results.append(dict(points=[np.zeros((0, 2), np.int32)] * n, probs=[np.zeros((0,), np.float32)] * n,
                            polygons=[np.zeros((0, 4, 2), np.float64)] * n))
    for q in range(len(page_shapes)):
        groups = precise_group_char_polygons(chars[q], labels[q])
        for row in rows[rows[:, 1] == q]:
            gid, out, k = int(row[11]), results[int(row[0])], int(row[10]) - 1
            if gid <= len(groups):
                out['points'][k], out['probs'][k] = groups[gid - 1].points, groups[gid - 1].probs
                out['polygons'][k] = remap_polygons(groups[gid - 1].polygons, row[2:10])
    return rough, page_shapes, rows, packed, too_large, pages, labels, results


@pytest.mark.parametrize('step', [256, 64], ids=['pages-of-one-height', 'shorter-last-page'])
def test_a_batch_equals_the_composition_of_public_pieces(step):
    inf, _ = build(torch.float16)
    configure(inf, False)
    # low enough that the regions of four small images need several pages (this model's regions come out up to 560 rows
    # high: the one above 492 is reported too large); in steps of 64 the last page is shorter: a batch of its own
    inf.config.precise_page_height_max, inf.config.precise_page_height_step = 512, step
    # two padded rough shapes, 128 x 160 three times (one chunk of three) and 96 x 224 (a chunk of one)
    imgs = [picture(shape, 40 + k) for k, shape in enumerate([(100, 150), (120, 155), (96, 200), (128, 160)])]
    first = inf.infer_batch(imgs, return_pages=True, return_labels=True)  # every graph signature's first call: eager
    replays = inf.graphs.replays
    rough, page_shapes, rows, packed, too_large, pages, labels, want = compose(inf, imgs)
    chars = sum(len(p) for w in want for p in w['points'])
    print(f'{[r.num_regions for r in rough]} regions, {int(packed.sum())} packed, {int(too_large.sum())} too large, pages '
          f'{page_shapes}, {chars} characters in {sum(len(p) > 0 for w in want for p in w["points"])} regions; rows per page '
          f'{np.bincount(rows[:, 1]).tolist()}, per image {np.bincount(rows[:, 0], minlength=4).tolist()}')
    assert len(page_shapes) >= 2 and chars >= 1, 'the batch must need at least two pages and hold a character'
    assert (page_shapes[-1] == page_shapes[0]) == (step == 256), 'one precise batch, or the full pages and the last page'
    assert len(set(rows[:, 0].tolist())) >= 2 and len(set(rows[rows[:, 1] == 0][:, 0].tolist())) >= 2, 'images share a page'
    later = [inf.infer_batch(imgs, return_pages=True, return_labels=True), inf.infer_batch(imgs)]
    assert inf.graphs.replays > replays, 'the later calls replay'
    first_of = np.concatenate([[0], np.cumsum([len(r.boxes) for r in rough])])
    for k, batch in enumerate([first] + later):
        assert batch.page_shapes == page_shapes and same(batch.rows, rows), k
        if k < 2:
            assert len(batch.pages) == len(batch.region_labels) == len(pages)
            assert all(same(a, b) for a, b in zip(batch.pages, pages)) and all(same(a, b) for a, b in zip(batch.region_labels, labels))
        else:
            assert batch.pages is None and batch.region_labels is None
        assert len(batch.results) == len(imgs)
        for i, (res, r, w) in enumerate(zip(batch.results, rough, want)):
            mine = rows[rows[:, 0] == i]
            mine = mine[np.argsort(mine[:, 10], kind='stable')]  # per image in region order
            assert res.image_shape == imgs[i].shape[:2]
            if k < 2:
                assert_regions_equal(res.regions, r, (k, i))
            else:
                assert res.regions.labels is None and res.regions.padded_image is None and same(res.regions.boxes, r.boxes)
            assert same(res.packed, packed[first_of[i]:first_of[i + 1]]) and same(res.too_large, too_large[first_of[i]:first_of[i + 1]])
            assert same(res.placements, np.ascontiguousarray(mine[:, 2:10])) and same(res.placement_regions, np.ascontiguousarray(mine[:, 10]))
            assert same(res.placement_pages, np.ascontiguousarray(mine[:, 1]))
            if len(mine):
                assert res.page_shape == page_shapes[mine[0, 1]]
                if k < 2:
                    assert same(res.page, pages[mine[0, 1]]) and same(res.region_labels, labels[mine[0, 1]])
            for name in ('points', 'probs', 'polygons'):
                got = getattr(res, name)
                assert len(got) == len(r.boxes)
                for region, (u, v) in enumerate(zip(got, w[name])):
                    assert same(u, v), (k, i, name, region)


def test_orient_flag_empty_list_and_an_image_without_regions():
    inf, _ = build(torch.float16)
    configure(inf, True)
    with pytest.raises(ValueError, match='orient'):
        inf.infer_batch([picture((100, 150), 1)])
    configure(inf, False)
    empty = inf.infer_batch([])
    assert empty.results == [] and empty.page_shapes == [] and empty.rows.shape == (0, 12) and empty.rows.dtype == np.int32
    assert empty.pages is None and empty.region_labels is None and inf.rough_infer_text_regions_batch([]) == []
    with pytest.raises(ValueError, match='uint8'):
        inf.infer_batch([np.zeros((64, 64, 3), np.float32)])
    # An all-black image between two images that share a padded rough shape of their own, so the neighbours' rough chunk is
    # the same with and without it.  This untrained model finds regions in a black image too (its biases alone: 6 regions
    # at 96 x 200, heights up to 1.284), so the height floor is set just above the largest height it predicts anywhere in
    # the black image: then none of the black image's regions has a valid height and none is kept, by construction, while
    # the neighbours keep the few regions that reach higher
    a, b, black = picture((200, 250), 1), picture((200, 250), 3), np.zeros((96, 200, 3), np.uint8)
    inf.config.rough_valid_char_height_min = 0.0
    top = np.float32(inf.rough_infer(black).rough_char_height_score_map.max())
    inf.config.rough_valid_char_height_min = float(np.nextafter(top, np.float32(2)))
    alone = inf.infer_batch([black])
    res = alone.results[0]
    print(f'black: largest height {top}, {res.regions.num_regions} regions, {int(res.regions.keep.sum())} kept')
    assert res.regions.num_regions > 0 and not res.regions.keep.any() and not res.packed.any() and not res.too_large.any()
    assert alone.rows.shape == (0, 12) and len(alone.page_shapes) == 1
    assert res.placements.shape == (0, 8) and res.placement_pages.shape == (0,) and res.page is None
    assert all(len(p) == 0 for p in res.points) and len(res.points) == len(res.polygons) == len(res.regions.boxes)
    assert_results_equal(res, inf.infer(black), 'black')
    pair = inf.infer_batch([a, b], return_pages=True, return_labels=True)
    trio = inf.infer_batch([a, black, b], return_pages=True, return_labels=True)
    assert all(sum(len(p) for p in r.points) > 0 for r in pair.results), 'both neighbours hold characters'
    # a global id is 1 + the region's position among ALL regions of the batch, kept or not: the black image's regions, none
    # of them kept, shift the ids of the image behind it, and nothing else
    n_a, n_black = len(pair.results[0].regions.boxes), len(trio.results[1].regions.boxes)
    shifted = lambda ids: np.where(ids > n_a, ids + n_black, ids).astype(ids.dtype)
    assert n_black > 0 and (pair.rows[:, 11] > n_a).any() and (pair.rows[:, 11] <= n_a).any()
    assert trio.page_shapes == pair.page_shapes and np.array_equal(trio.rows[:, 1:11], pair.rows[:, 1:11])
    assert np.array_equal(trio.rows[:, 11], shifted(pair.rows[:, 11]))
    assert trio.rows[:, 0].tolist() == [2 * s for s in pair.rows[:, 0].tolist()]
    assert all(same(u, v) for u, v in zip(trio.pages, pair.pages))
    assert all(same(u, shifted(v)) for u, v in zip(trio.region_labels, pair.region_labels))
    for got, want, what in ((trio.results[0], pair.results[0], 'first'), (trio.results[2], pair.results[1], 'last')):
        assert same(got.region_labels, shifted(want.region_labels)), what
        assert_results_equal(attrs.evolve(got, region_labels=None), attrs.evolve(want, region_labels=None), what)
    assert not trio.results[1].packed.any() and all(len(p) == 0 for p in trio.results[1].points)
