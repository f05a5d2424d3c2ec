"""Train-time augmentation, host side (no GPU): the numpy restatement of Pillow's boxed bicubic resize / flip / paste is pinned against live PIL and
against tests/golden/f12_augment.npz; `owl_bicubic_coeffs_box` (the tap tables the device kernels consume) equals the restatement's tables; the box
transform's closed forms; the sampler's determinism and invariants; the host check that a tile list covers its canvases."""
import os

import numpy as np
import pytest

from tests import augment_reference as R
from owl_vit_object_detection_amd import _lib
from owl_vit_object_detection_amd import preprocess as P


def _f12(golden_dir):
    return np.load(os.path.join(golden_dir, "f12_augment.npz"))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_matches_the_pillow_fixture(golden_dir):
    z = _f12(golden_dir)
    src = R.sources()
    for k, im in enumerate(src):
        assert np.array_equal(im, z[f"src_{k}"])
    assert int(z["size"]) == R.SIZE
    for name, (tiles, n_out) in R.cases().items():
        ta = z[f"tiles_{name}"]
        assert ta.shape[0] == len(tiles)
        for row, t in zip(ta, tiles):                         # the fixture was written for these very tiles
            assert tuple(row[:11]) == (t.src, *t.box, float(t.flip), t.b, t.x0, t.y0, t.cw, t.ch)
        assert np.array_equal(R.render(src, tiles, n_out, R.SIZE), z[f"canvas_{name}"]), name


def test_restatement_matches_live_pillow():
    pytest.importorskip("PIL")
    src = R.sources()
    for name, (tiles, n_out) in R.cases().items():
        assert np.array_equal(R.render(src, tiles, n_out, R.SIZE), R.render_pil(src, tiles, n_out, R.SIZE)), name
    # more boxes than the fixture holds: random float32 edges, down- and up-scales
    rng = np.random.default_rng(3)
    for _ in range(12):
        s = int(rng.integers(3))
        H, W = R.SHAPES[s]
        l, u = float(np.float32(rng.uniform(0, W - 4))), float(np.float32(rng.uniform(0, H - 4)))
        r, lo = float(np.float32(rng.uniform(l + 2, W))), float(np.float32(rng.uniform(u + 2, H)))
        cw, ch = int(rng.integers(3, 40)), int(rng.integers(3, 40))
        t = [R.Tile(s, (l, u, min(r, W), min(lo, H)), bool(rng.integers(2)), 0, 0, 0, cw, ch)]
        S = max(cw, ch)
        assert np.array_equal(R.render(src, t, 1, S), R.render_pil(src, t, 1, S)), t


def test_cases_reach_the_branches_they_claim():
    tiles, _ = R.cases()["single"]
    H = R.SHAPES[1][0]
    by, _, ks = R.coeffs_box(H, tiles[5].box[1], tiles[5].box[3], R.SIZE)
    assert by[0, 0] > 0 and by[-1, 0] + by[-1, 1] < H               # the row range excludes the first and the last source row
    assert R.coeffs_box(H, 0.0, float(H), R.SIZE)[2] == 13            # down-scale: ksize > 5
    bx, _, _ = R.coeffs_box(R.SHAPES[1][1], tiles[3].box[0], tiles[3].box[2], R.SIZE)
    assert bx[0, 1] < bx[R.SIZE // 2, 1]                              # taps clipped at the left border
    bx, _, _ = R.coeffs_box(R.SHAPES[1][1], tiles[4].box[0], tiles[4].box[2], R.SIZE)
    assert bx[-1, 0] + bx[-1, 1] == R.SHAPES[1][1] and bx[-1, 1] < bx[R.SIZE // 2, 1]    # ... and at the right one
    assert {t.cw for t in R.cases()["mixed"][0]} == {24, 12, 8}


# ---- owl_bicubic_coeffs_box ----------------------------------------------------------------------------------------------------------------------
def _lib_coeffs_box(in_size, in0, in1, out_size):
    ksize = P._ksize(in1 - in0, out_size)
    bounds = np.zeros(2 * out_size, dtype=np.int32)
    kk = np.full(out_size * ksize, -7, dtype=np.int32)
    ks = np.zeros(1, dtype=np.int32)
    _lib.call("owl_bicubic_coeffs_box", in_size, float(in0), float(in1), out_size, bounds.ctypes.data, kk.ctypes.data, kk.size, ks.ctypes.data)
    return bounds.reshape(out_size, 2), kk.reshape(out_size, int(ks[0])), int(ks[0])


@pytest.mark.parametrize("in_size,in0,in1,out_size", [
    (53, 0.0, 53.0, 24),            # the whole axis
    (53, 4.0, 40.0, 24),            # integer box
    (53, 3.25, 47.75, 24),          # fractional edges
    (64, 0.0, 20.5, 24),            # touching the left / top border, up-scale
    (64, 21.75, 64.0, 24),          # touching the right / bottom border
    (64, 0.0, 64.0, 24),            # down-scale, ksize 13
    (640, 17.3, 633.9, 96),         # down-scale, ksize 29 (edges that float32 does not hold: the entry takes doubles)
    (31, 10.0, 20.5, 24),           # up-scale
    (20, 5.0, 12.5, 768),           # up-scale by 100
    (480, 0.1, 479.9, 256),
    (7, 0.0, 1.0, 5),               # one source pixel
])
def test_coeffs_box_equals_the_restatement(in_size, in0, in1, out_size):
    eb, ek, eks = R.coeffs_box(in_size, in0, in1, out_size)
    gb, gk, gks = _lib_coeffs_box(in_size, in0, in1, out_size)
    assert gks == eks
    assert np.array_equal(gb, eb) and np.array_equal(gk, ek)
    assert (gb[:, 0] >= 0).all() and (gb[:, 0] + gb[:, 1] <= in_size).all() and (gb[:, 1] <= gks).all()       # what the kernels index with


@pytest.mark.parametrize("in_size,out_size", [(640, 768), (480, 768), (1333, 768), (53, 24), (20, 24), (64, 8), (96, 96)])
def test_coeffs_box_of_the_full_axis_is_owl_bicubic_coeffs(in_size, out_size):
    gb, gk, gks = _lib_coeffs_box(in_size, 0.0, float(in_size), out_size)
    bounds = np.zeros(2 * out_size, dtype=np.int32)
    kk = np.zeros(out_size * gks, dtype=np.int32)
    ks = np.zeros(1, dtype=np.int32)
    _lib.call("owl_bicubic_coeffs", in_size, out_size, bounds.ctypes.data, kk.ctypes.data, kk.size, ks.ctypes.data)
    assert int(ks[0]) == gks and np.array_equal(bounds.reshape(-1, 2), gb) and np.array_equal(kk.reshape(out_size, gks), gk)


def test_coeffs_box_refuses_bad_boxes():
    b, k, s = np.zeros(48, np.int32), np.zeros(24 * 13, np.int32), np.zeros(1, np.int32)
    for in0, in1 in ((-0.5, 10.0), (5.0, 5.0), (6.0, 5.0), (0.0, 53.5), (float("nan"), 10.0)):
        with pytest.raises(_lib.OwlLibError, match="owl_bicubic_coeffs_box"):
            _lib.call("owl_bicubic_coeffs_box", 53, in0, in1, 24, b.ctypes.data, k.ctypes.data, k.size, s.ctypes.data)
    with pytest.raises(_lib.OwlLibError, match="capacity"):
        _lib.call("owl_bicubic_coeffs_box", 53, 0.0, 53.0, 24, b.ctypes.data, k.ctypes.data, 10, s.ctypes.data)


def test_build_tile_tables_layout():
    """The descriptors' relative addresses point at the restatement's tables inside the arena; row range and intermediate offsets follow the tables."""
    tiles, _ = R.cases()["mixed"]
    tiles = [P.Tile(*t) for t in tiles]
    desc, arena, tmp_bytes, max_rows = P.build_tile_tables(R.SHAPES, tiles)
    assert desc.shape == (len(tiles), P.TILE_DESC_WORDS) and desc.dtype == np.int64 and arena.dtype == np.int32
    off = 0
    for d, t in zip(desc, tiles):
        H, W = R.SHAPES[t.src]
        bx, kx, ksx = R.coeffs_box(W, t.box[0], t.box[2], t.cw)
        by, ky, ksy = R.coeffs_box(H, t.box[1], t.box[3], t.ch)
        assert tuple(d[[0, 1, 2, 5, 8]]) == (t.src, H, W, ksx, ksy) and tuple(d[12:]) == (t.b, t.x0, t.y0, t.cw, t.ch, int(t.flip))
        assert np.array_equal(arena[d[3] // 4:d[3] // 4 + 2 * t.cw].reshape(-1, 2), bx) and np.array_equal(arena[d[4] // 4:d[4] // 4 + t.cw * ksx].reshape(-1, ksx), kx)
        assert np.array_equal(arena[d[6] // 4:d[6] // 4 + 2 * t.ch].reshape(-1, 2), by) and np.array_equal(arena[d[7] // 4:d[7] // 4 + t.ch * ksy].reshape(-1, ksy), ky)
        assert d[9] == by[0, 0] and d[9] + d[10] == by[-1, 0] + by[-1, 1] <= H
        assert d[11] == off and off % 256 == 0
        off += (int(d[10]) * t.cw * 3 + 255) // 256 * 256
    assert tmp_bytes == off and max_rows == desc[:, 10].max()
    d2 = desc.copy()
    P.resolve_tile_descs(d2, [1000, 2000, 3000], 1 << 40)
    assert np.array_equal(d2[:, 0], (desc[:, 0] + 1) * 1000) and np.array_equal(d2[:, [3, 4, 6, 7]], desc[:, [3, 4, 6, 7]] + (1 << 40))
    assert np.array_equal(np.delete(d2, [0, 3, 4, 6, 7], axis=1), np.delete(desc, [0, 3, 4, 6, 7], axis=1))


def test_tiles_that_do_not_cover_the_canvas_are_refused():
    S = R.SIZE
    for tiles, n_out in R.cases().values():
        P.check_tile_cover(tiles, n_out, S, R.SHAPES)
    tiles, n_out = R.cases()["mixed"]
    with pytest.raises(ValueError, match="cover"):
        P.check_tile_cover(tiles[:-1], n_out, S)                                       # a hole
    with pytest.raises(ValueError, match="overlap"):
        P.check_tile_cover(tiles[:-1] + [tiles[-2]], n_out, S)                         # the right area, one cell twice
    with pytest.raises(ValueError, match="outside"):
        P.check_tile_cover(tiles[:-1] + [tiles[-1]._replace(x0=S - 4)], n_out, S)      # a cell over the edge
    with pytest.raises(ValueError, match="output index"):
        P.check_tile_cover(tiles, n_out - 1, S)
    with pytest.raises(ValueError, match="box"):
        P.check_tile_cover([tiles[0]._replace(box=(1.0, 0.0, 31.5, 17.0))], 1, S, R.SHAPES)   # box wider than its 31-pixel source
    with pytest.raises(ValueError, match="empty"):
        P.check_tile_cover([], 1, S)


# ---- box transform: closed forms -------------------------------------------------------------------------------------------------------------------
W_, H_ = 80.0, 40.0
BOX = np.array([[20.0, 10.0, 40.0, 20.0]])          # xywh: x 20..60, y 10..30


def _tb(crop, flip=False, cell=(0, 0, 24, 24), size=24, boxes=BOX, **kw):
    got = P.transform_boxes(boxes, np.arange(len(boxes)), crop, flip, cell, size, **kw)
    assert got[0].dtype == np.float32
    if kw.pop("drop", True):                              # (the restatement has no last-resort mode)
        ref = R.transform_boxes(boxes, np.arange(len(boxes)), crop, flip, cell, size, **kw)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    return got


def test_box_transform_identity_crop_is_coco_to_model_input():
    import torch
    from owl_vit_object_detection_amd.train_util import coco_to_model_input
    b, l = _tb((0.0, 0.0, W_, H_))
    assert np.array_equal(b, np.array([[0.25, 0.25, 0.75, 0.75]], dtype=np.float32)) and l.tolist() == [0]
    want = coco_to_model_input(torch.from_numpy(BOX).float(), {"width": W_, "height": H_})
    assert np.array_equal(b, want.numpy())


def test_box_transform_half_image_crop_and_flip():
    b, _ = _tb((0.0, 0.0, 40.0, H_))                  # left half: x 20..40 of 0..40 visible (half the box)
    assert np.array_equal(b, np.array([[0.5, 0.25, 1.0, 0.75]], dtype=np.float32))
    b, _ = _tb((0.0, 0.0, 40.0, H_), flip=True)
    assert np.array_equal(b, np.array([[0.0, 0.25, 0.5, 0.75]], dtype=np.float32))
    b, _ = _tb((0.0, 0.0, W_, H_), flip=True, boxes=np.array([[8.0, 10.0, 24.0, 20.0]]))      # x 8..32 of 80 -> mirrored 48..72
    assert np.array_equal(b, np.array([[0.6, 0.25, 0.9, 0.75]], dtype=np.float32))


def test_box_transform_visibility_threshold_is_inclusive():
    # x 20..60 cut at 32: 12 of 40 columns = exactly 0.3 of the area stays; at 31.875 it is below
    b, l = _tb((0.0, 0.0, 32.0, H_), min_visibility=0.3)
    assert len(b) == 1 and np.array_equal(b, np.array([[0.625, 0.25, 1.0, 0.75]], dtype=np.float32))
    b, l = _tb((0.0, 0.0, 31.875, H_), min_visibility=0.3)
    assert len(b) == 0 and len(l) == 0 and b.shape == (0, 4)
    b, _ = _tb((0.0, 0.0, 31.875, H_), min_visibility=0.3, drop=False)                         # the sampler's last resort keeps it
    assert len(b) == 1


def test_box_transform_min_box_is_measured_in_canvas_pixels():
    small = np.array([[10.0, 10.0, 8.0, 20.0]])       # 8 source pixels wide; canvas 24 over 80 -> 2.4 px; over a 12-px cell -> 1.2 px
    assert len(_tb((0.0, 0.0, W_, H_), boxes=small, min_box=2.0)[0]) == 1
    assert len(_tb((0.0, 0.0, W_, H_), boxes=small, min_box=2.0, cell=(12, 0, 12, 12))[0]) == 0
    assert len(_tb((0.0, 0.0, W_, H_), boxes=np.array([[10.0, 10.0, 20.0 / 3.0, 20.0]]), min_box=2.0)[0]) == 1      # exactly 2 px: kept


def test_box_transform_cell_offsets_of_a_2x2_mosaic():
    for q, (cx, cy) in enumerate(((0, 0), (12, 0), (0, 12), (12, 12))):
        b, _ = _tb((0.0, 0.0, W_, H_), cell=(cx, cy, 12, 12))
        want = np.array([[cx / 24 + 0.125, cy / 24 + 0.125, cx / 24 + 0.375, cy / 24 + 0.375]], dtype=np.float32)
        assert np.array_equal(b, want), q
    b, l = _tb((40.0, 20.0, W_, H_), cell=(12, 12, 12, 12), boxes=np.array([[20.0, 10.0, 40.0, 20.0], [0.0, 0.0, 30.0, 15.0]]), min_visibility=0.25)
    assert l.tolist() == [0] and np.array_equal(b, np.array([[0.5, 0.5, 0.75, 0.75]], dtype=np.float32))          # a quarter of box 0 is visible; box 1 is outside the crop


# ---- sampler ---------------------------------------------------------------------------------------------------------------------------------------
def _batch(n=6):
    shapes = [R.SHAPES[i % 3] for i in range(n)]
    boxes = [np.array([[w / 4, h / 4, w / 2, h / 2]]) for h, w in shapes]          # each source: one box over its central quarter
    labels = [np.array([i % 4]) for i in range(n)]
    return shapes, boxes, labels


def _same(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))


def test_sampler_is_keyed_by_seed_rank_epoch_index():
    shapes, boxes, labels = _batch()
    kw = dict(mosaic=(1, 2, 3), seed=7)
    ref = P.TrainAugment(R.SIZE, **kw).sample(shapes, boxes, labels, 2, 5)
    a = P.TrainAugment(R.SIZE, **kw)
    a.sample(shapes, boxes, labels, 0, 0)                                          # earlier calls leave no trace
    assert _same(a.sample(shapes, boxes, labels, 2, 5), ref)
    assert not _same(P.TrainAugment(R.SIZE, rank=1, **kw).sample(shapes, boxes, labels, 2, 5), ref)
    assert not _same(a.sample(shapes, boxes, labels, 3, 5), ref)
    assert not _same(a.sample(shapes, boxes, labels, 2, 6), ref)
    assert not _same(P.TrainAugment(R.SIZE, mosaic=(1, 2, 3), seed=8).sample(shapes, boxes, labels, 2, 5), ref)


def test_sampler_invariants():
    shapes, boxes, labels = _batch(10)
    S = R.SIZE
    a = P.TrainAugment(S, mosaic=(1, 2, 3), seed=1)
    grids, flips, srcs_of_cell0 = set(), set(), []
    for index in range(40):
        tiles, ob, ol = a.sample(shapes, boxes, labels, 0, index)
        P.check_tile_cover(tiles, len(shapes), S, shapes)                          # cells tile every canvas; boxes inside their sources
        per_out = [[t for t in tiles if t.b == j] for j in range(len(shapes))]
        for j, ts in enumerate(per_out):
            g = S // ts[0].cw
            grids.add(g)
            assert len(ts) == g * g and ts[0].src == j and all(t.cw == t.ch == S // g for t in ts)
            assert len({t.src for t in ts}) == len(ts)                            # 10 images: without replacement
            for t in ts:
                flips.add(t.flip)
                H, W = shapes[t.src]
                l, u, r, lo = t.box
                assert all(float(np.float32(v)) == v for v in t.box)              # what Pillow's box= holds
                frac = (r - l) * (lo - u) / (H * W)
                assert 0.3 - 1e-3 <= frac <= 1.0 + 1e-6
                rel = ((r - l) / (lo - u)) / (W / H)
                assert 0.75 - 1e-2 <= rel <= 4 / 3 + 1e-2 or r - l == W or lo - u == H
        for b, l in zip(ob, ol):
            assert b.dtype == np.float32 and b.shape[1] == 4 and len(b) == len(l) >= 1          # every output image has a target
            assert (b >= 0).all() and (b <= 1).all() and (b[:, 2] > b[:, 0]).all() and (b[:, 3] > b[:, 1]).all()
    assert grids == {1, 2, 3} and flips == {False, True}
    assert a.fallbacks == 0              # a condition on these inputs (central-quarter boxes), checked when the test was written


def test_sampler_targets_are_the_box_transform_of_its_tiles():
    shapes, boxes, labels = _batch()
    S = R.SIZE
    tiles, ob, ol = P.TrainAugment(S, mosaic=(2,), seed=4).sample(shapes, boxes, labels, 0, 0)
    for j in range(len(shapes)):
        rb = [R.transform_boxes(boxes[t.src], labels[t.src], t.box, t.flip, (t.x0, t.y0, t.cw, t.ch), S) for t in tiles if t.b == j]
        assert np.array_equal(ob[j], np.concatenate([b for b, _ in rb])) and np.array_equal(ol[j], np.concatenate([l for _, l in rb]))


def test_sampler_small_batch_and_fallback():
    shapes, boxes, labels = _batch(2)                                               # 2 images, 4 cells: sources repeat
    a = P.TrainAugment(R.SIZE, mosaic=(2,), seed=0)
    tiles, ob, _ = a.sample(shapes, boxes, labels, 0, 0)
    assert len(tiles) == 8 and tiles[0].src == 0 and tiles[4].src == 1
    # a box that no crop of at most 30 % of the area can keep 99 % visible: every draw comes back empty -> whole source, g = 1, no flip
    a = P.TrainAugment(R.SIZE, mosaic=(2,), scale=(0.3, 0.3), min_visibility=0.99, seed=0, max_tries=3)
    big = [np.array([[0.0, 0.0, float(w), float(h)]]) for h, w in shapes]
    tiles, ob, ol = a.sample(shapes, big, labels, 0, 0)
    assert a.fallbacks == 2 and len(tiles) == 2
    for j, t in enumerate(tiles):
        assert t == P.Tile(j, (0.0, 0.0, float(shapes[j][1]), float(shapes[j][0])), False, j, 0, 0, R.SIZE, R.SIZE)
        assert np.array_equal(ob[j], np.array([[0, 0, 1, 1]], dtype=np.float32))
    with pytest.raises(ValueError, match="no box"):
        a.sample(shapes, [np.zeros((0, 4))] * 2, [np.zeros(0, dtype=np.int64)] * 2, 0, 0)


def test_constructor_checks():
    with pytest.raises(ValueError, match="divide"):
        P.TrainAugment(24, mosaic=(1, 5))
    with pytest.raises(ValueError):
        P.TrainAugment(24, scale=(0.0, 1.0))
    assert P.TrainAugment(768, mosaic=(1, 2, 3)).mosaic == (1, 2, 3)
