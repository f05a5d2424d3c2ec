"""CPU: the float64 merge reference of tests/slice_merge_reference.py on its named cases (0 undecided pairs everywhere, hand-written lists on the dyadic
lattice), every planted error shown to change a list, the slice grid's closed forms, the xform rows against float64, and SlicedPostProcess' argument
errors.  No GPU: tests/test_slice_merge_gpu.py runs the same cases through owl_slice_merge."""
import numpy as np
import pytest

from tests import slice_merge_reference as M

f32 = np.float32


@pytest.mark.parametrize("metric", M.METRICS)
@pytest.mark.parametrize("name", M.CASES)
def test_every_case_is_decided(name, metric):
    c = M.case(name)
    res = M.cached_reference(name, metric)
    assert len(res) == len(c["slice_offsets"]) - 1
    for g, r in enumerate(res):
        assert r.undecided == 0, (name, metric, g, r.undecided)
        k = len(r.src)
        assert r.boxes.shape == (k, 4) and r.boxes.dtype == f32 and r.scores.dtype == f32 and r.classes.dtype == np.int64 and r.src.dtype == np.int64
        assert len(set(r.src.tolist())) == k and k <= r.n
        key = r.scores.astype(np.float64) + 0.0
        assert np.all(key[:-1] >= key[1:]) and np.all((key[:-1] > key[1:]) | (r.src[:-1] < r.src[1:]))       # score descending, ties by c
        sl, rank = c["slice_offsets"][g] + r.src // c["K"], r.src % c["K"]
        assert np.all(rank < c["counts"][sl]) and not np.isnan(r.scores).any()
        assert np.array_equal(r.scores.view(np.uint32), c["scores"][sl, rank].view(np.uint32))                # the input's bits


def test_lattice_by_hand():
    c = M.case("lattice")
    assert c["K"] == 3 and c["counts"].tolist() == [2, 1, 1, 1, 3]
    for metric in M.METRICS:
        r = M.cached_reference("lattice", metric)[0]
        assert r.src.tolist() == c["expect"][metric] and r.n == 8
        a = M.reference(c, metric, class_aware=False)[0]
        assert a.undecided == 0 and a.src.tolist() == c["expect"][metric + "_agnostic"]
    iou, ios = (M.cached_reference("lattice", m)[0] for m in M.METRICS)
    # the small box inside the large one: every mapped coordinate is exact, IoS = 1 and IoU = 1 / 16, so the metrics disagree about it
    assert iou.boxes[2].tolist() == [0.25, 0.25, 0.375, 0.375] and iou.boxes[0].tolist() == [0.25, 0.25, 0.75, 0.75] and 0 not in ios.src
    big, small = iou.boxes[0].astype(np.float64), iou.boxes[2:3].astype(np.float64)
    assert M.pair_ios(big, small)[0][0] == 1.0 and M.pair_iou(big, small)[0][0] == 1.0 / 16
    # the unit boxes a quarter apart, from slices with different maps
    u = M.map_boxes(c["boxes"][3, :1], c["xform"][3:4])
    U = M.map_boxes(c["boxes"][4, 1:2], c["xform"][4:5])
    assert u.tolist() == [[20.5, 20.5, 21.5, 21.5]] and U.tolist() == [[20.75, 20.5, 21.75, 21.5]]
    assert M.pair_iou(U[0].astype(np.float64), u.astype(np.float64))[0][0] == 0.6 and M.pair_ios(U[0].astype(np.float64), u.astype(np.float64))[0][0] == 0.75


def test_pair_ios_bound_and_zero_rules():
    bi = np.asarray([0, 0, 2, 2], np.float64)
    bj = np.asarray([[1, 1, 3, 3], [2, 0, 3, 1], [5, 5, 6, 6], [1, 1, 1, 1], [0.5, 0.5, 1.5, 1.0]], np.float64)
    ios, e, sure = M.pair_ios(bi, bj)
    assert ios[0] == 0.25 and 0 < e[0] < 1e-6                            # inter 1 over min(4, 4)
    assert ios[1] == 0 and ios[2] == 0 and sure[1] and sure[2] and e[1] == 0 and e[2] == 0      # touching / disjoint: exactly 0
    assert np.isnan(ios[3]) and sure[3]                                   # a point: 0 / 0
    assert ios[4] == 1.0 and not sure[4]                                  # wholly inside
    # f32 evaluations of the same formula, in two association orders of the products, land within the bound
    rng = np.random.default_rng(0)
    for _ in range(200):
        a = rng.random(4).astype(f32); a[2:] += a[:2]
        b = rng.random(4).astype(f32); b[2:] += b[:2]
        v, e, _ = M.pair_ios(a.astype(np.float64), b[None].astype(np.float64))
        ai, aj = f32(a[2] - a[0]) * f32(a[3] - a[1]), f32(b[2] - b[0]) * f32(b[3] - b[1])
        w = max(f32(0), f32(min(a[2], b[2]) - max(a[0], b[0])))
        h = max(f32(0), f32(min(a[3], b[3]) - max(a[1], b[1])))
        got = f32(f32(w * h) / min(ai, aj))
        assert abs(float(got) - v[0]) <= e[0]


def test_merge_nms_iou_is_exact_nms():
    from tests import postprocess_reference as R
    b, s = R.random_case(150, 3, 5, cluster=True)
    cls = s.argmax(1)
    k0, u0 = R.exact_nms(b, cls, 0.45)
    k1, u1 = M.merge_nms(b, cls, 0.45, "iou")
    assert np.array_equal(k0, k1) and u0 == u1
    k2, _ = M.merge_nms(b, cls, 0.45, "ios")
    assert len(k2) < len(k0) or not np.array_equal(k0, k2)               # IoS >= IoU: it suppresses at least as much


@pytest.mark.parametrize("plant", sorted(M.PLANTS))
def test_planted_errors_change_a_list(plant):
    name, metric = M.PLANTS[plant]
    good, bad = M.cached_reference(name, metric), M.cached_reference(name, metric, plant)
    differs = any(not (np.array_equal(a.src, b.src) and np.array_equal(a.boxes.view(np.uint32), b.boxes.view(np.uint32))) for a, b in zip(good, bad))
    assert differs, plant
    if plant not in ("no_offset", "xform0", "swap_sxsy", "add_first"):   # those move the boxes; the others must show in the kept candidates themselves
        assert any(not np.array_equal(a.src, b.src) for a, b in zip(good, bad)), plant


def test_case_claims():
    assert {M.n_max(M.case(f"n_{n}")) for n in M._SIZES} == set(M._SIZES)
    for n in M._SIZES:
        assert M.cached_reference(f"n_{n}", "iou")[0].n == n              # every candidate live: n_valid on both sides of 64 / 1024 / 4096
    c = M.case("scan_edges")
    assert M.n_max(c) == 8192
    for metric in M.METRICS:
        r = M.cached_reference("scan_edges", metric)[0]
        assert r.n == 8192 and np.array_equal(r.src, c["expect_src"]) and len(r.src) == 8192 - 3
    assert M.case("empty_slice")["counts"][2] == 0 and M.case("all_empty")["counts"].tolist() == [0] * 4
    assert [r.n for r in M.cached_reference("all_empty", "ios")] == [0]
    assert M.case("k_one")["K"] == 1 and len(M.case("k_one")["xform"]) == 13
    nz = M.case("nan_zeros")
    live = M.cached_reference("nan_zeros", "ios")[0]
    assert int(np.isnan(nz["scores"][nz["scores"] != 2.0]).sum()) == 2 and live.n == 28
    zeros = live.scores[live.scores == 0]
    assert np.signbit(zeros).any() and (~np.signbit(zeros)).any()
    src0 = live.src[live.scores == 0]
    assert np.all(src0[:-1] < src0[1:])                                   # both zeros are one key: c decides
    rg = M.case("ragged")
    assert np.diff(rg["slice_offsets"]).tolist() == [1, 6] and [r.n for r in M.cached_reference("ragged", "ios")] == [50, 180]
    t = M.case("ties")
    assert len(np.unique(t["scores"][t["scores"] != 2.0])) == 4
    mo = M.case("max_out")
    full = M.reference(mo, "ios", max_out=10 ** 6)[0]
    cut = M.cached_reference("max_out", "ios")[0]
    assert len(full.src) > 9 == len(cut.src) and np.array_equal(full.src[:9], cut.src)
    ag, aw = M.cached_reference("agnostic", "ios")[0], M.cached_reference("cluster_13", "ios")[0]
    assert len(ag.src) < len(aw.src)                                      # the same candidates, class-aware against class-agnostic
    assert len(M.case("cluster_1")["xform"]) == 1 and len(M.case("cluster_2")["xform"]) == 2 and len(M.case("cluster_13")["xform"]) == 13
    for name in ("cluster_13", "n_1025"):                                 # the two metrics give different lists on ordinary inputs too
        assert not np.array_equal(M.cached_reference(name, "iou")[0].src, M.cached_reference(name, "ios")[0].src)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the slice grid
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_slice_starts_closed_forms():
    from owl_vit_object_detection_amd.preprocess import slice_starts
    assert slice_starts(160, 96, 0.25) == [(0, 96), (64, 160)]
    assert slice_starts(96, 96, 0.25) == [(0, 96)] and slice_starts(96, 96, 5.0) == [(0, 96)] and slice_starts(50, 96, 0.2) == [(0, 50)]
    assert slice_starts(97, 96, 0.0) == [(0, 96), (1, 97)] and slice_starts(192, 96, 0.0) == [(0, 96), (96, 192)]
    assert slice_starts(200, 96, 0.2) == [(0, 96), (77, 173), (104, 200)]
    for n in list(range(1, 420, 7)) + [96, 97, 192, 4000]:
        for s in (1, 5, 96, 100):
            for overlap in (0.0, 0.2, 0.25, 0.5, 0.99):
                if s - int(s * overlap) < 1:
                    continue
                w = slice_starts(n, s, overlap)
                if n <= s:
                    assert w == [(0, n)]
                    continue
                assert all(hi - lo == s for lo, hi in w) and w[0][0] == 0 and w[-1][1] == n
                assert all(b[0] > a[0] for a, b in zip(w, w[1:]))                                            # strictly advancing: no window twice
                assert all(a[1] - b[0] >= int(s * overlap) for a, b in zip(w, w[1:]))                        # consecutive overlap (and no gap: the union covers)
                step = s - int(s * overlap)
                assert all(b[0] - a[0] == step for a, b in zip(w[:-2], w[1:-1])) and w[-1][0] - w[-2][0] <= step
    for bad in (1.0, 1.5):
        with pytest.raises(ValueError, match="step"):
            slice_starts(200, 96, bad)
    with pytest.raises(ValueError):
        slice_starts(200, 96, -0.5)


def test_slice_plan():
    from owl_vit_object_detection_amd.preprocess import SlicePlan, Tile, slice_plan, slice_starts
    shapes = [(200, 300), (96, 96), (50, 300), (96, 160)]
    plan = slice_plan(shapes, 96, 0.2)
    assert isinstance(plan, SlicePlan) and plan.shapes == shapes
    assert plan.slice_offsets.dtype == np.int32 and plan.slice_offsets.tolist() == [0, 13, 14, 19, 22]     # 3 x 4 + 1 | 1 | 1 x 4 + 1 | 1 x 2 + 1
    assert plan.xform.dtype == f32 and plan.xform.shape == (22, 4) and len(plan.tiles) == 22
    for t, tile in enumerate(plan.tiles):
        assert isinstance(tile, Tile) and (tile.flip, tile.b, tile.x0, tile.y0, tile.cw, tile.ch) == (False, t, 0, 0, 96, 96)
        g = int(np.searchsorted(plan.slice_offsets, t, side="right") - 1)
        H, W = shapes[g]
        l, u, r, lo = tile.box
        assert tile.src == g and 0 <= l < r <= W and 0 <= u < lo <= H
        want = np.asarray([(r - l) / W, l / W, (lo - u) / H, u / H], np.float64).astype(f32)                 # formed in float64, rounded once
        assert np.array_equal(plan.xform[t].view(np.uint32), want.view(np.uint32))
    # row-major product of the axes' windows, then the whole image
    boxes0 = [t.box for t in plan.tiles[:13]]
    assert boxes0[:12] == [(l, u, r, lo) for (u, lo) in slice_starts(200, 96, 0.2) for (l, r) in slice_starts(300, 96, 0.2)] and boxes0[12] == (0, 0, 300, 200)
    assert plan.tiles[13].box == (0, 0, 96, 96) and plan.xform[13].tolist() == [1, 0, 1, 0]                  # one window: no extra whole-image slice
    assert plan.tiles[18].box == (0, 0, 300, 50)
    assert slice_plan(shapes, 96, 0.2, full_image=False).slice_offsets.tolist() == [0, 12, 13, 17, 19]
    assert np.array_equal(M.plan_xform(200, 300, 96, 0.2), plan.xform[:13]) and np.array_equal(M.plan_xform(96, 160, 96, 0.2), plan.xform[19:])
    # the processor's size may differ from the window: S is the canvas every slice is resampled to
    big = slice_plan([(200, 300)], 128, 0.25, size=96)
    assert all((t.cw, t.ch) == (96, 96) for t in big.tiles) and big.tiles[0].box == (0, 0, 128, 128)
    with pytest.raises(ValueError):
        slice_plan(shapes, 96, 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# SlicedPostProcess: argument errors (raised before anything touches a device)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_sliced_postprocess_argument_errors():
    import torch
    from owl_vit_object_detection_amd.postprocess import SlicedPostProcess
    from owl_vit_object_detection_amd.preprocess import slice_plan
    with pytest.raises(ValueError, match="merge_metric"):
        SlicedPostProcess(merge_metric="giou")
    with pytest.raises(ValueError, match="nms_route"):
        SlicedPostProcess(nms_route="fast")
    pp = SlicedPostProcess(0.1, 0.3)
    assert pp.merge_threshold == 0.3 and pp.merge_metric == "ios" and pp.per_slice_top_k == 200 and not pp.class_agnostic_merge
    assert SlicedPostProcess(0.1, 0.3, merge_threshold=0.6).merge_threshold == 0.6
    plan = slice_plan([(200, 300), (96, 96)], 96, 0.2)                   # 13 + 1 slices
    with pytest.raises(ValueError, match="14 slices"):
        pp(torch.zeros(13, 36, 4), torch.zeros(13, 36, 3), plan)
    with pytest.raises(ValueError, match=r"expected boxes \[T,P,4\]"):
        pp(torch.zeros(14, 36, 4), torch.zeros(14, 35, 3), plan)
    many = slice_plan([(96, 96), (1000, 1000)], 96, 0.2)                 # 13 x 13 + 1 = 170 slices in source image 1
    n = len(many.tiles)
    with pytest.raises(ValueError, match=r"source image 1 .*170 slices.*per_slice_top_k 200.*8192"):
        pp(torch.zeros(n, 36, 4), torch.zeros(n, 36, 3), many)
    with pytest.raises(ValueError, match=r"source image 0 .*13 slices.*per_slice_top_k 700.*8192"):
        SlicedPostProcess(per_slice_top_k=700)(torch.zeros(14, 36, 4), torch.zeros(14, 36, 3), plan)
