"""-m gpu: sliced inference on the device.  owl_slice_merge (csrc/slice_merge.hip: sm_sort_kernel, sm_mask_kernel, sm_scan_kernel) against the float64
reference of tests/slice_merge_reference.py on every named case and both metrics -- kept candidates, classes, counts and the BITS of scores and mapped boxes
--, its identity with owl_postprocess, `DeviceImageProcessor.slices` against the tile path and the restatement of Pillow's boxed resize, and `detect_sliced`
on the tiny model against the same steps done by hand.  A case is compared with float64 only because it has 0 undecided pairs (asserted): then any correct
f32 evaluation must return that list."""
import numpy as np
import pytest
import torch

from tests import slice_merge_reference as M

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8))


def run(c, metric, class_aware=None, max_out=None, n_max=None):
    """ops.slice_merge on a case dict -> padded numpy outputs (boxes, classes, scores, src, counts)."""
    from owl_vit_object_detection_amd import ops
    dev = "cuda"
    G = len(c["slice_offsets"]) - 1
    n_max = M.n_max(c) if n_max is None else n_max
    max_out = max_out or c.get("max_out") or n_max
    aware = c.get("class_aware", True) if class_aware is None else class_aware
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = ops.slice_merge(t(c["boxes"]), t(c["scores"]), t(c["classes"]), t(c["counts"]), t(c["xform"]), t(c["slice_offsets"]), G, n_max, max_out,
                          float(c["thr"]), metric, aware)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def matches(out, g, r):
    ob, oc, os_, osrc, cnt = out
    k = len(r.src)
    return (cnt[g] == k and np.array_equal(osrc[g, :k], r.src) and np.array_equal(oc[g, :k], r.classes)
            and np.array_equal(bits(os_[g, :k]), bits(r.scores)) and np.array_equal(bits(ob[g, :k]), bits(r.boxes)))


def assert_is(out, g, r, what=""):
    ob, oc, os_, osrc, cnt = out
    k = len(r.src)
    assert cnt[g] == k, (what, g, int(cnt[g]), k)
    assert np.array_equal(osrc[g, :k], r.src), what
    assert np.array_equal(oc[g, :k], r.classes), what
    assert np.array_equal(bits(os_[g, :k]), bits(r.scores)) and np.array_equal(bits(ob[g, :k]), bits(r.boxes)), what
    assert oc.dtype == np.int64 and osrc.dtype == np.int64 and cnt.dtype == np.int32
    assert np.all(oc[g, k:] == -1) and np.all(osrc[g, k:] == -1) and np.all(bits(os_[g, k:]) == 0) and np.all(bits(ob[g, k:]) == 0)      # the documented pads


@pytest.mark.parametrize("metric", M.METRICS)
@pytest.mark.parametrize("name", M.CASES)
def test_named_cases(name, metric):
    c = M.case(name)
    refs = M.cached_reference(name, metric)
    out = run(c, metric)
    again = run(c, metric)
    for a, b in zip(out, again):
        assert same(a, b)                                                  # two runs, the same bits
    assert out[0].shape == (len(refs), c.get("max_out") or M.n_max(c), 4)
    for g, r in enumerate(refs):
        assert r.undecided == 0
        assert_is(out, g, r, f"{name} {metric} source image {g}")
    if "expect" in c:
        assert out[3][0, :out[4][0]].tolist() == c["expect"][metric]
        ag = run(c, metric, class_aware=False)
        assert ag[3][0, :ag[4][0]].tolist() == c["expect"][metric + "_agnostic"]
    if "expect_src" in c:
        assert np.array_equal(out[3][0, :out[4][0]], c["expect_src"])


@pytest.mark.parametrize("plant", sorted(M.PLANTS))
def test_planted_errors_differ_from_the_device(plant):
    """The device equals the unplanted reference (test_named_cases); each planted reference is another list, so the device does not make that error."""
    name, metric = M.PLANTS[plant]
    out = run(M.case(name), metric)
    assert all(matches(out, g, r) for g, r in enumerate(M.cached_reference(name, metric)))
    assert not all(matches(out, g, r) for g, r in enumerate(M.cached_reference(name, metric, plant))), plant


def test_groups_are_independent():
    """A source image's list does not depend on the other source images of the call, nor on its position in it, nor on a larger n_max."""
    c = M.case("ragged")
    for metric in M.METRICS:
        joint = run(c, metric)
        K = c["K"]
        for g, (a, b) in enumerate(((0, 1), (1, 7))):
            alone = dict(c, boxes=c["boxes"][a:b], scores=c["scores"][a:b], classes=c["classes"][a:b], counts=c["counts"][a:b], xform=c["xform"][a:b],
                         slice_offsets=np.asarray([0, b - a], np.int32))
            single = run(alone, metric, n_max=6 * K)
            for x, y in zip(joint, single):
                assert same(x[g], y[0]), (metric, g)
        order = np.r_[1:7, 0:1]
        swapped = dict(c, boxes=c["boxes"][order], scores=c["scores"][order], classes=c["classes"][order], counts=c["counts"][order], xform=c["xform"][order],
                       slice_offsets=np.asarray([0, 6, 7], np.int32))
        moved = run(swapped, metric)
        for x, y in zip(joint, moved):
            assert same(x[0], y[1]) and same(x[1], y[0])
        wide = run(c, metric, n_max=8192, max_out=6 * K)
        for x, y in zip(joint, wide):
            assert same(x, y)


@pytest.mark.parametrize("P", (200, 8192))
def test_one_whole_image_slice_with_iou_is_postprocess(P):
    """One group of one slice, xform (1, 0, 1, 0), metric iou, thr = the NMS threshold, per-class route: merging owl_postprocess' output returns it bit for bit."""
    from owl_vit_object_detection_amd import ops
    from tests import postprocess_reference as R
    boxes, sims = R.random_case(P, 3, 900 + P)
    pb, pc, ps, pp, pcnt = ops.postprocess(torch.from_numpy(boxes).cuda()[None], torch.from_numpy(sims).cuda()[None], P, R.CONF, R.TEMPLATE_THR, "per_class")
    k = int(pcnt[0])
    assert 0 < k < P
    xf = torch.tensor([[1.0, 0.0, 1.0, 0.0]], device="cuda")
    offs = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    mb, mc, ms, msrc, mcnt = ops.slice_merge(pb, ps, pc, pcnt, xf, offs, 1, P, P, R.TEMPLATE_THR, "iou", True)
    assert int(mcnt[0]) == k and torch.equal(msrc[0, :k].cpu(), torch.arange(k)) and bool((msrc[0, k:] == -1).all())
    for a, b in ((mb, pb), (mc, pc), (ms, ps)):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_argument_checks():
    from owl_vit_object_detection_amd import _lib, ops
    c = M.case("cluster_2")
    with pytest.raises(_lib.OwlLibError, match="8192"):
        run(c, "ios", n_max=8193)
    with pytest.raises(_lib.OwlLibError, match="metric"):
        run(c, 2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    with pytest.raises(ValueError, match="slice_offsets"):
        ops.slice_merge(t(c["boxes"]), t(c["scores"]), t(c["classes"]), t(c["counts"]), t(c["xform"]), t(c["slice_offsets"]), 2, 200, 10, 0.5, "ios", True)
    with pytest.raises(TypeError, match="classes"):
        ops.slice_merge(t(c["boxes"]), t(c["scores"]), t(c["classes"]).int(), t(c["counts"]), t(c["xform"]), t(c["slice_offsets"]), 1, 200, 10, 0.5, "ios", True)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the slices themselves
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _images():
    rng = np.random.default_rng(11)
    return [rng.integers(0, 256, (160, 224, 3), dtype=np.uint8), rng.integers(0, 256, (50, 300, 3), dtype=np.uint8)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_slices_are_tiles_and_pillows_boxed_resize(dtype):
    from owl_vit_object_detection_amd.preprocess import DeviceImageProcessor
    from tests import augment_reference as A
    imgs = _images()
    ip = DeviceImageProcessor(size=96, dtype=dtype)
    got, plan = ip.slices(imgs)
    got = got.clone()
    assert plan.slice_offsets.tolist() == [0, 7, 12] and got.dtype == dtype and tuple(got.shape) == (12, 3, 96, 96)       # 2 x 3 + 1 | 1 x 4 + 1
    assert torch.equal(got, ip.tiles(imgs, plan.tiles, len(plan.tiles)))
    want = torch.from_numpy(A.pixel_values(A.render(imgs, plan.tiles, len(plan.tiles), 96)))
    assert torch.equal(got.cpu(), want.to(dtype))
    # an image of the model's own size: one slice, bitwise the plain processor
    sq = np.random.default_rng(12).integers(0, 256, (96, 96, 3), dtype=np.uint8)
    one, plan1 = ip.slices(sq)
    one = one.clone()
    assert plan1.slice_offsets.tolist() == [0, 1] and plan1.xform.tolist() == [[1, 0, 1, 0]]
    assert torch.equal(one, ip(images=sq)["pixel_values"])
    # windows larger than the model's input (a down-scale) go through the same path
    down, plan2 = ip.slices(imgs[:1], slice_size=128, overlap=0.25)
    want2 = torch.from_numpy(A.pixel_values(A.render(imgs[:1], plan2.tiles, len(plan2.tiles), 96)))
    assert len(plan2.tiles) == 5 and torch.equal(down.cpu(), want2.to(dtype))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_detect_sliced_on_the_tiny_model_equals_the_steps_by_hand():
    from owl_vit_object_detection_amd import metrics, train_util
    from owl_vit_object_detection_amd.models import PostProcess, load_model
    from owl_vit_object_detection_amd.postprocess import SlicedPostProcess, detect_sliced
    from owl_vit_object_detection_amd.preprocess import DeviceImageProcessor
    CONF, IOU, MERGE, K = 0.01, 0.6, 0.45, 20
    model = load_model({str(i): i for i in range(4)}, "cuda", arch="tiny").eval()
    ip = DeviceImageProcessor(size=96, dtype=torch.float32)
    imgs = _images()
    post = SlicedPostProcess(CONF, IOU, merge_threshold=MERGE, per_slice_top_k=K)
    boxes, classes, scores, plan = detect_sliced(model, ip, imgs, post, batch=32)
    counts, src = post.last_counts.cpu().numpy(), post.last_src.cpu().numpy()
    got = (boxes.cpu().numpy(), classes.cpu().numpy(), scores.cpu().numpy(), src, counts)
    assert plan.slice_offsets.tolist() == [0, 7, 12] and boxes.shape == (2, counts.max(), 4) and classes.shape == scores.shape == src.shape == (2, counts.max())

    # by hand: the model on each slice alone, PostProcess per slice, the float64 merge
    pv, plan_h = ip.slices(imgs)
    pv = pv.clone()
    pp = PostProcess(CONF, IOU)
    per = []
    with torch.no_grad():
        for t in range(pv.shape[0]):
            pb, _, ps, _ = model(pv[t:t + 1])
            b, c, s = pp(pb, ps)
            per.append((b[0, :K].cpu().numpy(), s[0, :K].cpu().numpy(), c[0, :K].cpu().numpy()))
    assert sum(len(p[1]) for p in per) > 24 and max(len(p[1]) for p in per) == K          # something to merge, and the per-slice cut is reached
    case = M.pack(per, plan_h.xform, plan_h.slice_offsets, MERGE, K=K)
    refs = M.reference(case, "ios")
    for g, r in enumerate(refs):
        assert r.undecided == 0
        assert 0 < len(r.src) < r.n                                                       # the merge removed something
        k = len(r.src)
        assert counts[g] == k and np.array_equal(src[g, :k], r.src) and np.array_equal(got[1][g, :k], r.classes)
        assert np.array_equal(bits(got[2][g, :k]), bits(r.scores)) and np.array_equal(bits(got[0][g, :k]), bits(r.boxes))
        assert np.all(got[1][g, k:] == -1) and np.all(bits(got[2][g, k:]) == 0)
    assert len(set((refs[0].src // K).tolist())) > 1                                      # the list draws on several slices

    # chunking the forward changes nothing; top_k is a prefix and does not synchronise on the counts
    b1, c1, s1, _ = detect_sliced(model, ip, imgs, post, batch=1)
    assert torch.equal(b1.view(torch.uint8), boxes.view(torch.uint8)) and torch.equal(c1, classes) and torch.equal(s1.view(torch.uint8), scores.view(torch.uint8))
    b5, c5, s5, _ = detect_sliced(model, ip, imgs, post, batch=5, top_k=4)
    assert b5.shape == (2, 4, 4) and torch.equal(c5, classes[:, :4]) and torch.equal(s5.view(torch.uint8), scores[:, :4].view(torch.uint8))
    assert post.last_counts.tolist() == [4, 4]

    # the result is what the eval loop's metric takes
    metric = metrics.MeanAveragePrecision(n_classes=4)
    gt_boxes = torch.tensor([[[0.1, 0.1, 0.5, 0.5], [0.4, 0.3, 0.9, 0.8]], [[0.2, 0.1, 0.6, 0.9], [0, 0, 0, 0]]])
    gt_labels = torch.tensor([[0, 2], [1, -1]])
    meta = {"width": torch.tensor([224.0, 300.0]), "height": torch.tensor([160.0, 50.0])}
    train_util.update_metrics(metric, meta, boxes, classes, scores, gt_boxes, gt_labels)
    res = metric.compute()
    assert "map" in res and np.isfinite(float(res["map"]))
