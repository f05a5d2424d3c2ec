"""COCO bbox mAP on the device (csrc/metrics.hip through metrics.MeanAveragePrecision) against the numpy restatement of the protocol
(tests/coco_eval_restatement.py).  The records (matched / ignored bits, ranks, ground-truth counts) are integers and the precision / recall arrays
are IEEE f64 quotients of the same integers with the same eps: all compared with array_equal.  The mean summaries are compared at 1e-9 (rounding
bound of an f64 mean over fewer than 10^6 values in [0, 1]; the device sums in another order than numpy).

The edge cases aimed at the kernels' own forms (compactions, rank cut, ground-truth order, area edges, the matching chain, padding, in-kernel scaling,
and owl_map_accumulate on hand-built records) are in tests/test_metrics_edges_gpu.py; profiles/eval_map_edges.md lists them."""
import numpy as np
import pytest
import torch

from tests import coco_eval_restatement as R

pytestmark = pytest.mark.gpu

TOL = 1e-9
SCALARS = ("map", "map_50", "map_75", "map_small", "map_medium", "map_large", "mar_1", "mar_10", "mar_100", "mar_small", "mar_medium", "mar_large")


def _metric(n_classes=None):
    from owl_vit_object_detection_amd.metrics import MeanAveragePrecision
    return MeanAveragePrecision(iou_type="bbox", class_metrics=True, n_classes=n_classes).to("cuda")


def _dicts(images):
    preds = [{"boxes": torch.from_numpy(im["det_boxes"]).cuda(), "scores": torch.from_numpy(im["det_scores"]).cuda(), "labels": torch.from_numpy(im["det_labels"]).cuda()} for im in images]
    targets = [{"boxes": torch.from_numpy(im["gt_boxes"]).cuda(), "labels": torch.from_numpy(im["gt_labels"]).cuda()} for im in images]
    return preds, targets


def _decode(mask):
    """[N,4] words -> matched [N,4,10], ignored [N,4,10]"""
    bits = (mask[:, :, None] >> np.arange(20)[None, None, :]) & 1
    return bits[:, :, :10].astype(bool), bits[:, :, 10:].astype(bool)


def _check(images, n_classes, batches=None):
    """Feed `images` (in `batches` update calls) to the device metric and hold every stage to the restatement.  -> (device summary, restatement summary)"""
    m = _metric(n_classes)
    for chunk in (batches or [images]):
        m.update(*_dicts(chunk))
    # ---- records
    (score, label, rank, mask), npig, C = m.records()
    assert C == n_classes
    ref = [R.match_image(im, n_classes) for im in images]
    keep = [r[0] >= 0 for r in ref]
    assert np.array_equal(label.cpu().numpy(), np.concatenate([r[0][k] for r, k in zip(ref, keep)]))
    assert np.array_equal(rank.cpu().numpy(), np.concatenate([r[1][k] for r, k in zip(ref, keep)]))
    assert np.array_equal(score.cpu().numpy(), np.concatenate([im["det_scores"][k] for im, k in zip(images, keep)]))
    matched, ignored = _decode(mask.cpu().numpy())
    assert np.array_equal(matched, np.concatenate([r[2][k] for r, k in zip(ref, keep)]))
    assert np.array_equal(ignored, np.concatenate([r[3][k] for r, k in zip(ref, keep)]))
    assert np.array_equal(npig.cpu().numpy(), np.sum([r[4] for r in ref], axis=0))
    # ---- precision / recall
    precision, recall = m.evaluate()
    rp, rr = R.accumulate(images, n_classes)
    precision, recall = precision.cpu().numpy(), recall.cpu().numpy()
    assert precision.shape == rp.shape and recall.shape == rr.shape and precision.dtype == np.float64
    assert np.array_equal(recall, rr)
    assert np.array_equal(precision, rp)
    # ---- summaries
    out = m.compute()
    want = R.summarize(rp, rr)
    got = {k: (v.cpu().numpy() if v.dim() else float(v)) for k, v in out.items()}
    print({k: got[k] for k in SCALARS})
    for k in SCALARS:
        assert out[k].dtype == torch.float64 and abs(got[k] - want[k]) <= TOL, (k, got[k], want[k])
    for k in ("map_per_class", "mar_100_per_class"):
        assert got[k].shape == (n_classes,) and np.all(np.abs(got[k] - want[k]) <= TOL), (k, got[k], want[k])
        assert np.array_equal(got[k] == -1, want[k] == -1)
    assert np.array_equal(got["classes"], np.arange(n_classes))
    # compute() leaves the state intact
    again = m.compute()
    assert all(torch.equal(out[k], again[k]) for k in out)
    return got, want


def test_worked_case():
    images = [R.image([[10, 10, 50, 50], [0, 0, 5, 5], [60, 60, 79, 73]], [0.9, 0.8, 0.7], [0, 0, 0], [[10, 10, 50, 50], [60, 60, 80, 80]], [0, 0])]
    got, _ = _check(images, 2)
    worked = {"map": (3 * ((51 + 50 * 2 / 3) / 101) + 7 * 51 / 101) / 10, "map_50": (51 + 50 * 2 / 3) / 101, "map_75": 51 / 101, "map_small": 0.15, "map_medium": 1.0,
              "map_large": -1.0, "mar_1": 0.5, "mar_10": 0.65, "mar_100": 0.65, "mar_small": 0.3}
    for k, v in worked.items():
        assert abs(got[k] - v) <= TOL, (k, got[k], v)
    assert abs(got["map_per_class"][0] - worked["map"]) <= TOL and got["map_per_class"][1] == -1.0


@pytest.mark.parametrize("seed", [0, 1])
def test_random_eval_sets(seed):
    """40 images, 10 classes, 200 unsorted detections per image around 1-16 ground truths, image sizes 200-640: all size ranges occur."""
    images = R.random_eval_set(seed)
    got, _ = _check(images, 10)
    for k in ("map", "map_small", "map_medium", "map_large", "mar_100"):
        assert 0.02 < got[k] < 0.98, (k, got[k])


def test_exact_score_ties_within_and_across_images():
    images = R.random_eval_set(5, n_images=12, n_det=120, tie_scores=True)          # scores on a grid of 8 levels
    assert len(np.unique(np.concatenate([im["det_scores"] for im in images]))) <= 9
    _check(images, 10)


def test_duplicate_ground_truths_last_wins():
    gt = [[10, 10, 60, 60], [10, 10, 60, 60], [100, 100, 140, 150], [10, 10, 60, 60]]
    images = [R.image([[10, 10, 60, 60], [12, 10, 60, 60], [10, 10, 60, 58], [100, 100, 140, 150]], [0.9, 0.8, 0.7, 0.6], [0, 0, 0, 0], gt, [0, 0, 0, 0]),
              R.image([[0, 0, 200, 200], [0, 0, 200, 200]], [0.5, 0.5], [1, 1], [[0, 0, 200, 200], [0, 0, 200, 200]], [1, 1])]
    _check(images, 2)


def test_integer_boxes_with_iou_exactly_on_thresholds():
    gt = [[0, 0, 10, 10]]
    images = [R.image([[0, 0, 10, h]], [0.9 - 0.01 * h], [0], gt, [0]) for h in (5, 6, 7, 8, 9, 10)]          # IoU = h / 10
    images += [R.image([[0, 0, 20, 15], [0, 0, 20, 11], [0, 0, 20, 13], [0, 0, 20, 17], [0, 0, 20, 19]], [0.9, 0.8, 0.7, 0.6, 0.5], [0] * 5, [[0, 0, 20, 20]] * 2, [0, 0]),   # .75 .55 .65 .85 .95
               R.image([[0, 0, 100, 200], [0, 0, 150, 200]], [0.3, 0.4], [1, 1], [[0, 0, 200, 200]], [1])]
    _check(images, 2)


def test_more_than_100_detections_of_a_class_in_an_image():
    rng = np.random.RandomState(7)
    gt = np.array([[20, 20, 80, 90], [150, 40, 300, 260], [10, 200, 40, 230]], dtype=np.float32)
    det = gt[rng.randint(0, 3, size=260)] + rng.normal(0, 6, size=(260, 4)).astype(np.float32)
    det[:, 2:] = np.maximum(det[:, 2:], det[:, :2] + 1)
    lab = np.where(np.arange(260) < 180, 0, 1)                     # 180 of class 0: 80 of them are cut; class 1 keeps all 80
    rng.shuffle(lab)
    images = [R.image(det, rng.uniform(0.01, 1, 260), lab, gt, [0, 0, 1]), R.image(det[:40], rng.uniform(0.01, 1, 40), lab[:40], gt[:2], [0, 1])]
    m_ref = R.match_image(images[0], 2)
    assert (m_ref[0] == -1).sum() == 80
    _check(images, 2)


def test_images_without_detections_or_ground_truth_and_a_class_with_detections_only():
    base = R.random_eval_set(11, n_images=6, n_classes=3, n_det=30)
    images = [base[0], R.image(gt_boxes=base[1]["gt_boxes"], gt_labels=base[1]["gt_labels"]),                         # no detections
              R.image(base[2]["det_boxes"], base[2]["det_scores"], base[2]["det_labels"]),                             # no ground truth
              R.image(), base[3]]                                                                                        # nothing at all
    # class 3 appears among the detections only, class 4 nowhere
    images.append(R.image(np.concatenate([base[4]["det_boxes"], [[5, 5, 90, 90]]]), np.concatenate([base[4]["det_scores"], [0.99]]),
                          np.concatenate([base[4]["det_labels"], [3]]), base[4]["gt_boxes"], base[4]["gt_labels"]))
    got, _ = _check(images, 5)
    assert got["map_per_class"][3] == -1.0 and got["map_per_class"][4] == -1.0
    # an out-of-range label is no record
    m = _metric(3)
    m.update(*_dicts(images))
    (_, label, _, _), _, _ = m.records()
    assert int(label.max()) <= 2


def test_several_updates_equal_one_update_over_the_concatenation():
    images = R.random_eval_set(3, n_images=10, n_det=60)
    got_one, _ = _check(images, 10)
    got_many, _ = _check(images, 10, batches=[images[:3], images[3:4], images[4:]])
    for k in got_one:
        assert np.array_equal(got_one[k], got_many[k]), k


def test_inferred_class_count_and_reset():
    images = R.random_eval_set(4, n_images=5, n_classes=7, n_det=40)
    m = _metric(None)
    m.update(*_dicts(images[:2]))
    m.update(*_dicts(images[2:]))
    out = m.compute()
    n = 1 + max(int(max(im["det_labels"].max(), im["gt_labels"].max())) for im in images)
    want = R.evaluate(images, n)
    assert out["map_per_class"].shape == (n,)
    for k in SCALARS:
        assert abs(float(out[k]) - want[k]) <= TOL, k
    m.reset()
    m.update(*_dicts(images[:1]))
    assert abs(float(m.compute()["map"]) - R.evaluate(images[:1])["map"]) <= TOL          # nothing of the first four images is left
    m.reset()
    empty = m.compute()
    assert float(empty["map"]) == -1.0 and float(empty["mar_100"]) == -1.0


def _tiny_eval_batch(B=4):
    from owl_vit_object_detection_amd import synth
    from owl_vit_object_detection_amd.models import PostProcess, load_model
    model = load_model({str(i): i for i in range(4)}, "cuda", arch="tiny").eval()
    img = torch.from_numpy(synth.make_images(model.cfg, B, seed=3)).cuda()
    with torch.no_grad():
        pred_boxes, _, pred_sims, _ = model(img)
    pp = PostProcess(0.01, 0.6)
    boxes, classes, scores = pp(pred_boxes, pred_sims, top_k=200)
    labels, gts = synth.make_targets(model.cfg, B, seed=5, max_boxes=6)
    G = max(len(l) for l in labels)
    gt_boxes = torch.zeros(B, G, 4)
    gt_labels = torch.full((B, G), -1, dtype=torch.int64)
    for b in range(B):
        gt_boxes[b, :len(labels[b])] = torch.from_numpy(gts[b])
        gt_labels[b, :len(labels[b])] = torch.from_numpy(np.asarray(labels[b], dtype=np.int64))
    gt_counts = torch.tensor([len(l) for l in labels], dtype=torch.int32)
    width = torch.tensor([640.0, 480.0, 333.0, 500.0][:B])
    height = torch.tensor([480.0, 640.0, 500.0, 375.0][:B])
    return boxes, classes, scores, pp.last_counts, gt_boxes.cuda(), gt_labels.cuda(), gt_counts.cuda(), width.cuda(), height.cuda()


def test_update_batched_on_postprocess_output_equals_update_bitwise_and_does_not_synchronise():
    boxes, classes, scores, counts, gt_boxes, gt_labels, gt_counts, width, height = _tiny_eval_batch()
    B = boxes.shape[0]
    assert boxes.shape[1] == 200 and int(counts.max()) > 0
    mb = _metric(4)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        mb.update_batched(boxes, classes, scores, counts, gt_boxes, gt_labels, gt_counts, width=width, height=height)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    # the same data as torchmetrics-style lists of pixel boxes (the f32 multiply of ref src/util.py:94-97 done here by torch)
    sc = torch.stack([width, height, width, height], dim=1)[:, None, :]
    px, gpx = boxes * sc, gt_boxes * sc
    preds = [{"boxes": px[b, :int(counts[b])], "scores": scores[b, :int(counts[b])], "labels": classes[b, :int(counts[b])]} for b in range(B)]
    targets = [{"boxes": gpx[b, :int(gt_counts[b])], "labels": gt_labels[b, :int(gt_counts[b])]} for b in range(B)]
    mu = _metric(4)
    mu.update(preds, targets)
    rb, ru = mb.records(), mu.records()
    assert rb[0][0].numel() == int(counts.sum()) > 0
    for x, y in zip(rb[0], ru[0]):
        assert torch.equal(x, y)
    assert torch.equal(rb[1], ru[1])
    ob, ou = mb.compute(), mu.compute()
    for k in ob:
        assert torch.equal(ob[k], ou[k]), k
    # and both are the restatement's
    images = [R.image(p["boxes"].cpu().numpy(), p["scores"].cpu().numpy(), p["labels"].cpu().numpy(), t["boxes"].cpu().numpy(), t["labels"].cpu().numpy()) for p, t in zip(preds, targets)]
    want = R.evaluate(images, 4)
    for k in SCALARS:
        assert abs(float(ob[k]) - want[k]) <= TOL, (k, float(ob[k]), want[k])


def test_update_metrics_leaves_its_inputs_unchanged():
    from owl_vit_object_detection_amd.train_util import update_metrics
    boxes, classes, scores, counts, gt_boxes, gt_labels, gt_counts, width, height = _tiny_eval_batch()
    args = [boxes, classes, scores, gt_boxes.cpu(), gt_labels.cpu()]          # ground truth arrives from the loader on the host (ref main.py:107)
    keep = [a.clone() for a in args]
    metadata = {"width": width.cpu(), "height": height.cpu()}
    m = _metric(4)
    update_metrics(m, metadata, *args)
    for a, k in zip(args, keep):
        assert torch.equal(a, k) and a.device == k.device
    ref = _metric(4)
    ref.update_batched(boxes, classes, scores, counts, gt_boxes, gt_labels, gt_counts, width=width, height=height)
    om, orf = m.compute(), ref.compute()
    for k in om:
        assert torch.equal(om[k], orf[k]), k


def test_limits_are_refused_with_the_limit_named():
    from owl_vit_object_detection_amd import _lib
    m = _metric(2)
    z = torch.zeros
    with pytest.raises(_lib.OwlLibError, match="K <= 1024"):
        m.update_batched(z(1, 1025, 4).cuda(), z(1, 1025, dtype=torch.int64).cuda(), z(1, 1025).cuda(), None, z(1, 2, 4).cuda(), z(1, 2, dtype=torch.int64).cuda(), None)
    with pytest.raises(_lib.OwlLibError, match="G <= 256"):
        m.update_batched(z(1, 8, 4).cuda(), z(1, 8, dtype=torch.int64).cuda(), z(1, 8).cuda(), None, z(1, 257, 4).cuda(), z(1, 257, dtype=torch.int64).cuda(), None)
    # the largest supported sizes run
    rng = np.random.RandomState(2)
    det = rng.uniform(0, 300, size=(1024, 4)).astype(np.float32); det[:, 2:] = det[:, :2] + rng.uniform(5, 120, size=(1024, 2)).astype(np.float32)
    gt = rng.uniform(0, 300, size=(256, 4)).astype(np.float32); gt[:, 2:] = gt[:, :2] + rng.uniform(5, 120, size=(256, 2)).astype(np.float32)
    _check([R.image(det, rng.uniform(0.01, 1, 1024), rng.randint(0, 2, 1024), gt, rng.randint(0, 2, 256))], 2)
