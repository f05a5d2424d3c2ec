"""COCO bbox mAP, the parts that need no GPU: the numpy restatement of the protocol (tests/coco_eval_restatement.py) against the worked case and
closed forms, the C ABI of the two kernels (declared, exported, argument checks), and the Python surface's refusals.

Tolerance of the mean summaries: 1e-9 absolute = the rounding bound of an f64 mean over fewer than 10^6 values in [0, 1]
(n * 2^-53 < 1.2e-10 for n = 10^6)."""
import ctypes
import os
import re

import numpy as np
import pytest

from owl_vit_object_detection_amd import _lib
from tests import coco_eval_restatement as R

TOL = 1e-9


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def worked_case():
    return [R.image([[10, 10, 50, 50], [0, 0, 5, 5], [60, 60, 79, 73]], [0.9, 0.8, 0.7], [0, 0, 0], [[10, 10, 50, 50], [60, 60, 80, 80]], [0, 0])]


WORKED = {"map": (3 * ((51 + 50 * 2 / 3) / 101) + 7 * 51 / 101) / 10, "map_50": (51 + 50 * 2 / 3) / 101, "map_75": 51 / 101, "map_small": 0.15, "map_medium": 1.0,
          "map_large": -1.0, "mar_1": 0.5, "mar_10": 0.65, "mar_100": 0.65, "mar_small": 0.3}


def test_restatement_reproduces_the_worked_case():
    s = R.evaluate(worked_case(), n_classes=2)
    for k, v in WORKED.items():
        assert abs(s[k] - v) <= TOL, (k, s[k], v)
    assert abs(s["map"] - 0.60396039) < 1e-8 and abs(s["map_50"] - 0.83498349) < 1e-8
    assert abs(s["map_per_class"][0] - WORKED["map"]) <= TOL and s["map_per_class"][1] == -1.0
    assert s["mar_100_per_class"][1] == -1.0 and list(s["classes"]) == [0, 1]
    # inferred class count = max label + 1
    assert R.evaluate(worked_case())["map_per_class"].shape == (1,)


def _gt_set(seed, n_images=6, n_classes=3):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n_images):
        g = rng.randint(1, 7)
        side = rng.choice([12.0, 50.0, 150.0], size=(g, 1)) * rng.uniform(0.8, 1.2, size=(g, 2))      # small, medium and large boxes
        xy = rng.uniform(0, 300, size=(g, 2))
        out.append((np.concatenate([xy, xy + side], 1).astype(np.float32), rng.randint(0, n_classes, size=g)))
    return out


def test_restatement_perfect_detections_score_one():
    imgs = [R.image(gt, np.linspace(0.9, 0.5, len(gl)), gl, gt, gl) for gt, gl in _gt_set(1)]
    s = R.evaluate(imgs, n_classes=3)
    for k in ("map", "map_50", "map_75", "map_small", "map_medium", "map_large", "mar_100", "mar_small", "mar_medium", "mar_large"):
        assert abs(s[k] - 1.0) <= TOL, (k, s[k])           # tp / (tp + eps): one rounding below 1
    assert np.all(np.abs(s["map_per_class"] - 1.0) <= TOL) and np.all(s["mar_100_per_class"] == 1.0)
    assert 0.0 < s["mar_1"] <= 1.0                            # one detection per image and class cannot recall several ground truths


def test_restatement_no_detections_score_zero():
    imgs = [R.image(gt_boxes=gt, gt_labels=gl) for gt, gl in _gt_set(2)]
    s = R.evaluate(imgs, n_classes=3)
    for k in ("map", "map_50", "map_75", "map_small", "map_medium", "map_large", "mar_1", "mar_10", "mar_100", "mar_small", "mar_medium", "mar_large"):
        assert s[k] == 0.0, (k, s[k])
    assert np.all(s["map_per_class"] == 0.0)


def test_restatement_class_without_ground_truth_is_excluded():
    gts = _gt_set(3, n_classes=2)
    # class 2 has detections only; classes 0 / 1 are detected perfectly: the means ignore class 2 instead of averaging a zero in
    imgs = [R.image(np.concatenate([gt, [[5, 5, 60, 60]]]), np.concatenate([np.linspace(0.9, 0.5, len(gl)), [0.95]]), np.concatenate([gl, [2]]), gt, gl) for gt, gl in gts]
    s = R.evaluate(imgs, n_classes=4)
    assert abs(s["map"] - 1.0) <= TOL and abs(s["mar_100"] - 1.0) <= TOL
    assert s["map_per_class"][2] == -1.0 and s["map_per_class"][3] == -1.0 and s["mar_100_per_class"][2] == -1.0
    assert np.all(np.abs(s["map_per_class"][:2] - 1.0) <= TOL)


def test_restatement_random_set_is_not_degenerate():
    s = R.evaluate(R.random_eval_set(0), n_classes=10)
    for k in ("map", "map_50", "map_small", "map_medium", "map_large", "mar_1", "mar_100", "mar_small", "mar_medium", "mar_large"):
        assert 0.02 < s[k] < 0.98, (k, s[k])
    assert np.all(s["map_per_class"] > 0)


def test_header_declares_and_library_exports_the_map_kernels(built):
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("owl_map_match", "owl_map_accumulate"):
        assert name in protos, name
        assert hasattr(lib, name), name
        for ty, _ in protos[name][1]:
            assert ty in _lib._CTYPES, (name, ty)
    assert _lib.header_abi_version() >= 7 and built.owl_abi_version() == _lib.header_abi_version()


def _match_args(ptr, B=1, K=200, G=16, C=10):
    return [None] + [ptr] * 15 + [B, K, G, C]


def test_map_kernels_check_their_arguments_without_a_device(built):
    # the checks run before any HIP call: safe without a device (the dummy pointers are never dereferenced)
    with pytest.raises(_lib.OwlLibError, match="null pointer"):
        _lib.call("owl_map_match", *_match_args(None))
    with pytest.raises(_lib.OwlLibError, match=r"K <= 1024"):
        _lib.call("owl_map_match", *_match_args(64, K=1025))
    with pytest.raises(_lib.OwlLibError, match=r"G <= 256"):
        _lib.call("owl_map_match", *_match_args(64, G=257))
    assert "G=257" in _lib.last_error()
    with pytest.raises(_lib.OwlLibError, match="null pointer"):
        _lib.call("owl_map_accumulate", None, None, None, None, None, None, None, 2.0 ** -52, None, None, 5, 3)


def test_unsupported_iou_type_raises():
    from owl_vit_object_detection_amd.metrics import MeanAveragePrecision
    with pytest.raises(ValueError, match="bbox"):
        MeanAveragePrecision(iou_type="segm")
    with pytest.raises(ValueError):
        MeanAveragePrecision(iou_type=("bbox", "segm"))
    m = MeanAveragePrecision(iou_type="bbox", class_metrics=True, n_classes=10)
    assert m.n_classes == 10
    with pytest.raises(ValueError, match="no CPU fallback"):
        m.to("cpu")


def test_labelmap_helpers():
    import torch
    from owl_vit_object_detection_amd.train_util import labels_to_classnames, reverse_labelmap
    labelmap = {"17": {"new_idx": 0, "name": "cat"}, "18": {"new_idx": 1, "name": "dog"}}
    assert reverse_labelmap(labelmap) == {0: {"actual_category": "17", "name": "cat"}, 1: {"actual_category": "18", "name": "dog"}}
    assert labels_to_classnames(torch.tensor([[1, 0, 1, -1]]), {"0": "cat", "1": "dog"}) == [["dog", "cat", "dog"]]


def test_package_does_not_import_the_restatement():
    pkg = os.path.dirname(os.path.abspath(_lib.__file__))
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith(".py"):
            assert not re.search(r"^\s*(from|import)\s.*coco_eval_restatement", open(os.path.join(pkg, fn)).read(), flags=re.M), fn


# ---- the named edge cases of tests/coco_eval_restatement.py have power: every planted protocol mistake changes an output of one of them ----------
# The planted code is a copy of R.match_image / R.accumulate_records with one switch per mistake (the IoU of a pair is computed once, not once per
# area range and threshold: same value).  With no mistake planted it must reproduce the restatement bit for bit on every case.
MATCH_PLANTS = {
    "gt_edge_outside": "a ground truth with area exactly on a range edge is outside (<= / >=)",
    "det_edge_outside": "an unmatched detection with area exactly on a range edge is outside",
    "equal_iou_keeps_earlier": "equal IoU keeps the earlier ground truth",
    "no_break": "a non-ignored match may be traded for an ignored ground truth",
    "touching_overlaps": "iw == 0 / ih == 0 counts as overlap",
    "tie_reversed": "equal scores are ranked later slot first",
    "cut_after_concat": "the cut at 100 is applied per class after concatenating the images",
    "taken_shared": "`taken` is shared between the IoU thresholds",
    "fused_width": "box width / height from a fused multiply-subtract, fl(b*s - fl(a*s))",
    "padding_read": "the slots behind det_counts / gt_counts are read",
    "label_truncated": "labels are compared as 32-bit integers (2^40 becomes class 0)",
}
ACC_PLANTS = {
    "searchsorted_right": "searchsorted(rc, thr, side='right')",
    "rank_ge_maxdet_is_fp": "records with rank >= maxDet are counted as false positives",
    "envelope_in_blocks_of_64": "the precision envelope is taken within blocks of 64 records only",
}


def _planted_iou(d, g, plant):
    iw = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    ih = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if (iw < 0 or ih < 0) if plant == "touching_overlaps" else (iw <= 0 or ih <= 0):
        return 0.0
    i = iw * ih
    with np.errstate(invalid="ignore", divide="ignore"):
        return i / (d[2] * d[3] + g[2] * g[3] - i)


def _planted_match_image(img, n_classes, plant=None):
    A, T = R.A, R.T
    scores, dlab, glab = img["det_scores"], img["det_labels"], img["gt_labels"]
    if plant == "label_truncated":
        dlab, glab = dlab.astype(np.int32), glab.astype(np.int32)
    dbox, gbox = R._xywh64(img["det_boxes"]), R._xywh64(img["gt_boxes"])
    if plant == "fused_width" and "det_wh" in img:
        dbox[:, 2:], gbox[:, 2:] = img["det_wh"], img["gt_wh"]
    n = len(scores)
    label, rank = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int32)
    matched, ignored = np.zeros((n, A, T), dtype=bool), np.zeros((n, A, T), dtype=bool)
    npig = np.zeros((n_classes, A), dtype=np.int32)
    outside = (lambda x, lo, hi: bool(x <= lo or x >= hi)), (lambda x, lo, hi: bool(x < lo or x > hi))
    for c in range(n_classes):
        didx = np.nonzero(dlab == c)[0]
        if plant == "tie_reversed":
            didx = didx[::-1]
        didx = didx[np.argsort(-scores[didx].astype(np.float64), kind="stable")]
        if plant != "cut_after_concat":
            didx = didx[:int(R.MAX_DETS[-1])]
        gidx = np.nonzero(glab == c)[0]
        label[didx], rank[didx] = c, np.arange(len(didx))
        iou = np.array([[_planted_iou(dbox[d], gbox[g], plant) for g in gidx] for d in didx]).reshape(len(didx), len(gidx))
        for a in range(A):
            lo, hi = R.AREA_RNG[a]
            g_ig = np.array([outside[plant != "gt_edge_outside"](gbox[g, 2] * gbox[g, 3], lo, hi) for g in gidx], dtype=bool)
            order = np.argsort(g_ig, kind="stable")
            gs_ig = g_ig[order]
            npig[c, a] = int((~g_ig).sum())
            taken = np.zeros(len(order), dtype=bool)
            for t in range(T):
                if plant != "taken_shared":
                    taken = np.zeros(len(order), dtype=bool)
                for di, d in enumerate(didx):
                    best, m = min(R.IOU_THRS[t], 1 - 1e-10), -1
                    for p, g in enumerate(order):
                        if taken[p]:
                            continue
                        if m > -1 and not gs_ig[m] and gs_ig[p] and plant != "no_break":
                            break
                        if iou[di, g] < best or (plant == "equal_iou_keeps_earlier" and m > -1 and iou[di, g] == best):
                            continue
                        best, m = iou[di, g], p
                    if m > -1:
                        taken[m], matched[d, a, t], ignored[d, a, t] = True, True, gs_ig[m]
                    else:
                        ignored[d, a, t] = outside[plant != "det_edge_outside"](dbox[d, 2] * dbox[d, 3], lo, hi)
    return label, rank, matched, ignored, npig


def _planted_accumulate_records(label, rank, score, matched, ignored, npig_all, n_classes, plant=None):
    T, A = R.T, R.A
    score = np.asarray(score, dtype=np.float32).astype(np.float64)
    precision, recall = -np.ones((T, R.R, n_classes, A, R.M)), -np.ones((T, n_classes, A, R.M))
    for k in range(n_classes):
        for a in range(A):
            npig = int(npig_all[k, a])
            if npig == 0:
                continue
            for mi, md in enumerate(R.MAX_DETS):
                sel = np.nonzero((label == k) & ((rank < md) | (plant in ("rank_ge_maxdet_is_fp", "cut_after_concat"))))[0]
                sel = sel[np.argsort(-score[sel], kind="stable")]
                if plant == "cut_after_concat":
                    sel = sel[:md]
                for t in range(T):
                    mt, ig = matched[sel, a, t], ignored[sel, a, t]
                    if plant == "rank_ge_maxdet_is_fp":
                        mt, ig = mt & (rank[sel] < md), ig & (rank[sel] < md)
                    tp, fp = np.cumsum(mt & ~ig).astype(np.float64), np.cumsum(~mt & ~ig).astype(np.float64)
                    nd = len(tp)
                    rc = tp / npig
                    pr = (tp / (fp + tp + R.EPS)).tolist()
                    recall[t, k, a, mi] = rc[-1] if nd else 0.0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1] and not (plant == "envelope_in_blocks_of_64" and i % 64 == 0):
                            pr[i - 1] = pr[i]
                    inds = np.searchsorted(rc, R.REC_THRS, side="right" if plant == "searchsorted_right" else "left")
                    for r, pi in enumerate(inds):
                        precision[t, r, k, a, mi] = pr[pi] if pi < nd else 0.0
    return precision, recall


def _planted_outputs(case, plant=None):
    """every array the device tests compare, with `plant` in force"""
    if "images" not in case:
        return _planted_accumulate_records(case["label"], case["rank"], case["score"], case["matched"], case["ignored"], case["npig"], case["n_classes"], plant)
    images, C = case["images"], case["n_classes"]
    if plant == "fused_width" and case["batched"] is not None:
        images = R.batched_images(case["batched"], fused=True)
    if plant == "padding_read" and case["batched"] is not None:
        images = R.batched_images(dict(case["batched"], counts=None, gt_counts=None))
    recs = [_planted_match_image(im, C, plant) for im in images]
    cat = [np.concatenate([r[i] for r in recs]) for i in range(4)]
    npig = np.sum([r[4] for r in recs], axis=0)
    score = np.concatenate([im["det_scores"] for im in images])
    return tuple(cat) + (npig,) + _planted_accumulate_records(cat[0], cat[1], score, cat[2], cat[3], npig, C, plant)


def test_the_named_cases_hold_what_their_names_say():
    """guards of the builders (the restatement's view): the cut, the straddling tie, the edge areas in both ranges, npig == 0, the scale case on 0.5"""
    for n, rec in zip(R.DET_NS, (R.match_image(im, 2) for im in R.match_cases()["det_distinct"]["images"])):
        assert (rec[0] == 1).sum() == min(n, 100) and (rec[0] == 0).sum() == min(n + 7, 100)
    for im in R.match_cases()["det_straddle"]["images"]:
        label, rank = R.match_image(im, 2)[:2]
        last = np.nonzero((label == 1) & (rank == 99))[0][0]
        twins = np.nonzero((im["det_labels"] == 1) & (im["det_scores"] == im["det_scores"][last]))[0]
        assert len(twins) == 2 and (label[twins] == 1).sum() == 1
    _, _, matched, ignored, npig = R.match_image(R.match_cases()["area_edges"]["images"][1], 1)
    assert not matched.any()
    # rows 0, 3, 6, 9, 12 are 32x32, 96x96, 1024x1, 9216x1, 1x1024; each is followed by its neighbours one f32 step down and up
    assert not ignored[[0, 6, 12], 1].any() and not ignored[[0, 6, 12], 2].any() and not ignored[[3, 9], 2].any() and not ignored[[3, 9], 3].any()
    assert ignored[[1, 7, 13], 2].all() and ignored[[2, 8, 14], 1].all() and ignored[[4, 10], 3].all() and ignored[[5, 11], 2].all()
    npig = np.sum([R.match_image(im, 2)[4] for im in R.match_cases()["gt_all_or_none_ignored"]["images"]], axis=0)
    assert npig[1].tolist() == [66, 0, 66, 0]
    assert R.match_image(R.match_cases()["gt_256_own256"]["images"][0], 2)[4][1, 0] == 256
    for im in R.match_cases()["scale_unfused"]["images"]:
        matched = R.match_image(im, 2)[2]
        assert matched[0, 0].tolist() == [True] + [False] * 9 and matched[1, 0].tolist() == [True] + [False] * 9
    for im in R.batched_images(R.match_cases()["scale_unfused"]["batched"], fused=True):          # one rounding instead of two: both matches are lost
        assert not _planted_match_image(im, 2, "fused_width")[2][:2, 0, 0].any()


def test_accumulate_cases_hold_what_their_names_say():
    c = R.accumulate_cases()["acc_patterns"]
    sizes = np.bincount(c["label"], minlength=c["n_classes"]).tolist()
    assert sorted(set(sizes)) == sorted(set(R.ACC_NS) | {7}) and sizes[3] == 0 and sizes[2] > 0 and sizes[4] > 0 and c["npig"][3].min() > 0
    r = R.accumulate_cases()["acc_patterns_ranks"]["rank"]
    assert (r >= 100).any() and ((r >= 10) & (r < 100)).any() and ((r >= 1) & (r < 10)).any() and (r == 0).any()
    z = R.accumulate_cases()["acc_no_records_and_no_ground_truth"]
    assert (z["npig"] == 0).any() and (z["npig"][np.bincount(z["label"], minlength=z["n_classes"]) == 0] > 0).any()
    # recall values on and beside the recall thresholds: how many of j / npig (j = 1..npig) are an entry of REC_THRS exactly
    on = {n: int(sum((np.float64(j) / n) in set(R.REC_THRS.tolist()) for j in range(1, n + 1))) for n in R.ACC_NPIG}
    print("recall values that coincide with a threshold:", on)
    assert on[7] == 1 and on[101] == 1 and 0 < on[10] < 10 and 0 < on[20] < 20 and 0 < on[100] < 100
    assert R.accumulate_cases()["acc_recall_steps"]["npig"][:, 0].tolist() == list(R.ACC_NPIG)


def _differs(x, y):
    return any(a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(x, y))


def test_planted_copy_reproduces_the_restatement_on_every_named_case():
    for name, case in R.match_cases().items():
        got = _planted_outputs(case)
        recs = [R.match_image(im, case["n_classes"]) for im in case["images"]]
        want = tuple(np.concatenate([r[i] for r in recs]) for i in range(4)) + (np.sum([r[4] for r in recs], axis=0),) + R.accumulate(case["images"], case["n_classes"])
        assert not _differs(got, want), name
    for name, case in R.accumulate_cases().items():
        want = R.accumulate_records(case["label"], case["rank"], case["score"], case["matched"], case["ignored"], case["npig"], case["n_classes"])
        assert not _differs(_planted_outputs(case), want), name


def test_every_planted_mistake_is_killed_by_a_named_case():
    """Every mistake changes at least one compared array of at least one named case; a mistake of the matching stage must do so on a match case,
    where the device's records are compared (it is not enough that it would shift a curve of hand-built records)."""
    cases = dict(R.match_cases())
    cases.update(R.accumulate_cases())
    base = {name: _planted_outputs(case) for name, case in cases.items()}
    survivors = []
    for plant, what in list(MATCH_PLANTS.items()) + list(ACC_PLANTS.items()):
        names = [n for n, c in cases.items() if "images" in c or plant in ACC_PLANTS or plant == "cut_after_concat"]
        killers = [n for n in names if _differs(_planted_outputs(cases[n], plant), base[n])]
        print(f"{plant} ({what}): killed by {', '.join(killers) if killers else 'NOTHING'}")
        if not killers:
            survivors.append(plant)
    assert not survivors, survivors
