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
