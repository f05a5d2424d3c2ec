"""Reference fixture for the open-vocabulary criterion: tests/golden/f17_open_vocab_loss.npz, recorded from live Hugging Face transformers.

transformers' DeformableDetrHungarianMatcher(class_cost 1, bbox_cost 5, giou_cost 2) and DeformableDetrImageLoss(focal_alpha 0.25, losses = labels, boxes)
in double on the inputs of tests/open_vocab_loss_reference.py::fixture_inputs -- three images of 36 patches with 1 / 3 / 5 targets, Q = 5, queries 3 and 4
of image 1 padded (-FLT_MAX: HF's term there is exactly 0) -- fed as HF wants them: pred_boxes and target boxes in centre form.  Stored, results only:
the inputs (f32 logits, corner boxes, mask, padded labels / corner targets / counts), the matcher's cost matrix per image, its indices, the three losses
and the autograd gradients of loss_ce + 5 loss_bbox + 2 loss_giou wrt the logits and wrt the CORNER boxes (through corners_to_center).

Run where transformers is installed:  python tests/golden/make_golden_open_vocab_loss.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import open_vocab_loss_reference as R  # noqa: E402

OUT = os.path.join(HERE, "f17_open_vocab_loss.npz")
WEIGHTS = (1.0, 5.0, 2.0)          # DeformableDetrConfig: loss_ce 1, bbox_loss_coefficient 5, giou_loss_coefficient 2


def hf_run(case, weights=WEIGHTS):
    """-> dict(cost per image [P, n], indices, losses [3], dlogits, dboxes) from live transformers in double."""
    from transformers import DeformableDetrConfig
    from transformers.loss.loss_deformable_detr import DeformableDetrHungarianMatcher, DeformableDetrImageLoss
    cfg = DeformableDetrConfig()
    assert (cfg.class_cost, cfg.bbox_cost, cfg.giou_cost, cfg.focal_alpha) == (1, 5, 2, 0.25)
    B, P, Q = case["logits"].shape
    logits = case["logits"].double().requires_grad_(True)
    corners = case["boxes"].double().requires_grad_(True)
    outputs = {"logits": logits, "pred_boxes": R.corners_to_center(corners)}
    targets = [{"class_labels": l, "boxes": R.corners_to_center(t.double())} for l, t in zip(case["labels"], case["tgt"])]
    matcher = DeformableDetrHungarianMatcher(class_cost=cfg.class_cost, bbox_cost=cfg.bbox_cost, giou_cost=cfg.giou_cost)
    crit = DeformableDetrImageLoss(matcher=matcher, num_classes=Q, focal_alpha=cfg.focal_alpha, losses=["labels", "boxes"])
    indices = matcher(outputs, targets)
    # the cost matrix itself: the matcher's own lines on the same tensors (it returns only the indices)
    import transformers.loss.loss_deformable_detr as M
    got = {}
    orig = M.linear_sum_assignment
    M.linear_sum_assignment = lambda c: (got.setdefault("c", []).append(c.detach().numpy().copy()), orig(c))[1]
    try:
        matcher(outputs, targets)
    finally:
        M.linear_sum_assignment = orig
    out = crit(outputs, targets)
    total = weights[0] * out["loss_ce"] + weights[1] * out["loss_bbox"] + weights[2] * out["loss_giou"]
    total.backward()
    return dict(cost=got["c"], indices=indices, losses=torch.stack([out["loss_ce"], out["loss_bbox"], out["loss_giou"]]).detach(),
                dlogits=logits.grad.detach(), dboxes=corners.grad.detach())


def main():
    case = R.fixture_inputs()
    hf = hf_run(case)
    B, P, Q = case["logits"].shape
    Nmax = max(case["counts"])
    labels = np.zeros((B, Nmax), np.int64)
    tgt = np.zeros((B, Nmax, 4), np.float32)
    pred_idx = np.zeros((B, Nmax), np.int64)
    tgt_idx = np.zeros((B, Nmax), np.int64)
    cost = np.zeros((B, P, Nmax), np.float64)
    for b, n in enumerate(case["counts"]):
        labels[b, :n], tgt[b, :n] = case["labels"][b].numpy(), case["tgt"][b].numpy()
        pred_idx[b, :n], tgt_idx[b, :n] = hf["indices"][b][0].numpy(), hf["indices"][b][1].numpy()
        cost[b, :, :n] = hf["cost"][b]
    np.savez_compressed(OUT, logits=case["logits"].numpy(), boxes=case["boxes"].numpy(), mask=case["mask"].numpy(), labels=labels, tgt=tgt,
                        counts=np.array(case["counts"], np.int32), cost=cost, pred_idx=pred_idx, tgt_idx=tgt_idx, losses=hf["losses"].numpy(),
                        dlogits=hf["dlogits"].numpy(), dboxes=hf["dboxes"].numpy(), weights=np.array(WEIGHTS))
    print(f"wrote {OUT}: losses {hf['losses'].tolist()}")


if __name__ == "__main__":
    main()
