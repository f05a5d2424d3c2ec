"""Reference fixture for label sets beyond 10 classes: tests/golden/f11_tiny_c80.npz.

One train step of the REFERENCE (through make_golden's `build_reference_model` / `run_reference_step`, imported as a module and used as they are) on the
`tiny` config at n_classes = 80, batch 1: pred_boxes / pred_sims, the matcher's output, the labels after spreading, the four losses, `scales`, all 29
gradients in full, and the targets.  80 classes = 240 prompts = 8 query blocks of the wide class head; the targets must carry labels from at least three
different 10-class blocks.

Before anything is written the decisions are checked for margin on the reference's own outputs, with make_golden's `decision_margins` and `MARGIN_BARS`
(called as `_full_margins` calls them).  Seeds are walked upward from 1234 until one passes (model, image and targets all follow the seed, as in
make_golden's `_full`); if none up to 1234 + 200 does, the targets are constructed around the reference's predictions (`anchored_targets`).  The chosen
seed and the margins are stored in the file.

Run on the CPU box (needs the reference checkout and transformers, like make_golden.py):  python tests/golden/make_golden_labelsets.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (sets up the reference imports and the torchvision stub)
from owl_vit_object_detection_amd import synth  # noqa: E402
from owl_vit_object_detection_amd.config import get_config  # noqa: E402

N_CLASSES = 80
FIRST_SEED, SEED_SPAN = 1234, 200
TAG = "f11_tiny_c80"
MARGIN_KEYS = ("gap", "coord", "inter", "iou", "simpos")


def _passes(m, labels):
    return all(m[k] >= bar for k, bar in MG.MARGIN_BARS.items()) and len({int(l) // 10 for l in labels}) >= 3


def _step(cfg, seed, targets=None):
    """-> (out, grads, labels, boxes, margins) of one reference step at `seed`; targets drawn from synth.make_targets unless given."""
    model, _ = MG.build_reference_model(cfg, seed)
    img = synth.make_images(cfg, 1, seed)
    if targets is None:
        labels, boxes = synth.make_targets(cfg, 1, seed, max_boxes=6)
        labels, boxes = labels[0], boxes[0]
    else:
        labels, boxes = targets
    scales = synth.class_scales(cfg, [labels])
    out, grads = MG.run_reference_step(model, cfg, img, labels, boxes, scales)
    out["scales"] = scales
    m = MG.decision_margins(cfg, out["pred_boxes"][0], out["pred_sims"][0], labels, boxes)
    return out, grads, labels, boxes, m


def main():
    cfg = get_config("tiny", n_classes=N_CLASSES)
    chosen = None
    for seed in range(FIRST_SEED, FIRST_SEED + SEED_SPAN + 1):
        out, grads, labels, boxes, m = _step(cfg, seed)
        ok = _passes(m, labels)
        print(f"seed {seed}: labels {labels.tolist()} margins", {k: round(m[k], 5) for k in MARGIN_KEYS}, "PASS" if ok else "fail")
        if ok:
            chosen = seed
            break
    anchored = 0
    if chosen is None:
        # no seeded draw has margin: construct the targets around the reference's own predictions at the first seed (as many anchors as the 6 x 6 grid
        # gives at anchored_targets' spacing)
        chosen, anchored = FIRST_SEED, 1
        out, _, _, _, _ = _step(cfg, chosen)
        tl, tb, anchors = None, None, None
        for n in (3, 2, 1):
            try:
                tl, tb, anchors = MG.anchored_targets(cfg, out["pred_boxes"][0], out["pred_sims"][0], seed=77, n=n)
                break
            except AssertionError:
                continue
        assert tl is not None, "anchored_targets found no anchor"
        out, grads, labels, boxes, m = _step(cfg, chosen, targets=(tl, tb))
        assert sorted(m["pred_idx"].tolist()) == sorted(anchors.tolist()), "an anchor lost its own target"
    MG._check_margins(m, TAG)
    assert len({int(l) // 10 for l in labels}) >= 3, ("targets must carry labels from three different 10-class blocks", labels)
    assert np.array_equal(np.sort(m["pred_idx"]), np.sort(out["pred_idx"]))
    out["target_classes"] = MG.recover_spread_labels(cfg, out)
    out["tgt_labels"], out["tgt_boxes"] = labels, boxes
    out["seed"], out["anchored"], out["n_classes"] = np.int64(chosen), np.int64(anchored), np.int64(N_CLASSES)
    for k in MARGIN_KEYS:
        out["margin/" + k] = np.float64(m[k])
    out["pred_boxes"] = out["pred_boxes"].astype(np.float32)
    out.update(MG.grad_summary(grads, full=True))
    assert sum(k.startswith("grad/") for k in out) == 29
    path = os.path.join(HERE, f"{TAG}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, os.path.getsize(path)
    print(TAG, "seed", chosen, "anchored", anchored, {k: float(out[k]) for k in ("loss_ce", "loss_bg", "loss_bbox", "loss_giou")},
          "positives after spreading", int((out["target_classes"] != cfg.n_classes).sum()), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
