"""Input-contract and eval-loop glue -- mirror of reference src/train_util.py (+ src/util.py:83-93,123-129).

`coco_to_model_input(boxes, metadata)`: absolute COCO `xywh` pixels -> `xyxy` normalised by the image
(width, height); same argument order and metadata keys ("width", "height") as the reference, batch-aware
(boxes [B,n,4], metadata values scalars or [B]).  Host-side elementwise glue on a few dozen numbers per
image (the reference runs it on the CPU before `.to(device)`, main.py:79) -- not a kernel.

`update_metrics(metric, metadata, pred_boxes, pred_classes, scores, boxes, labels, image_ids=None)` (ref src/train_util.py:37-64, called at main.py:120-128):
hands one post-processed batch to the mAP metric.  With `metrics.MeanAveragePrecision` the normalised boxes go to the device kernel as they are
(the scaling to pixels is the kernel's f32 multiply): no `.cpu()` / `.cuda()` hops, no host synchronisation, and the caller's tensors are not
scaled in place (the reference's are).  `reverse_labelmap` / `labels_to_classnames`: the labelmap helpers of ref src/train_util.py:26-34.
"""
import torch


def box_convert(boxes: torch.Tensor, in_fmt: str, out_fmt: str) -> torch.Tensor:
    """ref src/util.py:123-129 (torchvision.ops.box_convert semantics for xywh <-> xyxy)."""
    if in_fmt == out_fmt:
        return boxes.clone()
    if (in_fmt, out_fmt) == ("xywh", "xyxy"):
        x, y, w, h = boxes.unbind(-1)
        return torch.stack([x, y, x + w, y + h], dim=-1)
    if (in_fmt, out_fmt) == ("xyxy", "xywh"):
        x0, y0, x1, y1 = boxes.unbind(-1)
        return torch.stack([x0, y0, x1 - x0, y1 - y0], dim=-1)
    raise ValueError(f"unsupported conversion {in_fmt} -> {out_fmt}")


def scale_bounding_box(boxes: torch.Tensor, imwidth, imheight, mode: str) -> torch.Tensor:
    """ref src/util.py:83-93: mode "down" divides x by width and y by height, "up" multiplies."""
    assert mode in ("down", "up")
    shape = (-1,) + (1,) * (boxes.dim() - 1)          # per-image scalars broadcast over [n, coord]
    w = torch.as_tensor(imwidth, dtype=boxes.dtype, device=boxes.device).reshape(shape)
    h = torch.as_tensor(imheight, dtype=boxes.dtype, device=boxes.device).reshape(shape)
    out = boxes.clone()
    if mode == "down":
        out[..., 0::2] = out[..., 0::2] / w
        out[..., 1::2] = out[..., 1::2] / h
    else:
        out[..., 0::2] = out[..., 0::2] * w
        out[..., 1::2] = out[..., 1::2] * h
    return out


def coco_to_model_input(boxes: torch.Tensor, metadata) -> torch.Tensor:
    """absolute xywh -> relative xyxy (ref src/train_util.py:4-13)."""
    boxes = box_convert(boxes, "xywh", "xyxy")
    return scale_bounding_box(boxes, metadata["width"], metadata["height"], mode="down")


def model_output_to_image(boxes: torch.Tensor, metadata) -> torch.Tensor:
    """ref src/train_util.py:16-24: normalised xyxy -> pixels."""
    return scale_bounding_box(boxes, metadata["width"], metadata["height"], mode="up")


def reverse_labelmap(labelmap):
    """{category id: {"new_idx", "name"}} -> {new_idx: {"actual_category", "name"}} (ref src/train_util.py:26-30)."""
    out = {}
    for category, entry in labelmap.items():
        out[entry["new_idx"]] = {"actual_category": category, "name": entry["name"]}
    return out


def labels_to_classnames(labels, labelmap):
    """Class names of the FIRST image's labels, as a one-element batch (ref src/train_util.py:33-34; its batch size is 1).  -1 pads are dropped."""
    return [[labelmap[str(int(l))] for l in labels[0].tolist() if int(l) >= 0]]


def update_metrics(metric, metadata, pred_boxes, pred_classes, scores, boxes, labels, image_ids=None):
    """pred_boxes [B,K,4] / boxes [B,n,4]: normalised xyxy; pred_classes [B,K], labels [B,n] (-1 = padding); metadata["width"], ["height"]: number or [B];
    image_ids: None or [B] image keys for `metrics.MeanAveragePrecision` (see there; any other metric takes none)."""
    width, height = metadata["width"], metadata["height"]
    if hasattr(metric, "update_batched"):
        dev = pred_boxes.device
        metric.update_batched(pred_boxes, pred_classes, scores, None, boxes.to(dev, non_blocking=True), labels.to(dev, non_blocking=True), None,
                              width=width, height=height, image_ids=image_ids)
        return
    if image_ids is not None:
        raise ValueError("update_metrics: image_ids are for metrics.MeanAveragePrecision (this metric has no update_batched)")
    # any other metric with torchmetrics' interface: per-image dicts of pixel boxes, scaled out of place on the device the predictions are on
    dev = pred_boxes.device
    pred_px = scale_bounding_box(pred_boxes, width, height, mode="up")
    gt_px = scale_bounding_box(boxes.to(dev), width, height, mode="up")
    preds = [{"boxes": b[c >= 0], "scores": s[c >= 0], "labels": c[c >= 0]} for b, c, s in zip(pred_px, pred_classes, scores)]
    targets = [{"boxes": b[c >= 0], "labels": c[c >= 0]} for b, c in zip(gt_px, labels.to(dev))]
    metric.update(preds, targets)
