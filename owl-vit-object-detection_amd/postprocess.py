"""Inference post-process with the reference's call surface (ref src/models.py:122-146), on device.

``PostProcess(confidence_threshold, iou_threshold)(all_pred_boxes, pred_classes)`` -> ``(pred_boxes [1,K,4],
classes [1,K] i64, scores [1,K])`` exactly as the reference for its batch size of 1 (results ordered by descending
score, as ``torchvision.ops.batched_nms`` returns them).  Additions are keyword-only:

* ``top_k``  -- the eval loop's ``torch.topk(scores, min(200, K))`` (ref main.py:114-117) folded in: because the
  kept list is already score-descending it is a prefix, so the scan stops after ``top_k`` kept boxes;
* batch > 1 -- returns padded ``[B, Kmax, ...]`` tensors (classes padded with -1, scores with 0) and leaves the
  per-image counts in ``self.last_counts`` (device i32) -- with ``top_k`` given there is NO host sync at all.

* ``nms_route`` (constructor) -- ``torchvision.ops.batched_nms`` has two routes and picks by tensor size and device
  (torchvision/ops/boxes.py): per class on the raw coordinates, or all classes at once on ``boxes + class * (max + 1)``.
  The default ``"torchvision_gpu"`` does what torchvision does for a tensor on a GPU -- where the reference's eval loop
  runs (main.py:30,105-111): the coordinate trick up to 20 000 box coordinates past the threshold, i.e. always for
  OWL-ViT's <= 3600 boxes; ``"torchvision_cpu"`` mirrors the CPU path (per class above 1000 boxes); ``"per_class"`` /
  ``"coordinate_offset"`` pin one.  The routes only differ where the f32 rounding of the shifted coordinates moves an
  IoU across the threshold.

All arithmetic runs in ``owl_postprocess`` (csrc/postprocess.hip): one sort launch, one pair-mask launch, one scan
launch.  No CPU fallback.

``SlicedPostProcess`` / ``detect_sliced`` (below) are the sliced-inference form for large images with small objects: ``PostProcess`` on every slice of
``DeviceImageProcessor.slices``, then ``owl_slice_merge`` (csrc/slice_merge.hip) maps the slices' candidates into their source image and merges them.
"""
import numpy as np
import torch

from . import ops


def unpad_boxes(boxes, sizes, to="pixels"):
    """Boxes predicted on a `DeviceImageProcessor(resize="owlv2")` input are normalised to the PADDED square of side S = max(h, w), the image at its top
    left.  boxes [B, n, 4] (xyxy) with `sizes` [B, 2] = the images' (height, width) -- a tensor or a list of pairs -- or boxes [n, 4] with one pair.
    to="pixels": HF's Owlv2 `_scale_boxes`, both axes times S -> pixel coordinates of the original image (`boxes * S`, the same multiply).
    to="normalized": x * S / w, y * S / h -> normalised to the image itself, the frame of the reference's targets (formed in float64, rounded once);
    the inverse of preprocess.pad_square_targets.  Torch ops on the boxes' device, no sync."""
    if to not in ("pixels", "normalized"):
        raise ValueError(f"unpad_boxes: to={to!r}: \"pixels\" or \"normalized\"")
    sizes = torch.as_tensor(sizes, device=boxes.device)
    h, w = sizes[..., 0], sizes[..., 1]
    s = torch.maximum(h, w)
    if to == "pixels":
        return boxes * torch.stack([s, s, s, s], dim=-1).unsqueeze(-2)
    h, w, s = h.double(), w.double(), s.double()
    fx, fy = s / w, s / h
    return (boxes.double() * torch.stack([fx, fy, fx, fy], dim=-1).unsqueeze(-2)).to(boxes.dtype)


def top_objects(pred_boxes, objectness_logits, k):
    """OWLv2's class-agnostic proposals, "the k best objects first": pred_boxes [B, P, 4], objectness_logits [B, P] (`detect(..., objectness=True)`) ->
    (boxes [B, k, 4], scores [B, k] = sigmoid(objectness_logits), patch [B, k] i64) in the order of `torch.sort(scores, stable=True, descending=True)`:
    equal scores keep the lower patch index first.  It is `owl_postprocess` on a one-class score with a confidence threshold below every score and an IoU
    threshold nothing exceeds (no suppression): no new kernel, no host sync.  A NaN logit drops its patch, as torch.max's rule drops it everywhere in the
    post-process: the tail of that image is then padded (boxes 0, scores 0, patch -1).  1 <= k <= P."""
    if pred_boxes.dim() != 3 or pred_boxes.shape[-1] != 4 or objectness_logits.dim() != 2 or tuple(objectness_logits.shape) != tuple(pred_boxes.shape[:2]):
        raise ValueError(f"top_objects: expected pred_boxes [B, P, 4] and objectness_logits [B, P], got {tuple(pred_boxes.shape)} / {tuple(objectness_logits.shape)}")
    P = int(objectness_logits.shape[1])
    if not 1 <= int(k) <= P:
        raise ValueError(f"top_objects: 1 <= k <= {P} patches, got {k}")
    scores = torch.sigmoid(objectness_logits.detach().float())
    boxes, _, top, patch, _ = ops.postprocess(pred_boxes.detach().float().contiguous(), scores.unsqueeze(-1).contiguous(), int(k), -1.0, 1.0, "per_class")
    return boxes, top, patch


class PostProcess:
    def __init__(self, confidence_threshold=0.75, iou_threshold=0.3, *, nms_route="torchvision_gpu"):   # ref models.py:123-125 (same defaults)
        if nms_route not in ops.NMS_ROUTES:
            raise ValueError(f"PostProcess: nms_route must be one of {sorted(ops.NMS_ROUTES)}")
        self.confidence_threshold = confidence_threshold
        self.iou_threshold = iou_threshold
        self.nms_route = nms_route
        self.last_counts = None
        self.last_patch_idx = None

    def __call__(self, all_pred_boxes, pred_classes, *, top_k=None):
        if all_pred_boxes.dim() == 2:
            all_pred_boxes, pred_classes = all_pred_boxes[None], pred_classes[None]
        if all_pred_boxes.dim() != 3 or all_pred_boxes.shape[-1] != 4 or pred_classes.dim() != 3 \
                or pred_classes.shape[:2] != all_pred_boxes.shape[:2]:
            raise ValueError(f"PostProcess: expected boxes [B,P,4] and sims [B,P,C], got {tuple(all_pred_boxes.shape)} / {tuple(pred_classes.shape)}")
        B, P, C = pred_classes.shape
        max_out = int(top_k) if top_k is not None else P
        boxes, classes, scores, patch, counts = ops.postprocess(
            all_pred_boxes.detach().float().contiguous(), pred_classes.detach().float().contiguous(),
            max_out, float(self.confidence_threshold), float(self.iou_threshold), self.nms_route)
        self.last_counts, self.last_patch_idx = counts, patch
        if B == 1:                                  # the reference's contract: variable-length, one host read-back
            k = int(counts[0].item())
            self.last_patch_idx = patch[:, :k]
            return boxes[:, :k], classes[:, :k], scores[:, :k]
        if top_k is None:
            kmax = int(counts.max().item())
            self.last_patch_idx = patch[:, :kmax]
            return boxes[:, :kmax], classes[:, :kmax], scores[:, :kmax]
        return boxes, classes, scores


class SlicedPostProcess:
    """Post-process of sliced inference: ``PostProcess`` on every slice, then the merge of ``owl_slice_merge`` (csrc/slice_merge.hip) into one list per
    source image, both on the device.

    ``SlicedPostProcess(confidence_threshold, iou_threshold)(pred_boxes [T,P,4], pred_sims [T,P,C], plan)`` with ``plan`` the
    ``preprocess.SlicePlan`` the slices were cut by -> ``(boxes [G,Kmax,4] normalised xyxy in the FULL image, classes [G,Kmax] i64 (-1 pad),
    scores [G,Kmax] (0 pad))``, each list score-descending -- the form ``train_util.update_metrics`` takes.  ``last_counts`` (i32 [G]) and ``last_src``
    (i64: candidate index, ``src // per_slice_top_k`` = the slice within its image, ``src % per_slice_top_k`` = its rank there) stay on the device.
    With ``top_k`` given there is no host sync; without it one ``counts.max().item()``, as ``PostProcess`` does.

    * ``merge_metric`` -- ``"ios"`` (default): intersection over the smaller area, because an object cut by a slice border gives a partial box whose IoU
      with the whole box from the neighbouring slice is small; ``"iou"``: the per-slice NMS's own metric.  With ``"iou"``, ``merge_threshold =
      iou_threshold``, ``nms_route="per_class"`` and one whole-image slice the result is ``PostProcess``' bit for bit.
    * ``merge_threshold`` -- None: ``iou_threshold``.
    * ``class_agnostic_merge`` -- suppress across classes in the merge (the per-slice NMS stays class-aware).
    * ``per_slice_top_k`` -- candidates kept per slice; ``slices * per_slice_top_k <= 8192`` for every source image (the merge's sort is one workgroup).
    """

    def __init__(self, confidence_threshold=0.75, iou_threshold=0.3, *, merge_threshold=None, merge_metric="ios", class_agnostic_merge=False,
                 per_slice_top_k=200, nms_route="torchvision_gpu"):
        if nms_route not in ops.NMS_ROUTES:
            raise ValueError(f"SlicedPostProcess: nms_route must be one of {sorted(ops.NMS_ROUTES)}")
        if merge_metric not in ops.MERGE_METRICS:
            raise ValueError(f"SlicedPostProcess: merge_metric must be one of {sorted(ops.MERGE_METRICS)}, got {merge_metric!r}")
        if int(per_slice_top_k) < 1:
            raise ValueError(f"SlicedPostProcess: per_slice_top_k must be >= 1, got {per_slice_top_k}")
        self.confidence_threshold = confidence_threshold
        self.iou_threshold = iou_threshold
        self.merge_threshold = iou_threshold if merge_threshold is None else merge_threshold
        self.merge_metric = merge_metric
        self.class_agnostic_merge = bool(class_agnostic_merge)
        self.per_slice_top_k = int(per_slice_top_k)
        self.nms_route = nms_route
        self.last_counts = None
        self.last_src = None
        self._plan = None                          # (plan's arrays, device) -> their device copies: one upload per plan

    def _check(self, T, plan):
        offs = np.asarray(plan.slice_offsets)
        if len(plan.tiles) != T or plan.xform.shape != (T, 4) or int(offs[-1]) != T:
            raise ValueError(f"SlicedPostProcess: the plan holds {len(plan.tiles)} slices, the predictions {T}")
        per_group = np.diff(offs)
        K, lim = self.per_slice_top_k, ops.SLICE_MERGE_MAX
        for g in np.flatnonzero(per_group * K > lim).tolist():
            raise ValueError(f"SlicedPostProcess: source image {g} has {int(per_group[g])} slices x per_slice_top_k {K} = {int(per_group[g]) * K} candidates, "
                             f"above the merge's limit of {lim}: lower per_slice_top_k to at most {lim // int(per_group[g])} or cut fewer slices")
        return int(len(offs) - 1), int(per_group.max()) * K

    def __call__(self, pred_boxes, pred_sims, plan, *, top_k=None):
        if pred_boxes.dim() != 3 or pred_boxes.shape[-1] != 4 or pred_sims.dim() != 3 or pred_sims.shape[:2] != pred_boxes.shape[:2]:
            raise ValueError(f"SlicedPostProcess: expected boxes [T,P,4] and sims [T,P,C], got {tuple(pred_boxes.shape)} / {tuple(pred_sims.shape)}")
        T, P, _ = pred_sims.shape
        G, n_max = self._check(T, plan)
        dev = pred_boxes.device
        if self._plan is None or self._plan[0] is not plan or self._plan[1] != dev:
            self._plan = (plan, dev, torch.from_numpy(np.ascontiguousarray(plan.xform, dtype=np.float32)).to(dev, non_blocking=True),
                          torch.from_numpy(np.ascontiguousarray(plan.slice_offsets, dtype=np.int32)).to(dev, non_blocking=True))
        xform_d, offs_d = self._plan[2], self._plan[3]
        K = self.per_slice_top_k
        sb, sc, ss, _, scnt = ops.postprocess(pred_boxes.detach().float().contiguous(), pred_sims.detach().float().contiguous(), K,
                                              float(self.confidence_threshold), float(self.iou_threshold), self.nms_route)
        max_out = int(top_k) if top_k is not None else n_max
        boxes, classes, scores, src, counts = ops.slice_merge(sb, ss, sc, scnt, xform_d, offs_d, G, n_max, max_out, float(self.merge_threshold),
                                                              self.merge_metric, not self.class_agnostic_merge)
        self.last_counts, self.last_src = counts, src
        if top_k is None:
            kmax = int(counts.max().item())
            self.last_src = src[:, :kmax]
            return boxes[:, :kmax], classes[:, :kmax], scores[:, :kmax]
        return boxes, classes, scores


def detect_sliced(model, processor, images, post, *, batch=32, top_k=None, slice_size=None, overlap=0.2, full_image=True):
    """Sliced inference end to end: ``processor.slices(images)`` (the device resampler cuts and resizes the windows), the eval forward over the slices in
    chunks of ``batch`` (every image of a batch has the bits of its batch-1 run, so the chunking changes nothing), ``post`` (a ``SlicedPostProcess``)
    -> ``post``'s ``(boxes, classes, scores)`` plus the plan."""
    if int(batch) < 1:
        raise ValueError(f"detect_sliced: batch must be >= 1, got {batch}")
    pixel_values, plan = processor.slices(images, slice_size=slice_size, overlap=overlap, full_image=full_image)
    boxes, sims = [], []
    with torch.no_grad():
        for a in range(0, pixel_values.shape[0], int(batch)):
            pb, _, ps, _ = model(pixel_values[a:a + int(batch)])
            boxes.append(pb)
            sims.append(ps)
    out = post(torch.cat(boxes), torch.cat(sims), plan, top_k=top_k)
    return out + (plan,)
