"""COCO bbox mean average precision with the call surface the reference's eval loop uses (ref main.py:31,120-128,144-152:
``MeanAveragePrecision(iou_type="bbox", class_metrics=True)`` with ``.update / .compute / .reset``), resident on the device.

The contract is the pycocotools ``COCOeval`` bbox protocol (evaluateImg -> accumulate -> summarize) that torchmetrics delegates to: IoU thresholds
0.5:0.05:0.95, 101 recall thresholds, area ranges all / small (< 32^2) / medium / large (> 96^2), maxDets 1 / 10 / 100, no crowd annotations.
Neither library is a dependency; parity with torchmetrics itself is unpinned (it is not installed where this package is tested) and the
protocol is restated in ``tests/coco_eval_restatement.py``.

* ``update(preds, targets, image_ids=None)`` -- torchmetrics' lists of dicts (pixel xyxy ``boxes``, ``scores``, ``labels`` / ``boxes``, ``labels``).
* ``update_batched(boxes, labels, scores, counts, gt_boxes, gt_labels, gt_counts, width=None, height=None, image_ids=None)`` -- the padded batch that
  ``PostProcess(...)(..., top_k=200)`` returns (labels padded with -1, ``counts`` = ``PostProcess.last_counts``), ground truths padded the same way.
  With ``width`` / ``height`` the boxes are normalised and are scaled to pixels in the kernel (an f32 multiply, as ref src/util.py:94-97).
  One kernel launch (``owl_map_match``) on the current stream and NO host synchronisation, given ``n_classes`` and a metric that has been
  moved ``.to(device)`` (which uploads the protocol's constants) or updated before.
* ``compute()`` -- the only place that synchronises: concatenates the records, merges them over the ranks (below), checks the image keys,
  orders the records (``record_order``: stable ``torch.sort``s), one ``owl_map_accumulate`` launch, then the means.  State is left intact.
  Returns f64 tensors: ``map, map_50, map_75, map_small, map_medium, map_large, mar_1, mar_10, mar_100, mar_small, mar_medium, mar_large,
  map_per_class, mar_100_per_class, classes`` (-1 = nothing to average).

``n_classes=None`` infers ``max label + 1``: each update then reads the largest label back (one sync per update).  State = a list of per-update
record tensors on the device.  No CPU fallback.

Image keys and the order of the records.  pycocotools walks a class's detections in image-id order, each image's list by descending score, and
mergesorts them by ``-score``: ties in score are broken by image, then by the position within the image.  Every record therefore carries an
int64 image key, and the records are ordered by (class asc, score desc, image key asc, rank-within-image asc), ``rank`` being what
``owl_map_match`` writes (at equal score it follows slot order).  ``image_ids`` ([B] tensor or list of non-negative integers) gives the keys;
a device tensor is taken without a host synchronisation.  Without it the key of the i-th image this metric has seen since ``reset()`` is
``i * world + rank``: with one shard the arrival index (bit for bit the order of a metric without keys), and under data parallel the global
index that ``ddp.eval_indices`` / ``ddp.EvalSampler`` (and ``DistributedSampler(shuffle=False)``) give that image.

Data parallel.  ``shard=(rank, world)`` pins the shard; otherwise it is read from ``torch.distributed`` at the first update after construction
or ``reset()`` ((0, 1) without a process group).  With ``sync_on_compute=True`` (the default) and an active process group (``process_group``, or
the default one) of more than one rank -- or a single rank forced with ``OWL_FORCE_DIST=1``, for testing -- ``compute()`` / ``evaluate()`` gather the state of all ranks and evaluate the merged state: the record
counts are exchanged, the records padded to the largest count, gathered and cut by count (``ddp.all_gather_ragged``), the ground-truth counts
summed, and with ``n_classes=None`` the class count is the largest over the ranks.  RCCL gathers device tensors; any other backend (gloo) is
staged through host memory.  The collectives are issued in the current stream's order, behind the updates.  EVERY rank must call ``compute()``,
as with torchmetrics, and every rank gets the same bits; the local state is left intact (a second ``compute()`` gives the same answer, further
updates are allowed).  A rank that saw no image still takes part and needs a device: move the metric ``.to(device)``, or it raises "nothing was
updated and no device was given".  ``merge_state(other)`` is the in-process form: it appends another metric's records, keys kept.
An image key that occurs twice in the evaluated state raises ``ValueError``: the same image counted twice is what a padding
``DistributedSampler`` produces, and the result would be silently wrong.
"""
import torch
import torch.distributed as dist

from . import ddp, ops


def record_order(score, label, key, rank):
    """-> the permutation that orders records by (label asc, score desc, image key asc, rank asc): stable sorts, least significant key first.
    Plain torch on whatever device the tensors are on (host tensors included)."""
    order = torch.sort(rank, stable=True).indices
    for k, descending in ((key, False), (score, True), (label, False)):
        order = order[torch.sort(k[order], descending=descending, stable=True).indices]
    return order


class MeanAveragePrecision:
    def __init__(self, iou_type="bbox", class_metrics=True, *, n_classes=None, sync_on_compute=True, process_group=None, shard=None):
        if isinstance(iou_type, (tuple, list)) and len(iou_type) == 1:
            iou_type = iou_type[0]
        if iou_type != "bbox":
            raise ValueError(f"MeanAveragePrecision: only iou_type='bbox' is supported (got {iou_type!r}); the reference's eval loop uses no other")
        if n_classes is not None and int(n_classes) <= 0:
            raise ValueError("MeanAveragePrecision: n_classes must be positive")
        self.iou_type = iou_type
        self.class_metrics = bool(class_metrics)
        self.n_classes = None if n_classes is None else int(n_classes)
        self.sync_on_compute = bool(sync_on_compute)
        self.process_group = process_group
        self._pinned_shard = None if shard is None else ddp._shard(*shard)
        self.device = None
        self._shard = self._pinned_shard      # (rank, world); None = read from torch.distributed at the next update
        self._seen = 0                        # images since the last reset(): the default image key is _seen * world + rank
        self._records = []          # per update: (score [n], label [n] i64, rank [n] i32, mask [n,4] i32, npig [C_update,4] i64, key [n] i64, image_keys [B] i64)

    # ---- state ------------------------------------------------------------------------------------------------------------------------------
    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("MeanAveragePrecision: state and kernels live on the GPU (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._records and device != self.device:
            self._records = [tuple(t.to(device) for t in rec) for rec in self._records]
        self.device = device
        ops.map_constants(device)
        return self

    def reset(self):
        self._records = []
        self._seen = 0
        self._shard = self._pinned_shard

    def merge_state(self, other):
        """Append the records, ground-truth counts and image keys of `other`, a MeanAveragePrecision on the same device (torchmetrics' name for the
        in-process merge).  Keys are kept as they are: give the metrics distinct shards (or explicit image_ids); a key held by both fails at compute()."""
        if not isinstance(other, MeanAveragePrecision):
            raise TypeError("MeanAveragePrecision.merge_state: expected another MeanAveragePrecision")
        if other._records:
            if self.device is None:
                self.to(other.device)
            elif other.device != self.device:
                raise ValueError(f"MeanAveragePrecision lives on {self.device}, the merged state is on {other.device}")
            self._records.extend(other._records)

    # ---- update -----------------------------------------------------------------------------------------------------------------------------
    def update_batched(self, boxes, labels, scores, counts, gt_boxes, gt_labels, gt_counts, width=None, height=None, image_ids=None):
        """boxes [B,K,4], labels [B,K] (-1 pad), scores [B,K], counts [B] or None (= every slot; -1 labels still mark padding), gt_boxes [B,G,4],
        gt_labels [B,G] (-1 pad), gt_counts [B] or None; width / height: None (pixel boxes) or per-image sizes (number or [B]) of normalised boxes;
        image_ids: None (the default keys) or [B] non-negative integers (tensor: no host synchronisation; list: one small blocking upload)."""
        if not boxes.is_cuda:
            raise ValueError("MeanAveragePrecision.update_batched: device tensors only (no CPU fallback)")
        dev = boxes.device
        if self.device is None:
            self.to(dev)
        elif dev != self.device:
            raise ValueError(f"MeanAveragePrecision lives on {self.device}, the update is on {dev}")
        if boxes.dim() != 3 or boxes.shape[-1] != 4 or gt_boxes.dim() != 3 or gt_boxes.shape[-1] != 4 or gt_boxes.shape[0] != boxes.shape[0]:
            raise ValueError(f"MeanAveragePrecision.update_batched: expected boxes [B,K,4] and gt_boxes [B,G,4], got {tuple(boxes.shape)} / {tuple(gt_boxes.shape)}")
        B, K, G = boxes.shape[0], boxes.shape[1], gt_boxes.shape[1]
        if B == 0:
            return
        if K == 0:      # the kernel takes at least one slot of each kind
            boxes, labels, scores, K = boxes.new_zeros(B, 1, 4), torch.full((B, 1), -1, dtype=torch.int64, device=dev), boxes.new_zeros(B, 1), 1
        if G == 0:
            gt_boxes, gt_labels, G = boxes.new_zeros(B, 1, 4), torch.full((B, 1), -1, dtype=torch.int64, device=dev), 1
        boxes = boxes.detach().to(device=dev, dtype=torch.float32).contiguous()
        scores = scores.detach().to(device=dev, dtype=torch.float32).reshape(B, K).contiguous()
        labels = labels.detach().to(device=dev, dtype=torch.int64, non_blocking=True).reshape(B, K).contiguous()
        gt_boxes = gt_boxes.detach().to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
        gt_labels = gt_labels.detach().to(device=dev, dtype=torch.int64, non_blocking=True).reshape(B, G).contiguous()
        counts = self._counts(counts, B, K, dev)
        gt_counts = self._counts(gt_counts, B, G, dev)
        if width is None and height is None:
            scale = torch.ones(B, 2, dtype=torch.float32, device=dev)
        elif width is None or height is None:
            raise ValueError("MeanAveragePrecision.update_batched: give both width and height, or neither")
        else:
            scale = torch.stack([self._per_image(width, B, dev), self._per_image(height, B, dev)], dim=1).contiguous()
        C = self.n_classes
        if C is None:   # the one read-back of the inferred-classes mode
            C = max(int(torch.maximum(labels.max(), gt_labels.max()).item()) + 1, 1)
        score, label, rank, mask, npig = ops.map_match(boxes, scores, labels, counts, gt_boxes, gt_labels, gt_counts, scale, C)
        keys = self._image_keys(image_ids, B, dev)
        self._records.append((score.reshape(-1), label.reshape(-1), rank.reshape(-1), mask.reshape(-1, ops.MAP_A), npig.sum(dim=0),
                              keys[:, None].expand(B, K).reshape(-1), keys))

    def _image_keys(self, image_ids, B, dev):
        """-> [B] i64 on the device.  The images are counted either way (give ids to all updates or to none: a default key may equal an explicit one)."""
        if self._shard is None:
            self._shard = ddp._shard(group=self.process_group)
        first, self._seen = self._seen, self._seen + B
        if image_ids is None:
            rank, world = self._shard
            return torch.arange(first, first + B, dtype=torch.int64, device=dev) * world + rank
        if torch.is_tensor(image_ids):
            if image_ids.is_floating_point() or image_ids.is_complex() or image_ids.dtype == torch.bool or image_ids.numel() != B:
                raise ValueError(f"MeanAveragePrecision: image_ids must be {B} integers, got {image_ids.dtype} {tuple(image_ids.shape)}")
            if not image_ids.is_cuda and image_ids.numel() and int(image_ids.min()) < 0:
                raise ValueError("MeanAveragePrecision: image_ids must be non-negative")
            return image_ids.detach().to(device=dev, dtype=torch.int64, non_blocking=True).reshape(B).contiguous()      # (device ids: checked in compute())
        ids = [int(i) for i in image_ids]
        if len(ids) != B or any(i < 0 for i in ids):
            raise ValueError(f"MeanAveragePrecision: image_ids must be {B} non-negative integers")
        return torch.tensor(ids, dtype=torch.int64).to(dev)

    @staticmethod
    def _counts(counts, B, n, dev):
        if counts is None:
            return torch.full((B,), n, dtype=torch.int32, device=dev)
        return counts.detach().to(device=dev, dtype=torch.int32, non_blocking=True).reshape(B).contiguous()

    @staticmethod
    def _per_image(v, B, dev):
        if torch.is_tensor(v):
            return v.detach().to(device=dev, dtype=torch.float32, non_blocking=True).reshape(-1).expand(B)
        return torch.full((B,), float(v), dtype=torch.float32, device=dev)

    def update(self, preds, targets, image_ids=None):
        """torchmetrics' form: one dict per image, pixel xyxy ``boxes`` [n,4], ``scores`` [n], ``labels`` [n] / ``boxes`` [g,4], ``labels`` [g]; detections in any order.
        image_ids: as in update_batched."""
        if len(preds) != len(targets):
            raise ValueError("MeanAveragePrecision.update: preds and targets must have one entry per image")
        if not preds:
            return
        dev = self.device if self.device is not None else next((p["boxes"].device for p in preds if p["boxes"].is_cuda), None)
        if dev is None:
            raise ValueError("MeanAveragePrecision.update: move the metric .to(device) or pass device tensors (no CPU fallback)")
        B = len(preds)
        nd = [int(p["scores"].shape[0]) for p in preds]
        ng = [int(t["labels"].shape[0]) for t in targets]
        K, G = max(max(nd), 1), max(max(ng), 1)
        boxes = torch.zeros(B, K, 4, dtype=torch.float32, device=dev)
        scores = torch.zeros(B, K, dtype=torch.float32, device=dev)
        labels = torch.full((B, K), -1, dtype=torch.int64, device=dev)
        gt_boxes = torch.zeros(B, G, 4, dtype=torch.float32, device=dev)
        gt_labels = torch.full((B, G), -1, dtype=torch.int64, device=dev)
        for b, (p, t) in enumerate(zip(preds, targets)):
            if p["boxes"].reshape(-1, 4).shape[0] != nd[b] or p["labels"].shape[0] != nd[b] or t["boxes"].reshape(-1, 4).shape[0] != ng[b]:
                raise ValueError(f"MeanAveragePrecision.update: image {b}: boxes / scores / labels disagree in length")
            if nd[b]:
                boxes[b, :nd[b]] = p["boxes"].detach().reshape(-1, 4).to(dev)
                scores[b, :nd[b]] = p["scores"].detach().to(dev)
                labels[b, :nd[b]] = p["labels"].detach().to(dev)
            if ng[b]:
                gt_boxes[b, :ng[b]] = t["boxes"].detach().reshape(-1, 4).to(dev)
                gt_labels[b, :ng[b]] = t["labels"].detach().to(dev)
        self.update_batched(boxes, labels, scores, torch.tensor(nd, dtype=torch.int32).to(dev), gt_boxes, gt_labels, torch.tensor(ng, dtype=torch.int32).to(dev),
                            image_ids=image_ids)

    # ---- compute ----------------------------------------------------------------------------------------------------------------------------
    def _state(self):
        """The local state, padding removed: (score [N] f32, label [N] i64, rank [N] i32, mask [N,4] i32, key [N] i64), npig [C,4] i64, C, image_keys [I] i64."""
        if self.device is None:
            raise ValueError("MeanAveragePrecision: nothing was updated and no device was given")
        dev = self.device
        C = self.n_classes if self.n_classes is not None else max([1] + [int(r[4].shape[0]) for r in self._records])
        npig = torch.zeros(C, ops.MAP_A, dtype=torch.int64, device=dev)
        for r in self._records:
            npig[:r[4].shape[0]] += r[4]
        if self._records:
            score, label, rank, mask, key = (torch.cat([r[i] for r in self._records]) for i in (0, 1, 2, 3, 5))
            keep = label >= 0
            score, label, rank, mask, key = score[keep], label[keep], rank[keep], mask[keep], key[keep]
            image_keys = torch.cat([r[6] for r in self._records])
        else:
            score = torch.zeros(0, dtype=torch.float32, device=dev); label = torch.zeros(0, dtype=torch.int64, device=dev)
            rank = torch.zeros(0, dtype=torch.int32, device=dev); mask = torch.zeros(0, ops.MAP_A, dtype=torch.int32, device=dev)
            key = torch.zeros(0, dtype=torch.int64, device=dev); image_keys = torch.zeros(0, dtype=torch.int64, device=dev)
        return (score, label, rank, mask, key), npig, C, image_keys

    def records(self):
        """The local records of all updates in arrival order, padding removed: (score [N] f32, label [N] i64, rank [N] i32, mask [N,4] i32), npig [C,4] i32, C."""
        rec, npig, C, _ = self._state()
        return rec[:4], npig.to(torch.int32), C

    def image_keys(self):
        """The image keys of the local state in arrival order, one per image (images without detections included): [I] i64 on the device."""
        return self._state()[3]

    def _syncs(self):
        return self.sync_on_compute and ddp._active(self.process_group)

    def _merged_state(self):
        """_state() of all ranks of the group, in rank order (every rank calls this; every rank gets the same tensors)."""
        rec, npig, C, image_keys = self._state()
        group, dev = self.process_group, self.device
        via = ddp.collective_device(dev, group)
        if self.n_classes is None:       # the class count first: it sizes npig
            c = torch.tensor([C], dtype=torch.int64).to(via)
            dist.all_reduce(c, op=dist.ReduceOp.MAX, group=group)
            C = int(c)
            npig = torch.cat([npig, npig.new_zeros(C - npig.shape[0], ops.MAP_A)])
        rec, _ = ddp.all_gather_ragged(rec, group)
        (image_keys,), _ = ddp.all_gather_ragged([image_keys], group)
        npig = npig.to(via)
        dist.all_reduce(npig, op=dist.ReduceOp.SUM, group=group)
        return tuple(rec), npig.to(dev), C, image_keys

    @staticmethod
    def _check_keys(image_keys):
        """One sort of the per-image keys (not of the records) and one read-back: no key twice, none negative."""
        if image_keys.numel() == 0:
            return
        k = torch.sort(image_keys).values
        if bool(((k[1:] == k[:-1]).any() | (k[0] < 0)).item()):
            k = k.cpu()
            if int(k[0]) < 0:
                raise ValueError(f"MeanAveragePrecision: image_ids must be non-negative (got {int(k[0])})")
            twice = torch.unique(k[1:][k[1:] == k[:-1]]).tolist()
            raise ValueError(f"MeanAveragePrecision: {len(twice)} image key(s) occur more than once in the evaluated state (first: {twice[:5]}): the same "
                             "image was counted twice -- a padding DistributedSampler does that (use ddp.EvalSampler), or two shards were given the same ids")

    def evaluate(self):
        """-> (precision [10,101,C,4,3] f64, recall [10,C,4,3] f64) on the device: pycocotools' `eval["precision"]` / `eval["recall"]`, of the
        merged state of all ranks when the metric synchronises (then every rank must call this)."""
        (score, label, rank, mask, key), npig, C, image_keys = self._merged_state() if self._syncs() else self._state()
        self._check_keys(image_keys)
        order = record_order(score, label, key, rank)                              # plumbing: the order in which accumulate walks a class
        seg = torch.searchsorted(label[order], torch.arange(C + 1, dtype=torch.int64, device=self.device))
        return ops.map_accumulate(rank[order].contiguous(), mask[order].contiguous(), seg.contiguous(), npig.to(torch.int32).contiguous(), C)

    @staticmethod
    def _mean(x, dims=None):
        """mean over the entries > -1 (all of x, or per index of the kept dimension), -1 where there are none"""
        valid = x > -1
        if dims is None:
            n, s = valid.sum(), torch.where(valid, x, torch.zeros_like(x)).sum()
        else:
            n, s = valid.sum(dim=dims), torch.where(valid, x, torch.zeros_like(x)).sum(dim=dims)
        return torch.where(n > 0, s / n.clamp(min=1).to(x.dtype), torch.full_like(s, -1.0))

    def compute(self):
        precision, recall = self.evaluate()
        C = precision.shape[2]
        m = self._mean
        out = {
            "map": m(precision[:, :, :, 0, 2]), "map_50": m(precision[0, :, :, 0, 2]), "map_75": m(precision[5, :, :, 0, 2]),
            "map_small": m(precision[:, :, :, 1, 2]), "map_medium": m(precision[:, :, :, 2, 2]), "map_large": m(precision[:, :, :, 3, 2]),
            "mar_1": m(recall[:, :, 0, 0]), "mar_10": m(recall[:, :, 0, 1]), "mar_100": m(recall[:, :, 0, 2]),
            "mar_small": m(recall[:, :, 1, 2]), "mar_medium": m(recall[:, :, 2, 2]), "mar_large": m(recall[:, :, 3, 2]),
        }
        if self.class_metrics:
            out["map_per_class"] = m(precision[:, :, :, 0, 2], dims=(0, 1))
            out["mar_100_per_class"] = m(recall[:, :, 0, 2], dims=(0,))
        else:
            out["map_per_class"] = torch.full((), -1.0, dtype=torch.float64, device=self.device)
            out["mar_100_per_class"] = torch.full((), -1.0, dtype=torch.float64, device=self.device)
        out["classes"] = torch.arange(C, dtype=torch.int32, device=self.device)
        return out
