"""PushPullLoss -- host-side mirror of reference src/losses.py.

Same constructor and call signature (`PushPullLoss(n_classes, scales)(pred_sims, labels, pred_boxes,
boxes) -> {"loss_ce","loss_bg","loss_bbox","loss_giou"}`, ref src/losses.py:10,71-116).  The whole
criterion (matcher, box losses, sequential label spreading, focal-modulated BCE, and their gradients)
runs in HIP kernels with zero host syncs; batch > 1 means "mean over images of the reference's batch-1
loss" (the reference itself cannot run at batch > 1).
"""
import torch
import torch.nn as nn

from . import _lib, ops
from .autograd import mark_box_rows
from .matcher import HungarianMatcher, PackedTargets, box_iou, generalized_box_iou  # noqa: F401  (re-exported like the reference)
from .matcher import OpenVocabMatcher, _mask_u8, pack_open_vocab_targets


class _PushPullFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred_sims, pred_boxes, crit, tg):
        B, P, C = pred_sims.shape
        dev = pred_sims.device
        sims = pred_sims.detach().contiguous().float()
        boxes = pred_boxes.detach().contiguous().float()
        tc, pred_idx, tgt_idx, _ = crit.matcher.match_packed(sims, boxes, tg)
        s = ops.stream()
        _lib.call("owl_spread_labels", s, boxes, tc, B, P, crit.background_label, 0.85)
        need = pred_sims.requires_grad or pred_boxes.requires_grad
        per_image = torch.empty(B, 4, device=dev)
        losses = torch.empty(4, device=dev)
        dsims = torch.empty(B, P, C, device=dev) if need else None
        dl1 = torch.empty(B, P, 4, device=dev) if need else None
        dgiou = torch.empty(B, P, 4, device=dev) if need else None
        _lib.call("owl_push_pull_loss", s, sims, boxes, tc, crit.scales, tg.boxes, pred_idx, tgt_idx, tg.counts, per_image,
                  losses, dsims, dl1, dgiou, B, P, C, tg.Nmax, crit.background_label)
        ctx.saved = (tc, dsims, dl1, dgiou, B, P, C, crit.background_label)
        ctx.box_rows_cap = B * tg.Nmax          # the box losses read the matched predictions only: no other row of d(pred_boxes) can be non-zero
        crit.last = dict(target_classes=tc, pred_idx=pred_idx, tgt_idx=tgt_idx, per_image=per_image, sizes=tg.sizes)
        # four scalar outputs (not one 4-vector indexed afterwards: each index would cost a zero-fill + a copy in its backward)
        return losses[0], losses[1], losses[2], losses[3]

    @staticmethod
    def backward(ctx, g0, g1, g2, g3):
        tc, dsims, dl1, dgiou, B, P, C, bg = ctx.saved
        dev = tc.device
        g = torch.stack([g0, g1, g2, g3]).to(device=dev, dtype=torch.float32)
        out_sims = torch.empty(B, P, C, device=dev)
        out_boxes = torch.empty(B, P, 4, device=dev)
        _lib.call("owl_push_pull_loss_bwd", ops.stream(), g, tc, dsims, dl1, dgiou, out_sims, out_boxes, B, P, C, bg)
        return out_sims, mark_box_rows(out_boxes, ctx.box_rows_cap), None, None


class PushPullLoss(nn.Module):
    def __init__(self, n_classes, scales):
        super().__init__()
        self.matcher = HungarianMatcher(n_classes)
        self.scales = None if scales is None else torch.as_tensor(scales, dtype=torch.float32)
        self.background_label = n_classes
        self.last = None

    def pack(self, target_classes, target_boxes, device):
        if isinstance(target_classes, PackedTargets):
            return target_classes
        labels = list(target_classes) if not torch.is_tensor(target_classes) else list(target_classes.unbind(0))
        boxes = list(target_boxes) if not torch.is_tensor(target_boxes) else list(target_boxes.unbind(0))
        return PackedTargets(labels, boxes, device, self.background_label)

    def forward(self, predicted_classes, target_classes, predicted_boxes, target_boxes=None):
        dev = predicted_classes.device
        if self.scales is not None and self.scales.device != dev:
            self.scales = self.scales.to(dev)
        tg = self.pack(target_classes, target_boxes, dev)
        if len(tg.sizes) != predicted_classes.shape[0]:
            raise ValueError("batch size mismatch between predictions and targets")
        ce, bg, l1, giou = _PushPullFn.apply(predicted_classes, predicted_boxes, self, tg)
        return {"loss_ce": ce, "loss_bg": bg, "loss_bbox": l1, "loss_giou": giou}


class _OpenVocabFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, pred_boxes, crit, tg, mask_u8, nmasks, num_boxes):
        B, P, Q = logits.shape
        dev = logits.device
        lg = logits.detach().contiguous().float()
        boxes = pred_boxes.detach().contiguous().float()
        tc, pred_idx, tgt_idx, _ = crit.matcher.match_packed(lg, boxes, tg, mask_u8, nmasks)
        s = ops.stream()
        need = logits.requires_grad or pred_boxes.requires_grad
        nbytes = torch.zeros(1, dtype=torch.int64)
        _lib.call("owl_focal_loss_workspace_bytes", B, P, Q, nbytes)
        ws = torch.empty(int(nbytes.item()) // 8, dtype=torch.float64, device=dev)
        losses = torch.empty(3, device=dev)
        dl1 = torch.empty(B, P, 4, device=dev) if need else None
        dgiou = torch.empty(B, P, 4, device=dev) if need else None
        _lib.call("owl_focal_loss_fwd", s, lg, mask_u8, tc, ws, ws.numel() * 8, B, P, Q, nmasks, float(crit.alpha))
        _lib.call("owl_box_pair_loss", s, boxes, mask_u8, tg.labels, tg.boxes, pred_idx, tgt_idx, tg.counts, ws, ws.numel() * 8, dl1, dgiou, B, P, Q, nmasks, tg.Nmax)
        _lib.call("owl_open_vocab_loss_reduce", s, ws, ws.numel() * 8, losses, B, P, Q, float(num_boxes))
        # (the logits themselves are kept, not an unscaled gradient tensor: the backward recomputes the focal term from x and t)
        ctx.saved = (lg, mask_u8, nmasks, tc, dl1, dgiou, float(crit.alpha), float(num_boxes))
        ctx.box_rows_cap = B * tg.Nmax          # (as in _PushPullFn.forward)
        crit.last = dict(target_classes=tc, pred_idx=pred_idx, tgt_idx=tgt_idx, sizes=tg.sizes, num_boxes=float(num_boxes))
        # three scalar outputs, not one 3-vector indexed afterwards (see _PushPullFn.forward)
        return losses[0], losses[1], losses[2]

    @staticmethod
    def backward(ctx, g0, g1, g2):
        lg, mask_u8, nmasks, tc, dl1, dgiou, alpha, num_boxes = ctx.saved
        B, P, Q = lg.shape
        dev = lg.device
        g = torch.stack([g0, g1, g2]).to(device=dev, dtype=torch.float32)
        dlogits = torch.empty(B, P, Q, device=dev)
        dboxes = torch.empty(B, P, 4, device=dev)
        s = ops.stream()
        _lib.call("owl_focal_loss_bwd", s, g, lg, mask_u8, tc, dlogits, B, P, Q, nmasks, alpha, num_boxes)
        _lib.call("owl_box_pair_loss_bwd", s, g, dl1, dgiou, dboxes, B, P, num_boxes)
        return dlogits, mark_box_rows(dboxes, ctx.box_rows_cap), None, None, None, None, None


class OpenVocabLoss(nn.Module):
    """Criterion for the [B, P, Q] logits of `OwlViT.forward_queries` / `forward_text`: the DETR-family bipartite loss with sigmoid focal classification
    that transformers ships as DeformableDetrHungarianMatcher + DeformableDetrImageLoss(losses=["labels", "boxes"]) + sigmoid_focal_loss, evaluated on
    (logits, corners_to_center(pred_boxes)) -- matching, the three losses and their gradients in HIP kernels (csrc/open_vocab_loss.hip) with no host sync.

    `crit(logits, pred_boxes, targets, query_mask=None, num_boxes=None) -> {"loss_ce", "loss_bbox", "loss_giou"}`: three UNWEIGHTED scalars
    (HF weighs them 1 / bbox_loss_coefficient 5 / giou_loss_coefficient 2).  The cost defaults (class_cost 1, bbox_cost 5, giou_cost 2) and alpha 0.25 are
    DeformableDetrConfig's in transformers 5.15 (class_cost, bbox_cost, giou_cost, focal_alpha); the matcher's own alpha is HF's fixed 0.25.
    A negative `alpha` means no alpha weighting, as in HF.  gamma is 2; any other value raises.

    targets: a list of {"class_labels" | "labels", "boxes"} per image (a label indexes that image's own query list; images without targets are legal:
    pure negatives), or a PackedTargets.  pred_boxes are corners; target boxes are corners (`box_format="xyxy"`) or HF's centre form (`"cxcywh"`,
    converted once at packing).  `num_boxes` defaults to the batch's target count clamped at 1 (known on the host); a data-parallel caller passes the
    cross-rank mean as HF does.  `crit.last` holds the assignment of the last call, as PushPullLoss.last does."""

    def __init__(self, alpha=0.25, class_cost=1, bbox_cost=5, giou_cost=2, gamma=2, box_format="xyxy"):
        super().__init__()
        if gamma != 2:
            raise ValueError("OpenVocabLoss: gamma is 2 (the kernels square the modulating factor); other values are not built")
        if box_format not in ("xyxy", "cxcywh"):
            raise ValueError(f"box_format must be 'xyxy' or 'cxcywh', got {box_format!r}")
        self.matcher = OpenVocabMatcher(class_cost, bbox_cost, giou_cost)
        self.alpha = float(alpha)
        self.box_format = box_format
        self.last = None

    def forward(self, logits, pred_boxes, targets, query_mask=None, num_boxes=None):
        if logits.dim() != 3 or pred_boxes.shape != logits.shape[:2] + (4,):
            raise ValueError("logits must be [B, P, Q] and pred_boxes [B, P, 4]")
        B, P, Q = logits.shape
        tg = pack_open_vocab_targets(targets, logits.device, Q, query_mask, self.box_format)
        if len(tg.sizes) != B:
            raise ValueError("batch size mismatch between predictions and targets")
        if tg.Nmax > P:
            raise ValueError("more targets than predictions is not supported")
        mask_u8, nmasks = _mask_u8(query_mask, B, Q, logits.device)
        if num_boxes is None:
            num_boxes = max(1, sum(tg.sizes))
        if not float(num_boxes) > 0:
            raise ValueError("num_boxes must be positive")
        ce, l1, giou = _OpenVocabFn.apply(logits, pred_boxes, self, tg, mask_u8, nmasks, float(num_boxes))
        return {"loss_ce": ce, "loss_bbox": l1, "loss_giou": giou}
