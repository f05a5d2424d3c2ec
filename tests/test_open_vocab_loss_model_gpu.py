"""-m gpu: `OwlViT.forward_queries` -> `losses.OpenVocabLoss` -> backward -> FusedAdamW on `tiny`, B = 3.

Gradients: every trainable tensor (and the caller's query tensor) against the same step driven by HF's formula in torch ops on the same logits and the
same assignment, inside the project's band (tests/test_trainable_sets_gpu.py: REL_L2 2e-2, COS 0.9995).  Bitwise: in line against the deferred tail over
three steps; a bank-path PushPullLoss step afterwards against a twin model that never ran the criterion.  An image without targets trains."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import synth  # noqa: E402
from owl_vit_object_detection_amd.losses import OpenVocabLoss, PushPullLoss  # noqa: E402
from owl_vit_object_detection_amd.optim import FusedAdamW  # noqa: E402
from tests import open_vocab_loss_reference as R  # noqa: E402
from tests.test_open_vocab_train_gpu import NQ, _model, _queries  # noqa: E402
from tests.test_trainable_sets_gpu import COS, REL_L2, _grad_report  # noqa: E402

DEV = "cuda"
B = 3
WEIGHTS = (1.0, 5.0, 2.0)          # HF's loss_ce / bbox_loss_coefficient / giou_loss_coefficient


def _targets(cfg, counts, seed=0):
    """Per image: `counts[b]` corner boxes inside the image, labels among the image's live queries (image 1's queries 3 and 4 are padded)."""
    g = torch.Generator().manual_seed(100 + seed)
    out = []
    for b, n in enumerate(counts):
        xy = torch.rand(n, 2, generator=g) * 0.6
        wh = 0.05 + torch.rand(n, 2, generator=g) * 0.3
        nlive = 3 if b == 1 else NQ
        out.append({"class_labels": torch.randint(0, nlive, (n,), generator=g), "boxes": torch.cat([xy, xy + wh], -1)})
    return out


def _total(out):
    return WEIGHTS[0] * out["loss_ce"] + WEIGHTS[1] * out["loss_bbox"] + WEIGHTS[2] * out["loss_giou"]


def _hf_in_torch_ops(lg, pb, mask, last, targets):
    """HF's sigmoid_focal_loss + loss_boxes in torch f32 ops on the device, at the assignment the criterion found."""
    F = torch.nn.functional
    Q = lg.shape[-1]
    live = mask.to(lg.device)[:, None, :].expand_as(lg)
    x = torch.where(live, lg, torch.zeros_like(lg))
    t = (last["target_classes"][..., None] == torch.arange(Q, device=lg.device)).float()
    p = torch.sigmoid(x)
    ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    p_t = p * t + (1 - p) * (1 - t)
    el = (0.25 * t + 0.75 * (1 - t)) * (ce * (1 - p_t) ** 2)
    nb = last["num_boxes"]
    src = torch.cat([pb[b, last["pred_idx"][b, :n]] for b, n in enumerate(last["sizes"])])
    tgt = torch.cat([targets[b]["boxes"].to(lg.device)[last["tgt_idx"][b, :n]] for b, n in enumerate(last["sizes"])])
    l1 = (R.corners_to_center(src) - R.corners_to_center(tgt)).abs().sum() / nb
    gi = (1 - R.giou(src, tgt)).sum() / nb
    return {"loss_ce": torch.where(live, el, torch.zeros_like(el)).sum() / nb, "loss_bbox": l1, "loss_giou": gi}


def test_gradients_match_hfs_formula_in_torch_ops():
    cfg, model = _model("tiny")
    _, twin = _model("tiny")
    q, mask = _queries(cfg, B)
    img = torch.from_numpy(synth.make_images(cfg, B)).to(DEV)
    targets = _targets(cfg, [3, 1, 4])
    crit = OpenVocabLoss()
    qa = q.to(DEV).requires_grad_(True)
    pb, lg = model.forward_queries(img, qa, mask)
    out = crit(lg, pb, targets, query_mask=mask)
    _total(out).backward()
    model.finish()
    qb = q.to(DEV).requires_grad_(True)
    pb2, lg2 = twin.forward_queries(img, qb, mask)
    assert torch.equal(lg.detach(), lg2.detach()) and torch.equal(pb.detach(), pb2.detach())
    ref = _hf_in_torch_ops(lg2, pb2, mask, crit.last, targets)
    _total(ref).backward()
    twin.finish()
    torch.cuda.synchronize()
    assert crit.last["sizes"] == [3, 1, 4] and crit.last["num_boxes"] == 8.0
    assert int((crit.last["target_classes"] != NQ).sum()) == 8
    for k in ref:
        assert abs(float(out[k].detach()) - float(ref[k].detach())) <= 1e-4 * abs(float(ref[k].detach())), k
    names = list(model.flat_offsets)
    grads = {n: model.p(n).grad.detach().float().cpu() for n in names if n != "queries"}
    want = {n: twin.p(n).grad.detach().float().cpu() for n in names if n != "queries"}
    grads["query_embeds"], want["query_embeds"] = qa.grad.detach().float().cpu(), qb.grad.detach().float().cpu()
    assert all(float(w.abs().max()) > 0 for n, w in want.items() if "class_predictor" in n or "box_head" in n or n == "query_embeds")
    worst, worst_cos = _grad_report(grads, want, "forward_queries + OpenVocabLoss tiny B=3")
    assert worst < REL_L2 and worst_cos > COS, (worst, worst_cos)
    assert bool((qa.grad[1, 3:] == 0).all())


def _train(overlap, counts, steps=3):
    cfg, model = _model("tiny")
    q, mask = _queries(cfg, B)
    qe = q.to(DEV).requires_grad_(True)
    g = torch.Generator().manual_seed(9)
    imgs = [torch.randn(B, 3, cfg.image_size, cfg.image_size, generator=g).to(DEV) for _ in range(steps)]
    crit = OpenVocabLoss()
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1, overlap=overlap)
    qopt = torch.optim.SGD([qe], lr=0.5)
    assert model.overlap_tail == overlap
    p0 = model.flat_param.clone()
    hist, fg = [], []
    for s in range(steps):
        opt.zero_grad()
        qopt.zero_grad()
        pb, lg = model.forward_queries(imgs[s], qe, mask)
        out = crit(lg, pb, _targets(cfg, counts, seed=s), query_mask=mask)
        _total(out).backward()
        hist.append(torch.stack([out[k].detach() for k in ("loss_ce", "loss_bbox", "loss_giou")]))
        model.finish()
        fg.append(model.flat_grad.clone())
        opt.step()
        qopt.step()
    model.finish()
    torch.cuda.synchronize()
    return dict(loss=torch.stack(hist).cpu(), fg=fg, p=model.flat_param.clone(), q=qe.detach().clone(), p0=p0)


def test_in_line_is_bitwise_the_deferred_tail_over_three_steps():
    a, b = _train(False, [3, 1, 4]), _train(True, [3, 1, 4])
    assert bool(torch.isfinite(a["loss"]).all()) and torch.equal(a["loss"], b["loss"])
    assert not torch.equal(a["p"], a["p0"])
    for x, y in zip(a["fg"], b["fg"]):
        assert torch.equal(x, y) and float(x.abs().max()) > 0
    assert torch.equal(a["p"], b["p"]) and torch.equal(a["q"], b["q"])
    print(f"forward_queries + OpenVocabLoss tiny B={B}: (loss_ce, loss_bbox, loss_giou) per step {a['loss'].tolist()}")


def test_an_image_without_targets_trains():
    a = _train(False, [2, 0, 1], steps=2)
    assert bool(torch.isfinite(a["loss"]).all()) and bool((a["loss"] > 0).all())
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in a["fg"])
    assert not torch.equal(a["p"], a["p0"])
    none = _train(False, [0, 0, 0], steps=1)          # a batch of pure negatives: num_boxes clamps at 1, the box losses are 0
    assert float(none["loss"][0, 0]) > 0 and float(none["loss"][0, 1]) == 0 and float(none["loss"][0, 2]) == 0
    assert bool(torch.isfinite(none["fg"][0]).all()) and float(none["fg"][0].abs().max()) > 0


def test_the_bank_path_keeps_its_bits_after_the_criterion():
    def bank_step(model, cfg, img):
        labels, boxes = synth.make_targets(cfg, B, max_boxes=5)
        crit = PushPullLoss(cfg.n_classes, None)
        opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1)
        opt.zero_grad()
        pb, _, ps, _ = model(img)
        l = crit(ps, [torch.from_numpy(x).to(DEV) for x in labels], pb, [torch.from_numpy(x).to(DEV) for x in boxes])
        (l["loss_ce"] + l["loss_bg"] + l["loss_bbox"] + l["loss_giou"]).backward()
        grad = model.flat_grad.clone()
        opt.step()
        torch.cuda.synchronize()
        return grad, model.flat_param.clone()

    cfg, twin = _model("tiny")
    img = torch.from_numpy(synth.make_images(cfg, B)).to(DEV)
    g0, p0 = bank_step(twin, cfg, img)
    cfg, model = _model("tiny")
    q, mask = _queries(cfg, B)
    pb, lg = model.forward_queries(img, q.to(DEV).requires_grad_(True), mask)
    out = OpenVocabLoss()(lg, pb, _targets(cfg, [3, 1, 4]), query_mask=mask)
    _total(out).backward()
    assert float(model.flat_grad.abs().max()) > 0
    model.zero_grad()
    g1, p1 = bank_step(model, cfg, img)
    assert torch.equal(g0, g1) and torch.equal(p0, p1)
