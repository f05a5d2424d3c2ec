"""-m gpu: fine-tuning through HF's class head -- `OwlViT.forward_queries` (autograd.OwlViTQueryFunction, csrc/open_vocab_bwd.hip).

Yardstick for gradients: tests/test_trainable_sets_gpu.py's recipe and band -- the same seeded cotangents (0.1 randn for boxes and logits) into the HIP
backward and into the oracle under torch autograd, where dense0 and HF's head formula are applied to the oracle's `feats` tap in torch f32; every
trainable tensor and `query_embeds.grad` inside REL_L2 = 2e-2, COS = 0.9995.  One oracle backward per (config, batch) with every parameter recording
serves all trainable sets of that shape.  Bitwise: the forward against the bank path's boxes and ops.class_logits, in-line against the deferred tail,
a bank-path step after a forward_queries step against a twin model that never ran it, detect untouched."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import owl_oracle as O  # noqa: E402  (checker only)
from owl_vit_object_detection_amd import ops, synth, weights  # noqa: E402
from owl_vit_object_detection_amd.config import get_config  # noqa: E402
from owl_vit_object_detection_amd.losses import PushPullLoss  # noqa: E402
from owl_vit_object_detection_amd.models import OwlViT  # noqa: E402
from owl_vit_object_detection_amd.optim import FusedAdamW  # noqa: E402
from tests.test_trainable_sets_gpu import COS, EVERYTHING, REL_L2, _grad_report  # noqa: E402

DEV = "cuda"
HEADS_ONLY = ("class_predictor", "box")
NQ = 5
FMIN = torch.finfo(torch.float32).min
_ref_cache = {}


def _head(cfg):
    g = torch.Generator().manual_seed(21)
    D = cfg.hidden
    return {"logit_shift.weight": 0.3 / D ** 0.5 * torch.randn(D, generator=g), "logit_shift.bias": torch.tensor([0.05]),
            "logit_scale.weight": 1.0 / D ** 0.5 * torch.randn(D, generator=g), "logit_scale.bias": torch.tensor([0.1])}


def _queries(cfg, B):
    """Five queries per image, different per image; on image 1 (image 0 of a single-image batch) the last two are padded -- all zero -- and masked."""
    g = torch.Generator().manual_seed(22)
    q = torch.randn(B, NQ, cfg.text_dim, generator=g)
    q = q / q.norm(dim=-1, keepdim=True)
    mask = torch.ones(B, NQ, dtype=torch.bool)
    b = min(1, B - 1)
    q[b, 3:] = 0.0
    mask[b, 3:] = False
    return q, mask


def _hf_logits(feats, w0, b0, q, mask, head):
    """HF's OwlViTClassPredictionHead.forward in torch, on dense0's output."""
    F = torch.nn.functional
    e = F.linear(feats, w0, b0)
    eh = e / (torch.linalg.norm(e, dim=-1, keepdim=True) + 1e-6)
    qh = q / (torch.linalg.norm(q, dim=-1, keepdim=True) + 1e-6)
    cos = torch.einsum("bpd,bqd->bpq", eh, qh)
    shift = F.linear(feats, head["logit_shift.weight"][None], head["logit_shift.bias"])
    scale = F.elu(F.linear(feats, head["logit_scale.weight"][None], head["logit_scale.bias"])) + 1.0
    lg = (cos + shift) * scale
    return torch.where(mask[:, None, :], lg, torch.full_like(lg, FMIN))


def _reference(cname, B):
    """(Wnp, img, q, mask, d_boxes, d_logits, {name: oracle gradient}, oracle dq), once per shape and left unchanged."""
    if (cname, B) in _ref_cache:
        return _ref_cache[(cname, B)]
    cfg = get_config(cname)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    Wnp = weights.make_weights(cfg)
    img = synth.make_images(cfg, B)
    q, mask = _queries(cfg, B)
    g = torch.Generator().manual_seed(5)
    d_boxes = torch.randn(B, cfg.patches, 4, generator=g) * 0.1
    d_logits = torch.randn(B, cfg.patches, NQ, generator=g) * 0.1
    ww = {n: torch.from_numpy(v).clone().requires_grad_(True) for n, v in Wnp.items()}
    qq = q.clone().requires_grad_(True)
    taps = {}
    rb, _ = O.model_forward(cfg, ww, torch.from_numpy(img), taps)
    lg = _hf_logits(taps["feats"].view(B, cfg.patches, -1), ww["class_predictor.dense0.weight"], ww["class_predictor.dense0.bias"], qq, mask, _head(cfg))
    torch.autograd.backward([rb, lg], [d_boxes, d_logits])
    grads = {n: (ww[n].grad.detach() if ww[n].grad is not None else torch.zeros_like(ww[n])) for n in ww}
    out = (Wnp, img, q, mask, d_boxes, d_logits, grads, qq.grad.detach())
    _ref_cache[(cname, B)] = out
    return out


def _model(cname, Wnp=None, **kw):
    cfg = get_config(cname)
    model = OwlViT(cfg, weights.make_weights(cfg) if Wnp is None else Wnp, DEV, **kw)
    model.set_logit_head(_head(cfg))
    return cfg, model


@pytest.mark.parametrize("keep", [None, EVERYTHING, HEADS_ONLY], ids=["default", "everything", "heads_only"])
@pytest.mark.parametrize("cname,B", [("tiny", 3), ("tiny-l14", 5)])
def test_gradients_match_the_oracle(cname, B, keep):
    Wnp, img, q, mask, d_boxes, d_logits, gref, dq_ref = _reference(cname, B)
    cfg, model = _model(cname, Wnp, **({} if keep is None else dict(trainable=keep)))
    image = torch.from_numpy(img).to(DEV)
    qe = q.to(DEV).requires_grad_(True)
    pb, lg = model.forward_queries(image, qe, mask)
    # the forward: the bank path's boxes, ops.class_logits on the training workspace's e / feats, finfo.min where masked
    ws = model._workspace(B)
    lh = model.logit_head
    want = ops.class_logits(ws["e"], qe.detach(), ws["feats"], lh["logit_shift.weight"], lh["logit_shift.bias"], lh["logit_scale.weight"], lh["logit_scale.bias"],
                            B, cfg.patches, mask=mask.to(DEV).to(torch.uint8))[0]
    assert torch.equal(lg.detach(), want) and bool((lg.detach()[~mask.to(DEV)[:, None, :].expand_as(lg)] == FMIN).all())
    torch.autograd.backward([pb, lg], [d_boxes.to(DEV), d_logits.to(DEV)])
    torch.cuda.synchronize()
    with torch.no_grad():
        assert torch.equal(pb.detach(), model(image)[0])
    names = [n for n in weights.param_shapes(cfg) if weights.is_trainable(n, keep)] if keep is not None else list(model.flat_offsets)
    assert set(names) == set(model.flat_offsets)
    for n, p in model.named_parameters():
        assert (p.grad is not None) == (n in names), n          # frozen tensors get nothing
    if "queries" in names:
        assert float(model.p("queries").grad.abs().max()) == 0.0          # the learnable bank takes no part
    assert (keep == HEADS_ONLY) == (model.backward_floor == "heads")
    grads = {n: model.p(n).grad.detach().float().cpu() for n in names if n != "queries"}
    grads["query_embeds"] = qe.grad.detach().float().cpu()
    ref = {n: gref[n] for n in grads if n != "query_embeds"}
    ref["query_embeds"] = dq_ref
    worst, worst_cos = _grad_report(grads, ref, f"forward_queries {cname} B={B} {'default' if keep is None else '+'.join(keep)}")
    assert worst < REL_L2 and worst_cos > COS, (worst, worst_cos)
    assert bool((qe.grad[min(1, B - 1), 3:] == 0).all())          # padded and masked queries: exactly 0


def _focal(logits, target, live, alpha=0.25, gamma=2.0):
    """Sigmoid focal loss in torch ops over the live queries (masked logits are finfo.min: selected out, never multiplied)."""
    x = torch.where(live, logits, torch.zeros_like(logits))
    p = torch.sigmoid(x)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(x, target, reduction="none")
    pt = p * target + (1 - p) * (1 - target)
    w = alpha * target + (1 - alpha) * (1 - target)
    return torch.where(live, w * (1 - pt) ** gamma * ce, torch.zeros_like(ce)).sum() / live.sum()


def _train(cname, B, overlap, steps=3):
    cfg, model = _model(cname)
    q, mask = _queries(cfg, B)
    qe = q.to(DEV).requires_grad_(True)
    live = mask.to(DEV)[:, None, :].expand(B, cfg.patches, NQ)
    g = torch.Generator().manual_seed(9)
    target = (torch.rand(B, cfg.patches, NQ, generator=g) < 0.1).float().to(DEV)
    imgs = [torch.randn(B, 3, cfg.image_size, cfg.image_size, generator=g).to(DEV) for _ in range(steps)]
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1, overlap=overlap)
    qopt = torch.optim.SGD([qe], lr=0.5)          # a second optimizer steps the caller's query tensor: prompt tuning
    assert model.overlap_tail == overlap
    p0, q0 = model.flat_param.clone(), qe.detach().clone()
    hist, fg, qg = [], [], []
    for s in range(steps):
        opt.zero_grad()
        qopt.zero_grad()
        pb, lg = model.forward_queries(imgs[s], qe, mask)
        loss = _focal(lg, target, live) + 0.1 * pb.square().mean()
        loss.backward()
        hist.append(loss.detach())
        qg.append(qe.grad.detach().clone())
        model.finish()
        fg.append(model.flat_grad.clone())
        opt.step()
        qopt.step()
    model.finish()
    torch.cuda.synchronize()
    return dict(loss=torch.stack(hist).cpu(), fg=fg, qg=qg, p=model.flat_param.clone(), q=qe.detach().clone(), p0=p0, q0=q0)


@pytest.mark.parametrize("cname,B", [("tiny", 3), ("tiny-l14", 5)])
def test_three_steps_train_and_inline_is_bitwise_the_deferred_tail(cname, B):
    a, b = _train(cname, B, False), _train(cname, B, True)
    assert bool(torch.isfinite(a["loss"]).all()) and torch.equal(a["loss"], b["loss"])
    assert not torch.equal(a["p"], a["p0"]) and not torch.equal(a["q"], a["q0"])          # the parameters and the query tensor move
    for x, y in zip(a["fg"] + a["qg"], b["fg"] + b["qg"]):
        assert torch.equal(x, y) and float(x.abs().max()) > 0
    assert torch.equal(a["p"], b["p"]) and torch.equal(a["q"], b["q"])
    print(f"forward_queries {cname} B={B}: focal loss {a['loss'].tolist()}")


@pytest.mark.parametrize("cname,B", [("tiny", 3), ("tiny-l14", 5)])
def test_the_bank_path_and_detect_keep_their_bits(cname, B):
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

    cfg, twin = _model(cname)
    img = torch.from_numpy(synth.make_images(cfg, B)).to(DEV)
    g0, p0 = bank_step(twin, cfg, img)
    cfg, model = _model(cname)
    q, mask = _queries(cfg, B)
    det0 = model.detect(img, q, mask)
    qe = q.to(DEV).requires_grad_(True)
    pb, lg = model.forward_queries(img, qe, mask)
    live = mask.to(DEV)[:, None, :].expand_as(lg)
    (torch.where(live, lg, torch.zeros_like(lg)).square().mean() + pb.mean()).backward()
    assert float(model.flat_grad.abs().max()) > 0
    model.zero_grad()
    det1 = model.detect(img, q, mask)
    assert torch.equal(det0[0], det1[0]) and torch.equal(det0[1], det1[1])
    # under no_grad forward_queries is detect
    with torch.no_grad():
        nb, nl = model.forward_queries(img, q, mask)
    assert torch.equal(nb, det0[0]) and torch.equal(nl, det0[1])
    g1, p1 = bank_step(model, cfg, img)
    assert torch.equal(g0, g1) and torch.equal(p0, p1)


def test_forward_text_is_forward_queries_on_the_towers_embeddings():
    from owl_vit_object_detection_amd.config import get_text_config
    from owl_vit_object_detection_amd.text import TextTower
    cfg, model = _model("tiny")
    tc = get_text_config("tiny")
    tower = TextTower(tc, None, DEV)
    B = 2
    img = torch.from_numpy(synth.make_images(cfg, B)).to(DEV)
    g = torch.Generator().manual_seed(3)
    ids = torch.zeros(B, NQ, 16, dtype=torch.int64)          # BOS, three words, EOS, padding; image 1's last two prompts padded (all-zero ids)
    ids[..., 0], ids[..., 1:4], ids[..., 4] = tc.vocab - 2, torch.randint(1, min(1000, tc.vocab - 2), (B, NQ, 3), generator=g), tc.vocab - 1
    ids[1, 3:] = 0
    pb, lg = model.forward_text(img, ids, tower)
    assert lg.requires_grad and pb.requires_grad
    live = (ids[..., 0] > 0).to(DEV)[:, None, :].expand_as(lg)
    assert bool((lg.detach()[~live] == FMIN).all()) and bool(torch.isfinite(lg.detach()[live]).all())
    (torch.where(live, lg, torch.zeros_like(lg)).square().mean() + pb.mean()).backward()
    grad = model.flat_grad.clone()
    assert float(grad.abs().max()) > 0
    # the same call spelled out, HF's flat [B Q, S] layout included
    with torch.no_grad():
        emb = tower.encode(ids.reshape(B * NQ, 16)).reshape(B, NQ, -1)
    model.zero_grad()
    pb2, lg2 = model.forward_queries(img, emb, ids[..., 0] > 0)
    assert torch.equal(pb.detach(), pb2.detach()) and torch.equal(lg.detach(), lg2.detach())
    (torch.where(live, lg2, torch.zeros_like(lg2)).square().mean() + pb2.mean()).backward()
    assert torch.equal(grad, model.flat_grad)
    pb3, lg3 = model.forward_text(img, ids.reshape(B * NQ, 16), tower)
    assert torch.equal(lg3.detach(), lg.detach())
    torch.where(live, lg3, torch.zeros_like(lg3)).sum().backward()          # (consumes the recorded forward)


def test_errors():
    cfg, model = _model("tiny")
    B = 2
    img = torch.from_numpy(synth.make_images(cfg, B)).to(DEV)
    q, mask = _queries(cfg, B)
    pb1, lg1 = model.forward_queries(img, q, mask)
    pb2, lg2 = model.forward_queries(img, q, mask)
    with pytest.raises(RuntimeError, match="overwritten by a later gradient-recording forward"):
        torch.where(lg1 > -1e30, lg1, torch.zeros_like(lg1)).sum().backward()
    torch.where(lg2 > -1e30, lg2, torch.zeros_like(lg2)).sum().backward()          # the latest forward's backward runs
    model.set_logit_head(None)
    with pytest.raises(RuntimeError, match="forward_queries: no logit head.*set_logit_head"):
        model.forward_queries(img, q, mask)
