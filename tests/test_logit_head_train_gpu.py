"""-m gpu: training HF's logit shift and scale -- `OwlViT.set_logit_head(head, trainable=True)`, autograd.OwlViTQueryFunction, owl_class_logits_bwd_head.

Yardstick for the four gradients: tests/test_open_vocab_train_gpu.py's recipe and band -- the same seeded cotangents into the HIP backward and into the
oracle under torch autograd with HF's head formula on the oracle's `feats` tap, the head's four tensors recording; REL_L2 = 2e-2, COS = 0.9995.  One
oracle backward per (config, batch) serves the three trainable sets.  Bitwise: everything else a step computes against the same step with the head
frozen; names and bits of state_dict / parameters / flat_param / forward_queries / a bank-path step; in line against the deferred tail over three steps;
detect after a step; logit_head_state -> set_logit_head."""
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
from tests.test_open_vocab_train_gpu import HEADS_ONLY, NQ, _focal, _head, _hf_logits, _queries  # noqa: E402
from tests.test_trainable_sets_gpu import COS, EVERYTHING, REL_L2, _grad_report  # noqa: E402

DEV = "cuda"
KEYS = weights.LOGIT_HEAD_KEYS
SHAPES = [("tiny", 3), ("tiny-l14", 5)]
_ref_cache = {}


def _reference(cname, B):
    """(Wnp, img, q, mask, d_boxes, d_logits, {key: oracle gradient of the head's tensor}), once per shape and left unchanged."""
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
    with torch.no_grad():
        ww = {n: torch.from_numpy(v) for n, v in Wnp.items()}
        taps = {}
        O.model_forward(cfg, ww, torch.from_numpy(img), taps)
    head = {k: v.clone().requires_grad_(True) for k, v in _head(cfg).items()}
    lg = _hf_logits(taps["feats"].view(B, cfg.patches, -1), ww["class_predictor.dense0.weight"], ww["class_predictor.dense0.bias"], q, mask, head)
    lg.backward(d_logits)
    out = (Wnp, img, q, mask, d_boxes, d_logits, {k: head[k].grad.detach().reshape(-1) for k in KEYS})
    _ref_cache[(cname, B)] = out
    return out


def _model(cname, Wnp=None, head_trainable=True, **kw):
    cfg = get_config(cname)
    model = OwlViT(cfg, weights.make_weights(cfg) if Wnp is None else Wnp, DEV, **kw)
    model.set_logit_head(_head(cfg), trainable=head_trainable)
    return cfg, model


def _step(cname, B, keep, head_trainable):
    Wnp, img, q, mask, d_boxes, d_logits, _ = _reference(cname, B)
    cfg, model = _model(cname, Wnp, head_trainable, **({} if keep is None else dict(trainable=keep)))
    qe = q.to(DEV).requires_grad_(True)
    pb, lg = model.forward_queries(torch.from_numpy(img).to(DEV), qe, mask)
    torch.autograd.backward([pb, lg], [d_boxes.to(DEV), d_logits.to(DEV)])
    torch.cuda.synchronize()
    return model, qe, pb.detach(), lg.detach()


@pytest.mark.parametrize("keep", [None, EVERYTHING, HEADS_ONLY], ids=["default", "everything", "heads_only"])
@pytest.mark.parametrize("cname,B", SHAPES)
def test_head_gradients_match_the_oracle_and_the_rest_keeps_its_bits(cname, B, keep):
    href = _reference(cname, B)[6]
    frozen, qe0, pb0, lg0 = _step(cname, B, keep, False)
    model, qe, pb, lg = _step(cname, B, keep, True)
    assert (keep == HEADS_ONLY) == (model.backward_floor == "heads")          # (the heads-only floor forms no d(feats): the head gradients still come)
    assert all(t.grad is None for t in frozen.logit_head.values()) and frozen.logit_head_parameters() == []
    leaves = model.logit_head_parameters()
    assert len(leaves) == 4 and all(t.grad is not None and t.grad.shape == t.shape for t in leaves)
    grads = {k: model.logit_head[k].grad.detach().float().cpu() for k in KEYS}
    worst, worst_cos = _grad_report(grads, href, f"logit head {cname} B={B} {'default' if keep is None else '+'.join(keep)}")
    assert worst < REL_L2 and worst_cos > COS, (worst, worst_cos)
    # everything else: the same step with the head frozen, bit for bit
    assert torch.equal(pb, pb0) and torch.equal(lg, lg0)
    assert torch.equal(model.flat_grad, frozen.flat_grad) and float(model.flat_grad.abs().max()) > 0
    assert torch.equal(qe.grad, qe0.grad)
    for (n, p), (n0, p0) in zip(model.named_parameters(), frozen.named_parameters()):
        assert n == n0 and (p.grad is None) == (p0.grad is None) and (p.grad is None or torch.equal(p.grad, p0.grad)), n


def test_only_the_head_trains():
    """Neither the query tensor nor (heads-only floor) anything below the heads asks for a gradient of its own: the head's still arrive."""
    cname, B = "tiny", 3
    href = _reference(cname, B)[6]
    Wnp, img, q, mask, d_boxes, d_logits, _ = _reference(cname, B)
    cfg, model = _model(cname, Wnp, True, trainable=("box",))
    assert model.backward_floor == "heads"
    pb, lg = model.forward_queries(torch.from_numpy(img).to(DEV), q.to(DEV), mask)
    torch.autograd.backward([pb, lg], [d_boxes.to(DEV), d_logits.to(DEV)])
    model.finish()
    grads = {k: model.logit_head[k].grad.detach().float().cpu() for k in KEYS}
    worst, worst_cos = _grad_report(grads, href, "logit head, box head only")
    assert worst < REL_L2 and worst_cos > COS, (worst, worst_cos)


def _bank_step(model, cfg, img, B):
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


@pytest.mark.parametrize("cname,B", SHAPES)
def test_a_trainable_head_changes_no_name_and_no_bit(cname, B):
    cfg, twin = _model(cname, head_trainable=False)
    cfg, model = _model(cname, head_trainable=True)
    assert [n for n, _ in model.named_parameters()] == [n for n, _ in twin.named_parameters()]
    assert len(list(model.parameters())) == len(list(twin.parameters()))
    ids = {id(p) for p in model.parameters()}
    assert not any(id(t) in ids for t in model.logit_head_parameters())
    sd, sd0 = model.state_dict(), twin.state_dict()
    assert list(sd) == list(sd0) and all(torch.equal(sd[k], sd0[k]) for k in sd) and not any("logit" in k for k in sd)
    assert list(model.flat_offsets.items()) == list(twin.flat_offsets.items()) and torch.equal(model.flat_param, twin.flat_param)
    assert model.flat_grad.shape == twin.flat_grad.shape
    img = torch.from_numpy(synth.make_images(cfg, B)).to(DEV)
    q, mask = _queries(cfg, B)
    with torch.no_grad():
        a, b = model.forward_queries(img, q, mask), twin.forward_queries(img, q, mask)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    pa, la = model.forward_queries(img, q, mask)
    pt, lt = twin.forward_queries(img, q, mask)
    assert la.requires_grad and torch.equal(pa.detach(), pt.detach()) and torch.equal(la.detach(), lt.detach())
    live = mask.to(DEV)[:, None, :].expand_as(la)
    for p_, l_ in ((pa, la), (pt, lt)):
        (torch.where(live, l_, torch.zeros_like(l_)).square().mean() + p_.mean()).backward()
    assert torch.equal(model.flat_grad, twin.flat_grad)
    model.zero_grad(); twin.zero_grad()
    g1, p1 = _bank_step(model, cfg, img, B)
    g0, p0 = _bank_step(twin, cfg, img, B)
    assert torch.equal(g0, g1) and torch.equal(p0, p1)


def _train(cname, B, overlap, steps=3):
    cfg, model = _model(cname)
    q, mask = _queries(cfg, B)
    qe = q.to(DEV).requires_grad_(True)
    live = mask.to(DEV)[:, None, :].expand(B, cfg.patches, NQ)
    g = torch.Generator().manual_seed(9)
    target = (torch.rand(B, cfg.patches, NQ, generator=g) < 0.1).float().to(DEV)
    imgs = [torch.randn(B, 3, cfg.image_size, cfg.image_size, generator=g).to(DEV) for _ in range(steps)]
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1, overlap=overlap)
    hopt = torch.optim.AdamW(model.logit_head_parameters() + [qe], lr=1e-2, weight_decay=0.0)          # the caller's optimizer: the head and a query tensor
    assert model.overlap_tail == overlap
    flat0 = model._logit_head_flat.clone()
    p0 = model.flat_param.clone()
    hist, fg, hg = [], [], []
    for s in range(steps):
        opt.zero_grad()
        hopt.zero_grad()
        pb, lg = model.forward_queries(imgs[s], qe, mask)
        loss = _focal(lg, target, live) + 0.1 * pb.square().mean()
        loss.backward()
        hist.append(loss.detach())
        hg.append(torch.cat([model.logit_head[k].grad.detach().reshape(-1) for k in KEYS] + [qe.grad.detach().reshape(-1)]).clone())
        model.finish()
        fg.append(model.flat_grad.clone())
        opt.step()
        hopt.step()
    model.finish()
    torch.cuda.synchronize()
    return dict(loss=torch.stack(hist).cpu(), fg=fg, hg=hg, p=model.flat_param.clone(), p0=p0, head=model._logit_head_flat.clone(), head0=flat0,
                q=qe.detach().clone(), model=model, img=imgs[-1], mask=mask)


@pytest.mark.parametrize("cname,B", SHAPES)
def test_three_steps_inline_is_bitwise_the_deferred_tail(cname, B):
    a, b = _train(cname, B, False), _train(cname, B, True)
    assert bool(torch.isfinite(a["loss"]).all()) and torch.equal(a["loss"], b["loss"])
    assert not torch.equal(a["p"], a["p0"]) and not torch.equal(a["head"], a["head0"])          # the parameters and the head move
    assert bool((a["head"] != a["head0"]).all())                                                   # ... every element of the four tensors
    for x, y in zip(a["fg"] + a["hg"], b["fg"] + b["hg"]):
        assert torch.equal(x, y) and float(x.abs().max()) > 0
    assert torch.equal(a["p"], b["p"]) and torch.equal(a["head"], b["head"]) and torch.equal(a["q"], b["q"])
    print(f"logit head {cname} B={B}: focal loss {a['loss'].tolist()}")
    # after the steps detect runs ops.class_logits on the UPDATED tensors: the leaves are the storage the optimizer stepped
    model, img, mask = a["model"], a["img"], a["mask"]
    cfg, D = model.cfg, model.cfg.hidden
    lh, flat = model.logit_head, model._logit_head_flat
    assert torch.equal(torch.cat([lh["logit_shift.weight"], lh["logit_scale.weight"], lh["logit_shift.bias"], lh["logit_scale.bias"]]).detach(), flat)
    boxes, logits = model.detect(img, a["q"], mask)
    ws = model._workspace(B, train=False)
    want = ops.class_logits(ws["e"], a["q"], ws["feats"], flat[:D], flat[2 * D:2 * D + 1], flat[D:2 * D], flat[2 * D + 1:], B, cfg.patches,
                            mask=mask.to(DEV).to(torch.uint8))[0]
    assert torch.equal(logits, want)
    h0 = a["head0"]
    stale = ops.class_logits(ws["e"], a["q"], ws["feats"], h0[:D], h0[2 * D:2 * D + 1], h0[D:2 * D], h0[2 * D + 1:], B, cfg.patches,
                             mask=mask.to(DEV).to(torch.uint8))[0]
    assert not torch.equal(stale, logits)          # (the head before the steps gives other logits)
    frozen0 = _model(cname, head_trainable=False)[1]
    # logit_head_state -> set_logit_head round-trips bitwise, into a frozen head as into a trainable one
    st = model.logit_head_state()
    assert list(st) == list(KEYS) and st["logit_shift.weight"].shape == (D,) and st["logit_shift.bias"].shape == ()
    for tr in (False, True):
        frozen0.set_logit_head(st, trainable=tr)
        assert all(torch.equal(frozen0.logit_head[k].detach(), lh[k].detach()) for k in KEYS)
        assert len(frozen0.logit_head_parameters()) == (4 if tr else 0)


def test_a_frozen_head_gives_an_optimizer_nothing():
    cfg, model = _model("tiny", head_trainable=False)
    assert model.logit_head_parameters() == []
    with pytest.raises(ValueError, match="empty parameter list"):
        torch.optim.AdamW(model.logit_head_parameters())
    model.set_logit_head(None)
    assert model.logit_head_parameters() == []
