"""-m gpu: OWLv2's objectness head at model level on `tiny` -- detect_text(..., objectness=True) through the `owlv2.` names against fixture F20 (live HF,
tests/golden/make_golden_objectness.py), the bits that must not move when a head is set and the flag is not, training the six tensors
(autograd.OwlViTObjectnessFunction) against HF's autograd gradients, in-line against the deferred tail, a rectangular input, and postprocess.top_objects
against torch.sort.  The head's weights are rebuilt by F20's seed; the text tower and the trunk are the seeded sets HF was loaded with."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import synth, weights  # noqa: E402
from owl_vit_object_detection_amd.config import get_config, get_text_config  # noqa: E402
from owl_vit_object_detection_amd.losses import PushPullLoss  # noqa: E402
from owl_vit_object_detection_amd.models import load_model  # noqa: E402
from owl_vit_object_detection_amd.optim import FusedAdamW  # noqa: E402
from owl_vit_object_detection_amd.postprocess import top_objects  # noqa: E402
from owl_vit_object_detection_amd.text import TextTower  # noqa: E402
from tests import objectness_reference as R  # noqa: E402
from tests.golden.make_golden_objectness import B, IMG_SEED, KEYS, objectness_head  # noqa: E402
from tests.golden.make_golden_open_vocab import logit_head  # noqa: E402
from tests.golden.make_golden_owlv2 import v2_state_dict  # noqa: E402
from tests.test_trainable_sets_gpu import COS, REL_L2  # noqa: E402  (the project's end-to-end gradient band: 2e-2, 0.9995)

DEV = "cuda"
LABELMAP = {i: f"c{i}" for i in range(4)}


@pytest.fixture(scope="module")
def f20(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "f20_owlv2_objectness.npz")))
    cfg, tc = get_config("tiny"), get_text_config("tiny")
    sd = v2_state_dict(cfg, tc)
    sd.update({"class_head." + k: np.asarray(v, np.float32) for k, v in logit_head(cfg).items()})
    head = objectness_head(cfg, int(g["head_seed"]))
    for k in KEYS:
        sd["objectness_head." + k] = np.asarray(head[k], np.float32).reshape(sd["objectness_head." + k].shape)          # HF's [1, D] / [1] for dense2
    return dict(g=g, cfg=cfg, sd=sd, state=weights.from_hf_state_dict(sd, queries=weights.make_weights(cfg)["queries"]), tower=TextTower(tc, None, DEV),
                img=torch.from_numpy(synth.make_images(cfg, B, seed=IMG_SEED)).to(DEV), ids=torch.from_numpy(g["input_ids"]))


def _model(f, head="frozen", **kw):
    """head: None (no objectness head), "frozen" or "trainable"."""
    extra = {} if head is None else dict(objectness_head=weights.hf_objectness_head(f["sd"]), objectness_head_trainable=head == "trainable")
    return load_model(LABELMAP, DEV, arch="tiny", state=f["state"], logit_head=weights.hf_logit_head(f["sd"]), **extra, **kw)


def test_detect_text_against_hf(f20):
    g, model = f20["g"], _model(f20)
    boxes, logits, obj = model.detect_text(f20["img"], f20["ids"], f20["tower"], objectness=True)
    b0, l0 = model.detect_text(f20["img"], f20["ids"], f20["tower"])
    torch.cuda.synchronize()
    assert torch.equal(boxes, b0) and torch.equal(logits, l0)          # the flag adds an output and moves nothing
    assert obj.dtype == torch.float32 and tuple(obj.shape) == g["objectness_logits"].shape
    err = (obj.cpu().double() - torch.from_numpy(g["objectness_logits"]).double()).abs()
    ratio = err / torch.from_numpy(g["tol"]).double()
    print(f"objectness_logits against HF: max |d| {float(err.max()):.3e}, worst err / tol {float(ratio.max()):.3f} (tol {g['tol'].min():.3f} .. {g['tol'].max():.3f})")
    assert float(ratio.max()) <= 1.0
    assert torch.equal(obj.cpu().argmax(1), torch.from_numpy(g["objectness_logits"]).argmax(1))          # decided by the fixture's margin
    # the other entries agree with detect_text's
    with torch.no_grad():
        b1, l1, o1 = model.forward_text(f20["img"], f20["ids"], f20["tower"], objectness=True)
    emb = f20["tower"].encode(f20["ids"])
    b2, l2, s2, o2 = model.detect(f20["img"], emb, return_scores=True, objectness=True)
    assert torch.equal(o1, obj) and torch.equal(o2, obj) and torch.equal(b1, boxes) and torch.equal(l2, logits) and torch.equal(s2, torch.sigmoid(l2))
    model.set_objectness_head(None)
    with pytest.raises(RuntimeError, match="detect: no objectness head.*set_objectness_head"):
        model.detect_text(f20["img"], f20["ids"], f20["tower"], objectness=True)
    with pytest.raises(RuntimeError, match="forward_queries: no objectness head"):
        model.forward_queries(f20["img"], emb, objectness=True)
    assert model.objectness_head_parameters() == []


def _bank_steps(model, cfg, img, steps=3):
    labels, boxes = synth.make_targets(cfg, B, max_boxes=5)
    crit = PushPullLoss(cfg.n_classes, None)
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1)
    grads = []
    for _ in range(steps):
        opt.zero_grad()
        pb, _, ps, _ = model(img)
        l = crit(ps, [torch.from_numpy(x).to(DEV) for x in labels], pb, [torch.from_numpy(x).to(DEV) for x in boxes])
        (l["loss_ce"] + l["loss_bg"] + l["loss_bbox"] + l["loss_giou"]).backward()
        grads.append(model.flat_grad.clone())
        opt.step()
    torch.cuda.synchronize()
    return grads, model.flat_param.clone()


@pytest.mark.parametrize("kind", ["frozen", "trainable"])
def test_a_head_that_is_set_but_not_asked_for_moves_no_bit(f20, kind):
    cfg, img = f20["cfg"], f20["img"]
    emb = f20["tower"].encode(f20["ids"])
    twin, model = _model(f20, None), _model(f20, kind)
    assert list(twin.state_dict()) == list(model.state_dict()) and [n for n, _ in twin.named_parameters()] == [n for n, _ in model.named_parameters()]
    assert torch.equal(twin.flat_param, model.flat_param) and list(twin.flat_offsets.items()) == list(model.flat_offsets.items())
    assert len(model.objectness_head_parameters()) == (6 if kind == "trainable" else 0)
    outs = []
    for m in (twin, model):
        with torch.no_grad():
            bank = m(img)
        det = m.detect(img, emb)
        pb, lg = m.forward_queries(img, emb)
        (lg.square().mean() + pb.mean()).backward()
        fg = m.flat_grad.clone()
        m.zero_grad()
        outs.append((bank[0], bank[2], det[0], det[1], pb.detach(), lg.detach(), fg) + tuple(_bank_steps(m, cfg, img)[0]) + (m.flat_param.clone(),))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not torch.equal(model.flat_param, _model(f20, None).flat_param)          # (the three steps did move the parameters)


def _losses(model, f, target):
    pb, lg, obj = model.forward_text(f["img"], f["ids"], f["tower"], objectness=True)
    loss_main = lg.square().mean() + pb.mean()
    loss_obj = torch.nn.functional.binary_cross_entropy_with_logits(obj, target, reduction="sum") / B
    return loss_main, loss_obj, obj


def _head_grads(model, clear=True):
    out = [p.grad.detach().clone() for p in model.objectness_head_parameters()]
    if clear:
        for p in model.objectness_head_parameters():
            p.grad = None
    return out


def test_gradients_against_hf_and_independence_of_the_main_backward(f20):
    g, model = f20["g"], _model(f20, "trainable")
    target = torch.from_numpy(g["target"]).to(DEV)
    leaves = model.objectness_head_parameters()
    assert len(leaves) == 6 and all(p.is_leaf and p.requires_grad for p in leaves) and all(p.grad is None for p in leaves)
    # alone
    _, loss_obj, obj = _losses(model, f20, target)
    assert obj.grad_fn is not None and abs(float(loss_obj) - float(g["loss"])) < 0.05 * float(g["loss"])
    loss_obj.backward()
    assert float(model.flat_grad.abs().max()) == 0.0          # nothing of the head reaches the trunk's bucket
    alone = _head_grads(model)
    worst, worst_cos = 0.0, 1.0
    for k, got in zip(KEYS, alone):
        ref = torch.from_numpy(g["grad/" + k]).double().reshape(-1)
        x = got.cpu().double().reshape(-1)
        assert x.numel() == ref.numel(), k
        rel, cos = float((x - ref).norm() / ref.norm()), float((x * ref).sum() / (x.norm() * ref.norm()))
        print(f"objectness gradient {k}: rel-L2 {rel:.3e}, cosine {cos:.6f}")
        worst, worst_cos = max(worst, rel), min(worst_cos, cos)
    assert worst <= REL_L2 and worst_cos >= COS, (worst, worst_cos)
    # main alone, then the sum: flat_grad keeps its bits
    model.zero_grad()
    loss_main, _, _ = _losses(model, f20, target)
    loss_main.backward()
    fg_main = model.flat_grad.clone()
    assert float(fg_main.abs().max()) > 0 and all(p.grad is None for p in leaves)
    model.zero_grad()
    loss_main, loss_obj, _ = _losses(model, f20, target)
    (loss_main + loss_obj).backward()
    assert torch.equal(model.flat_grad, fg_main)
    both = _head_grads(model)
    # the objectness loss before / after the main loss
    model.zero_grad()
    loss_main, loss_obj, _ = _losses(model, f20, target)
    loss_obj.backward()
    loss_main.backward()
    before = _head_grads(model)
    assert torch.equal(model.flat_grad, fg_main)
    model.zero_grad()
    loss_main, loss_obj, _ = _losses(model, f20, target)
    loss_main.backward()
    loss_obj.backward()
    after = _head_grads(model)
    for a, b, c, d in zip(alone, both, before, after):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


def _train(f, overlap, steps=3):
    model = _model(f, "trainable")
    target = torch.from_numpy(f["g"]["target"]).to(DEV)
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1, overlap=overlap)
    hopt = torch.optim.AdamW(model.objectness_head_parameters(), lr=1e-2)
    assert model.overlap_tail == overlap
    gen = torch.Generator().manual_seed(9)
    imgs = [f["img"]] + [torch.randn(f["img"].shape, generator=gen).to(DEV) for _ in range(steps - 1)]
    hist, hg = [], []
    for s in range(steps):
        opt.zero_grad()
        hopt.zero_grad()
        pb, lg, obj = model.forward_text(imgs[s], f["ids"], f["tower"], objectness=True)
        loss = lg.square().mean() + pb.mean() + torch.nn.functional.binary_cross_entropy_with_logits(obj, target, reduction="sum") / B
        loss.backward()
        hist.append(loss.detach())
        hg.append(torch.cat([p.grad.reshape(-1) for p in model.objectness_head_parameters()]).clone())
        opt.step()
        hopt.step()
    model.finish()
    torch.cuda.synchronize()
    return dict(model=model, loss=torch.stack(hist).cpu(), hg=hg, p=model.flat_param.clone(), head=model.objectness_head_state())


def test_three_steps_inline_is_bitwise_the_deferred_tail_and_detect_follows_the_trained_head(f20):
    a, b = _train(f20, False), _train(f20, True)
    assert bool(torch.isfinite(a["loss"]).all()) and torch.equal(a["loss"], b["loss"]) and torch.equal(a["p"], b["p"])
    for x, y in zip(a["hg"], b["hg"]):
        assert torch.equal(x, y) and float(x.abs().max()) > 0
    start = weights.hf_objectness_head(f20["sd"])
    for k in KEYS:
        assert np.array_equal(a["head"][k], b["head"][k]) and not np.array_equal(a["head"][k].reshape(-1), start[k].reshape(-1)), k
    D = f20["cfg"].hidden          # HF's shapes: the six tensors go back into an Owlv2ForObjectDetection state dict as they are
    assert [a["head"][k].shape for k in KEYS] == [(D, D), (D,), (D, D), (D,), (1, D), (1,)] == [f20["sd"]["objectness_head." + k].shape for k in KEYS]
    print(f"objectness training, three steps: loss {a['loss'].tolist()}")
    # detect on the trained head: the float64 head on the updated buffer and the device's own feats, within the kernel-level bound
    model = a["model"]
    obj = model.detect_text(f20["img"], f20["ids"], f20["tower"], objectness=True)[2]
    P = model.cfg.patches
    feats = model._workspace(B, train=False)["feats"][:B * P].float().cpu()
    ref, tol = R.bounds_head(feats, a["head"])
    worst = R.check("detect on the trained head", obj.cpu().reshape(-1), ref["o"], tol)
    print(f"detect on the trained head: worst err / tol {worst:.3f}")
    # the state round trip is bitwise, frozen or trainable
    for trainable in (False, True):
        model.set_objectness_head(None)
        assert model.objectness_head is None
        back = model.set_objectness_head(a["head"], trainable=trainable).objectness_head_state()
        assert all(np.array_equal(back[k].reshape(-1).view(np.int32), a["head"][k].reshape(-1).view(np.int32)) for k in KEYS)
        assert len(model.objectness_head_parameters()) == (6 if trainable else 0)
        assert torch.equal(model.detect_text(f20["img"], f20["ids"], f20["tower"], objectness=True)[2], obj)


def test_stale_generation_frozen_head_and_bad_heads(f20):
    model = _model(f20, "trainable")
    emb = f20["tower"].encode(f20["ids"])
    _, _, o1 = model.forward_queries(f20["img"], emb, objectness=True)
    pb2, lg2, o2 = model.forward_queries(f20["img"], emb, objectness=True)
    with pytest.raises(RuntimeError, match="overwritten by a later gradient-recording forward"):
        o1.sum().backward()
    (o2.sum() + lg2.mean() + pb2.mean()).backward()          # the latest forward's backward runs
    assert all(p.grad is not None for p in model.objectness_head_parameters())
    # a trainable objectness head alone makes the forward a recording one: with every parameter frozen by hand the call is refused loudly (the trainable
    # set is chosen at construction), it does not fall through to `detect` and hand back logits that train nothing
    model.zero_grad()
    model.requires_grad_(False)
    with pytest.raises(RuntimeError, match="requires_grad=False"):
        model.forward_queries(f20["img"], emb, objectness=True)
    assert model.forward_queries(f20["img"], emb)[1].grad_fn is None          # (without the flag nothing asks for a gradient: `detect`)
    frozen = _model(f20, "frozen")
    assert frozen.objectness_head_parameters() == []
    pb, lg, obj = frozen.forward_queries(f20["img"], emb, objectness=True)
    assert obj.grad_fn is None and not obj.requires_grad and lg.requires_grad
    with torch.no_grad():
        assert torch.equal(obj, frozen.detect(f20["img"], emb, objectness=True)[2])          # the training workspace's feats carry the eval forward's bits here
    lg.mean().backward()
    head = dict(weights.hf_objectness_head(f20["sd"]))
    with pytest.raises(ValueError, match="`dense1.weight` must be"):
        frozen.set_objectness_head(dict(head, **{"dense1.weight": np.zeros((4, 4), np.float32)}))
    del head["dense0.bias"]
    with pytest.raises(KeyError, match="`dense0.bias` is missing"):
        frozen.set_objectness_head(head)


def test_rectangular_input(f20):
    """image_size = (96, 160): P = 60 is not the table's count.  The head against its float64 form on the device's own feats, inside bounds_head."""
    model = _model(f20, "frozen", image_size=(96, 160))
    P = model.cfg.patches
    assert P == 60
    gen = torch.Generator().manual_seed(4)
    img = torch.randn(2, 3, 96, 160, generator=gen).to(DEV)
    emb = f20["tower"].encode(f20["ids"])
    boxes, logits, obj = model.detect(img, emb, objectness=True)
    assert tuple(obj.shape) == (2, P) and torch.equal(boxes, model.detect(img, emb)[0])
    feats = model._workspace(2, train=False)["feats"][:2 * P].float().cpu()
    ref, tol = R.bounds_head(feats, weights.hf_objectness_head(f20["sd"]))
    worst = R.check("rectangular head", obj.cpu().reshape(-1), ref["o"], tol)
    print(f"rectangular (96, 160): worst err / tol {worst:.3f}")


def test_top_objects_is_a_stable_descending_sort(f20):
    model = _model(f20)
    boxes, _, obj = model.detect_text(f20["img"], f20["ids"], f20["tower"], objectness=True)
    P = obj.shape[1]
    tied = obj.clone()
    tied[0, 5], tied[0, 20], tied[1, 3:9] = tied[0, 11], tied[0, 11], 40.0          # exact ties, the second set saturated (sigmoid = 1)
    for name, o in (("device", obj), ("ties", tied)):
        s = torch.sigmoid(o)
        want = torch.sort(s.cpu(), dim=1, stable=True, descending=True)
        for k in (1, 8, P):
            tb, ts, tp = top_objects(boxes, o, k)
            assert tuple(tb.shape) == (B, k, 4) and tp.dtype == torch.int64
            assert torch.equal(tp.cpu(), want.indices[:, :k]), (name, k)
            assert torch.equal(R.bits(ts.cpu()), R.bits(want.values[:, :k]))
            assert torch.equal(tb, torch.gather(boxes, 1, tp[..., None].expand(-1, -1, 4)))
