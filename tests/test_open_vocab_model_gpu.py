"""-m gpu: zero-shot inference (OwlViT.detect / detect_text) on a real MI355X against Hugging Face's OwlViTForObjectDetection, fixture F15
(tests/golden/make_golden_open_vocab.py), on `tiny`, with one case on `tiny-l14`.

The tolerance on a logit is not a free number: it is the forward budget tests/test_model_gpu.py already asserts at this geometry carried through the
head's formula (make_golden_open_vocab.model_tolerance): |d logit| <= scale (d_cos + d_shift) + |cos + shift| d_scale, d_cos = its bar on pred_sims
(3.5e-3), d_shift / d_scale = sum |w| x its 1e-2 bar on an O(1) output of the bf16 trunk, ELU's slope <= 1.  Each test prints its worst err / tol;
profiles/open_vocab_reference.md records them."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import synth, weights  # noqa: E402
from owl_vit_object_detection_amd.config import get_config, get_text_config  # noqa: E402
from owl_vit_object_detection_amd.losses import PushPullLoss  # noqa: E402
from owl_vit_object_detection_amd.models import OwlViT, load_model  # noqa: E402
from owl_vit_object_detection_amd.optim import FusedAdamW  # noqa: E402
from owl_vit_object_detection_amd.postprocess import PostProcess  # noqa: E402
from owl_vit_object_detection_amd.text import TextTower  # noqa: E402
from tests.golden.make_golden_open_vocab import D_BOXES, THRESHOLD, model_tolerance  # noqa: E402

DEV = "cuda"
FMIN = float(torch.finfo(torch.float32).min)


@pytest.fixture(scope="module")
def f15(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "f15_open_vocab.npz")))
    cfg = get_config("tiny")
    head = {k: g["head/" + k] for k in weights.LOGIT_HEAD_KEYS}
    model = OwlViT(cfg, weights.make_weights(cfg), DEV)
    assert model.logit_head is None
    model.set_logit_head(head)
    tower = TextTower(get_text_config("tiny"), None, DEV)
    img = torch.from_numpy(np.concatenate([synth.make_images(cfg, 1, seed=int(g["img_seed"][0]), first=int(i)) for i in g["img_index"]])).to(DEV)
    # the reference's scale and cos + shift per patch, in float64 from the stored HF tensors
    f = torch.from_numpy(g["image_embeds"]).double()
    x = f @ torch.from_numpy(head["logit_scale.weight"]).double() + float(head["logit_scale.bias"])
    scale = (torch.where(x > 0, x, torch.expm1(x)) + 1.0)[..., None].numpy()
    return dict(g=g, cfg=cfg, head=head, model=model, tower=tower, img=img, scale=scale)


def _corners(cxcywh):
    cx, cy, w, h = (cxcywh[..., k] for k in range(4))
    return np.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def test_detect_text_against_hf(f15):
    g, model = f15["g"], f15["model"]
    B, P, Q = g["logits"].shape
    boxes, logits, scores = model.detect_text(f15["img"], g["input_ids"], f15["tower"], return_scores=True)
    torch.cuda.synchronize()
    assert boxes.shape == (B, P, 4) and logits.shape == (B, P, Q) and scores.shape == (B, P, Q) and logits.dtype == torch.float32
    lg, sc, ref = logits.cpu().double().numpy(), scores.cpu().numpy(), g["logits"].astype(np.float64)
    live = np.broadcast_to(g["query_mask"][:, None, :], ref.shape)
    tol = model_tolerance(f15["scale"], ref / f15["scale"], f15["head"]["logit_shift.weight"], f15["head"]["logit_scale.weight"])
    ratio = np.where(live, np.abs(lg - ref) / tol, 0.0)
    eb = float(np.abs(boxes.cpu().numpy() - _corners(g["pred_boxes"])).max())
    print(f"detect_text vs HF (tiny, B={B}, Q={Q}): max |d logit| {float(np.abs(lg - ref)[live].max()):.3e}, worst err / tol {ratio.max():.3f} "
          f"(tol {tol[live].min():.2e} .. {tol[live].max():.2e}); max |d boxes| {eb:.3e} (bar {D_BOXES})")
    # masked entries: exactly finfo.min, score exactly 0
    assert np.array_equal(lg[~live], np.full_like(lg[~live], FMIN)) and not sc[~live].any() and int((~live).sum()) == 2 * P
    assert ratio.max() <= 1.0
    assert eb < D_BOXES          # corners here, (cx, cy, w, h) in HF
    # the per-patch arg-max query is HF's on every decided patch (the generator holds the undecided ones to 5 %)
    decided = g["decided"]
    assert decided.mean() >= 0.95
    ours, theirs = logits.argmax(-1).cpu().numpy(), np.where(live, ref, -np.inf).argmax(-1)
    assert np.array_equal(ours[decided], theirs[decided]), np.nonzero(ours != theirs)
    assert np.array_equal(sc > 0, live)
    # the [B Q, S] layout of HF and the [B, Q, S] one are the same call; a [Q, S] list shared by the batch is image 0's prompts for every image
    b2, l2 = model.detect_text(f15["img"], g["input_ids"].reshape(B * Q, -1), f15["tower"])
    assert torch.equal(l2, logits) and torch.equal(b2, boxes)
    b3, l3 = model.detect_text(f15["img"], g["input_ids"][0], f15["tower"], shared=True)
    assert torch.equal(l3[0], logits[0]) and not torch.equal(l3[2], logits[2])


def test_post_process_is_hfs_detection_set(f15):
    """HF's post_process_object_detection = PostProcess(confidence_threshold, iou_threshold=1.0) on `scores`: the same (patch, label) set, scores and
    boxes for every detection whose score is further from the threshold than the tolerance."""
    g, model, cfg = f15["g"], f15["model"], f15["cfg"]
    B, P, Q = g["logits"].shape
    boxes, logits, scores = model.detect_text(f15["img"], g["input_ids"], f15["tower"], return_scores=True)
    pp = PostProcess(confidence_threshold=THRESHOLD, iou_threshold=1.0)
    ob, oc, osc = pp(boxes, scores)
    counts, patch = pp.last_counts.cpu().numpy(), pp.last_patch_idx.cpu().numpy()
    ob, oc, osc = ob.cpu().numpy(), oc.cpu().numpy(), osc.cpu().numpy()
    ref = g["logits"].astype(np.float64)
    live = np.broadcast_to(g["query_mask"][:, None, :], ref.shape)
    tol = model_tolerance(f15["scale"], ref / f15["scale"], f15["head"]["logit_shift.weight"], f15["head"]["logit_scale.weight"])
    checked = 0
    for b in range(B):
        top = np.where(live[b], ref[b], -np.inf)
        best = top.argmax(-1)
        s_ref = 1.0 / (1.0 + np.exp(-top.max(-1)))
        s_tol = 0.25 * np.take_along_axis(tol[b], best[:, None], -1)[:, 0]          # sigmoid's slope is at most 1 / 4
        hf_patches = np.nonzero(s_ref > THRESHOLD)[0]          # HF filters in patch order: its n-th detection is the n-th such patch
        n = int(g["pp_count"][b])
        assert len(hf_patches) == n and np.allclose(g["pp_scores"][b, :n], s_ref[hf_patches], atol=1e-6) and np.array_equal(g["pp_labels"][b, :n], best[hf_patches])
        mine = {int(p): k for k, p in enumerate(patch[b, :counts[b]])}
        for j, p in enumerate(range(P)):
            if abs(s_ref[p] - THRESHOLD) <= s_tol[p]:
                continue
            checked += 1
            assert (p in mine) == (s_ref[p] > THRESHOLD), (b, p)
            if p in mine:
                k = mine[p]
                assert abs(float(osc[b, k]) - s_ref[p]) <= s_tol[p] + 1e-6
                if g["decided"][b, p]:
                    assert int(oc[b, k]) == int(best[p])
                n_hf = int(np.nonzero(hf_patches == p)[0][0])
                assert float(np.abs(ob[b, k] * cfg.image_size - g["pp_boxes"][b, n_hf]).max()) < D_BOXES * cfg.image_size
    assert checked >= 0.9 * B * P
    print(f"post-process: {checked} of {B * P} patches further from the threshold than the tolerance, all in HF's set; counts {counts.tolist()} (HF {g['pp_count'].tolist()})")


@pytest.mark.parametrize("cname", ["tiny", "tiny-l14"])
def test_image_guided_detection(f15, cname):
    """`detect(img, embed_image_query(ex)[0][None])` is HF's image_guided_detection for one exemplar.  On `tiny` against the fixture's case B (logits under
    the same tolerance, the same box index); on `tiny-l14` (frozen layers above the trainable one) the call against detect on the same query handed in
    as a shared bank, and against the float64 head on the device's own e and features."""
    g = f15["g"]
    if cname == "tiny":
        model, cfg = f15["model"], f15["cfg"]
    else:
        cfg = get_config(cname)
        model = load_model({i: f"c{i}" for i in range(cfg.n_classes)}, DEV, arch=cname, logit_head=f15["head"])
        assert model.logit_head is not None
    P = cfg.patches
    ex = torch.from_numpy(synth.make_images(cfg, 1, seed=int(g["img_seed"][0]), first=int(g["b_query_first"][0]))).to(DEV)
    q, idx, _ = model.embed_image_query(ex)
    boxes, logits = model.detect(f15["img"][:1], q[None])
    torch.cuda.synchronize()
    assert logits.shape == (1, P, 1) and boxes.shape == (1, P, 4)
    b2, l2 = model.detect(f15["img"][:1], q)          # [Q, Dt]: the shared-bank form, same bits
    assert torch.equal(l2, logits) and torch.equal(b2, boxes)
    if cname == "tiny":
        ref = g["b_logits"].astype(np.float64)
        tol = model_tolerance(f15["scale"][:1], ref / f15["scale"][:1], f15["head"]["logit_shift.weight"], f15["head"]["logit_scale.weight"])
        err = np.abs(logits.cpu().double().numpy() - ref)
        print(f"image-guided vs HF: box index {int(idx[0])} (HF {int(g['b_box_index'][0])}); max |d logit| {err.max():.3e}, worst err / tol {(err / tol).max():.3f}")
        assert int(idx[0]) == int(g["b_box_index"][0])
        assert (err / tol).max() <= 1.0
    else:
        from tests import open_vocab_reference as R
        ws = model._workspace(1, train=False)
        lh = model.logit_head
        r = R.exact_logits(ws["e"][:P].cpu(), q.cpu(), ws["feats"][:P].cpu(), lh["logit_shift.weight"].cpu(), lh["logit_shift.bias"].cpu(),
                           lh["logit_scale.weight"].cpu(), lh["logit_scale.bias"].cpu(), 1, P)
        worst = R.check_logits("tiny-l14 detect on its own e / feats", logits, None, r)
        print(f"tiny-l14 image-guided: err / tol against the float64 head on the device's e and features {worst[0]:.3f}")


def _train_setup(B=2):
    cfg = get_config("tiny")
    model = OwlViT(cfg, weights.make_weights(cfg), DEV)
    img = torch.from_numpy(synth.make_images(cfg, B)).to(DEV)
    labels, boxes = synth.make_targets(cfg, B, max_boxes=5)
    return cfg, model, img, [torch.from_numpy(l).to(DEV) for l in labels], [torch.from_numpy(b).to(DEV) for b in boxes], PushPullLoss(cfg.n_classes, None)


@pytest.mark.parametrize("overlap", [False, True])
def test_detect_between_training_steps_moves_nothing(f15, overlap):
    """detect between a training forward and its backward, and between two steps (FusedAdamW in line and with the deferred tail): losses and flat_param
    are bitwise those of a twin model that never called it; model(image) before and after is bitwise equal; without a logit head it raises."""
    g = f15["g"]
    qe = torch.from_numpy(g["text_embeds"]).to(DEV)

    def train(with_detect, steps=3):
        cfg, model, img, lab, box, crit = _train_setup()
        opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1, overlap=overlap)
        if with_detect:
            with pytest.raises(RuntimeError, match="logit head"):
                model.detect(f15["img"], qe)
            model.set_logit_head(f15["head"])
            n_params, sd_keys = sum(p.numel() for p in model.parameters()), list(model.state_dict())
            assert not any("logit" in k for k in sd_keys)
        hist, seen = [], []
        for s in range(steps):
            opt.zero_grad()
            pb, _, ps, _ = model(img)
            if with_detect:          # between a recording forward and its backward, at another batch size and at the same one
                seen.append(model.detect(f15["img"], qe, torch.from_numpy(g["query_mask"]))[1])
                seen.append(model.detect(img, qe[0])[1])
            l = crit(ps, lab, pb, box)
            loss = l["loss_ce"] + l["loss_bg"] + l["loss_bbox"] + l["loss_giou"]
            loss.backward()
            hist.append(loss.detach())
            opt.step()
            if with_detect:          # behind the (possibly deferred) optimizer step
                seen.append(model.detect(f15["img"], qe)[1])
        model.finish()
        torch.cuda.synchronize()
        if with_detect:
            assert sum(p.numel() for p in model.parameters()) == n_params and list(model.state_dict()) == sd_keys
            assert not torch.equal(seen[0], seen[-1])          # the trained weights moved its logits: it read the current parameters
        return model.flat_param.clone(), torch.stack(hist).cpu(), model

    p0, h0, _ = train(False)
    p1, h1, model = train(True)
    assert torch.equal(h0, h1) and torch.equal(p0, p1)
    with torch.no_grad():
        img = f15["img"]
        a = model(img)
        d1 = model.detect(img, qe, return_scores=True)
        b = model(img)
        d2 = model.detect(img, qe, return_scores=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and all(torch.equal(u, v) for u, v in zip(d1, d2))
    assert torch.equal(d1[0], a[0])          # detect's boxes are forward's
