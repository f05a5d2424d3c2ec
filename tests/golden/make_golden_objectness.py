"""Reference fixture for OWLv2's objectness head: tests/golden/f20_owlv2_objectness.npz, written from live Hugging Face transformers.

`Owlv2ForObjectDetection` at the `tiny` geometry (make_golden_owlv2.build_hf: vision weights from weights.make_weights, text weights from
weights.make_text_weights, the logit head of make_golden_open_vocab.logit_head) with a seeded NON-ZERO objectness head -- `objectness_head(cfg, seed)`
below: weights at the box head's init scale (std D^-0.5), biases 0.02 z, dense2.bias = -1 -- which the GPU test re-runs by seed: the weights are not
stored, only `head_seed`.  Three seeded 96 x 96 inputs (synth.make_images, IMG_SEED), five prompts shared by the batch.

Stored: HF's objectness_logits [3, P], logits [3, P, 5], pred_boxes (cxcywh), feats = image_embeds [3, P, D], input_ids [5, S].
Gradient case: L = binary_cross_entropy_with_logits(objectness_logits, t, reduction="sum") / 3 on a seeded 0/1 target `t`; stored: HF's autograd gradient
of the six tensors (`grad/<key>`, HF's shapes).  The vision tower's gradient from that loss is asserted None or zero: HF detaches the features.
Per-element tolerance `tol` [3, P]: tests/objectness_reference.model_tolerance on HF's feats -- the 1e-2 feature bar of tests/test_model_gpu.py carried
through the float64 head to first order, plus the head's two bf16 hidden layers' storage roundings, by torch autograd in double.
At these tolerances (a few 1e-2 against a logit spread of a few 1e-1) a fixed-k top set is not decided, so none is asserted against HF.  Instead the
generator searches the head seed until every image's arg-max patch leads the runner-up by more than the sum of their two tolerances, and asserts it.

Run where transformers is installed:  python tests/golden/make_golden_objectness.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from owl_vit_object_detection_amd import rng as crng, synth  # noqa: E402
from owl_vit_object_detection_amd.config import get_config, get_text_config  # noqa: E402

CNAME = "tiny"
B, Q = 3, 5
IMG_SEED = 2020
PROMPT_SEED = 2021
TARGET_SEED = 2022
HEAD_SEEDS = range(200, 400)          # the search's extent
KEYS = ("dense0.weight", "dense0.bias", "dense1.weight", "dense1.bias", "dense2.weight", "dense2.bias")


def objectness_head(cfg, seed):
    """The six tensors as weights.hf_objectness_head gives them (float32; dense2.weight [D], dense2.bias 0-d).  numpy only."""
    D = cfg.hidden
    n = lambda name, k: crng.normal(seed, "objectness_head." + name, k)
    return {"dense0.weight": (D ** -0.5 * n("dense0.weight", D * D)).reshape(D, D).astype(np.float32), "dense0.bias": (0.02 * n("dense0.bias", D)).astype(np.float32),
            "dense1.weight": (D ** -0.5 * n("dense1.weight", D * D)).reshape(D, D).astype(np.float32), "dense1.bias": (0.02 * n("dense1.bias", D)).astype(np.float32),
            "dense2.weight": (D ** -0.5 * n("dense2.weight", D)).astype(np.float32), "dense2.bias": np.float32(-1.0)}


def target(cfg):
    """The gradient case's 0/1 target [B, P] float32."""
    return (crng.uniform(TARGET_SEED, "objectness/target", B * cfg.patches) < 0.2).astype(np.float32).reshape(B, cfg.patches)


def input_ids(tc):
    from tests.golden.make_golden_open_vocab import prompts
    return prompts(tc, PROMPT_SEED)[0, :Q]


def set_head(hf, head):
    import torch
    sd = hf.state_dict()
    for k in KEYS:
        key = "objectness_head." + k
        sd[key] = torch.from_numpy(np.asarray(head[k], np.float32)).reshape(sd[key].shape)
    hf.load_state_dict(sd)


def main():
    import torch
    import transformers
    from tests import objectness_reference as R
    from tests.golden.make_golden_open_vocab import logit_head
    from tests.golden.make_golden_owlv2 import build_hf
    cfg, tc = get_config(CNAME), get_text_config(CNAME)
    hf = build_hf(cfg, tc, logit_head(cfg))
    img = torch.from_numpy(synth.make_images(cfg, B, seed=IMG_SEED))
    ids = input_ids(tc)
    flat = torch.from_numpy(np.tile(ids, (B, 1)))
    att = (torch.arange(flat.shape[1])[None, :] <= flat.argmax(1)[:, None]).to(torch.int64)
    P, D = cfg.patches, cfg.hidden
    with torch.no_grad():
        feats = hf.image_embedder(pixel_values=img)[0].reshape(B, P, D)
    chosen = None
    for seed in HEAD_SEEDS:
        head = objectness_head(cfg, seed)
        o = R.head64(feats.reshape(B * P, D), head)["o"].reshape(B, P)
        tol = R.model_tolerance(feats.reshape(B * P, D), head).reshape(B, P)
        top = torch.topk(o, 2, dim=1)
        lead = top.values[:, 0] - top.values[:, 1] - tol.gather(1, top.indices).sum(1)
        if bool((lead > 0).all()):
            chosen = (seed, head, tol, float(lead.min()))
            break
    assert chosen is not None, "no head seed decides every image's arg-max patch"
    seed, head, tol, lead = chosen
    set_head(hf, head)
    for p in hf.parameters():
        p.requires_grad_(True)
    out = hf(input_ids=flat, attention_mask=att, pixel_values=img)
    obj = out.objectness_logits
    assert tuple(obj.shape) == (B, P)
    o64 = R.head64(feats.reshape(B * P, D), head)["o"].reshape(B, P)
    assert float((obj.detach().double() - o64).abs().max()) < 1e-5
    top = torch.topk(o64, 2, dim=1)
    assert bool((top.values[:, 0] - top.values[:, 1] > tol.gather(1, top.indices).sum(1)).all())          # the margin the GPU test's arg-max check rests on
    t = torch.from_numpy(target(cfg))
    loss = torch.nn.functional.binary_cross_entropy_with_logits(obj, t, reduction="sum") / B
    loss.backward()
    sd_grads = {n: p.grad for n, p in hf.named_parameters()}
    for n, g in sd_grads.items():
        if not n.startswith("objectness_head."):
            assert g is None or float(g.abs().max()) == 0.0, n          # HF detaches the features: nothing reaches the trunk (or any other head)
    res = {"transformers_version": np.asarray([int(v) for v in transformers.__version__.split(".")[:3]]), "head_seed": np.asarray(seed),
           "input_ids": ids, "objectness_logits": obj.detach().numpy(), "logits": out.logits.detach().numpy(), "pred_boxes": out.pred_boxes.detach().numpy(),
           "feats": feats.numpy(), "tol": tol.numpy(), "target": t.numpy(), "loss": np.asarray(float(loss.detach()))}
    for k in KEYS:
        res["grad/" + k] = sd_grads["objectness_head." + k].detach().numpy()
    path = os.path.join(HERE, "f20_owlv2_objectness.npz")
    np.savez_compressed(path, **res)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; head seed {seed}; logits {float(o64.min()):.3f} .. {float(o64.max()):.3f} (spread per image "
          f"{[round(float(v), 3) for v in (o64.max(1).values - o64.min(1).values)]}), tol {float(tol.min()):.3f} .. {float(tol.max()):.3f}, arg-max lead over the "
          f"two tolerances {lead:.3f}; loss {float(loss):.4f}")


if __name__ == "__main__":
    main()
