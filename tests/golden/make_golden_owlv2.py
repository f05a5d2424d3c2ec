"""Reference fixture for OWLv2's input stage: tests/golden/f19_owlv2_input.npz, written from live Hugging Face transformers (and, under it, scipy).

 Input cases: for every (H, W) -> N of tests/owlv2_input_reference.CASES the seeded u8 source (`src/<H>x<W>_<N>`) and HF's
   `Owlv2ImageProcessorPil(size=N x N)` pixel_values (`pv/...`, float32 [3, N, N]); N <= 48, a few hundred KB in all.
 Model case: a u8 70 x 100 image, HF's processor at 96 (`m_pixel_values`), and `Owlv2ForObjectDetection` at the `tiny` geometry -- vision weights from
   weights.make_weights, text weights from weights.make_text_weights, both loaded through the `owlv2.` names (`v2_state_dict`, which the GPU test
   rebuilds by seed), the logit head of make_golden_open_vocab.logit_head -- run on five prompts: stored are HF's text_embeds (the queries), logits,
   pred_boxes (cxcywh, normalised to the padded square), image_embeds and `post_process_object_detection(threshold=0, target_sizes=[(70, 100)])`'s pixel
   boxes, which are `_scale_boxes` = both axes times max(h, w).

Run where transformers and scipy are installed:  python tests/golden/make_golden_owlv2.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from owl_vit_object_detection_amd import weights  # noqa: E402
from owl_vit_object_detection_amd.config import get_config, get_text_config  # noqa: E402
from tests import owlv2_input_reference as R  # noqa: E402

CNAME = "tiny"
M_H, M_W = 70, 100           # the model case's image
M_Q = 5
PROMPT_SEED = 1919


def v2_state_dict(cfg, tc=None):
    """weights.make_weights (and, with `tc`, weights.make_text_weights) under Owlv2ForObjectDetection's names, plus the six `objectness_head.*` tensors
    (zeros: the path skips them) -- float32 ndarrays.  No transformers needed: the GPU test rebuilds the dict with this."""
    sd = {}
    for name, arr in weights.make_weights(cfg).items():
        if name == "queries":
            continue
        if name.startswith("backbone."):
            key = "owlv2.vision_model." + name[len("backbone."):]
        elif name.startswith("post_post_layernorm."):
            key = "layer_norm." + name[len("post_post_layernorm."):]
        elif name.startswith("class_predictor.dense0."):
            key = "class_head.dense0." + name[len("class_predictor.dense0."):]
        else:
            key = name
        sd[key] = arr.copy()
    if tc is not None:
        for name, arr in weights.make_text_weights(tc).items():
            sd["owlv2." + name] = arr.copy()
    D = cfg.hidden
    for k, shape in (("dense0.weight", (D, D)), ("dense0.bias", (D,)), ("dense1.weight", (D, D)), ("dense1.bias", (D,)), ("dense2.weight", (1, D)), ("dense2.bias", (1,))):
        sd["objectness_head." + k] = np.zeros(shape, np.float32)
    return sd


def build_hf(cfg, tc, head):
    import torch
    from transformers import Owlv2Config, Owlv2ForObjectDetection
    hf_cfg = Owlv2Config(
        vision_config=dict(hidden_size=cfg.hidden, intermediate_size=cfg.mlp, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                           image_size=cfg.image_size, patch_size=cfg.patch_size, hidden_act="quick_gelu", layer_norm_eps=cfg.ln_eps),
        text_config=dict(hidden_size=tc.width, intermediate_size=tc.mlp, num_hidden_layers=tc.layers, num_attention_heads=tc.heads, vocab_size=tc.vocab,
                         max_position_embeddings=tc.max_pos, hidden_act="quick_gelu", layer_norm_eps=tc.ln_eps, bos_token_id=tc.vocab - 2,
                         eos_token_id=tc.vocab - 1, pad_token_id=0),
        projection_dim=tc.proj_dim)
    hf_cfg._attn_implementation = "eager"
    hf_cfg.text_config._attn_implementation = "eager"
    hf_cfg.vision_config._attn_implementation = "eager"
    hf = Owlv2ForObjectDetection(hf_cfg).eval()
    sd = hf.state_dict()
    for key, arr in v2_state_dict(cfg, tc).items():
        assert key in sd and tuple(sd[key].shape) == arr.shape, (key, arr.shape)
        sd[key] = torch.from_numpy(arr)
    for k, v in head.items():
        key = "class_head." + k
        sd[key] = torch.from_numpy(np.asarray(v, np.float32)).reshape(sd[key].shape)
    hf.load_state_dict(sd)
    return hf


def hf_pixel_values(img, N):
    from transformers.models.owlv2.image_processing_pil_owlv2 import Owlv2ImageProcessorPil
    proc = Owlv2ImageProcessorPil(size={"height": N, "width": N})
    # (channels_last said, not inferred: HF reads a 1 x 40 x 3 image as channels-first otherwise)
    pv = np.asarray(proc(images=img, return_tensors="np", input_data_format="channels_last")["pixel_values"])
    assert pv.shape == (1, 3, N, N) and pv.dtype == np.float32, (pv.shape, pv.dtype)
    return pv[0]


def main():
    import torch
    import transformers
    from transformers.models.owlv2.image_processing_pil_owlv2 import Owlv2ImageProcessorPil
    from tests.golden.make_golden_open_vocab import logit_head, prompts
    res = {"transformers_version": np.asarray([int(v) for v in transformers.__version__.split(".")[:3]])}
    worst = 0.0
    for H, W, N in R.CASES:
        img = R.make_image(H, W)
        pv = hf_pixel_values(img, N)
        worst = max(worst, float(np.abs(pv - R.forward64(img, N)).max()))
        res["src/" + R.case_key(H, W, N)], res["pv/" + R.case_key(H, W, N)] = img, pv
    # ---- the model case
    cfg, tc = get_config(CNAME), get_text_config(CNAME)
    head = logit_head(cfg)
    hf = build_hf(cfg, tc, head)
    m_img = R.make_image(M_H, M_W)
    m_pv = hf_pixel_values(m_img, cfg.image_size)
    ids = prompts(tc, PROMPT_SEED)[0, :M_Q]
    flat = torch.from_numpy(ids)
    att = (torch.arange(flat.shape[1])[None, :] <= flat.argmax(1)[:, None]).to(torch.int64)
    with torch.no_grad():
        out = hf(input_ids=flat, attention_mask=att, pixel_values=torch.from_numpy(m_pv)[None])
    pp = Owlv2ImageProcessorPil().post_process_object_detection(out, threshold=0.0, target_sizes=[(M_H, M_W)])[0]
    P = out.logits.shape[1]
    assert len(pp["boxes"]) == P          # a sigmoid is > 0: every patch is kept, in patch order
    res.update({"m_src": m_img, "m_pixel_values": m_pv, "m_input_ids": ids, "m_text_embeds": out.text_embeds.numpy().reshape(1, M_Q, -1),
                "m_logits": out.logits.numpy(), "m_pred_boxes": out.pred_boxes.numpy(), "m_image_embeds": out.image_embeds.numpy().reshape(1, P, cfg.hidden),
                "m_pp_boxes": pp["boxes"].numpy(), "m_size": np.asarray([M_H, M_W]), **{"head/" + k: np.asarray(v, np.float32) for k, v in head.items()}})
    path = os.path.join(HERE, "f19_owlv2_input.npz")
    np.savez_compressed(path, **res)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; {len(R.CASES)} input cases, worst |HF - float64 restatement| {worst:.3e}; model case "
          f"{M_H} x {M_W} -> {cfg.image_size}, {P} patches, {M_Q} prompts")


if __name__ == "__main__":
    main()
