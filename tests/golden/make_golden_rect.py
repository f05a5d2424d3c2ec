"""Reference fixture for rectangular inputs: tests/golden/f18_rect.npz, written from live Hugging Face transformers.

A random-init `OwlViTForObjectDetection` at the `tiny` geometry (native 96: a 6 x 6 position table), built by the recipe of make_golden_open_vocab.py
(vision weights from weights.make_weights, text weights from weights.make_text_weights, both by seed -- the tests rebuild them; its trained-like logit
head).  Stored:

 * `pos_<gh>x<gw>`: `OwlViTVisionEmbeddings.interpolate_pos_encoding(., gh * 16, gw * 16)` of the native table for the grids (6, 10), (10, 6), (4, 9) --
   the 36 patches of the native table on a rectangle: HF resamples it because height != width -- and (7, 1); `bias_<gh>x<gw>`: HF's
   `compute_box_bias(gh, gw)` for the same grids.
 * one forward at 96 x 160 with `interpolate_pos_encoding=True`, 2 images, 5 text queries per image: `pixel_levels` (the u8 levels
   synth.make_images(cfg at (96, 160), 2, seed=IMG_SEED) normalises; asserted here), `query_embeds` (HF's text_embeds), `logits`, `pred_boxes` (HF's
   cxcywh) and `scale` (ELU(w_scale . f + b_scale) + 1 per patch in float64, what tests/test_open_vocab_model_gpu.py's tolerance is built from).

Run where transformers is installed:  python tests/golden/make_golden_rect.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from owl_vit_object_detection_amd import synth  # noqa: E402
from owl_vit_object_detection_amd.config import get_config, get_text_config  # noqa: E402
from tests.golden import make_golden_open_vocab as OV  # noqa: E402

CNAME = "tiny"
GRIDS = ((6, 10), (10, 6), (4, 9), (7, 1))
HW = (96, 160)
B, Q = 2, 5
IMG_SEED = 1818
PROMPT_SEED = 1001


def main():
    import transformers
    cfg, tc = get_config(CNAME), get_text_config(CNAME)
    head = OV.logit_head(cfg)
    hf = OV.build_hf(cfg, tc, head)
    ps, D = cfg.patch_size, cfg.hidden
    res = {"transformers_version": np.asarray([int(v) for v in transformers.__version__.split(".")[:3]]), "img_seed": np.asarray([IMG_SEED]),
           "hw": np.asarray(HW), "grids": np.asarray(GRIDS)}
    emb = hf.owlvit.vision_model.embeddings
    with torch.no_grad():
        for gh, gw in GRIDS:
            table = emb.interpolate_pos_encoding(torch.zeros(1, gh * gw + 1, D), gh * ps, gw * ps)
            assert tuple(table.shape) == (1, gh * gw + 1, D)
            res[f"pos_{gh}x{gw}"] = table[0].numpy()
            res[f"bias_{gh}x{gw}"] = hf.compute_box_bias(gh, gw).numpy()
        assert not np.array_equal(res["pos_4x9"], emb.position_embedding.weight.numpy()), "HF must resample the 36-patch rectangle"
        rect = cfg.replace(image_size=HW, pos_grid=cfg.grid)
        img = synth.make_images(rect, B, seed=IMG_SEED)
        levels = synth.make_images_u8(rect, B, seed=IMG_SEED, layout="chw")
        x = levels.astype(np.float64) / 255.0
        assert np.array_equal(((x - synth.CLIP_MEAN[:, None, None]) / synth.CLIP_STD[:, None, None]).astype(np.float32), img)
        ids = OV.prompts(tc, PROMPT_SEED)[:B]
        flat = torch.from_numpy(ids.reshape(B * Q, -1))
        att = (torch.arange(flat.shape[1])[None, :] <= flat.argmax(1)[:, None]).to(torch.int64)
        out = hf(input_ids=flat, attention_mask=att, pixel_values=torch.from_numpy(img), interpolate_pos_encoding=True)
    P = (HW[0] // ps) * (HW[1] // ps)
    assert tuple(out.logits.shape) == (B, P, Q) and tuple(out.pred_boxes.shape) == (B, P, 4)
    f = out.image_embeds.double().reshape(B, P, D)
    xs = f @ torch.from_numpy(head["logit_scale.weight"]).double() + float(head["logit_scale.bias"])
    assert bool((xs > 0.05).any()) and bool((xs < -0.05).any()), "the ELU's argument must take both signs across patches"
    res.update({"pixel_levels": levels, "input_ids": ids, "query_mask": ids[..., 0] > 0, "query_embeds": out.text_embeds.numpy().reshape(B, Q, -1),
                "logits": out.logits.numpy(), "pred_boxes": out.pred_boxes.numpy(), "scale": (torch.where(xs > 0, xs, torch.expm1(xs)) + 1.0).numpy(),
                **{"head/" + k: np.asarray(v, np.float32) for k, v in head.items()}})
    path = os.path.join(HERE, "f18_rect.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    assert size < 200 * 1024, size
    print(f"wrote {path}: {size} bytes; grids {GRIDS}; forward at {HW}: logits in [{float(out.logits.min()):.2f}, {float(out.logits.max()):.2f}]")


if __name__ == "__main__":
    main()
