"""Reference fixture for the image-conditioned queries: tests/golden/f14_image_query.npz, written from live Hugging Face transformers.

A random-init `OwlViTForObjectDetection` at the `tiny` geometry (6 x 6 patches, width 128, class embeddings of width 64) is handed 6 random feature
maps [6, 6, 6, 128] and asked for `embed_image_query` (HF5 modeling_owlvit.py:1246-1288).  Stored, arrays only: HF's `class_embeds` [6, 36, 64] (the
un-normalised output of the class head's dense0), the predicted boxes as corners [6, 36, 4], HF's `query_embeds` [6, 64] and `box_indices` [6], and
the transformers version.  The generator searches seeds until HF's own margins -- every box's distance from the 80 % threshold and the gap between
the two smallest mean similarities -- exceed 1e-4 on all 6 cases, and asserts that it found such a seed, so the pin does not hang on f32 round-off.
tests/test_image_query_reference.py holds the float64 restatement to it.

Run where transformers is installed:  python tests/golden/make_golden_image_queries.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES, GRID, WIDTH, DT = 6, 6, 128, 64
MARGIN = 1e-4
FEATURE_SCALE = 8.0          # random-init heads have weights of std 0.02: unit features would give embeddings (and margins) of 1e-2


def hf_case(seed):
    """-> dict of numpy arrays of one seed, with HF's own margins (`margin_thr`, `margin_sim`, each [6])."""
    import torch
    from transformers import OwlViTConfig, OwlViTForObjectDetection
    from transformers.models.owlvit.modeling_owlvit import box_iou, center_to_corners_format
    torch.manual_seed(seed)
    cfg = OwlViTConfig(text_config=dict(hidden_size=DT, intermediate_size=2 * DT, num_hidden_layers=1, num_attention_heads=1, vocab_size=97, max_position_embeddings=16, bos_token_id=1, eos_token_id=2),
                       vision_config=dict(hidden_size=WIDTH, intermediate_size=2 * WIDTH, num_hidden_layers=1, num_attention_heads=2, image_size=16 * GRID, patch_size=16),
                       projection_dim=DT)
    model = OwlViTForObjectDetection(cfg).eval()
    fmap = FEATURE_SCALE * torch.randn(CASES, GRID, GRID, WIDTH)
    feats = fmap.reshape(CASES, GRID * GRID, WIDTH)
    with torch.no_grad():
        query_embeds, box_indices, pred_boxes = model.embed_image_query(feats, fmap)
        _, class_embeds = model.class_predictor(feats)
        boxes = center_to_corners_format(pred_boxes)
        m_thr, m_sim = [], []
        for n in range(CASES):
            iou = box_iou(torch.tensor([[0.0, 0.0, 1.0, 1.0]]), boxes[n])[0][0]
            thr = iou.max() * 0.8
            m_thr.append(float((iou - thr).abs().min()))
            sims = torch.einsum("d,id->i", class_embeds[n].mean(0), class_embeds[n][iou >= thr])
            top = sims.sort().values
            m_sim.append(float(top[1] - top[0]) if top.numel() > 1 else float("inf"))
    assert query_embeds.shape == (CASES, 1, DT) and box_indices.shape == (CASES, 1)          # (no case dropped: the whole image overlaps every box)
    return dict(class_embeds=class_embeds.numpy().astype(np.float32), boxes=boxes.numpy().astype(np.float32),
                query_embeds=query_embeds[:, 0].numpy().astype(np.float32), box_indices=box_indices[:, 0].numpy().astype(np.int64),
                margin_thr=np.asarray(m_thr), margin_sim=np.asarray(m_sim))


def main():
    import transformers
    found = None
    for seed in range(14, 14 + 200):
        case = hf_case(seed)
        if case["margin_thr"].min() > MARGIN and case["margin_sim"].min() > MARGIN:
            found = seed
            break
    assert found is not None, "no seed in 200 gives HF margins above 1e-4 on all 6 cases"
    out = {"transformers_version": np.asarray([int(v) for v in transformers.__version__.split(".")[:3]]), "seed": np.asarray([found]),
           "geometry": np.asarray([CASES, GRID, WIDTH, DT]), **case}
    path = os.path.join(HERE, "f14_image_query.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, seed {found}, margins thr {case['margin_thr'].min():.3e} sim {case['margin_sim'].min():.3e}")


if __name__ == "__main__":
    main()
