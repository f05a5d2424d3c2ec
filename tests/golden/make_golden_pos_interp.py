"""Reference fixture for the resampled position table: tests/golden/f13_pos_interp.npz, written from live Hugging Face transformers.

A random-init `OwlViTVisionModel` at the `tiny` geometry (96 x 96 pixels in 16-pixel patches, width 128: a 6 x 6 + 1 row position table) is asked for
`embeddings.interpolate_pos_encoding` at 128 x 128 (8 x 8 + 1 rows), HF's `interpolate_pos_encoding=True` path.  Stored: the native table and that
output, both float32 (arrays only).  tests/test_pos_resample_reference.py holds the float64 tap-matrix reference to it at f32 round-off, so the pin
survives on a machine without transformers.

Run where transformers is installed:  python tests/golden/make_golden_pos_interp.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE, PATCH, WIDTH, SIZE = 96, 16, 128, 128


def main():
    import torch
    import transformers
    from transformers import OwlViTVisionConfig, OwlViTVisionModel
    torch.manual_seed(13)
    cfg = OwlViTVisionConfig(hidden_size=WIDTH, intermediate_size=2 * WIDTH, num_hidden_layers=1, num_attention_heads=2, image_size=NATIVE, patch_size=PATCH)
    emb = OwlViTVisionModel(cfg).eval().vision_model.embeddings
    g = SIZE // PATCH
    with torch.no_grad():
        native = emb.position_embedding.weight.detach().clone()
        used = emb.interpolate_pos_encoding(torch.zeros(1, g * g + 1, WIDTH), SIZE, SIZE)[0]
    assert native.shape == ((NATIVE // PATCH) ** 2 + 1, WIDTH) and used.shape == (g * g + 1, WIDTH)
    out = {"transformers_version": np.asarray([int(v) for v in transformers.__version__.split(".")[:3]]),
           "geometry": np.asarray([NATIVE, PATCH, WIDTH, SIZE]), "native": native.numpy().astype(np.float32), "used": used.numpy().astype(np.float32)}
    path = os.path.join(HERE, "f13_pos_interp.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
