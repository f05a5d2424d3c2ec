"""Reference fixture for the colour half of train-time augmentation: tests/golden/f16_color.npz, written from live Pillow.

For every case of tests/color_reference.cases() on 24 x 24 canvases -- boxed bicubic resizes of four small uint8 sources into the cells of the canvases,
each cell then put through `ImageEnhance.Brightness / Contrast / Color(cell).enhance(f)` in the tile's order before it is pasted -- it stores Pillow's
canvases together with the sources, the tiles' parameters and the colour rows (arrays only).  tests/test_color_reference.py holds the numpy restatement
to these bytes, so the pin survives on a machine without Pillow.  (The 330-pixel case is pinned against live Pillow only: its canvases would be 1 MB.)

Run where Pillow is installed:  python tests/golden/make_golden_color.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import color_reference as C  # noqa: E402


def tile_array(tiles):
    """[n,11] float64: src, box (4), flip, b, x0, y0, cw, ch."""
    return np.asarray([[t.src, *t.box, float(t.flip), t.b, t.x0, t.y0, t.cw, t.ch] for t in tiles], dtype=np.float64)


def main():
    import PIL
    src = C.sources()
    out = {"pillow_version": np.asarray([int(v) for v in PIL.__version__.split(".")[:3]]), "size": np.asarray(C.SIZE)}
    for k, im in enumerate(src):
        out[f"src_{k}"] = im
    for name, (tiles, color, n_out, size) in C.cases().items():
        if size != C.SIZE:
            continue
        out[f"tiles_{name}"] = tile_array(tiles)
        out[f"color_{name}"] = np.asarray(color, dtype=np.float32)
        out[f"canvas_{name}"] = C.render_color_pil(src, tiles, color, n_out, size)
    path = os.path.join(HERE, "f16_color.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
