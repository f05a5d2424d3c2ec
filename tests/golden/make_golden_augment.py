"""Reference fixture for train-time augmentation: tests/golden/f12_augment.npz, written from live Pillow.

For every case of tests/augment_reference.cases() -- boxed bicubic resizes of three small uint8 sources into the cells of 24 x 24 canvases, with and
without flip, at mosaic grids 1, 2 and 3 -- it stores what `Image.resize((cw, ch), BICUBIC, box=...)`, `transpose(FLIP_LEFT_RIGHT)` and `paste` produce,
together with the sources and the tiles' parameters (arrays only).  tests/test_augment.py holds the numpy restatement to these bytes, so the pin survives
on a machine without Pillow.

Run where Pillow is installed:  python tests/golden/make_golden_augment.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import augment_reference as R  # noqa: E402


def tile_array(tiles):
    """[n,12] float64: src, box (4), flip, b, x0, y0, cw, ch, 0."""
    return np.asarray([[t.src, *t.box, float(t.flip), t.b, t.x0, t.y0, t.cw, t.ch, 0.0] for t in tiles], dtype=np.float64)


def main():
    import PIL
    src = R.sources()
    out = {"pillow_version": np.asarray([int(v) for v in PIL.__version__.split(".")[:3]]), "size": np.asarray(R.SIZE)}
    for k, im in enumerate(src):
        out[f"src_{k}"] = im
    for name, (tiles, n_out) in R.cases().items():
        out[f"tiles_{name}"] = tile_array(tiles)
        out[f"canvas_{name}"] = R.render_pil(src, tiles, n_out, R.SIZE)
    path = os.path.join(HERE, "f12_augment.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
