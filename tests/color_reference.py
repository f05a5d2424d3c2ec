"""Numpy restatement of the colour half of train-time augmentation, independent of the package (no torch, no PIL at import): Pillow's
`Image.convert("L")` luma, `Image.blend` on uint8 (float32, two roundings), `ImageEnhance.Brightness / Contrast / Color`, applied per tile to the resized
(and flipped) cell of tests/augment_reference.py before it is pasted.  tests/test_color_reference.py pins it against live Pillow and against
tests/golden/f16_color.npz (written from Pillow by tests/golden/make_golden_color.py); the device path is then compared with it bit for bit.

The arithmetic lives in the methods of `Restatement`, so that a test can plant an error in a copy (a subclass) and show that the pins catch it;
the module-level functions are the methods of the one correct instance."""
import itertools

import numpy as np

from tests import augment_reference as A

ORDERS = tuple("".join(p) for p in itertools.permutations("bcs"))        # bcs bsc cbs csb sbc scb: what `order` 0..5 of a colour row indexes

_RESIZED = {}


def resized_cell(images, t):
    """The tile's cell before colour: boxed resize, flip.  Cached (the sources are identified by their bytes): the planted-error checks render every case
    several times and differ only after this point."""
    im = np.asarray(images[t.src])
    key = (im.shape, im.tobytes(), tuple(t.box), t.cw, t.ch, bool(t.flip))
    if key not in _RESIZED:
        cell = A.resize_box_u8(im, t.box, t.cw, t.ch)
        _RESIZED[key] = np.ascontiguousarray(cell[:, ::-1] if t.flip else cell)
    return _RESIZED[key]


class Restatement:
    def luma(self, rgb):
        """u8 [...,3] -> u8 [...]: Image.convert("L")."""
        c = np.asarray(rgb).astype(np.int64)
        return ((19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 0x8000) >> 16).astype(np.uint8)

    def blend_value(self, a, b, f):
        """float32 v = f32(a) + fl32(f32(f) * f32(b - a)): numpy rounds the float32 product and the float32 sum separately."""
        a, b = np.asarray(a).astype(np.int32), np.asarray(b).astype(np.int32)
        return a.astype(np.float32) + np.float32(f) * (b - a).astype(np.float32)

    def to_u8(self, v, f):
        """Blend.c: 0 <= f <= 1 -> (UINT8) v (truncation; v lies in [0, 255]); otherwise v <= 0 -> 0, v >= 255 -> 255, else truncation."""
        t = np.trunc(v)
        if 0.0 <= np.float32(f) <= 1.0:
            return t.astype(np.int64).astype(np.uint8)
        return np.where(v <= 0.0, 0, np.where(v >= 255.0, 255, t)).astype(np.int64).astype(np.uint8)

    def blend_u8(self, a, b, f):
        """Image.blend(A, B, f) on uint8 levels (broadcast)."""
        return self.to_u8(self.blend_value(a, b, f), f)

    def mean_level(self, L):
        """ImageEnhance.Contrast: int(mean(L) + 0.5), in integers."""
        n = int(L.size)
        return (2 * int(np.asarray(L).astype(np.int64).sum()) + n) // (2 * n)

    def contrast_input(self, original, current):
        """The image whose mean luma contrast blends towards: the cell as it is when the op is reached."""
        return current

    def enhance(self, cell, kind, f, m=None):
        """ImageEnhance.{Brightness 'b', Contrast 'c', Color 's'}(cell).enhance(f) on a u8 [h,w,3] cell; `m` overrides contrast's mean level."""
        cell = np.asarray(cell)
        if kind == "b":
            return self.blend_u8(np.zeros_like(cell), cell, f)
        if kind == "s":
            return self.blend_u8(self.luma(cell)[..., None], cell, f)
        if kind == "c":
            return self.blend_u8(self.mean_level(self.luma(cell)) if m is None else m, cell, f)
        raise ValueError(kind)

    def apply_color(self, cell, row, m=None):
        """The tile's three ops in its order; row = (fb, fc, fs, order)."""
        fb, fc, fs, order = row
        factor = {"b": np.float32(fb), "c": np.float32(fc), "s": np.float32(fs)}
        cur = np.asarray(cell)
        for kind in ORDERS[int(order)]:
            if kind == "c" and m is None:
                cur = self.enhance(cur, "c", factor["c"], self.mean_level(self.luma(self.contrast_input(cell, cur))))
            else:
                cur = self.enhance(cur, kind, factor[kind], m)
        return cur

    def tile_means(self, cells, tiles, color):
        """Per tile: an override of contrast's mean level, or None (= the cell's own, taken where the op is reached)."""
        return [None] * len(tiles)

    def render_color(self, images, tiles, color, n_out, size):
        """The augmented canvases u8 [n_out,size,size,3]: resize each tile's box to its cell, flip, colour, paste."""
        canvas = np.zeros((n_out, size, size, 3), dtype=np.uint8)
        cells = [resized_cell(images, t) for t in tiles]
        means = self.tile_means(cells, tiles, color)
        for t, cell, row, m in zip(tiles, cells, np.asarray(color, dtype=np.float32), means):
            canvas[t.b, t.y0:t.y0 + t.ch, t.x0:t.x0 + t.cw] = self.apply_color(cell, row, m)
        return canvas


REF = Restatement()
luma, blend_u8, enhance, apply_color, render_color = REF.luma, REF.blend_u8, REF.enhance, REF.apply_color, REF.render_color


def render_color_pil(images, tiles, color, n_out, size):
    """The same canvases from live Pillow: resize -> [transpose] -> ImageEnhance.X(cell).enhance(f) in the tile's order -> paste."""
    from PIL import Image, ImageEnhance
    op = {"b": ImageEnhance.Brightness, "c": ImageEnhance.Contrast, "s": ImageEnhance.Color}
    canv = [Image.new("RGB", (size, size)) for _ in range(n_out)]
    for t, (fb, fc, fs, order) in zip(tiles, np.asarray(color, dtype=np.float32)):
        cell = Image.fromarray(np.asarray(images[t.src])).resize((t.cw, t.ch), Image.BICUBIC, box=tuple(float(v) for v in t.box))
        if t.flip:
            cell = cell.transpose(Image.FLIP_LEFT_RIGHT)
        factor = {"b": float(fb), "c": float(fc), "s": float(fs)}
        for kind in ORDERS[int(order)]:
            cell = op[kind](cell).enhance(factor[kind])
        canv[t.b].paste(cell, (t.x0, t.y0))
    return np.stack([np.asarray(c) for c in canv])


# ---- the cases shared by the fixture, the CPU tests and the GPU tests -----------------------------------------------------------------------
SIZE = A.SIZE
BIG = 330                                                       # cw = 330 spans two 256-column workgroups, 330 rows = 82 four-row units + 2; cells of 165 and 110
GREY = 100                                                      # the two-level source holds GREY and GREY + 1 in equal number: mean luma GREY + 0.5 exactly


def sources():
    """augment_reference's three sources + a SIZE x SIZE image of two grey levels in equal number (left half GREY, right half GREY + 1)."""
    two = np.full((SIZE, SIZE, 3), GREY, dtype=np.uint8)
    two[:, SIZE // 2:] = GREY + 1
    return A.sources() + [two]


def _rows(*rows):
    return np.asarray(rows, dtype=np.float32).reshape(-1, 4)


def _grid_tiles(rng, b, g, size):
    """g x g cells of output b from random boxes of the three textured sources (edges multiples of 1/8), as augment_reference's 'mixed'."""
    c, out = size // g, []
    for q in range(g * g):
        s = int(rng.integers(3))
        H, W = A.SHAPES[s]
        w, h = rng.integers(8 * 6, 8 * W + 1) / 8.0, rng.integers(8 * 6, 8 * H + 1) / 8.0
        l, u = rng.integers(0, int(8 * (W - w)) + 1) / 8.0, rng.integers(0, int(8 * (H - h)) + 1) / 8.0
        out.append(A.Tile(s, (float(l), float(u), float(l + w), float(u + h)), bool(rng.integers(2)), b, (q % g) * c, (q // g) * c, c, c))
    return out


def cases():
    """name -> (tiles, color f32 [n,4], n_out, size) over `sources()`.

    'single': augment_reference's eight one-tile outputs -- each op alone, below and above 1; saturation 0 (grayscale); brightness 2.5 (the upper clip on
        the bright parts of the ramps); contrast 3 (both clips); the identity row.
    'orders': the same eight geometries (six used), all six orders with three non-trivial factors, contrast below and above 1.
    'mixed': augment_reference's g = 1, 2, 3 outputs, seeded factors in [0, 2]; every third tile without contrast (fc = 1), two with fs = 0 -- tiles with and
        without the contrast sum in one launch, neighbours of one canvas with different factors.
    'twogrey': the identity tile of the two-level source under contrast 0.25 and 0 (output = the mean level itself) and 1.5: mean luma k + 0.5 exactly.
    'big': canvases of 330 at g = 1, 2, 3 from the same small sources: a cell two workgroups wide, a row count that is no multiple of the four-row unit,
        cells of 165 and 110; contrast in every order position, and tiles without it."""
    S = SIZE
    single, n_single = A.cases()["single"]
    mixed, n_mixed = A.cases()["mixed"]
    out = {}
    out["single"] = (single, _rows((1.4, 1, 1, 0), (1, 0.6, 1, 0), (1, 1, 1.875, 0), (1, 1, 0, 3), (2.5, 1, 1, 5), (1, 3, 1, 2), (0.25, 1, 0.5, 4), (1, 1, 1, 0)), n_single, S)
    orders = [single[j]._replace(b=j) for j in range(6)]
    fac = ((1.4, 0.6, 1.875), (0.6, 1.4, 0.25), (1.2, 0.3, 1.5), (0.8, 2.0, 0.9), (1.875, 0.9, 0.1), (0.5, 1.7, 1.3))
    out["orders"] = (orders, _rows(*[f + (j,) for j, f in enumerate(fac)]), 6, S)
    rng = np.random.default_rng(16)
    col = np.empty((len(mixed), 4), dtype=np.float32)
    col[:, :3] = rng.uniform(0.0, 2.0, size=(len(mixed), 3)).astype(np.float32)
    col[:, 3] = rng.integers(6, size=len(mixed))
    col[::3, 1] = 1.0
    col[[4, 9], 2] = 0.0
    out["mixed"] = (mixed, col, n_mixed, S)
    ident = (0.0, 0.0, float(S), float(S))
    out["twogrey"] = ([A.Tile(3, ident, False, 0, 0, 0, S, S), A.Tile(3, ident, True, 1, 0, 0, S, S), A.Tile(3, ident, False, 2, 0, 0, S, S)],
                      _rows((1, 0.25, 1, 0), (1, 0, 1, 2), (1, 1.5, 1, 4)), 3, S)
    rng = np.random.default_rng(33)
    big = [A.Tile(0, (3.25, 2.5, 47.75, 30.125), True, 0, 0, 0, BIG, BIG)] + _grid_tiles(rng, 1, 2, BIG) + _grid_tiles(rng, 2, 3, BIG)
    col = np.empty((len(big), 4), dtype=np.float32)
    col[:, :3] = rng.uniform(0.3, 1.9, size=(len(big), 3)).astype(np.float32)
    col[:, 3] = np.arange(len(big)) % 6
    col[0] = (1.3, 0.7, 1.6, 4)                                 # g = 1: saturation, brightness, then the contrast sum over two workgroup columns
    col[[2, 7, 11], 1] = 1.0
    out["big"] = (big, col, 3, BIG)
    return out


pixel_values = A.pixel_values                                    # u8 [n,S,S,3] -> f32 [n,3,S,S] through the normalisation table
