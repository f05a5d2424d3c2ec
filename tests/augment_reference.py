"""Numpy restatement of what train-time augmentation must compute, independent of the package: Pillow's boxed bicubic resize
(`Image.resize((cw, ch), BICUBIC, box=...)`: float64 tap tables -> 22-bit fixed point, two passes with the u8 round / clamp between them),
`transpose(FLIP_LEFT_RIGHT)`, `paste`, the normalisation table, and the box transform.  tests/test_augment.py pins it against live PIL and against
tests/golden/f12_augment.npz (written from PIL by tests/golden/make_golden_augment.py); the device path is then compared with it bit for bit."""
import math
from collections import namedtuple

import numpy as np

PRECISION_BITS = 32 - 8 - 2

# the fields of owl_vit_object_detection_amd.preprocess.Tile, restated: box = (left, upper, right, lower) of source `src` -> cell (x0, y0, cw, ch) of output `b`
Tile = namedtuple("Tile", "src box flip b x0 y0 cw ch")


def bicubic_filter(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs_box(in_size: int, in0: float, in1: float, out_size: int):
    """Pillow Resample.c precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter -> (bounds int32 [out,2], kk int32 [out,ksize], ksize)."""
    scale = (in1 - in0) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic_filter((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


def _clip8(acc):
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_box_u8(img: np.ndarray, box, cw: int, ch: int) -> np.ndarray:
    """u8 [H,W,3] -> u8 [ch,cw,3]: horizontal pass over the rows the vertical taps read, u8 round / clamp, vertical pass (Resample.c ImagingResample)."""
    H, W = img.shape[:2]
    l, u, r, lo = (float(v) for v in box)
    bx, kx, _ = coeffs_box(W, l, r, cw)
    by, ky, _ = coeffs_box(H, u, lo, ch)
    y_first, y_last = int(by[0, 0]), int(by[-1, 0] + by[-1, 1])
    rows = img[y_first:y_last].astype(np.int64)
    tmp = np.zeros((y_last - y_first, cw, 3), dtype=np.uint8)
    for x in range(cw):
        x0, n = int(bx[x, 0]), int(bx[x, 1])
        acc = (rows[:, x0:x0 + n, :] * kx[x, :n].astype(np.int64)[None, :, None]).sum(axis=1) + (1 << (PRECISION_BITS - 1))
        tmp[:, x] = _clip8(acc)
    out = np.zeros((ch, cw, 3), dtype=np.uint8)
    t64 = tmp.astype(np.int64)
    for y in range(ch):
        y0, n = int(by[y, 0]) - y_first, int(by[y, 1])
        acc = (t64[y0:y0 + n] * ky[y, :n].astype(np.int64)[:, None, None]).sum(axis=0) + (1 << (PRECISION_BITS - 1))
        out[y] = _clip8(acc)
    return out


def render(images, tiles, n_out: int, size: int) -> np.ndarray:
    """The augmented canvases u8 [n_out,size,size,3]: resize each tile's box to its cell, flip, paste."""
    canvas = np.zeros((n_out, size, size, 3), dtype=np.uint8)
    for t in tiles:
        cell = resize_box_u8(np.asarray(images[t.src]), t.box, t.cw, t.ch)
        if t.flip:
            cell = cell[:, ::-1]
        canvas[t.b, t.y0:t.y0 + t.ch, t.x0:t.x0 + t.cw] = cell
    return canvas


def render_pil(images, tiles, n_out: int, size: int) -> np.ndarray:
    """The same canvases from live Pillow."""
    from PIL import Image
    out = []
    canv = [Image.new("RGB", (size, size)) for _ in range(n_out)]
    for t in tiles:
        cell = Image.fromarray(np.asarray(images[t.src])).resize((t.cw, t.ch), Image.BICUBIC, box=tuple(float(v) for v in t.box))
        if t.flip:
            cell = cell.transpose(Image.FLIP_LEFT_RIGHT)
        canv[t.b].paste(cell, (t.x0, t.y0))
    for c in canv:
        out.append(np.asarray(c))
    return np.stack(out)


def normalize_lut(mean=(0.48145466, 0.4578275, 0.40821073), std=(0.26862954, 0.26130258, 0.27577711), rescale_factor=1 / 255) -> np.ndarray:
    """[3,256] f32: transformers' rescale (f64 multiply, f32 cast) + normalize (f32) of each u8 level (HF OwlViTImageProcessor defaults)."""
    v = (np.arange(256, dtype=np.uint8).astype(np.float64) * rescale_factor).astype(np.float32)
    m = np.array(mean, dtype=np.float32)[:, None]
    s = np.array(std, dtype=np.float32)[:, None]
    return ((v[None, :] - m) / s).astype(np.float32)


def pixel_values(canvas: np.ndarray) -> np.ndarray:
    """u8 [n,S,S,3] -> f32 [n,3,S,S] through the table."""
    lut = normalize_lut()
    return np.stack([lut[c][canvas[..., c]] for c in range(3)], axis=1)


def transform_boxes(boxes_xywh, labels, crop, flip, cell, size, min_visibility=0.3, min_box=2.0):
    """One box at a time, plain Python floats (= float64): intersect with the crop, the two drop rules, map into the cell, mirror, normalise."""
    l, u, r, lo = (float(v) for v in crop)
    cx0, cy0, cw, ch = cell
    out, keep = [], []
    for (x, y, w, h), lab in zip(np.asarray(boxes_xywh, dtype=np.float64).reshape(-1, 4).tolist(), np.asarray(labels).reshape(-1).tolist()):
        ix1, iy1, ix2, iy2 = max(x, l), max(y, u), min(x + w, r), min(y + h, lo)
        vw, vh = ix2 - ix1, iy2 - iy1
        if vw <= 0.0 or vh <= 0.0 or w * h <= 0.0:
            continue
        if (vw * vh) / (w * h) < min_visibility:
            continue
        sx, sy = cw / (r - l), ch / (lo - u)
        if vw * sx < min_box or vh * sy < min_box:
            continue
        a, b = (ix1 - l) * sx, (ix2 - l) * sx
        if flip:
            a, b = cw - b, cw - a
        box = [(cx0 + a) / size, (cy0 + (iy1 - u) * sy) / size, (cx0 + b) / size, (cy0 + (iy2 - u) * sy) / size]
        out.append([min(max(v, 0.0), 1.0) for v in box])
        keep.append(lab)
    return np.asarray(out, dtype=np.float64).reshape(-1, 4).astype(np.float32), np.asarray(keep, dtype=np.asarray(labels).dtype)


# ---- the cases shared by the fixture, the CPU tests and the GPU tests -----------------------------------------------------------------------
SIZE = 24
SHAPES = ((37, 53), (64, 48), (20, 31))                     # (H, W)


def sources():
    rng = np.random.default_rng(12)
    out = []
    for H, W in SHAPES:
        # smooth ramp + noise: resampling a pure-noise image saturates the clamp far more often than a photograph does
        yy, xx = np.mgrid[0:H, 0:W]
        base = np.stack([xx * 255.0 / W, yy * 255.0 / H, (xx + yy) * 255.0 / (H + W)], axis=2)
        out.append(np.clip(base + rng.integers(-90, 91, size=(H, W, 3)), 0, 255).astype(np.uint8))
    return out


def cases():
    """name -> (tiles, n_out).  Box edges are multiples of 1/8 (exact in float32, which Pillow's `box=` holds).
    'single': one tile per output -- the identity; fractional edges, plain and flipped; boxes flush with each border (taps clipped to the image); a box whose
    vertical support (rows 18..46 of 64) excludes the first and last source rows; a down-scale with ksize 13; an up-scale.
    'mixed': output 0 at g = 1, output 1 at g = 2, output 2 at g = 3, sources, boxes and flips mixed."""
    S = SIZE
    single = [
        ((0, (0.0, 0.0, 53.0, 37.0), False)),
        ((0, (3.25, 2.5, 47.75, 30.125), False)),
        ((0, (3.25, 2.5, 47.75, 30.125), True)),
        ((1, (0.0, 0.0, 20.5, 33.25), False)),              # flush left and top
        ((1, (17.5, 21.75, 48.0, 64.0), True)),             # flush right and bottom
        ((1, (5.5, 20.0, 40.25, 44.0), False)),             # rows 18..46 only
        ((1, (0.0, 0.0, 48.0, 64.0), True)),                # 64 -> 24: ksize 13
        ((2, (10.0, 5.0, 20.5, 12.5), False)),              # up-scale
    ]
    out = {"single": ([Tile(s, b, f, i, 0, 0, S, S) for i, (s, b, f) in enumerate(single)], len(single))}
    mixed = [Tile(2, (1.125, 0.0, 31.0, 17.375), True, 0, 0, 0, S, S)]
    rng = np.random.default_rng(5)
    for b, g in ((1, 2), (2, 3)):
        c = S // g
        for q in range(g * g):
            s = int(rng.integers(3))
            H, W = SHAPES[s]
            w, h = rng.integers(8 * 6, 8 * W + 1) / 8.0, rng.integers(8 * 6, 8 * H + 1) / 8.0
            l, u = rng.integers(0, int(8 * (W - w)) + 1) / 8.0, rng.integers(0, int(8 * (H - h)) + 1) / 8.0
            mixed.append(Tile(s, (float(l), float(u), float(l + w), float(u + h)), bool(rng.integers(2)), b, (q % g) * c, (q // g) * c, c, c))
    out["mixed"] = (mixed, 3)
    return out
