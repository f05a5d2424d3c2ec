"""Device input pipeline with the call surface the reference uses (ref src/dataset.py:69-71):

    pixel_values = image_processor(images=image, return_tensors="pt")["pixel_values"]

``DeviceImageProcessor`` is the HF ``OwlViTImageProcessor`` (PIL backend: bicubic resize to size x size, no crop,
x(1/255), CLIP mean/std) re-built for the GPU: the u8 image goes to HBM once (0.9 MB for a COCO image instead of
7 MB of f32 pixel_values), two HIP kernels reproduce Pillow's fixed-point separable bicubic bit-for-bit and the
normalisation is a 768-entry table of the reference's own float results.  Output is [B,3,S,S] f32 (the reference's
contract) or bf16 (what the patch-embed loader consumes) on the device.  No CPU fallback: the resize runs in
libowlhip.so or not at all; only Pillow's f64 tap tables are computed on the host (``owl_bicubic_coeffs``), cached
per image size.

``DeviceImageProcessor(size, resize="owlv2")`` is HF's ``Owlv2ImageProcessorPil`` instead (what the ``google/owlv2-*`` checkpoints were trained behind):
x(1/255), pad bottom / right to a square of side S = max(H, W), scipy's Gaussian blur with sigma = max(0, (S/N - 1)/2) and bilinear zoom to N x N (both
"mirror"), normalise.  Blur and zoom are separable and linear and the pad is a constant, so the stage folds into one float tap table per axis
(``owl_pad_resize_coeffs``, host, f64) and the same two passes with float weights and an f32 intermediate (csrc/pad_resize.hip).  Not bit-exact -- HF
itself stores f32 between scipy's passes -- but inside a bound that counts every rounding (tests/owlv2_input_reference.py).  Predictions on such an input
are normalised to the PADDED square: ``postprocess.unpad_boxes`` maps them back, ``pad_square_targets`` maps training targets in.
"""
import math

import numpy as np
import torch

from . import _lib, ops

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)     # HF OPENAI_CLIP_MEAN / OPENAI_CLIP_STD (OwlViTImageProcessor defaults)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def normalize_lut(mean, std, rescale_factor) -> np.ndarray:
    """[3,256] f32 = what transformers' rescale (f64 multiply, f32 cast) + normalize (f32) give for each u8 level."""
    v = (np.arange(256, dtype=np.uint8).astype(np.float64) * rescale_factor).astype(np.float32)
    m = np.array(mean, dtype=np.float32)[:, None]
    s = np.array(std, dtype=np.float32)[:, None]
    return ((v[None, :] - m) / s).astype(np.float32)


def size_hw(size):
    """(H, W) of a `size` given as an int (square) or a pair (height, width)."""
    if isinstance(size, (tuple, list)):
        if len(size) != 2:
            raise ValueError(f"size={size!r}: an int (square) or a pair (height, width)")
        return int(size[0]), int(size[1])
    return int(size), int(size)


def _size_attr(size):
    """What the `size` attribute holds: the int for a square (a square pair included), else the pair (H, W)."""
    H, W = size_hw(size)
    if H < 1 or W < 1:
        raise ValueError(f"size={size!r}: both sides must be positive")
    return H if H == W else (H, W)


PAD_RESIZE_MAX_RATIO = 16   # owl_pad_resize_coeffs: padded side S <= 16 x the model size N (the blur then has at most 62 taps per axis)
_PAD_TAPS = 64              # capacity per output index handed to owl_pad_resize_coeffs

_OWLV2_PLAIN_ONLY = ("{what} is not built for resize=\"owlv2\": crop, flip, mosaic, colour jitter and slices resample with Pillow's bicubic into a "
                     "canvas without a pad, which is not the input an OWLv2 checkpoint expects.  The plain path -- __call__, normalize_sized, "
                     "DevicePrefetcher(processor=) without augment= -- runs in this mode")

_SQUARE_ONLY = ("{what} takes a square size: crop / flip / mosaic canvases, colour jitter and slices are built for S x S model inputs and the size "
                "here is {size} (height, width).  The plain path -- __call__, normalize_sized, DevicePrefetcher without augment= -- runs at a rectangular size")


class DeviceImageProcessor:
    """`size`: the model's input size, an int (square) or a pair (height, width).  The plain path (__call__: Pillow's resize of each image to H x W plus the
    table; normalize_sized) runs at either; the tile paths (run_tiles / tiles / slices) are square only and raise ValueError on a rectangle.

    `resize`: "pillow" (the default: HF's OwlViTImageProcessor, every launch and bit as ever) or "owlv2" (HF's Owlv2ImageProcessorPil: pad bottom / right
    to a square, blur, bilinear zoom -- the module docstring).  In "owlv2" mode `size` must be square (the pad makes a square), an image's longer side may be
    at most PAD_RESIZE_MAX_RATIO x size, and only the plain path runs: run_tiles / tiles / slices raise ValueError.  `pad_value`: the level of the pad in
    pre-normalisation [0, 1] units (a fraction of the u8 range).  HF pads 0.0; other OWLv2 pipelines pad mid-grey, 0.5."""

    def __init__(self, size=768, image_mean=CLIP_MEAN, image_std=CLIP_STD, rescale_factor=1 / 255, device="cuda",
                 dtype=torch.float32, resize="pillow", pad_value=0.0):
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("DeviceImageProcessor: dtype must be torch.float32 or torch.bfloat16")
        if resize not in ("pillow", "owlv2"):
            raise ValueError(f"DeviceImageProcessor: resize={resize!r}: \"pillow\" or \"owlv2\"")
        if resize == "owlv2" and len(set(size_hw(size))) > 1:
            raise ValueError(f"DeviceImageProcessor: resize=\"owlv2\" pads every image to a square and takes a square size; got {tuple(size_hw(size))} (height, width)")
        if not 0.0 <= float(pad_value) <= 1.0:
            raise ValueError(f"DeviceImageProcessor: pad_value={pad_value!r} is in pre-normalisation units: 0 <= pad_value <= 1")
        self.resize = resize
        self.pad_value = float(pad_value)
        self.size = _size_attr(size)         # the int for a square, (H, W) for a rectangle
        self.hw = size_hw(size)
        self.device = torch.device(device)
        self.dtype = dtype
        self.lut = torch.from_numpy(normalize_lut(image_mean, image_std, rescale_factor)).to(self.device)
        self._tables = {}
        self._tmp = None
        self._ws = None                      # partial sums of the colour path (owl_preprocess_color_workspace_bytes)
        # resize="owlv2": one affine step per channel, a_c = rescale / std_c and b_c = -mean_c / std_c, each formed in f64 and rounded once
        m, sd = np.asarray(image_mean, dtype=np.float64), np.asarray(image_std, dtype=np.float64)
        self._norm = torch.from_numpy(np.concatenate([rescale_factor / sd, -m / sd]).astype(np.float32)).to(self.device) if resize == "owlv2" else None
        self._pad_tables = {}
        self._tmp_f32 = None

    def _square(self, what: str):
        if self.resize == "owlv2":
            raise ValueError(_OWLV2_PLAIN_ONLY.format(what=what))
        if isinstance(self.size, tuple):
            raise ValueError(_SQUARE_ONLY.format(what=what, size=self.size))

    def _axis_tables(self, in_size: int, out: int):
        key = (in_size, out)
        if key not in self._tables:
            ksize = int(math.ceil(2.0 * max(in_size / out, 1.0))) * 2 + 1
            bounds = torch.zeros(out * 2, dtype=torch.int32)
            kk = torch.zeros(out * ksize, dtype=torch.int32)
            ks = torch.zeros(1, dtype=torch.int32)
            _lib.call("owl_bicubic_coeffs", in_size, out, bounds, kk, kk.numel(), ks)
            assert int(ks.item()) == ksize
            self._tables[key] = (bounds.to(self.device), kk.to(self.device), ksize)
        return self._tables[key]

    def _pad_axis_tables(self, extent: int, padded: int, out: int):
        """resize="owlv2": the float tap table of one axis of `extent` real pixels inside the padded length -> (bounds int32 [2 out + 1] = {first, count}
        per output then `live`, weights f32 [out ksize + out] = the rows then their sums, ksize, live4), cached on the device."""
        key = (extent, padded, out)
        if key not in self._pad_tables:
            bounds = torch.zeros(out * 2 + 1, dtype=torch.int32)
            w = torch.zeros(out * _PAD_TAPS, dtype=torch.float32)
            wsum = torch.zeros(out, dtype=torch.float32)
            ks = torch.zeros(1, dtype=torch.int32)
            _lib.call("owl_pad_resize_coeffs", extent, padded, out, bounds, w, w.numel(), ks, wsum)
            ksize = int(ks.item())
            has = torch.nonzero(bounds[1:2 * out:2]).reshape(-1)
            live = int(has[-1]) + 1 if has.numel() else 0
            bounds[2 * out] = live
            self._pad_tables[key] = (bounds.to(self.device), torch.cat([w[:out * ksize], wsum]).to(self.device), ksize, (live + 3) // 4 * 4)
        return self._pad_tables[key]

    def _pad_resize_plan(self, imgs):
        """resize="owlv2": the host half of one launch -> (descriptor rows: 10 ints per image, as owl_preprocess_u8_pad_resize reads them; bytes of the
        f32 intermediate; the largest image height).  Raises ValueError, before any table is built, if an image exceeds PAD_RESIZE_MAX_RATIO."""
        N = self.hw[0]
        for im in imgs:
            S = max(int(im.shape[0]), int(im.shape[1]))
            if S > PAD_RESIZE_MAX_RATIO * N:
                raise ValueError(f"DeviceImageProcessor(resize=\"owlv2\"): an image of {int(im.shape[0])} x {int(im.shape[1])} pads to a square of side {S}, more than "
                                 f"{PAD_RESIZE_MAX_RATIO} x the model size {N} = {PAD_RESIZE_MAX_RATIO * N}: the blur would need more than {_PAD_TAPS} taps per "
                                 "pixel and axis.  Downscale such an image first")
        rows, off, max_h = [], 0, 0
        for im in imgs:
            H, W = int(im.shape[0]), int(im.shape[1])
            S = max(H, W)
            bx, wx, ksx, live4 = self._pad_axis_tables(W, S, N)
            by, wy, ksy, _ = self._pad_axis_tables(H, S, N)
            rows.append((im.data_ptr(), H, W, bx.data_ptr(), wx.data_ptr(), ksx, by.data_ptr(), wy.data_ptr(), ksy, off))
            off += (H * live4 * 12 + 255) // 256 * 256           # the horizontal pass's f32 intermediate: H rows of live4 pixels
            max_h = max(max_h, H)
        return rows, off, max_h

    def _call_owlv2(self, imgs):
        """One launch pair for the (ragged) batch: owl_preprocess_u8_pad_resize."""
        n, N = len(imgs), self.hw[0]
        rows, tmp_bytes, max_h = self._pad_resize_plan(imgs)     # (raises before anything is allocated or launched)
        out = torch.empty(n, 3, N, N, dtype=self.dtype, device=self.device)
        if self._tmp_f32 is None or self._tmp_f32.numel() * 4 < tmp_bytes:
            self._tmp_f32 = torch.empty(tmp_bytes // 4, dtype=torch.float32, device=self.device)
        desc_d = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(self.device, non_blocking=True)
        _lib.call("owl_preprocess_u8_pad_resize", ops.stream(), desc_d, n, max_h, self._tmp_f32, self._norm, self.pad_value, out,
                  1 if self.dtype == torch.bfloat16 else 0, N, N)
        self._keep = (imgs, desc_d)          # keep the sources alive until the stream has consumed them
        return {"pixel_values": out}

    def _to_device(self, img):
        if isinstance(img, np.ndarray):
            img = torch.from_numpy(np.ascontiguousarray(img))
        elif not torch.is_tensor(img):                       # PIL.Image without importing PIL here
            img = torch.from_numpy(np.ascontiguousarray(np.asarray(img.convert("RGB") if hasattr(img, "convert") else img)))
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise ValueError(f"DeviceImageProcessor: expected an RGB uint8 [H,W,3] image, got {img.dtype} {tuple(img.shape)}")
        return img.to(self.device, non_blocking=True).contiguous()

    def __call__(self, images, return_tensors="pt", **_):
        single = not isinstance(images, (list, tuple))
        imgs = [self._to_device(im) for im in ([images] if single else list(images))]
        if self.resize == "owlv2":
            return self._call_owlv2(imgs)
        n = len(imgs)
        out_h, out_w = self.hw
        out = torch.empty(n, 3, out_h, out_w, dtype=self.dtype, device=self.device)
        # one launch pair for the whole (ragged) batch: a 10-int64 descriptor per image
        rows, off, max_h = [], 0, 0
        for im in imgs:
            H, W = int(im.shape[0]), int(im.shape[1])
            bx, kx, ksx = self._axis_tables(W, out_w)
            by, ky, ksy = self._axis_tables(H, out_h)
            rows.append((im.data_ptr(), H, W, bx.data_ptr(), kx.data_ptr(), ksx, by.data_ptr(), ky.data_ptr(), ksy, off))
            off += (H * out_w * 3 + 255) // 256 * 256          # the horizontal pass's u8 intermediate: the image's H rows of out_w pixels
            max_h = max(max_h, H)
        if self._tmp is None or self._tmp.numel() < off:
            self._tmp = torch.empty(off, dtype=torch.uint8, device=self.device)
        desc_d = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(self.device, non_blocking=True)
        _lib.call("owl_preprocess_u8_batch", ops.stream(), desc_d, n, max_h, self._tmp, self.lut, out,
                  1 if self.dtype == torch.bfloat16 else 0, out_h, out_w)
        self._keep = (imgs, desc_d)          # keep the sources alive until the stream has consumed them
        return {"pixel_values": out}

    def run_tiles(self, desc_d: torch.Tensor, n_tiles: int, max_rows: int, tmp_bytes: int, n_out: int, color=None) -> torch.Tensor:
        """Launch owl_preprocess_u8_tiles on the current stream for descriptors that are already on the device with absolute addresses (`build_tile_tables` +
        `resolve_tile_descs`) and whose cover the caller has checked (`check_tile_cover`) -> [n_out,3,S,S] self.dtype.  `color`: a DEVICE f32 [n_tiles,4] array of
        (fb, fc, fs, order) rows the caller has checked (`check_color`) -> owl_preprocess_u8_tiles_color instead; None: the plain launch pair, as ever."""
        self._square("DeviceImageProcessor.run_tiles")
        if self._tmp is None or self._tmp.numel() < tmp_bytes:
            self._tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=self.device)
        out = torch.empty(n_out, 3, self.size, self.size, dtype=self.dtype, device=self.device)
        if color is None:
            _lib.call("owl_preprocess_u8_tiles", ops.stream(), desc_d, n_tiles, max_rows, self._tmp, self.lut, out,
                      1 if self.dtype == torch.bfloat16 else 0, n_out, self.size, self.size)
            return out
        if not (torch.is_tensor(color) and color.is_cuda and color.dtype == torch.float32 and tuple(color.shape) == (n_tiles, 4) and color.is_contiguous()):
            raise ValueError(f"run_tiles: color must be a contiguous device float32 [{n_tiles},4] tensor")
        need = color_workspace_bytes(n_tiles, self.size)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        _lib.call("owl_preprocess_u8_tiles_color", ops.stream(), desc_d, color, n_tiles, max_rows, self._tmp, self._ws, self._ws.numel(), self.lut, out,
                  1 if self.dtype == torch.bfloat16 else 0, n_out, self.size, self.size)
        return out

    def tiles(self, images, tiles, n_out: int, color=None) -> torch.Tensor:
        """The augmenting form of __call__: every `Tile` resamples a source box of `images[tile.src]` into a cell of output image `tile.b`, flipped or not --
        Pillow's `resize((cw, ch), BICUBIC, box=...)`, `transpose(FLIP_LEFT_RIGHT)` and `paste`, bit for bit, in one launch pair.  Raises ValueError unless
        the cells of every output image cover it exactly.  `color` (host, [n_tiles,4] rows of (fb, fc, fs, order): `ColorJitter.sample`, `check_color`) puts
        Pillow's `ImageEnhance.Brightness / Contrast / Color` on each resized cell, in the row's order, between the resize and the table."""
        self._square("DeviceImageProcessor.tiles")
        imgs = [self._to_device(im) for im in images]
        shapes = [(int(im.shape[0]), int(im.shape[1])) for im in imgs]
        tiles = list(tiles)
        check_tile_cover(tiles, n_out, self.size, shapes)
        color_d = None
        if color is not None:
            color_d = torch.from_numpy(check_color(color, len(tiles))).to(self.device, non_blocking=True)
        desc, arena, tmp_bytes, max_rows = build_tile_tables(shapes, tiles)
        arena_d = torch.from_numpy(arena).to(self.device, non_blocking=True)
        resolve_tile_descs(desc, [im.data_ptr() for im in imgs], arena_d.data_ptr())
        desc_d = torch.from_numpy(desc).to(self.device, non_blocking=True)
        out = self.run_tiles(desc_d, len(tiles), max_rows, tmp_bytes, n_out, color=color_d)
        self._keep = (imgs, arena_d, desc_d, color_d)          # keep the sources and tables alive until the stream has consumed them
        return out

    def slices(self, images, slice_size=None, overlap=0.2, full_image=True):
        """Sliced inference's input: every window of `slice_plan` resampled to one size x size canvas -> (pixel_values [T,3,S,S], plan).  A slice is a tile
        whose cell is the whole canvas, so this is `tiles()` unchanged and each canvas is Pillow's `resize((S, S), BICUBIC, box=window)` followed by the
        table.  `slice_size=None`: windows of the processor's own size (one model pixel per source pixel)."""
        self._square("DeviceImageProcessor.slices")
        imgs = [self._to_device(im) for im in (list(images) if isinstance(images, (list, tuple)) else [images])]
        shapes = [(int(im.shape[0]), int(im.shape[1])) for im in imgs]
        plan = slice_plan(shapes, self.size if slice_size is None else slice_size, overlap, full_image, size=self.size)
        return self.tiles(imgs, plan.tiles, len(plan.tiles)), plan

    def normalize_sized(self, src_u8: torch.Tensor, chw: bool) -> torch.Tensor:
        """Images that already have the model's size: u8 [B,S,S,3] (chw=False) or [B,3,S,S] (chw=True) ON THE DEVICE -> [B,3,S,S] self.dtype.  Pillow's resize to
        the size an image already has is a copy, so only the table step of the reference pipeline is left (owl_normalize_u8)."""
        if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or not src_u8.is_cuda:
            raise ValueError(f"normalize_sized: expected a device uint8 [B,S,S,3] / [B,3,S,S] tensor, got {src_u8.dtype} {tuple(src_u8.shape)} on {src_u8.device}")
        n = int(src_u8.shape[0])
        H, W_ = (int(src_u8.shape[2]), int(src_u8.shape[3])) if chw else (int(src_u8.shape[1]), int(src_u8.shape[2]))
        if (int(src_u8.shape[1]) if chw else int(src_u8.shape[3])) != 3 or (H, W_) != self.hw:
            raise ValueError(f"normalize_sized: expected {self.hw[0]} x {self.hw[1]} RGB images, got {tuple(src_u8.shape)} (chw={chw})")
        src_u8 = src_u8.contiguous()
        out = torch.empty(n, 3, H, W_, dtype=self.dtype, device=self.device)
        _lib.call("owl_normalize_u8", ops.stream(), src_u8, 1 if chw else 0, self.lut, out, 1 if self.dtype == torch.bfloat16 else 0, n, H, W_)
        return out


def pad_square_targets(boxes_xyxy_norm, sizes):
    """Training targets for a resize="owlv2" input: normalised xyxy boxes in the frame of the IMAGE -> the frame of the padded square the model sees
    (x * W / S, y * H / S with S = max(H, W); the image sits at the top left, so nothing shifts).  boxes [..., n, 4] with `sizes` [..., 2] = (height, width)
    per leading index, or boxes [n, 4] with one (height, width).  Torch ops on the boxes' device, no sync; the inverse of
    postprocess.unpad_boxes(to="normalized")."""
    sizes = torch.as_tensor(sizes, device=boxes_xyxy_norm.device).double()
    h, w = sizes[..., 0], sizes[..., 1]
    s = torch.maximum(h, w)
    fx, fy = w / s, h / s
    # (formed in float64 and rounded once, so that unpad_boxes(to="normalized") of the result is the input to 1 ulp)
    return (boxes_xyxy_norm.double() * torch.stack([fx, fy, fx, fy], dim=-1).unsqueeze(-2)).to(boxes_xyxy_norm.dtype)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Train-time augmentation (random crop, horizontal flip, mosaic) folded into the device resampler.  Every augmentation that changes scale is a
# resample, and a g x g mosaic needs g^2 of them per output image: done in DataLoader workers that is exactly the CPU work the device resize took
# off the host.  Here the host only draws the parameters and builds Pillow's tap tables for the crop boxes (`owl_bicubic_coeffs_box`); crop, flip and
# placement ride in the two resize passes (`owl_preprocess_u8_tiles`), one interpolation per source pixel, bit-exact against
# `Image.resize(cell, BICUBIC, box=crop)` / `transpose(FLIP_LEFT_RIGHT)` / `paste`.
# ---------------------------------------------------------------------------------------------------------------------------------------
from collections import namedtuple

# one resample: the box (left, upper, right, lower -- float pixel edges, as Pillow's `box=`) of source image `src` -> the cw x ch cell at (x0, y0) of output
# image `b`, mirrored left-right if `flip`
Tile = namedtuple("Tile", "src box flip b x0 y0 cw ch")

TILE_DESC_WORDS = 18           # int64 words per tile descriptor (csrc/preprocess.hip: struct TileDesc)


def check_tile_cover(tiles, n_out: int, size: int, shapes=None):
    """Raises ValueError unless the cells of every output image 0..n_out-1 lie inside the size x size canvas, do not overlap and cover it -- the kernels write
    each output pixel from exactly one tile and leave no pixel unwritten only then -- and (given the sources' (H, W) `shapes`) every box lies inside its source."""
    if not tiles:
        raise ValueError("tiles: empty tile list")
    a = np.asarray([(t.b, t.x0, t.y0, t.cw, t.ch) for t in tiles], dtype=np.int64)
    b, x0, y0, cw, ch = a.T
    if (b < 0).any() or (b >= n_out).any():
        raise ValueError(f"tiles: output index outside [0, {n_out})")
    if (cw <= 0).any() or (ch <= 0).any() or (x0 < 0).any() or (y0 < 0).any() or (x0 + cw > size).any() or (y0 + ch > size).any():
        raise ValueError(f"tiles: a cell lies outside the {size} x {size} canvas")
    area = np.bincount(b, weights=(cw * ch).astype(np.float64), minlength=n_out)
    if (area != float(size * size)).any():
        raise ValueError(f"tiles: the cells of output image {int(np.flatnonzero(area != float(size * size))[0])} do not cover the canvas exactly")
    for i in range(n_out):                                   # inside + total area = canvas: an exact cover unless two cells overlap
        m = np.flatnonzero(b == i)
        if m.size > 1:
            ox = (x0[m, None] < (x0 + cw)[None, m]) & (x0[None, m] < (x0 + cw)[m, None])
            oy = (y0[m, None] < (y0 + ch)[None, m]) & (y0[None, m] < (y0 + ch)[m, None])
            if int((ox & oy).sum()) != m.size:               # (every cell overlaps itself)
                raise ValueError(f"tiles: cells of output image {i} overlap")
    if shapes is not None:
        src = np.asarray([t.src for t in tiles], dtype=np.int64)
        if (src < 0).any() or (src >= len(shapes)).any():
            raise ValueError(f"tiles: source index outside the batch of {len(shapes)}")
        hw = np.asarray(shapes, dtype=np.float64).reshape(-1, 2)[src]
        l, u, r, lo = np.asarray([t.box for t in tiles], dtype=np.float64).reshape(-1, 4).T
        bad = ~((0.0 <= l) & (l < r) & (r <= hw[:, 1]) & (0.0 <= u) & (u < lo) & (lo <= hw[:, 0]))           # (written so that a NaN edge fails)
        if bad.any():
            t = tiles[int(np.flatnonzero(bad)[0])]
            raise ValueError(f"tiles: box {tuple(t.box)} is empty or outside its {shapes[t.src][1]} x {shapes[t.src][0]} source")


# ---------------------------------------------------------------------------------------------------------------------------------------
# Sliced inference: the slice grid.  A large image is cut into overlapping windows, each window becomes one full-resolution model input (a tile whose
# cell is the whole canvas), and the per-slice detections are mapped back with `xform` and merged on the device (csrc/slice_merge.hip,
# postprocess.SlicedPostProcess).  Pure numpy: nothing here needs a GPU.
# ---------------------------------------------------------------------------------------------------------------------------------------
SlicePlan = namedtuple("SlicePlan", "tiles slice_offsets xform shapes")


def slice_starts(n: int, s: int, overlap: float):
    """The (lo, hi) windows of one axis of length n: the single window (0, n) if n <= s; else windows of length s every s - int(s * overlap), the first one
    that would pass n replaced by (n - s, n), which ends the list (so the last window is flush with the axis and overlaps its neighbour at least as much).
    A window that ends exactly at n ends the list too: no window is cut twice."""
    n, s = int(n), int(s)
    if n <= 0 or s <= 0:
        raise ValueError(f"slice_starts: need n > 0 and s > 0 (n={n} s={s})")
    if n <= s:
        return [(0, n)]
    step = s - int(s * overlap)
    if not 1 <= step <= s:
        raise ValueError(f"slice_starts: overlap {overlap} of a window of {s} leaves a step of {step}; need 1 <= step <= {s}")
    out, p = [], 0
    while p + s <= n:
        out.append((p, p + s))
        if p + s == n:
            return out
        p += step
    out.append((n - s, n))
    return out


def slice_plan(shapes, slice_size, overlap=0.2, full_image=True, size=None):
    """shapes: the sources' (H, W).  Per source the row-major product of its two axes' `slice_starts` windows as boxes (left, upper, right, lower), plus --
    with `full_image` and more than one window -- the whole image as one more slice (what finds the objects larger than a window).  -> SlicePlan(
    tiles: one Tile(src, box, False, t, 0, 0, S, S) per slice (S = `size`, default slice_size); slice_offsets int32 [G + 1], a CSR over the sources;
    xform float32 [T, 4] rows (sx, ox, sy, oy) = ((right - left) / W, left / W, (lower - upper) / H, upper / H), each quotient formed in float64 and rounded
    once: a slice's normalised box maps into its source as x = ox + bx * sx, y = oy + by * sy; shapes)."""
    S = int(slice_size if size is None else size)
    shapes = [(int(h), int(w)) for h, w in shapes]
    tiles, offs, xf = [], [0], []
    for g, (H, W) in enumerate(shapes):
        boxes = [(l, u, r, lo) for (u, lo) in slice_starts(H, slice_size, overlap) for (l, r) in slice_starts(W, slice_size, overlap)]
        if full_image and len(boxes) > 1:
            boxes.append((0, 0, W, H))
        for (l, u, r, lo) in boxes:
            tiles.append(Tile(g, (l, u, r, lo), False, len(tiles), 0, 0, S, S))
            xf.append(((r - l) / W, l / W, (lo - u) / H, u / H))
        offs.append(len(tiles))
    return SlicePlan(tiles, np.asarray(offs, dtype=np.int32), np.asarray(xf, dtype=np.float64).reshape(-1, 4).astype(np.float32), shapes)


def _ksize(extent: float, out: int) -> int:
    return int(math.ceil(2.0 * max(extent / out, 1.0))) * 2 + 1          # Pillow's ksize for the bicubic filter (support 2)


def _table_calls(jobs):
    """jobs: (in_size, in0, in1, out_size, bounds address, kk address, kk capacity, expected ksize).  ctypes releases the GIL for the duration of each call."""
    fn = _lib.load().owl_bicubic_coeffs_box
    got = np.zeros(1, dtype=np.int32)
    pgot = got.ctypes.data
    for n_in, in0, in1, n_out, pb, pk, cap, ks in jobs:
        if fn(n_in, in0, in1, n_out, pb, pk, cap, pgot) != 0:
            raise _lib.OwlLibError(f"owl_bicubic_coeffs_box failed: {_lib.last_error()}")
        assert got[0] == ks


def build_tile_tables(shapes, tiles):
    """Host half of the tile path: Pillow's tap tables of every tile's two axes (`owl_bicubic_coeffs_box`), packed in one int32 arena, and the descriptors with
    RELATIVE addresses -- source = index into the batch, tables = byte offsets into the arena -- because the device addresses exist only once the staging slab
    has been allocated (`resolve_tile_descs`).  -> (desc int64 [n,18], arena int32, tmp bytes, max rows)."""
    n = len(tiles)
    hw = np.asarray([shapes[t.src] for t in tiles], dtype=np.int64).reshape(n, 2)
    box = np.asarray([t.box for t in tiles], dtype=np.float64).reshape(n, 4)
    cw = np.asarray([t.cw for t in tiles], dtype=np.int64)
    ch = np.asarray([t.ch for t in tiles], dtype=np.int64)
    ksx = np.asarray([_ksize(b[2] - b[0], w) for b, w in zip(box.tolist(), cw.tolist())], dtype=np.int64)
    ksy = np.asarray([_ksize(b[3] - b[1], h) for b, h in zip(box.tolist(), ch.tolist())], dtype=np.int64)
    sizes = np.stack([2 * cw, cw * ksx, 2 * ch, ch * ksy], axis=1)                  # ints of bx, kx, by, ky per tile
    ends = np.cumsum(sizes.reshape(-1)).reshape(n, 4)
    offs = ends - sizes                                                             # int32 offsets into the arena
    arena = np.zeros(int(ends[-1, -1]), dtype=np.int32)
    addr = arena.ctypes.data + 4 * offs
    jobs = []
    for i in range(n):
        H, W = hw[i].tolist()
        l, u, r, lo = box[i].tolist()
        pbx, pkx, pby, pky = addr[i].tolist()
        jobs.append((W, l, r, int(cw[i]), pbx, pkx, int(sizes[i, 1]), int(ksx[i])))
        jobs.append((H, u, lo, int(ch[i]), pby, pky, int(sizes[i, 3]), int(ksy[i])))
    _table_calls(jobs)
    y_first = arena[offs[:, 2]].astype(np.int64)
    n_rows = arena[offs[:, 2] + 2 * ch - 2].astype(np.int64) + arena[offs[:, 2] + 2 * ch - 1] - y_first
    tmp_sizes = (n_rows * cw * 3 + 255) // 256 * 256
    desc = np.zeros((n, TILE_DESC_WORDS), dtype=np.int64)
    desc[:, 0] = [t.src for t in tiles]
    desc[:, 1:3] = hw
    desc[:, 3], desc[:, 4], desc[:, 5] = 4 * offs[:, 0], 4 * offs[:, 1], ksx
    desc[:, 6], desc[:, 7], desc[:, 8] = 4 * offs[:, 2], 4 * offs[:, 3], ksy
    desc[:, 9], desc[:, 10], desc[:, 11] = y_first, n_rows, np.cumsum(tmp_sizes) - tmp_sizes
    desc[:, 12] = [t.b for t in tiles]
    desc[:, 13] = [t.x0 for t in tiles]
    desc[:, 14] = [t.y0 for t in tiles]
    desc[:, 15], desc[:, 16] = cw, ch
    desc[:, 17] = [1 if t.flip else 0 for t in tiles]
    return desc, arena, int(tmp_sizes.sum()), int(n_rows.max())


def resolve_tile_descs(desc: np.ndarray, src_ptrs, arena_ptr: int):
    """In place: source indices -> device addresses of the sources, arena offsets -> device addresses of the tables."""
    desc[:, 0] = np.asarray(src_ptrs, dtype=np.int64)[desc[:, 0]]
    desc[:, [3, 4, 6, 7]] += np.int64(arena_ptr)


def transform_boxes(boxes_xywh, labels, crop, flip, cell, size, min_visibility=0.3, min_box=2.0, drop=True, return_mask=False):
    """COCO `xywh` pixel boxes of a source -> the boxes of its tile, float64 numpy on the host: intersect with the crop (left, upper, right, lower); drop a box
    whose visible area / original area < `min_visibility` or one of whose visible sides, measured in canvas pixels, is below `min_box`; map into the cell
    (x0, y0, cw, ch) of the size x size canvas, mirrored about the cell's vertical axis under `flip`.  -> (normalised xyxy in [0, 1] float32 [k,4], labels [k])
    -- the form `train_util.coco_to_model_input` returns.  `crop`, `flip` and `cell` are one tile's, or arrays with a row per box (the boxes of several tiles
    in one call).  drop=False keeps every box with a non-empty intersection (the sampler's last resort); return_mask=True appends the mask of kept boxes."""
    bx = np.asarray(boxes_xywh, dtype=np.float64).reshape(-1, 4)
    lb = np.asarray(labels).reshape(-1)
    c = np.asarray(crop, dtype=np.float64)
    l, u, r, lo = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    ce = np.asarray(cell, dtype=np.float64)
    cx0, cy0, cw, ch = ce[..., 0], ce[..., 1], ce[..., 2], ce[..., 3]
    x1, y1, x2, y2 = bx[:, 0], bx[:, 1], bx[:, 0] + bx[:, 2], bx[:, 1] + bx[:, 3]
    ix1, iy1, ix2, iy2 = np.maximum(x1, l), np.maximum(y1, u), np.minimum(x2, r), np.minimum(y2, lo)
    vw, vh = np.maximum(ix2 - ix1, 0.0), np.maximum(iy2 - iy1, 0.0)
    sx, sy = cw / (r - l), ch / (lo - u)                       # canvas pixels per source pixel
    keep = (vw > 0.0) & (vh > 0.0)
    if drop:
        area = bx[:, 2] * bx[:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            keep &= ~((vw * vh) / area < min_visibility) & (area > 0.0)
        keep &= ~(vw * sx < min_box) & ~(vh * sy < min_box)
    ux1, ux2 = (ix1 - l) * sx, (ix2 - l) * sx
    f = np.asarray(flip, dtype=bool)
    ux1, ux2 = np.where(f, cw - ux2, ux1), np.where(f, cw - ux1, ux2)
    out = np.stack([(cx0 + ux1) / size, (cy0 + (iy1 - u) * sy) / size, (cx0 + ux2) / size, (cy0 + (iy2 - u) * sy) / size], axis=1)
    res = (np.clip(out[keep], 0.0, 1.0).astype(np.float32), lb[keep])
    return res + (keep,) if return_mask else res


# ---------------------------------------------------------------------------------------------------------------------------------------
# The photometric half: brightness, contrast, saturation and random grayscale, per TILE, on the resized cell (csrc/color_jitter.hip) -- Pillow's
# `ImageEnhance.Brightness / Contrast / Color(cell).enhance(f)`, bit for bit (what torchvision's PIL path calls for `adjust_brightness / contrast /
# saturation`).  No hue: Pillow's RGB <-> HSV round trip is not pinned.  The host only draws the factors.
# ---------------------------------------------------------------------------------------------------------------------------------------
COLOR_ORDERS = ("bcs", "bsc", "cbs", "csb", "sbc", "scb")     # itertools.permutations("bcs"), lexicographic: what `order` 0..5 of a colour row indexes


def check_color(color, n_tiles: int) -> np.ndarray:
    """-> `color` as a contiguous float32 [n_tiles,4] array of (fb, fc, fs, order) rows; raises ValueError unless every value is finite, every factor >= 0
    and every order one of 0..5."""
    try:
        c = np.ascontiguousarray(np.asarray(color, dtype=np.float32))
    except (TypeError, ValueError) as e:
        raise ValueError(f"color: expected a float [n_tiles,4] array ({e})") from None
    if c.shape != (int(n_tiles), 4):
        raise ValueError(f"color: expected shape ({int(n_tiles)}, 4) = a (brightness, contrast, saturation, order) row per tile, got {c.shape}")
    if not np.isfinite(c).all():
        raise ValueError("color: non-finite value")
    if (c[:, :3] < 0).any():
        raise ValueError("color: factors must be >= 0")
    if not np.isin(c[:, 3], np.arange(6, dtype=np.float32)).all():
        raise ValueError("color: order must be one of 0..5 (itertools.permutations('bcs'))")
    return c


def color_workspace_bytes(n_tiles: int, size: int) -> int:
    """Bytes of device workspace owl_preprocess_u8_tiles_color needs for `n_tiles` tiles of size x size canvases (asked of the library)."""
    got = np.zeros(1, dtype=np.int64)
    _lib.call("owl_preprocess_color_workspace_bytes", int(n_tiles), int(size), int(size), got.ctypes.data)
    return int(got[0])


class ColorJitter:
    """Deterministic host-side sampler of per-tile colour factors: `TrainAugment(size, color=ColorJitter(0.4, 0.4, 0.4, gray=0.1))`.

    `brightness`, `contrast`, `saturation`: a strength x >= 0 = a factor uniform in [max(0, 1 - x), 1 + x] (torchvision's convention), or an explicit
    (lo, hi) range with 0 <= lo <= hi.  `gray`: the probability that a tile's saturation factor becomes 0 (Pillow's `convert("L")` in all three channels).
    `p`: the probability that a tile is jittered at all; the others get the identity row.  The three ops are applied in a random one of their six orders.

    `sample(n_tiles, key)` draws from `numpy.random.default_rng((*key, 1))`, key = (seed, rank, epoch, index) -- a stream of its own beside
    `TrainAugment.sample`'s, so turning colour on changes no tile, box or label.  The six arrays (brightness, contrast, saturation, order, gray, p) are
    ALWAYS drawn, each for all tiles, in that sequence, whatever the strengths: changing one strength never shifts another op's draws."""

    def __init__(self, brightness=0.0, contrast=0.0, saturation=0.0, gray=0.0, p=1.0):
        self.brightness = self._range("brightness", brightness)
        self.contrast = self._range("contrast", contrast)
        self.saturation = self._range("saturation", saturation)
        self.gray, self.p = float(gray), float(p)
        if not (0.0 <= self.gray <= 1.0 and 0.0 <= self.p <= 1.0):
            raise ValueError("ColorJitter: gray and p are probabilities in [0, 1]")

    @staticmethod
    def _range(name, x):
        if isinstance(x, (tuple, list)):
            if len(x) != 2:
                raise ValueError(f"ColorJitter: {name} must be a strength or a (lo, hi) range")
            lo, hi = float(x[0]), float(x[1])
        else:
            x = float(x)
            if not x >= 0.0:
                raise ValueError(f"ColorJitter: {name} strength must be >= 0")
            lo, hi = max(0.0, 1.0 - x), 1.0 + x
        if not (0.0 <= lo <= hi and math.isfinite(hi)):
            raise ValueError(f"ColorJitter: {name} needs 0 <= lo <= hi, got ({lo}, {hi})")
        return lo, hi

    def sample(self, n_tiles: int, key) -> np.ndarray:
        """-> float32 [n_tiles,4] rows of (fb, fc, fs, order), factors rounded to float32 here (the kernel and Pillow take them as they are)."""
        n = int(n_tiles)
        rng = np.random.default_rng(tuple(int(k) for k in key) + (1,))
        u = [rng.random(n) for _ in range(3)]                                     # brightness, contrast, saturation
        order = rng.integers(6, size=n)
        u_gray, u_p = rng.random(n), rng.random(n)
        out = np.empty((n, 4), dtype=np.float32)
        for k, (lo, hi) in enumerate((self.brightness, self.contrast, self.saturation)):
            out[:, k] = np.minimum(lo + u[k] * (hi - lo), hi).astype(np.float32)
        out[u_gray < self.gray, 2] = 0.0
        out[:, 3] = order
        out[~(u_p < self.p)] = 1.0                                                 # the identity row (the order of three unit factors is immaterial)
        return out


class TrainAugment:
    """Deterministic host-side sampler of train-time crops, flips and mosaics, plus the box transform; the pixels are produced on the device by
    `DevicePrefetcher(..., augment=TrainAugment(size))` (or `DeviceImageProcessor.tiles`).

    Per output image `j` of a batch it draws a grid `g` from `mosaic` (g x g cells of size/g pixels; `size % g == 0`), and per cell a source image of the
    same batch (cell 0: image `j` itself; the others without replacement among the other images where the batch has enough, with replacement otherwise), a crop
    box -- area fraction uniform in `scale`, aspect log-uniform in `ratio` RELATIVE to the source's own aspect (the plain pipeline already maps every image to
    a square), placed uniformly inside the image, float edges rounded to float32 (what Pillow's `box=` holds) -- and a flip with probability `hflip`.
    All draws of batch `index` of epoch `epoch` come from `numpy.random.default_rng((seed, rank, epoch, index))`: the same key gives the same batch bit for bit,
    ranks differ, nothing depends on thread timing.

    Targets: `sample` takes the sources' COCO `xywh` PIXEL boxes and returns, per output image, NORMALISED `xyxy` float32 boxes in [0, 1] and their labels
    (`transform_boxes`) -- the form `coco_to_model_input` returns, so the caller SKIPS that function for augmented batches.  `PackedTargets` needs at least one
    box per image: an output image left without one is redrawn up to `max_tries` times, then falls back to its whole, unflipped source at g = 1 with every box
    kept; `fallbacks` counts those.

    `color=ColorJitter(...)` adds per-tile brightness / contrast / saturation / grayscale on the resized cells: `sample_color(n_tiles, epoch, index)` draws the
    tiles' (fb, fc, fs, order) rows from a stream of its own under the same key, so `sample` returns the same tiles, boxes and labels with colour on or off."""

    def __init__(self, size, *, mosaic=(1,), scale=(0.3, 1.0), ratio=(3 / 4, 4 / 3), hflip=0.5, min_visibility=0.3, min_box=2.0, seed=0, rank=0, max_tries=10,
                 color=None):
        if isinstance(size, (tuple, list)) and len(set(size_hw(size))) > 1:
            raise ValueError(_SQUARE_ONLY.format(what="TrainAugment", size=tuple(size)))
        self.size = _size_attr(size)
        self.mosaic = tuple(int(g) for g in mosaic)
        if not self.mosaic or any(g < 1 or self.size % g for g in self.mosaic):
            raise ValueError(f"TrainAugment: every mosaic grid must be >= 1 and divide size = {self.size}, got {mosaic}")
        self.scale = (float(scale[0]), float(scale[1]))
        self.ratio = (float(ratio[0]), float(ratio[1]))
        if not 0.0 < self.scale[0] <= self.scale[1] <= 1.0 or not 0.0 < self.ratio[0] <= self.ratio[1]:
            raise ValueError("TrainAugment: need 0 < scale[0] <= scale[1] <= 1 and 0 < ratio[0] <= ratio[1]")
        self.hflip = float(hflip)
        self.min_visibility = float(min_visibility)
        self.min_box = float(min_box)
        self.seed, self.rank, self.max_tries = int(seed), int(rank), int(max_tries)
        self.fallbacks = 0
        if color is not None and not hasattr(color, "sample"):
            raise TypeError("TrainAugment: color must be a ColorJitter (or None)")
        self.color = color

    def sample_color(self, n_tiles, epoch, index):
        """The colour rows of the `n_tiles` tiles `sample` returned for batch `index` of epoch `epoch` -> float32 [n_tiles,4], or None without `color`."""
        if self.color is None:
            return None
        return check_color(self.color.sample(n_tiles, (self.seed, self.rank, int(epoch), int(index))), n_tiles)

    def _crops(self, rng, H, W):
        """One crop per entry of the float64 arrays H, W -> [n,4] (left, upper, right, lower)."""
        n = len(H)
        area = rng.uniform(self.scale[0], self.scale[1], n)
        r = np.exp(rng.uniform(math.log(self.ratio[0]), math.log(self.ratio[1]), n))
        w, h = np.minimum(W * np.sqrt(area * r), W), np.minimum(H * np.sqrt(area / r), H)
        l, u = rng.uniform(0.0, 1.0, n) * (W - w), rng.uniform(0.0, 1.0, n) * (H - h)
        box = np.stack([l, u, l + w, u + h], axis=1).astype(np.float32).astype(np.float64)
        box[:, 2], box[:, 3] = np.minimum(box[:, 2], W), np.minimum(box[:, 3], H)         # (float32 rounding may step over the border)
        bad = (box[:, 2] - box[:, 0] < 1.0) | (box[:, 3] - box[:, 1] < 1.0)                # an image too small for the draw: take it whole
        box[bad] = np.stack([0.0 * W, 0.0 * H, W, H], axis=1)[bad]
        return box

    def _draw(self, rng, J, hw, allb, alll, first, count):
        """One draw for each output image of the index array J, vectorised over all their cells -> per-tile arrays (output image, source, box [T,4], flip,
        cell [T,4]) and the surviving targets (output image of each, boxes, labels), ordered by output image, then cell, then source box."""
        B, S = len(hw), self.size
        g = np.asarray(self.mosaic, dtype=np.int64)[rng.integers(len(self.mosaic), size=len(J))]
        n = g * g
        T = int(n.sum())
        row = np.repeat(np.arange(len(J)), n)                                    # which entry of J a tile belongs to
        q = np.arange(T) - np.repeat(np.cumsum(n) - n, n)                       # its cell within the grid
        out = J[row]
        # sources: cell 0 is the image itself; the others walk a random order of the other images (no repeats) where the batch has enough of them
        order = np.argsort(rng.random((len(J), max(B - 1, 1))), axis=1)
        others = order + (order >= J[:, None])
        src = np.where(q == 0, out, others[row, np.minimum(np.maximum(q - 1, 0), max(B - 2, 0))]) if B > 1 else out.copy()
        again = rng.integers(B, size=T)
        short = (np.repeat(n, n) - 1 > B - 1) & (q > 0)                         # a grid with more cells than the batch has other images: with replacement
        src = np.where(short, again, src)
        box = self._crops(rng, hw[src, 0], hw[src, 1])
        flip = rng.random(T) < self.hflip
        c = S // np.repeat(g, n)
        cell = np.stack([(q % np.repeat(g, n)) * c, (q // np.repeat(g, n)) * c, c, c], axis=1)
        cnt = count[src]
        per = np.repeat(np.arange(T), cnt)                                       # the tile of every candidate box
        idx = first[src][per] + np.arange(len(per)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        keep_b, keep_l, kept = transform_boxes(allb[idx], alll[idx], box[per], flip[per], cell[per], S, self.min_visibility, self.min_box, return_mask=True)
        return out, src, box, flip, cell, out[per][kept], keep_b, keep_l

    def sample(self, shapes, boxes, labels, epoch, index):
        """shapes: the batch's (H, W); boxes / labels: per source image [n,4] COCO xywh pixels / [n].  -> (tiles, boxes, labels): the `Tile`s of the whole batch
        (output image j = tiles with b == j, in cell order) and per output image normalised xyxy float32 [k,4] / labels [k], k >= 1."""
        rng = np.random.default_rng((self.seed, self.rank, int(epoch), int(index)))
        B, S = len(shapes), self.size
        hw = np.asarray(shapes, dtype=np.float64).reshape(B, 2)
        boxes = [np.asarray(b, dtype=np.float64).reshape(-1, 4) for b in boxes]
        labels = [np.asarray(l).reshape(-1) for l in labels]
        allb, alll = np.concatenate(boxes), np.concatenate(labels)
        count = np.asarray([len(b) for b in boxes], dtype=np.int64)
        first = np.cumsum(count) - count
        tiles, out_b, out_l = [None] * B, [None] * B, [None] * B
        J = np.arange(B)
        for _ in range(self.max_tries):                                          # images left without a box are drawn again
            out, src, box, flip, cell, owner, kb, kl = self._draw(rng, J, hw, allb, alll, first, count)
            have = np.bincount(owner, minlength=B)
            for j in J[have[J] > 0].tolist():
                m = out == j
                tiles[j] = [Tile(k, tuple(bq), f, j, *cq) for k, bq, f, cq in zip(src[m].tolist(), box[m].tolist(), flip[m].tolist(), cell[m].tolist())]
                out_b[j], out_l[j] = kb[owner == j], kl[owner == j]
            J = J[have[J] == 0]
            if not len(J):
                break
        for j in J.tolist():                                                      # last resort: the whole, unflipped source at g = 1, every box kept
            H, W = shapes[j]
            tiles[j] = [Tile(j, (0.0, 0.0, float(W), float(H)), False, j, 0, 0, S, S)]
            out_b[j], out_l[j] = transform_boxes(boxes[j], labels[j], tiles[j][0].box, False, (0, 0, S, S), S, drop=False)
            if not len(out_b[j]):
                raise ValueError(f"TrainAugment: image {j} of batch {index} has no box inside the image (every image needs at least one target)")
            self.fallbacks += 1
        return [t for ts in tiles for t in ts], out_b, out_l


# ---------------------------------------------------------------------------------------------------------------------------------------
# The reference's loop does `image = image.to(device)` in front of every step (ref main.py:77-79): 7.1 MB of f32 pixels per B/16 image over
# PCIe, serialised with the step -- the HBM-resident kernels then wait for the bus (measured: 1003 against 1217 img/s at batch 32).  What
# the hot path needs from its caller is the next batch already in HBM when the step starts, and as few bytes over the bus as the data has:
# the u8 pixels (1.8 MB per 768^2 image; 0.9 MB for a COCO-size one that is resized on the device).
# ---------------------------------------------------------------------------------------------------------------------------------------
def _as_u8_tensor(img):
    """torch u8 tensor view of one host image (torch / numpy / PIL), no copy where the source allows it."""
    if torch.is_tensor(img):
        return img
    if isinstance(img, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(img))
    return torch.from_numpy(np.ascontiguousarray(np.asarray(img.convert("RGB") if hasattr(img, "convert") else img)))


def classify_images(images, size):
    """`size`: the model's input size, an int S or a pair (H, W); below S x S stands for H x W.
    What a host batch's image part is -> (kind, items).  kind: 'dense' (f32 / bf16 [B,3,S,S] pixel_values, the reference DataLoader's output: copied, cast to
    the compute type on the device), 'u8_chw' / 'u8_hwc' (uint8 [B,3,S,S] / [B,S,S,3] already at the model's size: table step only), 'u8_ragged' (a list of -- or
    a [B,H,W,3] tensor of -- uint8 HWC images of any sizes: Pillow-exact bicubic resize + table on the device).  Pure host logic (CPU-tested)."""
    H, W = size_hw(size)
    if isinstance(images, (list, tuple)):
        items = [_as_u8_tensor(im) for im in images]
        if not items:
            raise ValueError("DevicePrefetcher: empty image list")
        if all(t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3 for t in items):
            return "u8_ragged", items
        if all(t.dtype in (torch.float32, torch.bfloat16) and tuple(t.shape) == (3, H, W) for t in items):
            return "dense", [torch.stack(items)]
        raise ValueError("DevicePrefetcher: a list of images must hold uint8 [H,W,3] images (or [3,S,S] pixel_values)")
    t = images if torch.is_tensor(images) else _as_u8_tensor(images)
    if t.dtype in (torch.float32, torch.bfloat16):
        if t.dim() == 3:
            t = t.unsqueeze(0)
        if t.dim() != 4 or tuple(t.shape[1:]) != (3, H, W):
            raise ValueError(f"DevicePrefetcher: pixel_values must be [B,3,{H},{W}], got {tuple(t.shape)}")
        return "dense", [t]
    if t.dtype != torch.uint8:
        raise TypeError(f"DevicePrefetcher: images must be uint8 (raw pixels) or float32 / bfloat16 (pixel_values), got {t.dtype}")
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4:
        raise ValueError(f"DevicePrefetcher: uint8 images must be [B,H,W,3] or [B,3,S,S], got {tuple(t.shape)}")
    if tuple(t.shape[1:]) == (3, H, W):
        return "u8_chw", [t]
    if t.shape[3] == 3:
        if tuple(t.shape[1:3]) == (H, W):
            return "u8_hwc", [t]
        return "u8_ragged", [t[i] for i in range(t.shape[0])]
    raise ValueError(f"DevicePrefetcher: cannot interpret a uint8 tensor of shape {tuple(t.shape)}")


def pack_plan(items, align: int = 256):
    """Byte offsets of `items` (host tensors) in one staging slab, each aligned -> (offsets, total bytes)."""
    offs, off = [], 0
    for t in items:
        offs.append(off)
        off += (t.numel() * t.element_size() + align - 1) // align * align
    return offs, off


class _PinnedRing:
    """`n` pinned host slabs (grown on demand), each with the event of the last H2D copy that read it: a slab is rewritten only after that copy has finished."""

    def __init__(self, n):
        self.slabs = [None] * n
        self.events = [None] * n
        self.k = 0

    def next(self, nbytes):
        i = self.k
        self.k = (self.k + 1) % len(self.slabs)
        if self.events[i] is not None:
            self.events[i].synchronize()                    # (blocks the staging thread only)
        if self.slabs[i] is None or self.slabs[i].numel() < nbytes:
            self.slabs[i] = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, pin_memory=True)
        return i, self.slabs[i]


class DevicePrefetcher:
    """Wraps any iterable of host batches `(images, *targets)` -- the reference's `train_dataloader` (ref main.py:70-73) -- and yields the same tuples with the
    images ALREADY in HBM as the model's bf16 `[B,3,S,S]` input, one batch ahead of the step that consumes them:

        host batch -> pinned ring slab -> copy stream (H2D) -> DeviceImageProcessor (resize / table / cast, same stream) -> event -> handed to the caller's stream

    `images` may be uint8 raw pixels (a list of `[H,W,3]` images of any sizes, a `[B,H,W,3]` tensor, or `[B,S,S,3]` / `[B,3,S,S]` at the model's size) --
    a quarter (or an eighth, for COCO-size images) of the PCIe bytes of f32 pixel_values, processed bit-exactly like the reference's HF processor (fixture F7) --
    or the reference's own f32 `[B,3,S,S]` pixel_values (copied and cast only).  Targets: `target_transform(*targets)` runs on the HOST first (e.g. the
    reference's `coco_to_model_input`, ref main.py:79), then tensors and lists of tensors are moved to the device on the copy stream (`move_targets`); dicts
    (the reference's `metadata`) and everything else pass through untouched.  The reference loop's own `.to(device)` calls become no-ops.

    Ordering: the consumer's stream waits for the batch's event and the tensors are `record_stream`-ed on it, so the caching allocator does not recycle them
    while the step still reads them; a pinned slab is reused only after its own copy has completed.

    `augment=TrainAugment(size)` (train loops only; eval never augments) turns on random crops, flips and mosaics: the loader must then yield
    `(images, labels, boxes, *rest)` with uint8 HWC images, per-image label tensors and per-image COCO `xywh` PIXEL boxes.  The staging thread draws the
    batch's tiles (keyed by the augment's seed and rank, `set_epoch`'s epoch and the batch's index), builds their tap tables and descriptors, ships them in
    the same slab as the pixels and runs `owl_preprocess_u8_tiles` on the copy stream (with `TrainAugment(..., color=ColorJitter(...))` the tiles' colour
    rows ride in that slab too and the launch is `owl_preprocess_u8_tiles_color`; boxes and labels are the same either way); it hands over `(pixel_values, labels, boxes, *rest)` with the boxes
    already NORMALISED `xyxy` (skip `coco_to_model_input` for such batches).  `target_transform` then sees the augmented targets.  `threaded=True` pulls from the loader, stages and
    enqueues from a background thread (`depth` batches ahead); `threaded=False` does the same work inside `__next__`, one batch ahead.
    No CPU fallback: images are processed by libowlhip.so on the device or not at all."""

    _END = object()

    def __init__(self, loader, device="cuda", size=768, dtype=torch.bfloat16, depth=2, processor=None, target_transform=None,
                 move_targets=True, threaded=True, augment=None):
        self.loader = loader
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("DevicePrefetcher: the device must be a GPU (there is no CPU path)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.size = _size_attr(size)       # the int for a square, (H, W) for a rectangle (plain path only: augment= is square)
        self.dtype = dtype
        self.depth = max(1, int(depth))
        self.processor = processor if processor is not None else DeviceImageProcessor(size=size, device=self.device, dtype=dtype)
        if self.processor.size != self.size or self.processor.dtype != dtype:
            raise ValueError("DevicePrefetcher: the processor's size / dtype must match")
        self.target_transform = target_transform
        self.move_targets = bool(move_targets)
        self.threaded = bool(threaded)
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self._ring = _PinnedRing(self.depth + 2)
        from collections import deque
        self._inflight = deque()
        self._thread = None
        self._stop = None
        self._q = None
        self.bytes_h2d = 0                 # bytes sent over the bus so far (statistics: bench.py reports bytes per image)
        self.batches = 0
        self.stage_seconds = 0.0           # host time spent staging (pull from the loader excluded): must stay below the step time for the stage to hide
        self.augment = augment
        if augment is not None and isinstance(self.size, tuple):
            raise ValueError(_SQUARE_ONLY.format(what="DevicePrefetcher(augment=)", size=self.size))
        if augment is not None and getattr(self.processor, "resize", "pillow") == "owlv2":
            raise ValueError(_OWLV2_PLAIN_ONLY.format(what="DevicePrefetcher(augment=)"))
        if augment is not None and augment.size != self.size:
            raise ValueError(f"DevicePrefetcher: augment.size = {augment.size} but size = {self.size}")
        self.augment_seconds = 0.0         # of which: drawing the tiles and building their tap tables and descriptors
        self._epoch = 0
        self._index = 0                    # index of the next batch within the epoch (reset by __iter__)

    def set_epoch(self, epoch: int):
        """The epoch that keys the augmentation's draws (as DistributedSampler.set_epoch: call it before iterating)."""
        self._epoch = int(epoch)

    def __len__(self):
        return len(self.loader)

    # -- staging (runs in the background thread when threaded) ------------------------------------------------------------------------------
    def _h2d(self, items, patch=None):
        """Host tensors (the batch's images AND its target tensors) -> ONE pinned ring slab -> ONE H2D copy -> device views (never one small copy per tensor: a
        pageable source makes every `.to(device)` a blocking round trip).  A large tensor the caller already pinned (DataLoader(pin_memory=True)) goes as it is.
        The host-side copy into the slab is a plain memmove (ctypes: releases the GIL): torch's own CPU copy fans out over the intra-op thread pool, which --
        called from a second thread on a many-core host -- costs several times the copy itself (measured: 40 ms per 57 MB batch on the 256-thread GPU box).
        `patch(out)` runs once every item's device address is known and before the host bytes are copied into the slab: the tile descriptors, which ride
        in this slab, hold device addresses of other items of it."""
        import ctypes
        while self._inflight and self._inflight[0][0].query():          # caller-pinned sources whose copies have completed
            self._inflight.popleft()
        out = [None] * len(items)
        packed = []
        for k, t in enumerate(items):
            if t.is_cuda:
                out[k] = t if t.device == self.device else t.to(self.device, non_blocking=True)
            elif t.is_pinned() and t.is_contiguous() and t.numel() * t.element_size() >= (1 << 20):
                dst = torch.empty(t.shape, dtype=t.dtype, device=self.device)
                dst.copy_(t, non_blocking=True)
                ev = torch.cuda.Event(); ev.record(self.copy_stream)
                self._inflight.append((ev, t))                           # keeps the pinned source alive until its copy has run
                self.bytes_h2d += t.numel() * t.element_size()
                out[k] = dst
            else:
                packed.append(k)
        if packed:
            src = [items[k].contiguous() for k in packed]
            offs, total = pack_plan(src)
            i, slab = self._ring.next(total)
            base = slab.data_ptr()
            dslab = torch.empty(total, dtype=torch.uint8, device=self.device)
            for k, t, o in zip(packed, src, offs):
                out[k] = dslab[o:o + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
            if patch is not None:
                patch(out)
            for t, o in zip(src, offs):
                n = t.numel() * t.element_size()
                if n:
                    ctypes.memmove(base + o, t.data_ptr(), n)
            dslab.copy_(slab[:total], non_blocking=True)
            ev = torch.cuda.Event(); ev.record(self.copy_stream)
            self._ring.events[i] = ev
            self.bytes_h2d += total
        elif patch is not None:
            patch(out)
        return out

    def _images_on_device(self, kind, dev):
        if kind == "dense":
            x = dev[0]
            if x.dtype == self.dtype:
                return x
            if x.dtype == torch.float32 and self.dtype == torch.bfloat16:
                return ops.cast_bf16(x.contiguous())         # the model's own first step (same kernel, same rounding), off the critical path
            return x.to(self.dtype)
        if kind in ("u8_chw", "u8_hwc"):
            return self.processor.normalize_sized(dev[0], chw=(kind == "u8_chw"))
        return self.processor(dev)["pixel_values"]

    def _stage(self, batch):
        if not isinstance(batch, (list, tuple)) or len(batch) < 1:
            raise TypeError("DevicePrefetcher: the loader must yield (images, *targets) tuples")
        images, rest = batch[0], tuple(batch[1:])
        import time
        plan = None
        if self.augment is not None:
            ta = time.perf_counter()
            items, rest, plan = self._augment(images, rest)
            self.augment_seconds += time.perf_counter() - ta
        if self.target_transform is not None:
            rest = self.target_transform(*rest)
            if not isinstance(rest, tuple):
                rest = (rest,)
        t0 = time.perf_counter()
        if plan is None:
            kind, items = classify_images(images, self.size)
        # target tensors ride in the same slab: (position in `rest`, index inside a list or None)
        where, tensors = [], []
        if self.move_targets:
            for r, obj in enumerate(rest):
                if torch.is_tensor(obj):
                    where.append((r, None)); tensors.append(obj)
                elif isinstance(obj, (list, tuple)) and obj and all(torch.is_tensor(o) for o in obj):
                    for j, o in enumerate(obj):
                        where.append((r, j)); tensors.append(o)
        with torch.cuda.stream(self.copy_stream):
            if plan is None:
                dev = self._h2d(list(items) + tensors)
                img = self._images_on_device(kind, dev[:len(items)])
            else:
                desc, arena, tmp_bytes, max_rows, color = plan
                n = len(items)
                extra = [torch.from_numpy(arena), torch.from_numpy(desc)] + ([torch.from_numpy(color)] if color is not None else [])
                k = len(items) + len(tensors)                                      # arena, descriptors [, colour rows] ride behind the pixels and targets
                dev = self._h2d(list(items) + tensors + extra,
                                patch=lambda out: resolve_tile_descs(desc, [t.data_ptr() for t in out[:n]], out[k].data_ptr()))
                img = self.processor.run_tiles(dev[k + 1], desc.shape[0], max_rows, tmp_bytes, n, color=dev[k + 2] if color is not None else None)
                dev = dev[:k]
            if tensors:
                seq = {r: type(rest[r]) for r, j in where if j is not None}       # lists / tuples of tensors keep their type
                rest = [list(o) if r in seq else o for r, o in enumerate(rest)]
                for (r, j), d in zip(where, dev[len(items):]):
                    if j is None:
                        rest[r] = d
                    else:
                        rest[r][j] = d
                rest = tuple(seq[r](o) if r in seq else o for r, o in enumerate(rest))
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        self.batches += 1
        self.stage_seconds += time.perf_counter() - t0
        return (img,) + tuple(rest), ev

    def _augment(self, images, rest):
        """(images, labels, boxes, *more) -> the batch's uint8 sources, (labels, boxes, *more) of the AUGMENTED images, and the host half of the tile path."""
        kind, items = classify_images(images, self.size)
        if kind == "dense":
            raise ValueError("DevicePrefetcher: augment= needs uint8 images: crop, flip and mosaic are folded into the uint8 resampler (one interpolation per "
                             "source pixel), and float pixel_values have already been resized and normalised -- feed the raw pixels, or augment=None")
        if kind == "u8_chw":
            raise ValueError("DevicePrefetcher: augment= reads uint8 HWC images ([H,W,3] each, or [B,H,W,3]); got channels-first [B,3,S,S]")
        if kind == "u8_hwc":
            items = [items[0][i] for i in range(items[0].shape[0])]
        items = [t.contiguous() for t in items]
        if len(rest) < 2 or len(rest[0]) != len(items) or len(rest[1]) != len(items):
            raise ValueError("DevicePrefetcher: with augment= the loader must yield (images, labels, boxes, *rest) with per-image labels and COCO xywh boxes")
        labels = [np.asarray(torch.as_tensor(l)) for l in rest[0]]
        boxes = [np.asarray(torch.as_tensor(b), dtype=np.float64).reshape(-1, 4) for b in rest[1]]
        shapes = [(int(t.shape[0]), int(t.shape[1])) for t in items]
        tiles, ob, ol = self.augment.sample(shapes, boxes, labels, self._epoch, self._index)
        color = self.augment.sample_color(len(tiles), self._epoch, self._index) if getattr(self.augment, "color", None) is not None else None
        self._index += 1
        check_tile_cover(tiles, len(items), self.size, shapes)
        plan = build_tile_tables(shapes, tiles) + (color,)
        return items, ([torch.from_numpy(l) for l in ol], [torch.from_numpy(b) for b in ob]) + tuple(rest[2:]), plan

    # -- hand-over (the caller's thread and stream) ------------------------------------------------------------------------------------------------
    def _hand_over(self, staged):
        out, ev = staged
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        for o in out:
            for t in (o if isinstance(o, (list, tuple)) else (o,)):
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(cur)
        return out

    def _worker(self, it, q, stop):
        import queue
        try:
            torch.cuda.set_device(self.device)
            for batch in it:
                item = self._stage(batch)
                while not stop.is_set():
                    try:
                        q.put(item, timeout=0.1)
                        break
                    except queue.Full:
                        continue
                if stop.is_set():
                    return
            item = self._END
        except BaseException as e:          # re-raised in the consumer's thread
            item = e
        while not stop.is_set():
            try:
                q.put(item, timeout=0.1)
                return
            except queue.Full:
                continue

    def close(self):
        """Stop the background thread (also called when the iterator is exhausted, abandoned by a new __iter__, or collected)."""
        if self._stop is not None:
            self._stop.set()
        if self._thread is not None and self._thread.is_alive():
            self._thread.join(timeout=5.0)
        self._thread = self._stop = self._q = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __iter__(self):
        self.close()
        self._index = 0
        it = iter(self.loader)
        if not self.threaded:
            from collections import deque
            pending = deque()
            done = False
            while True:
                while not done and len(pending) < 1 + 1:          # the batch handed over now + one in flight behind it
                    try:
                        pending.append(self._stage(next(it)))
                    except StopIteration:
                        done = True
                if not pending:
                    return
                yield self._hand_over(pending.popleft())
        import queue
        import threading
        q, stop = queue.Queue(maxsize=self.depth), threading.Event()
        th = threading.Thread(target=self._worker, args=(it, q, stop), daemon=True, name="owl-prefetch")
        self._thread, self._stop, self._q = th, stop, q
        th.start()
        try:
            while True:
                item = q.get()
                if item is self._END:
                    return
                if isinstance(item, BaseException):
                    raise item
                yield self._hand_over(item)
        finally:
            stop.set()
