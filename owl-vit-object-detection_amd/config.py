"""Architecture table for the OWL-ViT vision path.

The reference hard-wires ``google/owlvit-base-patch32`` (reference src/models.py:152-153); the
BASELINE configs ask for B/16 @768 and L/14 @840.  All numbers are the
public HF config values (``OwlViTVisionConfig`` / ``OwlViTTextConfig``).  ``tiny*`` configs exist
only for the parity tests: they keep dh = 64 (what the attention kernels are built for), L = 12 so
the literal ``"layers.11"`` freeze rule (reference src/models.py:175) still selects a layer, and an
L = 14 variant so frozen layers sit *above* the trainable one as in L/14.
"""
from dataclasses import dataclass, asdict
from math import isqrt

MAX_PATCHES = 8192     # P ceiling of owl_spread_labels / owl_postprocess (one workgroup walks an image's patches)
MAX_GRID_SIDE = 256    # side ceiling of either grid of owl_pos_resample_hw (only a rectangle can reach it below MAX_PATCHES)


def image_hw(image_size):
    """(H, W) of an `image_size` given as an int (square) or a pair (height, width)."""
    if isinstance(image_size, (tuple, list)):
        if len(image_size) != 2:
            raise ValueError(f"image_size={image_size!r}: an int (square) or a pair (height, width)")
        return int(image_size[0]), int(image_size[1])
    return int(image_size), int(image_size)


@dataclass(frozen=True)
class OwlConfig:
    name: str
    image_size: int      # S (square) or (H, W); a pair with H == W is stored as the int, so a square config has one form
    patch_size: int
    hidden: int          # D
    heads: int           # H (dh = D / H must be 64)
    mlp: int             # I
    layers: int          # L
    text_dim: int        # Dt (query / class-embedding width)
    n_classes: int = 10  # C; queries = 3 * C (reference src/models.py:155-159)
    ln_eps: float = 1e-5
    pos_grid: int = 0    # side of the NATIVE position table (the checkpoint's); 0 = `grid`.  Another value: the table is resampled to `grid` (models.OwlViT)

    def __post_init__(self):
        if isinstance(self.image_size, (tuple, list)):
            H, W = image_hw(self.image_size)
            object.__setattr__(self, "image_size", H if H == W else (H, W))

    @property
    def image_hw(self) -> tuple:       # (H, W)
        return image_hw(self.image_size)

    @property
    def is_square(self) -> bool:
        return not isinstance(self.image_size, tuple)

    @property
    def grid_h(self) -> int:           # gh
        return self.image_hw[0] // self.patch_size

    @property
    def grid_w(self) -> int:           # gw
        return self.image_hw[1] // self.patch_size

    @property
    def grid(self) -> int:
        if not self.is_square:         # a square-only consumer must not compute on the wrong grid
            raise ValueError(f"OwlConfig.grid: image_size={self.image_size} is not square ({self.grid_h} x {self.grid_w} patches); use grid_h and grid_w")
        return self.image_size // self.patch_size

    @property
    def native_grid(self) -> int:      # g0
        if not self.pos_grid and not self.is_square:
            raise ValueError(f"OwlConfig: image_size={self.image_size} is not square, so the side of the native (square) position table cannot be "
                             "taken from it: set pos_grid (load_model(..., image_size=(H, W)) does)")
        return self.pos_grid or self.grid

    @property
    def resampled(self) -> bool:       # the run table is a resample of the native one.  Decided by the grid, not by P: 4 x 9 has the 36 patches of 6 x 6
        return (self.grid_h, self.grid_w) != (self.native_grid, self.native_grid)

    @property
    def pos_rows(self) -> int:         # rows of the position-embedding PARAMETER: g0 * g0 + 1, whatever the input size
        return self.native_grid * self.native_grid + 1

    @property
    def patches(self) -> int:          # P
        return self.grid_h * self.grid_w

    @property
    def tokens(self) -> int:           # T = P + 1 (class token first, HF5:338-339)
        return self.patches + 1

    @property
    def tokens_padded(self) -> int:    # Tp: per-image row stride in HBM (multiple of 8)
        return (self.tokens + 7) // 8 * 8

    @property
    def head_dim(self) -> int:
        return self.hidden // self.heads

    @property
    def queries(self) -> int:          # Q = 3C
        return 3 * self.n_classes

    @property
    def patch_k(self) -> int:          # K of the patch-embed contraction (3 * p * p)
        return 3 * self.patch_size * self.patch_size

    def replace(self, **kw) -> "OwlConfig":
        d = asdict(self)
        d.update(kw)
        return OwlConfig(**d)

    # ---- algorithmic work (2*MACs of matmuls only) -------------------
    def flops_layer(self) -> float:
        T, D, I = self.tokens, self.hidden, self.mlp
        return 8.0 * T * D * D + 4.0 * T * D * I + 4.0 * T * T * D

    def flops_heads(self) -> float:
        P, D, Dt, Q = self.patches, self.hidden, self.text_dim, self.queries
        return 2.0 * P * D * Dt + 2.0 * P * Dt * Q + 2.0 * P * (2 * D * D + 4 * D)

    def flops_forward(self) -> float:
        return self.layers * self.flops_layer() + 2.0 * self.patches * self.patch_k * self.hidden + self.flops_heads()

    def trainable_layer(self) -> int:
        """Index selected by the literal substring rule ``"layers.11" in name``."""
        return 11

    def flops_backward(self, trainable_layers=None, floor=None) -> float:
        """Default: the reference set.  Another set is stated by its trainable encoder layers and the floor of its dX chain (models.OwlViT's
        `trainable_layers` / `backward_floor`); the heads count 2x whichever of them train."""
        # trainable layer: dX + dW = 2x its forward; frozen layers above it: dX only
        # (linear 1x, attention 2x of their forward parts); heads 2x.
        T, D, I = self.tokens, self.hidden, self.mlp
        lin = 8.0 * T * D * D + 4.0 * T * D * I
        att = 4.0 * T * T * D
        if trainable_layers is None and floor is None:
            above = self.layers - 1 - self.trainable_layer()
            return 2.0 * self.flops_layer() + above * (lin + 2.0 * att) + 2.0 * self.flops_heads()
        tls = tuple(sorted(trainable_layers or ()))
        floor = (tls[0] if tls else "heads") if floor is None else floor
        if floor in ("heads", "post_post_layernorm", "post_layernorm"):
            return 2.0 * self.flops_heads()
        low = floor if isinstance(floor, int) else 0          # lowest layer the chain crosses
        crossed = self.layers - low - len([i for i in tls if i >= low])
        # (a trainable layer counts 2x its forward wherever it sits, as in the default: its LayerNorm 1 needs the dX through QKV either way)
        total = 2.0 * self.flops_heads() + crossed * (lin + 2.0 * att) + len([i for i in tls if i >= low]) * 2.0 * self.flops_layer()
        if floor == "embeddings":
            total += 2.0 * self.patches * self.patch_k * self.hidden          # the patch-embedding weight gradient
        return total

    def flops_train_step(self, trainable_layers=None, floor=None) -> float:
        return self.flops_forward() + self.flops_backward(trainable_layers, floor)


CONFIGS = {
    "owlvit-base-patch32": OwlConfig("owlvit-base-patch32", 768, 32, 768, 12, 3072, 12, 512),
    "owlvit-base-patch16": OwlConfig("owlvit-base-patch16", 768, 16, 768, 12, 3072, 12, 512),
    "owlvit-large-patch14": OwlConfig("owlvit-large-patch14", 840, 14, 1024, 16, 4096, 24, 768),
    # OWLv2 (google/owlv2-*): the same vision path at 960 / 1008 (native grids 60 / 72); inputs from DeviceImageProcessor(resize="owlv2")
    "owlv2-base-patch16": OwlConfig("owlv2-base-patch16", 960, 16, 768, 12, 3072, 12, 512),
    "owlv2-large-patch14": OwlConfig("owlv2-large-patch14", 1008, 14, 1024, 16, 4096, 24, 768),
    # parity-test configs (not real checkpoints)
    "tiny": OwlConfig("tiny", 96, 16, 128, 2, 256, 12, 64, n_classes=4),
    "tiny-l14": OwlConfig("tiny-l14", 96, 16, 128, 2, 256, 14, 64, n_classes=4),
    "small": OwlConfig("small", 192, 16, 256, 4, 512, 12, 128, n_classes=10),
}


def table_grid(pos_rows: int) -> int:
    """Side g0 of a position table of `pos_rows` rows (class row + g0 x g0 patch rows); ValueError if the patch rows are no square."""
    rows = int(pos_rows)
    g0 = isqrt(max(rows - 1, 0))
    if rows < 2 or g0 * g0 != rows - 1:
        raise ValueError(f"a position table of {rows} rows is not a class row plus a square grid of patch rows; the nearest tables that are have "
                         f"{max(g0, 1) ** 2 + 1} ({max(g0, 1)} x {max(g0, 1)}) and {(g0 + 1) ** 2 + 1} ({g0 + 1} x {g0 + 1}) rows")
    return g0


def _check_image_hw(H: int, W: int, p: int):
    """check_image_size for a pair (height, width) -> (gh, gw)."""
    for side, v in (("height", H), ("width", W)):
        if v < p or v % p:
            lo, hi = max(v // p, 1) * p, (max(v // p, 0) + 1) * p
            near = f"{lo} and {hi}" if lo != hi and hi <= MAX_GRID_SIDE * p else f"{min(lo, MAX_GRID_SIDE * p)}"
            raise ValueError(f"image_size=({H}, {W}): the {side} {v} is not a positive multiple of the patch size {p}; the nearest sizes that are: {near}")
    gh, gw = H // p, W // p
    for side, g, other in (("height", gh, gw), ("width", gw, gh)):
        if g > MAX_GRID_SIDE:
            raise ValueError(f"image_size=({H}, {W}): the {side} gives {g} patches of {p} pixels; the position-table kernels take grids of at most "
                             f"{MAX_GRID_SIDE} per side: the largest {side} is {MAX_GRID_SIDE * p}")
    if gh * gw > MAX_PATCHES:
        raise ValueError(f"image_size=({H}, {W}) gives {gh * gw} patches of {p} pixels ({gh} x {gw}); the loss and post-process kernels take at most "
                         f"{MAX_PATCHES} per image: the largest height at this width is {min(MAX_PATCHES // gw, MAX_GRID_SIDE) * p}, the largest width at this "
                         f"height {min(MAX_PATCHES // gh, MAX_GRID_SIDE) * p}")
    return gh, gw


def check_image_size(image_size, patch_size: int, pos_rows: int = None):
    """Host-side validation of a requested input size, an int (square) or a pair (height, width): each side a positive multiple of the patch size, at most
    MAX_PATCHES patches (a pair: at most MAX_GRID_SIDE per side as well), and -- given the row count of the position table it will be run with -- a table
    that is a class row plus a square grid.  -> the run grid: g for an int, (gh, gw) for a pair.  Every failure is a ValueError naming the nearest valid sizes."""
    if isinstance(image_size, (tuple, list)):
        grid = _check_image_hw(*image_hw(image_size), int(patch_size))
        if pos_rows is not None:
            table_grid(pos_rows)
        return grid
    S, p = int(image_size), int(patch_size)
    top = isqrt(MAX_PATCHES) * p
    if S < p or S % p:
        lo, hi = max(S // p, 1) * p, (max(S // p, 0) + 1) * p
        near = f"{lo} and {hi}" if lo != hi and hi <= top else f"{min(lo, top)}"
        raise ValueError(f"image_size={S} is not a positive multiple of the patch size {p}; the nearest sizes that are: {near}")
    g = S // p
    if g * g > MAX_PATCHES:
        raise ValueError(f"image_size={S} gives {g * g} patches of {p} pixels; the loss and post-process kernels take at most {MAX_PATCHES} per image: "
                         f"the largest size is {top} ({isqrt(MAX_PATCHES)} x {isqrt(MAX_PATCHES)} patches)")
    if pos_rows is not None:
        table_grid(pos_rows)
    return g


def get_config(name: str, **overrides) -> OwlConfig:
    name = name.replace("google/", "")
    cfg = CONFIGS[name]
    return cfg.replace(**overrides) if overrides else cfg


@dataclass(frozen=True)
class TextConfig:
    """CLIP-style text tower used once to initialise the query bank (ref src/models.py:155-169; HF ``OwlViTTextConfig``
    defaults for the base models, public ``google/owlvit-large-patch14`` values for L/14).  dh = width / heads = 64."""
    name: str
    width: int
    heads: int
    mlp: int
    layers: int
    proj_dim: int            # = OwlConfig.text_dim (query width); HF needs proj_dim == width (class head out_dim, HF5:1009)
    vocab: int = 49408
    max_pos: int = 16
    ln_eps: float = 1e-5


TEXT_CONFIGS = {
    "owlvit-base-patch32": TextConfig("owlvit-base-text", 512, 8, 2048, 12, 512),
    "owlvit-base-patch16": TextConfig("owlvit-base-text", 512, 8, 2048, 12, 512),
    "owlvit-large-patch14": TextConfig("owlvit-large-text", 768, 12, 3072, 12, 768),
    "owlv2-base-patch16": TextConfig("owlvit-base-text", 512, 8, 2048, 12, 512),          # Owlv2TextConfig = OwlViTTextConfig, value for value
    "owlv2-large-patch14": TextConfig("owlvit-large-text", 768, 12, 3072, 12, 768),
    "tiny": TextConfig("tiny-text", 64, 1, 128, 3, 64, vocab=97, max_pos=16),
    "tiny-l14": TextConfig("tiny-text", 64, 1, 128, 3, 64, vocab=97, max_pos=16),
    "small": TextConfig("small-text", 128, 2, 256, 3, 128, vocab=97, max_pos=16),
}


def get_text_config(name: str) -> TextConfig:
    return TEXT_CONFIGS[name.replace("google/", "")]
