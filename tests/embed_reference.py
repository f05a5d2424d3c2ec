"""Float64 / int64 reference of the patch embedding (owl_patch_embed_bf16, include/owl_hip.h) and of the two small kernels below it
(owl_im2row_bf16, owl_embed_bwd), with elementwise bounds derived the way tests/gemm_reference.py derives them.  CPU only: numpy / torch.

THE OPERATION (HF5:282-288 Conv2d k = s = ps without bias; HF5:336-343 flatten + positions), for image b, patch p = py G + px, column d:

    x[b, 1 + p, d] = sum_{c, ky, kx} image[b, c, py ps + ky, px ps + kx] w[d, c, ky, kx]  +  pos[1 + p, d]

into a [B, Tp, D] f32 buffer whose row 0 of every image (the class token), rows T .. Tp - 1 (pad rows, T = P + 1) and everything past image B - 1 the
entry must NOT write (`exact` returns that mask).

THE K ORDER (restated from the header's text, not from the kernels): a patch row is padded to psp = the power of two >= ps positions,
k = (c ps + ky) psp + pos, position `pos` holds pixel min(8 (pos // 8), ps - 8) + pos % 8 -- the last 16-byte chunk of a row overlaps its predecessor --
and K = 3 ps psp is zero-padded to Kg = K rounded up to 64.  `gather_rows` builds that matrix; times weights.patch_weight_gather_layout(w)^T it must be the
convolution (tests/test_embed_reference.py, every even ps in 8 .. 64).

THE BOUND.  u = 2^-8 is bf16's unit round-off, f = 2^-24 f32's (tests/gemm_reference.py's conventions).
  * A product of two bf16 values has 16 significant bits: exact in f32.  (A product below 2^-126 may be flushed: n 2^-126 absolute, n = 3 ps^2.)
  * The n = 3 ps^2 real products (the weight is ZERO at the duplicated and the padded positions, and adding an exact zero does not round) are added in
    f32 in an order the test does not assume, by MFMA adders whose rounding mode it does not assume either (2 f per add):
        |acc~ - acc| <= gamma2(n) sum |a| |w|,     gamma2(n) = 2 n f / (1 - 2 n f)             (gemm_reference.gamma2, the any-order form)
  * out = fl(acc~ + pos): one more f32 rounding (a plain round-to-nearest add), f |acc~ + pos| <= f (|ref| + acc_tol).
        tol = acc_tol + f (|ref| + acc_tol) + n 2^-126
No measured constant.  On the `integers` profile every partial sum in any order is an integer below 2^24: tol is replaced by torch.equal.

THE PROFILES (make_inputs): `integers` pixels and weights in [-8, 8], pos integers with |pos| <= 2^16: sum |a| |w| <= 64 * 3 ps^2 = 786 432 at ps = 64,
plus 2^16 stays below 2^24 (assert_exact_ok checks the actual figure); `clip_pixels` the values the pre-process table produces for random u8 levels
(transformers' rescale + normalize, CLIP mean / std), bf16-rounded, with HF-init weights (std 0.02) and positions (std 0.02); `saturated` level 255 in
every pixel; `pos_dominates` |pos| ~ 1e3 against |acc| ~ 1e-3 (weights std 0.02 * 2^-9); `cancels` pos[1 + p] = -f32(acc64[image 0, p]): the output of
image 0 is the accumulation error alone, so only the ABSOLUTE part of the bound admits it."""
import numpy as np
import torch
import torch.nn.functional as Fn

from tests import gemm_reference as GR

F = GR.F
TINY = GR.TINY
BK = 64                                   # K-tile of the GEMM family
PATCH_SIZES = tuple(range(8, 65, 2))      # "EVERY even patch size 8 <= ps <= 64" (include/owl_hip.h)
TILES = (7, 256, 128)                     # two-phase ping-pong, single-phase 256 x 256, single-phase 128 x 128
PROFILES = ("integers", "clip_pixels", "saturated", "pos_dominates", "cancels")
FLOAT_PROFILES = PROFILES[1:]
SENTINEL_BITS = 0x4B5A3C96                # f32 14 302 358.0: finite, NaN-free, no value any profile produces, a bit pattern a stray zero / pos store breaks
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# geometry of the K order
# ---------------------------------------------------------------------------------------------------------------------------------------------
def psp_of(ps):
    psp = 8
    while psp < ps:
        psp *= 2
    return psp


def k_real(ps):
    return 3 * ps * psp_of(ps)


def kg_of(ps):
    return (k_real(ps) + BK - 1) // BK * BK


def pixel_of(pos, ps):
    return min(8 * (pos // 8), ps - 8) + pos % 8


def tp_of(P, extra=None):
    """Tokens padded to 8 per image (the model's rule); extra = rows beyond T = P + 1 instead."""
    return (P + 1 + 7) // 8 * 8 if extra is None else P + 1 + extra


def patches_of(img, ps):
    """[B, 3, S, S] -> [B P, 3, ps, ps], row b P + py G + px."""
    B, C, S, _ = img.shape
    G = S // ps
    return img.reshape(B, C, G, ps, G, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, C, ps, ps)


def gather_rows(img, ps):
    """The A operand in the header's K order: [B P, Kg], k = (c ps + ky) psp + pos = pixel (c, ky, pixel_of(pos)), zeros in [K, Kg)."""
    psp = psp_of(ps)
    pt = patches_of(img, ps)
    pix = [pixel_of(pos, ps) for pos in range(psp)]
    rows = pt[:, :, :, pix].reshape(pt.shape[0], 3 * ps * psp)
    out = torch.zeros(pt.shape[0], kg_of(ps), dtype=img.dtype)
    out[:, :rows.shape[1]] = rows
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# reference and bound
# ---------------------------------------------------------------------------------------------------------------------------------------------
def conv64(img, w):
    """float64 convolution k = s = ps, no bias -> [B, P, D]."""
    ps = w.shape[-1]
    return Fn.conv2d(img.double(), w.double(), stride=ps).flatten(2).transpose(1, 2).contiguous()


def exact(img_bf16, w_bf16, pos, Tp, extra_images=1):
    """(ref float64 [B + extra, Tp, D], mask bool [B + extra, Tp]).  ref = conv64 + pos[1 + p] on rows 1 .. P of images 0 .. B - 1 (zeros elsewhere);
    mask names the rows the entry must not write: row 0 of every image, rows T .. Tp - 1, every row of the extra image blocks."""
    acc = conv64(img_bf16, w_bf16)
    B, P, D = acc.shape
    assert pos.shape == (P + 1, D) and Tp >= P + 1
    ref = torch.zeros(B + extra_images, Tp, D, dtype=torch.float64)
    ref[:B, 1:P + 1] = acc + pos.double()[1:]
    mask = torch.ones(B + extra_images, Tp, dtype=torch.bool)
    mask[:B, 1:P + 1] = False
    return ref, mask


def bounds(img_bf16, w_bf16, pos, Tp, extra_images=1):
    """Elementwise tolerance [B + extra, Tp, D] for `exact`'s ref (module docstring); 0 on the rows of the mask (those are held to their sentinel bits)."""
    ps = w_bf16.shape[-1]
    n = 3 * ps * ps
    ref, _ = exact(img_bf16, w_bf16, pos, Tp, extra_images)
    acc_abs = conv64(img_bf16.double().abs(), w_bf16.double().abs())
    B, P, D = acc_abs.shape
    acc_tol = GR.gamma2(n) * acc_abs
    tol = torch.zeros_like(ref)
    tol[:B, 1:P + 1] = acc_tol + F * (ref[:B, 1:P + 1].abs() + acc_tol) + n * TINY
    return tol


def assert_exact_ok(img, w, pos):
    """The `integers` promise: sum |a| |w| + |pos| < 2^24 everywhere, so every partial sum in any order is exact in f32."""
    worst = float(conv64(img.double().abs(), w.double().abs()).max()) + float(pos.abs().max())
    assert worst < 2.0 ** 24, worst
    return worst


def poison_patch(img, b, p, ps):
    """A copy of img with every pixel of patch p of image b NaN."""
    out = img.clone()
    G = img.shape[-1] // ps
    py, px = divmod(p, G)
    out[b, :, py * ps:(py + 1) * ps, px * ps:(px + 1) * ps] = float("nan")
    return out


def bits(t):
    return GR.bits(t)


def sentinel(shape, device="cpu"):
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int32, device=device).view(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# input profiles
# ---------------------------------------------------------------------------------------------------------------------------------------------
def normalize_table():
    """[3, 256] f32: transformers' rescale (f64 multiply, f32 cast) + normalize (f32) of each u8 level -- what the pre-process kernels look up."""
    v = (np.arange(256).astype(np.float64) * (1 / 255)).astype(np.float32)
    m = np.array(CLIP_MEAN, dtype=np.float32)[:, None]
    s = np.array(CLIP_STD, dtype=np.float32)[:, None]
    return torch.from_numpy(((v[None, :] - m) / s).astype(np.float32))


def _clip_image(levels):
    lut = normalize_table()
    B, C, S, _ = levels.shape
    return torch.stack([lut[c][levels[:, c]] for c in range(3)], 1).bfloat16()


def make_inputs(profile, B, S, ps, D, seed=0):
    """(image bf16 [B, 3, S, S], w bf16 [D, 3, ps, ps], pos f32 [P + 1, D]) on the CPU."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * ps + B + S + D + PROFILES.index(profile))
    P = (S // ps) ** 2
    if profile == "integers":
        img = torch.randint(-8, 9, (B, 3, S, S), generator=g).bfloat16()
        w = torch.randint(-8, 9, (D, 3, ps, ps), generator=g).bfloat16()
        pos = torch.randint(-2 ** 16, 2 ** 16 + 1, (P + 1, D), generator=g).float()
        return img, w, pos
    if profile == "saturated":
        img = _clip_image(torch.full((B, 3, S, S), 255, dtype=torch.int64))
    else:
        img = _clip_image(torch.randint(0, 256, (B, 3, S, S), generator=g))
    w = (torch.randn(D, 3, ps, ps, generator=g) * 0.02).bfloat16()
    pos = torch.randn(P + 1, D, generator=g) * 0.02
    if profile == "pos_dominates":
        w = (w.float() * 2.0 ** -9).bfloat16()
        pos = torch.randn(P + 1, D, generator=g) * 1e3
    elif profile == "cancels":
        pos = pos.clone()
        pos[1:] = -conv64(img[:1], w)[0].float()
    return img, w, pos


def device_integers(B, S, seed, device):
    """The `integers` image generated on the device (a multi-GiB batch): int pixels in [-8, 8] as bf16, reproducible per image."""
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(-8, 9, (B, 3, S, S), generator=g, device=device, dtype=torch.int8).bfloat16()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# f32 emulations (what a correct kernel may compute): the real products added in f32 in two different orders, then + pos in f32
# ---------------------------------------------------------------------------------------------------------------------------------------------
def emulate(img_bf16, w_bf16, pos, Tp, order, extra_images=1):
    """order 'sequential': k = 0, 1, ... of the conv weight's own (c, ky, kx) order one at a time; 'chunks32': the sum of each run of 32 k (formed
    sequentially from zero) added to the accumulator."""
    ps = w_bf16.shape[-1]
    a = patches_of(img_bf16.float(), ps).reshape(-1, 3 * ps * ps)
    w = w_bf16.float().reshape(w_bf16.shape[0], -1)
    K = a.shape[1]
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    step = 1 if order == "sequential" else 32
    for k0 in range(0, K, step):
        part = torch.zeros_like(acc)
        for k in range(k0, min(K, k0 + step)):
            part = part + a[:, k, None] * w[None, :, k]        # (the product is exact in f32; one rounding per add)
        acc = acc + part
    B = img_bf16.shape[0]
    P = a.shape[0] // B
    out = sentinel((B + extra_images, Tp, w.shape[0])).clone()
    out[:B, 1:P + 1] = acc.view(B, P, -1) + pos[1:]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------------------------------
def check_untouched(name, got, mask, fails=None):
    """Every row the mask names still holds the sentinel's bits."""
    bad = (bits(got.cpu()) != SENTINEL_BITS).any(-1) & mask
    nb = int(bad.sum())
    if nb:
        msg = f"{name}: {nb} rows the entry must not write lost their sentinel; first (image, row) {bad.nonzero()[:6].tolist()}"
        if fails is None:
            raise AssertionError(msg)
        fails.append(msg)
    return nb


def check_exact(name, got, ref, mask, fails=None, nan_rows=None):
    """torch.equal on every written row (float64 of the f32 output against the int64-valued reference); rows of `nan_rows` (bool [B + extra, Tp]) must
    instead be NaN in every column."""
    g = got.cpu().double()
    written = ~mask if nan_rows is None else ~mask & ~nan_rows
    bad = (g != ref).any(-1) & written
    msgs = []
    if int(bad.sum()):
        i = tuple(bad.nonzero()[0].tolist())
        col = int((g[i] != ref[i]).nonzero()[0])
        msgs.append(f"{name}: {int(bad.sum())} written rows differ from the exact reference; first (image, row) {bad.nonzero()[:6].tolist()}, "
                    f"column {col}: got {float(g[i][col])!r} ref {float(ref[i][col])!r}")
    if nan_rows is not None:
        notnan = (~torch.isnan(g)).any(-1) & nan_rows
        if int(notnan.sum()):
            msgs.append(f"{name}: {int(notnan.sum())} rows of a NaN patch hold a number; first {notnan.nonzero()[:6].tolist()}")
    for m in msgs:
        if fails is None:
            raise AssertionError(m)
        fails.append(m)
    return len(msgs)


def check_bounds(name, got, ref, tol, mask, fails=None):
    """Every written element within tol of ref (NaN counts as outside); returns the worst err / tol."""
    w = ~mask
    return GR.check(name, got.cpu()[w], ref[w], tol[w], fails)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# which kernel, how many tiles: gemm_plan.h's documented rule and the launchers' grid rule, restated
# ---------------------------------------------------------------------------------------------------------------------------------------------
def auto_big(M, D):
    """gemm_plan.h, gemm_auto_big."""
    return M >= 512 and D >= 256 and ((M + 255) // 256) * ((D + 255) // 256) >= 48


def takes_two_phase(M, D, ps, tile):
    """The two-phase kernel is taken iff the tile is 7, or 0 with gemm_auto_big, and Kg >= 128 (csrc/gemm.hip, patch_embed_takes_pp2)."""
    return (tile == 7 or (tile == 0 and auto_big(M, D))) and kg_of(ps) >= 128


def tile_side(M, D, tile):
    """Row / column side of the output tile the call runs on."""
    if tile == 7 or tile == 256 or (tile == 0 and auto_big(M, D)):
        return 256
    return 128


def workgroups(tile_px):
    """Persistent grid of the kernel: one workgroup per CU for the 256 x 256 kernels (128 KiB of LDS), two for the 128 x 128 one."""
    return 256 if tile_px == 256 else 512


def geometry(B, S, ps, D, tile):
    """What a case reaches: K-tiles, K padding rows, a K-tile that straddles two channels, images under the first row tile, ragged tiles, tile count."""
    G = S // ps
    P = G * G
    M = B * P
    psp, Kg = psp_of(ps), kg_of(ps)
    side = tile_side(M, D, tile)
    rows_per_kt = BK // psp if psp <= BK else 0
    nkt = Kg // BK
    straddle = False
    if psp != ps and rows_per_kt > 1:
        for kt in range(nkt):
            r0, r1 = kt * rows_per_kt, min(3 * ps - 1, (kt + 1) * rows_per_kt - 1)
            if r0 < 3 * ps and r0 // ps != r1 // ps:
                straddle = True
    tiles_m, tiles_n = (M + side - 1) // side, (D + side - 1) // side
    first_tile_rows = min(M, side)
    return dict(M=M, P=P, ktiles=nkt, k_pad_rows=(Kg - 3 * ps * psp) // psp, straddle=straddle,
                images_in_first_tile=(first_tile_rows - 1) // P + 1, ragged_rows=M % side != 0, ragged_cols=D % side != 0,
                tiles=tiles_m * tiles_n, tiles_m=tiles_m, persistent=tiles_m * tiles_n > workgroups(side), side=side)


def scratch_bytes(B, S, ps, D, tile):
    """owl_patch_embed_scratch_bytes: a host call (no device)."""
    from owl_vit_object_detection_amd import _lib
    n = torch.zeros(1, dtype=torch.int64)
    _lib.call("owl_patch_embed_scratch_bytes", B, S, ps, D, tile, n)
    return int(n.item())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the GPU case lists (tests/test_embed_reference_gpu.py runs them, tests/test_embed_reference.py shows what they reach)
# (ps, G, B, D, Tp rule): Tp rule None = P + 1 rounded up to 8, else the number of rows beyond T
# ---------------------------------------------------------------------------------------------------------------------------------------------
EVERY_PS = [(ps, 3, 3, 136, "tp16") for ps in PATCH_SIZES]                 # Tp = 16: M = 27, one ragged tile over three images
ROW_PS = (8, 14, 16, 36)
ROW_GB = [(1, 1), (2, 1), (16, 1), (16, 2), (5, 12), (7, 6)]
ROW_GEOMETRY = [(ps, G, B, 128, None) for ps in ROW_PS for (G, B) in ROW_GB] + [(14, 5, 3, 128, 0), (16, 5, 3, 128, 16)]
COL_GEOMETRY = [(ps, 5, 3, D, None) for ps in (16, 14) for D in (8, 72, 128, 264, 520)]
TILE_WALK = [(8, 64, 17, 128, None), (10, 64, 17, 128, None)]              # S = 512 / 640: M = 69 632, 272 row tiles of 256
AUTO = [(8, 32, 12, 256, None, True), (8, 32, 11, 256, None, False)]       # S = 256: M = 12 288 / 11 264 -> 48 / 44 tiles of 256
POISON_PS = (8, 10, 14, 16, 22, 36, 64)
BOUND_PS = (14, 16, 32)
BOUND_CASE = dict(B=3, G=6, D=128)
ALIGN8 = dict(ps=14, S=42, B=2, D=128)                                     # image[1:] of B + 1 images: base 3 * 42 * 42 * 2 = 10 584 bytes in, 8 mod 16
BIG = dict(ps=64, S=1024, B=344, D=64, images=(0, 340, 341, 342, 343))    # 344 * 3 * 1024^2 * 2 = 2.16e9 bytes; byte 2^31 lies in image 341


def tp_rule(P, rule):
    if rule == "tp16":
        return 16
    return tp_of(P, rule)
