"""Float64 references and derived bounds for rectangular inputs: the position table [g0 g0 + 1, D] resampled onto a gh x gw grid
(owl_pos_resample_hw / owl_pos_resample_bwd_hw), the box bias of a gh x gw grid (models.box_bias_table(gh, gw)) and the patch embedding of an image
[B, 3, H, W] (owl_patch_embed_bf16_hw, owl_im2row_bf16_hw).  Checker side; nothing here imports the package's Python ops.

Position table.  tests/pos_resample_reference.py already works per axis: `tap_matrix(g0, g)` is M [g, g0].  The rectangular table's patch rows are
(My (x) Mx) pos_patch with My = tap_matrix(g0, gh), Mx = tap_matrix(g0, gw), row 1 + y gw + x (HF: interpolate(size=(gh, gw), mode="bicubic",
align_corners=False) on the [g0, g0, D] patch rows; tests/test_rect_reference.py holds `forward64_hw` to torch and to live transformers).  The bounds
are pos_resample_reference's with one tap matrix per axis; the rounding count per element is unchanged -- 16 fmaf forward, ny nx + 1 on a source cell's
chain (ny, nx: `touch_counts` of the y axis with gh, of the x axis with gw).

Box bias.  HF's compute_box_bias(num_patches_height, num_patches_width) in float64: x / gw, y / gh, size bias (1 / gw, 1 / gh), rows p = y gw + x.

Patch embedding.  tests/embed_reference.py's `exact` (a float64 conv2d) takes a rectangle as it is; this module adds the rectangular input maker, the
patch poisoner and the patch-major copy the im2row test compares with.

`wrong_*` build what the PLANTED ERRORS of the issue would compute; tests/test_rect_reference.py shows that each misses the bound or the exact
comparison on the GPU cases' own inputs (profiles/rect_inputs_reference.md lists them)."""
import numpy as np
import torch

from tests import embed_reference as EM
from tests import pos_resample_reference as R
from tests.gemm_reference import F, TINY, gamma as gam

# (g0, gh, gw, D) of tests/test_rect_kernels_gpu.py, the grids of the CPU test (g0 = 6) and of the fixture
POS_SHAPES = ((6, 6, 10, 128), (6, 10, 6, 128), (6, 4, 9, 128), (6, 4, 8, 64), (6, 1, 7, 64), (6, 7, 1, 64), (1, 3, 5, 64), (6, 8, 6, 128), (24, 16, 40, 768))
CPU_GRIDS = ((6, 10), (10, 6), (4, 9), (4, 8), (1, 7), (7, 1), (8, 6))
FIXTURE_GRIDS = ((6, 10), (10, 6), (4, 9), (7, 1))
# (ps, H, W) of the patch-embedding cases
EMBED_SHAPES = ((16, 32, 80), (16, 80, 32), (8, 16, 40), (14, 28, 70), (14, 70, 28))
EMBED_B, EMBED_D = 3, (64, 128)
# byte offsets above 2^31 on a rectangle, shaped after embed_reference.BIG: 344 images of 3 x 512 x 2048 bf16 = 2.16e9 bytes
BIG = dict(ps=64, H=512, W=2048, B=344, D=64, images=(0, 340, 341, 342, 343))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# position table
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _kron(My, Mx, rows, ny, nx):
    """rows [ny nx, D] (row y nx + x) -> (My (x) Mx) rows, My [oy, ny], Mx [ox, nx] -> [oy ox, D]."""
    D = rows.shape[-1]
    return torch.einsum("yi,xj,ijd->yxd", My, Mx, rows.reshape(ny, nx, D)).reshape(-1, D)


def forward64_hw(pos, g0, gh, gw):
    """pos [g0 g0 + 1, D] -> U [gh gw + 1, D] float64, row 1 + y gw + x."""
    pos = pos.double()
    return torch.cat([pos[:1], _kron(R.tap_matrix(g0, gh), R.tap_matrix(g0, gw), pos[1:], g0, g0)], 0)


def adjoint64_hw(dU, g0, gh, gw):
    """dU [gh gw + 1, D] -> K^T dU [g0 g0 + 1, D] float64."""
    dU = dU.double()
    return torch.cat([dU[:1], _kron(R.tap_matrix(g0, gh).t().contiguous(), R.tap_matrix(g0, gw).t().contiguous(), dU[1:], gh, gw)], 0)


def _axis(g0, g):
    """Per axis: Ma (|w| + E_w scattered), Mw (|w| scattered), both [g, g0]."""
    idx, w, E = R.axis_weights(g0, g)
    return R._scatter(idx, w.abs() + E, g0), R._scatter(idx, w.abs(), g0)


def bound_fwd_hw(pos, g0, gh, gw):
    """tolerance [gh gw + 1, D] of owl_pos_resample_hw against forward64_hw on the same f32 table (pos_resample_reference.bound_fwd, one matrix per axis)."""
    (May, Mwy), (Max, Mwx) = _axis(g0, gh), _axis(g0, gw)
    pa = pos.double().abs()
    tol = (1.0 + gam(R.N_FWD)) * (1.0 + F) * _kron(May, Max, pa[1:], g0, g0) - _kron(Mwy, Mwx, pa[1:], g0, g0) + TINY * (1.0 + 17.0 * float(pa.max()))
    return torch.cat([torch.zeros_like(pa[:1]), tol], 0)


def _axis_bwd(g0, g):
    """Per axis: A'^T = (|m| + E_m)^T and |M|^T, both [g0, g] (pos_resample_reference.bound_bwd)."""
    idx, w, E = R.axis_weights(g0, g)
    k = R._scatter(idx, torch.ones_like(w), g0)
    M = R._scatter(idx, w, g0)
    Em = R._scatter(idx, E, g0) + gam((k - 1.0).clamp_min(0.0)) * R._scatter(idx, w.abs() + E, g0)
    return (M.abs() + Em).t().contiguous(), M.abs().t().contiguous()


def bound_bwd_hw(dU, old, g0, gh, gw):
    """tolerance [g0 g0 + 1, D] of owl_pos_resample_bwd_hw against old + adjoint64_hw(dU): n = ny nx + 1 roundings on a source cell's chain."""
    (Aty, Mty), (Atx, Mtx) = _axis_bwd(g0, gh), _axis_bwd(g0, gw)
    n = (R.touch_counts(g0, gh).double()[:, None] * R.touch_counts(g0, gw).double()[None, :]).reshape(-1, 1) + 1.0
    da, oa = dU.double().abs(), old.double().abs()
    tol = (1.0 + gam(n)) * (1.0 + F) * _kron(Aty, Atx, da[1:], gh, gw) - _kron(Mty, Mtx, da[1:], gh, gw) + gam(n) * oa[1:] \
        + TINY * (1.0 + 2.0 * float(n.max()) * float(da.max()))
    return torch.cat([gam(1) * (da[:1] + oa[:1]) + TINY, tol], 0)


def make_case_hw(g0, gh, gw, D, seed=0):
    """pos_resample_reference.make_case for a rectangle: pos [g0 g0 + 1, D], dU [gh gw + 1, D], old [g0 g0 + 1, D], f32, a trained-like table (std 0.02
    with two outliers of 60) so that a tolerance relative to max |pos| would hide the rest."""
    gen = torch.Generator(device="cpu").manual_seed(1000003 * seed + 10007 * g0 + 101 * gh + 13 * gw + D)
    pos = 0.02 * torch.randn(g0 * g0 + 1, D, generator=gen)
    pos[1 + (g0 * g0) // 2, D // 3] = 60.0
    pos[g0 * g0, D - 1] = -60.0
    dU = torch.randn(gh * gw + 1, D, generator=gen)
    old = torch.randn(g0 * g0 + 1, D, generator=gen) * float(max(gh, gw)) / float(g0)
    return pos.float(), dU.float(), old.float()


def _tap_matrix_at(g0, g, n_out):
    """tap_matrix's rows for output indices 0 .. n_out - 1 evaluated with grid g (n_out != g: what a kernel that takes an axis' taps with the OTHER side computes)."""
    o = torch.arange(n_out, dtype=torch.int64)
    num, den = (2 * o + 1) * g0 - g, 2 * g
    f = torch.div(num, den, rounding_mode="floor")
    t = (num - f * den).double() / den
    w = torch.stack([R._c2(t + 1.0, R.A), R._c1(t, R.A), R._c1(1.0 - t, R.A), R._c2(2.0 - t, R.A)], 1)
    return R._scatter((f[:, None] - 1 + torch.arange(4)).clamp(0, g0 - 1), w, g0)


POS_ERRORS = ("y_taps_with_gw", "row_stride_g0", "row_stride_gh", "transposed", "skipped_at_equal_P")


def wrong_forward(pos, g0, gh, gw, kind):
    """The table a planted error would write into a zeroed [gh gw + 1, D] buffer (stores past the table dropped, later stores win)."""
    pos = pos.double()
    if kind == "skipped_at_equal_P":
        return pos.clone() if gh * gw == g0 * g0 else forward64_hw(pos, g0, gh, gw)
    My = _tap_matrix_at(g0, gw, gh) if kind == "y_taps_with_gw" else R.tap_matrix(g0, gh)
    val = _kron(My, R.tap_matrix(g0, gw), pos[1:], g0, g0).reshape(gh, gw, -1)
    out = torch.zeros(gh * gw + 1, pos.shape[1], dtype=torch.float64)
    out[0] = pos[0]
    for y in range(gh):
        for x in range(gw):
            row = {"row_stride_g0": 1 + y * g0 + x, "row_stride_gh": 1 + y * gh + x, "transposed": 1 + x * gh + y}.get(kind, 1 + y * gw + x)
            if row < out.shape[0]:
                out[row] = val[y, x]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# box bias
# ---------------------------------------------------------------------------------------------------------------------------------------------
BOX_ERRORS = ("x_over_gh", "sizes_swapped")


def box_bias_hw(gh, gw, wrong=None, raw=False):
    """HF compute_box_bias(gh, gw) in float64 -> [gh gw, 4], row y gw + x: (x / gw, y / gh) through log(c + 1e-4) - log1p(-c + 1e-4), then the same of
    the size (1 / gw, 1 / gh).  `wrong`: a planted error (BOX_ERRORS)."""
    x = torch.arange(1, gw + 1, dtype=torch.float64) / (gh if wrong == "x_over_gh" else gw)
    y = torch.arange(1, gh + 1, dtype=torch.float64) / gh
    c = torch.stack([x[None, :].expand(gh, gw), y[:, None].expand(gh, gw)], -1).reshape(-1, 2).clamp(0.0, 1.0)
    s = torch.tensor([1.0 / gw, 1.0 / gh] if wrong != "sizes_swapped" else [1.0 / gh, 1.0 / gw], dtype=torch.float64).expand(gh * gw, 2)
    if raw:          # the four arguments of the log pair (box_bias_tol)
        return torch.cat([c, s], -1)
    b = lambda v: torch.log(v + 1e-4) - torch.log1p(-v + 1e-4)
    return torch.cat([b(c), b(s)], -1)


def box_bias_tol(gh, gw):
    """Elementwise f32 round-off of HF's (and the product's) f32 evaluation against box_bias_hw: the f32 value v~ of v = c or 1 / g is within 2^-24 v,
    v~ + 1e-4 and -v~ + 1e-4 each round once more (arguments <= 1: 2^-24 absolute), so d log(v + 1e-4) <= 3 * 2^-24 / (v + 1e-4) and
    d log1p(-v + 1e-4) <= 3 * 2^-24 / (1 - v + 1e-4) -- 6e-4 relative at v = 1, the last cell of an axis --, plus an ulp of each log (|log| < 9.3) and of
    their difference: 4 * 2^-24 * 9.3."""
    v = box_bias_hw(gh, gw, raw=True)
    return 3.0 * 2.0 ** -24 * (1.0 / (v + 1e-4) + 1.0 / (1.0 - v + 1e-4)) + 4.0 * 2.0 ** -24 * 9.3


# ---------------------------------------------------------------------------------------------------------------------------------------------
# patch embedding
# ---------------------------------------------------------------------------------------------------------------------------------------------
def make_integers_hw(B, H, W, ps, D, seed=0):
    """embed_reference's `integers` profile on a rectangle: (image bf16 [B, 3, H, W], w bf16 [D, 3, ps, ps], pos f32 [gh gw + 1, D]); every f32 partial
    sum in any order is exact (EM.assert_exact_ok)."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * ps + B + 3 * H + 7 * W + D)
    P = (H // ps) * (W // ps)
    img = torch.randint(-8, 9, (B, 3, H, W), generator=g).bfloat16()
    w = torch.randint(-8, 9, (D, 3, ps, ps), generator=g).bfloat16()
    pos = torch.randint(-2 ** 16, 2 ** 16 + 1, (P + 1, D), generator=g).float()
    return img, w, pos


def patches_of_hw(img, ps):
    """[B, 3, H, W] -> [B gh gw, 3, ps, ps], row (b gh + py) gw + px."""
    B, C, H, W = img.shape
    gh, gw = H // ps, W // ps
    return img.reshape(B, C, gh, ps, gw, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, C, ps, ps)


def poison_patch_hw(img, b, p, ps):
    """A copy of img with every pixel of patch p = py gw + px of image b NaN."""
    out = img.clone()
    py, px = divmod(p, img.shape[-1] // ps)
    out[b, :, py * ps:(py + 1) * ps, px * ps:(px + 1) * ps] = float("nan")
    return out


def device_integers_hw(B, H, W, seed, device):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(-8, 9, (B, 3, H, W), generator=g, device=device, dtype=torch.int8).bfloat16()


EMBED_ERRORS = ("patch_order_x_gh_y", "channel_stride_WW")


def wrong_embed(img, w, pos, Tp, kind):
    """EM.exact's ref for a planted gather error: `patch_order_x_gh_y` stores patch (py, px) in row 1 + px gh + py; `channel_stride_WW` reads channel c of a
    patch W W elements behind channel 0 instead of H W (addresses taken modulo the batch: a CPU stand-in for whatever lies there)."""
    B, _, H, W = img.shape
    ps = w.shape[-1]
    gh, gw = H // ps, W // ps
    if kind == "patch_order_x_gh_y":
        acc = EM.conv64(img, w).reshape(B, gh, gw, -1).transpose(1, 2).reshape(B, gh * gw, -1)
    else:
        flat = img.double().reshape(-1)
        b, c, py, px, ky, kx = torch.meshgrid(torch.arange(B), torch.arange(3), torch.arange(gh), torch.arange(gw), torch.arange(ps), torch.arange(ps), indexing="ij")
        addr = ((b * 3) * H + py * ps + ky) * W + px * ps + kx + c * W * W
        pt = flat[addr % flat.numel()].permute(0, 2, 3, 1, 4, 5).reshape(B, gh * gw, 3 * ps * ps)
        acc = pt @ w.double().reshape(w.shape[0], -1).t()
    ref = torch.zeros(B + 1, Tp, w.shape[0], dtype=torch.float64)
    ref[:B, 1:gh * gw + 1] = acc + pos.double()[1:]
    return ref


def scratch_bytes_hw(B, H, W, ps, D, tile):
    """owl_patch_embed_scratch_bytes_hw: a host call (no device)."""
    from owl_vit_object_detection_amd import _lib
    n = torch.zeros(1, dtype=torch.int64)
    _lib.call("owl_patch_embed_scratch_bytes_hw", B, H, W, ps, D, tile, n)
    return int(n.item())


def np64(t):
    return np.asarray(t, dtype=np.float64)
