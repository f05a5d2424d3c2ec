"""-m gpu: the rectangular entries of the C ABI -- owl_patch_embed_bf16_hw on each of its kernels, owl_im2row_bf16_hw, owl_pos_resample_hw /
owl_pos_resample_bwd_hw -- against the float64 references of tests/rect_reference.py.

Patch embedding: the `integers` profile of tests/embed_reference.py on rectangles (every f32 partial sum is exact in any order: torch.equal against the
float64 conv), into a sentinel buffer with one extra image block, from an image batch with one extra image of NaN, the scratch sized by
owl_patch_embed_scratch_bytes_hw and started as NaN.  Position table: inside the derived bounds of rect_reference (nothing excluded); each case prints
its worst err / tol (profiles/rect_inputs_reference.md).  tests/test_rect_reference.py shows on the CPU that these inputs reject the planted errors."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import _lib, ops, weights  # noqa: E402
from tests import embed_reference as EM  # noqa: E402
from tests import pos_resample_reference as R  # noqa: E402
from tests import rect_reference as RR  # noqa: E402

DEV = "cuda"
NAN = float("nan")
PINS = (0, 7, 256, 128)


# ---- patch embedding ------------------------------------------------------------------------------------------------------------------------------
def _launch(img_dev, wk, pos_dev, B, H, W, ps, D, Tp, tile):
    n = RR.scratch_bytes_hw(B, H, W, ps, D, tile)
    if tile != 0:
        assert (n == 0) == (EM.psp_of(ps) == ps or tile == 7), (ps, tile, n)
    scratch = torch.full((n // 2,), NAN, dtype=torch.bfloat16, device=DEV) if n else None
    x = EM.sentinel((B + 1, Tp, D), DEV)
    ops.patch_embed_hw(img_dev, wk, pos_dev, x.view((B + 1) * Tp, D), B, H, W, ps, D, Tp, scratch=scratch, tile=tile)
    torch.cuda.synchronize()
    return x


def _device_inputs(img, w, pos, ps):
    B, _, H, W = img.shape
    img_dev = torch.full((B + 1, 3, H, W), NAN, dtype=torch.bfloat16, device=DEV)
    img_dev[:B] = img.to(DEV)
    wk = weights.patch_weight_gather_layout(w, ps).contiguous().to(DEV)
    return img_dev, wk, pos.to(DEV)


@pytest.mark.parametrize("D", RR.EMBED_D)
@pytest.mark.parametrize("ps,H,W", RR.EMBED_SHAPES, ids=[f"ps{c[0]}-{c[1]}x{c[2]}" for c in RR.EMBED_SHAPES])
def test_patch_embed_is_exact_on_every_pin(ps, H, W, D):
    """Exact on every kernel pin, the same bits across the pins, and a NaN patch stays in its own row (an interior-column patch of image 1 and its last)."""
    B = RR.EMBED_B
    gh, gw = H // ps, W // ps
    P = gh * gw
    Tp = EM.tp_of(P)
    base, w, pos = RR.make_integers_hw(B, H, W, ps, D)
    EM.assert_exact_ok(base, w, pos)
    poisoned = (1, P - 1)
    for label, img, nan_of in (("plain", base, None), ("poison", RR.poison_patch_hw(RR.poison_patch_hw(base, 1, poisoned[0], ps), 1, poisoned[1], ps), poisoned)):
        ref, mask = EM.exact(img, w, pos, Tp)
        nan_rows = torch.isnan(ref).any(-1) if nan_of else None
        if nan_of:
            assert sorted(nan_rows.nonzero().tolist()) == sorted([1, 1 + p] for p in nan_of)
        img_dev, wk, pos_dev = _device_inputs(img, w, pos, ps)
        fails, outs = [], {}
        for tile in PINS:
            x = _launch(img_dev, wk, pos_dev, B, H, W, ps, D, Tp, tile)
            name = f"{label} ps={ps} {H}x{W} D={D} tile={tile}"
            EM.check_untouched(name, x, mask, fails)
            EM.check_exact(name, x, ref, mask, fails, nan_rows=nan_rows)
            outs[tile] = x
        assert not fails, "\n".join(fails)
        for tile in PINS[1:]:
            assert torch.equal(EM.bits(outs[tile]), EM.bits(outs[0])), f"{label}: tile {tile} differs from the automatic choice"


@pytest.mark.parametrize("ps,S", [(16, 48), (14, 42), (8, 24)])
def test_patch_embed_hw_of_a_square_is_bitwise_the_square_entry(ps, S):
    B, D = 3, 128
    P = (S // ps) ** 2
    Tp = EM.tp_of(P)
    img, w, pos = EM.make_inputs("clip_pixels", B, S, ps, D)
    img_dev, wk, pos_dev = _device_inputs(img, w, pos, ps)
    for tile in PINS:
        x = _launch(img_dev, wk, pos_dev, B, S, S, ps, D, Tp, tile)
        n = EM.scratch_bytes(B, S, ps, D, tile)
        assert n == RR.scratch_bytes_hw(B, S, S, ps, D, tile)
        scratch = torch.full((n // 2,), NAN, dtype=torch.bfloat16, device=DEV) if n else None
        y = EM.sentinel((B + 1, Tp, D), DEV)
        ops.patch_embed(img_dev, wk, pos_dev, y.view((B + 1) * Tp, D), B, S, ps, D, Tp, scratch=scratch, tile=tile)
        torch.cuda.synchronize()
        assert torch.equal(EM.bits(x), EM.bits(y)), f"ps={ps} tile={tile}"


def test_patch_embed_offsets_above_2_31_bytes_on_a_rectangle():
    """344 images of 3 x 512 x 2048 bf16 = 2.16e9 bytes: images 341 .. 343 lie above byte 2^31.  The channel stride is H W = 2^20 elements; W W = 2^22
    would leave the image, and a 32-bit product formed with it the batch."""
    c = RR.BIG
    ps, H, W, B, D = c["ps"], c["H"], c["W"], c["B"], c["D"]
    P = (H // ps) * (W // ps)
    Tp = EM.tp_of(P)
    assert 2 ** 31 + 2 * 3 * H * W * 2 < B * 3 * H * W * 2 < 2 ** 32 and 341 * 3 * H * W * 2 < 2 ** 31 < 342 * 3 * H * W * 2
    _, w, pos = RR.make_integers_hw(1, H, W, ps, D)
    img_dev = torch.empty((B + 1, 3, H, W), dtype=torch.bfloat16, device=DEV)
    img_dev[:B] = RR.device_integers_hw(B, H, W, 5, DEV)
    img_dev[B] = NAN
    pick = list(c["images"])
    sub = img_dev[pick].cpu()
    assert float(sub.float().abs().max()) == 8.0 and not torch.equal(sub[1], sub[2])
    EM.assert_exact_ok(sub, w, pos)
    ref, _ = EM.exact(sub, w, pos, Tp, extra_images=0)
    wk = weights.patch_weight_gather_layout(w, ps).contiguous().to(DEV)
    mask = torch.ones(B + 1, Tp, dtype=torch.bool)
    mask[:B, 1:P + 1] = False
    fails = []
    for tile in (7, 128):
        x = _launch(img_dev, wk, pos.to(DEV), B, H, W, ps, D, Tp, tile)
        EM.check_untouched(f"big tile={tile}", x, mask, fails)
        got = x[pick].cpu().double()
        bad = (got[:, 1:P + 1] != ref[:, 1:P + 1]).any(-1)
        if bool(bad.any()):
            fails.append(f"big tile={tile}: images {sorted({pick[i] for i in bad.nonzero()[:, 0].tolist()})} differ from the exact reference "
                         f"({int(bad.sum())} rows; first (slot, patch) {bad.nonzero()[:4].tolist()})")
        del x
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("ps,H,W", RR.EMBED_SHAPES + ((2, 6, 10), (64, 64, 192)), ids=lambda v: str(v))
def test_im2row_hw_is_a_bit_exact_copy(ps, H, W):
    B = 2
    P, K = (H // ps) * (W // ps), 3 * ps * ps
    ld = (K + 7) // 8 * 8 + 8
    g = torch.Generator().manual_seed(ps + H)
    img = torch.randint(-2 ** 15, 2 ** 15, (B, 3, H, W), generator=g, dtype=torch.int32).to(torch.int16)      # every bf16 bit pattern
    img_dev = torch.full((B + 1, 3, H, W), 0x7FC1, dtype=torch.int16, device=DEV)
    img_dev[:B] = img.to(DEV)
    SENT = 0x4B5A
    out = torch.full((B * P + 3, ld), SENT, dtype=torch.int16, device=DEV)
    ops.im2row_bf16_hw(img_dev.view(torch.bfloat16), out.view(torch.bfloat16), B, H, W, ps)
    torch.cuda.synchronize()
    ref = RR.patches_of_hw(img, ps).reshape(B * P, K)
    got = out.cpu()
    assert torch.equal(got[:B * P, :K], ref), f"the copy differs at {(got[:B * P, :K] != ref).nonzero()[:4].tolist()}"
    assert bool((got[:B * P, K:] == SENT).all()) and bool((got[B * P:] == SENT).all())
    if H == W:
        sq = torch.full_like(out, SENT)
        ops.im2row_bf16(img_dev.view(torch.bfloat16), sq.view(torch.bfloat16), B, H, ps)
        assert torch.equal(sq, out)


def test_im2row_hw_of_a_square_is_bitwise_the_square_entry():
    for ps, S in ((16, 48), (14, 42)):
        B, P, K = 2, (S // ps) ** 2, 3 * ps * ps
        img = torch.randn(B, 3, S, S, device=DEV).bfloat16()
        a = torch.zeros(B * P, (K + 7) // 8 * 8, dtype=torch.bfloat16, device=DEV)
        b = torch.zeros_like(a)
        ops.im2row_bf16(img, a, B, S, ps)
        ops.im2row_bf16_hw(img, b, B, S, S, ps)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---- position table ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g0,gh,gw,D", RR.POS_SHAPES)
def test_pos_resample_hw_forward_and_adjoint_against_float64(g0, gh, gw, D):
    pos, dU, old = RR.make_case_hw(g0, gh, gw, D)
    T0, T = g0 * g0 + 1, gh * gw + 1
    outs = []
    for _ in range(2):
        out = torch.full((T + 1, D), NAN, device=DEV)          # one sentinel row past the table
        ops.pos_resample_hw(pos.to(DEV), out, g0, gh, gw, D)
        dpos = torch.cat([old, torch.full((1, D), NAN)]).to(DEV)          # NON-ZERO: the adjoint adds onto what is there
        ops.pos_resample_bwd_hw(dU.to(DEV), dpos, g0, gh, gw, D)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[T]).all()) and bool(torch.isnan(dpos[T0]).all())
        outs.append((out[:T].cpu(), dpos[:T0].cpu()))
    (u, dp), (u2, dp2) = outs
    assert torch.equal(u, u2) and torch.equal(dp, dp2)          # two runs, the same bits
    assert torch.equal(u[0], pos[0])
    r_f = R.check(f"forward {g0}->{gh}x{gw} D={D}", u, RR.forward64_hw(pos, g0, gh, gw), RR.bound_fwd_hw(pos, g0, gh, gw))
    ref_b, tol_b = old.double() + RR.adjoint64_hw(dU, g0, gh, gw), RR.bound_bwd_hw(dU, old, g0, gh, gw)
    r_b = R.check(f"backward {g0}->{gh}x{gw} D={D}", dp, ref_b, tol_b)
    r_b_patch = float(R.ratios(dp[1:], ref_b[1:], tol_b[1:]).max())
    print(f"RECTREF pos_resample_hw g0={g0} gh={gh} gw={gw} D={D}: worst err / tol forward {r_f:.3f}, backward {r_b:.4f} (patch rows {r_b_patch:.3f})")
    assert r_f < 1.0 and r_b < 1.0


@pytest.mark.parametrize("g0,g,D", [(6, 8, 128), (6, 4, 64), (3, 7, 64)])
def test_pos_resample_hw_of_a_square_is_bitwise_the_square_entry(g0, g, D):
    pos, dU, old = R.make_case(g0, g, D)
    a, b = torch.zeros(g * g + 1, D, device=DEV), torch.zeros(g * g + 1, D, device=DEV)
    ops.pos_resample(pos.to(DEV), a, g0, g, D)
    ops.pos_resample_hw(pos.to(DEV), b, g0, g, g, D)
    da, db = old.to(DEV), old.to(DEV)
    ops.pos_resample_bwd(dU.to(DEV), da, g0, g, D)
    ops.pos_resample_bwd_hw(dU.to(DEV), db, g0, g, g, D)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(da, db) and float(a.abs().max()) > 0


# ---- refused arguments: each raises before any launch ---------------------------------------------------------------------------------------------------
def test_refused_arguments():
    x = torch.zeros(4096, device=DEV)
    xb = torch.zeros(4096, dtype=torch.bfloat16, device=DEV)
    n = torch.zeros(1, dtype=torch.int64)
    s = ops.stream()

    def embed(B, H, W, ps, D, Tp, tile=0):
        _lib.call("owl_patch_embed_bf16_hw", s, xb, xb, x, x, None, B, H, W, ps, D, Tp, tile)

    for args, what in (((1, 40, 32, 16, 64, 8), "multiple of the patch size"), ((1, 32, 40, 16, 64, 8), "multiple of the patch size"),
                       ((1, 30, 45, 15, 64, 8), "patch size even"), ((1, 12, 18, 6, 64, 8), "8 <= patch size"), ((1, 66, 132, 66, 64, 8), "patch size <= 64"),
                       ((1, 32, 48, 16, 64, 6), "Tp"), ((1, 32, 48, 16, 60, 8), "D % 8"),
                       ((342, 1024, 2048, 64, 64, 520), "beyond 4 GiB"), ((0, 32, 48, 16, 64, 8), "beyond 4 GiB"), ((1, 32, 48, 16, 64, 8, 5), "tile must be")):
        with pytest.raises(_lib.OwlLibError, match=what):
            embed(*args)
    for args in ((1, 40, 32, 16, 64), (1, 32, 40, 16, 64), (1, 30, 45, 15, 64), (0, 32, 48, 16, 64)):
        with pytest.raises(_lib.OwlLibError, match="bad arguments"):
            _lib.call("owl_patch_embed_scratch_bytes_hw", args[0], args[1], args[2], args[3], args[4], 0, n)
    for args in ((1, 40, 32, 16), (1, 32, 40, 16), (1, 30, 45, 15), (1, 16, 8208, 16)):
        with pytest.raises(_lib.OwlLibError, match="divides the image size"):
            _lib.call("owl_im2row_bf16_hw", s, xb, xb, 768, *args)
    with pytest.raises(_lib.OwlLibError, match="ld_out"):
        _lib.call("owl_im2row_bf16_hw", s, xb, xb, 760, 1, 32, 48, 16)
    for name in ("owl_pos_resample_hw", "owl_pos_resample_bwd_hw"):
        for g0, gh, gw, D in ((0, 4, 8, 64), (6, 0, 8, 64), (6, 4, 0, 64), (6, 257, 4, 64), (6, 4, 257, 64), (257, 4, 8, 64)):
            with pytest.raises(_lib.OwlLibError, match="side 1 .. 256"):
                _lib.call(name, s, x, x, g0, gh, gw, D)
        with pytest.raises(_lib.OwlLibError, match="multiple of 8"):
            _lib.call(name, s, x, x, 6, 4, 8, 12)
    with pytest.raises(ValueError, match="must hold"):
        ops.pos_resample_hw(x[:37 * 8].view(37, 8), x[:30 * 8].view(30, 8), 6, 4, 8, 8)
    with pytest.raises(ValueError, match="must hold"):
        ops.im2row_bf16_hw(xb[:3 * 32 * 48], xb[:5 * 768].view(5, 768), 1, 32, 48, 16)
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0 and float(xb.float().abs().max()) == 0.0          # nothing was launched onto the buffers
