"""-m gpu: owl_patch_embed_bf16 on each of its kernels -- the two-phase ping-pong kernel's image gather (csrc/gemm_pp2.hip, stage_A), the single-phase
kernels' own gather at 2^n patch sizes and their explicit im2row + EPI_PATCHM_F32 elsewhere (csrc/gemm.hip) -- against the float64 / int64 reference and
the derived bounds of tests/embed_reference.py, at EVERY even patch size 8 .. 64; and owl_im2row_bf16 at every even patch size 2 .. 64.

Every call: x_out carries one extra image block and starts at a NaN-free sentinel bit pattern (row 0 of every image, the pad rows T .. Tp - 1 and the
extra block must keep it: the old pad check ran on zeros and could not see a stray store of zeros); the image carries one extra image of NaN; the
scratch buffer has the size owl_patch_embed_scratch_bytes answers (0 for 2^n sizes and for tile 7, non-zero otherwise) and starts as NaN.  The
`integers` profile is compared with torch.equal (every f32 partial sum is exact in any order), the float profiles element by element with `bounds`.
tests/test_embed_reference.py shows on the CPU what the shape lists reach and that the checks reject planted gather errors.  The EMBEDREF lines are the
worst err / tol per (kernel, patch size, profile): profiles/embed_reference.md."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import ops, weights  # noqa: E402
from tests import embed_reference as R  # noqa: E402

DEV = "cuda"
NAN = float("nan")


def _launch(img_dev, wk, pos_dev, B, S, ps, D, Tp, tile, expect_scratch=None):
    """One call into a sentinel buffer of B + 1 image blocks; img_dev holds B + 1 images (the last one NaN).  Returns x [B + 1, Tp, D] (device)."""
    n = R.scratch_bytes(B, S, ps, D, tile)
    pow2 = R.psp_of(ps) == ps
    if tile != 0:
        assert (n == 0) == (pow2 or tile == 7), (ps, tile, n)
    if expect_scratch is not None:
        assert (n != 0) == expect_scratch, (ps, tile, n)
    scratch = torch.full((n // 2,), NAN, dtype=torch.bfloat16, device=DEV) if n else None
    x = R.sentinel((B + 1, Tp, D), DEV)
    ops.patch_embed(img_dev, wk, pos_dev, x.view((B + 1) * Tp, D), B, S, ps, D, Tp, scratch=scratch, tile=tile)
    torch.cuda.synchronize()
    return x


def _device_inputs(img, w, pos, ps):
    B, _, S, _ = img.shape
    img_dev = torch.full((B + 1, 3, S, S), NAN, dtype=torch.bfloat16, device=DEV)
    img_dev[:B] = img.to(DEV)
    wk = weights.patch_weight_gather_layout(w, ps).contiguous().to(DEV)
    assert wk.shape == (w.shape[0], R.kg_of(ps))
    return img_dev, wk, pos.to(DEV)


def _exact_case(ps, G, B, D, Tp, tiles=R.TILES, img=None, nan_rows_of=None, tag=""):
    """`integers` on every kernel of `tiles`: written rows torch.equal the reference, the mask's rows keep the sentinel.  Returns the outputs."""
    S = G * ps
    base, w, pos = R.make_inputs("integers", B, S, ps, D)
    img = base if img is None else img(base)
    R.assert_exact_ok(base, w, pos)
    ref, mask = R.exact(img, w, pos, Tp)
    nan_rows = torch.isnan(ref).any(-1) if nan_rows_of else None
    if nan_rows_of:
        assert sorted(nan_rows.nonzero().tolist()) == sorted(nan_rows_of)
    img_dev, wk, pos_dev = _device_inputs(img, w, pos, ps)
    fails, outs = [], {}
    for tile in tiles:
        x = _launch(img_dev, wk, pos_dev, B, S, ps, D, Tp, tile)
        name = f"{tag} ps={ps} G={G} B={B} D={D} Tp={Tp} tile={tile}"
        R.check_untouched(name, x, mask, fails)
        R.check_exact(name, x, ref, mask, fails, nan_rows=nan_rows)
        outs[tile] = x
    assert not fails, "\n".join(fails)
    return outs


# ---- a. every even patch size, exact -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps,G,B,D,rule", R.EVERY_PS, ids=[f"ps{c[0]}" for c in R.EVERY_PS])
def test_every_even_patch_size_is_exact(ps, G, B, D, rule):
    _exact_case(ps, G, B, D, R.tp_rule(G * G, rule), tag="every-ps")


# ---- b. row geometry ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps,G,B,D,rule", R.ROW_GEOMETRY, ids=[f"ps{c[0]}-G{c[1]}-B{c[2]}-tp{c[4]}" for c in R.ROW_GEOMETRY])
def test_row_geometry_is_exact(ps, G, B, D, rule):
    _exact_case(ps, G, B, D, R.tp_rule(G * G, rule), tag="rows")


# ---- c. column geometry ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps,G,B,D,rule", R.COL_GEOMETRY, ids=[f"ps{c[0]}-D{c[3]}" for c in R.COL_GEOMETRY])
def test_column_geometry_is_exact(ps, G, B, D, rule):
    _exact_case(ps, G, B, D, R.tp_rule(G * G, rule), tag="cols")


# ---- d. more tiles than workgroups: a workgroup decodes a second tile and restarts its K walk ---------------------------------------------------------
@pytest.mark.parametrize("ps,G,B,D,rule", R.TILE_WALK, ids=[f"ps{c[0]}" for c in R.TILE_WALK])
def test_tile_walk_is_exact(ps, G, B, D, rule):
    for tile in R.TILES:
        assert R.geometry(B, G * ps, ps, D, tile)["persistent"]
    _exact_case(ps, G, B, D, R.tp_rule(G * G, rule), tag="walk")


# ---- e. the automatic choice, on both sides of its rule -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps,G,B,D,rule,big", R.AUTO, ids=["big", "not-big"])
def test_automatic_choice_is_exact_on_both_sides(ps, G, B, D, rule, big):
    M = B * G * G
    assert R.auto_big(M, D) == big
    # which side the LIBRARY is on: a patch size that is not 2^n with the same M and D needs no scratch exactly on the two-phase kernel
    assert (R.scratch_bytes(B, G * 10, 10, D, 0) == 0) == big
    outs = _exact_case(ps, G, B, D, R.tp_rule(G * G, rule), tiles=(0, 7, 128), tag="auto")
    assert torch.equal(outs[0], outs[7]) and torch.equal(outs[0], outs[128])
    # ... and at that other patch size itself, where the two sides are different code (gather | im2row + matrix)
    outs = _exact_case(10, G, B, D, R.tp_rule(G * G, rule), tiles=(0, 7), tag="auto")
    assert torch.equal(outs[0], outs[7])


# ---- f. a poisoned patch stays local ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", R.POISON_PS)
def test_poisoned_patch_stays_local(ps):
    """No read outside the patch, no garbage-times-zero: with the interior patch 4 and the corner patch 8 of image 1 NaN, exactly their rows are NaN -- in
    every column, zero weights included -- and every other row, their neighbours' included, is still bit-exact.  Covers the K padding rows (any row of the
    OWN patch) and the overlapping last chunk."""
    G, B, D = 3, 3, 136
    _exact_case(ps, G, B, D, 16, img=lambda im: R.poison_patch(R.poison_patch(im, 1, 4, ps), 1, 8, ps), nan_rows_of=[[1, 5], [1, 9]], tag="poison")


# ---- g. float64 bounds ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", R.FLOAT_PROFILES)
@pytest.mark.parametrize("ps", R.BOUND_PS)
def test_float_profiles_stay_inside_the_derived_bound(ps, profile):
    B, G, D = R.BOUND_CASE["B"], R.BOUND_CASE["G"], R.BOUND_CASE["D"]
    S, Tp = G * ps, R.tp_of(G * G)
    img, w, pos = R.make_inputs(profile, B, S, ps, D)
    ref, mask = R.exact(img, w, pos, Tp)
    tol = R.bounds(img, w, pos, Tp)
    img_dev, wk, pos_dev = _device_inputs(img, w, pos, ps)
    fails = []
    for tile in R.TILES + (0,):
        x = _launch(img_dev, wk, pos_dev, B, S, ps, D, Tp, tile)
        name = f"{profile} ps={ps} tile={tile}"
        R.check_untouched(name, x, mask, fails)
        worst = R.check_bounds(name, x, ref, tol, mask, fails)
        print(f"EMBEDREF tile={tile} ps={ps} profile={profile} worst_err_over_tol={worst:.4f}")
    assert not fails, "\n".join(fails)


# ---- h. same bits -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", R.BOUND_PS)
def test_same_bits_across_kernels_runs_and_batch_position(ps):
    B, G, D = R.BOUND_CASE["B"], R.BOUND_CASE["G"], R.BOUND_CASE["D"]
    S, Tp = G * ps, R.tp_of(G * G)
    img, w, pos = R.make_inputs("clip_pixels", B, S, ps, D)
    img_dev, wk, pos_dev = _device_inputs(img, w, pos, ps)
    one_dev, _, _ = _device_inputs(img[1:2], w, pos, ps)
    base = _launch(img_dev, wk, pos_dev, B, S, ps, D, Tp, 256)
    for tile in R.TILES:
        x = _launch(img_dev, wk, pos_dev, B, S, ps, D, Tp, tile)
        assert torch.equal(R.bits(x), R.bits(base)), f"tile {tile} differs from tile 256 at ps={ps}"
        assert torch.equal(R.bits(_launch(img_dev, wk, pos_dev, B, S, ps, D, Tp, tile)), R.bits(x)), f"tile {tile}: two runs differ"
        alone = _launch(one_dev, wk, pos_dev, 1, S, ps, D, Tp, tile)
        assert torch.equal(R.bits(alone[0]), R.bits(x[1])), f"tile {tile}: image 1 of 3 differs from the same image as a batch of 1"


# ---- i. an image view at 8-byte alignment --------------------------------------------------------------------------------------------------------------
def test_sliced_batch_at_8_byte_alignment_is_exact():
    """What a caller slicing a batch hands over: image[1:] of an allocation, 3 * 42 * 42 * 2 = 10 584 bytes in (8 mod 16)."""
    ps, S, B, D = R.ALIGN8["ps"], R.ALIGN8["S"], R.ALIGN8["B"], R.ALIGN8["D"]
    G = S // ps
    Tp = R.tp_of(G * G)
    img, w, pos = R.make_inputs("integers", B, S, ps, D)
    ref, mask = R.exact(img, w, pos, Tp)
    whole = torch.full((B + 2, 3, S, S), NAN, dtype=torch.bfloat16, device=DEV)          # image 0 (skipped) and the image behind the batch: NaN
    whole[1:B + 1] = img.to(DEV)
    view = whole[1:]
    assert (view.data_ptr() - whole.data_ptr()) == 10584 and view.data_ptr() % 16 == 8 and view.is_contiguous()
    wk = weights.patch_weight_gather_layout(w, ps).contiguous().to(DEV)
    fails = []
    for tile in R.TILES:
        x = _launch(view, wk, pos.to(DEV), B, S, ps, D, Tp, tile)
        R.check_untouched(f"align8 tile={tile}", x, mask, fails)
        R.check_exact(f"align8 tile={tile}", x, ref, mask, fails)
    assert not fails, "\n".join(fails)


# ---- j. gather byte offsets above 2^31 ----------------------------------------------------------------------------------------------------------------
def test_offsets_above_2_31_bytes_are_exact():
    """344 images of 3 x 1024 x 1024 bf16 = 2.16e9 bytes: images 341 .. 343 lie above byte 2^31 (341 contains it).  The width argument -- why no intermediate of
    the gathers exceeds 32 unsigned bits -- is in profiles/embed_reference.md; this is the run."""
    ps, S, B, D = R.BIG["ps"], R.BIG["S"], R.BIG["B"], R.BIG["D"]
    G = S // ps
    P = G * G
    Tp = R.tp_of(P)
    assert B * 3 * S * S * 2 > 2 ** 31 + 2 * 3 * S * S * 2 and B * 3 * S * S * 2 < 2 ** 32
    assert 341 * 3 * S * S * 2 < 2 ** 31 < 342 * 3 * S * S * 2
    _, w, pos = R.make_inputs("integers", 1, S, ps, D)
    img_dev = torch.empty((B + 1, 3, S, S), dtype=torch.bfloat16, device=DEV)
    img_dev[:B] = R.device_integers(B, S, 5, DEV)
    img_dev[B] = NAN
    pick = list(R.BIG["images"])
    sub = img_dev[pick].cpu()
    assert float(sub.float().abs().max()) == 8.0 and not torch.equal(sub[1], sub[2])
    R.assert_exact_ok(sub, w, pos)
    ref, _ = R.exact(sub, w, pos, Tp, extra_images=0)
    wk = weights.patch_weight_gather_layout(w, ps).contiguous().to(DEV)
    mask = torch.ones(B + 1, Tp, dtype=torch.bool)
    mask[:B, 1:P + 1] = False
    fails = []
    for tile in (7, 128):
        x = _launch(img_dev, wk, pos.to(DEV), B, S, ps, D, Tp, tile)
        R.check_untouched(f"big tile={tile}", x, mask, fails)
        got = x[pick].cpu().double()
        bad = (got[:, 1:P + 1] != ref[:, 1:P + 1]).any(-1)
        if bool(bad.any()):
            fails.append(f"big tile={tile}: images {sorted({pick[i] for i in bad.nonzero()[:, 0].tolist()})} differ from the int64 reference "
                         f"({int(bad.sum())} rows; first (slot, patch) {bad.nonzero()[:4].tolist()})")
        del x
    assert not fails, "\n".join(fails)


# ---- owl_im2row_bf16, the backward's operand: a bit-exact copy at every even patch size 2 .. 64 (both vector widths) -------------------------------
@pytest.mark.parametrize("ps", list(range(2, 65, 2)))
def test_im2row_is_a_bit_exact_copy_at_every_even_patch_size(ps):
    B, G = 2, 3
    S, P, K = G * ps, G * G, 3 * ps * ps
    ld = (K + 7) // 8 * 8 + 8
    g = torch.Generator().manual_seed(ps)
    img = torch.randint(-2 ** 15, 2 ** 15, (B, 3, S, S), generator=g, dtype=torch.int32).to(torch.int16)      # every bf16 bit pattern, NaNs included
    img_dev = torch.full((B + 1, 3, S, S), 0x7FC1, dtype=torch.int16, device=DEV)                             # + one image of (tagged) NaN behind the batch
    img_dev[:B] = img.to(DEV)
    SENT = 0x4B5A                                                                                             # bf16 14 286 848.0
    out = torch.full((B * P + 3, ld), SENT, dtype=torch.int16, device=DEV)
    ops.im2row_bf16(img_dev.view(torch.bfloat16), out.view(torch.bfloat16), B, S, ps)
    torch.cuda.synchronize()
    ref = R.patches_of(img, ps).reshape(B * P, K)
    got = out.cpu()
    assert torch.equal(got[:B * P, :K], ref), f"ps={ps}: the copy differs at {(got[:B * P, :K] != ref).nonzero()[:4].tolist()}"
    assert bool((got[:B * P, K:] == SENT).all()), f"ps={ps}: pad columns [{K}, {ld}) were written"
    assert bool((got[B * P:] == SENT).all()), f"ps={ps}: rows behind the last patch were written"
