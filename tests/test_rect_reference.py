"""CPU: the references of tests/rect_reference.py held to torch, to live transformers and to fixture F18 (tests/golden/make_golden_rect.py); the
planted errors of a rectangular grid shown to miss the bounds / the exact comparison on the GPU cases' own inputs; OwlConfig, check_image_size and
the input stage's host logic with a pair (height, width)."""
import os

import numpy as np
import pytest
import torch

from owl_vit_object_detection_amd import weights
from owl_vit_object_detection_amd.config import MAX_PATCHES, OwlConfig, check_image_size, get_config
from owl_vit_object_detection_amd.models import box_bias_table
from tests import embed_reference as EM
from tests import pos_resample_reference as R
from tests import rect_reference as RR

POS = "backbone.embeddings.position_embedding.weight"


@pytest.fixture(scope="module")
def f18(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "f18_rect.npz")))


def _interp(pos, g0, gh, gw):
    D = pos.shape[1]
    p = pos[1:].double().reshape(1, g0, g0, D).permute(0, 3, 1, 2)
    u = torch.nn.functional.interpolate(p, size=(gh, gw), mode="bicubic", align_corners=False).permute(0, 2, 3, 1).reshape(-1, D)
    return torch.cat([pos[:1].double(), u], 0)


def _check_tables(pos, hf_table, hf_bias, gh, gw):
    """HF's f32 table and box bias against the float64 references at f32 round-off, derived (f = 2^-24):
      * torch forms the source coordinate in f32 -- scale = g0 / g (relative f), scale (o + 0.5) and the - 0.5 (half an ulp of a value below g0 = 6 < 8
        each: 4 f): |d t| <= (6 + 4 + 4) f = 14 f.  The cubic's slopes add up to at most 4 over the four taps (|c1'| <= 1.35, |c2'| <= 0.6), so an axis'
        weights move by sum |d w| <= 56 f, and the output by at most 2 * 56 f * 1.25 * max |pos[:, d]| (the other axis' sum |w| <= 1.25);
      * the weights' own polynomial roundings, the 16 products and the adds: within 32 roundings of sum |w| |pos|, elementwise."""
    g0 = 6
    ref = RR.forward64_hw(pos, g0, gh, gw)
    (_, Mwy), (_, Mwx) = RR._axis(g0, gh), RR._axis(g0, gw)
    pa = pos[1:].double().abs()
    slack = 2.0 ** -24 * (32.0 * RR._kron(Mwy, Mwx, pa, g0, g0) + 2.0 * 56.0 * 1.25 * pa.max(0, keepdim=True).values)
    assert tuple(hf_table.shape) == tuple(ref.shape) and bool(((hf_table[1:] - ref[1:]).abs() <= slack).all())
    assert torch.equal(hf_table[0], pos[0].double())
    assert bool(((hf_bias - RR.box_bias_hw(gh, gw)).abs() <= RR.box_bias_tol(gh, gw)).all())          # f32 round-off, derived per element
    assert bool(((box_bias_table(gh, gw).double() - RR.box_bias_hw(gh, gw)).abs() <= RR.box_bias_tol(gh, gw)).all())


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gh,gw", RR.CPU_GRIDS)
def test_per_axis_tap_matrices_are_torchs_bicubic(gh, gw):
    g0, D = 6, 16
    pos, dU, _ = RR.make_case_hw(g0, gh, gw, D)
    assert float((RR.forward64_hw(pos, g0, gh, gw) - _interp(pos, g0, gh, gw)).abs().max()) < 4e-15 * 60.0
    # the adjoint equals torch autograd of interpolate(size=(gh, gw))
    p = pos.double().requires_grad_(True)
    (_interp(p, g0, gh, gw) * dU.double()).sum().backward()
    assert float((RR.adjoint64_hw(dU, g0, gh, gw) - p.grad).abs().max()) < 1e-12
    # gh == gw is pos_resample_reference's square form
    if gh == gw:
        assert torch.equal(RR.forward64_hw(pos, g0, gh, gw), R.forward64(pos, g0, gh))


def test_square_forms_are_the_square_reference():
    pos, dU, old = R.make_case(6, 8, 64)
    assert torch.equal(RR.forward64_hw(pos, 6, 8, 8), R.forward64(pos, 6, 8)) and torch.equal(RR.adjoint64_hw(dU, 6, 8, 8), R.adjoint64(dU, 6, 8))
    assert torch.allclose(RR.bound_fwd_hw(pos, 6, 8, 8), R.bound_fwd(pos, 6, 8), rtol=1e-12, atol=0)
    assert torch.allclose(RR.bound_bwd_hw(dU, old, 6, 8, 8), R.bound_bwd(dU, old, 6, 8), rtol=1e-12, atol=0)
    assert bool(((RR.box_bias_hw(6, 6) - box_bias_table(6).double()).abs() <= RR.box_bias_tol(6, 6)).all())


def test_tables_against_live_transformers_and_the_fixture(f18):
    """interpolate_pos_encoding(., H, W) and compute_box_bias(gh, gw) of the installed transformers, at f32 round-off, and the same from the fixture."""
    transformers = pytest.importorskip("transformers")
    from tests.golden import make_golden_open_vocab as OV
    from owl_vit_object_detection_amd.config import get_text_config
    cfg = get_config("tiny")
    hf = OV.build_hf(cfg, get_text_config("tiny"), OV.logit_head(cfg))
    pos = torch.from_numpy(weights.make_weights(cfg)[POS])
    emb = hf.owlvit.vision_model.embeddings
    for gh, gw in RR.FIXTURE_GRIDS:
        with torch.no_grad():
            live = emb.interpolate_pos_encoding(torch.zeros(1, gh * gw + 1, cfg.hidden), gh * 16, gw * 16)[0]
            bias = hf.compute_box_bias(gh, gw)
        _check_tables(pos, live.double(), bias.double(), gh, gw)
    assert transformers.__version__


@pytest.mark.parametrize("gh,gw", RR.FIXTURE_GRIDS)
def test_tables_against_the_fixture(f18, gh, gw):
    cfg = get_config("tiny")
    pos = torch.from_numpy(weights.make_weights(cfg)[POS])
    _check_tables(pos, torch.from_numpy(f18[f"pos_{gh}x{gw}"]).double(), torch.from_numpy(f18[f"bias_{gh}x{gw}"]).double(), gh, gw)


def test_box_bias_one_argument_call_keeps_its_bits():
    for g in (1, 6, 24, 48, 60):
        c = torch.arange(1, g + 1, dtype=torch.float32)
        xx, yy = torch.meshgrid(c, c, indexing="xy")
        bc = torch.stack((xx, yy), dim=-1)
        bc[..., 0] /= g
        bc[..., 1] /= g
        bc = torch.clip(bc.view(-1, 2), 0.0, 1.0)
        cb = torch.log(bc + 1e-4) - torch.log1p(-bc + 1e-4)
        sz = torch.full_like(cb, 1.0)
        sz[..., 0] /= g
        sz[..., 1] /= g
        old = torch.cat([cb, torch.log(sz + 1e-4) - torch.log1p(-sz + 1e-4)], dim=-1)
        assert torch.equal(box_bias_table(g), old) and torch.equal(box_bias_table(g, g), old)


# ---- planted errors -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", RR.POS_ERRORS)
def test_planted_table_errors_miss_the_bound_on_the_gpu_shapes(kind):
    """Per error: the GPU shapes (f32 table, the derived forward bound) on which it is outside the bound somewhere -- at least one, and every shape
    where the error computes something else than the kernel at all.  D is cut to 16 columns (the bound is per element)."""
    killed, same = [], []
    for g0, gh, gw, D in RR.POS_SHAPES:
        pos, _, _ = RR.make_case_hw(g0, gh, gw, D)
        pos = pos[:, :16].contiguous()
        pos[1 + (g0 * g0) // 2, 5] = 60.0
        ref, tol = RR.forward64_hw(pos, g0, gh, gw), RR.bound_fwd_hw(pos, g0, gh, gw)
        bad = RR.wrong_forward(pos, g0, gh, gw, kind)
        (killed if bool(((bad - ref).abs() > tol).any()) else same).append((g0, gh, gw))
        if not bool(((bad - ref).abs() > tol).any()):
            # never "a different table that slips through": the same table to float64 round-off (a one-cell table's weights add up to 1 whatever the taps)
            assert float((bad - ref).abs().max()) <= 1e-13 * 60.0, (kind, g0, gh, gw)
    print(f"planted {kind}: outside the bound on {killed}; the same table on {same}")
    assert killed
    if kind == "skipped_at_equal_P":
        assert killed == [(6, 4, 9)]
    if kind == "y_taps_with_gw":
        assert set(killed) >= {(6, 6, 10), (6, 10, 6), (6, 4, 9), (24, 16, 40)}


@pytest.mark.parametrize("kind", RR.BOX_ERRORS)
def test_planted_box_bias_errors_are_far_outside_round_off(kind):
    for gh, gw in ((6, 10), (10, 6), (4, 9), (7, 5)):
        assert float((RR.box_bias_hw(gh, gw, wrong=kind) - RR.box_bias_hw(gh, gw)).abs().max()) > 0.3
        assert bool(((box_bias_table(gh, gw).double() - RR.box_bias_hw(gh, gw)).abs() <= RR.box_bias_tol(gh, gw)).all())


@pytest.mark.parametrize("kind", RR.EMBED_ERRORS)
@pytest.mark.parametrize("ps,H,W", RR.EMBED_SHAPES)
def test_planted_gather_errors_miss_the_exact_comparison(ps, H, W, kind):
    B, D = 2, 8
    img, w, pos = RR.make_integers_hw(B, H, W, ps, D)
    EM.assert_exact_ok(img, w, pos)
    Tp = EM.tp_of((H // ps) * (W // ps))
    ref, mask = EM.exact(img, w, pos, Tp)
    assert tuple(ref.shape) == (B + 1, Tp, D)
    # the reference's row order is conv2d(...).flatten(2): patch (py, px) in row 1 + py gw + px
    pt = RR.patches_of_hw(img, ps).double().reshape(B, -1, 3 * ps * ps) @ w.double().reshape(D, -1).t()
    assert torch.equal(ref[:B, 1:pt.shape[1] + 1], pt + pos.double()[1:])
    bad = RR.wrong_embed(img, w, pos, Tp, kind)
    assert EM.check_exact(f"{kind} ps={ps} {H}x{W}", bad.float(), ref, mask, fails=[]) > 0


# ---- config and validation ------------------------------------------------------------------------------------------------------------------------
def test_config_pair_and_int_forms():
    cfg = get_config("tiny")
    assert cfg.replace(image_size=(96, 96)) == cfg and cfg.replace(image_size=[96, 96]).image_size == 96 and cfg.replace(image_size=128).grid == 8
    assert cfg.image_hw == (96, 96) and (cfg.grid_h, cfg.grid_w, cfg.grid, cfg.patches, cfg.resampled) == (6, 6, 6, 36, False)
    r = cfg.replace(image_size=(96, 160), pos_grid=6)
    assert r.image_size == (96, 160) and r.image_hw == (96, 160) and (r.grid_h, r.grid_w, r.patches, r.tokens, r.tokens_padded) == (6, 10, 60, 61, 64)
    assert r.native_grid == 6 and r.pos_rows == 37 and r.resampled and hash(r) != hash(cfg)
    with pytest.raises(ValueError, match="not square"):
        r.grid
    with pytest.raises(ValueError, match="set pos_grid"):
        cfg.replace(image_size=(96, 160)).native_grid
    # the 36-patch rectangle is resampled although P is the native table's
    q = cfg.replace(image_size=(64, 144), pos_grid=6)
    assert q.patches == cfg.patches and q.resampled and not cfg.replace(pos_grid=6).resampled
    # the flops follow P and T
    sq = cfg.replace(image_size=128)
    r2 = cfg.replace(image_size=(64, 256), pos_grid=6)
    assert r2.patches == sq.patches and r2.flops_forward() == sq.flops_forward() and r2.flops_train_step() == sq.flops_train_step()
    assert isinstance(r, OwlConfig) and r.replace(n_classes=3).image_size == (96, 160)
    assert weights.param_shapes(r) == weights.param_shapes(cfg)          # the checkpoint side does not see the input size


def test_check_image_size_pair():
    assert check_image_size(128, 16, 37) == 8 and check_image_size((96, 160), 16, 37) == (6, 10) and check_image_size((128, 128), 16) == (8, 8)
    assert check_image_size((16, 16 * 256), 16) == (1, 256) and check_image_size((16 * 64, 16 * 128), 16) == (64, 128)
    with pytest.raises(ValueError, match=r"the width 150 is not a positive multiple of the patch size 16; the nearest sizes that are: 144 and 160"):
        check_image_size((96, 150), 16)
    with pytest.raises(ValueError, match=r"the height 8 is not a positive multiple of the patch size 16; the nearest sizes that are: 16"):
        check_image_size((8, 160), 16)
    with pytest.raises(ValueError, match=r"8256 patches.*at most 8192.*largest height at this width is 2048, the largest width at this height 1008"):
        check_image_size((16 * 129, 16 * 64), 16)
    assert MAX_PATCHES == 8192
    with pytest.raises(ValueError, match=r"the width gives 257 patches.*at most 256 per side: the largest width is 4096"):
        check_image_size((16, 16 * 257), 16)
    with pytest.raises(ValueError, match="36 rows"):
        check_image_size((96, 160), 16, 36)
    with pytest.raises(ValueError, match="an int .square. or a pair"):
        check_image_size((96, 160, 3), 16)
    # the int form is untouched
    with pytest.raises(ValueError, match=r"image_size=100 is not a positive multiple of the patch size 16; the nearest sizes that are: 96 and 112"):
        check_image_size(100, 16)


def test_input_stage_host_logic_with_a_pair():
    from owl_vit_object_detection_amd import preprocess as PP
    assert PP.size_hw(96) == (96, 96) and PP.size_hw((96, 160)) == (96, 160) and PP._size_attr((96, 96)) == 96 and PP._size_attr([96, 160]) == (96, 160)
    u8 = torch.zeros(2, 96, 160, 3, dtype=torch.uint8)
    assert PP.classify_images(u8, (96, 160))[0] == "u8_hwc" and PP.classify_images(u8, (160, 96))[0] == "u8_ragged" and PP.classify_images(u8, 96)[0] == "u8_ragged"
    assert PP.classify_images(u8.permute(0, 3, 1, 2).contiguous(), (96, 160))[0] == "u8_chw"
    assert PP.classify_images(torch.zeros(2, 3, 96, 160), (96, 160))[0] == "dense"
    with pytest.raises(ValueError, match=r"pixel_values must be \[B,3,160,96\]"):
        PP.classify_images(torch.zeros(2, 3, 96, 160), (160, 96))
    with pytest.raises(ValueError, match="TrainAugment takes a square size"):
        PP.TrainAugment((96, 160))
    assert PP.TrainAugment((96, 96)).size == 96
