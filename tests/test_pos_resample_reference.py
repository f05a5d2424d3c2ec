"""CPU: the float64 reference and the bounds of tests/pos_resample_reference.py (what tests/test_pos_resample_gpu.py holds the kernels to), the host-side
size validator and the native-shape parameter.  No device is needed."""
import os

import numpy as np
import pytest
import torch

from owl_vit_object_detection_amd import weights
from owl_vit_object_detection_amd.config import MAX_PATCHES, check_image_size, get_config, table_grid
from tests import pos_resample_reference as R
from tests.gemm_reference import F, TINY, gamma2

PAIRS = R.PAIRS
D = 8


def _torch_interp(pos, g0, g):
    """[g0 g0 + 1, D] float64 -> torch.nn.functional.interpolate on the patch rows, the class row copied (HF5:296-332)."""
    Dn = pos.shape[1]
    grid = pos[1:].reshape(1, g0, g0, Dn).permute(0, 3, 1, 2)
    up = torch.nn.functional.interpolate(grid, size=(g, g), mode="bicubic", align_corners=False)
    return torch.cat([pos[:1], up.permute(0, 2, 3, 1).reshape(g * g, Dn)], 0)


@pytest.mark.parametrize("g0,g", PAIRS)
def test_reference_is_torch_bicubic_in_float64_forward_and_adjoint(g0, g):
    gen = torch.Generator().manual_seed(g0 * 100 + g)
    pos = torch.randn(g0 * g0 + 1, D, generator=gen, dtype=torch.float64).requires_grad_(True)
    dU = torch.randn(g * g + 1, D, generator=gen, dtype=torch.float64)
    want = _torch_interp(pos, g0, g)
    got = R.forward64(pos.detach(), g0, g)
    err = float((got - want.detach()).abs().max())
    want.backward(dU)
    err_adj = float((R.adjoint64(dU, g0, g) - pos.grad).abs().max())
    print(f"{g0} -> {g}: forward {err:.2e}, adjoint {err_adj:.2e}")
    assert err < 1e-12 and err_adj < 1e-12
    # <dU, K p> == <K^T dU, p>
    lhs, rhs = float((dU * got).sum()), float((R.adjoint64(dU, g0, g) * pos.detach()).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


@pytest.mark.parametrize("g0,g", PAIRS)
def test_rows_of_the_tap_matrix_sum_to_one(g0, g):
    M = R.tap_matrix(g0, g)
    assert M.shape == (g, g0) and float((M.sum(1) - 1.0).abs().max()) < 1e-14


@pytest.mark.parametrize("g0", [1, 2, 3, 6, 24])
def test_same_grid_is_the_identity_exactly(g0):
    assert torch.equal(R.tap_matrix(g0, g0), torch.eye(g0, dtype=torch.float64))
    idx, w = R.emulate_taps(g0, g0)          # ... and in the kernel's f32 arithmetic: weights {0, 1, 0, 0} to the bit
    assert torch.equal(w, torch.tensor([[0.0, 1.0, 0.0, 0.0]]).expand(g0, 4)) and torch.equal(idx[:, 1], torch.arange(g0))
    pos, _, _ = R.make_case(g0, g0, D)
    assert torch.equal(R.emulate_fwd(pos, g0, g0), pos)


@pytest.mark.parametrize("g0,g", PAIRS + ((60, 72), (48, 60), (24, 4), (7, 10)))
def test_the_backward_walks_exactly_the_output_cells_that_touch_a_source_cell(g0, g):
    """touch_range restates the kernel's integer formula: it must give, for every source index, the first and last output index with a tap on it, and
    every index between them must have one (the rectangle holds no stranger)."""
    idx, w, _ = R.taps64(g0, g)
    hit = torch.zeros(g, g0, dtype=torch.bool)
    hit.scatter_(1, idx, torch.ones_like(idx, dtype=torch.bool))
    for s in range(g0):
        lo, hi = R.touch_range(s, g0, g)
        os_ = hit[:, s].nonzero()[:, 0].tolist()
        assert os_ == list(range(lo, hi + 1)), (s, lo, hi, os_)
        assert 0 <= lo and hi <= g - 1
    assert torch.equal(R.touch_counts(g0, g), hit.sum(0))


@pytest.mark.parametrize("g0,g", PAIRS)
def test_f32_simulation_of_the_kernels_is_inside_the_bound(g0, g):
    """The bound is not vacuous the other way either: the kernels' arithmetic, run in f32 on the CPU in the order the source writes it, stays inside it."""
    pos, dU, old = R.make_case(g0, g, D)
    r_f = R.check(f"fwd {g0}->{g}", R.emulate_fwd(pos, g0, g), R.forward64(pos, g0, g), R.bound_fwd(pos, g0, g))
    r_b = R.check(f"bwd {g0}->{g}", R.emulate_bwd(dU, old, g0, g), old.double() + R.adjoint64(dU, g0, g), R.bound_bwd(dU, old, g0, g))
    print(f"{g0} -> {g}: simulated err / tol forward {r_f:.3f}, backward {r_b:.3f}")
    # and it is tight to within two orders: a bound 100x the error it admits would be no bound
    assert (r_f > 1e-2 or g0 == 1) and r_b > 1e-2
    # the adjoint identity from the f32 outputs, to the bounds' own sum
    got_f, got_b = R.emulate_fwd(pos, g0, g).double(), R.emulate_bwd(dU, torch.zeros_like(old), g0, g).double()
    lhs, rhs = (dU.double() * got_f).sum(), (got_b * pos.double()).sum()
    slack = (dU.double().abs() * R.bound_fwd(pos, g0, g)).sum() + (R.bound_bwd(dU, torch.zeros_like(old), g0, g) * pos.double().abs()).sum()
    assert float((lhs - rhs).abs()) <= float(slack) + 1e-12 * float(lhs.abs())


@pytest.mark.parametrize("g0,g", PAIRS)
@pytest.mark.parametrize("variant", ["a05", "align", "reflect"])
def test_the_bound_has_teeth(g0, g, variant):
    """A table resampled with A = -0.5, with align_corners=True, or with mirrored instead of clamped borders lies OUTSIDE the forward bound, and its
    adjoint outside the backward bound.  A one-cell table (1 -> 4) cannot tell them apart -- every output IS that cell -- which is asserted instead."""
    pos, dU, old = R.make_case(g0, g, D)
    ref, tol = R.forward64(pos, g0, g), R.bound_fwd(pos, g0, g)
    if g0 == 1:
        if variant != "reflect":
            assert float((R.forward64(pos, g0, g, variant) - ref).abs().max()) < 1e-14
        return
    wrong = R.forward64(pos, g0, g, variant)
    worst = float(R.ratios(wrong, ref, tol).max())
    Mt = R.tap_matrix(g0, g, variant).t().contiguous()
    wrong_b = old.double() + torch.cat([dU.double()[:1], R._kron_apply(Mt, Mt, dU.double()[1:], g)], 0)
    worst_b = float(R.ratios(wrong_b, old.double() + R.adjoint64(dU, g0, g), R.bound_bwd(dU, old, g0, g)).max())
    print(f"{g0} -> {g} {variant}: err / tol forward {worst:.3g}, backward {worst_b:.3g}")
    assert worst > 1.0 and worst_b > 1.0
    # ... so do planted slips of the kernels themselves: a dropped tap, an overwrite where the gradient accumulates
    assert float(R.ratios(R.emulate_fwd(pos, g0, g, hooks=("skip_last_tap",)), ref, tol).max()) > 1.0 or float(R.taps64(g0, g)[1][:, 3].abs().max()) == 0.0
    assert float(R.ratios(R.emulate_bwd(dU, old, g0, g, hooks=("overwrite",)), old.double() + R.adjoint64(dU, g0, g), R.bound_bwd(dU, old, g0, g)).max()) > 1.0


def _bound_torch_f32(pos, g0, g):
    """What float32 torch may be off by from forward64 (the fixture's own error, NOT the kernel's bound): its source coordinate is formed in f32 --
    scale = fl(g0 / g), s = fl(fl(scale (o + 0.5)) - 0.5), t = fl(s - floor(s)): four roundings of values below g0 + 1, |dt| <= 4 F (g0 + 1) --, the
    weights are cubics with |dw / dt| <= 1.35 on [0, 1] (c1) and <= 0.75 on [1, 2] (c2) evaluated in at most 8 roundings, and the 16 products are added
    in an order this test does not assume (gamma2(17): 16 adds and the product, rounding mode unknown)."""
    idx, w, _ = R.taps64(g0, g)
    E = 1.35 * 4.0 * F * (g0 + 1) + 8.0 * F * w.abs()
    Ma, Mw = R._scatter(idx, w.abs() + E, g0), R._scatter(idx, w.abs(), g0)
    pa = pos.double().abs()
    tol = (1.0 + gamma2(17)) * R._kron_apply(Ma, Ma, pa[1:], g0) - R._kron_apply(Mw, Mw, pa[1:], g0) + TINY
    return torch.cat([torch.zeros_like(pa[:1]), tol], 0)


def test_reference_matches_the_hugging_face_fixture(golden_dir):
    """tests/golden/f13_pos_interp.npz: `OwlViTVisionEmbeddings.interpolate_pos_encoding` of a random-init model at the tiny geometry, 96 -> 128."""
    g = np.load(os.path.join(golden_dir, "f13_pos_interp.npz"))
    native, used = torch.from_numpy(g["native"]), torch.from_numpy(g["used"])
    S0, p, Dn, S = (int(v) for v in g["geometry"])
    g0, g1 = S0 // p, S // p
    assert native.shape == (g0 * g0 + 1, Dn) and used.shape == (g1 * g1 + 1, Dn) and (g0, g1) == (6, 8)
    ref = R.forward64(native, g0, g1)
    worst = R.check("HF interpolate_pos_encoding", used, ref, _bound_torch_f32(native, g0, g1))
    rel = float((used.double() - ref).abs().max() / ref.abs().max())
    print(f"HF fixture: worst err / f32 tol {worst:.3f}, max |err| / max |ref| {rel:.2e}")
    assert rel < 1e-6


def test_size_validator():
    assert check_image_size(128, 16) == 8 and check_image_size(96, 16, 37) == 6 and check_image_size(1008, 14, 60 * 60 + 1) == 72
    with pytest.raises(ValueError, match=r"100 is not a positive multiple of the patch size 16.*96 and 112"):
        check_image_size(100, 16)
    # a 37-row table is 6 x 6 + 1; read WITHOUT its class row (36 + 1 = 37 patch rows -> 38) or as 37 patch rows it is no square
    assert table_grid(37) == 6
    with pytest.raises(ValueError, match=r"38 rows.*37 \(6 x 6\) and 50 \(7 x 7\)"):
        check_image_size(96, 16, 38)
    with pytest.raises(ValueError, match=r"36 rows.*26 \(5 x 5\) and 37 \(6 x 6\)"):
        table_grid(36)
    top = 90 * 16
    assert check_image_size(top, 16) == 90 and 90 * 90 <= MAX_PATCHES < 91 * 91
    with pytest.raises(ValueError, match=rf"8281 patches.*at most 8192.*largest size is {top}"):
        check_image_size(top + 16, 16)
    with pytest.raises(ValueError, match="positive multiple"):
        check_image_size(0, 16)


def test_param_shapes_keep_the_native_table_under_pos_grid():
    cfg = get_config("tiny")
    assert cfg.pos_grid == 0 and cfg.native_grid == cfg.grid == 6 and cfg.pos_rows == cfg.tokens == 37
    big = cfg.replace(image_size=128, pos_grid=6)
    assert big.grid == 8 and big.tokens == 65 and big.native_grid == 6 and big.pos_rows == 37
    name = "backbone.embeddings.position_embedding.weight"
    s0, s1 = weights.param_shapes(cfg), weights.param_shapes(big)
    assert s1[name] == (37, cfg.hidden) and s0 == s1          # every shape: checkpoints and the flat bucket are interchangeable
    assert weights.param_shapes(cfg.replace(image_size=128))[name] == (65, cfg.hidden)          # without pos_grid: a table drawn at 128, as before
    w0, w1 = weights.make_weights(cfg), weights.make_weights(big.replace(name="tiny"))
    assert all(np.array_equal(w0[k], w1[k]) for k in w0)
    assert get_config("tiny", image_size=128).replace(n_classes=7).pos_grid == 0          # replace() carries the field, default unchanged
