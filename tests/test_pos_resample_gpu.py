"""-m gpu: owl_pos_resample / owl_pos_resample_bwd (csrc/pos_resample.hip) against the float64 tap-matrix reference, inside the bounds derived in
tests/pos_resample_reference.py (no fitted tolerance).  Shapes (g0, g, D): up- and down-sampling, grids below 4 (every tap clamped), a one-cell table,
a non-integer ratio at model width (24 -> 30, D = 768) and D = 1024 (every thread of a workgroup busy).  Each case prints its worst err / tol;
profiles/pos_resample_reference.md records them."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import ops  # noqa: E402
from tests import pos_resample_reference as R  # noqa: E402

DEV = "cuda"


@pytest.mark.parametrize("g0,g,D", R.GPU_SHAPES)
def test_forward_and_adjoint_against_float64(g0, g, D):
    pos, dU, old = R.make_case(g0, g, D)
    T0, T = g0 * g0 + 1, g * g + 1
    outs = []
    for _ in range(2):
        out = torch.full((T + 1, D), float("nan"), device=DEV)          # one sentinel row past the end
        ops.pos_resample(pos.to(DEV), out, g0, g, D)
        dpos = torch.cat([old, torch.full((1, D), float("nan"))]).to(DEV)          # NON-ZERO: the backward accumulates
        ops.pos_resample_bwd(dU.to(DEV), dpos, g0, g, D)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[T]).all()) and bool(torch.isnan(dpos[T0]).all())          # nothing past the last row is written
        outs.append((out[:T].cpu(), dpos[:T0].cpu()))
    (u, dp), (u2, dp2) = outs
    assert torch.equal(u, u2) and torch.equal(dp, dp2)          # bitwise reproducible
    assert torch.equal(u[0], pos[0])                            # the class row is a copy
    r_f = R.check(f"forward {g0}->{g} D={D}", u, R.forward64(pos, g0, g), R.bound_fwd(pos, g0, g))
    ref_b, tol_b = old.double() + R.adjoint64(dU, g0, g), R.bound_bwd(dU, old, g0, g)
    r_b = R.check(f"backward {g0}->{g} D={D}", dp, ref_b, tol_b)
    r_b_patch = float(R.ratios(dp[1:], ref_b[1:], tol_b[1:]).max())          # (the class row is ONE rounding of old + dU[0]: its ratio sits just below 1 by construction)
    # <dU, K p> == <K^T dU, p> from the device outputs (the adjoint into zeros), to the float64 round-off of the two sums plus what the bounds allow the
    # device values themselves
    z = torch.zeros_like(old)
    dz = z.to(DEV)
    ops.pos_resample_bwd(dU.to(DEV), dz, g0, g, D)
    kt = dz.cpu().double()
    lhs, rhs = (dU.double() * u.double()).sum(), (kt * pos.double()).sum()
    slack = (dU.double().abs() * R.bound_fwd(pos, g0, g)).sum() + (R.bound_bwd(dU, z, g0, g) * pos.double().abs()).sum()
    gap = float((lhs - rhs).abs())
    print(f"pos_resample g0={g0} g={g} D={D}: err / tol forward {r_f:.3f}, backward {r_b:.4f} (patch rows {r_b_patch:.3f}); |<dU, K p> - <K^T dU, p>| = {gap:.3e} "
          f"(allowed {float(slack):.3e}, |<dU, K p>| = {float(lhs.abs()):.3e})")
    assert r_f < 1.0 and r_b < 1.0
    assert gap <= float(slack) + 1e-12 * float(lhs.abs())


def test_same_grid_is_a_copy():
    """g == g0: the weights are exactly {0, 1, 0, 0} (the model never launches this case; the kernel still has to be right on it)."""
    g0, D = 6, 128
    pos, dU, old = R.make_case(g0, g0, D)
    out = torch.zeros(g0 * g0 + 1, D, device=DEV)
    ops.pos_resample(pos.to(DEV), out, g0, g0, D)
    dpos = old.to(DEV)
    ops.pos_resample_bwd(dU.to(DEV), dpos, g0, g0, D)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), pos) and torch.equal(dpos.cpu(), old + dU)


def test_argument_errors():
    from owl_vit_object_detection_amd import _lib
    x = torch.zeros(65, 128, device=DEV)
    with pytest.raises(_lib.OwlLibError, match="multiple of 8"):
        _lib.call("owl_pos_resample", ops.stream(), x, x, 6, 8, 12)
    with pytest.raises(_lib.OwlLibError, match="side 1 .. 256"):
        _lib.call("owl_pos_resample_bwd", ops.stream(), x, x, 0, 8, 128)
    with pytest.raises(ValueError, match="must hold"):
        ops.pos_resample(x[:37], x[:60], 6, 8, 128)
