"""-m gpu: autograd.weight_grad -- the one launcher of the weight-gradient products -- against the two launch sequences written out by hand (bitwise) and
against float64 (the any-order bound of tests/gemm_reference.py), at the smallest shapes that reach each branch of autograd._dw_plan and each reducer.
rows = 200 is no multiple of 64 or 128: every split tail and every pad column is reached."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import _lib, autograd as A, ops  # noqa: E402
from tests import gemm_reference as GR  # noqa: E402

DEV = "cuda"
ROWS = 200
# (id, route, n_out, n_in, bias, tn_all, splits the hand-written sequence requests): TN = 256 items over the 256 x 256 tiles (one n tile for the 32 rows);
# NT = min(pad_rows(200) // 64, 512 // tiles of 128 x 128) = 4
CASES = [("tn_bias", "tn", 256, 256, True, False, 256), ("tn", "tn", 512, 256, False, False, 128), ("tn_small", "tn", 32, 256, False, True, 256),
         ("nt_bias", "nt", 128, 64, True, False, 4), ("nt", "nt", 64, 128, False, False, 4), ("nt_padded", "nt", 128, 588, False, False, 4)]


def _scratch(n_out, n_in, slab_elems, tn_all):
    ld, bf = ops.pad_rows(ROWS), torch.bfloat16
    return dict(slab=torch.zeros(slab_elems, device=DEV), part=ops.rowreduce_workspace(1, ROWS, n_out, DEV), bslab=torch.zeros(256 * n_out, device=DEV),
                tA=torch.zeros(n_out, ld, dtype=bf, device=DEV), tB=torch.zeros(n_in, ld, dtype=bf, device=DEV), tn_all=tn_all)


def _by_hand(route, dy, x, gw, gb, n_out, n_in, splits, s, accumulate):
    """The launch sequence of one route, entry by entry."""
    if route == "tn":
        ns = ops.gemm_tn_slab(dy, x, s["slab"], ROWS, n_out, n_in, splits, bias_slab=s["bslab"] if gb is not None else None)
        _lib.call("owl_slab_reduce", ops.stream(), s["slab"], gw, n_out * n_in, n_out * n_in, ns, accumulate)
        if gb is not None:
            _lib.call("owl_slab_reduce", ops.stream(), s["bslab"], gb, n_out, n_out, ns, 1)
        return
    ld, Kp = ops.pad_rows(ROWS), (n_in + 7) // 8 * 8
    ops.transpose_colsum(dy, s["tA"], gb, ROWS, n_out, ld_in=dy.shape[-1], ld_out=ld, partials=s["part"])
    ops.transpose_colsum(x, s["tB"], None, ROWS, n_in, ld_in=x.shape[-1], ld_out=ld)
    ns = _lib.load().owl_gemm_effective_splits(ld, splits)
    ops.gemm(ops.EPI_SLAB_F32, s["tA"], s["tB"], s["slab"], M=n_out, N=Kp, K=ld, lda=ld, ldw=ld, ldo=Kp, a_rows=n_out, w_rows=n_in, splits=splits)
    if Kp == n_in:
        _lib.call("owl_slab_reduce", ops.stream(), s["slab"], gw, n_out * n_in, n_out * n_in, ns, accumulate)
    else:
        _lib.call("owl_slab_reduce_rows", ops.stream(), s["slab"], gw, n_out, n_in, Kp, n_out * Kp, ns, accumulate)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_weight_grad_is_the_hand_written_sequence(case):
    _, route, n_out, n_in, bias, tn_all, splits = case
    Kp = (n_in + 7) // 8 * 8
    plan = A._dw_plan(n_out, n_in, bias=bias, tn_all=tn_all, rows=ROWS)
    assert plan.tn == (route == "tn") and plan.splits == splits and plan.n_in_pad == Kp
    g = torch.Generator().manual_seed(23)
    dy = torch.zeros(ops.pad_rows(ROWS), n_out, dtype=torch.bfloat16)
    x = torch.zeros(ops.pad_rows(ROWS), Kp, dtype=torch.bfloat16)          # (pad rows and pad columns zero, as every operand buffer of the backward)
    dy[:ROWS] = torch.randn(ROWS, n_out, generator=g).to(torch.bfloat16)
    x[:ROWS, :n_in] = torch.randn(ROWS, n_in, generator=g).to(torch.bfloat16)
    dy64, x64 = dy[:ROWS].double(), x[:ROWS, :n_in].double()
    ref_w, abs_w = dy64.t() @ x64, dy64.abs().t() @ x64.abs()
    ref_b, abs_b = dy64.sum(0), dy64.abs().sum(0)
    dy, x = dy.to(DEV), x.to(DEV)
    mine, hand = _scratch(n_out, n_in, plan.slab_elems, tn_all), _scratch(n_out, n_in, splits * n_out * Kp, tn_all)
    for accumulate in (0, 1):
        # accumulate = 0 overwrites garbage; accumulate = 1 adds into values of the gradient's own size.  The bias gradient is always added into
        s_w = torch.randn(n_out, n_in, generator=g) * float(ref_w.abs().mean()) if accumulate else torch.full((n_out, n_in), float("nan"))
        s_b = torch.randn(n_out, generator=g) * float(ref_b.abs().mean())
        gw, gw_h = s_w.to(DEV), s_w.to(DEV)
        gb, gb_h = (s_b.to(DEV), s_b.to(DEV)) if bias else (None, None)
        A.weight_grad(dy, x, gw, n_out, n_in, ROWS, mine, gb, accumulate=accumulate)
        _by_hand(route, dy, x, gw_h, gb_h, n_out, n_in, splits, hand, accumulate)
        torch.cuda.synchronize()
        assert torch.equal(gw, gw_h) and not bool(torch.isnan(gw).any())
        # bf16 operands (products exact in f32), f32 accumulation over `ROWS` terms in an order the test does not assume, the slab reduction's adds (at most
        # 256 splits) and the add into the value already there: |err| <= gamma2(ROWS + 257 [+ 1]) (sum |dy| |x| + |seed|)
        seed_w = s_w.double() if accumulate else torch.zeros(n_out, n_in, dtype=torch.float64)
        tol_w = GR.gamma2(ROWS + 257 + accumulate) * (abs_w + seed_w.abs()) + 2.0 ** -126
        err_w = (gw.cpu().double() - (ref_w + seed_w)).abs()
        print(f"weight_grad {case[0]} accumulate={accumulate}: max |err| / tol, weight = {float((err_w / tol_w).max()):.3f}")
        assert bool((err_w <= tol_w).all())
        if bias:
            assert torch.equal(gb, gb_h)
            tol_b = GR.gamma2(ROWS + 257 + 1) * (abs_b + s_b.double().abs()) + 2.0 ** -126
            err_b = (gb.cpu().double() - (ref_b + s_b.double())).abs()
            print(f"   bias = {float((err_b / tol_b).max()):.3f}")
            assert bool((err_b <= tol_b).all())
    if route == "nt":          # the pad columns of the transposed operands are never written
        assert not bool(mine["tA"][:, ROWS:].any()) and not bool(mine["tB"][:, ROWS:].any())
