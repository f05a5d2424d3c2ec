"""The 16x16x32 MFMA block primitive of the bf16 GEMM family (csrc/gemm_common.h: frag_off / frag_read, mma_block_*, acc_block_32x32) in every mainloop
that runs it: the single-phase kernels of gemm.hip (128 x 128 and 256 x 256 tiles), the two-phase kernel (gemm_pp2.hip) and the half-height kernel
(gemm_pph.hip).

1. Exact placement, independent of any accumulation order: A is one-hot per row (a single 1.0 at k0(m) = (7 m + 3) mod K), W holds integers of
   [-128, 127], the bias is zero, so every output is exactly W[n, k0(m)] -- in bf16 and in f32.  A wrong row map of the permuted row-side fragment, a wrong
   direction of the lane exchange, a wrong k-chunk or swizzle key moves or replaces values and cannot hide behind a tolerance.
2. Small-integer sums: A and W in {-2 .. 2} at K = 768; every partial sum is an integer below 2^24, so the f32 result is exact in any order.
3. One bound check of tests/gemm_reference.py (float64 reference, derived elementwise bound) per kernel at K = 128 and K = 768 on the "randn" profile;
   the worst err / tol is printed (MFMASHAPE lines; profiles/mfma_shape.md).  The reference's accumulation model counts K / 16 + 16 roundings (the
   32x32x16 chain); the 16x16x32 chain has K / 32 + 32 in the worst case -- fewer from K = 512 on, formally more below.

Every case asks owl_gemm_nt_plan which kernels the library launches for it and asserts the intended ones.

The half-height kernel is reached two ways: `tile = 6` and the whole-round split of the automatic choice (M = 25 600, N = 768: 85 row panels on the
two-phase kernel, 15 on the half-height one).  The planner gives `tile = 6` the half-height kernel only from 48 tiles of 256 x 256 on, which M = 4096
reaches at N = 768 but not at N = 256: the N = 256 cases of that kernel run at M = 12 288 (and 12 288 - 200) instead.  The half-height kernel has no f32
epilogue (gemm_plan.h, pph_takes): in test 2 it runs EPI_BIAS_BF16 against the exact integer sum rounded to bf16 (nearest even, what pack_bf2 does) --
still an exact comparison."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import ops  # noqa: E402
from tests import gemm_reference as R  # noqa: E402

DEV = "cuda"
SP128, SP256, PP2, PPH = 128, 256, 7, 6          # `tile` of owl_gemm_nt_bf16 (include/owl_hip.h)
PLAN_NAME = {SP128: "sp128", SP256: "sp256", PP2: "pp2", PPH: "pph"}
SPLIT = (25600, 768)                             # tile 0: whole rounds on the two-phase kernel + the remainder on the half-height kernel


def _launch(epi, A, W, bias, M, N, K, tile, want):
    """out [M, N] of one call into a NaN-filled buffer, after asserting that the library's plan for it is `want` ([(kernel, rows)])."""
    assert R.library_path(epi, M, N, K, tile, M, has_aux=0) == want, (epi, M, N, K, tile, want)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16 if epi == R.EPI_BIAS else torch.float32, device=DEV)
    ops.gemm(epi, A, W, out, bias=bias, M=M, N=N, K=K, tile=tile)
    return out


def _kernels(M, N):
    """[(tile, epilogues, plan)] that the shape (M, N) can reach."""
    ks = [(t, (R.EPI_BIAS, R.EPI_F32), [(PLAN_NAME[t], M)]) for t in (SP128, SP256, PP2)]
    if 48 <= ((M + 255) // 256) * ((N + 255) // 256) <= 128:
        ks.append((PPH, (R.EPI_BIAS,), [("pph", M)]))
    return ks


_ONE_HOT = {}


def _one_hot(M, N, K):
    """(A, W, bias, expected [M, N] float32), built once per shape and never modified."""
    if (M, N, K) not in _ONE_HOT:
        g = torch.Generator(device="cpu").manual_seed(20260 + 7 * N + K)
        W = torch.randint(-128, 128, (N, K), generator=g).to(DEV)
        k0 = (7 * torch.arange(M, device=DEV) + 3) % K
        A = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
        A[torch.arange(M, device=DEV), k0] = 1.0
        _ONE_HOT.clear()
        _ONE_HOT[(M, N, K)] = (A, W.to(torch.bfloat16), torch.zeros(N, dtype=torch.float32, device=DEV), W[:, k0].t().contiguous().float())
    return _ONE_HOT[(M, N, K)]


def _assert_placed(out, expect, tag):
    got = out.float()
    if not torch.equal(got, expect):
        bad = (got != expect) | torch.isnan(got)
        idx = bad.nonzero()[:6].tolist()
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} outputs are not W[n, k0(m)]; first at "
                             + "; ".join(f"{i}: got {float(got[tuple(i)])} want {float(expect[tuple(i)])}" for i in idx))


PLACEMENT_SHAPES = [(M, N, K) for K in (128, 192, 768) for N in (256, 768) for M in (4096, 4096 - 200)]
PPH_N256_SHAPES = [(M, 256, K) for K in (128, 192, 768) for M in (12288, 12288 - 200)]


@pytest.mark.parametrize("M,N,K", PLACEMENT_SHAPES)
def test_one_hot_rows_place_every_weight_exactly(M, N, K):
    """EPI_BIAS_BF16 and EPI_F32 on the 128 x 128, 256 x 256 and two-phase kernels, EPI_BIAS_BF16 on the half-height kernel (N = 768): whole and guarded
    row tiles, two / three (odd buffer parity) / twelve K-tiles."""
    A, W, bias, expect = _one_hot(M, N, K)
    kernels = _kernels(M, N)
    assert len(kernels) == (4 if N == 768 else 3)
    for tile, epis, want in kernels:
        for epi in epis:
            _assert_placed(_launch(epi, A, W, bias, M, N, K, tile, want), expect, f"{M}x{N}x{K} {PLAN_NAME[tile]} epi={R.EPI_NAMES[epi]}")


@pytest.mark.parametrize("M,N,K", PPH_N256_SHAPES)
def test_one_hot_rows_half_height_kernel_at_n256(M, N, K):
    """The half-height kernel with a single column tile: the smallest M at which `tile = 6` reaches it at N = 256 (module docstring)."""
    A, W, bias, expect = _one_hot(M, N, K)
    _assert_placed(_launch(R.EPI_BIAS, A, W, bias, M, N, K, PPH, [("pph", M)]), expect, f"{M}x{N}x{K} pph")


@pytest.mark.parametrize("K", [128, 192, 768])
def test_one_hot_rows_whole_round_split(K):
    """The automatic choice at M = 25 600, N = 768: 21 760 rows on the two-phase kernel, 3840 on the half-height kernel, in one output."""
    M, N = SPLIT
    A, W, bias, expect = _one_hot(M, N, K)
    M_main = R.gemm_split(M, N, 0)
    assert M_main == 21760
    _assert_placed(_launch(R.EPI_BIAS, A, W, bias, M, N, K, 0, [("pp2", M_main), ("pph", M - M_main)]), expect, f"{M}x{N}x{K} pp2+pph")


def test_small_integer_sums_are_exact():
    """A, W in {-2 .. 2}, K = 768: |partial sums| <= 3072 < 2^24, the f32 accumulator is exact whatever the order of the adds.  EPI_F32 against the int64
    product on the three kernels that have the epilogue; the half-height kernel (bf16 outputs only) against the same integers rounded to bf16."""
    M, N, K = 4096 - 200, 768, 768
    g = torch.Generator(device="cpu").manual_seed(31)
    A = torch.randint(-2, 3, (M, K), generator=g).to(DEV)
    W = torch.randint(-2, 3, (N, K), generator=g).to(DEV)
    exact = (A.double() @ W.double().t()).round().to(torch.int64)            # (products and sums of small integers: exact in float64 too)
    assert int(exact.abs().max()) <= 4 * K
    Ab, Wb = A.to(torch.bfloat16), W.to(torch.bfloat16)
    for tile in (SP128, SP256, PP2):
        out = _launch(R.EPI_F32, Ab, Wb, None, M, N, K, tile, [(PLAN_NAME[tile], M)])
        assert torch.equal(out.to(torch.int64), exact) and torch.equal(out, exact.float()), f"{PLAN_NAME[tile]}: {int((out != exact.float()).sum())} sums differ"
    out = _launch(R.EPI_BIAS, Ab, Wb, None, M, N, K, PPH, [("pph", M)])
    assert torch.equal(out, exact.float().to(torch.bfloat16)), f"pph: {int((out != exact.float().to(torch.bfloat16)).sum())} sums differ"


_BOUND = {}


@pytest.mark.parametrize("tile", [SP128, SP256, PP2, PPH], ids=lambda t: PLAN_NAME[t])
@pytest.mark.parametrize("K", [128, 768])
def test_inside_the_float64_bound(K, tile):
    """EPI_BIAS_BF16 on the "randn" profile against `exact` / `bounds` / `check` of tests/gemm_reference.py, every element."""
    M, N = 4096 - 200, 768
    if _BOUND.get("K") != K:
        inp = {k: v.to(DEV) for k, v in R.make_inputs("randn", M, N, K, 5, R.EPI_BIAS).items()}
        ex = R.exact(R.EPI_BIAS, inp["A"], inp["W"], bias=inp["bias"])
        _BOUND.clear()
        _BOUND.update(K=K, A=inp["A"].bfloat16(), W=inp["W"].bfloat16(), bias=inp["bias"].contiguous(), ref=ex["out"], tol=R.bounds(ex)["out"])
    b = _BOUND
    out = _launch(R.EPI_BIAS, b["A"], b["W"], b["bias"], M, N, K, tile, [(PLAN_NAME[tile], M)])
    print(f"MFMASHAPE bound K={K} kernel={PLAN_NAME[tile]} worst err/tol={float(R.ratios(out, b['ref'], b['tol']).max()):.4f}")
    R.check(f"{PLAN_NAME[tile]} K={K}", out, b["ref"], b["tol"])
