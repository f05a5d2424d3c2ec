"""The GEMM checker (tests/gemm_reference.py) checked without a GPU: over the case set of tests/test_gemm_reference_gpu.py (M capped at 600) the
f32 simulation of the kernels sits inside every derived bound, the bounds are not slack, the profiles reach the tails they are meant to reach, and
every planted error is rejected by `check` / `untouched`."""
import math

import pytest
import torch

from tests import gemm_reference as R

M_CAP = 600
CASES = [(min(M, M_CAP), N, K, form, profile) for (M, N, K, form, profile) in R.cases()]


def _run(M, N, K, form, profile, hooks=None, seed=1, accumulate=0, inp=None):
    name, epi, alpha, with_bias, _inplace, splits = R.FORM[form]
    inp = inp or R.make_inputs(profile, M, N, K, seed, epi)
    kw = dict(bias=inp["bias"] if with_bias else None, alpha=alpha, resid=inp["resid"], aux_in=inp["aux_in"], splits=splits, accumulate=accumulate)
    ex = R.exact(epi, inp["A"], inp["W"], **kw)
    em = R.emulate(epi, inp["A"], inp["W"], hooks=hooks, **kw)
    return inp, ex, R.bounds(ex), em


def _keys(epi):
    return ("out", "reduced") if epi == R.EPI_SLAB else (("out", "aux") if epi in (R.EPI_QGELU, R.EPI_GELU) else ("out",))


def _worst(ex, tol, em, fails):
    return max(R.check(k, em[k], ex[k], tol[k], fails) for k in _keys(ex["epi"]))


def test_constants_of_the_bounds():
    """The sups the propagation remainders use hold on a dense grid, the Abramowitz-Stegun form stays inside its published error, and the chain
    bound lies below the any-order bound at every K of the case set."""
    x = torch.linspace(-40.0, 40.0, 800001, dtype=torch.float64)
    assert float(R.qgelu_d2(x).abs().max()) <= R.QG_SUP2 and float(R.qgelu_d3(x).abs().max()) <= R.QG_SUP3
    assert float(R.gelu_d2(x).abs().max()) <= R.GELU_SUP2
    assert float(R.qgelu_d1(x).abs().max()) <= 1.2 and float(R.gelu_d1(x).abs().max()) <= 1.2
    z = torch.linspace(0.0, 12.0, 400001, dtype=torch.float64)
    t = 1.0 / (1.0 + R.AS_P * z)
    poly = sum(c * t ** (i + 1) for i, c in enumerate(R.AS_A))
    assert float((1.0 - poly * torch.exp(-z * z) - torch.erf(z)).abs().max()) <= R.AS_ERR
    for K in sorted({K for (_, _, K) in R.SHAPES + [R.TALL]}):
        assert R.gamma2(R.n_acc(K)) <= R.gamma2(K + 1)
    # the derivatives are the derivatives (central differences in float64)
    x = torch.linspace(-8.0, 8.0, 4001, dtype=torch.float64); h = 1e-5
    for f, d in ((R.qgelu, R.qgelu_d1), (R.qgelu_d1, R.qgelu_d2), (R.qgelu_d2, R.qgelu_d3), (R.gelu, R.gelu_d1), (R.gelu_d1, R.gelu_d2)):
        assert float(((f(x + h) - f(x - h)) / (2 * h) - d(x)).abs().max()) < 1e-8


def test_shapes_reach_the_kernels_named():
    """From the planner's conditions (gemm_plan.h, gemm_plan, restated in gemm_reference.dispatch_path): (2900, 1000, 128) is the smallest-M problem of 48
    tiles -- tile 6 takes the half-height kernel on all of it, tile 0 the two-phase one; the tall case splits into one whole round on the two-phase
    kernel and 44 remainder tiles on the half-height one.  N = 248 (300 x 1 tiles as well) would NOT: the automatic rule wants N >= 256."""
    M, N, K = R.SHAPES[-1]
    assert ((M + 255) // 256) * ((N + 255) // 256) == 48
    for epi in R.PPH_EPIS:
        assert R.dispatch_path(epi, M, N, K, 6) == [("pph", M)] and R.dispatch_path(epi, M, N, K, 0) == [("pp2", M)]
        assert R.dispatch_path(epi, M - 256, N, K, 6) == [("sp128", M - 256)]
    M, N, K = R.TALL
    assert R.gemm_split(M, N, 0) == 65536 and (M + 255) // 256 == 300
    for epi in R.PPH_EPIS:
        assert R.dispatch_path(epi, M, N, K, 0) == [("pp2", 65536), ("pph", M - 65536)]
        assert R.dispatch_path(epi, M, N, K, 7) == [("pp2", M)] and R.dispatch_path(epi, M, N, K, 256) == [("sp256", M)]
        assert R.dispatch_path(epi, M, 248, K, 0) == [("sp128", M)]
    for epi in (R.EPI_RESID, R.EPI_SLAB):
        assert R.dispatch_path(epi, M, N, K, 0) == [("sp256", M)]
    rows = R.sample_rows(M, 65536)
    assert {65535, 65536}.issubset(rows) and {r // 128 for r in rows} == set(range((M + 127) // 128))
    # every shape x tile lands on a kernel of the family, and the case set holds every form at every shape
    assert {k for (M, N, K) in R.SHAPES for t in R.TILES for e in R.EPI_NAMES for (k, _) in R.dispatch_path(e, M, N, K, t)} == {"pp2", "pph", "sp128", "sp256"}
    assert {(M, N, K, f) for (M, N, K, f, _) in R.cases()} == {(M, N, K, f[0]) for (M, N, K) in R.SHAPES + R.TOWER_SHAPES for f in R.FORMS}
    for epi in R.EPI_NAMES:
        for p in R.profiles_of(epi):
            assert sum(1 for (_, _, _, f, q) in R.cases() if R.FORM[f][1] == epi and q == p) >= 2, (epi, p)


@pytest.mark.parametrize("M,N,K,form,profile", CASES)
def test_emulation_inside_bounds_and_bounds_not_slack(M, N, K, form, profile):
    """Neither too tight: the f32 simulation lies inside `tol` of `exact` at every element (and inside the any-order bound, which is wider).  Nor too
    loose, on randn: bf16 outputs -- median tol / max(|ref|, 2^-10) <= 2^-7 (two bf16 roundings, the figure of test_gemm_model_row_counts); f32
    outputs -- median tol / acc_abs <= 4 gamma(K + 2)."""
    epi = R.FORM[form][1]
    fails = []
    for accumulate in ((0, 1) if epi == R.EPI_SLAB else (0,)):
        inp, ex, tol, em = _run(M, N, K, form, profile, accumulate=accumulate)
        _worst(ex, tol, em, fails)
        wide = R.bounds(ex, any_order=True)
        for k in _keys(epi):
            assert bool((wide[k] >= tol[k]).all())
    assert not fails, "\n".join(fails)
    if profile != "randn":
        return
    if epi in R.BF16_OUT:
        for k in _keys(epi):
            med = float((tol[k] / ex[k].abs().clamp(min=2.0 ** -10)).median())
            assert med <= 2.0 ** -7, (k, med)
    elif epi == R.EPI_SLAB:
        for (a, b), t, sa in zip(ex["ranges"], tol["out"], ex["slab_abs"]):
            assert float((t / sa).median()) <= 4.0 * R.gamma(b - a + 2)
        assert float((tol["reduced"] / ex["slab_abs"].sum(0)).median()) <= 4.0 * R.gamma(K + 2)
    else:
        scale = abs(R.FORM[form][2])
        assert float((tol["out"] / (scale * ex["acc_abs"])).median()) <= 4.0 * R.gamma(K + 2)


def test_profiles_reach_the_tails():
    """`tails` (bias / given aux = linspace(-14, 14)) sweeps every row across both saturated ends: the erf-GELU output is -0 in the simulation and
    subnormal in the reference, the derivative's exp2 flushes to 0 (|a| > 13.2).  +-14 cannot reach the OVERFLOW of the sigmoid's exp2, which needs a
    pre-activation below -52.1: `tails_wide` (+-60) does, and no other profile does either."""
    M, N, K = 129, 264, 192
    lo = {}
    for p in R.PROFILES[:4]:
        inp, ex, tol, em = _run(M, N, K, "gelu", p)
        lo[p] = float(ex["pre"].min())
        sub = (ex["out"] != 0) & (ex["out"].abs() < R.TINY)
        neg0 = (em["out"] == 0) & torch.signbit(em["out"]) & (ex["pre"] < -6.0)
        assert bool(sub.any()) == (p in ("tails", "tails_wide")) and bool(neg0.any()) == (p in ("tails", "tails_wide")), p
        assert (float(ex["pre"].max()) > 10.0) == (p in ("tails", "tails_wide"))
        over = torch.isinf(torch.exp2(torch.tensor(-R.C_Q, dtype=torch.float32) * em["pre"]))
        assert bool(over.any()) == (p == "tails_wide") and bool((ex["pre"] < -52.1).any()) == (p == "tails_wide"), p
        a = R.make_inputs(p, M, N, K, 1, R.EPI_DGELU)["aux_in"]
        flushed = torch.exp2(a * a * -R.C_D) < R.TINY
        assert bool(flushed.any()) == (p in ("tails", "tails_wide")), p
    assert lo["tails"] < -10.0 and lo["tails_wide"] < -55.0
    inp, ex, tol, em = _run(M, N, K, "qgelu", "tails_wide")
    assert bool(((em["out"] == 0) & (ex["pre"] < -52.1)).any()) and bool(((ex["out"].abs() > R.TINY) & (em["out"] == 0)).any())
    # cancel: |acc| << acc_abs;  resid_large: the residual's rounding dominates
    inp, ex, tol, em = _run(M, N, K, "f32_a1", "cancel")
    assert float((ex["acc"].abs() / ex["acc_abs"]).median()) < 2.0 ** -8
    inp, ex, tol, em = _run(M, N, K, "resid", "resid_large")
    assert float((R.F * ex["out"].abs() / tol["out"]).median()) > 0.5


# ---------------------------------------------------------------------------------------------------------------------------------------------
# planted errors: small mutators of the simulation, each of which `check` must reject (at least one element outside its bound)
# ---------------------------------------------------------------------------------------------------------------------------------------------
S1, S2 = (129, 264, 192), (300, 256, 192)
BF = R.bf16_round
f32 = lambda v: torch.tensor(v, dtype=torch.float32)


def _rejected(ex, tol, got):
    fails = []
    for k in got:
        R.check(k, got[k], ex[k], tol[k], fails)
    return len(fails) > 0


def _plant_bias_quad(shape, form, profile):
    inp = R.make_inputs(profile, *shape, 1, R.FORM[form][1])
    _, ex, tol, _ = _run(*shape, form, profile, inp=inp)
    bad = dict(inp); bad["bias"] = inp["bias"].clone(); bad["bias"][4:8] = 0.0
    name, epi, alpha, _, _, _ = R.FORM[form]
    em = R.emulate(epi, bad["A"], bad["W"], bias=bad["bias"], alpha=alpha, resid=bad["resid"], aux_in=bad["aux_in"])
    return ex, tol, {"out": em["out"]}


def _plant_alpha_after_bias(shape, form, profile):
    inp, ex, tol, _ = _run(*shape, form, profile)
    name, epi, alpha, _, _, _ = R.FORM[form]
    em = R.emulate(epi, inp["A"], inp["W"], bias=inp["bias"] * f32(alpha), alpha=alpha)
    return ex, tol, {"out": em["out"]}


def _plant_ktile_dropped(shape, form, profile):
    inp = R.make_inputs(profile, *shape, 1, R.FORM[form][1])
    A, W = inp["A"], inp["W"]
    blk = A[32:64, 64:128] @ W[32:64, 64:128].t()
    if R.FORM[form][1] == R.EPI_SLAB:
        _, ex, tol, em = _run(*shape, form, profile, inp=inp)
        s = next(i for i, (a, b) in enumerate(ex["ranges"]) if a <= 64 < b)
        out = em["out"].clone(); out[s, 32:64, 32:64] -= blk
        red = em["reduced"].clone(); red[32:64, 32:64] -= blk
        return ex, tol, {"out": out, "reduced": red}

    def drop(acc):
        acc = acc.clone(); acc[32:64, 32:64] -= blk
        return acc
    _, ex, tol, em = _run(*shape, form, profile, hooks={"acc": drop}, inp=inp)
    return ex, tol, {k: em[k] for k in _keys(ex["epi"])}


def _plant_bands_swapped(shape, form, profile):
    _, ex, tol, em = _run(*shape, form, profile)
    got = {}
    for k in _keys(ex["epi"]):
        v = em[k].clone()
        v[..., 0:128, :], v[..., 128:256, :] = em[k][..., 128:256, :], em[k][..., 0:128, :]
        got[k] = v
    return ex, tol, got


def _plant_tanh_gelu(shape, form, profile):
    _, ex, tol, em = _run(*shape, form, profile)
    return ex, tol, {"out": BF(R.gelu_tanh(em["pre"]))}


def _plant_dqgelu_at_bf16_u(shape, form, profile):
    _, ex, tol, em = _run(*shape, form, profile)
    ub = BF(em["pre"])
    return ex, tol, {"aux": BF(R.dqgelu_from_s_f32(ub, R.sigmoid1702_f32(ub)))}


def _plant_dgelu_without_phi_term(shape, form, profile):
    inp, ex, tol, em = _run(*shape, form, profile)
    return ex, tol, {"out": BF(em["pre"] * R.dgelu_erf_f32(inp["aux_in"], with_phi_term=False))}


def _plant_last_quad_unwritten(shape, form, profile):
    _, ex, tol, em = _run(*shape, form, profile)
    got = {}
    for k in _keys(ex["epi"]):
        v = em[k].clone(); v[..., shape[1] - 8:shape[1] - 4] = 7.0          # what the buffer held before the call
        got[k] = v
    return ex, tol, got


def _plant_resid_twice(shape, form, profile):
    inp, ex, tol, em = _run(*shape, form, profile)
    return ex, tol, {"out": em["out"] + inp["resid"]}


def _plant_reduce_skips_last_split(shape, form, profile):
    _, ex, tol, em = _run(*shape, form, profile, hooks={"reduce": lambda s: s[:-1]})
    return ex, tol, {"reduced": em["reduced"]}


def _plant_bf16_partial_sums(shape, form, profile):
    _, ex, tol, em = _run(*shape, form, profile, hooks={"partial": lambda acc, kt: BF(acc)})
    return ex, tol, {k: em[k] for k in _keys(ex["epi"])}


ALL_BUT_SLAB = ["bias", "qgelu", "gelu", "resid", "f32_a0.5", "acc", "dqgelu", "dgelu"]
PLANTED = {
    "bias missing on one column quad": (_plant_bias_quad, [S1], ["bias", "qgelu", "gelu", "resid", "f32_a0.5_b"], ["randn", "tails"]),
    "alpha applied after the bias": (_plant_alpha_after_bias, [S1], ["f32_a0.5_b", "f32_a-2_b"], ["randn", "tails"]),
    "one K-tile dropped for one 32 x 32 block": (_plant_ktile_dropped, [S1, S2], ALL_BUT_SLAB + ["slab2", "slab3"], ["randn"]),
    "two adjacent 128-row bands swapped": (_plant_bands_swapped, [S2], ALL_BUT_SLAB + ["slab2"], ["randn"]),
    "tanh-GELU in place of erf-GELU": (_plant_tanh_gelu, [S1, S2], ["gelu"], ["tails"]),
    "quick_gelu' at the bf16-rounded u": (_plant_dqgelu_at_bf16_u, [S1, S2], ["qgelu"], ["randn", "tails"]),
    "erf-GELU' without its u phi(u) term": (_plant_dgelu_without_phi_term, [S1], ["dgelu"], ["randn", "tails"]),
    "the last column quad left unwritten": (_plant_last_quad_unwritten, [S1, (513, 520, 256)], ALL_BUT_SLAB + ["slab2"], ["randn"]),
    "RESID adds the residual twice": (_plant_resid_twice, [S1], ["resid", "resid_inplace"], ["randn", "resid_large"]),
    "the slab reduce skips the last split": (_plant_reduce_skips_last_split, [S1], ["slab2", "slab3", "slab5"], ["randn", "cancel"]),
    "partial sums rounded to bf16 per K-tile": (_plant_bf16_partial_sums, [S1, S2], ALL_BUT_SLAB + ["slab1"], ["cancel"]),
}


@pytest.mark.parametrize("name", list(PLANTED))
def test_planted_error_is_rejected(name):
    plant, shapes, forms, profiles = PLANTED[name]
    missed = []
    for shape in shapes:
        for form in forms:
            for profile in profiles:
                ex, tol, got = plant(shape, form, profile)
                if not _rejected(ex, tol, got):
                    missed.append((shape, form, profile))
    assert not missed, f"{name}: passed the bounds at {missed}"


@pytest.mark.parametrize("sentinel", [7.0, float("nan")], ids=["finite", "nan"])
def test_a_row_past_M_or_a_column_past_N_written_is_reported(sentinel):
    """`untouched` compares bits: one row >= M written, one column quad between N and ldo written, one element of an outer third written -- each is
    reported, with a finite or a NaN sentinel; a call that stays inside [0, M) x [col0, col0 + N) is not."""
    M, N = 129, 264
    for dtype in (torch.bfloat16, torch.float32):
        before = torch.full((M + 3, 3 * N), sentinel, dtype=dtype)
        val = torch.randn(M, N).to(dtype)
        ok = before.clone(); ok[:M, N:2 * N] = val
        assert R.untouched("ok", ok, before, M, N, N, fails=[]) == 0
        for r, c in ((M, N), (0, 2 * N), (M - 1, N - 4), (M + 2, 3 * N - 4)):
            bad = ok.clone(); bad[r, c:c + 4] = 1.0
            fails = []
            assert R.untouched("bad", bad, before, M, N, N, fails) == 4 and fails
    # and `check` itself: a NaN, or one element one part in 2^20 outside its bound, fails; the bound itself passes
    ref = torch.ones(4, 8, dtype=torch.float64); tol = torch.full_like(ref, 1e-3)
    assert R.check("ok", ref + 1e-3 * (1 - 2.0 ** -20), ref, tol) <= 1.0
    got = ref.clone(); got[2, 3] += 1e-3 * (1 + 2.0 ** -20)
    with pytest.raises(AssertionError, match=r"1/32 outside"):
        R.check("bad", got, ref, tol)
    got[2, 3] = float("nan")
    with pytest.raises(AssertionError):
        R.check("nan", got, ref, tol)
    assert math.isinf(R.check("nan", got, ref, tol, fails=[]))
