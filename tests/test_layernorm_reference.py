"""CPU test of tests/layernorm_reference.py: over the GPU test's own case list the f32 simulation of every kernel lies inside the derived bounds (and
not vanishingly deep inside), every input profile reaches the tail it is documented to reach, every planted error is rejected by `check`, the closed
form of the backward equals float64 autograd, and the chain lengths the docstring states are the ones the simulation's loops perform."""
import collections

import pytest
import torch
import torch.nn.functional as Fn

from tests import layernorm_reference as R

SEED = 3


def _fwd_inputs(D, profile, rows):
    return R.make_inputs(profile, rows, D, SEED)


def _stats(inp, eps=R.EPS):
    e = R.emulate_fwd(inp["x"], inp["gamma"], inp["beta"], eps)
    return e["mean"], e["rstd"]


def _old(D):
    return {"dgamma": torch.linspace(-0.5, 0.75, D), "dbeta": torch.linspace(1.0, -0.25, D), "colsum": torch.full((D,), 2.0)}


def _check_fwd(tag, em, ex, tol, out_bf16, fails=None):
    w = {"mean": R.check(f"{tag} mean", em["mean"], ex["mean"], tol["mean"], fails), "rstd": R.check(f"{tag} rstd", em["rstd"], ex["rstd"], tol["rstd"], fails)}
    w["bf16" if out_bf16 else "f32"] = R.check(f"{tag} y", em["y"], ex["y"], tol["bf16" if out_bf16 else "f32"], fails)
    return w


def _check_bwd(tag, em, ex, tol, old, fails=None):
    w = {}
    for k in ("dx", "dx_bf16"):
        w[k] = R.check(f"{tag} {k}", em[k], ex["dx"], tol[k], fails)
    for k in ("dgamma", "dbeta", "colsum"):
        w[k] = R.check(f"{tag} {k}", em[k], ex[k] + old[k].double(), tol[k], fails)
    return w


def _dy_list(rows):
    if rows > 1000:
        return [("white", True), ("aligned", False)]
    return [(k, b) for k in R.DY_KINDS for b in (True, False)]


# floors: the worst err / tol this simulation measured on the randn profile, divided by 4 (measured value beside each)
FLOORS = {
    ("ln_fwd", "mean"): 0.194 / 4,
    ("ln_fwd", "rstd"): 0.198 / 4,
    ("ln_fwd", "bf16"): 0.995 / 4,        # (the bf16 rounding itself fills the bound)
    ("ln_fwd", "f32"): 0.195 / 4,
    ("ln_bwd", "dx"): 0.977 / 4,          # (sparse dy: two roundings make the whole error of most elements)
    ("ln_bwd", "dx_bf16"): 0.996 / 4,
    ("ln_bwd", "dgamma"): 0.080 / 4,
    ("ln_bwd", "dbeta"): 0.055 / 4,
    ("ln_bwd", "colsum"): 0.059 / 4,
    ("merge", "cls_ln"): 0.200 / 4,
    ("merge", "feats"): 0.993 / 4,
    ("merge", "stats1"): 0.195 / 4,
    ("merge", "stats2"): 0.073 / 4,
}


def test_emulation_inside_bounds_and_bounds_not_slack():
    worst = collections.defaultdict(float)
    fails = []

    def note(kernel, profile, w):
        for k, v in w.items():
            worst[(kernel, k, profile)] = max(worst[(kernel, k, profile)], v)

    for D, profile, rows in R.fwd_cases():
        inp = _fwd_inputs(D, profile, rows)
        for form, (d1, d2) in (("plain", (None, None)), ("delta", (inp["delta"], None)), ("delta2", (inp["delta"], inp["delta2"]))):
            ex = R.exact_fwd(inp["x"], inp["gamma"], inp["beta"], R.EPS, d1, d2)
            tol = R.bounds_fwd(ex)
            for ob in (True, False):
                em = R.emulate_fwd(inp["x"], inp["gamma"], inp["beta"], R.EPS, d1, d2, ob)
                assert torch.equal(R.bits(em["s"]), R.bits(ex["s"]))
                note("ln_fwd", profile, _check_fwd(f"fwd D={D} {profile} rows={rows} {form}", em, ex, tol, ob, fails))
    for D, profile, rows in R.bwd_cases():
        inp = _fwd_inputs(D, profile, rows)
        mean, rstd = _stats(inp)
        dres = 0.05 * torch.randn(rows, D, generator=torch.Generator().manual_seed(rows + D)) * R.row_scale(profile, rows)
        old = _old(D)
        for kind, b16 in _dy_list(rows):
            dy = R.make_dy(kind, inp["x"], mean, rstd, inp["gamma"], SEED, b16)
            ex = R.exact_bwd(dy, inp["x"], mean, rstd, inp["gamma"], dres)
            em = R.emulate_bwd(dy, inp["x"], mean, rstd, inp["gamma"], dres, old)
            note("ln_bwd", profile, _check_bwd(f"bwd D={D} {profile} rows={rows} dy={kind}/{'bf16' if b16 else 'f32'}", em, ex, R.bounds_bwd(ex, old=old), old, fails))
    for D, profile, B, P in R.merge_cases():
        inp = R.make_inputs(profile, B * (P + 1), D, SEED)
        i2 = R.make_inputs(profile, 1, D, SEED + 1)
        x = inp["x"].reshape(B, P + 1, D)
        for delta in (None, inp["delta"].reshape(B, P + 1, D)):
            ex = R.exact_merge(x, inp["gamma"], inp["beta"], i2["gamma"], i2["beta"], R.EPS, delta)
            tol = R.bounds_merge(ex)
            em = R.emulate_merge(x, inp["gamma"], inp["beta"], i2["gamma"], i2["beta"], R.EPS, delta)
            tag = f"merge D={D} {profile} B={B} P={P} delta={delta is not None}"
            note("merge", profile, {k: R.check(f"{tag} {k}", em[k], ex[k], tol[k], fails) for k in ("cls_ln", "feats", "stats1", "stats2")})
    for (kernel, out, profile), v in sorted(worst.items()):
        print(f"LNREF-CPU {kernel:7s} {out:8s} {profile:8s} worst err/tol {v:.3f}")
    assert not fails, "\n".join(fails[:20])
    for (kernel, out), floor in FLOORS.items():
        assert worst[(kernel, out, "randn")] >= floor, f"{kernel} {out}: worst err / tol {worst[(kernel, out, 'randn')]:.4f} on randn is below {floor:.4f}: the bound is slack"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# every profile reaches its tail
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [260, 768, 1024])
def test_profiles_reach_their_tails(D):
    rows = 67
    # outlier: one in vector 0 of lane 0, one in the last vector; the normalised values are small
    inp = R.make_inputs("outlier", rows, D, SEED)
    ax = inp["x"].abs()
    assert bool((ax[:, 0] >= 64).all()) and bool((ax[:, D - 1] >= 64).all()) and bool((ax[:, :4].amax(1) <= 256).all())
    nout = (ax >= 64).sum(1)
    assert int(nout.min()) >= 2 and int(nout.max()) <= 4
    ex = R.exact_fwd(inp["x"], inp["gamma"], inp["beta"])
    assert float(ex["y"].abs().median()) < 0.2
    # offset: |mean| in [2^10, 2^12], unit spread, and one-pass variance in f32 is outside the bound
    inp = R.make_inputs("offset", rows, D, SEED)
    ex = R.exact_fwd(inp["x"], inp["gamma"], inp["beta"])
    assert bool((ex["mean"].abs() >= 2.0 ** 10 - 4).all()) and bool((ex["mean"].abs() <= 2.0 ** 12 + 4).all())
    assert 0.5 < float(ex["var"].min()) and float(ex["var"].max()) < 2.0
    bad = R.emulate_fwd(inp["x"], inp["gamma"], inp["beta"], hooks=("one_pass",))
    assert float(R.ratios(bad["rstd"], ex["rstd"], R.bounds_fwd(ex)["rstd"]).max()) > 1.0
    # flat: var << eps, rstd within 1 % of eps^-1/2; exactly-zero rows give store(beta) and mean 0
    inp = R.make_inputs("flat", rows, D, SEED)
    ex = R.exact_fwd(inp["x"], inp["gamma"], inp["beta"])
    assert float(ex["var"].max()) < 1e-2 * R.EPS
    assert float((ex["rstd"] * R.EPS ** 0.5 - 1).abs().max()) < 0.01
    zero = (inp["x"] == 0).all(1)
    assert int(zero.sum()) >= rows // 3 and not bool(zero[0])
    for ob in (True, False):
        em = R.emulate_fwd(inp["x"], inp["gamma"], inp["beta"], out_bf16=ob)
        want = R.bf16_round(inp["beta"]) if ob else inp["beta"]
        assert torch.equal(R.bits(em["y"][zero]), R.bits(want.expand(int(zero.sum()), D))) and bool((em["mean"][zero] == 0).all())
    # scaled: both scales present, nothing overflows
    inp = R.make_inputs("scaled", rows, D, SEED)
    rms = inp["x"].double().pow(2).mean(1).sqrt()
    assert float(rms[0::2].max()) < 2.0 ** -39 and float(rms[1::2].min()) > 2.0 ** 39
    em = R.emulate_fwd(inp["x"], inp["gamma"], inp["beta"])
    assert bool(torch.isfinite(em["y"]).all()) and bool(torch.isfinite(em["rstd"]).all())
    # hard affine: exact zeros, negative entries, magnitude 8; some y cancel to near zero against terms of order one
    ga = inp["gamma"]
    assert bool((ga == 0).any()) and bool((ga < 0).any()) and float(ga.abs().max()) == 8.0
    inp = R.make_inputs("offset", rows, D, SEED)
    ex = R.exact_fwd(inp["x"], inp["gamma"], inp["beta"])
    cols = torch.arange(3, D, 4)
    big = inp["beta"][cols].abs() > 0.5
    assert int(big.sum()) > 0 and float(ex["y"][0, cols][big].abs().max()) < 1e-6
    # aligned dy: dx is a cancellation (|dx| / rstd far below |g dy|; with zeros in gamma it can only be partial, so on a plain affine); sparse: one
    # nonzero per row
    for prof in ("randn", "outlier"):
        i2 = R.make_inputs(prof, rows, D, SEED)
        m2, r2 = _stats(i2)
        dy = R.make_dy("aligned", i2["x"], m2, r2, i2["gamma"], SEED, False)
        eb = R.exact_bwd(dy, i2["x"], m2, r2, i2["gamma"])
        assert float((eb["dx0"] / eb["r"]).abs().median()) < 1e-2 * float(eb["gd"].abs().median())
    mean, rstd = _stats(inp)
    dy = R.make_dy("sparse", inp["x"], mean, rstd, inp["gamma"], SEED, True)
    assert bool(((dy != 0).sum(1) == 1).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# planted errors
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _rejected(fn):
    with pytest.raises(AssertionError, match="outside the bound"):
        fn()


@pytest.mark.parametrize("hook,profile,D,eps", [
    ("one_pass", "offset", 768, R.EPS),            # E[x^2] - mean^2
    ("skip_tail", "outlier", 260, R.EPS),          # lane 0's second vector (columns 256..259, the last outlier) left out of the statistics
    ("skip_tail", "randn", 1020, R.EPS),
    ("dm1", "randn", 768, R.EPS),                  # variance over D - 1
    ("eps_outside", "flat", 768, R.EPS),           # 1 / (sqrt(var) + eps)
    ("eps", "flat", 1024, 1e-6),                   # eps = 1e-6
])
def test_planted_forward_errors_are_rejected(hook, profile, D, eps):
    inp = R.make_inputs(profile, 5, D, SEED)
    ex = R.exact_fwd(inp["x"], inp["gamma"], inp["beta"])
    tol = R.bounds_fwd(ex)
    good = R.emulate_fwd(inp["x"], inp["gamma"], inp["beta"], out_bf16=False)
    _check_fwd("good", good, ex, tol, False)
    bad = R.emulate_fwd(inp["x"], inp["gamma"], inp["beta"], eps, out_bf16=False, hooks=(hook,))
    _rejected(lambda: R.check("rstd", bad["rstd"], ex["rstd"], tol["rstd"]))
    _rejected(lambda: R.check("y", bad["y"], ex["y"], tol["f32"]))


def test_planted_association_of_the_two_deltas_changes_bits():
    inp = R.make_inputs("randn", 67, 260, SEED)
    ex = R.exact_fwd(inp["x"], inp["gamma"], inp["beta"], R.EPS, inp["delta"], inp["delta2"])
    good = R.emulate_fwd(inp["x"], inp["gamma"], inp["beta"], R.EPS, inp["delta"], inp["delta2"])
    bad = R.emulate_fwd(inp["x"], inp["gamma"], inp["beta"], R.EPS, inp["delta"], inp["delta2"], hooks=("assoc",))
    assert torch.equal(R.bits(good["s"]), R.bits(ex["s"])) and not torch.equal(R.bits(bad["s"]), R.bits(ex["s"]))


@pytest.mark.parametrize("profile", ["randn", "outlier"])
def test_planted_one_bf16_ulp_is_rejected(profile):
    """an output moved by one bf16 ulp, away from the reference, in an element whose whole tolerance is below that ulp (so E < u |ref|)."""
    inp = R.make_inputs(profile, 5, 768, SEED)
    ex = R.exact_fwd(inp["x"], inp["gamma"], inp["beta"])
    tol = R.bounds_fwd(ex)["bf16"]
    em = R.emulate_fwd(inp["x"], inp["gamma"], inp["beta"])
    y = em["y"].clone()
    ulp = 2.0 ** (torch.floor(torch.log2(y.abs().double())) - 7)
    ok = (tol < ulp) & (y != 0)
    assert float(ok.double().mean()) > 0.25, "most elements must have a tolerance below one bf16 ulp"
    idx = tuple(ok.nonzero()[len(ok.nonzero()) // 2].tolist())
    assert float((tol - R.U * ex["y"].abs() * (1 + R.U))[idx]) < float(R.U * ex["y"].abs()[idx])          # E < u |ref|
    y[idx] = y[idx] + float(ulp[idx]) * (1.0 if float(y[idx]) >= float(ex["y"][idx]) else -1.0)
    assert float(R.bf16_round(y)[idx]) == float(y[idx])
    R.check("good", em["y"], ex["y"], tol)
    _rejected(lambda: R.check("ulp", y, ex["y"], tol))


@pytest.mark.parametrize("hook,out,profile,dykind,rows", [
    ("no_s2", "dx", "randn", "white", 67),
    ("no_s2", "dx", "flat", "aligned", 67),
    ("mean_dy", "dx", "offset", "white", 67),          # mean(dy) in place of mean(g dy): needs gamma != 1
    ("no_dres", "dx", "randn", "white", 67),
    ("drop_last_row", "dgamma", "randn", "white", 67),
    ("drop_last_row", "dgamma", "outlier", "sparse", 131),
    ("drop_slab16", "dbeta", "randn", "white", 1100),
    ("drop_slab16", "dgamma", "outlier", "white", 2100),
])
def test_planted_backward_errors_are_rejected(hook, out, profile, dykind, rows):
    D = 128 if rows > 1000 else 260
    inp = R.make_inputs(profile, rows, D, SEED)
    mean, rstd = _stats(inp)
    dres = 0.05 * torch.randn(rows, D, generator=torch.Generator().manual_seed(1))
    dy = R.make_dy(dykind, inp["x"], mean, rstd, inp["gamma"], SEED, True)
    old = _old(D)
    ex = R.exact_bwd(dy, inp["x"], mean, rstd, inp["gamma"], dres)
    tol = R.bounds_bwd(ex, old=old)
    _check_bwd("good", R.emulate_bwd(dy, inp["x"], mean, rstd, inp["gamma"], dres, old), ex, tol, old)
    bad = R.emulate_bwd(dy, inp["x"], mean, rstd, inp["gamma"], dres, old, hooks=(hook,))
    ref = ex[out] if out == "dx" else ex[out] + old[out].double()
    _rejected(lambda: R.check(out, bad[out], ref, tol[out]))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the closed form and the counts
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", R.PROFILES)
def test_closed_form_backward_equals_float64_autograd(profile):
    rows, D = 5, 260
    inp = R.make_inputs(profile, rows, D, SEED)
    ex = R.exact_fwd(inp["x"], inp["gamma"], inp["beta"])
    dy = R.make_dy("white", inp["x"], ex["mean"], ex["rstd"], inp["gamma"], SEED, False).double()
    x = inp["x"].double().requires_grad_(True); g = inp["gamma"].double().requires_grad_(True); b = inp["beta"].double().requires_grad_(True)
    Fn.layer_norm(x, (D,), g, b, ex["eps"]).backward(dy)
    eb = R.exact_bwd(dy, inp["x"], ex["mean"], ex["rstd"], inp["gamma"])           # float64 statistics: the exact ones
    # two float64 evaluations of one formula: 8 D roundings of the terms, times the condition of x -> xhat (1 + rstd max |x|: the subtraction of the mean)
    d64 = 8 * D * 2.0 ** -53 * (1.0 + float((eb["r"][:, 0] * inp["x"].double().abs().amax(1)).max()))
    assert float((eb["dx"] - x.grad).abs().max()) <= d64 * float((eb["r"] * (eb["gd"].abs() + eb["xh"].abs() * eb["s2"].abs())).max())
    assert float((eb["dgamma"] - g.grad).abs().max()) <= d64 * float((eb["dy"].abs() * (1.0 + eb["xh"].abs())).sum(0).max())
    assert float((eb["dbeta"] - b.grad).abs().max()) <= d64 * float(eb["dy"].abs().sum(0).max())


@pytest.mark.parametrize("D", R.WIDTHS)
def test_chain_lengths_are_the_ones_the_simulation_performs(D):
    """n_s and n_r are UPPER bounds of the longest path of any element: the simulation's counters add one per executed add statement of the chain
    (4 per vector: three inside the vector and one onto the lane's sum), while the deepest element of a row sum passes 3 + nv + 6 of them; the count
    the bound uses is the larger, statement-wise one."""
    c = {}
    inp = R.make_inputs("randn", 2, D, SEED)
    R.emulate_fwd(inp["x"], inp["gamma"], inp["beta"], counts=c)
    assert c["n_sum"] == R.n_sum(D) == 4 * ((D + 255) // 256) + 6
    for rows in (64, 131, 1100, 2100) if D == 128 else (64,):
        inp = R.make_inputs("randn", rows, D, SEED)
        mean, rstd = _stats(inp)
        c = {}
        R.emulate_bwd(inp["x"] * 0.1, inp["x"], mean, rstd, inp["gamma"], None, _old(D), counts=c)
        assert c["n_sum"] == R.n_sum(D)
        assert c["n_rows"] == R.n_rows(rows) == 16 + 3 + ((rows + 63) // 64 + 15) // 16 + 15 + 1


# ---------------------------------------------------------------------------------------------------------------------------------------------
# merge backward (merge_ln_bwd_kernel + cls_ln_bwd_kernel)
# ---------------------------------------------------------------------------------------------------------------------------------------------
MB_OUTS = ("dx", "dx_bf16", "dcls", "dg1", "db1", "dg2", "db2", "colsum")
# measured on the randn profile by the simulation, divided by 4 (measured value beside each)
MB_FLOORS = {"dx": 0.224 / 4, "dx_bf16": 0.995 / 4, "dcls": 0.121 / 4, "dg1": 0.082 / 4, "db1": 0.076 / 4,
             "dg2": 0.034 / 4, "db2": 0.021 / 4, "colsum": 0.032 / 4}


def _old_merge(D):
    return {"dg1": torch.linspace(-0.5, 0.75, D), "db1": torch.linspace(1.0, -0.25, D), "dg2": torch.full((D,), -1.5), "db2": torch.linspace(0.25, 2.0, D),
            "colsum": torch.full((D,), 2.0)}


def _merge_bwd_case(D, profile, B, P, kind):
    """inputs of one merge backward case: the forward simulation's own statistics and class row are what the backward is given."""
    inp = R.make_inputs(profile, B * (P + 1), D, SEED)
    i2 = R.make_inputs(profile, 1, D, SEED + 1)
    x = inp["x"].reshape(B, P + 1, D)
    fw = R.emulate_merge(x, inp["gamma"], inp["beta"], i2["gamma"], i2["beta"])
    given = {"stats1": fw["stats1"], "stats2": fw["stats2"], "cls_ln": fw["cls_ln"]}
    df = R.make_dfeats(kind, x, given, inp["gamma"], inp["beta"], i2["gamma"], SEED)
    return x, df, given, (inp["gamma"], inp["beta"], i2["gamma"])


def _check_merge_bwd(tag, em, ex, tol, old, fails=None):
    w = {}
    for k in MB_OUTS:
        ref = ex["dx"] if k == "dx_bf16" else ex[k] + (old[k].double() if k in old else 0.0)
        w[k] = R.check(f"{tag} {k}", em[k], ref, tol[k], fails)
    return w


def test_merge_backward_emulation_inside_bounds_and_bounds_not_slack():
    worst = collections.defaultdict(float)
    fails = []
    for D, profile, B, P in R.merge_cases():
        old = _old_merge(D)
        for kind in R.DFEATS_KINDS:
            x, df, given, (g1, b1, g2) = _merge_bwd_case(D, profile, B, P, kind)
            ex = R.exact_merge_bwd(df, x, g1, b1, g2, R.EPS, given)
            em = R.emulate_merge_bwd(df, x, given["cls_ln"], given["stats1"], given["stats2"], g1, b1, g2, old)
            for k, v in _check_merge_bwd(f"merge_bwd D={D} {profile} B={B} P={P} {kind}", em, ex, R.bounds_merge_bwd(ex, old), old, fails).items():
                worst[(k, profile)] = max(worst[(k, profile)], v)
    for (out, profile), v in sorted(worst.items()):
        print(f"LNREF-CPU mrg_bwd {out:8s} {profile:8s} worst err/tol {v:.3f}")
    assert not fails, "\n".join(fails[:20])
    for out, floor in MB_FLOORS.items():
        assert worst[(out, "randn")] >= floor, f"merge_bwd {out}: worst err / tol {worst[(out, 'randn')]:.4f} on randn is below {floor:.4f}: the bound is slack"


@pytest.mark.parametrize("profile,B,P", [("randn", 2, 37), ("outlier", 3, 67), ("randn", 1, 1)])
def test_planted_merge_backward_without_class_rows_is_rejected(profile, B, P):
    D = 260
    old = _old_merge(D)
    x, df, given, (g1, b1, g2) = _merge_bwd_case(D, profile, B, P, "white")
    ex = R.exact_merge_bwd(df, x, g1, b1, g2, R.EPS, given)
    tol = R.bounds_merge_bwd(ex, old)
    _check_merge_bwd("good", R.emulate_merge_bwd(df, x, given["cls_ln"], given["stats1"], given["stats2"], g1, b1, g2, old), ex, tol, old)
    bad = R.emulate_merge_bwd(df, x, given["cls_ln"], given["stats1"], given["stats2"], g1, b1, g2, old, hooks=("no_cls_param",))
    for k in ("dg1", "db1"):
        _rejected(lambda: R.check(k, bad[k], ex[k] + old[k].double(), tol[k]))


@pytest.mark.parametrize("profile", R.PROFILES)
def test_closed_form_merge_backward_equals_float64_autograd(profile):
    B, P, D = 2, 5, 260
    inp = R.make_inputs(profile, B * (P + 1), D, SEED)
    i2 = R.make_inputs(profile, 1, D, SEED + 1)
    x = inp["x"].reshape(B, P + 1, D)
    e = R.eps32(R.EPS)
    df = 0.1 * torch.randn(B, P, D, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    X = x.double().requires_grad_(True)
    G1, B1, G2, B2 = (t.double().requires_grad_(True) for t in (inp["gamma"], inp["beta"], i2["gamma"], i2["beta"]))
    y = Fn.layer_norm(X, (D,), G1, B1, e)
    y.retain_grad()
    Fn.layer_norm(y[:, 1:] * y[:, :1], (D,), G2, B2, e).backward(df)
    ex = R.exact_merge_bwd(df, x, inp["gamma"], inp["beta"], i2["gamma"], R.EPS)             # given=None: the exact statistics and class row
    # two float64 evaluations of one expression: relative to the size of each output, times the condition of the two normalisations (the subtractions of
    # the means: 1 + rstd max |v|) and 16 D roundings
    m = R.exact_merge(x, inp["gamma"], inp["beta"], i2["gamma"], i2["beta"])
    cond = (1.0 + float((m["stats1"][..., 1] * x.double().abs().amax(-1)).max())) * (1.0 + float((m["stats2"][..., 1] * m["z"].abs().amax(-1)).max()))
    d64 = 16 * D * 2.0 ** -53 * cond
    for k, ref in (("dx", X.grad), ("dg1", G1.grad), ("db1", B1.grad), ("dg2", G2.grad), ("db2", B2.grad), ("colsum", X.grad.sum((0, 1)))):
        scale = float(ref.abs().max()) + float(ex["dx"].abs().max())
        assert float((ex[k] - ref).abs().max()) <= d64 * scale * (B * (P + 1) if ref.dim() == 1 else 1), (k, float((ex[k] - ref).abs().max()), d64 * scale)


@pytest.mark.parametrize("B,P", R.MERGE_BP + ((17, 70),))
def test_merge_backward_chain_lengths(B, P):
    """the row chains `bounds_merge_bwd` charges are upper bounds of what the simulation's loops perform (equal when a 64-row block is full)."""
    D = 128
    x, df, given, (g1, b1, g2) = _merge_bwd_case(D, "randn", B, P, "white")
    c = {}
    R.emulate_merge_bwd(df, x, given["cls_ln"], given["stats1"], given["stats2"], g1, b1, g2, _old_merge(D), counts=c)
    full = 64 - min(P, 64)
    assert c["n_dcls"] == R.n_rows_merge(B, P, False) - full
    assert c["n_param"] == R.n_rows_merge(B, P) - full
    assert c["n_cls"] == R.n_rows_cls(B)
    assert R.N_MOMENT == 3 + 6 + 3 + 2
