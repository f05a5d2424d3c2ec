"""CPU test of tests/heads_reference.py: every closed form equals float64 autograd of the reference expression, every profile reaches what it names,
the f32 simulation of every kernel lies inside the derived bounds on every profile, the arg-max equality is excused on at most 1 % of the
(row, class) pairs, every planted error is rejected, and the shape lists kept for the GPU test reach every form of the launchers."""
import pytest
import torch
import torch.nn.functional as Fn

from tests import heads_reference as R

SEED = 5


def _pool(s_all, C):
    return Fn.max_pool1d(s_all[None], 3, 3)[0]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# closed forms == float64 autograd
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile,C", [("randn", 10), ("trained", 3), ("aligned", 1), ("tiny", 3)])
def test_class_head_closed_forms_equal_autograd(profile, C):
    rows, Dt = 23, 64
    inp = R.make_inputs(profile, rows, Dt, C, SEED)
    e = inp["e"].double().requires_grad_(True)
    Q = inp["Q"].double().requires_grad_(True)
    qh = Q / torch.linalg.norm(Q, dim=-1, keepdim=True) + R.EPS6
    qh.retain_grad()
    # (the norm with torch's subgradient 0 at 0: linalg.norm's backward is that)
    s_all = (e / (torch.linalg.norm(e, dim=-1, keepdim=True) + R.EPS6)) @ qh.t()
    sims = _pool(s_all, C)
    ex_q = R.exact_qhat(inp["Q"])
    assert torch.allclose(ex_q["qhat"], qh.detach(), rtol=1e-13, atol=0)
    table = R.to_table(qh.detach(), C, False)
    ex = R.exact_sims(inp["e"], table, C)
    assert torch.allclose(ex["sims"], sims.detach(), rtol=1e-12, atol=1e-300)
    assert torch.equal(ex["argmax"], s_all.detach().view(rows, C, 3).argmax(-1))
    assert torch.allclose(ex["margin"], (lambda t: t[..., 0] - t[..., 1])(s_all.detach().view(rows, C, 3).topk(2, -1).values), atol=1e-15)
    ds = R.make_dsims(profile, ex["sims"], SEED).double()
    sims.backward(ds)
    b = R.exact_sims_bwd(ds, inp["e"], table, ex["sims"], ex["argmax"], ex["inv"])
    scale = float(e.grad.abs().max())
    assert float((b["de"] - e.grad).abs().max()) <= 1e-10 * scale
    zero = (inp["e"] == 0).all(1)
    if profile == "tiny":
        assert bool(zero.any()) and bool(torch.isfinite(e.grad[zero]).all()) and float(e.grad[zero].abs().max()) > 0
    # dqhat = G^T e at exact G, then the normalisation's backward
    inv = ex["inv"]
    Gx = torch.zeros(rows, 32, dtype=torch.float64)
    Gx.scatter_(1, R.prompt_cols(C, False)[None] + ex["argmax"], ds * inv[:, None])
    dqhat = Gx.t() @ inp["e"].double()
    assert float((dqhat[:3 * C] - qh.grad).abs().max()) <= 1e-10 * float(qh.grad.abs().max())
    old = torch.randn(3 * C, Dt, dtype=torch.float64)
    qb = R.exact_qhat_bwd(qh.grad, inp["Q"], old)
    assert float((qb["dq"] - old - Q.grad).abs().max()) <= 1e-10 * float(Q.grad.abs().max())


def test_wide_reference_is_the_narrow_one_per_block():
    C, rows, Dt = 23, 9, 64
    inp = R.make_inputs("randn", rows, Dt, C, SEED, wide=True)
    ex = R.exact_sims(inp["e"], inp["qhat"], C, wide=True)
    for b in range(3):
        Cb = min(10, C - 10 * b)
        nb = R.exact_sims(inp["e"], inp["qhat"][32 * b:32 * b + 32], Cb)
        assert torch.equal(nb["sims"], ex["sims"][:, 10 * b:10 * b + Cb]) and torch.equal(nb["argmax"], ex["argmax"][:, 10 * b:10 * b + Cb])
    ds = R.make_dsims("randn", ex["sims"], SEED)
    w = R.exact_sims_bwd(ds, inp["e"], inp["qhat"], ex["sims"], ex["argmax"], ex["inv"], wide=True)
    assert w["G"].shape == (rows, 256) and int((w["G"] != 0).sum()) <= rows * C
    cols = (R.prompt_cols(C, True)[None] + ex["argmax"])
    keep = torch.zeros(rows, 256, dtype=torch.bool).scatter_(1, cols, True)
    assert bool((w["G"][~keep] == 0).all())


@pytest.mark.parametrize("profile", R.BOX_PROFILES)
def test_box_closed_forms_equal_autograd(profile):
    rows, D = 21, 64
    inp = R.make_box_inputs(profile, rows, D, SEED)
    u = inp["u1"].double().requires_grad_(True)
    W = inp["w2"].double().requires_grad_(True)
    b2 = inp["b2"].double().requires_grad_(True)
    gel = Fn.gelu(u)
    hq = inp["h1"].double() + (gel - gel.detach())            # value = the saved bf16 h1, gradient = gelu'(u)
    x = hq @ W.t() + b2 + inp["box_bias"].double()[torch.arange(rows) % inp["P"]]
    s = torch.sigmoid(x)
    boxes = R._corners(s)
    ex = R.exact_box_final(inp["h1"], inp["w2"], inp["b2"], inp["box_bias"], inp["P"])
    assert torch.allclose(ex["sig"], s.detach(), rtol=1e-13, atol=0) and torch.allclose(ex["boxes"], boxes.detach(), rtol=1e-13, atol=1e-300)
    boxes.backward(inp["dboxes"].double())
    bw = R.exact_box_final_bwd(inp["dboxes"], s.detach(), inp["h1"], inp["u1"], inp["w2"])
    for k, ref in (("du1", u.grad), ("dW2", W.grad), ("db2", b2.grad)):
        assert float((bw[k] - ref).abs().max()) <= 1e-9 * max(float(ref.abs().max()), 1e-300), k
    assert float((bw["colsum"] - u.grad.sum(0)).abs().max()) <= 1e-9 * max(float(u.grad.abs().max()), 1e-300)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# profiles reach what they name
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_profiles_reach_their_claims():
    rows, Dt, C = 300, 512, 10
    tr = R.make_inputs("trained", rows, Dt, C, SEED)
    n = tr["e"].norm(dim=-1)
    assert float(n.min()) < 2.0 ** -5 and float(n.max()) > 2.0 ** 5
    cr = (tr["e"] / n[:, None]).pow(2).mean(0).sqrt().sort().values            # column RMS of the unit rows: three channels 16 x the rest
    assert float(cr[-3]) > 12 * float(cr.median()) and float(cr[-4]) < 2 * float(cr.median())
    q = tr["Q"].double().view(C, 3, Dt)
    qn = q / q.norm(dim=-1, keepdim=True)
    assert float((qn @ qn.transpose(1, 2)).min()) >= 0.98
    ex = R.exact_sims(tr["e"], tr["qhat"], C)
    tol = R.bounds_sims(ex)
    E3 = tol["prods"].view(rows, C, 3)
    need = (E3.gather(2, ex["argmax"][..., None]) + E3.gather(2, ex["second"][..., None]))[..., 0]
    assert float(ex["margin"].median()) < 0.02 and float((ex["margin"] > need).double().mean()) >= 0.99          # small margins, but above the bound
    ti = R.make_inputs("ties", rows, Dt, C, SEED)
    assert bool((ti["e"][:, list(R.TIE_COLS)] == 0).all())
    t = ti["qhat"][:30].view(C, 3, Dt)
    for c in range(C):
        if c % 3 == 0:
            assert torch.equal(t[c, 0], t[c, 1]) and torch.equal(t[c, 0], t[c, 2])
        elif c % 3 == 1:
            assert torch.equal(t[c, 1], t[c, 2]) and not torch.equal(t[c, 0], t[c, 1])
        else:
            keep = torch.ones(Dt, dtype=torch.bool); keep[list(R.TIE_COLS)] = False
            assert torch.equal(t[c, 0, keep], t[c, 1, keep]) and torch.equal(t[c, 0, keep], t[c, 2, keep]) and not torch.equal(t[c, 0], t[c, 1])
    ext = R.exact_sims(ti["e"], ti["qhat"], C)
    tk = ti["tie_kind"]
    assert bool((ext["argmax"][:, (tk == 1) | (tk == 3)] == 0).all()) and bool((ext["argmax"][:, tk == 2] != 2).all())
    assert bool((ext["margin"][:, (tk == 1) | (tk == 3)] == 0).all())
    ty = R.make_inputs("tiny", rows, Dt, C, SEED)
    ny = ty["e"].double().norm(dim=-1)
    assert bool((ny[0::7] == 0).all())
    for lvl in (1e-3, 1e-5, 1e-7):
        assert int(((ny > 0.5 * lvl) & (ny < 2 * lvl)).sum()) > rows // 5
    al = R.make_inputs("aligned", rows, Dt, C, SEED)
    exa = R.exact_sims(al["e"], al["qhat"], C)
    ds = R.make_dsims("aligned", exa["sims"], SEED).double()
    resid = ds - (ds * exa["sims"]).sum(-1, keepdim=True) / (exa["sims"] ** 2).sum(-1, keepdim=True) * exa["sims"]
    assert float(resid.abs().max()) < 1e-2 and float(ds.abs().max()) > 0.1
    sa = R.make_box_inputs("saturated", rows, 512, SEED)
    ax = sa["x"].abs()
    assert float(ax.min()) >= 8 - 1e-3 and float(ax.max()) > 90 and float(ax[ax < 50].max()) > 39
    s = sa["sig"]
    assert float(s[s > 0].min()) < 1e-17 and bool((s == 0).any()) and bool((s == 1).any()) and float(s[s < 1].max()) > 1 - 1e-7
    assert float((torch.exp(-sa["x"].float()) == float("inf")).float().sum()) > 0          # expf overflows on the far side
    g = sa["dboxes"]
    assert float(((g[:, 2] - g[:, 0]).abs() / g[:, 0].abs().clamp(min=1e-3)).max()) < 1e-4


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the emulation inside every bound, the planted errors outside
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _sims_checks(inp, C, wide, em, fails, tag):
    rows = inp["e"].shape[0]
    ex = R.exact_sims(inp["e"], inp["qhat"], C, wide)
    tol = R.bounds_sims(ex)
    w = {"sims": R.check(f"{tag} sims", em["sims"][:rows], ex["sims"], tol["sims"], fails),
         "inv": R.check(f"{tag} inv", em["inv"][:rows], ex["inv"], tol["inv"], fails)}
    share = R.check_argmax(f"{tag} argmax", em["argmax"][:rows], ex, tol["prods"], fails, inp["tie_kind"] if bool(inp["tie_kind"].any()) else None)
    for k in ("sims", "argmax", "inv"):                                            # the buffers started at 7
        t = em[k].reshape(em[k].shape[0], -1).float()
        R.untouched(f"{tag} {k} pad", t, torch.full_like(t, 7.0), rows, 0, t.shape[1], fails)
    return ex, tol, w, share


def _bwd_checks(inp, ex, ds, wide, em, fails, tag, given=None):
    rows, Dt = inp["e"].shape
    gv = given or {"sims": ex["sims"].float(), "argmax": ex["argmax"].to(torch.uint8), "inv": ex["inv"].float()}
    xb = R.exact_sims_bwd(ds, inp["e"], inp["qhat"], gv["sims"], gv["argmax"], gv["inv"], wide)
    tol = R.bounds_sims_bwd(xb, Dt)
    w = {"de": R.check(f"{tag} de", em["de"][:rows], xb["de"], tol["de"], fails)}
    for k in ("G", "e_bf16"):
        if not torch.equal(R.bits(em[k][:rows].bfloat16()), R.bits(xb[k])):
            fails.append(f"{tag} {k}: bits differ in {int((R.bits(em[k][:rows].bfloat16()) != R.bits(xb[k])).sum())} elements")
        if not bool((em[k][rows:] == 7.0).all()):
            fails.append(f"{tag} {k}: pad rows written")
    if not bool((em["de"][rows:] == 7.0).all()):
        fails.append(f"{tag} de: pad rows written")
    return w


CPU_CLASS_CASES = [(37, 64, 3, False), (37, 192, 10, False), (41, 512, 1, False), (37, 192, 11, True), (9, 64, 81, True)]


@pytest.mark.parametrize("rows,Dt,C,wide", CPU_CLASS_CASES)
@pytest.mark.parametrize("profile", R.PROFILES)
def test_class_head_emulation_inside_bounds(profile, rows, Dt, C, wide):
    inp = R.make_inputs(profile, rows, Dt, C, SEED, wide)
    fails = []
    tag = f"{profile} rows={rows} Dt={Dt} C={C}"
    em = R.emulate_sims(inp["e"], inp["qhat"], C, wide)
    ex, tol, w, share = _sims_checks(inp, C, wide, em, fails, tag)
    ds = R.make_dsims(profile, ex["sims"], SEED)
    given = {"sims": em["sims"][:rows], "argmax": em["argmax"][:rows], "inv": em["inv"][:rows]}
    eb = R.emulate_sims_bwd(ds, given["sims"], given["argmax"], given["inv"], inp["e"], inp["qhat"], wide)
    w.update(_bwd_checks(inp, ex, ds, wide, eb, fails, tag, given))
    xb = R.exact_sims_bwd(ds, inp["e"], inp["qhat"], given["sims"], given["argmax"], given["inv"], wide)
    w["de_f32"] = R.check(f"{tag} de before its bf16 rounding", eb["de_f32"], xb["de"], R.bounds_sims_bwd(xb, Dt)["de_f32"], fails)
    print(f"HEADSREF-CPU {tag}: " + " ".join(f"{k} {v:.3f}" for k, v in w.items()) + f" argmax excused {share:.4f}")
    assert not fails, "\n".join(fails[:10])
    if profile != "ties":
        assert share <= 0.01, share
    assert w["inv"] > 0.01 and w["de"] > 0.25 and w["de_f32"] > 0.01, ("a bound this slack catches nothing", w)        # (sims: the order-independent dot bound, slack by sqrt(Dt): profiles/heads_reference.md)
    # the defect: without the select, a zero row of e gives NaN -- outside every bound
    if profile == "tiny":
        bad = []
        _bwd_checks(inp, ex, ds, wide, R.emulate_sims_bwd(ds, given["sims"], given["argmax"], given["inv"], inp["e"], inp["qhat"], wide, fixed=False), bad, tag, given)
        assert bad and "de" in bad[0]


def test_qhat_emulation_inside_bounds_and_planted():
    for nq, Dt in ((3, 64), (30, 192), (32, 768)):
        Q = torch.randn(nq, Dt, generator=torch.Generator().manual_seed(nq)) * 3.0
        ex = R.exact_qhat(Q)
        tol = R.bounds_qhat(ex)
        t, n = R.emulate_qhat(Q, C=nq // 3 if nq % 3 == 0 else None)
        w1 = R.check("qhat", t[:nq], ex["qhat"], tol["qhat"])
        R.check("qnorm", n, ex["n"], tol["qnorm"])
        assert bool((t[nq:] == 0).all()) and w1 > 0.05
        with pytest.raises(AssertionError):
            R.check("qhat", R.emulate_qhat(Q, C=nq // 3 if nq % 3 == 0 else None, hooks=("eps_inside",))[0][:nq], ex["qhat"], tol["qhat"])
        dh = torch.randn(nq, Dt, generator=torch.Generator().manual_seed(nq + 1))
        old = torch.randn(nq, Dt, generator=torch.Generator().manual_seed(nq + 2))
        xb = R.exact_qhat_bwd(dh, Q, old)
        tb = R.bounds_qhat_bwd(xb)
        w2 = R.check("dq", R.emulate_qhat_bwd(dh, Q, old), xb["dq"], tb["dq"])
        assert w2 > 0.01
        with pytest.raises(AssertionError):
            R.check("dq", R.emulate_qhat_bwd(dh, Q, old, hooks=("no_projection",)), xb["dq"], tb["dq"])


def _planted_fwd(profile, rows, Dt, C, wide, hook):
    inp = R.make_inputs(profile, rows, Dt, C, SEED, wide)
    fails = []
    _sims_checks(inp, C, wide, R.emulate_sims(inp["e"], inp["qhat"], C, wide, hooks=(hook,)), fails, hook)
    return fails


@pytest.mark.parametrize("profile,Dt,C,wide,hook", [
    ("randn", 64, 3, False, "drop_half"), ("randn", 192, 3, False, "drop_half"), ("trained", 192, 10, False, "drop_half"),
    ("randn", 64, 3, False, "masked_live"), ("randn", 192, 10, False, "masked_live"),
    ("randn", 192, 3, False, "clamp_store"), ("ties", 192, 10, False, "ge_max"), ("randn", 192, 10, False, "col_off"), ("trained", 192, 10, False, "col_off"),
    ("trained", 192, 3, False, "inv_neighbor"), ("tiny", 192, 3, False, "inv_neighbor"), ("randn", 64, 11, True, "wide_pad_class"),
])
def test_planted_forward_errors_are_caught(profile, Dt, C, wide, hook):
    assert not _planted_fwd(profile, 37, Dt, C, wide, "none"), "the clean emulation must pass"
    fails = _planted_fwd(profile, 37, Dt, C, wide, hook)
    assert fails, f"{hook} on {profile} was not caught"


@pytest.mark.parametrize("profile,C,wide,hook", [
    ("randn", 10, False, "G_second"), ("trained", 10, False, "G_second"), ("aligned", 3, False, "coef_sign"), ("trained", 10, False, "coef_sign"),
    ("randn", 3, False, "stale_last"), ("trained", 10, False, "stale_last"), ("randn", 81, True, "skip_chunk2"), ("randn", 11, True, "G_second"),
    ("aligned", 11, True, "coef_sign"),
])
def test_planted_backward_errors_are_caught(profile, C, wide, hook):
    rows, Dt = 37, 64
    inp = R.make_inputs(profile, rows, Dt, C, SEED, wide)
    em = R.emulate_sims(inp["e"], inp["qhat"], C, wide)
    ex = R.exact_sims(inp["e"], inp["qhat"], C, wide)
    ds = R.make_dsims(profile, ex["sims"], SEED)
    given = {"sims": em["sims"][:rows], "argmax": em["argmax"][:rows], "inv": em["inv"][:rows]}
    hooks = {hook: ex["second"] if hook == "G_second" else True}
    clean, fails = [], []
    _bwd_checks(inp, ex, ds, wide, R.emulate_sims_bwd(ds, given["sims"], given["argmax"], given["inv"], inp["e"], inp["qhat"], wide), clean, "clean", given)
    assert not clean, clean
    _bwd_checks(inp, ex, ds, wide, R.emulate_sims_bwd(ds, given["sims"], given["argmax"], given["inv"], inp["e"], inp["qhat"], wide, hooks=hooks), fails, hook, given)
    assert fails, f"{hook} on {profile} was not caught"


def _box_bwd(inp, old, hooks=None, fails=None):
    rows, D = inp["h1"].shape
    ex = R.exact_box_final_bwd(inp["dboxes"], inp["sig"], inp["h1"], inp["u1"], inp["w2"], old)
    tol = R.bounds_box_final_bwd(ex, old)
    em = R.emulate_box_final_bwd(inp["dboxes"], inp["sig"], inp["h1"], inp["u1"], inp["w2"], old, hooks)
    return {k: R.check(k, em[k], ex[k], tol[k], fails) for k in ("du1", "dW2", "db2", "colsum")}


@pytest.mark.parametrize("profile", R.BOX_PROFILES)
@pytest.mark.parametrize("rows,D", [(1, 8), (9, 516), (300, 128), (2304, 64), (4097, 8)])
def test_box_emulation_inside_bounds(profile, rows, D):
    inp = R.make_box_inputs(profile, rows, D, SEED)
    ex = R.exact_box_final(inp["h1"], inp["w2"], inp["b2"], inp["box_bias"], inp["P"])
    tol = R.bounds_box_final(ex)
    em = R.emulate_box_final(inp["h1"], inp["w2"], inp["b2"], inp["box_bias"], inp["P"])
    w = {"sig": R.check("sig", em["sig"], ex["sig"], tol["sig"]), "boxes": R.check("boxes", em["boxes"], ex["boxes"], tol["boxes"])}
    if profile == "saturated":
        small = ex["sig"] < 1e-3
        assert float((tol["sig"][small] / ex["sig"][small].clamp(min=R.TINY * 1e6)).median()) < 1e-3       # relative (|x| times the dot product's error), not 1e-6 absolute
    w.update(_box_bwd(inp, R.box_old(D)))
    print(f"HEADSREF-CPU box {profile} rows={rows} D={D}: " + " ".join(f"{k} {v:.3f}" for k, v in w.items()))
    assert w["du1"] > 0.25 and w["sig"] > 0.01


@pytest.mark.parametrize("profile,hook,val", [("randn", "dW2_drop_last_row", 3), ("randn", "db2_drop_wave", 2), ("randn", "no_dgelu_group", 5),
                                              ("saturated", "no_dgelu_group", 0), ("saturated", "sig_from", None), ("randn", "sig_from", None)])
def test_planted_box_errors_are_caught(profile, hook, val):
    rows, D = 2304, 64
    inp = R.make_box_inputs(profile, rows, D, SEED)
    old = R.box_old(D)
    if hook == "sig_from":
        val = R.emulate_box_final(inp["h1"], inp["w2"], inp["b2"], inp["box_bias"], inp["P"])["boxes"]
    fails = []
    _box_bwd(inp, old, {hook: val}, fails)
    assert fails, f"{hook} was not caught"
    with pytest.raises(AssertionError):          # and the forward without its box bias
        ex = R.exact_box_final(inp["h1"], inp["w2"], inp["b2"], inp["box_bias"], inp["P"])
        R.check("sig", R.emulate_box_final(inp["h1"], inp["w2"], inp["b2"], inp["box_bias"], inp["P"], hooks=("no_box_bias",))["sig"], ex["sig"],
                R.bounds_box_final(ex)["sig"])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the shape lists reach every form
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_shape_lists_reach_every_form():
    assert R.sims_waves(R.SIMS_FWD_TALL[0]) == 5 and R.sims_waves(R.SIMS_FWD_TALL[0] - 33) == 4
    assert R.cdiv(R.cdiv(R.SIMS_FWD_TALL[0], 32), 5) * 5 > R.cdiv(R.SIMS_FWD_TALL[0], 32)            # a last workgroup with waves past the rows
    assert all(R.sims_waves(r) == 4 for r in R.SIMS_FWD_ROWS) and {r % 32 for r in R.SIMS_FWD_ROWS} >= {1, 31}
    by = {"generic": set(), "pf": set()}
    exits, odd = set(), False
    for rows, Dt in R.SIMS_BWD:
        k = R.sims_bwd_kernel(Dt)
        by[k].add(R.sims_bwd_rpw(rows))
        if k == "pf":
            exits |= R.sims_bwd_exits(rows)
        else:
            odd |= R.sims_bwd_odd_tail(rows)
    assert by["pf"] == {2, 3, 4, 5, 18} and {2, 3, 18} <= by["generic"] and exits == {"cond", "break1", "break2", "break3"} and odd
    assert {Dt for _, Dt in R.SIMS_BWD} == {64, 192, 512, 768}
    assert [R.wide_nt(Dt) for Dt in R.WIDE_NT_DT] == [1, 1, 2, 4, 6, 8] and R.wide_qp(80) == 256 and R.wide_qp(81) == 512 and R.wide_qp(384) == 1280
    for cases, cs in ((R.sims_fwd_cases(), R.NARROW_C), (R.sims_bwd_cases(), R.NARROW_C), (R.wide_cases(), R.WIDE_C)):
        assert {p for *_, p in cases} == set(R.PROFILES) and {c for _, _, c, _ in cases} == set(cs)
        assert len(set(cases)) == len(cases)
    assert {(r, d) for r, d, _, _ in R.sims_fwd_cases()} >= {(r, d) for r in R.SIMS_FWD_ROWS for d in R.SIMS_FWD_DT} | {R.SIMS_FWD_TALL}
    assert {(r, d) for r, d, _, _ in R.sims_bwd_cases()} == set(R.SIMS_BWD)
    wc = R.wide_cases()
    assert {(r, d, c) for r, d, c, _ in wc} >= {(r, d, c) for r in R.WIDE_ROWS for d in R.WIDE_DT for c in R.WIDE_C} | {(33, d, 11) for d in R.WIDE_NT_DT}
    assert {p for r, d, c, p in wc if c == 81} == set(R.PROFILES)
    forms = {rows: R.box_bwd_forms(rows) for rows, _ in R.BOX_BWD}
    assert forms[4097] == {"rpb": 9, "ragged": True, "tall": True, "nr_mod4": True} and R.box_bwd_rpb(4096) == 8
    assert forms[32257]["rpb"] == 64 and forms[32257]["ragged"] and R.box_bwd_rpb(32256) == 63
    assert forms[2304]["tall"] and not forms[300]["tall"] and {D for _, D in R.BOX_BWD} == {8, 128, 516, 768, 1024}
    assert {r for r, _ in R.BOX_BWD} >= {1, 7, 9, 2304}


@pytest.mark.parametrize("profile", [p for p in R.PROFILES if p != "ties"])
def test_argmax_excused_share_over_the_gpu_cases(profile):
    """The share of (row, class) pairs of the GPU test's own cases whose arg-max is excused from equality: a property of the inputs and the bound,
    so it is held to the 1 % here, per profile, over every case below 1000 rows."""
    excused = pairs = 0
    for wide, cases in ((False, R.sims_fwd_cases() + R.sims_bwd_cases()), (True, R.wide_cases())):
        for rows, Dt, C, p in set(cases):
            if p != profile or rows > 1000:
                continue
            inp = R.make_inputs(p, rows, Dt, C, 5, wide)
            ex = R.exact_sims(inp["e"], inp["qhat"], C, wide)
            E3 = R.bounds_sims(ex)["prods"].view(rows, C, 3)
            need = (E3.gather(2, ex["argmax"][..., None]) + E3.gather(2, ex["second"][..., None]))[..., 0]
            zero = (ex["dots_abs"].view(rows, C, 3) == 0).all(-1)
            excused += int(((ex["margin"] <= need) & ~zero).sum())
            pairs += rows * C
    print(f"HEADSREF-CPU argmax excused share over the GPU cases, {profile}: {excused}/{pairs} = {excused / pairs:.5f}")
    assert pairs > 10000 and excused <= 0.01 * pairs
