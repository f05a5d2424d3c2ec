"""The LayerNorm family (norm.hip: ln_fwd_kernel in every form, cls_ln_kernel + merge_ln_kernel, cls_rows_kernel; backward.hip: ln_bwd_body in every
form, ln_bwd_kernel_768, merge_ln_bwd_kernel + cls_ln_bwd_kernel, partials_reduce_kernel) against the float64 references and derived bounds of tests/layernorm_reference.py, at the smallest
shapes at which each mechanism exists: widths that leave lanes without a vector, with one vector in a second round (260), with a ragged last round
(252, 1020), the 768 / 1024 instantiations; row counts with a ragged last workgroup and a ragged last 64-row block, and 18 / 33 blocks for the strided
loop of the partial-sum reduce; inputs with outlier channels, a large mean, a spread far below eps, exactly-zero rows and rows scaled by 2^+-40.

What is pinned, per case: every element of every output and statistic inside its elementwise bound; x_out bit for bit the f32 sum formed on the CPU;
every pad row and sentinel region bit for bit what it was (inputs' pad rows hold NaN); a second call gives the same bits; the first row, the last and one of
another wave, each computed alone (rows = 1; B = P = 1 for the merge), have the bits they have inside the batch (outputs, statistics and dx); dx_bf16 == bf16(dx); the parameter-only backward gives the full
form's dgamma / dbeta bits.  tests/test_layernorm_reference.py shows on the CPU that these bounds hold for a correct f32 kernel and reject each planted
error.  The LNREF-GPU lines this test prints are the source of profiles/layernorm_reference.md."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import ops  # noqa: E402
from tests import layernorm_reference as R  # noqa: E402

DEV = "cuda"
SENTINEL = 7.0
PAD = 3
NAN = float("nan")
SEED = 3


def _up(t, fill, dtype=None):
    """valid rows on the device followed by PAD rows of `fill`."""
    return R.padded(t if dtype is None else t.to(dtype), PAD, fill).to(DEV).contiguous()


def _sent(rows, width, dtype):
    return torch.full((rows + PAD, width), SENTINEL, dtype=dtype, device=DEV)


def _same(name, a, b, fails):
    if not torch.equal(R.bits(a), R.bits(b)):
        fails.append(f"{name}: bits differ in {int((R.bits(a) != R.bits(b)).sum())} elements")


def _report(kernel, out, profile, tag, worst):
    print(f"LNREF-GPU {kernel:7s} {out:8s} {profile:8s} {tag} worst err/tol {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------------------
FORM_SPEC = {   # name: (deltas, out dtype, out aliases x, own x_out buffer, store_x, stats)
    "bf16": (0, torch.bfloat16, False, False, True, True),
    "f32": (0, torch.float32, False, False, True, True),
    "f32_inplace": (0, torch.float32, True, False, True, True),
    "delta": (1, torch.bfloat16, False, True, True, True),
    "delta_alias": (1, torch.bfloat16, False, False, True, True),
    "delta2": (2, torch.float32, False, True, True, True),
    "nostore": (2, torch.bfloat16, False, False, False, True),
    "nostats": (0, torch.bfloat16, False, False, True, False),
}
assert tuple(FORM_SPEC) == R.FWD_FORMS


def _run_fwd(form, inp, lo, hi, fails, tag):
    """one call of ops.layernorm on rows [lo, hi) of the case -> dict y, mean, rstd, s (CPU), after the untouched checks."""
    nd, odt, inplace, own_xout, store_x, with_stats = FORM_SPEC[form]
    rows, D = hi - lo, inp["x"].shape[1]
    x = _up(inp["x"][lo:hi], NAN)
    x0 = x.clone()
    delta = _up(inp["delta"][lo:hi], NAN, torch.bfloat16) if nd >= 1 else None
    delta2 = _up(inp["delta2"][lo:hi], NAN, torch.bfloat16) if nd >= 2 else None
    gamma, beta = inp["gamma"].to(DEV), inp["beta"].to(DEV)
    out = x if inplace else _sent(rows, D, odt)
    out0 = out.clone()
    stats = _sent(rows, 2, torch.float32) if with_stats else None
    stats0 = stats.clone() if with_stats else None
    x_out = _sent(rows, D, torch.float32) if own_xout else None
    xo0 = x_out.clone() if own_xout else None
    ops.layernorm(x, gamma, beta, out, rows, D, stats, R.EPS, delta=delta, x_out=x_out, delta2=delta2, store_x=store_x)
    torch.cuda.synchronize()
    R.untouched(f"{tag} out", out, out0, rows, 0, D, fails)
    if with_stats:
        R.untouched(f"{tag} stats", stats, stats0, rows, 0, 2, fails)
    res = {"y": out[:rows].float().cpu(), "s": None}
    if with_stats:
        res["mean"], res["rstd"] = stats[:rows, 0].cpu(), stats[:rows, 1].cpu()
    if own_xout:
        R.untouched(f"{tag} x_out", x_out, xo0, rows, 0, D, fails)
        res["s"] = x_out[:rows].cpu()
    if form == "delta_alias":
        R.untouched(f"{tag} x (aliased x_out)", x, x0, rows, 0, D, fails)
        res["s"] = x[:rows].cpu()
    elif not inplace:
        _same(f"{tag} x must not change", x, x0, fails)
    return res


@pytest.mark.parametrize("D,profile,rows", R.fwd_cases(), ids=lambda v: str(v))
def test_layernorm_forward(D, profile, rows):
    inp = R.make_inputs(profile, rows, D, SEED)
    deltas = {0: (None, None), 1: (inp["delta"], None), 2: (inp["delta"], inp["delta2"])}
    ex = {k: R.exact_fwd(inp["x"], inp["gamma"], inp["beta"], R.EPS, *d) for k, d in deltas.items()}
    tol = {k: R.bounds_fwd(e) for k, e in ex.items()}
    fails, got = [], {}
    zero = (inp["x"] == 0).all(1)
    for form in R.FWD_FORMS:
        nd, odt = FORM_SPEC[form][:2]
        tag = f"D={D} rows={rows} {form}"
        g = got[form] = _run_fwd(form, inp, 0, rows, fails, tag)
        e, t = ex[nd], tol[nd]
        kind = "bf16" if odt == torch.bfloat16 else "f32"
        _report("ln_fwd", kind, profile, tag, R.check(f"{tag} y", g["y"], e["y"], t[kind], fails))
        if "mean" in g:
            _report("ln_fwd", "mean", profile, tag, R.check(f"{tag} mean", g["mean"], e["mean"], t["mean"], fails))
            _report("ln_fwd", "rstd", profile, tag, R.check(f"{tag} rstd", g["rstd"], e["rstd"], t["rstd"], fails))
        if g["s"] is not None:
            _same(f"{tag} x_out vs fl(fl(x + d) + d2)", g["s"], e["s"], fails)
        if nd == 0 and bool(zero.any()):                       # exactly-zero rows: out = store(beta), mean = 0
            want = (R.bf16_round(inp["beta"]) if kind == "bf16" else inp["beta"]).expand(int(zero.sum()), D)
            _same(f"{tag} zero rows give store(beta)", g["y"][zero], want, fails)
            if "mean" in g and not bool((g["mean"][zero] == 0).all()):
                fails.append(f"{tag}: mean of a zero row is not 0")
        # a second call gives the same bits; the last row alone has the bits it has inside the batch
        g2 = _run_fwd(form, inp, 0, rows, fails, tag + " (second call)")
        for k in ("y", "mean", "rstd", "s"):
            if g.get(k) is not None:
                _same(f"{tag} {k} second call", g2[k], g[k], fails)
        for r in sorted({rows - 1, 0, min(5, rows - 1)}):       # the last row, the first, and one of another wave of the workgroup
            alone = _run_fwd(form, inp, r, r + 1, fails, tag + f" (row {r} alone)")
            for k in ("y", "mean", "rstd", "s"):
                if g.get(k) is not None:
                    _same(f"{tag} {k} row {r} alone", alone[k], g[k][r:r + 1], fails)
    _same(f"D={D} rows={rows} stats=None changes the output", got["nostats"]["y"], got["bf16"]["y"], fails)
    assert not fails, "\n".join(fails[:20])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _old(D):
    return {"dgamma": torch.linspace(-0.5, 0.75, D), "dbeta": torch.linspace(1.0, -0.25, D), "colsum": torch.full((D,), 2.0)}


def _run_bwd(form, dy_c, b16, inp, mean, rstd, dres_c, lo, hi, fails, tag):
    rows, D = hi - lo, inp["x"].shape[1]
    x = _up(inp["x"][lo:hi], NAN)
    dy = _up(dy_c[lo:hi], NAN, torch.bfloat16 if b16 else torch.float32)
    stats = _up(torch.stack([mean, rstd], -1)[lo:hi], NAN)
    gamma = inp["gamma"].to(DEV)
    with_dx = form != "param"
    with_res = form in ("full", "colsum")
    with_par = form != "dx_only"
    dres = _up(dres_c[lo:hi], NAN) if with_res else None
    dx = _sent(rows, D, torch.float32) if with_dx else None
    dxb = _sent(rows, D, torch.bfloat16) if with_res else None
    old = _old(D)
    dg, db = (old["dgamma"].to(DEV), old["dbeta"].to(DEV)) if with_par else (None, None)
    cs = old["colsum"].to(DEV) if form == "colsum" else None
    keep = [(n, t, t.clone()) for n, t in (("dx", dx), ("dx_bf16", dxb)) if t is not None]
    ins = [(n, t, t.clone()) for n, t in (("x", x), ("dy", dy), ("stats", stats), ("dres", dres)) if t is not None]
    ops.layernorm_bwd(dy, x, stats, gamma, dres, dx, dg, db, rows, D, dx_bf16=dxb, dx_colsum=cs)
    torch.cuda.synchronize()
    for n, t, t0 in keep:
        R.untouched(f"{tag} {n}", t, t0, rows, 0, D, fails)
    for n, t, t0 in ins:
        _same(f"{tag} input {n} must not change", t, t0, fails)
    res = {"dx": dx[:rows].cpu() if with_dx else None, "dx_bf16": dxb[:rows].float().cpu() if dxb is not None else None,
           "dgamma": dg.cpu() if with_par else None, "dbeta": db.cpu() if with_par else None, "colsum": cs.cpu() if cs is not None else None}
    if dxb is not None:
        _same(f"{tag} dx_bf16 == bf16(dx)", dxb[:rows], dx[:rows].bfloat16(), fails)
    return res


@pytest.mark.parametrize("D,profile,rows", R.bwd_cases(), ids=lambda v: str(v))
def test_layernorm_backward(D, profile, rows):
    inp = R.make_inputs(profile, rows, D, SEED)
    # the statistics the backward is given: the forward kernel's own
    st = torch.zeros(rows, 2, device=DEV)
    ops.layernorm(inp["x"].to(DEV), inp["gamma"].to(DEV), inp["beta"].to(DEV), torch.empty(rows, D, device=DEV, dtype=torch.bfloat16), rows, D, st)
    mean, rstd = st[:, 0].cpu(), st[:, 1].cpu()
    dres = 0.05 * torch.randn(rows, D, generator=torch.Generator().manual_seed(rows + D)) * R.row_scale(profile, rows)
    old = _old(D)
    fails = []
    dys = [("white", True), ("aligned", False)] if rows > 1000 else [(k, b) for k in R.DY_KINDS for b in (True, False)]
    for kind, b16 in dys:
        dy = R.make_dy(kind, inp["x"], mean, rstd, inp["gamma"], SEED, b16)
        ex = {True: R.exact_bwd(dy, inp["x"], mean, rstd, inp["gamma"], dres), False: R.exact_bwd(dy, inp["x"], mean, rstd, inp["gamma"], None)}
        tol = {k: R.bounds_bwd(e, old=old) for k, e in ex.items()}
        got = {}
        for form in ("param", "full", "dx_only") + (("colsum",) if b16 else ()):
            tag = f"D={D} rows={rows} dy={kind}/{'bf16' if b16 else 'f32'} {form}"
            g = got[form] = _run_bwd(form, dy, b16, inp, mean, rstd, dres, 0, rows, fails, tag)
            e, t = ex[form != "dx_only"], tol[form != "dx_only"]
            for k in ("dx", "dx_bf16"):
                if g[k] is not None:
                    _report("ln_bwd", k, profile, tag, R.check(f"{tag} {k}", g[k], e["dx"], t[k], fails))
            for k in ("dgamma", "dbeta", "colsum"):
                if g[k] is not None:
                    _report("ln_bwd", k, profile, tag, R.check(f"{tag} {k}", g[k], e[k] + old[k].double(), t[k], fails))
            g2 = _run_bwd(form, dy, b16, inp, mean, rstd, dres, 0, rows, fails, tag + " (second call)")
            for k, v in g.items():
                if v is not None:
                    _same(f"{tag} {k} second call", g2[k], v, fails)
            if g["dx"] is not None:
                for r in sorted({rows - 1, 0, min(65, rows - 1)}):       # the last row, the first, and one of another wave (and block) than either
                    alone = _run_bwd(form, dy, b16, inp, mean, rstd, dres, r, r + 1, fails, tag + f" (row {r} alone)")
                    _same(f"{tag} dx row {r} alone", alone["dx"], g["dx"][r:r + 1], fails)
        for k in ("dgamma", "dbeta"):
            _same(f"D={D} rows={rows} dy={kind} parameter-only vs full {k}", got["param"][k], got["full"][k], fails)
            if b16:
                _same(f"D={D} rows={rows} dy={kind} column-sum form vs full {k}", got["colsum"][k], got["full"][k], fails)
    assert not fails, "\n".join(fails[:20])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# merge forward, cls_rows
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _run_merge(x_c, delta_c, aff, B, P, Tp, D, fails, tag):
    T = P + 1
    x = torch.full((B * Tp + PAD, D), NAN, device=DEV)
    xv = x[:B * Tp].view(B, Tp, D)
    xv[:, :T] = x_c.to(DEV)
    x0 = x.clone()
    delta = None
    if delta_c is not None:
        delta = torch.full((B * Tp + PAD, D), NAN, device=DEV, dtype=torch.bfloat16)
        delta[:B * Tp].view(B, Tp, D)[:, :T] = delta_c.to(DEV).bfloat16()
    cls_ln = _sent(B, D, torch.float32); feats = _sent(B * P, D, torch.bfloat16)
    st1 = _sent(B * Tp, 2, torch.float32); st2 = _sent(B * P, 2, torch.float32)
    c0, f0, s10, s20 = cls_ln.clone(), feats.clone(), st1.clone(), st2.clone()
    g1, b1, g2, b2 = (t.to(DEV) for t in aff)
    ops.merge_ln(x, g1, b1, g2, b2, cls_ln, feats, st1, st2, B, P, Tp, D, R.EPS, delta=delta)
    torch.cuda.synchronize()
    R.untouched(f"{tag} cls_ln", cls_ln, c0, B, 0, D, fails)
    R.untouched(f"{tag} feats", feats, f0, B * P, 0, D, fails)
    R.untouched(f"{tag} stats2", st2, s20, B * P, 0, 2, fails)
    valid = torch.zeros(B * Tp + PAD, dtype=torch.bool, device=DEV)
    valid[:B * Tp].view(B, Tp)[:, :T] = True
    _same(f"{tag} stats1 outside the valid tokens", st1[~valid], s10[~valid], fails)
    _same(f"{tag} x outside the valid tokens", x[~valid], x0[~valid], fails)
    if delta is None:
        _same(f"{tag} x must not change", x, x0, fails)
    return {"cls_ln": cls_ln[:B].cpu(), "feats": feats[:B * P].float().cpu().view(B, P, D), "stats1": st1[:B * Tp].view(B, Tp, 2)[:, :T].cpu(),
            "stats2": st2[:B * P].view(B, P, 2).cpu(), "s": xv[:, :T].cpu()}


@pytest.mark.parametrize("D,profile,B,P", R.merge_cases(), ids=lambda v: str(v))
def test_merge_ln_forward(D, profile, B, P):
    Tp = R.roundup(P + 1, 8)
    Tp = Tp + 8 if Tp == P + 1 else Tp
    inp = R.make_inputs(profile, B * (P + 1), D, SEED)
    i2 = R.make_inputs(profile, 1, D, SEED + 1)
    aff = (inp["gamma"], inp["beta"], i2["gamma"], i2["beta"])
    x = inp["x"].reshape(B, P + 1, D)
    fails = []
    for delta in (None, inp["delta"].reshape(B, P + 1, D)):
        tag = f"D={D} B={B} P={P} delta={delta is not None}"
        ex = R.exact_merge(x, *aff, R.EPS, delta)
        tol = R.bounds_merge(ex)
        g = _run_merge(x, delta, aff, B, P, Tp, D, fails, tag)
        for k in ("cls_ln", "feats", "stats1", "stats2"):
            _report("merge", k, profile, tag, R.check(f"{tag} {k}", g[k], ex[k], tol[k], fails))
        _same(f"{tag} x_out vs fl(x + d)", g["s"], ex["s"], fails)
        g2 = _run_merge(x, delta, aff, B, P, Tp, D, fails, tag + " (second call)")
        for k, v in g.items():
            _same(f"{tag} {k} second call", g2[k], v, fails)
        for b, p in sorted({(B - 1, P - 1), (0, 0)}):            # image b's class token with patch row p alone (B = 1, P = 1)
            pick = lambda t: None if t is None else torch.stack([t[b, 0], t[b, 1 + p]])[None]
            a = _run_merge(pick(x), pick(delta), aff, 1, 1, 8, D, fails, tag + f" (image {b} patch {p} alone)")
            _same(f"{tag} cls_ln image {b} alone", a["cls_ln"], g["cls_ln"][b:b + 1], fails)
            _same(f"{tag} feats [{b}, {p}] alone", a["feats"][0], g["feats"][b, p:p + 1], fails)
            _same(f"{tag} stats2 [{b}, {p}] alone", a["stats2"][0], g["stats2"][b, p:p + 1], fails)
            _same(f"{tag} stats1 [{b}, {p}] alone", a["stats1"][0], g["stats1"][b, [0, 1 + p]], fails)
    assert not fails, "\n".join(fails[:20])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# merge backward
# ---------------------------------------------------------------------------------------------------------------------------------------------
MB_OLD = {"dg1": (-0.5, 0.75), "db1": (1.0, -0.25), "dg2": (-1.5, -1.5), "db2": (0.25, 2.0), "colsum": (2.0, 2.0)}


def _run_merge_bwd(df_c, x_c, given, aff, B, P, Tp, D, fails, tag):
    """one call of ops.merge_ln_bwd with dx_bf16 and dx_colsum on nonzero accumulators; pad tokens hold NaN on inputs and the sentinel on outputs."""
    T = P + 1
    g1, b1, g2 = (t.to(DEV) for t in aff)

    def tokens(valid, fill, dtype=torch.float32):        # [B * Tp + PAD, W] with `valid` [B, T, W] in the valid tokens
        t = torch.full((B * Tp + PAD, valid.shape[-1]), fill, device=DEV, dtype=dtype)
        t[:B * Tp].view(B, Tp, -1)[:, :T] = valid.to(DEV)
        return t

    x, st1 = tokens(x_c, NAN), tokens(given["stats1"], NAN)
    st2 = _up(given["stats2"].reshape(B * P, 2), NAN)
    df = _up(df_c.reshape(B * P, D), NAN)
    cls_ln = _up(given["cls_ln"], NAN)
    dx, dxb = _sent(B * Tp, D, torch.float32), _sent(B * Tp, D, torch.bfloat16)
    dcls = _sent(B, D, torch.float32)
    acc = {k: torch.linspace(lo, hi, D).to(DEV) for k, (lo, hi) in MB_OLD.items()}
    keep = [(n, t, t.clone()) for n, t in (("dx", dx), ("dx_bf16", dxb), ("dcls", dcls))]
    ins = [(n, t, t.clone()) for n, t in (("x", x), ("dfeats", df), ("stats1", st1), ("stats2", st2), ("cls_ln", cls_ln))]
    ops.merge_ln_bwd(df, x, cls_ln, st1, st2, g1, b1, g2, dx, dcls, acc["dg1"], acc["db1"], acc["dg2"], acc["db2"], B, P, Tp, D,
                     dx_bf16=dxb, dx_colsum=acc["colsum"])
    torch.cuda.synchronize()
    valid = torch.zeros(B * Tp + PAD, dtype=torch.bool, device=DEV)
    valid[:B * Tp].view(B, Tp)[:, :T] = True
    for n, t, t0 in keep[:2]:
        _same(f"{tag} {n} outside the valid tokens", t[~valid], t0[~valid], fails)
    R.untouched(f"{tag} dcls", dcls, keep[2][2], B, 0, D, fails)
    for n, t, t0 in ins:
        _same(f"{tag} input {n} must not change", t, t0, fails)
    _same(f"{tag} dx_bf16 == bf16(dx)", dxb[valid], dx[valid].bfloat16(), fails)
    res = {k: v.cpu() for k, v in acc.items()}
    res.update(dx=dx[:B * Tp].view(B, Tp, D)[:, :T].cpu(), dx_bf16=dxb[:B * Tp].view(B, Tp, D)[:, :T].float().cpu(), dcls=dcls[:B].cpu())
    return res


@pytest.mark.parametrize("D,profile,B,P", R.merge_cases(), ids=lambda v: str(v))
def test_merge_ln_backward(D, profile, B, P):
    Tp = R.roundup(P + 1, 8)
    Tp = Tp + 8 if Tp == P + 1 else Tp
    inp = R.make_inputs(profile, B * (P + 1), D, SEED)
    i2 = R.make_inputs(profile, 1, D, SEED + 1)
    aff = (inp["gamma"], inp["beta"], i2["gamma"])
    x = inp["x"].reshape(B, P + 1, D)
    fails = []
    # what the backward is given: the forward kernels' own statistics and class row
    fw = _run_merge(x, None, aff + (i2["beta"],), B, P, Tp, D, fails, f"D={D} B={B} P={P} forward")
    given = {k: fw[k] for k in ("stats1", "stats2", "cls_ln")}
    old = {k: torch.linspace(lo, hi, D) for k, (lo, hi) in MB_OLD.items()}
    for kind in R.DFEATS_KINDS:
        tag = f"D={D} B={B} P={P} dfeats={kind}"
        df = R.make_dfeats(kind, x, given, *aff, SEED)
        ex = R.exact_merge_bwd(df, x, *aff, R.EPS, given)
        tol = R.bounds_merge_bwd(ex, old)
        g = _run_merge_bwd(df, x, given, aff, B, P, Tp, D, fails, tag)
        for k in ("dx", "dx_bf16", "dcls", "dg1", "db1", "dg2", "db2", "colsum"):
            ref = ex["dx"] if k == "dx_bf16" else ex[k] + (old[k].double() if k in old else 0.0)
            _report("mrg_bwd", k, profile, tag, R.check(f"{tag} {k}", g[k], ref, tol[k], fails))
        g2 = _run_merge_bwd(df, x, given, aff, B, P, Tp, D, fails, tag + " (second call)")
        for k, v in g.items():
            _same(f"{tag} {k} second call", g2[k], v, fails)
        for b, p in sorted({(B - 1, P - 1), (0, 0)}):            # patch row p of image b alone: its dx is a function of that row and cls_ln[b]
            pk = lambda t: torch.stack([t[b, 0], t[b, 1 + p]])[None]
            one = {"stats1": pk(given["stats1"]), "stats2": given["stats2"][b:b + 1, p:p + 1], "cls_ln": given["cls_ln"][b:b + 1]}
            a = _run_merge_bwd(df[b:b + 1, p:p + 1], pk(x), one, aff, 1, 1, 8, D, fails, tag + f" (image {b} patch {p} alone)")
            _same(f"{tag} dx [{b}, {p}] alone", a["dx"][0, 1:], g["dx"][b, 1 + p:2 + p], fails)
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("D", [4, 260, 1024])
def test_cls_rows_exact_bits(D):
    B, Tp = 3, 8
    g = torch.Generator().manual_seed(D)
    cls, pos = torch.randn(D, generator=g), torch.randn(D, generator=g) * 100.0
    x = torch.full((B * Tp + PAD, D), NAN, device=DEV)
    x0 = x.clone()
    ops.cls_rows(x, cls.to(DEV), pos.to(DEV), B, Tp, D)
    torch.cuda.synchronize()
    rows = torch.zeros(B * Tp + PAD, dtype=torch.bool, device=DEV)
    rows[torch.arange(B) * Tp] = True
    assert torch.equal(R.bits(x[rows].cpu()), R.bits((cls + pos).expand(B, D)))
    assert torch.equal(R.bits(x[~rows]), R.bits(x0[~rows]))
