"""The detection heads (heads.hip, class_head_wide.hip, the class-head / query / box-head backwards of backward.hip) against the float64 references and
derived bounds of tests/heads_reference.py, at the smallest shapes that reach each form of the launchers (tests/test_heads_reference.py shows that the
shape lists reach them): partial waves and a ragged last workgroup of the forward, every rows-per-wave and every exit of the backward's 4-row rotation,
the generic kernel's odd-row tail, every NT instantiation and the two-chunk G of the wide backward, rpb 8 / 9 / 64 with ragged blocks and both slab
reduces of the box-head backward; inputs with trained-like norms and near-tied prompts, exact ties, tiny and all-zero rows, aligned upstream, and a
saturated box head.

Per case: every output buffer starts at a sentinel and carries extra rows, every input row past `rows` is poisoned -- once with +-1e30, once with NaN --
and the test asserts the pads untouched, every element inside its bound, the bit tests (G, e_bf16, zero rows of qhat), and that the second run (under
the other poison) gives the same bits.  The HEADSREF lines this test prints are the source of profiles/heads_reference.md."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import _lib, ops  # noqa: E402
from tests import heads_reference as R  # noqa: E402

DEV = "cuda"
SENT = 7.0
PAD = 3
SEED = 5
POISONS = ("finite", "nan")


def _in(t, poison, dtype=None):
    t = R.poison_rows(t, PAD, poison)
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def _out(rows, width, dtype=torch.float32, fill=SENT):
    shape = (rows + PAD,) if width is None else (rows + PAD, width)
    return torch.full(shape, fill, dtype=dtype, device=DEV)


def _pads(name, buf, rows, fails, fill=SENT):
    """rows past `rows` of an output that started at `fill` hold their bits."""
    b = buf.reshape(buf.shape[0], -1).float()
    R.untouched(name, b, torch.full_like(b, fill), rows, 0, b.shape[1], fails)


def _same(name, a, b, fails):
    a, b = a.float(), b.float()
    if not torch.equal(R.bits(a), R.bits(b)):
        fails.append(f"{name}: bits differ in {int((R.bits(a) != R.bits(b)).sum())} elements")


def _report(kernel, tensor, profile, tag, worst):
    print(f"HEADSREF {kernel:10s} {tensor:7s} {profile:9s} {tag} worst err/tol {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# class head, forward and backward, narrow and wide
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _run_sims(inp, C, wide, poison, fails, tag):
    rows, Dt = inp["e"].shape
    e, qhat = _in(inp["e"], poison), inp["qhat"].to(DEV)
    sims, am, inv = _out(rows, C), _out(rows, C, torch.uint8, 7), _out(rows, None)
    (ops.class_sims_wide if wide else ops.class_sims)(e, qhat, sims, am, inv, rows, Dt, C)
    torch.cuda.synchronize()
    for n, t in (("sims", sims), ("argmax", am), ("inv", inv)):
        _pads(f"{tag} {n} pad rows ({poison})", t, rows, fails)
    return sims[:rows], am[:rows], inv[:rows]


def _run_sims_bwd(inp, ds, given, C, wide, poison, fails, tag):
    rows, Dt = inp["e"].shape
    sims, am, inv = given
    args = [_in(ds, poison), _in(sims.cpu(), poison), _in(am.cpu(), poison), _in(inv.cpu(), poison), _in(inp["e"], poison), inp["qhat"].to(DEV)]
    W = R.wide_qp(C) if wide else 32
    de, G, eb = _out(rows, Dt, torch.bfloat16), _out(rows, W, torch.bfloat16), _out(rows, Dt, torch.bfloat16)
    (ops.class_sims_wide_bwd if wide else ops.class_sims_bwd)(*args, de, G, eb, rows, Dt, C)
    torch.cuda.synchronize()
    for n, t in (("de", de), ("G", G), ("e_bf16", eb)):
        _pads(f"{tag} {n} pad rows ({poison})", t, rows, fails)
    return de[:rows], G[:rows], eb[:rows]


def _class_case(rows, Dt, C, profile, wide, backward=True):
    kern = ("wide" if wide else "narrow")
    tag = f"rows={rows} Dt={Dt} C={C}"
    inp = R.make_inputs(profile, rows, Dt, C, SEED, wide)
    fails = []
    e_d, q_d = inp["e"].to(DEV), inp["qhat"].to(DEV)
    ex = R.exact_sims(e_d, q_d, C, wide)
    tol = R.bounds_sims(ex)
    if Dt % 64 == 0:
        runs = [_run_sims(inp, C, wide, p, fails, tag) for p in POISONS]
        sims, am, inv = runs[0]
        for n, x, y in zip(("sims", "argmax", "inv"), runs[0], runs[1]):
            _same(f"{tag} {n} second run", x, y, fails)
        _report(kern + "_fwd", "sims", profile, tag, R.check(f"{tag} sims", sims, ex["sims"], tol["sims"], fails))
        _report(kern + "_fwd", "inv", profile, tag, R.check(f"{tag} inv", inv, ex["inv"], tol["inv"], fails))
        share = R.check_argmax(f"{tag} argmax", am, ex, tol["prods"], fails, inp["tie_kind"] if profile == "ties" else None)
        print(f"HEADSREF {kern}_fwd argmax  {profile:9s} {tag} excused share {share:.4f}")
    else:           # a width only the backward takes (Dt % 32 == 0): it is given the f32 nearest to the reference's forward
        sims, am, inv = ex["sims"].float(), ex["argmax"].to(torch.uint8), ex["inv"].float()
    if backward:
        ds = R.make_dsims(profile, sims.cpu(), SEED)
        xb = R.exact_sims_bwd(ds.to(DEV), e_d, q_d, sims, am, inv, wide)
        tb = R.bounds_sims_bwd(xb, Dt)
        bruns = [_run_sims_bwd(inp, ds, (sims, am, inv), C, wide, p, fails, tag) for p in POISONS]
        de, G, eb = bruns[0]
        for n, a, b in zip(("de", "G", "e_bf16"), bruns[0], bruns[1]):
            _same(f"{tag} {n} second run", a, b, fails)
        _report(kern + "_bwd", "de", profile, tag, R.check(f"{tag} de", de.float(), xb["de"], tb["de"], fails))
        _same(f"{tag} G == bf16(fl32(dsims inv)) at the routed column, +0 elsewhere", G, xb["G"], fails)
        _same(f"{tag} e_bf16 == bf16(e)", eb, xb["e_bf16"], fails)
        zero = (e_d == 0).all(1)
        if bool(zero.any()) and not bool(torch.isfinite(de[zero].float()).all()):
            fails.append(f"{tag}: de of an all-zero row of e is not finite")
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("rows,Dt,C,profile", R.sims_fwd_cases(), ids=lambda v: str(v))
def test_class_sims_forward(rows, Dt, C, profile):
    _class_case(rows, Dt, C, profile, False, backward=False)


@pytest.mark.parametrize("rows,Dt,C,profile", R.sims_bwd_cases(), ids=lambda v: str(v))
def test_class_sims_backward(rows, Dt, C, profile):
    _class_case(rows, Dt, C, profile, False)


@pytest.mark.parametrize("rows,Dt,C,profile", R.wide_cases(), ids=lambda v: str(v))
def test_wide_class_head(rows, Dt, C, profile):
    _class_case(rows, Dt, C, profile, True, backward=True)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# query_normalize and its backward
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _qhat_case(nq, Dt, wide):
    C = nq // 3 if wide else None
    tag = f"nq={nq} Dt={Dt} {'wide' if wide else 'narrow'}"
    g = torch.Generator().manual_seed(nq * 131 + Dt)
    Q = torch.randn(nq, Dt, generator=g) * (2.0 ** torch.randint(-6, 7, (nq, 1), generator=g).float())
    trows = R.table_rows(C, True) if wide else 32
    live = (32 * (torch.arange(nq) // 30) + torch.arange(nq) % 30) if wide else torch.arange(nq)
    dead = torch.ones(trows, dtype=torch.bool); dead[live] = False
    ex = R.exact_qhat(Q.to(DEV))
    tol = R.bounds_qhat(ex)
    fails, runs = [], []
    for poison in POISONS:
        qhat, qn = _out(trows, Dt), _out(trows, None)
        (ops.query_normalize_wide if wide else ops.query_normalize)(_in(Q, poison), qhat, qn, nq, Dt)
        torch.cuda.synchronize()
        _pads(f"{tag} qhat pad rows", qhat, trows, fails)
        _pads(f"{tag} qnorm pad rows", qn, trows, fails)
        runs.append((qhat[:trows], qn[:trows]))
    qhat, qn = runs[0]
    _same(f"{tag} qhat second run", qhat, runs[1][0], fails)
    _same(f"{tag} qnorm second run", qn, runs[1][1], fails)
    _report("qhat", "qhat", "scaled", tag, R.check(f"{tag} qhat", qhat[live], ex["qhat"], tol["qhat"], fails))
    _report("qhat", "qnorm", "scaled", tag, R.check(f"{tag} qnorm", qn[live], ex["n"], tol["qnorm"], fails))
    if bool(dead.any()) and not torch.equal(R.bits(qhat[dead]), torch.zeros_like(R.bits(qhat[dead]))):
        fails.append(f"{tag}: rows >= nq / rows 30, 31 / classes >= C of qhat are not exactly +0")
    if wide and not bool((qn[dead] == 0).all()):
        fails.append(f"{tag}: qnorm of a dead row is not 0")
    # backward: accumulate onto a non-zero old; the rows of dqhat the kernel must not read are poisoned
    dh = torch.randn(nq, Dt, generator=g)
    old = torch.randn(nq, Dt, generator=g) * 0.5
    xb = R.exact_qhat_bwd(dh.to(DEV), Q.to(DEV), old.to(DEV))
    tb = R.bounds_qhat_bwd(xb)
    bruns = []
    for poison in POISONS:
        dq_in = R.poison_rows(torch.zeros(0, Dt), trows + PAD, poison).to(DEV)
        dq_in[live] = dh.to(DEV)
        dq = _out(nq, Dt)
        dq[:nq] = old.to(DEV)
        (ops.query_normalize_wide_bwd if wide else _query_normalize_bwd)(dq_in, _in(Q, poison), dq, nq, Dt)
        torch.cuda.synchronize()
        _pads(f"{tag} dQ pad rows", dq, nq, fails)
        bruns.append(dq[:nq])
    _same(f"{tag} dQ second run", bruns[0], bruns[1], fails)
    _report("qhat_bwd", "dQ", "scaled", tag, R.check(f"{tag} dQ", bruns[0], xb["dq"], tb["dq"], fails))
    assert not fails, "\n".join(fails[:20])


def _query_normalize_bwd(dqhat, queries, dqueries, nq, Dt):
    _lib.call("owl_query_normalize_bwd", ops.stream(), dqhat, queries, dqueries, nq, Dt)


@pytest.mark.parametrize("Dt", [64, 192, 768])
@pytest.mark.parametrize("nq", R.QHAT_NQ)
def test_query_normalize(nq, Dt):
    _qhat_case(nq, Dt, False)


@pytest.mark.parametrize("C", R.WIDE_C)
def test_query_normalize_wide(C):
    _qhat_case(3 * C, 512, True)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# box head
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,D", R.BOX_FWD, ids=lambda v: str(v))
def test_box_final_forward_saturated(rows, D):
    """sig and boxes held to the derived RELATIVE bound on a saturated head (the forms test keeps 1e-6 absolute on randn at the model's shapes)."""
    tag = f"rows={rows} D={D}"
    inp = R.make_box_inputs("saturated", rows, D, SEED)
    ex = R.exact_box_final(inp["h1"].to(DEV), inp["w2"].to(DEV), inp["b2"].to(DEV), inp["box_bias"].to(DEV), inp["P"])
    tol = R.bounds_box_final(ex)
    fails, runs = [], []
    for poison in POISONS:
        boxes, sig = _out(rows, 4), _out(rows, 4)
        ops.box_final(_in(inp["h1"], poison, torch.bfloat16), inp["w2"].to(DEV), inp["b2"].to(DEV), inp["box_bias"].to(DEV), boxes, sig, rows, inp["P"], D)
        torch.cuda.synchronize()
        _pads(f"{tag} boxes pad rows", boxes, rows, fails)
        _pads(f"{tag} sig pad rows", sig, rows, fails)
        runs.append((boxes[:rows], sig[:rows]))
    _same(f"{tag} boxes second run", runs[0][0], runs[1][0], fails)
    _same(f"{tag} sig second run", runs[0][1], runs[1][1], fails)
    _report("box_fwd", "sig", "saturated", tag, R.check(f"{tag} sig", runs[0][1], ex["sig"], tol["sig"], fails))
    _report("box_fwd", "boxes", "saturated", tag, R.check(f"{tag} boxes", runs[0][0], ex["boxes"], tol["boxes"], fails))
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("profile", R.BOX_PROFILES)
@pytest.mark.parametrize("rows,D", R.BOX_BWD, ids=lambda v: str(v))
def test_box_final_backward(rows, D, profile):
    tag = f"rows={rows} D={D}"
    inp = R.make_box_inputs(profile, rows, D, SEED)
    old = R.box_old(D)
    old_d = {k: v.to(DEV) for k, v in old.items()}
    ex = R.exact_box_final_bwd(inp["dboxes"].to(DEV), inp["sig"].to(DEV), inp["h1"].to(DEV), inp["u1"].to(DEV), inp["w2"].to(DEV), old_d)
    tol = R.bounds_box_final_bwd(ex, old_d)
    nblk = _lib.load().owl_box_final_bwd_blocks(rows)
    assert nblk == R.box_bwd_blocks(rows)
    fails, runs = [], []
    for poison, with_cs in (("finite", True), ("nan", True), ("nan", False)):
        du1 = _out(rows, D, torch.bfloat16)
        part = torch.full((nblk, 5 * D + 4), float("nan"), device=DEV)          # the scratch need not be initialised: NaN, so a word read before it is written shows
        g = torch.cat([old["dW2"].reshape(-1), old["db2"]]).to(DEV)
        cs = old["colsum"].to(DEV).clone() if with_cs else None
        ops.box_final_bwd(_in(inp["dboxes"], poison), _in(inp["sig"], poison), _in(inp["h1"], poison, torch.bfloat16), _in(inp["u1"], poison, torch.bfloat16),
                          inp["w2"].to(DEV), du1, part, g, rows, D, du1_colsum=cs)
        torch.cuda.synchronize()
        _pads(f"{tag} du1 pad rows ({poison})", du1, rows, fails)
        runs.append({"du1": du1[:rows].float(), "dW2": g[:4 * D].view(4, D), "db2": g[4 * D:], "colsum": cs})
    for k in ("du1", "dW2", "db2", "colsum"):
        _report("box_bwd", k, profile, tag, R.check(f"{tag} {k}", runs[0][k], ex[k], tol[k], fails))
        _same(f"{tag} {k} second run", runs[0][k], runs[1][k], fails)
        if k != "colsum":
            _same(f"{tag} {k} without du1_colsum", runs[0][k], runs[2][k], fails)
    assert not fails, "\n".join(fails[:20])
