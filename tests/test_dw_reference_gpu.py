"""-m gpu: the weight-gradient path -- ops.gemm_tn_slab (gemm_tn_pp_kernel with its bias fold, gemm_tn_slab_kernel), owl_slab_reduce,
autograd.weight_grad, ops.colsum_bf16 / colsum_f32 / transpose_colsum -- against the float64 references and derived bounds of tests/dw_reference.py, at
the smallest shapes at which a work item runs several K-tiles (the ping-pong stream: second prologue request, K-tile c + 2 requested into the buffer
being computed from, the counted wait, the buffer alternation, the whole-tile fast path followed by the zero-row path in one item) and at which the
single-phase kernel walks several items per workgroup.

What is pinned, per case: EVERY slab and EVERY bias partial against its own per-split reference (a K-tile counted in the wrong split cancels in the sum),
then the reduce with accumulate 0 (onto NaN) and 1 (onto values of the gradient's own size); `int_tagged` bit for bit (every f32 add exact: any order
gives the reference), `randn` / `cancel` / `one_hot_token` inside the derived bounds; pad rows [rows, pad_rows(rows)) of both operands and pad columns
[n, ld) poisoned, once with large finite integers (a leak breaks the exact profile) and once with NaN; slab[nsplit:], bias_slab[nsplit:] and everything
behind a reduce's n elements untouched; the operands unchanged; a second run the same bits; variant 1 (single-phase, no bias slab) the bits of variant 2.
Variants 0 and 2 are both the ping-pong kernel (gemm_tn.hip:416): both run on int_tagged and must agree; the float profiles run 0 and 1.
tests/test_dw_reference.py shows on the CPU that these checks hold for a correct f32 kernel and reject each of nine planted errors.  The DWREF lines
this test prints are the worst err / tol per output."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import _lib, autograd as A, ops  # noqa: E402
from tests import dw_reference as R  # noqa: E402

DEV = "cuda"
NAN = float("nan")
KEYS = ("slab", "bias", "w0", "w1", "b0", "b1")


def _same(a, b):
    return bool((R.bits(a) == R.bits(b)).all())


def _launch(dy, x, rows, n_out, n_in, splits, variant, with_bias, ns, tag, fails):
    """One ops.gemm_tn_slab call into NaN-filled buffers two slabs longer than needed -> (slab buffer, bias buffer | None), the tails checked."""
    slab = torch.full((ns + 2, n_out, n_in), NAN, device=DEV)
    bslab = torch.full((ns + 2, n_out), NAN, device=DEV) if with_bias else None
    dy0, x0 = dy.clone(), x.clone()
    used = ops.gemm_tn_slab(dy, x, slab, rows, n_out, n_in, splits, variant=variant, bias_slab=bslab)
    if used != ns:
        fails.append(f"{tag}: {used} splits used, the split rule says {ns}")
    R.untouched_rows(f"{tag} slab[nsplit:]", slab, torch.full_like(slab, NAN), ns, fails)
    if with_bias:
        R.untouched_rows(f"{tag} bias_slab[nsplit:]", bslab, torch.full_like(bslab, NAN), ns, fails)
    if not (_same(dy, dy0) and _same(x, x0)):
        fails.append(f"{tag}: an operand changed")
    return slab, bslab


def _reduce(parts, ns, old, accumulate, tag, fails):
    """owl_slab_reduce of parts[:ns] into a buffer of NaN (accumulate 0) or `old` (1) with 8 sentinel elements behind it."""
    shape = parts.shape[1:]
    n = parts[0].numel()
    tgt = torch.full((n + 8,), NAN, device=DEV)
    if accumulate:
        tgt[:n] = old.reshape(-1)
    _lib.call("owl_slab_reduce", ops.stream(), parts, tgt, n, n, ns, accumulate)
    if not bool(torch.isnan(tgt[n:]).all()):
        fails.append(f"{tag}: the reduce wrote past n")
    return tgt[:n].reshape(shape).clone()


def _run_profile(case, profile, poison, pos, variants, fails, lines):
    rows, splits, n_out, n_in, ldy, ldx = case
    dy_c, x_c = R.make_inputs(profile, rows, n_out, n_in, 1, ldy, ldx, poison, pos)
    dy_f, x_f = dy_c.to(DEV), x_c.to(DEV)
    ex = R.exact_tn(dy_f, x_f, rows, n_out, n_in, splits)
    old_w, old_b = R.make_old(profile, ex["w0"], 1).to(DEV), R.make_old(profile, ex["b0"], 2).to(DEV)
    R.set_old(ex, old_w, old_b)
    tol = R.bounds_tn(ex)
    ns = ex["ns"]
    exact = profile == "int_tagged"
    if exact:
        R.assert_exact_ok(ex, str(case))
    dy, x = dy_f.bfloat16(), x_f.bfloat16()
    tagp = f"{profile}{'' if pos is None else '@' + str(pos)} poison={'nan' if poison != poison else 'int'}"
    base = None
    for variant in variants:
        tag = f"{tagp} variant={variant}"
        with_bias = variant != 1
        slab, bslab = _launch(dy, x, rows, n_out, n_in, splits, variant, with_bias, ns, tag, fails)
        slab2, bslab2 = _launch(dy, x, rows, n_out, n_in, splits, variant, with_bias, ns, tag + " (second run)", fails)
        if not (_same(slab, slab2) and (not with_bias or _same(bslab, bslab2))):
            fails.append(f"{tag}: two runs give different bits")
        got = {"slab": slab[:ns]}
        if with_bias:
            got["bias"] = bslab[:ns]
            for accumulate in (0, 1):
                got[f"w{accumulate}"] = _reduce(slab, ns, old_w, accumulate, f"{tag} weight reduce", fails)
                got[f"b{accumulate}"] = _reduce(bslab, ns, old_b, accumulate, f"{tag} bias reduce", fails)
        worst = {}
        for k, v in got.items():
            if exact:
                R.check_exact(f"{tag} {k}", v, ex[k], fails)
            worst[k] = R.check(f"{tag} {k}", v, ex[k], tol[k], fails)
        if base is None:
            base = slab
        elif not _same(base[:ns], slab[:ns]):
            d = (base[:ns].double() - slab[:ns].double()).abs()
            fails.append(f"{tag}: slabs differ from variant {variants[0]}'s at {int((d > 0).sum())} elements, max |diff| {float(d.max()):.3g}")
        lines.append(f"DWREF tn rows={rows} splits={splits} n_out={n_out} n_in={n_in} ld=({ldy},{ldx}) per={ex['per']} ns={ns} {tag} "
                     + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


def _run_case(case, big=False):
    rows, splits = case[:2]
    fails, lines = [], []
    _run_profile(case, "int_tagged", R.POISON_INT, None, (0, 2, 1), fails, lines)
    _run_profile(case, "int_tagged", NAN, None, (0, 1), fails, lines)
    _run_profile(case, "randn", NAN, None, (0, 1), fails, lines)
    if not big:
        _run_profile(case, "cancel", NAN, None, (0, 1), fails, lines)
        for pos in R.one_hot_positions(rows, splits):
            _run_profile(case, "one_hot_token", NAN, pos, (0, 1), fails, lines)
    torch.cuda.synchronize()
    print("\n".join(lines))
    assert not fails, f"{case}\n" + "\n".join(fails)


@pytest.mark.parametrize("case", R.tn_cases(), ids=lambda c: "x".join(str(v) for v in c))
def test_gemm_tn_slab_per_split(case):
    """ROW_CASES x the baseline width, the other WIDTHS x the reduced row set stated at dw_reference.WIDE_ROW_CASES, and the operands with ld > width."""
    _run_case(case)


def test_gemm_tn_slab_persistent_walk():
    """768 x 512 at rows = 5605, splits = 44: nk = 88, per = 2, 6 tiles x 44 splits = 264 items > 256 -- the single-phase kernel (variant 1) runs 256
    persistent workgroups, eight of which take a second item whose first K-tile is staged under the first item's last (gemm_tn.hip:57-59, :139).
    int_tagged (both poisons) and randn; the ping-pong kernel runs the same 264 items one per workgroup."""
    rows, splits, n_out, n_in = R.PERSISTENT
    assert R.n_items(rows, splits, n_out, n_in) == 264 and R.split_rule(rows, splits)[1] == 2
    _run_case((rows, splits, n_out, n_in, n_out, n_in), big=True)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# autograd.weight_grad
# ---------------------------------------------------------------------------------------------------------------------------------------------
WG_ROWS = 357
# (id, route, n_out, n_in, bias, DW_ITEMS).  At 357 rows (nk = 6) the planner's own request -- 256 items for the one 256 x 256 tile -- is clamped to 6
# splits of ONE K-tile (gemm_tn.hip:406), and the NT route's _split_k(128, 592, 384) = 6 splits of one 64-column K-tile likewise: the planner reaches
# several K-tiles per split only at model row counts.  The third case therefore sets the planner's item budget (autograd.DW_ITEMS, bench.py --dw-items)
# to 2: splits = 2, three K-tiles per split, on the same route.
WG_CASES = [("tn_bias", "tn", 256, 256, True, None), ("nt_bias_padded", "nt", 128, 588, True, None), ("tn_bias_2_items", "tn", 256, 256, True, 2)]


@pytest.mark.parametrize("case", WG_CASES, ids=[c[0] for c in WG_CASES])
def test_weight_grad_exact_integers(case, monkeypatch):
    """autograd.weight_grad on int_tagged operands, bit for bit, with accumulate 0 (onto NaN) and 1; the bias gradient is always added into.  Pad rows
    and pad columns of the operands hold 4096; the NT route's transposed operands keep their zero pad columns; nothing behind the gradients is written."""
    _, route, n_out, n_in, bias, items = case
    if items is not None:
        monkeypatch.setattr(A, "DW_ITEMS", items)
    rows, Kp, ld = WG_ROWS, (n_in + 7) // 8 * 8, ops.pad_rows(WG_ROWS)
    plan = A._dw_plan(n_out, n_in, bias=bias, tn_all=False, rows=rows)
    assert plan.tn == (route == "tn")
    if route == "tn":
        assert R.split_rule(rows, plan.splits)[1] == (3 if items == 2 else 1)
    dy_c, x_c = R.make_inputs("int_tagged", rows, n_out, n_in, 3, n_out, Kp, R.POISON_INT)
    dy_f, x_f = dy_c.to(DEV), x_c.to(DEV)
    ex = R.exact_tn(dy_f, x_f, rows, n_out, n_in, 1)
    old_w, old_b = R.make_old("int_tagged", ex["w0"], 3).to(DEV), R.make_old("int_tagged", ex["b0"], 4).to(DEV)
    R.assert_exact_ok(R.set_old(ex, old_w, old_b))
    dy, x = dy_f.bfloat16(), x_f.bfloat16()
    bf = torch.bfloat16
    scratch = dict(slab=torch.zeros(plan.slab_elems, device=DEV), part=ops.rowreduce_workspace(1, rows, n_out, DEV), bslab=torch.zeros(256 * n_out, device=DEV),
                   tA=torch.zeros(n_out, ld, dtype=bf, device=DEV), tB=torch.zeros(n_in, ld, dtype=bf, device=DEV), tn_all=False)
    fails = []
    for accumulate in (0, 1):
        gw = torch.full((n_out * n_in + 8,), NAN, device=DEV)
        gb = torch.full((n_out + 8,), NAN, device=DEV)
        if accumulate:
            gw[:n_out * n_in] = old_w.reshape(-1)
        gb[:n_out] = old_b
        A.weight_grad(dy, x, gw, n_out, n_in, rows, scratch, gb if bias else None, accumulate=accumulate)
        torch.cuda.synchronize()
        R.check_exact(f"weight_grad {case[0]} accumulate={accumulate} weight", gw[:n_out * n_in].view(n_out, n_in), ex[f"w{accumulate}"], fails)
        R.check_exact(f"weight_grad {case[0]} accumulate={accumulate} bias", gb[:n_out], ex["b1"], fails)
        if not (bool(torch.isnan(gw[n_out * n_in:]).all()) and bool(torch.isnan(gb[n_out:]).all())):
            fails.append(f"{case[0]}: written behind a gradient")
    if route == "nt":
        if bool(scratch["tA"][:, rows:].any()) or bool(scratch["tB"][:, rows:].any()):
            fails.append(f"{case[0]}: pad columns [rows, ld) of the transposed operands written")
        if not (torch.equal(scratch["tA"][:, :rows], dy[:rows, :n_out].t()) and torch.equal(scratch["tB"][:, :rows], x[:rows, :n_in].t())):
            fails.append(f"{case[0]}: the transposed operands are not the operands")
    print(f"DWREF weight_grad {case[0]} rows={rows} route={route} splits requested={plan.splits}: int_tagged equal={not fails}")
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _colsum_once(kind, src, rows, C, old, tag, fails):
    """colsum (+)= column sums of src[:rows, :C] onto `old`, 4 sentinel elements behind it."""
    dst = torch.full((C + 4,), NAN, device=DEV)
    dst[:C] = old
    src0 = src.clone()
    if kind == "bf16":
        ops.colsum_bf16(src, dst, rows, C)
    elif kind == "f32":
        ops.colsum_f32(src, dst, rows, C)
    else:
        ops.transpose_colsum(src, None, dst, rows, C, ld_in=src.shape[-1])
    if not bool(torch.isnan(dst[C:]).all()):
        fails.append(f"{tag}: written behind the column sums")
    if not _same(src, src0):
        fails.append(f"{tag}: the input changed")
    return dst[:C].clone()


def _colsum_case(kind, rows, C, ld, fails, lines):
    for profile, poison in (("int_tagged", R.POISON_INT), ("int_tagged", NAN), ("randn", NAN), ("cancel", NAN)):
        src_f = R.make_colsum_input(profile, kind, rows, C, ld=ld, poison=poison).to(DEV)
        old = R.make_old(profile, src_f[:rows, :C].sum(0), 5).to(DEV)
        ex = R.exact_colsum(src_f, rows, C, old)
        tol = R.bounds_colsum(kind, rows, ex)
        src = src_f if kind == "f32" else src_f.bfloat16()
        tag = f"colsum_{kind} R={rows} C={C} ld={ld} {profile} poison={'nan' if poison != poison else 'int'}"
        got = _colsum_once(kind, src, rows, C, old, tag, fails)
        if not _same(got, _colsum_once(kind, src, rows, C, old, tag + " (second run)", fails)):
            fails.append(f"{tag}: two runs give different bits")
        if profile == "int_tagged":
            R.assert_exact_ok(ex, tag)
            R.check_exact(tag, got, ex["ref"], fails)
        lines.append(f"DWREF {tag} err/tol={R.check(tag, got, ex['ref'], tol, fails):.3f}")


@pytest.mark.parametrize("rows", R.COLSUM_R)
@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_colsum(kind, rows):
    """colsum_bf16_kernel / colsum_f32_kernel + partials_reduce onto a nonzero old value: one lane, a full column block, a second column block with 8 (4)
    columns; rows >= R (and, in the bf16 case with ld > C, columns >= C) poisoned."""
    fails, lines = [], []
    for C in R.COLSUM_C[kind]:
        _colsum_case(kind, rows, C, C, fails, lines)
    if kind == "bf16" and rows == R.COLSUM_LD[0]:
        _colsum_case(kind, *R.COLSUM_LD, fails, lines)
    torch.cuda.synchronize()
    print("\n".join(lines))
    assert not fails, "\n".join(fails)


def _transpose_once(src, rows, C, ld_in, with_sums, old, tag, fails):
    ld_out = ops.pad_rows(rows)
    out = torch.full((C + 2, ld_out), NAN, dtype=torch.bfloat16, device=DEV)
    before = out.clone()
    dst = None
    if with_sums:
        dst = torch.full((C + 4,), NAN, device=DEV)
        dst[:C] = old
    ops.transpose_colsum(src, out, dst, rows, C, ld_in=ld_in, ld_out=ld_out)
    R.untouched(f"{tag} transposed", out, before, C, 0, rows, fails)          # pad columns [R, ld_out) and the rows behind C
    if not _same(out[:C, :rows], src[:rows, :C].t()):
        fails.append(f"{tag}: the transpose is not exact")
    if with_sums and not bool(torch.isnan(dst[C:]).all()):
        fails.append(f"{tag}: written behind the column sums")
    return dst[:C].clone() if with_sums else None


@pytest.mark.parametrize("rows", R.TRANSPOSE_R)
def test_transpose_colsum(rows):
    """transpose_colsum_kernel: the transpose bit-exact with its pad columns untouched, the column sums (with the transposed copy, and with dst = None)
    equal on int_tagged and inside the bounds on randn / cancel; C = 588 (ld 592) transposes alone through the scalar load path."""
    fails, lines = [], []
    for C in R.TRANSPOSE_C:
        for profile, poison in (("int_tagged", R.POISON_INT), ("int_tagged", NAN), ("randn", NAN), ("cancel", NAN)):
            src_f = R.make_colsum_input(profile, "transpose", rows, C, ld=C + 8, poison=poison, rows_alloc=ops.pad_rows(rows) + 1).to(DEV)
            old = R.make_old(profile, src_f[:rows, :C].sum(0), 6).to(DEV)
            ex = R.exact_colsum(src_f, rows, C, old)
            tol = R.bounds_colsum("transpose", rows, ex)
            src = src_f.bfloat16()
            tag = f"transpose_colsum R={rows} C={C} {profile} poison={'nan' if poison != poison else 'int'}"
            got = _transpose_once(src, rows, C, C + 8, True, old, tag, fails)
            alone = _colsum_once("transpose", src, rows, C, old, tag + " dst=None", fails)
            if not (_same(got, alone) and _same(got, _transpose_once(src, rows, C, C + 8, True, old, tag + " (second run)", fails))):
                fails.append(f"{tag}: the sums differ between runs, or with and without the transposed copy")
            if profile == "int_tagged":
                R.assert_exact_ok(ex, tag)
                R.check_exact(tag, got, ex["ref"], fails)
            lines.append(f"DWREF {tag} err/tol={R.check(tag, got, ex['ref'], tol, fails):.3f}")
    C = R.TRANSPOSE_ONLY_C
    for poison in (R.POISON_INT, NAN):
        src = R.make_colsum_input("int_tagged", "transpose", rows, C, ld=C + 4, poison=poison, rows_alloc=ops.pad_rows(rows) + 1).to(DEV).bfloat16()
        _transpose_once(src, rows, C, C + 4, False, None, f"transpose R={rows} C={C}", fails)
    torch.cuda.synchronize()
    print("\n".join(lines))
    assert not fails, "\n".join(fails)
