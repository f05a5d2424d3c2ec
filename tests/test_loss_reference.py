"""CPU test of tests/loss_reference.py: the kernel's operation sequence written over (value, error) pairs has the float64 autograd values; the f32 CPU
oracle and an f32 restatement of the kernels sit inside every derived bound, at no more than half of it; the contention costs drive the solver deep;
every spreading chain ends as its docstring says; and every planted error falls outside a named bound or changes a named decision."""
import numpy as np
import pytest
import torch

from oracle import owl_oracle as O
from tests import loss_reference as R

G4 = torch.tensor([2.0, 0.25, 5.0, 3.0])
COUNTS = {1: [1], 3: [9, 1, 4]}
SPREAD = {1: 0, 3: 2}
SCALES = {3: torch.tensor([3.1, 4.7, 3.9]), 10: torch.tensor([3.1, 4.7, 3.9, 4.2, 3.3, 5.0, 4.4, 3.6, 4.9, 3.0])}
WORST = {}


def _note(name, r):
    WORST[name] = max(WORST.get(name, 0.0), r)
    return r


# ---------------------------------------------------------------------------------------------------------------------------------------------
# f32 evaluations: the oracle (torch autograd in f32), and the kernels' own formulas in f32 with places to plant an error
# ---------------------------------------------------------------------------------------------------------------------------------------------
def oracle_f32(case, C, scales, g):
    sims, boxes = case["sims"], case["boxes"]
    B = sims.shape[0]
    so, bo = sims.clone().requires_grad_(True), boxes.clone().requires_grad_(True)
    det, per = [], []
    for b in range(B):
        d = {}
        l = O.push_pull_loss_one(so[b], case["labels"][b], bo[b], case["tgt"][b], C, scales, d)
        det.append(d)
        per.append(torch.stack([l["loss_ce"], l["loss_bg"], l["loss_bbox"], l["loss_giou"]]))
    per = torch.stack(per)
    losses = per.sum(0) / B
    (losses * g).sum().backward()
    return dict(det=det, per_image=per.detach(), losses=losses.detach(), grad_sims=so.grad, grad_boxes=bo.grad)


def k_class(sims, tc, bg, scales, plant=None):
    """class_loss_kernel in f32 -> (losses [2], dsims [P, C])."""
    P, C = sims.shape
    s, a, pos = sims, sims.abs(), tc != bg
    y = torch.zeros(P, C)
    y[pos, tc[pos]] = 1.0
    w = torch.ones(C) if scales is None else scales
    la, l1a = torch.log(a).clamp(min=-100.0), torch.log1p(-a).clamp(min=-100.0)
    l = -w * (y * la + (1.0 - y) * l1a)
    em = torch.exp(-l)
    om = 1.0 - em
    t = om * om * l
    npos = pos.sum().float()
    nbg = P - npos
    dp, db = (npos, nbg) if plant != "divide_by_P" else (torch.tensor(float(P)), torch.tensor(float(P)))
    loss = torch.stack([t[pos].sum() / dp, t[~pos].sum() / db])
    dF = 2.0 * om * em * l + om * om
    wg = torch.ones(C) if plant == "no_scales_in_grad" else w
    dl = wg * (a - y) / ((1.0 - a) * a).clamp(min=1e-12)
    return loss, dF * dl * torch.sign(s) * torch.where(pos, 1.0 / npos, 1.0 / nbg)[:, None]


def k_box(boxes, tgt, pi, ti, plant=None):
    """box_loss_kernel in f32 -> (losses [2], dl1 [P, 4], dgiou [P, 4])."""
    P, n = boxes.shape[0], pi.shape[0]
    A, T = boxes[pi], tgt[ti]
    ax, ay, az, aw = A.unbind(1)
    tx, ty, tz, tw = T.unbind(1)
    invn = torch.tensor(1.0) / n
    zero = torch.zeros(())
    l1 = (((ax - tx).abs() + (ay - ty).abs()) + (az - tz).abs()) + (aw - tw).abs()
    area_a, area_b = (az - ax) * (aw - ay), (tz - tx) * (tw - ty)
    ltx, lty, rbx, rby = torch.max(ax, tx), torch.max(ay, ty), torch.min(az, tz), torch.min(aw, tw)
    w, h = torch.max(rbx - ltx, zero), torch.max(rby - lty, zero)
    inter = w * h
    uni = area_a + area_b - inter
    iou = inter / uni
    cx0, cy0, cx1, cy1 = torch.min(ax, tx), torch.min(ay, ty), torch.max(az, tz), torch.max(aw, tw)
    cw, ch = torch.max(cx1 - cx0, zero), torch.max(cy1 - cy0, zero)
    area_c = cw * ch
    giou = iou - (area_c - uni) / area_c
    loss = torch.stack([l1.sum() * invn, (1.0 - giou).sum() * invn])
    tie = 1.0 if plant == "tie_weight_1" else 0.5
    gt = lambda p, q: torch.where(p > q, 1.0, torch.where(p == q, tie, 0.0))        # noqa: E731
    lt = lambda p, q: gt(q, p)                                                      # noqa: E731
    on = (lambda d: (d > 0).float()) if plant == "closed_at_zero_width" else (lambda d: (d >= 0).float())
    dw_on, dh_on, dcw_on, dch_on = on(rbx - ltx), on(rby - lty), on(cx1 - cx0), on(cy1 - cy0)
    d_inter = [dw_on * -gt(ax, tx) * h, w * dh_on * -gt(ay, ty), dw_on * lt(az, tz) * h, w * dh_on * lt(aw, tw)]
    d_area_a = [-(aw - ay), -(az - ax), aw - ay, az - ax]
    d_area_c = [dcw_on * -lt(ax, tx) * ch, cw * dch_on * -lt(ay, ty), dcw_on * gt(az, tz) * ch, cw * dch_on * gt(aw, tw)]
    dl1, dg = torch.zeros(P, 4), torch.zeros(P, 4)
    dl1[pi] = torch.sign(A - T) * invn
    for k in range(4):
        d_uni = d_area_a[k] - d_inter[k]
        d_iou = (d_inter[k] * uni - inter * d_uni) / (uni * uni)
        d_ratio = (d_uni * area_c - uni * d_area_c[k]) / (area_c * area_c)
        dg[pi, k] = -(d_iou + d_ratio) * invn
    return loss, dl1, dg


def k_combine(g, tc, bg, dsims, dl1, dgiou, B, plant=None):
    """loss_bwd_kernel in f32 on [rows, .] inputs."""
    invB = torch.tensor(1.0) / B
    if plant == "invB_twice":
        invB = invB * invB
    i0, i1, i2, i3 = {"swap_g0_g1": (1, 0, 2, 3), "swap_g2_g3": (0, 1, 3, 2)}.get(plant, (0, 1, 2, 3))
    gk = torch.where(tc != bg, g[i0], g[i1]) * invB
    return gk[:, None] * dsims, (g[i2] * invB) * dl1 + (g[i3] * invB) * dgiou


def kernels_f32(case, dec, C, scales, g, plant=None):
    """The whole criterion through k_class / k_box / k_combine at the given decisions."""
    B, P, _ = case["sims"].shape
    per, ds, d1, d2 = [], [], [], []
    for b in range(B):
        lc, dsb = k_class(case["sims"][b], dec["tc"][b], C, scales, plant)
        lb, d1b, d2b = k_box(case["boxes"][b], case["tgt"][b], dec["pi"][b], dec["ti"][b], plant)
        per.append(torch.cat([lc, lb])); ds.append(dsb); d1.append(d1b); d2.append(d2b)
    per = torch.stack(per)
    gs, gb = k_combine(g, dec["tc"].reshape(-1), C, torch.cat(ds), torch.cat(d1), torch.cat(d2), B, plant)
    return dict(per_image=per, losses=per.sum(0) / B, grad_sims=gs.view(B, P, -1), grad_boxes=gb.view(B, P, 4))


def _decide(case, C):
    """The oracle's decisions from its own f32 costs."""
    out = dict(pi=[], ti=[], tc=[], cost=[])
    for b in range(case["sims"].shape[0]):
        cost, i, j, tc = O.match_one(case["sims"][b], case["boxes"][b], case["labels"][b], case["tgt"][b], C)
        out["cost"].append(cost); out["pi"].append(i); out["ti"].append(j)
        out["tc"].append(O.spread_labels(case["boxes"][b], tc, C))
    out["tc"] = torch.stack(out["tc"])
    return out


def _reference(case, dec, C, scales, g):
    return R.criterion(case["sims"], case["boxes"], dec["tc"], dec["pi"], dec["ti"], case["tgt"], C, scales, g)


NAMES = ("per_image", "losses", "grad_sims", "grad_boxes")
GRID = [(profile, P, C, B) for profile in R.PROFILES for (P, C, B) in ((48, 3, 3), (577, 10, 3), (48, 10, 1), (2304, 3, 1))]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the bounds hold for correct f32 evaluations, with room
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile,P,C,B", GRID)
def test_f32_evaluations_sit_inside_half_of_every_bound(profile, P, C, B):
    for scales in (None, SCALES[C]):
        case = R.make_case(profile, B, P, C, seed=P + C, counts=COUNTS[B], spread=SPREAD[B])
        dec = _decide(case, C)
        if B == 3:
            assert int((dec["tc"][0] != C).sum()) > COUNTS[3][0], "spreading: positives must outnumber the matches"
            assert int((dec["tc"][1] != C).sum()) == 3
        else:
            assert int((dec["tc"][0] != C).sum()) == 1, "npos = 1"
        ref = _reference(case, dec, C, scales, G4)
        got_o = oracle_f32(case, C, scales, G4)
        for b in range(B):
            assert torch.equal(got_o["det"][b]["target_classes"], dec["tc"][b])
            cs = R.cost_stage(case["sims"][b], case["boxes"][b], case["labels"][b], case["tgt"][b])
            r = _note("oracle.cost", float(R.ratios(dec["cost"][b], cs["ref"], cs["tol"]).max()))
            assert r <= 0.5, ("cost", b, r)
        got_k = kernels_f32(case, dec, C, scales, G4)
        for who, got in (("oracle", got_o), ("kernel_f32", got_k)):
            for name in NAMES:
                r = _note(f"{who}.{name}", float(R.ratios(got[name], *ref[name]).max()))
                assert r <= 0.5, (who, name, profile, r)
    print("LOSSREF cpu worst ratios", {k: round(v, 3) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("profile", R.PROFILES)
def test_kernel_formulas_have_the_autograd_values(profile):
    """The (value, error) restatement of the kernels is the float64 autograd of the oracle's expressions: |v - ref| <= 1e-8 |ref| (the f32 constant
    1e-12f in the BCE-backward clamp is 4e-9 from torch's double one), so `tol = e + |v - ref|` hides no wrong formula."""
    C = 10
    case = R.make_case(profile, 1, 200, C, seed=3, counts=[12], spread=2)
    dec = _decide(case, C)
    cls = R.class_stage(case["sims"][0], dec["tc"][0], C, SCALES[C])
    box = R.box_stage(case["boxes"][0], case["tgt"][0], dec["pi"][0], dec["ti"][0])
    cst = R.cost_stage(case["sims"][0], case["boxes"][0], case["labels"][0], case["tgt"][0])
    for name, ev, ref in (("class loss", cls["ev_loss"], cls["loss"][0]), ("dsims", cls["ev_dsims"], cls["dsims"][0]),
                          ("box loss", box["ev_loss"], box["loss"][0]), ("dl1", box["ev_dl1"], box["dl1"][0]), ("dgiou", box["ev_dgiou"], box["dgiou"][0]),
                          ("cost", cst["ev"], cst["ref"])):
        assert bool(((ev.v - ref).abs() <= 1e-8 * ref.abs() + 1e-300).all()), name
    if profile == "trained_like":
        a = case["sims"][0].abs()
        assert bool(((1 - a.max(1).values) <= 4 * 2.0 ** -24).all()), "a column within 4 ulp of 1 in every row"
        # the bound widens where it should: relative tolerance of the loss term's gradient is far above 1e-3 on some elements, far below on others
        rel = cls["dsims"][1] / cls["dsims"][0].abs().clamp(min=1e-300)
        assert float(rel.max()) > 1e-3 and float(rel.min()) < 1e-5
    if profile == "tiny":
        assert bool((case["sims"].abs() < 2.0 ** -126).any()) and bool(torch.isfinite(cls["dsims"][0]).all())
        # a subnormal in the label column of a positive row whose log is NOT clamped: an evaluation that flushes it reads -100 for about -90
        tc = dec["tc"][0]
        lab = case["sims"][0].abs()[tc != C].gather(1, tc[tc != C][:, None])
        assert bool(((lab < 2.0 ** -126) & (lab > 1e-43)).any())
    if profile == "exact":
        assert bool((case["sims"] == 0).any()) and bool((case["sims"].abs() == 1).any()) and bool(torch.isfinite(cls["dsims"][0]).all())


def test_double_class_loss_is_the_oracles_in_f32():
    case = R.make_case("uniform", 1, 48, 3, seed=1, counts=[5], spread=1)
    tc = _decide(case, 3)["tc"][0]
    for scales in (None, SCALES[3]):
        assert all(torch.equal(x, y) for x, y in zip(R.class_loss_any_dtype(case["sims"][0], tc, 3, scales), O.class_loss(case["sims"][0], tc, 3, scales)))


def test_edge_pairs_reach_ties_and_zero_width():
    boxes, tgt, pi, ti = R.edge_pairs()
    assert bool((boxes[0] == tgt[0]).all()) and boxes[1, 0] == tgt[1, 0] and boxes[1, 3] == tgt[1, 3]
    assert torch.min(boxes[2, 2], tgt[2, 2]) - torch.max(boxes[2, 0], tgt[2, 0]) == 0
    ref = R.box_stage(boxes, tgt, pi, ti)
    loss, dl1, dg = k_box(boxes, tgt, pi, ti)
    for name, got in (("loss", loss), ("dgiou", dg)):
        assert float(R.ratios(got, *ref[name]).max()) <= 0.5, name
    # dl1 = +-fl(1 / n) is ONE rounding: its bound f |v| is attainable, and fl(1 / 6) sits at exactly half of it
    assert float(R.ratios(dl1, *ref["dl1"]).max()) <= 0.5 + 1e-6
    assert float(ref["dgiou"][0][2].abs().max()) > 0.1, "the touching pair has a gradient through the clamp"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the builders do what they claim
# ---------------------------------------------------------------------------------------------------------------------------------------------
CONTENTION = [(40, 64), (48, 48), (100, 2304)]


@pytest.mark.parametrize("n,P", CONTENTION)
def test_contention_costs_drive_the_solver_deep(n, P):
    cost = R.contention_cost(n, P)
    col4row, trace = R.sap_trace(cost)
    i, j = O.linear_sum_assignment(cost.T)
    assert np.array_equal(np.sort(col4row), i) and np.array_equal(np.argsort(col4row), j), "the restated loop is not the oracle's"
    scanned, chain = max(t[0] for t in trace), max(t[1] for t in trace)
    print(f"LOSSREF contention n={n} P={P} rows scanned {scanned} chain {chain}")
    assert scanned >= n / 2 and chain >= n / 4, (scanned, chain)
    if P > n:   # what the uniform costs of the earlier tests reach where predictions outnumber targets, for the record: a handful of rows
        _, shallow = R.sap_trace(np.random.RandomState(0).rand(n, P).astype(np.float32))
        assert max(t[0] for t in shallow) < n / 4 and max(t[1] for t in shallow) < n / 8


@pytest.mark.parametrize("P", [33, 64, 65, 2304, 3600, 4200])
@pytest.mark.parametrize("pattern", R.SPREAD_PATTERNS)
def test_spreading_chains_end_as_documented(P, pattern):
    c = R.spread_case(P, pattern)
    out = O.spread_labels(c["boxes"], c["tc"], R.SPREAD_BG)
    for row, lab in c["expect"].items():
        assert int(out[row]) == lab, (row, int(out[row]), lab)
    assert int((out != c["tc"]).sum()) == c["changed"], "a row outside the documented ones changed"
    if pattern == "background":
        assert c["changed"] == 0
    else:
        assert c["changed"] >= 2
    if pattern == "mixed":
        iou, _ = O.box_iou(c["boxes"][12:13], c["boxes"][13:15])
        assert float(iou[0, 0]) == R.THR32 and float(iou[0, 1]) == float(np.nextafter(np.float32(0.85), np.float32(1)))
    if pattern == "forward" and P >= 2304:
        assert {0, 31, 32, 2047, 2048, 2111, 2112, P - 1} <= set(c["expect"])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# planted errors
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _spread_variant(boxes, tc, bg, plant):
    tc = tc.clone()
    P = tc.shape[0]
    seeds = (tc != bg).clone()
    passes = 3 if plant == "revisits_rows_behind" else 1
    for _ in range(passes):
        for p in range(P):
            if int(tc[p]) == bg or (plant == "one_pass_not_transitive" and not seeds[p]) or (plant == "blind_from_row_2048" and p >= 2048):
                continue
            iou, _ = O.box_iou(boxes[p:p + 1], boxes)
            hit = iou[0] > 0.85
            if plant == "keeps_existing_positive":
                hit &= tc == bg
            tc[hit] = int(tc[p])
    return tc


@pytest.mark.parametrize("plant,pattern,P,row", [("revisits_rows_behind", "mixed", 65, 5), ("keeps_existing_positive", "overwrite", 65, 1),
                                                  ("blind_from_row_2048", "forward", 2304, 2049), ("one_pass_not_transitive", "forward", 65, 30)])
def test_planted_spreading_errors_change_a_decision(plant, pattern, P, row):
    c = R.spread_case(P, pattern)
    assert torch.equal(_spread_variant(c["boxes"], c["tc"], R.SPREAD_BG, None), O.spread_labels(c["boxes"], c["tc"], R.SPREAD_BG))
    bad = _spread_variant(c["boxes"], c["tc"], R.SPREAD_BG, plant)
    assert int(bad[row]) != c["expect"][row], f"{plant}: row {row} of the {pattern} chain still ends {c['expect'][row]}"
    print(f"LOSSREF planted {plant}: caught by the decision at row {row} of spread_case({P}, {pattern!r})")


def test_planted_greedy_assignment_changes_a_decision():
    cost = R.contention_cost(40, 64)
    i, j = O.linear_sum_assignment(cost.T)
    taken, greedy = set(), []
    for t in range(40):
        p = next(int(p) for p in np.argsort(cost[t], kind="stable") if int(p) not in taken)
        taken.add(p); greedy.append(p)
    opt = np.empty(40, np.int64); opt[j] = i
    assert not np.array_equal(np.asarray(greedy), opt), "greedy assignment: the indices still agree"
    assert cost.astype(np.float64)[np.arange(40), greedy].sum() > cost.astype(np.float64)[j, i].sum()
    print("LOSSREF planted greedy_assignment: caught by the decision pred_idx / the assigned cost of contention_cost(40, 64)")


PLANTS = [("divide_by_P", "per_image"), ("no_scales_in_grad", "grad_sims"), ("swap_g0_g1", "grad_sims"), ("swap_g2_g3", "grad_boxes"),
          ("invB_twice", "grad_sims")]


@pytest.mark.parametrize("plant,bound", PLANTS)
def test_planted_arithmetic_errors_fall_outside_a_bound(plant, bound):
    C, B = 3, 3
    case = R.make_case("uniform", B, 48, C, seed=11, counts=COUNTS[B], spread=2)
    dec = _decide(case, C)
    ref = _reference(case, dec, C, SCALES[C], G4)
    good = kernels_f32(case, dec, C, SCALES[C], G4)
    assert all(float(R.ratios(good[n], *ref[n]).max()) <= 0.5 for n in NAMES)
    bad = kernels_f32(case, dec, C, SCALES[C], G4, plant)
    r = float(R.ratios(bad[bound], *ref[bound]).max())
    assert r > 1.0, f"{plant}: inside the bound of {bound} (ratio {r:.3f})"
    print(f"LOSSREF planted {plant}: caught by the bound of {bound}, ratio {r:.3g}")


@pytest.mark.parametrize("plant,pair", [("tie_weight_1", 1), ("closed_at_zero_width", 2)])
def test_planted_box_gradient_errors_fall_outside_a_bound(plant, pair):
    boxes, tgt, pi, ti = R.edge_pairs()
    ref = R.box_stage(boxes, tgt, pi, ti)
    _, _, dg = k_box(boxes, tgt, pi, ti, plant)
    r = float(R.ratios(dg[pair], ref["dgiou"][0][pair], ref["dgiou"][1][pair]).max())
    assert r > 1.0, f"{plant}: inside the bound of dgiou at edge pair {pair} (ratio {r:.3f})"
    print(f"LOSSREF planted {plant}: caught by the bound of dgiou at edge pair {pair}, ratio {r:.3g}")
