"""The criterion of csrc/loss.hip against the float64 references and derived bounds of tests/loss_reference.py.

What is pinned: the solver on costs that make it scan most target rows and re-route long chains (indices, labels and padding bit for bit against
oracle/lsap.c); label spreading at the word, probe and cursor edges of spread_kernel at the model's own P (bit for bit, with the number of rows that
changed asserted); matching cost, the four losses, their per-image terms and both gradients elementwise inside the derived bounds at upstream weights
(2, 0.25, 5, 3), so that no two terms can trade places unseen; each loss backward alone, one-sided requires_grad, no-grad forward and the batch
invariant.  tests/test_loss_reference.py shows on the CPU that the bounds hold for a correct f32 evaluation at no more than half and catch the planted
errors.  The measured worst ratios are kept in profiles/loss_reference.md."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import owl_oracle as O  # noqa: E402  (checker only)
from owl_vit_object_detection_amd import _lib, ops  # noqa: E402
from owl_vit_object_detection_amd.losses import PushPullLoss  # noqa: E402
from tests import loss_reference as R  # noqa: E402

DEV = "cuda"
BG = 99
G4 = (2.0, 0.25, 5.0, 3.0)
KEYS = ("loss_ce", "loss_bg", "loss_bbox", "loss_giou")
COUNTS = {1: [1], 3: [9, 1, 4]}
SPREAD = {1: 0, 3: 2}
SCALES = {3: torch.tensor([3.1, 4.7, 3.9]), 10: torch.tensor([3.1, 4.7, 3.9, 4.2, 3.3, 5.0, 4.4, 3.6, 4.9, 3.0])}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# owl_hungarian, called directly
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _solve(costT, counts, labels):
    B, Nmax, P = costT.shape
    pi = torch.full((B, Nmax), -7, dtype=torch.int64, device=DEV)
    ti = torch.full((B, Nmax), -7, dtype=torch.int64, device=DEV)
    tc = torch.full((B, P), -5, dtype=torch.int64, device=DEV)
    _lib.call("owl_hungarian", ops.stream(), torch.from_numpy(costT).to(DEV).contiguous(), labels.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV),
              pi, ti, tc, B, P, Nmax, BG)
    return pi.cpu(), ti.cpu(), tc.cpu()


def _check_solver(costT, counts):
    B, Nmax, P = costT.shape
    labels = (torch.arange(B * Nmax).reshape(B, Nmax) * 7 + 3) % 11
    pi, ti, tc = _solve(costT, counts, labels)
    for b, n in enumerate(counts):
        c = costT[b, :n].astype(np.float64)
        i, j = O.linear_sum_assignment(c.T)
        assert np.array_equal(pi[b, :n].numpy(), i) and np.array_equal(ti[b, :n].numpy(), j), f"image {b}: indices differ from the oracle's"
        assert bool((pi[b, n:] == 0).all()) and bool((ti[b, n:] == 0).all()), f"image {b}: padding not zero-filled"
        want = torch.full((P,), BG, dtype=torch.int64)
        want[torch.from_numpy(i)] = labels[b][torch.from_numpy(j)]
        assert torch.equal(tc[b], want), f"image {b}: target_classes"
        assert c[ti[b, :n].numpy(), pi[b, :n].numpy()].sum() == c[j, i].sum(), f"image {b}: assigned cost"
    again = _solve(costT, counts, labels)
    assert all(torch.equal(x, y) for x, y in zip((pi, ti, tc), again)), "two runs differ"


@pytest.mark.parametrize("n,P", [(40, 64), (48, 48), (100, 2304)])
def test_hungarian_contention_costs(n, P):
    """Costs on which an augmentation scans >= n / 2 rows and re-routes a chain >= n / 4 long (tests/test_loss_reference.py measures it): the dual
    update over many scanned rows, the `remaining` compaction many steps deep and the long `path` walk.  (48, 48): n = Nmax = P."""
    _check_solver(R.contention_cost(n, P)[None], [n])


def test_hungarian_ragged_batch_with_nan_padding():
    counts = [40, 7, 1]
    costT = np.full((3, 40, 64), np.nan, np.float32)
    for b, n in enumerate(counts):
        costT[b, :n] = R.contention_cost(n, 64, seed=b)
    _check_solver(costT, counts)


def test_hungarian_duplicated_columns_tie_exactly():
    """Pairs of identical prediction columns: exact real-valued ties in every scan; scipy's rule decides (first minimum, unless a later equal one is free)."""
    costT = R.contention_cost(40, 64)
    costT[:, 1::2] = costT[:, 0::2]
    costT[:, 40:48] = costT[:, 32:33]
    _check_solver(costT[None], [40])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# owl_spread_labels, called directly
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _spread(boxes, tc):
    B, P = tc.shape
    out = tc.to(DEV).clone()
    _lib.call("owl_spread_labels", ops.stream(), boxes.to(DEV).contiguous(), out, B, P, R.SPREAD_BG, 0.85)
    return out.cpu()


@pytest.mark.parametrize("P", [33, 64, 65, 2304, 3600, 4200])
def test_spreading_at_word_probe_and_cursor_edges(P):
    """Every pattern of loss_reference.spread_case alone, then three of them as one batch: bit for bit against the oracle's sequential loop, the batch
    equal to its B = 1 calls, and the number of rows that changed as the builder states it (no comparison of background with background)."""
    cases = {pattern: R.spread_case(P, pattern) for pattern in R.SPREAD_PATTERNS}
    alone = {}
    for pattern, c in cases.items():
        want = O.spread_labels(c["boxes"], c["tc"], R.SPREAD_BG)
        got = _spread(c["boxes"][None], c["tc"][None])[0]
        assert int((want != c["tc"]).sum()) == c["changed"], pattern
        assert c["changed"] == 0 if pattern == "background" else c["changed"] >= 2, pattern
        bad = (got != want).nonzero().flatten().tolist()
        assert not bad, f"{pattern}: rows {bad[:8]} got {got[bad[:8]].tolist()} want {want[bad[:8]].tolist()}"
        for row, lab in c["expect"].items():
            assert int(got[row]) == lab, (pattern, row)
        alone[pattern] = got
    for trio in (("forward", "overwrite", "mixed"), ("mixed", "background", "forward")):
        got = _spread(torch.stack([cases[p]["boxes"] for p in trio]), torch.stack([cases[p]["tc"] for p in trio]))
        for b, pattern in enumerate(trio):
            assert torch.equal(got[b], alone[pattern]), f"image {b} ({pattern}) of the batch differs from its B = 1 call"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# PushPullLoss, forward and backward
# ---------------------------------------------------------------------------------------------------------------------------------------------
class Tally:
    """Per tensor: the worst |got - ref| / bound and the first offenders."""

    def __init__(self):
        self.worst, self.fails = {}, []

    def add(self, name, where, got, ref, tol):
        r = R.ratios(got.detach().cpu(), ref, tol)
        self.worst[name] = max(self.worst.get(name, 0.0), float(r.max()))
        bad = r > 1.0
        if bool(bad.any()):
            first = []
            for idx in bad.nonzero()[:4].tolist():
                i = tuple(idx)
                first.append(f"{list(i)}: got {float(got[i]):.9g} ref {float(ref[i]):.9g} bound {float(tol[i]):.3g}")
            self.fails.append(f"{name} {where}: {int(bad.sum())}/{bad.numel()} outside the bound, worst ratio {float(r.max()):.3f}; " + "; ".join(first))

    def finish(self, tag):
        print(f"LOSSREF {tag} " + " ".join(f"{k}={v:.3f}" for k, v in sorted(self.worst.items())))
        assert not self.fails, tag + "\n" + "\n".join(self.fails)


def _run(case, C, scales, g=G4, grad=(True, True), only=None):
    """One PushPullLoss call (and the backward of sum_k g_k loss_k, or of g_only loss_only alone) on the device."""
    sims = case["sims"].to(DEV).requires_grad_(grad[0])
    boxes = case["boxes"].to(DEV).requires_grad_(grad[1])
    crit = PushPullLoss(C, scales)
    labels, tgt = [l.to(DEV) for l in case["labels"]], [t.to(DEV) for t in case["tgt"]]
    out = crit(sims, labels, boxes, tgt)
    if any(grad):
        (g[only] * out[KEYS[only]] if only is not None else sum(w * out[k] for w, k in zip(g, KEYS))).backward()
    torch.cuda.synchronize()
    return dict(losses=torch.stack([out[k].detach() for k in KEYS]).cpu(), per_image=crit.last["per_image"].cpu(), tc=crit.last["target_classes"].cpu(),
                pi=crit.last["pred_idx"].cpu(), ti=crit.last["tgt_idx"].cpu(), grad_sims=None if sims.grad is None else sims.grad.cpu(),
                grad_boxes=None if boxes.grad is None else boxes.grad.cpu(), crit=crit)


def _device_costs(case, C):
    crit = PushPullLoss(C, None)
    tg = crit.pack([l.to(DEV) for l in case["labels"]], [t.to(DEV) for t in case["tgt"]], DEV)
    return crit.matcher.match_packed(case["sims"].to(DEV), case["boxes"].to(DEV), tg)[3].cpu()


def _decisions(case, C, got, tally=None, where=""):
    """The device's matching cost inside its bound; then the device's decisions equal to the oracle's on THAT cost matrix, bit for bit."""
    costT = _device_costs(case, C)
    pis, tis = [], []
    for b, labels in enumerate(case["labels"]):
        n = labels.shape[0]
        cost = costT[b, :n].t().contiguous()
        if tally is not None:
            cs = R.cost_stage(case["sims"][b], case["boxes"][b], labels, case["tgt"][b])
            tally.add("cost", f"{where}[b={b}]", cost, cs["ref"], cs["tol"])
        i, j, _, tc = R.decisions(cost.numpy(), labels, case["boxes"][b], C)
        assert torch.equal(got["pi"][b, :n], i) and torch.equal(got["ti"][b, :n], j), f"{where} image {b}: assignment"
        assert torch.equal(got["tc"][b], tc), f"{where} image {b}: post-spreading labels"
        pis.append(i); tis.append(j)
    return pis, tis


def _reference(case, C, got, pis, tis, scales, g):
    return R.criterion(case["sims"], case["boxes"], got["tc"], pis, tis, case["tgt"], C, scales, torch.tensor(g))


@pytest.mark.parametrize("C", [3, 10])
@pytest.mark.parametrize("P", [48, 577, 2304])
@pytest.mark.parametrize("profile", R.PROFILES)
def test_push_pull_loss_inside_derived_bounds(profile, P, C):
    """B = 1 with a single target and no spreading (npos = 1) and B = 3 with spreading (positives outnumber matches), with and without `scales`:
    cost, per-image terms, losses and both gradients element by element inside the derived bounds, at upstream weights (2, 0.25, 5, 3)."""
    tally = Tally()
    for B in (1, 3):
        for scales in (None, SCALES[C]):
            where = f"B={B} scales={scales is not None}"
            case = R.make_case(profile, B, P, C, seed=P + C, counts=COUNTS[B], spread=SPREAD[B])
            got = _run(case, C, scales)
            pis, tis = _decisions(case, C, got, tally, where)
            npos = (got["tc"] != C).sum(1).tolist()
            assert npos == [1] if B == 1 else (npos[0] > COUNTS[3][0] and npos[1] > 1), npos
            ref = _reference(case, C, got, pis, tis, scales, G4)
            for name in ("per_image", "losses", "grad_sims", "grad_boxes"):
                tally.add(name, where, got[name], *ref[name])
    tally.finish(f"profile={profile} P={P} C={C}")


def _routing_case():
    C, B, P = 10, 3, 577
    return R.make_case("uniform", B, P, C, seed=23, counts=COUNTS[B], spread=SPREAD[B]), C


def test_each_loss_backward_alone():
    """g[0] / g[1] route by row kind, g[2] / g[3] by box term: the backward of one loss alone must be that loss's gradient and nothing of the others."""
    case, C = _routing_case()
    tally = Tally()
    for k in range(4):
        got = _run(case, C, SCALES[C], only=k)
        pis, tis = _decisions(case, C, got)
        g = [0.0] * 4
        g[k] = G4[k]
        ref = _reference(case, C, got, pis, tis, SCALES[C], g)
        for name in ("grad_sims", "grad_boxes"):
            tally.add(f"{KEYS[k]}.{name}", "", got[name], *ref[name])
        live = "grad_sims" if k < 2 else "grad_boxes"
        dead = "grad_boxes" if k < 2 else "grad_sims"
        assert float(got[live].abs().max()) > 0 and float(got[dead].abs().max()) == 0, KEYS[k]
    tally.finish("each loss alone")


def test_one_sided_requires_grad_and_no_grad_forward_keep_the_bits():
    case, C = _routing_case()
    both = _run(case, C, SCALES[C])
    only_s = _run(case, C, SCALES[C], grad=(True, False))
    only_b = _run(case, C, SCALES[C], grad=(False, True))
    none = _run(case, C, SCALES[C], grad=(False, False))
    assert only_s["grad_boxes"] is None and torch.equal(only_s["grad_sims"], both["grad_sims"])
    assert only_b["grad_sims"] is None and torch.equal(only_b["grad_boxes"], both["grad_boxes"])
    for other in (only_s, only_b, none):
        assert torch.equal(other["losses"], both["losses"]) and torch.equal(other["per_image"], both["per_image"])
        assert torch.equal(other["tc"], both["tc"]) and torch.equal(other["pi"], both["pi"]) and torch.equal(other["ti"], both["ti"])


@pytest.mark.parametrize("profile,P,C", [("uniform", 577, 10), ("trained_like", 2304, 3)])
def test_image_of_a_batch_holds_its_batch1_terms(profile, P, C):
    B = 3
    case = R.make_case(profile, B, P, C, seed=5, counts=COUNTS[B], spread=SPREAD[B])
    got = _run(case, C, SCALES[C])
    for b in range(B):
        one = dict(sims=case["sims"][b:b + 1], boxes=case["boxes"][b:b + 1], labels=case["labels"][b:b + 1], tgt=case["tgt"][b:b + 1])
        g1 = _run(one, C, SCALES[C])
        n = COUNTS[B][b]
        assert torch.equal(g1["per_image"][0], got["per_image"][b]), f"image {b}: per-image terms differ from its batch-1 call"
        assert torch.equal(g1["tc"][0], got["tc"][b]) and torch.equal(g1["pi"][0, :n], got["pi"][b, :n]) and torch.equal(g1["ti"][0, :n], got["ti"][b, :n])
        # B = 1: the mean over one image is that image's term
        assert torch.equal(g1["losses"], g1["per_image"][0])
