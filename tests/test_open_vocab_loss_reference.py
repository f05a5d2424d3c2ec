"""CPU: the float64 restatement of tests/open_vocab_loss_reference.py against live transformers and against the recorded fixture
tests/golden/f17_open_vocab_loss.npz; its builders; an f32 emulation of the kernels' operation sequences inside the derived bounds; the planted errors
the bounds must catch on the GPU cases' inputs; the Python surface's errors and `allow_empty`."""
import os

import numpy as np
import pytest
import torch

from tests import open_vocab_loss_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f17_open_vocab_loss.npz")
G3 = torch.tensor([1.0, 5.0, 2.0])
_crit_cache = {}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def _restated(case, weights=(1.0, 5.0, 2.0)):
    """The restatement on a case: per-image cost, decisions, the three losses and the autograd gradients, all in double."""
    B, P, Q = case["logits"].shape
    costs = [R.cost_double(case["logits"][b], case["boxes"][b], case["labels"][b], case["tgt"][b], None if case["mask"] is None else case["mask"][b])
             for b in range(B)]
    tcs, pi, ti = R.oracle_decisions(case)
    nb = float(max(1, sum(case["counts"])))
    ld = case["logits"].double().requires_grad_(True)
    bd = case["boxes"].double().requires_grad_(True)
    ce, l1, gi = R.loss_double(ld, bd, case["mask"], tcs, pi, ti, case["tgt"], 0.25, nb)
    (weights[0] * ce + weights[1] * l1 + weights[2] * gi).backward()
    return dict(cost=costs, pi=pi, ti=ti, tcs=tcs, losses=torch.stack([ce, l1, gi]).detach(), dlogits=ld.grad, dboxes=bd.grad)


def test_the_restatement_is_live_transformers():
    pytest.importorskip("transformers")
    from tests.golden.make_golden_open_vocab_loss import hf_run
    free = R.make_case(B=2, P=36, Q=7, counts=[4, 2], mask_kind=None, profile="uniform", fill=R.FMIN, seed=31, ties=False)
    for case in (R.fixture_inputs(), free):
        hf, me = hf_run(case), _restated(case)
        for b, n in enumerate(case["counts"]):
            assert _rel(me["cost"][b], torch.from_numpy(hf["cost"][b])) < 1e-12
            assert torch.equal(me["pi"][b], hf["indices"][b][0]) and torch.equal(me["ti"][b], hf["indices"][b][1])
        for k in ("losses", "dlogits", "dboxes"):
            assert _rel(me[k], hf[k]) < 1e-12, k
    # the cost defaults OpenVocabLoss documents are DeformableDetrConfig's
    from transformers import DeformableDetrConfig
    c = DeformableDetrConfig()
    assert (c.class_cost, c.bbox_cost, c.giou_cost, c.focal_alpha) == (1, 5, 2, 0.25)


def _fixture():
    z = np.load(GOLDEN)
    counts = z["counts"].tolist()
    case = dict(logits=torch.from_numpy(z["logits"]), boxes=torch.from_numpy(z["boxes"]), mask=torch.from_numpy(z["mask"]), counts=counts,
                labels=[torch.from_numpy(z["labels"][b, :n]) for b, n in enumerate(counts)], tgt=[torch.from_numpy(z["tgt"][b, :n]) for b, n in enumerate(counts)])
    return z, case


def test_the_restatement_is_the_recorded_fixture():
    z, case = _fixture()
    built = R.fixture_inputs()
    assert torch.equal(built["logits"], case["logits"]) and torch.equal(built["boxes"], case["boxes"]) and torch.equal(built["mask"], case["mask"])
    assert case["counts"] == [1, 3, 5] and case["logits"].shape == (3, 36, 5) and int((~case["mask"]).sum()) == 2
    me = _restated(case, tuple(z["weights"].tolist()))
    for b, n in enumerate(case["counts"]):
        assert _rel(me["cost"][b], torch.from_numpy(z["cost"][b, :, :n])) < 1e-12
        assert me["pi"][b].tolist() == z["pred_idx"][b, :n].tolist() and me["ti"][b].tolist() == z["tgt_idx"][b, :n].tolist()
    for k in ("losses", "dlogits", "dboxes"):
        assert _rel(me[k], torch.from_numpy(z[k])) < 1e-12, k
    # margin: the second-best assignment of every image costs visibly more than the best (the device's f32 cost cannot flip it)
    for b, n in enumerate(case["counts"]):
        c = me["cost"][b]
        best = float(c[me["pi"][b], me["ti"][b]].sum())
        for k in range(n):
            alt = c.clone()
            alt[me["pi"][b][k], me["ti"][b][k]] = 1e6
            i, j, _ = R.decide(alt.numpy(), case["labels"][b], 5)
            assert float(c[i, j].sum()) - best > 0.05


def test_the_builders_do_what_they_claim():
    u = R.make_logits("uniform", 2, 36, 7, 0)
    assert float(u.abs().max()) <= 8.0 and float(u.min()) < -6 and float(u.max()) > 6
    s = R.make_logits("saturated", 2, 36, 7, 0)
    assert {40.0, -40.0, 100.0, -100.0} <= set(s.unique().tolist())
    assert float(R.make_logits("zero", 1, 4, 3, 0).abs().max()) == 0.0
    t = R.make_logits("tiny", 2, 36, 7, 0)
    assert float(t.abs().max()) <= 1.01e-7 and bool((t.abs() < 2.0 ** -126).any()) and bool((t != 0).all())
    m = R.make_logits("mixed", 3, 36, 9, 0)
    assert bool((m == 0).any()) and bool((m.abs() >= 40).any()) and bool(((m.abs() > 0) & (m.abs() < 1e-6)).any())
    seen_q, seen_p, seen_b, kinds, fills = set(), set(), set(), set(), set()
    for name, kw in R.GPU_CASES.items():
        c = R.gpu_case(name)
        B, P, Q = c["logits"].shape
        seen_q.add(Q); seen_p.add(P); seen_b.add(B); kinds.add(kw["mask_kind"]); fills.add("nan" if kw["fill"] != kw["fill"] else "fmin")
        live = R._live(c["mask"], B, P, Q)
        assert bool(torch.isfinite(c["logits"][live]).all())
        if c["mask"] is not None:
            dead = c["logits"][~live]
            assert dead.numel() > 0 and bool(torch.isnan(dead).all() if kw["fill"] != kw["fill"] else (dead == R.FMIN).all())
        for b in range(B):
            n = c["counts"][b]
            assert c["labels"][b].shape == (n,) and c["tgt"][b].shape == (n, 4)
            if n:
                row = None if c["mask"] is None else c["mask"][b if c["mask"].shape[0] == B else 0]
                assert bool(R.label_ok(c["labels"][b], row, Q).all())
                assert bool((c["tgt"][b][:, 2:] > c["tgt"][b][:, :2]).all())
                # every fourth target shares x0 and y1 with some prediction exactly (max / min ties)
                assert bool((c["tgt"][b][0, 0] == c["boxes"][b][:, 0]).any()) and bool((c["tgt"][b][0, 3] == c["boxes"][b][:, 3]).any())
    assert seen_q >= {1, 3, 31, 32, 33, 70, 260} and seen_p == {4, 36, 576} and seen_b == {1, 3, 5}
    assert kinds == {None, "shared", "per_image"} and fills == {"nan", "fmin"}
    counts = [n for kw in R.GPU_CASES.values() for n in kw["counts"]]
    assert 0 in counts and 1 in counts and R.GPU_CASES["p4_full"]["counts"] == [4] and R.GPU_CASES["p4_full"]["P"] == 4
    # the class kernel's workgroup count: one chunk each up to the cap, several at "stride" alone
    kw = R.GPU_CASES["stride"]
    assert kw["B"] * kw["P"] * kw["Q"] > R.CHUNK * R.MAX_PARTS and R.n_parts(kw["B"], kw["P"], kw["Q"]) == R.MAX_PARTS
    assert all(R.n_parts(k["B"], k["P"], k["Q"]) < R.MAX_PARTS for n_, k in R.GPU_CASES.items() if n_ != "stride")
    assert R.n_parts(5, 576, 260) > 1 and R.n_parts(1, 4, 3) == 1


def _emulate_class(logits, tc, live, alpha=0.25):
    """ovl_focal in torch f32 ops, one op per written operation."""
    Q = logits.shape[1]
    x = torch.where(live, logits, torch.zeros_like(logits))
    t = tc[:, None] == torch.arange(Q)[None, :]
    one = torch.ones_like(x)
    z = torch.where(t, -x, x)
    e = torch.exp(-z.abs())
    d = 1.0 + e
    sp = z.clamp(min=0.0) + torch.log1p(e)
    nn = z >= 0
    s = torch.where(nn, one, e) / d
    m = s * s
    at = torch.where(t, torch.tensor(alpha), torch.tensor(1.0) - torch.tensor(alpha))
    v = at * (sp * m)
    c = torch.where(nn, e, one) / d
    gz = at * (m * ((2.0 * c) * sp + s))
    gz = torch.where(t, -gz, gz)
    zero = torch.zeros_like(x)
    return torch.where(live, v, zero), torch.where(live, gz, zero)


def _emulate_cost(logits, boxes, labels, tgt):
    x = logits[:, labels]
    pr = 1.0 / (1.0 + torch.exp(-x))
    om = 1.0 - pr
    eps = torch.tensor(1e-8, dtype=torch.float32)
    pos = (0.25 * (om * om)) * (-torch.log(pr + eps))
    neg = (0.75 * (pr * pr)) * (-torch.log(om + eps))
    a, t = boxes[:, None, :], tgt[None, :, :]
    ctr = lambda b: ((b[..., 0] + b[..., 2]) * 0.5, (b[..., 1] + b[..., 3]) * 0.5, b[..., 2] - b[..., 0], b[..., 3] - b[..., 1])          # noqa: E731
    ca, ct = ctr(a), ctr(t)
    l1 = (((ca[0] - ct[0]).abs() + (ca[1] - ct[1]).abs()) + (ca[2] - ct[2]).abs()) + (ca[3] - ct[3]).abs()
    g = R.giou(a, t)
    return (5.0 * l1 + 1.0 * (pos - neg)) + 2.0 * (-g)


@pytest.mark.parametrize("name", ["p4_full", "q31_empty", "q32_sat_nan", "q70_tiny"])
def test_an_f32_evaluation_of_the_kernels_sequence_is_inside_the_bounds(name):
    case = R.gpu_case(name)
    B, P, Q = case["logits"].shape
    tcs, pi, ti = R.oracle_decisions(case)
    live = R._live(case["mask"], B, P, Q).reshape(B * P, Q)
    cs = R.class_stage(case["logits"].reshape(B * P, Q), tcs.reshape(-1), live)
    v, gz = _emulate_class(case["logits"].reshape(B * P, Q), tcs.reshape(-1), live)
    worst = R.check("element", v, cs["el"][0], R.tol_of(cs["el"][1], cs["el"][0]))
    worst_g = R.check("d element", gz, cs["del_"][0], R.tol_of(cs["del_"][1], cs["del_"][0]))
    assert 0 < max(worst, worst_g) <= 1.0 or float(case["logits"].abs().max()) == 0
    if case["mask"] is None:
        for b in range(B):
            st = R.cost_stage(case["logits"][b], case["boxes"][b], case["labels"][b], case["tgt"][b])
            R.check("cost", _emulate_cost(case["logits"][b], case["boxes"][b], case["labels"][b], case["tgt"][b]), st["ref"], st["tol"])


def test_the_cost_bound_is_wide_only_where_hf_cancels():
    """1 - sigmoid(x) + 1e-8 at x = 17: the f32 difference is one or two ulps of 1 against a true 4e-8 -- the bound there is of order 1, as it must be;
    at |x| <= 8 it stays below 1e-3, and at x >= 40, where both evaluations give exactly 1e-8, it is tight again."""
    boxes = torch.tensor([[0.1, 0.1, 0.4, 0.5]])
    tgt = torch.tensor([[0.12, 0.1, 0.41, 0.52]])
    lab = torch.tensor([0])
    tol = {x: float(R.cost_stage(torch.tensor([[x]]), boxes, lab, tgt)["tol"]) for x in (-8.0, 0.0, 8.0, 17.0, 40.0)}
    assert max(tol[-8.0], tol[0.0], tol[8.0]) < 1e-3 and tol[17.0] > 0.1 and tol[40.0] < 1e-4, tol


def _bounds(name):
    if name not in _crit_cache:
        case = R.gpu_case(name)
        dec = R.oracle_decisions(case)
        nb = float(max(1, sum(case["counts"])))
        B = case["logits"].shape[0]
        costs = {}
        for b in range(B):
            row = None if case["mask"] is None else case["mask"][b if case["mask"].shape[0] == B else 0]
            costs[b] = R.cost_stage(case["logits"][b], case["boxes"][b], case["labels"][b], case["tgt"][b], row)
        _crit_cache[name] = (case, dec, nb, R.criterion(case["logits"], case["boxes"], case["mask"], *dec, case["tgt"], 0.25, nb, G3), costs)
    return _crit_cache[name]


@pytest.mark.parametrize("variant", R.PLANTED)
def test_planted_errors_fall_outside_the_bounds(variant):
    caught = []
    for name in ("q31_empty", "q32_sat_nan", "p4_full", "q33_nan"):
        case, dec, nb, crit, costs = _bounds(name)
        for key, wrong in R.planted(case, variant, dec, nb, G3).items():
            ref, tol = (costs[key[1]]["ref"], costs[key[1]]["tol"]) if isinstance(key, tuple) else crit[key]
            if float(R.ratios(wrong, ref, tol).max()) > 1.0:
                caught.append(name)
        if caught:
            break
    assert caught, variant
    # and the formula itself passes its own bounds (the check can tell right from wrong)
    case, dec, nb, crit, _ = _bounds("q31_empty")
    B, P, Q = case["logits"].shape
    ld = torch.where(R._live(case["mask"], B, P, Q), case["logits"].double(), torch.zeros(B, P, Q, dtype=torch.float64))
    right = torch.stack(R.loss_double(ld, case["boxes"].double(), case["mask"], *dec, case["tgt"], 0.25, nb))
    assert float(R.ratios(right, *crit["losses"]).max()) <= 1.0


def test_the_bounds_are_tight_where_nothing_cancels():
    case, dec, nb, crit, costs = _bounds("q31_empty")
    ref, tol = crit["losses"]
    assert bool((tol / ref.abs() < 1e-5).all()), (tol / ref.abs()).tolist()
    ref, tol = crit["dlogits"]
    assert float((tol / ref.abs().clamp(min=1e-30)).median()) < 1e-5
    ref, tol = crit["dboxes"]
    assert float(tol[ref == 0].max()) < 1e-40                         # unmatched rows: exact zeros


# ---- the Python surface (host tensors: nothing below launches a kernel) ------------------------------------------------------------------------------
def _targets(labels, n_boxes=None):
    return [{"class_labels": torch.tensor(l, dtype=torch.int64), "boxes": torch.rand(len(l), 4) * 0.3 + torch.tensor([0.0, 0.0, 0.4, 0.4])} for l in labels]


def test_surface_errors():
    from owl_vit_object_detection_amd.losses import OpenVocabLoss
    from owl_vit_object_detection_amd.matcher import OpenVocabMatcher, pack_open_vocab_targets
    crit = OpenVocabLoss()
    logits, boxes = torch.zeros(2, 4, 5), torch.rand(2, 4, 4)
    with pytest.raises(IndexError, match=r"outside \[0, 5\)"):
        crit(logits, boxes, _targets([[0, 5], [1]]))
    with pytest.raises(IndexError, match=r"outside \[0, 5\)"):
        crit(logits, boxes, _targets([[-1], [1]]))
    mask = torch.ones(2, 5, dtype=torch.bool)
    mask[1, 3:] = False
    with pytest.raises(IndexError, match="masked query"):
        crit(logits, boxes, _targets([[4], [3]]), query_mask=mask)
    with pytest.raises(ValueError, match="more targets than predictions"):
        crit(logits, boxes, _targets([[0, 1, 2, 3, 4], [1]]))
    with pytest.raises(ValueError, match="batch size mismatch"):
        crit(logits, boxes, _targets([[0]]))
    with pytest.raises(ValueError, match="query_mask must be"):
        crit(logits, boxes, _targets([[0], [1]]), query_mask=torch.ones(3, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match="num_boxes must be positive"):
        crit(logits, boxes, _targets([[0], [1]]), num_boxes=0)
    with pytest.raises(ValueError, match="box_format"):
        OpenVocabLoss(box_format="xywh")
    with pytest.raises(ValueError, match="box_format"):
        pack_open_vocab_targets(_targets([[0]]), "cpu", 5, None, "xywh")
    with pytest.raises(ValueError, match="gamma is 2"):
        OpenVocabLoss(gamma=1.5)
    with pytest.raises(ValueError, match="all costs"):
        OpenVocabMatcher(0, 0, 0)
    # cxcywh targets are converted once at packing; "labels" is accepted for "class_labels"
    t = [{"labels": torch.tensor([2]), "boxes": torch.tensor([[0.5, 0.5, 0.2, 0.4]])}]
    tg = pack_open_vocab_targets(t, "cpu", 5, None, "cxcywh")
    assert torch.allclose(tg.boxes[0, 0], torch.tensor([0.4, 0.3, 0.6, 0.7])) and tg.labels.tolist() == [[2]]
    assert torch.equal(pack_open_vocab_targets(t, "cpu", 5).boxes[0, 0], t[0]["boxes"][0])


def test_allow_empty():
    from owl_vit_object_detection_amd.matcher import PackedTargets, pack_open_vocab_targets
    lab = [torch.tensor([1, 2]), torch.zeros(0, dtype=torch.int64)]
    box = [torch.rand(2, 4), torch.zeros(0, 4)]
    with pytest.raises(ValueError, match="at least one target box"):
        PackedTargets(lab, box, "cpu")
    tg = PackedTargets(lab, box, "cpu", allow_empty=True)
    assert tg.sizes == [2, 0] and tg.Nmax == 2 and tg.counts.tolist() == [2, 0] and float(tg.boxes[1].abs().max()) == 0
    none = PackedTargets([lab[1], lab[1]], [box[1], box[1]], "cpu", allow_empty=True)
    assert none.Nmax == 1 and none.labels.shape == (2, 1) and none.counts.tolist() == [0, 0]
    # the default keeps today's packing
    full = PackedTargets([lab[0]], [box[0]], "cpu")
    assert full.Nmax == 2 and torch.equal(full.boxes[0], box[0])
    tg2 = pack_open_vocab_targets([{"class_labels": lab[1], "boxes": box[1]}], "cpu", 3)
    assert tg2.sizes == [0] and tg2.Nmax == 1
