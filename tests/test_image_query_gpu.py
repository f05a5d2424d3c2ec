"""-m gpu: the query bank from image exemplars on a real MI355X.

* owl_image_query_select (csrc/image_query.hip) against the float64 restatement of HF's `embed_image_query` inside the bounds derived in
  tests/image_query_reference.py (no fitted tolerance), the profiles spread over the shapes of R.GPU_CASES; nothing written past an output; two runs
  bitwise equal.  Each case prints its worst err / tol; profiles/image_queries_reference.md records them.
* owl_query_bank_fill against float64: rows with 1, 2 and 5 members, untouched rows and a sentinel row bitwise.
* the model level on `tiny` and `tiny-l14`: embed_image_query against the oracle, the closed form of an exemplar-initialised class, the rows of
  classes without exemplars, one optimizer step, and two constructions giving the same bits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import owl_oracle as O  # noqa: E402  (checker only)
from owl_vit_object_detection_amd import _lib, models, ops, synth, weights  # noqa: E402
from owl_vit_object_detection_amd.config import get_config  # noqa: E402
from owl_vit_object_detection_amd.losses import PushPullLoss  # noqa: E402
from owl_vit_object_detection_amd.models import OwlViT, load_model  # noqa: E402
from owl_vit_object_detection_amd.optim import FusedAdamW  # noqa: E402
from tests import heads_reference as H  # noqa: E402
from tests import image_query_reference as R  # noqa: E402

DEV = "cuda"
NAN = float("nan")
E_E, E_BOX = 4e-3, 2e-3          # the output tolerances of the bf16 forward: e-scale quantities (relative to an exemplar's largest |e|), boxes (absolute)


def _run_select(e, boxes, qbox, N, P, Dt):
    """The raw entry with ONE sentinel row past every output."""
    e_d, b_d, q_d = e.to(DEV), boxes.to(DEV), (None if qbox is None else qbox.to(DEV))
    ws = torch.empty(ops.image_query_workspace_bytes(N, P, Dt), dtype=torch.uint8, device=DEV)
    best = torch.full((N + 1,), -77, dtype=torch.int32, device=DEV)
    info = torch.full((N + 1, 2), -77, dtype=torch.int32, device=DEV)
    query = torch.full((N + 1, Dt), NAN, device=DEV)
    v = torch.full((N + 1, P), NAN, device=DEV)
    mean = torch.full((N + 1, Dt), NAN, dtype=torch.float64, device=DEV)
    sim = torch.full((N + 1, P), NAN, dtype=torch.float64, device=DEV)
    _lib.call("owl_image_query_select", ops.stream(), e_d, b_d, q_d, N, P, Dt, ws, ws.numel(), best, query, info, v, mean, sim)
    torch.cuda.synchronize()
    assert int(best[N]) == -77 and bool((info[N] == -77).all())
    assert bool(torch.isnan(query[N]).all()) and bool(torch.isnan(v[N]).all()) and bool(torch.isnan(mean[N]).all()) and bool(torch.isnan(sim[N]).all())
    return dict(best=best[:N].cpu(), info=info[:N].cpu(), query=query[:N].cpu(), v=v[:N].cpu(), mean=mean[:N].cpu(), sim=sim[:N].cpu())


@pytest.mark.parametrize("N,P,Dt,profile", R.GPU_CASES)
def test_select_against_float64(N, P, Dt, profile):
    e, boxes, qbox = R.make_case(profile, N, P, Dt)
    a, b = _run_select(e, boxes, qbox, N, P, Dt), _run_select(e, boxes, qbox, N, P, Dt)
    for k in a:          # bitwise reproducible (NaN-free outputs; +inf compares equal)
        assert torch.equal(a[k], b[k]), k
    fails, worst, undecided = [], dict(v=0.0, mean=0.0, sim=0.0), 0
    for n in range(N):
        ref = R.exact_select(e[n], boxes[n], qbox[n])
        out = dict(best=int(a["best"][n]), query=a["query"][n], flags=int(a["info"][n, 0]), nsel=int(a["info"][n, 1]), v=a["v"][n], mean=a["mean"][n], sim=a["sim"][n])
        r = R.check_select(f"{profile} ({N}, {P}, {Dt}) exemplar {n}", out, ref, e[n], fails)
        worst = {k: max(worst[k], r[k]) for k in worst}
        undecided += not ref["decided"]
        if profile == "touching":          # facts of exact arithmetic, whatever the bounds leave open
            assert out["best"] == P // 3 and out["nsel"] == 1 and out["flags"] == R.FLAG_FALLBACK and float(out["v"][P // 3]) == 0.0
        if profile == "disjoint":
            assert out["best"] == -1 and out["nsel"] == 0 and out["flags"] == (R.FLAG_FALLBACK | R.FLAG_EMPTY) and not bool(out["query"].any())
        if profile == "ties":
            assert out["nsel"] == P and (P == 1 or out["best"] % 2 == 0)
    print(f"image_query_select {profile} N={N} P={P} Dt={Dt}: err / tol v {worst['v']:.3f} mean {worst['mean']:.3f} sim {worst['sim']:.3f}; "
          f"{undecided} of {N} exemplars left to the bounds")
    assert not fails, "\n".join(fails[:8])
    if profile in R.UNDECIDED_CAP:
        assert undecided <= R.UNDECIDED_CAP[profile] * N


def test_null_query_box_is_the_whole_image_and_the_wrapper_is_the_entry():
    N, P, Dt = 3, 36, 64
    e, boxes, _ = R.make_case("randn", N, P, Dt, seed=5)
    whole = torch.tensor(R.WHOLE).repeat(N, 1)
    a, b = _run_select(e, boxes, None, N, P, Dt), _run_select(e, boxes, whole, N, P, Dt)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    best, query, info, v, mean, sim = ops.image_query_select(e.to(DEV), boxes.to(DEV), None, N, P, Dt, diagnostics=True)
    for k, t in dict(best=best, query=query, info=info, v=v, mean=mean, sim=sim).items():
        assert torch.equal(t.cpu(), a[k]), k
    best2, query2, info2 = ops.image_query_select(e.to(DEV), boxes.to(DEV), None, N, P, Dt)          # the diagnostics are optional: same decisions without them
    assert torch.equal(best2.cpu(), a["best"]) and torch.equal(query2.cpu(), a["query"]) and torch.equal(info2.cpu(), a["info"])


@pytest.mark.parametrize("N,Dt", [(6, 64), (7, 512), (5, 768)])
def test_bank_fill_against_float64(N, Dt):
    g = torch.Generator().manual_seed(N + Dt)
    query = torch.randn(N, Dt, generator=g) * torch.logspace(-3, 3, N)[:, None]          # norms over six decades: unit() must not care
    table = [[2], [], [0, 3], [0, 1, 2, 3, 4], [], [N - 1], []]
    nq = len(table)
    old = torch.randn(nq + 1, Dt, generator=g)
    old[nq] = NAN          # the sentinel row
    row_ptr, members = models.slots_csr(table)
    runs = []
    for _ in range(2):
        bank = old.to(DEV)
        ops.query_bank_fill(query.to(DEV), torch.from_numpy(row_ptr).to(DEV), torch.from_numpy(members).to(DEV), bank, N, nq, Dt)
        torch.cuda.synchronize()
        runs.append(bank.cpu())
    bank = runs[0]
    assert torch.equal(H.bits(runs[0]), H.bits(runs[1]))
    for r, mem in enumerate(table + [[]]):
        if not mem:
            assert torch.equal(H.bits(bank[r]), H.bits(old[r])), f"row {r} has no members and changed"
    ref, tol = R.exact_bank(query, table, old[:nq])
    live = [r for r, m in enumerate(table) if m]
    worst = R.check(f"bank fill N={N} Dt={Dt}", bank[live], ref[live], tol[live])
    print(f"query_bank_fill N={N} Dt={Dt}: err / tol {worst:.3f}")
    assert torch.allclose(torch.linalg.norm(bank[live].double(), dim=-1), torch.ones(len(live), dtype=torch.float64), atol=1e-6)


# ---- the model level ------------------------------------------------------------------------------------------------------------------------
QBOXES = [None, (0.1, 0.2, 0.5, 0.7), (0.4, 0.3, 0.9, 0.9), (0.25, 0.05, 0.75, 0.45)]
IMG_SEED = 77
# (image index of synth.make_images(seed = 77), query box): picked on the CPU so that the oracle decides at least 6 of the 8 under (E_E, E_BOX)
EXEMPLARS = {"tiny": [(3, 3), (5, 3), (38, 2), (6, 2), (7, 1), (14, 0), (26, 0), (0, 0)],
             "tiny-l14": [(0, 3), (1, 0), (29, 0), (2, 2), (9, 0), (16, 0), (7, 0), (3, 0)]}


def _exemplar_batch(cfg, cname):
    img = np.concatenate([synth.make_images(cfg, 1, seed=IMG_SEED, first=i) for i, _ in EXEMPLARS[cname]])
    qb = torch.tensor([R.WHOLE if QBOXES[q] is None else QBOXES[q] for _, q in EXEMPLARS[cname]])
    return torch.from_numpy(img), qb


@pytest.mark.parametrize("cname", ["tiny", "tiny-l14"])
def test_embed_image_query_against_oracle(cname):
    cfg = get_config(cname)
    Wnp = weights.make_weights(cfg)
    img, qb = _exemplar_batch(cfg, cname)
    N, P = img.shape[0], cfg.patches
    w = {k: torch.from_numpy(v) for k, v in Wnp.items()}
    taps = {}
    rb, _ = O.model_forward(cfg, w, img, taps)
    e64 = F.linear(taps["feats"].double(), w["class_predictor.dense0.weight"].double(), w["class_predictor.dense0.bias"].double()).view(N, P, -1)
    scale = [float(e64[n].abs().max()) for n in range(N)]
    refs = [R.exact_select(e64[n], rb[n].double(), qb[n], E_e=E_E * scale[n], E_box=E_BOX) for n in range(N)]
    decided = [n for n in range(N) if refs[n]["decided"]]
    assert len(decided) >= 6, f"the oracle decides only {decided} under the bf16 tolerances: pick other exemplars"

    model = OwlViT(cfg, Wnp, DEV)
    query, idx, boxes = model.embed_image_query(img.to(DEV), qb)          # (query boxes on the host: any device is taken)
    e_ws = model._workspace(N, train=False)["e"][:N * P].view(N, P, -1).clone()
    torch.cuda.synchronize()
    assert query.shape == (N, cfg.text_dim) and query.dtype == torch.float32 and idx.shape == (N,) and idx.dtype == torch.int64 and boxes.shape == (N, P, 4)
    eb = float((boxes.cpu() - rb).abs().max())
    ee = max(float((e_ws[n].cpu().double() - e64[n]).abs().max()) / scale[n] for n in range(N))
    print(f"{cname}: oracle decides {len(decided)} of {N}; max |d boxes| {eb:.3e} (compared under {E_BOX}), max |d e| / max |e| {ee:.3e} (compared under {E_E})")
    # (printed, not asserted: E_E / E_BOX are the tolerances the decisions are compared under, as set for this test; the forward's own error is held
    #  by tests/test_model_gpu.py.  Measured on an MI355X: boxes 1.7e-3, e 5.8e-3 of its scale on `tiny` -- the e figure is ABOVE E_E, so a decision this
    #  test calls decided could in principle flip; none of the asserted ones does, and the kernel-level check below does not depend on either figure)
    for n in decided:
        assert int(idx[n]) == refs[n]["best"], (n, int(idx[n]), refs[n]["best"], refs[n]["margin_best"])
    for n in range(N):
        assert int(idx[n]) >= 0 and torch.equal(query[n], e_ws[n, int(idx[n])])
        kern = R.exact_select(e_ws[n].cpu(), boxes[n].cpu(), qb[n])          # and on the device's own e and boxes: the kernel-level check
        if kern["decided"]:
            assert int(idx[n]) == kern["best"]
    # None = the whole image, HF's rule; and the forward left behind is the plain eval forward's
    q2, i2, b2 = model.embed_image_query(img.to(DEV))
    whole = model.embed_image_query(img.to(DEV), torch.tensor(R.WHOLE).repeat(N, 1).to(DEV))
    assert torch.equal(q2, whole[0]) and torch.equal(i2, whole[1]) and torch.equal(b2, whole[2])
    with torch.no_grad():
        pb = model(img.to(DEV))[0]
    assert torch.equal(pb, b2)


def test_embed_image_query_chunks_and_leaves_a_pending_backward_alone():
    """More than 32 images: two chunks, the same bits as the images one by one chunk; a training forward's backward still runs afterwards."""
    cfg = get_config("tiny")
    model = OwlViT(cfg, weights.make_weights(cfg), DEV)
    img = torch.from_numpy(synth.make_images(cfg, 35, seed=IMG_SEED)).to(DEV)
    pb, _, ps, _ = model(img[:2])          # a recording forward whose backward is still pending
    q, i, b = model.embed_image_query(img)
    q0, i0, b0 = model.embed_image_query(img[:32])
    q1, i1, b1 = model.embed_image_query(img[32:])
    assert torch.equal(q, torch.cat([q0, q1])) and torch.equal(i, torch.cat([i0, i1])) and torch.equal(b, torch.cat([b0, b1]))
    (pb.sum() + ps.sum()).backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(model.p("queries").grad).all())


def _labelmap(C):
    return {i: f"class{i}" for i in range(C)}


def test_closed_form_of_an_exemplar_initialised_class():
    """One exemplar for one class: its three rows are unit(e_best), so on the exemplar's own image pred_sims[best, c] = e^ . (e^ + 1e-6) inside the
    class head's bound (tests/heads_reference.py) plus what the bank's single f32 rounding and its renormalisation move qhat by."""
    cfg = get_config("tiny")
    img = torch.from_numpy(synth.make_images(cfg, 1, seed=IMG_SEED, first=10)).to(DEV)
    qb = torch.tensor([QBOXES[3]])
    c = 2
    model = load_model(_labelmap(cfg.n_classes), DEV, arch="tiny", exemplars=(img, [c], qb))
    with torch.no_grad():
        _, _, sims, _ = model(img)
    ws = model._workspace(1, train=False)
    e = ws["e"][:cfg.patches].clone()
    _, idx, _ = model.embed_image_query(img, qb)
    torch.cuda.synchronize()
    best = int(idx[0])
    ex = H.exact_sims(e, ws["qhat"], cfg.n_classes)
    tol = H.bounds_sims(ex)["sims"]
    H.check("sims on the given table", sims[0], ex["sims"], tol)
    eb = e[best].double()
    unit = eb / torch.linalg.norm(eb)
    closed = float((eb / (torch.linalg.norm(eb) + H.EPS6)) @ (unit + H.EPS6))
    bank = model.p("queries").detach().view(cfg.queries, -1)
    E_q = H.bounds_qhat(H.exact_qhat(bank))["qhat"][3 * c] + ((1 + R.F) / (1 - R.F) - 1) * unit.abs()
    allowed = float(tol[best, c]) + float((eb.abs() / torch.linalg.norm(eb)) @ E_q)
    got = float(sims[0, best, c])
    print(f"closed form: pred_sims[best = {best}, {c}] = {got:.9f}, e^ . (e^ + 1e-6) = {closed:.9f}, |diff| {abs(got - closed):.3e} (allowed {allowed:.3e})")
    assert abs(got - closed) <= allowed
    assert torch.equal(bank[3 * c], bank[3 * c + 1]) and torch.equal(bank[3 * c], bank[3 * c + 2])


def test_classes_without_exemplars_keep_their_rows_and_none_changes_nothing():
    cfg = get_config("tiny")
    lm = _labelmap(cfg.n_classes)
    img = torch.from_numpy(synth.make_images(cfg, 3, seed=IMG_SEED, first=6)).to(DEV)
    plain = load_model(lm, DEV, arch="tiny")
    a = load_model(lm, DEV, arch="tiny", exemplars=(img, [1, 3, 1]))
    b = load_model(lm, DEV, arch="tiny", exemplars=(img, torch.tensor([1, 3, 1]), None))
    qa, qb_, q0 = (m.p("queries").detach().view(cfg.queries, -1) for m in (a, b, plain))
    assert torch.equal(H.bits(qa), H.bits(qb_))          # two constructions: the same bits
    for cls in (0, 2):
        assert torch.equal(H.bits(qa[3 * cls:3 * cls + 3]), H.bits(q0[3 * cls:3 * cls + 3]))
    for cls in (1, 3):
        assert not torch.equal(qa[3 * cls:3 * cls + 3], q0[3 * cls:3 * cls + 3])
        assert torch.allclose(torch.linalg.norm(qa[3 * cls:3 * cls + 3].double().cpu(), dim=-1), torch.ones(3, dtype=torch.float64), atol=1e-6)
    assert torch.equal(qa[3], qa[5]) and not torch.equal(qa[3], qa[4])          # class 1 has two exemplars: slots (0), (1), (0 again)
    # every other parameter is untouched, and exemplars=None is the plain constructor's model, bit for bit
    for (n, p), (_, p0) in zip(a.named_parameters(), plain.named_parameters()):
        if n != "queries":
            assert torch.equal(p, p0), n
    direct = OwlViT(get_config("tiny", n_classes=len(lm)), weights.make_weights(get_config("tiny", n_classes=len(lm)), 1234), DEV)
    with torch.no_grad():
        (b0, _, s0, _), (b1, _, s1, _) = plain(img), direct(img)
    assert torch.equal(b0, b1) and torch.equal(s0, s1)
    info = a.set_queries_from_exemplars(img, [1, 3, 1])          # an existing model: the same rows again, and the report
    assert torch.equal(H.bits(a.p("queries").detach().view(cfg.queries, -1)), H.bits(qb_))
    assert info["slots"][3:6] == [[0], [2], [0]] and info["slots"][9:12] == [[1], [1], [1]] and len(info["box_indices"]) == 3
    assert all(n >= 1 for n in info["n_selected"]) and info["fallback"] == [False] * 3


def test_errors_on_the_device():
    cfg = get_config("tiny")
    model = load_model(_labelmap(cfg.n_classes), DEV, arch="tiny")
    img = torch.from_numpy(synth.make_images(cfg, 2, seed=IMG_SEED)).to(DEV)
    before = model.p("queries").detach().clone()
    with pytest.raises(ValueError, match=r"query_boxes must be \[2, 4\]"):
        model.embed_image_query(img, torch.zeros(3, 4))
    opt = FusedAdamW(model, lr=1e-4, ema_decay=0.9)
    with opt.ema_weights():
        with pytest.raises(RuntimeError, match="ema_weights"):
            model.set_queries_from_exemplars(img, [0, 1])
    assert torch.equal(model.p("queries").detach(), before)
    with pytest.raises(ValueError, match="exemplars= is"):
        load_model(_labelmap(cfg.n_classes), DEV, arch="tiny", exemplars=(img,))


def test_one_optimizer_step_on_an_exemplar_initialised_model():
    cfg = get_config("tiny")
    B = 2
    img = torch.from_numpy(synth.make_images(cfg, B, seed=IMG_SEED, first=6)).to(DEV)
    labels, boxes = synth.make_targets(cfg, B, max_boxes=6)
    model = load_model(_labelmap(cfg.n_classes), DEV, arch="tiny", exemplars=(img, [0, 2]))
    crit = PushPullLoss(cfg.n_classes, synth.class_scales(cfg, labels))
    opt = FusedAdamW(model, lr=3e-6, weight_decay=0.1)
    opt.zero_grad()
    pb, _, ps, _ = model(img)
    losses = crit(ps, [torch.from_numpy(x).to(DEV) for x in labels], pb, [torch.from_numpy(x).to(DEV) for x in boxes])
    (losses["loss_ce"] + losses["loss_bg"] + losses["loss_bbox"] + losses["loss_giou"]).backward()
    g = model.p("queries").grad.detach().clone()
    before = model.p("queries").detach().clone()
    opt.step()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert bool(torch.isfinite(model.flat_param).all()) and not torch.equal(model.p("queries").detach(), before)
