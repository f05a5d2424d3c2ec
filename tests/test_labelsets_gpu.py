"""Label sets beyond 10 classes on a real MI355X: the wide class head (csrc/class_head_wide.hip) against float64, bit for bit against the narrow
kernels on every 10-class block, the model against the reference fixture f11_tiny_c80 (tiny config, 80 classes), and the public surface."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import owl_oracle as O  # noqa: E402  (checker only)
from owl_vit_object_detection_amd import ops, synth, weights  # noqa: E402
from owl_vit_object_detection_amd.config import get_config  # noqa: E402
from owl_vit_object_detection_amd.losses import PushPullLoss  # noqa: E402
from owl_vit_object_detection_amd.models import OwlViT, load_model  # noqa: E402

DEV = "cuda"
LOSS_KEYS = ("loss_ce", "loss_bg", "loss_bbox", "loss_giou")
KERNEL_SHAPES = [(rows, Dt, C) for rows in (37, 300) for Dt, C in ((64, 11), (192, 20), (512, 80), (768, 91), (512, 384))]


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def report(name, got, ref, atol, rtol):
    got = got.double(); ref = ref.double()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    print(f"   {name}: max err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e})")
    if bad.any():
        raise AssertionError(f"{name}: {int(bad.sum())}/{bad.numel()} off; max err {float(err.max()):.4g} (ref max {float(ref.abs().max()):.4g}); "
                             f"first bad idx {bad.nonzero()[:8].tolist()}; got {got[bad][:4].tolist()} ref {ref[bad][:4].tolist()}")


def _s_all64(e, Q):
    """The class head's expression (ref src/models.py:24-38) in float64: [rows, 3C] cosines before the max over prompts."""
    qh = Q.double() / torch.linalg.norm(Q.double(), dim=-1, keepdim=True) + 1e-6
    return (e.double() / (torch.linalg.norm(e.double(), dim=-1, keepdim=True) + 1e-6)) @ qh.t()


def _draw(rows, Dt, C):
    """e [rows, Dt], Q [3C, Dt] such that no prompt triple's top two are within 1e-4 in float64: rows that hold such a triple are drawn again."""
    e = rnd(rows, Dt, scale=0.7, seed=1)
    Q = rnd(3 * C, Dt, seed=4)
    for it in range(400):
        top2 = _s_all64(e, Q).view(rows, C, 3).topk(2, dim=-1).values
        tied = ((top2[..., 0] - top2[..., 1]) < 1e-4).any(dim=1)
        if not bool(tied.any()):
            break
        idx = tied.nonzero().flatten()
        e[idx] = rnd(int(idx.numel()), Dt, scale=0.7, seed=1000 + it)
    top2 = _s_all64(e, Q).view(rows, C, 3).topk(2, dim=-1).values
    assert float((top2[..., 0] - top2[..., 1]).min()) >= 1e-4, "a prompt triple ties within 1e-4 in the float64 reference"
    return e, Q


def _to_wide_rows(C):
    """bank row j = 3 c + p -> row 32 (c / 10) + 3 (c % 10) + p of the wide layout"""
    j = torch.arange(3 * C, device=DEV)
    return 32 * (j // 30) + j % 30


def _wide_forward(e, Q, rows, Dt, C, fill=7.0):
    nb, Qp = ops.wide_blocks(C), ops.wide_qp(C)
    qhat = torch.full((32 * nb, Dt), fill, device=DEV); qn = torch.full((32 * nb,), fill, device=DEV)
    ops.query_normalize_wide(Q, qhat, qn, 3 * C, Dt)
    sims = torch.full((rows, C), fill, device=DEV); am = torch.full((rows, C), 7, dtype=torch.uint8, device=DEV); inv = torch.full((rows,), fill, device=DEV)
    ops.class_sims_wide(e, qhat, sims, am, inv, rows, Dt, C)
    return qhat, qn, sims, am, inv, nb, Qp


@pytest.mark.parametrize("rows,Dt,C", KERNEL_SHAPES)
def test_wide_class_head_kernels_match_float64(rows, Dt, C):
    """owl_query_normalize_wide, owl_class_sims_wide_fwd, owl_class_sims_wide_bwd and owl_query_normalize_wide_bwd against the torch expressions of
    test_class_sims_forward_backward_match_torch_autograd evaluated in float64.  Bands are the narrow tests' (sims 2e-5 / 1e-4, de 2e-3 max / 8e-3,
    dqhat 2e-2 max / 2e-2); every output buffer starts at 7.0 so that an unwritten element shows; the backward run twice gives equal bits.
    Shapes: 37 / 300 rows = a partial wave / a partial workgroup; C = 11: a second tile with one class; 20: two full tiles; 91: a last tile with one
    class; Dt = 64 / 192: a half-chunk past Dt; C = 384: the ceiling (a second 256-column chunk of G, with pad columns)."""
    e, Q = _draw(rows, Dt, C)
    qhat, qn, sims, am, inv, nb, Qp = _wide_forward(e, Q, rows, Dt, C)
    wr = _to_wide_rows(C)
    # ---- forward
    Qr = Q.double().requires_grad_(True)
    er = e.double().requires_grad_(True)
    qh = Qr / torch.linalg.norm(Qr, dim=-1, keepdim=True) + 1e-6
    qh.retain_grad()
    s_all = (er / (torch.linalg.norm(er, dim=-1, keepdim=True) + 1e-6)) @ qh.t()
    ref = F.max_pool1d(s_all[None], 3, 3)[0]
    report("qhat", qhat[wr], qh.detach(), 1e-6, 1e-5)
    pad = torch.ones(32 * nb, dtype=torch.bool, device=DEV); pad[wr] = False
    assert float(qhat[pad].abs().max()) == 0.0, "pad rows of the wide query table must be zero"
    report("qnorm", qn[wr], torch.linalg.norm(Q.double(), dim=-1), 1e-6, 1e-5)
    report("sims", sims, ref.detach(), 2e-5, 1e-4)
    assert torch.equal(am.long(), s_all.detach().view(rows, C, 3).argmax(-1)), "argmax"
    report("inv_norm", inv, 1 / (torch.linalg.norm(e.double(), dim=-1) + 1e-6), 1e-6, 1e-5)
    # ---- backward
    dsims = rnd(rows, C, seed=7)
    ref.backward(dsims.double())
    de = torch.full((rows, Dt), 7.0, device=DEV, dtype=torch.bfloat16); G = torch.full((rows, Qp), 7.0, device=DEV, dtype=torch.bfloat16)
    eb = torch.full((rows, Dt), 7.0, device=DEV, dtype=torch.bfloat16)
    ops.class_sims_wide_bwd(dsims, sims, am, inv, e, qhat, de, G, eb, rows, Dt, C)
    assert torch.equal(eb, e.bfloat16())
    report("de", de, er.grad, 2e-3 * float(er.grad.abs().max()), 8e-3)
    # G[r, j] = dsims[r, c] * inv[r] at class c's arg-max prompt (wide column), 0 elsewhere -- pad columns included
    Gref = torch.zeros(rows, Qp, device=DEV, dtype=torch.float64)
    cols = wr.view(C, 3)[:, 0][None] + am.long()
    Gref.scatter_(1, cols, dsims.double() * (1 / (torch.linalg.norm(e.double(), dim=-1) + 1e-6))[:, None])
    report("G", G, Gref, 1e-6, 8e-3)
    dqhat_w = G.float().t() @ eb.float()                          # [Qp, Dt], what the weight-gradient GEMM computes
    report("dqhat", dqhat_w[wr], qh.grad, 2e-2 * float(qh.grad.abs().max()), 2e-2)
    assert float(dqhat_w[pad.nonzero().flatten()].abs().max()) == 0.0 and float(dqhat_w[32 * nb:].abs().max() if Qp > 32 * nb else 0.0) == 0.0
    de2 = torch.zeros_like(de); G2 = torch.zeros_like(G); eb2 = torch.zeros_like(eb)
    ops.class_sims_wide_bwd(dsims, sims, am, inv, e, qhat, de2, G2, eb2, rows, Dt, C)
    assert torch.equal(de, de2) and torch.equal(G, G2) and torch.equal(eb, eb2)
    # ---- dQ: (1) the kernel alone on the float64 prompt gradient, pad rows of its input holding 7.0 (never read), accumulating; test_query_normalize_bwd's band
    dq_in = torch.full((Qp, Dt), 7.0, device=DEV)
    dq_in[wr] = qh.grad.float()
    rowmax = Qr.grad.abs().amax(1, keepdim=True)
    init = (rnd(3 * C, Dt, seed=9).double() * 0.5 * rowmax).float()
    dQ = init.clone()
    ops.query_normalize_wide_bwd(dq_in, Q, dQ, 3 * C, Dt)
    report("dQ (kernel alone)", dQ, init.double() + Qr.grad, 1e-5 * rowmax, 1e-6)
    # (2) the chain as the model runs it: bf16 G^T e -> dQ, at the prompt gradient's band
    dQ2 = torch.zeros(3 * C, Dt, device=DEV)
    ops.query_normalize_wide_bwd(dqhat_w, Q, dQ2, 3 * C, Dt)
    report("dQ (chain)", dQ2, Qr.grad, 2e-2 * float(Qr.grad.abs().max()), 2e-2)
    dQ3 = torch.zeros_like(dQ2)
    ops.query_normalize_wide_bwd(dqhat_w, Q, dQ3, 3 * C, Dt)
    assert torch.equal(dQ2, dQ3)


@pytest.mark.parametrize("rows,Dt,C", [(300, 512, 80), (37, 768, 91)])
def test_wide_columns_are_the_narrow_kernels_bits(rows, Dt, C):
    """Column c of the wide result depends on the e row and class c's three prompts only, and carries the bits the narrow kernel (ops.class_sims on
    ops.query_normalize) gives for a call on classes 10 (c // 10) .. + 9 alone; argmax and inv_norm likewise."""
    e = rnd(rows, Dt, scale=0.7, seed=1)
    Q = rnd(3 * C, Dt, seed=4)
    qhat, qn, sims, am, inv, nb, Qp = _wide_forward(e, Q, rows, Dt, C)
    for b in range(nb):
        Cb = min(10, C - 10 * b)
        q32 = torch.zeros(32, Dt, device=DEV); n32 = torch.zeros(32, device=DEV)
        ops.query_normalize(Q[30 * b: 30 * b + 3 * Cb].contiguous(), q32, n32, 3 * Cb, Dt)
        assert torch.equal(q32, qhat[32 * b: 32 * b + 32]), f"qhat block {b}"
        assert torch.equal(n32[: 3 * Cb], qn[32 * b: 32 * b + 3 * Cb])
        s = torch.zeros(rows, Cb, device=DEV); a = torch.zeros(rows, Cb, dtype=torch.uint8, device=DEV); i = torch.zeros(rows, device=DEV)
        ops.class_sims(e, q32, s, a, i, rows, Dt, Cb)
        assert torch.equal(s, sims[:, 10 * b: 10 * b + Cb]), f"sims block {b}"
        assert torch.equal(a, am[:, 10 * b: 10 * b + Cb]), f"argmax block {b}"
        assert torch.equal(i, inv), f"inv_norm block {b}"


# ---------------------------------------------------------------------------------------------------
# the model against the reference fixture f11_tiny_c80 (tests/golden/make_golden_labelsets.py)
# ---------------------------------------------------------------------------------------------------
TOL_BOXES, TOL_SIMS_SMALLCFG = 4e-3, 3.5e-3           # tests/test_model_gpu.py's bands for f1_tiny
LOSS_REL_SMALLCFG = 2e-2


@pytest.fixture(scope="module")
def f11(golden_dir):
    g = np.load(os.path.join(golden_dir, "f11_tiny_c80.npz"))
    cfg = get_config("tiny", n_classes=int(g["n_classes"]))
    seed = int(g["seed"])
    return dict(g=g, cfg=cfg, seed=seed, W=weights.make_weights(cfg, seed), img=synth.make_images(cfg, 1, seed))


def _grad_report(grads, ref, tag):
    """tests/test_model_gpu.py's: rel-L2 per tensor against max(|ref|, 1e-3 * largest |ref|), cosine where the reference is not ~0."""
    floor = 1e-3 * max(float(r.float().norm()) for r in ref.values())
    worst, worst_cos, lines = 0.0, 1.0, []
    for n, r in ref.items():
        g, r = grads[n].float(), r.float()
        rel = float((g - r).norm() / max(float(r.norm()), floor))
        cos = float((g * r).sum() / (g.norm() * r.norm() + 1e-20)) if float(r.norm()) > floor else 1.0
        lines.append(f"  {n:58s} rel_l2={rel:.3e} cos={cos:.5f} |ref|={float(r.norm()):.3e}")
        worst, worst_cos = max(worst, rel), min(worst_cos, cos)
    print(f"[{tag}] worst rel-L2 grad error {worst:.3e}, worst cos {worst_cos:.5f}\n" + "\n".join(lines))
    return worst, worst_cos


def test_f11_forward_matches_reference(f11):
    g, cfg = f11["g"], f11["cfg"]
    model = OwlViT(cfg, f11["W"], DEV)
    assert model.wide_head
    with torch.no_grad():
        pb, _, ps, _ = model(torch.from_numpy(f11["img"]).to(DEV))
    assert ps.shape == (1, cfg.patches, 80)
    eb = float((pb.cpu() - torch.from_numpy(g["pred_boxes"])).abs().max()); es = float((ps.cpu() - torch.from_numpy(g["pred_sims"])).abs().max())
    print(f"tiny C=80 vs reference fixture F11: max|d boxes|={eb:.3e} max|d sims|={es:.3e}")
    assert eb < TOL_BOXES and es < TOL_SIMS_SMALLCFG, (eb, es)


def test_f11_loss_on_reference_outputs(f11):
    """PushPullLoss(80, scales) on the reference's own pred_sims / pred_boxes: identical assignment and labels after spreading, losses within 1e-5."""
    g = f11["g"]
    crit = PushPullLoss(80, g["scales"])
    n = len(g["tgt_labels"])
    losses = crit(torch.from_numpy(g["pred_sims"]).to(DEV), [torch.from_numpy(g["tgt_labels"]).to(DEV)], torch.from_numpy(g["pred_boxes"]).to(DEV),
                  [torch.from_numpy(g["tgt_boxes"]).to(DEV)])
    assert np.array_equal(crit.last["pred_idx"][0, :n].cpu().numpy(), g["pred_idx"])
    assert np.array_equal(crit.last["tgt_idx"][0, :n].cpu().numpy(), g["tgt_idx"])
    assert np.array_equal(crit.last["target_classes"][0].cpu().numpy(), g["target_classes"])
    for k in LOSS_KEYS:
        print(f"   {k}: {float(losses[k]):.7f} ref {float(g[k]):.7f}")
        assert float(losses[k]) == pytest.approx(float(g[k]), rel=1e-5), k


def test_f11_backward_chain_matches_oracle_given_same_upstream(f11):
    """Identical upstream (d_boxes, d_sims) into the HIP backward and the oracle's autograd at 80 classes: all 29 tensors at the chain band of
    tests/test_model_gpu.py (rel-L2 2e-2, cosine 0.9995); `queries` also per 10-class block, so a block without gradient cannot hide in the norm."""
    cfg, B = f11["cfg"], 1
    gen = torch.Generator().manual_seed(5)
    d_boxes = torch.randn(B, cfg.patches, 4, generator=gen) * 0.1
    d_sims = torch.randn(B, cfg.patches, cfg.n_classes, generator=gen) * 0.1
    w = {k: torch.from_numpy(v) for k, v in f11["W"].items()}
    names = O.trainable_names(w)
    ww = {n: (t.clone().requires_grad_(True) if n in names else t) for n, t in w.items()}
    taps = {}
    img = torch.from_numpy(f11["img"])
    rb, rs = O.model_forward(cfg, ww, img, taps)
    with torch.no_grad():          # no upstream where the top two prompts are within bf16 forward noise (the routing would be a coin flip), as in the narrow chain test
        e = F.linear(taps["feats"], w["class_predictor.dense0.weight"], w["class_predictor.dense0.bias"])
        e = e / (torch.linalg.norm(e, dim=-1, keepdim=True) + 1e-6)
        q = w["queries"] / torch.linalg.norm(w["queries"], dim=-1, keepdim=True) + 1e-6
        top2 = (e @ q.transpose(1, 2)).view(B, cfg.patches, cfg.n_classes, 3).topk(2, dim=-1).values
        d_sims = d_sims * ((top2[..., 0] - top2[..., 1]) > 0.02).float()
    model = OwlViT(cfg, f11["W"], DEV)
    pb, _, ps, _ = model(img.to(DEV))
    torch.autograd.backward([pb, ps], [d_boxes.to(DEV), d_sims.to(DEV)])
    grads = {n: p.grad.detach().float().cpu() for n, p in model.named_parameters() if p.requires_grad}
    torch.autograd.backward([rb, rs], [d_boxes, d_sims])
    gref = {n: ww[n].grad for n in names}
    assert len(grads) == 29 and set(grads) == set(gref)
    worst, worst_cos = _grad_report(grads, gref, "backward-only tiny C=80")
    assert worst < 2e-2 and worst_cos > 0.9995
    gq, rq = grads["queries"].reshape(240, -1), gref["queries"].reshape(240, -1)
    for b in range(8):
        gb, rb_ = gq[30 * b: 30 * b + 30], rq[30 * b: 30 * b + 30]
        assert float(rb_.norm()) > 0
        rel = float((gb - rb_).norm() / rb_.norm()); cos = float((gb * rb_).sum() / (gb.norm() * rb_.norm()))
        print(f"   queries block {b}: rel-L2 {rel:.3e} cos {cos:.5f}")
        assert rel < 2e-2 and cos > 0.9995, (b, rel, cos)


def test_f11_train_step_matches_reference(f11):
    """End to end at 80 classes: the reference's decisions, losses and all 29 gradients at the bands tests/test_model_gpu.py holds f1_tiny to."""
    g, cfg = f11["g"], f11["cfg"]
    model = OwlViT(cfg, f11["W"], DEV)
    crit = PushPullLoss(cfg.n_classes, g["scales"])
    pb, _, ps, _ = model(torch.from_numpy(f11["img"]).to(DEV))
    losses = crit(ps, [torch.from_numpy(g["tgt_labels"]).to(DEV)], pb, [torch.from_numpy(g["tgt_boxes"]).to(DEV)])
    (losses["loss_ce"] + losses["loss_bg"] + losses["loss_bbox"] + losses["loss_giou"]).backward()
    n = len(g["tgt_labels"])
    assert np.array_equal(crit.last["pred_idx"][0, :n].cpu().numpy(), g["pred_idx"]) and np.array_equal(crit.last["tgt_idx"][0, :n].cpu().numpy(), g["tgt_idx"])
    assert np.array_equal(crit.last["target_classes"][0].cpu().numpy(), g["target_classes"])
    for k in LOSS_KEYS:
        rel = abs(float(losses[k].detach()) - float(g[k])) / abs(float(g[k]))
        print(f"   {k}: {float(losses[k].detach()):.6f} ref {float(g[k]):.6f} rel {rel:.2e}")
        assert rel <= LOSS_REL_SMALLCFG, k
    grads = {nm: p.grad.detach().float().cpu() for nm, p in model.named_parameters() if p.requires_grad}
    ref = {k[5:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("grad/")}
    assert len(ref) == 29 and set(ref) == set(grads)
    worst, worst_cos = _grad_report(grads, ref, "tiny C=80 vs reference fixture")
    assert worst_cos > 0.99


# ---------------------------------------------------------------------------------------------------
# public surface
# ---------------------------------------------------------------------------------------------------
def _five_steps(seed):
    from owl_vit_object_detection_amd.optim import FusedAdamW
    model = load_model({i: f"label {i}" for i in range(80)}, DEV, arch="tiny", seed=seed)
    cfg = model.cfg
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.0)          # (no decay: only a gradient moves a parameter)
    B = 2
    img = torch.from_numpy(synth.make_images(cfg, B, seed)).to(DEV)
    labels, boxes = synth.make_targets(cfg, B, seed, max_boxes=6)
    # one target per 10-class block on top of the seeded ones: every block of the query bank gets a pull gradient
    rs = np.random.default_rng(seed)
    for i in range(B):
        xy, wh = rs.uniform(0.05, 0.6, (8, 2)), rs.uniform(0.1, 0.3, (8, 2))
        labels[i] = np.concatenate([labels[i], np.arange(4 * i, 80, 10)]).astype(np.int64)
        boxes[i] = np.concatenate([boxes[i], np.concatenate([xy, xy + wh], 1)]).astype(np.float32)
    crit = PushPullLoss(cfg.n_classes, synth.class_scales(cfg, labels))
    q0 = model.queries.detach().clone()
    hist = []
    for _ in range(5):
        opt.zero_grad()
        pb, _, ps, _ = model(img)
        losses = crit(ps, [torch.from_numpy(l).to(DEV) for l in labels], pb, [torch.from_numpy(b).to(DEV) for b in boxes])
        (losses["loss_ce"] + losses["loss_bg"] + losses["loss_bbox"] + losses["loss_giou"]).backward()
        opt.step()
        hist.append([float(losses[k]) for k in LOSS_KEYS])
        q1 = model.queries.detach().clone()
        moved = (q1 - q0).reshape(240, -1).abs().amax(1).view(8, 30).amax(1)
        assert bool((moved > 0).all()), ("queries did not change in every 10-class block", moved.tolist())
        q0 = q1
    torch.cuda.synchronize()
    return model, hist


def test_load_model_80_labels_trains_and_is_deterministic():
    m1, h1 = _five_steps(1234)
    assert m1.wide_head and m1.queries.shape == (1, 240, m1.cfg.text_dim)
    assert np.isfinite(np.asarray(h1)).all(), h1
    m2, h2 = _five_steps(1234)
    assert h1 == h2 and torch.equal(m1.flat_param, m2.flat_param)


def test_load_model_80_labels_with_text_queries():
    from owl_vit_object_detection_amd.config import get_text_config
    from owl_vit_object_detection_amd.text import TextTower
    ids = np.zeros((240, 16), np.int64)
    rng = np.random.default_rng(0)
    for n in range(240):
        L = 1 + n % 6
        ids[n, 0] = 95; ids[n, 1:1 + L] = rng.integers(1, 95, L); ids[n, 1 + L] = 96
    model = load_model({i: f"label {i}" for i in range(80)}, DEV, arch="tiny", prompt_ids=ids)
    exp = TextTower(get_text_config("tiny")).query_bank(ids)
    assert model.queries.shape == (1, 240, 64) and model.queries.requires_grad
    assert torch.equal(model.queries.detach(), exp)
    with torch.no_grad():
        pb, _, ps, _ = model(torch.from_numpy(synth.make_images(model.cfg, 1)).to(DEV))
    assert ps.shape == (1, model.cfg.patches, 80) and bool(torch.isfinite(ps).all())


def test_eval_path_80_classes_map_per_class():
    from owl_vit_object_detection_amd.metrics import MeanAveragePrecision
    from owl_vit_object_detection_amd.models import PostProcess
    from owl_vit_object_detection_amd.train_util import update_metrics
    B = 2
    model = load_model({i: f"label {i}" for i in range(80)}, DEV, arch="tiny").eval()
    with torch.no_grad():
        pred_boxes, _, pred_sims, _ = model(torch.from_numpy(synth.make_images(model.cfg, B, seed=3)).to(DEV))
    boxes, classes, scores = PostProcess(0.01, 0.6)(pred_boxes, pred_sims, top_k=200)
    assert int(classes.max()) < 80
    labels, gts = synth.make_targets(model.cfg, B, seed=5, max_boxes=6)
    G = max(len(l) for l in labels)
    gt_boxes = torch.zeros(B, G, 4); gt_labels = torch.full((B, G), -1, dtype=torch.int64)
    for b in range(B):
        gt_boxes[b, :len(labels[b])] = torch.from_numpy(gts[b]); gt_labels[b, :len(labels[b])] = torch.from_numpy(np.asarray(labels[b], dtype=np.int64))
    metric = MeanAveragePrecision(iou_type="bbox", class_metrics=True, n_classes=80).to(DEV)
    update_metrics(metric, {"width": 640.0, "height": 480.0}, boxes, classes, scores, gt_boxes, gt_labels)
    out = metric.compute()
    assert out["map_per_class"].numel() == 80


def test_385_labels_raise_at_construction():
    with pytest.raises(ValueError, match="384"):
        load_model({i: f"label {i}" for i in range(385)}, DEV, arch="tiny")


def test_ten_classes_stay_on_the_narrow_path():
    from owl_vit_object_detection_amd.autograd import _bws
    cfg = get_config("tiny", n_classes=10)
    model = OwlViT(cfg, weights.make_weights(cfg), DEV)
    assert not model.wide_head
    B = 2
    pb, _, ps, _ = model(torch.from_numpy(synth.make_images(cfg, B)).to(DEV))
    (pb.sum() + ps.sum()).backward()
    Mh = ops.pad_rows(B * cfg.patches)
    ws, bw = model._workspace(B), _bws(model, B)
    assert tuple(ws["qhat"].shape) == (32, cfg.text_dim) and tuple(ws["qnorm"].shape) == (32,)
    assert tuple(bw["g32"].shape) == (Mh, 32) and tuple(bw["dqhat"].shape) == (32, cfg.text_dim)
    wide = OwlViT(get_config("tiny", n_classes=11), weights.make_weights(get_config("tiny", n_classes=11)), DEV)
    assert wide.wide_head and tuple(wide._workspace(B)["qhat"].shape) == (64, cfg.text_dim)
