"""What fine-tuning through HF's class head costs on the card: `owl_class_logits_bwd` (its launches: q^, the row pass, and -- with a query gradient --
the dq^ slabs and their reduction) at B/16 768^2 batch 32 (rows = 32 x 2304, Dt = 512, D = 768) for Q = 30, 91, 365 and 1203 queries per image,
per-image banks and masks.  Beside it: the bank head's `owl_class_sims_wide_bwd` at the same rows and the nearest column count (C = ceil(Q / 3) classes,
at most 384; it writes de and the routed G, its query gradient is a further weight-gradient GEMM not timed here) and `owl_class_logits_fwd`.  Then the
whole `forward_queries` train step (forward, a focal loss in torch ops, backward, FusedAdamW) beside the bank-path step (PushPullLoss) of the same
build on owlvit-base-patch16, batch 32.
  python tools/open_vocab_bwd_timing.py [--out profiles/open_vocab_bwd.md] [--windows 5] [--launches 10] [--limit 600] [--no-model]
Method: one fresh child process under its own time limit; a window is `--launches` launches (3 steps for the whole-model rows) between two HIP events,
the forms alternate window by window after a warm-up window of each; every figure is the median of `--windows` windows (min .. max).  Recorded, not
asserted."""
import argparse, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: F401  (the importable alias of the package directory)

B, P, DT, D = 32, 2304, 512, 768
QS = (30, 91, 365, 1203)
STEP_Q = 91


def child(windows, launches, with_model):
    import torch
    from owl_vit_object_detection_amd import ops
    dev = "cuda"

    def between_events(fn, n):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n * 1e3          # us

    def measure(forms, n):
        for fn in forms.values():
            between_events(fn, 2)
        us = {k: [] for k in forms}
        for _ in range(windows):
            for k, fn in forms.items():
                us[k].append(between_events(fn, n))
        return {k: dict(median=statistics.median(v), lo=min(v), hi=max(v)) for k, v in us.items()}

    g = torch.Generator().manual_seed(0)
    rows = B * P
    e = (0.7 * torch.randn(rows, DT, generator=g)).to(dev)
    feats = torch.randn(rows, D, generator=g).to(torch.bfloat16).to(dev)
    w_shift, w_scale = (torch.randn(D, generator=g) / D ** 0.5).to(dev), (torch.randn(D, generator=g) / D ** 0.5).to(dev)
    b_shift, b_scale = torch.tensor([0.05], device=dev), torch.tensor([0.1], device=dev)
    rowstats = torch.empty(rows, 2, device=dev)
    inv_norm = torch.empty(rows, device=dev)
    de, e_bf = torch.empty(rows, DT, dtype=torch.bfloat16, device=dev), torch.empty(rows, DT, dtype=torch.bfloat16, device=dev)
    dfeats = torch.empty(rows, D, device=dev)
    out = []
    for Q in QS:
        bank = torch.randn(B, Q, DT, generator=g).to(dev)
        mask = (torch.rand(B, Q, generator=g) > 0.1).to(torch.uint8).to(dev)
        logits = torch.empty(B, P, Q, device=dev)
        dlog = torch.empty(B, P, Q, device=dev).normal_().mul_(0.1)
        dq = torch.empty_like(bank)
        wsp = torch.empty(ops.class_logits_bwd_workspace_bytes(B, P, Q, B, DT, True), dtype=torch.uint8, device=dev)
        ops.class_logits(e, bank, feats, w_shift, b_shift, w_scale, b_scale, B, P, mask=mask, rowstats=rowstats, logits=logits)
        C = min((Q + 2) // 3, ops.WIDE_MAX_CLASSES)
        qw = torch.randn(3 * C, DT, generator=g).to(dev)
        qhat = torch.zeros(32 * ops.wide_blocks(C), DT, device=dev)
        ops.query_normalize_wide(qw, qhat, None, 3 * C, DT)
        sims, argmax = torch.empty(rows, C, device=dev), torch.empty(rows, C, dtype=torch.uint8, device=dev)
        ops.class_sims_wide(e, qhat, sims, argmax, inv_norm, rows, DT, C)
        dsims = torch.empty(rows, C, device=dev).normal_().mul_(0.1)
        gr = torch.empty(rows, ops.wide_qp(C), dtype=torch.bfloat16, device=dev)
        forms = dict(
            bwd=lambda: ops.class_logits_bwd(dlog, e, bank, w_shift, w_scale, rowstats, B, P, mask=mask, de=de, dfeats=dfeats, dqueries=dq, workspace=wsp),
            bwd_no_dq=lambda: ops.class_logits_bwd(dlog, e, bank, w_shift, w_scale, rowstats, B, P, mask=mask, de=de, dfeats=dfeats, dqueries=False, workspace=wsp),
            wide_bwd=lambda: ops.class_sims_wide_bwd(dsims, sims, argmax, inv_norm, e, qhat, de, gr, e_bf, rows, DT, C),
            fwd=lambda: ops.class_logits(e, bank, feats, w_shift, b_shift, w_scale, b_scale, B, P, mask=mask, rowstats=rowstats, logits=logits))
        out.append(dict(Q=Q, C=C, cols=32 * ((Q + 31) // 32), cols_wide=32 * ops.wide_blocks(C), workspace_mb=wsp.numel() / 2 ** 20, us=measure(forms, launches)))
        del bank, mask, logits, dlog, dq, wsp, sims, argmax, dsims, gr
    model_res = None
    if with_model:
        from owl_vit_object_detection_amd import synth, weights
        from owl_vit_object_detection_amd.config import get_config
        from owl_vit_object_detection_amd.losses import PushPullLoss
        from owl_vit_object_detection_amd.models import OwlViT
        from owl_vit_object_detection_amd.optim import FusedAdamW
        del e, feats, de, e_bf, dfeats
        torch.cuda.empty_cache()
        cfg = get_config("owlvit-base-patch16")
        model = OwlViT(cfg, weights.make_weights(cfg), dev)
        model.set_logit_head({"logit_shift.weight": w_shift, "logit_shift.bias": b_shift, "logit_scale.weight": w_scale, "logit_scale.bias": b_scale})
        opt = FusedAdamW(model, lr=1e-5, weight_decay=0.1)
        img = torch.from_numpy(synth.make_images(cfg, 4)).to(dev).repeat(B // 4, 1, 1, 1).to(torch.bfloat16)
        labels, boxes = synth.make_targets(cfg, B, max_boxes=5)
        lab, box = [torch.from_numpy(x).to(dev) for x in labels], [torch.from_numpy(x).to(dev) for x in boxes]
        crit = PushPullLoss(cfg.n_classes, None)
        qe = torch.randn(B, STEP_Q, cfg.text_dim, generator=g).to(dev)
        qm = (torch.rand(B, STEP_Q, generator=g) > 0.1).to(dev)
        live = qm[:, None, :].expand(B, cfg.patches, STEP_Q)
        target = (torch.rand(B, cfg.patches, STEP_Q, generator=g) < 0.01).float().to(dev)

        def focal(lg):
            x = torch.where(live, lg, torch.zeros_like(lg))
            p = torch.sigmoid(x)
            ce = torch.nn.functional.binary_cross_entropy_with_logits(x, target, reduction="none")
            pt = p * target + (1 - p) * (1 - target)
            return torch.where(live, (0.25 * target + 0.75 * (1 - target)) * (1 - pt) ** 2 * ce, torch.zeros_like(ce)).sum() / live.sum()

        def bank_step():
            opt.zero_grad()
            pb, _, ps, _ = model(img)
            l = crit(ps, lab, pb, box)
            (l["loss_ce"] + l["loss_bg"] + l["loss_bbox"] + l["loss_giou"]).backward()
            opt.step()

        def query_step(q):
            opt.zero_grad()
            pb, lg = model.forward_queries(img, q, qm)
            (focal(lg) + 0.1 * pb.square().mean()).backward()
            opt.step()

        qt = qe.clone().requires_grad_(True)
        forms = dict(bank=bank_step, queries=lambda: query_step(qe), queries_dq=lambda: query_step(qt))
        model_res = dict(Q=STEP_Q, C=cfg.n_classes, us=measure(forms, 3))
    print("RESULT " + json.dumps(dict(kernel=out, model=model_res)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--limit", type=int, default=600, help="seconds for the child process")
    ap.add_argument("--no-model", action="store_true", help="the kernels only (skips building B/16 and the train-step rows)")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.windows, args.launches, not args.no_model)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--windows", str(args.windows), "--launches", str(args.launches)] + (["--no-model"] if args.no_model else [])
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"no result within {args.limit} s -- stopped: nothing more is started on the device")
    res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not res:
        sys.exit(f"exit {r.returncode}\n{r.stderr[-2000:]}\n-- stopped: nothing more is started on the device")
    print(res[-1], flush=True)
    data = json.loads(res[-1][7:])
    f = lambda x: f"{x['median']:.1f} ({x['lo']:.1f} .. {x['hi']:.1f})"
    lines = [f"`owl_class_logits_bwd` at rows = {B} x {P}, Dt = {DT}, D = {D}, per-image banks and masks; us per call, median (min .. max) of the windows", "",
             "| Q | de + dfeats + dqueries | de + dfeats (dqueries NULL) | `owl_class_sims_wide_bwd`, C classes | `owl_class_logits_fwd` | workspace MiB |",
             "|---|---|---|---|---|---|"]
    for o in data["kernel"]:
        u = o["us"]
        lines.append(f"| {o['Q']} ({o['cols']} columns) | {f(u['bwd'])} | {f(u['bwd_no_dq'])} | {f(u['wide_bwd'])} (C = {o['C']}, {o['cols_wide']} columns) | {f(u['fwd'])} | {o['workspace_mb']:.0f} |")
    if data["model"]:
        m = data["model"]
        lines += ["", f"Train step on owlvit-base-patch16, batch {B}, bf16 images, the default trainable set, FusedAdamW in-line; us per step", "",
                  f"| bank path (`model(image)`, PushPullLoss, C = {m['C']}) | `forward_queries`, {m['Q']} queries per image, focal loss in torch ops | the same with `query_embeds.requires_grad` |",
                  "|---|---|---|", f"| {f(m['us']['bank'])} | {f(m['us']['queries'])} | {f(m['us']['queries_dq'])} |"]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
