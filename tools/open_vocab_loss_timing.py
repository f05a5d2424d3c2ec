"""What the open-vocabulary criterion costs on the card: every launch of csrc/open_vocab_loss.hip (cost, owl_hungarian, class forward, box pairs, reduce,
class backward, box combine) at B/16 768^2 batch 32 (rows = 32 x 2304) for Q = 30, 91, 365 and 1203 queries per image, per-image masks, five targets per
image; their sum; and, in the same windows, the parent's way of doing it: the sigmoid focal loss in torch ops of tools/open_vocab_bwd_timing.py, forward
plus backward (which does no matching and no box loss).  Then the whole `forward_queries` train step at 91 queries both ways on owlvit-base-patch16.
  python tools/open_vocab_loss_timing.py [--out profiles/open_vocab_loss.md] [--windows 5] [--launches 10] [--limit 600] [--no-model]
Method: one fresh child process under its own time limit; a window is `--launches` launches (3 steps for the whole-model rows) between two HIP events,
the forms alternate window by window after a warm-up window of each; every figure is the median of `--windows` windows (min .. max).  GB/s of the two
class kernels: logits read once (forward), read once and written once (backward).  Recorded, not asserted."""
import argparse, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: F401  (the importable alias of the package directory)

B, P = 32, 2304
QS = (30, 91, 365, 1203)
STEP_Q = 91
NT = 5
LN_TBS = 6.2          # TB/s the LayerNorm kernels reach (profiles/): the yardstick for a streaming kernel on this card


def child(windows, launches, with_model):
    import torch
    from owl_vit_object_detection_amd import _lib, ops
    from owl_vit_object_detection_amd.matcher import PackedTargets
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
    xy = torch.rand(B, P, 2, generator=g) * 0.6
    boxes = torch.cat([xy, xy + 0.05 + 0.3 * torch.rand(B, P, 2, generator=g)], -1).to(dev)
    s = ops.stream()
    out = []
    for Q in QS:
        mask_b = torch.rand(B, Q, generator=g) > 0.1
        mask_b[:, :NT] = True
        mask = mask_b.to(torch.uint8).to(dev)
        live = mask_b.to(dev)[:, None, :].expand(B, P, Q)
        logits = torch.where(live, torch.empty(B, P, Q, device=dev).normal_().mul_(3.0).sub_(4.0), torch.full((), torch.finfo(torch.float32).min, device=dev))
        rows = [torch.randperm(P, generator=g)[:NT] for _ in range(B)]
        tgts = [boxes[b, rows[b].to(dev)].cpu() + 0.01 * (torch.rand(NT, 4, generator=g) - 0.5) for b in range(B)]
        labs = [torch.randint(0, NT, (NT,), generator=g) for _ in range(B)]
        tg = PackedTargets(labs, tgts, dev, None, allow_empty=True)
        N, nb = tg.Nmax, float(B * NT)
        costT = torch.empty(B, N, P, device=dev)
        pred_idx, tgt_idx = torch.empty(B, N, dtype=torch.int64, device=dev), torch.empty(B, N, dtype=torch.int64, device=dev)
        tc = torch.empty(B, P, dtype=torch.int64, device=dev)
        nbytes = torch.zeros(1, dtype=torch.int64)
        _lib.call("owl_focal_loss_workspace_bytes", B, P, Q, nbytes)
        ws = torch.empty(int(nbytes) // 8, dtype=torch.float64, device=dev)
        losses, g3 = torch.empty(3, device=dev), torch.tensor([1.0, 5.0, 2.0], device=dev)
        dl1, dgiou, dboxes = torch.empty(B, P, 4, device=dev), torch.empty(B, P, 4, device=dev), torch.empty(B, P, 4, device=dev)
        dlogits = torch.empty(B, P, Q, device=dev)
        target = (torch.rand(B, P, Q, generator=g) < 0.01).float().to(dev)
        lg_t = logits.clone().requires_grad_(True)

        def torch_focal():
            x = torch.where(live, lg_t, torch.zeros_like(lg_t))
            p = torch.sigmoid(x)
            ce = torch.nn.functional.binary_cross_entropy_with_logits(x, target, reduction="none")
            pt = p * target + (1 - p) * (1 - target)
            l = torch.where(live, (0.25 * target + 0.75 * (1 - target)) * (1 - pt) ** 2 * ce, torch.zeros_like(ce)).sum() / live.sum()
            lg_t.grad = None
            l.backward()

        forms = dict(
            cost=lambda: _lib.call("owl_focal_match_cost", s, logits, mask, boxes, tg.labels, tg.boxes, tg.counts, costT, B, P, Q, B, N, 0.25, 1.0, 5.0, 2.0),
            hungarian=lambda: _lib.call("owl_hungarian", s, costT, tg.labels, tg.counts, pred_idx, tgt_idx, tc, B, P, N, Q),
            class_fwd=lambda: _lib.call("owl_focal_loss_fwd", s, logits, mask, tc, ws, int(nbytes), B, P, Q, B, 0.25),
            pairs=lambda: _lib.call("owl_box_pair_loss", s, boxes, mask, tg.labels, tg.boxes, pred_idx, tgt_idx, tg.counts, ws, int(nbytes), dl1, dgiou, B, P, Q, B, N),
            reduce=lambda: _lib.call("owl_open_vocab_loss_reduce", s, ws, int(nbytes), losses, B, P, Q, nb),
            class_bwd=lambda: _lib.call("owl_focal_loss_bwd", s, g3, logits, mask, tc, dlogits, B, P, Q, B, 0.25, nb),
            boxes_bwd=lambda: _lib.call("owl_box_pair_loss_bwd", s, g3, dl1, dgiou, dboxes, B, P, nb),
            torch_focal=torch_focal)
        out.append(dict(Q=Q, mb=B * P * Q * 4 / 2 ** 20, us=measure(forms, launches)))
        del logits, dlogits, target, lg_t, live, costT
        torch.cuda.empty_cache()
    model_res = None
    if with_model:
        from owl_vit_object_detection_amd import synth, weights
        from owl_vit_object_detection_amd.config import get_config
        from owl_vit_object_detection_amd.losses import OpenVocabLoss
        from owl_vit_object_detection_amd.models import OwlViT
        from owl_vit_object_detection_amd.optim import FusedAdamW
        cfg = get_config("owlvit-base-patch16")
        D = cfg.hidden
        model = OwlViT(cfg, weights.make_weights(cfg), dev)
        model.set_logit_head({"logit_shift.weight": (torch.randn(D, generator=g) / D ** 0.5).to(dev), "logit_shift.bias": torch.tensor([0.05], device=dev),
                              "logit_scale.weight": (torch.randn(D, generator=g) / D ** 0.5).to(dev), "logit_scale.bias": torch.tensor([0.1], device=dev)})
        opt = FusedAdamW(model, lr=1e-5, weight_decay=0.1)
        img = torch.from_numpy(synth.make_images(cfg, 4)).to(dev).repeat(B // 4, 1, 1, 1).to(torch.bfloat16)
        qe = torch.randn(B, STEP_Q, cfg.text_dim, generator=g).to(dev)
        qm_host = torch.rand(B, STEP_Q, generator=g) > 0.1
        qm_host[:, :NT] = True
        qm = qm_host.to(dev)
        live = qm[:, None, :].expand(B, cfg.patches, STEP_Q)
        target = (torch.rand(B, cfg.patches, STEP_Q, generator=g) < 0.01).float().to(dev)
        xy = torch.rand(B, NT, 2, generator=g) * 0.6
        targets = [{"class_labels": torch.randint(0, NT, (NT,), generator=g), "boxes": torch.cat([xy[b], xy[b] + 0.05 + 0.3 * torch.rand(NT, 2, generator=g)], -1)}
                   for b in range(B)]
        crit = OpenVocabLoss()

        def focal(lg):
            x = torch.where(live, lg, torch.zeros_like(lg))
            p = torch.sigmoid(x)
            ce = torch.nn.functional.binary_cross_entropy_with_logits(x, target, reduction="none")
            pt = p * target + (1 - p) * (1 - target)
            return torch.where(live, (0.25 * target + 0.75 * (1 - target)) * (1 - pt) ** 2 * ce, torch.zeros_like(ce)).sum() / live.sum()

        def torch_step():
            opt.zero_grad()
            pb, lg = model.forward_queries(img, qe, qm)
            (focal(lg) + 0.1 * pb.square().mean()).backward()
            opt.step()

        def crit_step():
            opt.zero_grad()
            pb, lg = model.forward_queries(img, qe, qm)
            o = crit(lg, pb, targets, query_mask=qm)
            (o["loss_ce"] + 5.0 * o["loss_bbox"] + 2.0 * o["loss_giou"]).backward()
            opt.step()

        model_res = dict(Q=STEP_Q, us=measure(dict(torch_ops=torch_step, criterion=crit_step), 3))
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
    names = ("cost", "hungarian", "class_fwd", "pairs", "reduce", "class_bwd", "boxes_bwd")
    lines = [f"The open-vocabulary criterion at rows = {B} x {P}, per-image masks, {NT} targets per image; us per launch, median (min .. max) of the windows", "",
             "| Q (logits MiB) | cost | owl_hungarian | class fwd | box pairs | reduce | class bwd | boxes bwd | sum | torch-ops focal fwd + bwd (no matching, no boxes) |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for o in data["kernel"]:
        u = o["us"]
        total = sum(u[k]["median"] for k in names)
        lines.append(f"| {o['Q']} ({o['mb']:.0f}) | " + " | ".join(f(u[k]) for k in names) + f" | {total:.1f} | {f(u['torch_focal'])} |")
    lines += ["", f"Achieved traffic of the two class kernels (logits read once; read once + written once), GB/s, beside the {LN_TBS} TB/s the LayerNorm kernels reach", "",
              "| Q | class fwd GB/s | class bwd GB/s |", "|---|---|---|"]
    for o in data["kernel"]:
        nbytes = B * P * o["Q"] * 4
        lines.append(f"| {o['Q']} | {nbytes / o['us']['class_fwd']['median'] / 1e3:.0f} | {2 * nbytes / o['us']['class_bwd']['median'] / 1e3:.0f} |")
    if data["model"]:
        m = data["model"]["us"]
        d = (m["criterion"]["median"] - m["torch_ops"]["median"]) / m["torch_ops"]["median"] * 100
        lines += ["", f"`forward_queries` train step on owlvit-base-patch16, batch {B}, {STEP_Q} queries per image, bf16 images, FusedAdamW in-line; us per step", "",
                  "| focal loss in torch ops + 0.1 mean(boxes^2) (the parent's step, re-measured in this run) | OpenVocabLoss (matching + focal + L1 + GIoU) | change |",
                  "|---|---|---|", f"| {f(m['torch_ops'])} | {f(m['criterion'])} | {d:+.2f} % |"]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
