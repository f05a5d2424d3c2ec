"""What zero-shot inference costs on the card: `owl_class_logits_fwd` (its two launches: the row pre-pass and the MFMA kernel) at B/16 768^2 batch 32
(rows = 32 x 2304, Dt = 512, D = 768) for Q = 30, 91, 365 and 1203 queries per image, per-image banks, with scores; and the whole `detect_text` call.
Yardstick: the fine-tuning head's `owl_class_sims_wide_fwd` at the same rows and the nearest column count (C = ceil(Q / 3) classes, at most 384): the
same contraction on the same MFMA, so the new kernel should sit near it per (row, table column); the ratio is reported.  A table column is one of the
32 columns of a query block, computed whether it holds a query or not: 32 ceil(Q / 32) here, 32 ceil(C / 10) there.
  python tools/open_vocab_timing.py [--out profiles/open_vocab.md] [--windows 7] [--launches 20] [--limit 600] [--no-model]
Method: one fresh child process under its own time limit; a window is `--launches` launches between two HIP events, the forms alternate window by
window after a warm-up window of each; every figure is the median of `--windows` windows (min .. max).  Recorded, not asserted."""
import argparse, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: F401  (the importable alias of the package directory)

B, P, DT, D = 32, 2304, 512, 768
QS = (30, 91, 365, 1203)


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
    out = []
    for Q in QS:
        bank = torch.randn(B, Q, DT, generator=g).to(dev)
        mask = (torch.rand(B, Q, generator=g) > 0.1).to(torch.uint8).to(dev)
        logits, scores = torch.empty(B, P, Q, device=dev), torch.empty(B, P, Q, device=dev)
        C = min((Q + 2) // 3, ops.WIDE_MAX_CLASSES)
        qw = torch.randn(3 * C, DT, generator=g).to(dev)
        qhat = torch.zeros(32 * ops.wide_blocks(C), DT, device=dev)
        ops.query_normalize_wide(qw, qhat, None, 3 * C, DT)
        sims, argmax = torch.empty(rows, C, device=dev), torch.empty(rows, C, dtype=torch.uint8, device=dev)
        forms = dict(
            logits=lambda: ops.class_logits(e, bank, feats, w_shift, b_shift, w_scale, b_scale, B, P, mask=mask, rowstats=rowstats, logits=logits, scores=scores),
            logits_shared=lambda: ops.class_logits(e, bank[0], feats, w_shift, b_shift, w_scale, b_scale, B, P, rowstats=rowstats, logits=logits),
            wide=lambda: ops.class_sims_wide(e, qhat, sims, argmax, inv_norm, rows, DT, C))
        out.append(dict(Q=Q, C=C, cols=32 * ((Q + 31) // 32), cols_wide=32 * ops.wide_blocks(C), us=measure(forms, launches)))
        del bank, mask, logits, scores, sims, argmax
    model_res = []
    if with_model:
        from owl_vit_object_detection_amd import synth, weights
        from owl_vit_object_detection_amd.config import get_config, get_text_config
        from owl_vit_object_detection_amd.models import OwlViT
        from owl_vit_object_detection_amd.text import TextTower
        del e, feats
        cfg, tc = get_config("owlvit-base-patch16"), get_text_config("owlvit-base-patch16")
        model = OwlViT(cfg, weights.make_weights(cfg), dev)
        model.set_logit_head({"logit_shift.weight": w_shift, "logit_shift.bias": b_shift, "logit_scale.weight": w_scale, "logit_scale.bias": b_scale})
        tower = TextTower(tc, None, dev)
        img = torch.from_numpy(synth.make_images(cfg, 4)).to(dev).repeat(B // 4, 1, 1, 1).to(torch.bfloat16)
        for Q, shared in ((30, False), (91, True), (1203, True)):
            lead = (Q,) if shared else (B, Q)
            ids = torch.zeros(lead + (16,), dtype=torch.int64)          # BOS, three words, EOS, padding
            ids[..., 0], ids[..., 1:4], ids[..., 4] = tc.vocab - 2, torch.randint(1, 1000, lead + (3,), generator=g), tc.vocab - 1
            forms = dict(detect_text=lambda: model.detect_text(img, ids, tower, return_scores=True, shared=shared),
                         forward=lambda: model(img))
            with torch.no_grad():
                model_res.append(dict(Q=Q, shared=shared, us=measure(forms, max(1, launches // 10))))
    print("RESULT " + json.dumps(dict(kernel=out, model=model_res)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--limit", type=int, default=600, help="seconds for the child process")
    ap.add_argument("--no-model", action="store_true", help="the kernels only (skips building B/16 and the detect_text rows)")
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
    rows = B * P
    lines = [f"`owl_class_logits_fwd` at rows = {B} x {P}, Dt = {DT}, D = {D}; us per call, median (min .. max) of the windows", "",
             "| Q | per-image banks + mask + scores | one shared bank, logits only | `owl_class_sims_wide_fwd`, C classes | ps per (row, table column): new / wide | ratio |",
             "|---|---|---|---|---|---|"]
    for o in data["kernel"]:
        u = o["us"]
        a, w = u["logits_shared"]["median"] * 1e6 / (rows * o["cols"]), u["wide"]["median"] * 1e6 / (rows * o["cols_wide"])
        lines.append(f"| {o['Q']} ({o['cols']} columns) | {f(u['logits'])} | {f(u['logits_shared'])} | {f(u['wide'])} (C = {o['C']}, {o['cols_wide']} columns) | {a:.2f} / {w:.2f} | {a / w:.2f} |")
    if data["model"]:
        lines += ["", f"`detect_text` on owlvit-base-patch16, batch {B}, bf16 images, with scores (text tower + forward + head); the plain eval forward beside it", "",
                  "| Q | prompts | `detect_text` us | `model(image)` us |", "|---|---|---|---|"]
        for o in data["model"]:
            lines.append(f"| {o['Q']} | {'one list for the batch' if o['shared'] else 'per image'} | {f(o['us']['detect_text'])} | {f(o['us']['forward'])} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
