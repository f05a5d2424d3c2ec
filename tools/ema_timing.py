"""What the exponential moving average of the trainable bucket costs on the card: the optimizer launch at the B/16 reference bucket (8,684,292 f32 elements)
in three forms -- `owl_adamw_step` alone (the step every earlier commit launches; csrc/optim.hip is unchanged), the fused `owl_adamw_step_ema`, and
`owl_adamw_step` followed by `owl_ema_update` -- and the full train step (forward, loss, backward, FusedAdamW) at bench.py's flagship setting (B/16 768^2,
batch 32, lr 3e-6, weight decay 0.1, in-line schedule) with `ema_decay=None` and `ema_decay=0.999`.
  python tools/ema_timing.py [--out profiles/ema.md] [--windows 5] [--launches 200] [--steps 6] [--arch owlvit-base-patch16] [--batch 32] [--limit 500]
Method: one fresh child process under its own time limit.  The forms ALTERNATE window by window (a, b, c, a, b, c, ...) after a warm-up window of each;
a launch window is `--launches` launches between two HIP events on buffers of their own, a step window `--steps` train steps between two HIP events; every
figure is the median of `--windows` windows with the spread (min .. max).  Nothing is asserted.  A child that fails ends the run: nothing more is started
on the device.  The table (markdown) goes to stdout and to --out."""
import argparse, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: F401  (the importable alias of the package directory)

BUCKET = 8684292          # B/16, C = 10: trainable parameters under the reference's freeze rule (the model's bucket adds 4 elements of alignment padding)


def child(arch, batch, windows, launches, steps):
    import torch
    from owl_vit_object_detection_amd import _lib, ops, synth, weights
    from owl_vit_object_detection_amd.config import get_config
    from owl_vit_object_detection_amd.losses import PushPullLoss
    from owl_vit_object_detection_amd.models import OwlViT
    from owl_vit_object_detection_amd.optim import FusedAdamW, ema_coefficients
    dev = "cuda"

    def between_events(fn, n):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    def alternate(forms, n, warm):
        for fn in forms.values():
            between_events(fn, warm)
        ms = {k: [] for k in forms}
        for _ in range(windows):
            for k, fn in forms.items():
                ms[k].append(between_events(fn, n))
        return {k: dict(median=statistics.median(v), lo=min(v), hi=max(v)) for k, v in ms.items()}

    # ---- the optimizer launch on buffers of the bucket's size ----
    n = BUCKET
    p, g, m, v, ema = (torch.randn(n, device=dev) * s for s in (1.0, 1e-3, 1e-4, 1e-4, 1.0))
    v = v.abs()
    bf = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    d, w = ema_coefficients(0.999)
    hyper = (n, 3e-6, 0.9, 0.999, 1e-8, 0.1, 10, 1.0)
    step = lambda: _lib.call("owl_adamw_step", ops.stream(), p, g, m, v, bf, *hyper)
    fused = lambda: _lib.call("owl_adamw_step_ema", ops.stream(), p, g, m, v, bf, *hyper, None, None, None, 0, 0.0, None, None, ema, d, w)

    def two():
        step()
        _lib.call("owl_ema_update", ops.stream(), ema, p, n, d, w)

    out = dict(arch=arch, batch=batch, n=n, windows=windows, launches=launches, steps=steps,
               launch_us={k: {s: x * 1e3 for s, x in r.items()} for k, r in alternate(dict(step=step, fused=fused, two=two), launches, 20).items()})

    # ---- the full train step, with and without the average ----
    cfg = get_config(arch)
    model = OwlViT(cfg, weights.make_weights(cfg), dev)
    img = torch.from_numpy(synth.make_images(cfg, batch)).to(dev)
    labels, boxes = synth.make_targets(cfg, batch, max_boxes=6)
    lab = [torch.from_numpy(x).to(dev) for x in labels]; box = [torch.from_numpy(x).to(dev) for x in boxes]
    crit = PushPullLoss(cfg.n_classes, None)
    opts = dict(off=FusedAdamW(model, lr=3e-6, weight_decay=0.1), on=FusedAdamW(model, lr=3e-6, weight_decay=0.1, ema_decay=0.999))

    def train(opt):
        opt.zero_grad()
        pb, _, ps, _ = model(img)
        l = crit(ps, lab, pb, box)
        (l["loss_ce"] + l["loss_bg"] + l["loss_bbox"] + l["loss_giou"]).backward()
        opt.step()

    out["bucket"] = model.flat_numel
    out["step_ms"] = alternate({k: (lambda o=o: train(o)) for k, o in opts.items()}, steps, 3)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--arch", default="owlvit-base-patch16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--limit", type=int, default=500, help="seconds for the child process")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.arch, args.batch, args.windows, args.launches, args.steps)
        return
    argv = ["--child", "--arch", args.arch, "--batch", str(args.batch), "--windows", str(args.windows), "--launches", str(args.launches), "--steps", str(args.steps)]
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"no result within {args.limit} s -- stopped: nothing more is started on the device")
    res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not res:
        sys.exit(f"exit {r.returncode}\n{r.stderr[-2000:]}\n-- stopped: nothing more is started on the device")
    o = json.loads(res[-1][7:])
    print(res[-1], flush=True)
    f = lambda x, nd=1: f"{x['median']:.{nd}f} ({x['lo']:.{nd}f} .. {x['hi']:.{nd}f})"
    L, S = o["launch_us"], o["step_ms"]
    names = dict(step="`owl_adamw_step` (no average; the parent commit's launch)", fused="`owl_adamw_step_ema` (fused)",
                 two="`owl_adamw_step` + `owl_ema_update` (two launches)")
    streams = dict(step=7.5, fused=9.5, two=10.5)          # f32 streams of n elements moved (the bf16 copy counts as half)
    lines = [f"| optimizer launch, {o['n']:,} elements | us, median (min .. max) | over the plain step, us | f32 streams moved | GB/s |", "|---|---|---|---|---|"]
    for k in ("step", "fused", "two"):
        lines.append(f"| {names[k]} | {f(L[k])} | {L[k]['median'] - L['step']['median']:+.1f} | {streams[k]} | {streams[k] * 4 * o['n'] / L[k]['median'] / 1e3:.0f} |")
    gain = L["two"]["median"] - L["fused"]["median"]
    spread = max(L[k]["hi"] - L[k]["lo"] for k in ("fused", "two"))
    lines += ["", f"Fused against two launches: {gain:+.1f} us per step in favour of the fused form; the widest window spread of the two is {spread:.1f} us "
              f"-- the fused form is {'faster by more than the spread' if gain > spread else 'NOT faster by more than the spread'}.", "",
              f"| train step, {o['arch']}, batch {o['batch']}, bucket {o['bucket']:,} | ms / step, median (min .. max) | images / s |", "|---|---|---|"]
    for k, what in (("off", "`ema_decay=None`"), ("on", "`ema_decay=0.999`")):
        lines.append(f"| {what} | {f(S[k], 2)} | {o['batch'] / S[k]['median'] * 1e3:.1f} |")
    lines += ["", f"Median of {o['windows']} windows (min .. max of the windows); a launch window is {o['launches']} launches, a step window {o['steps']} train steps, between two HIP "
              "events; the forms alternate window by window in one process.", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
