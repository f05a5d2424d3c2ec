"""Full train step (forward, loss, backward, FusedAdamW) under different trainable sets (`OwlViT(..., trainable=...)`), B/16 batch 32 and L/14 batch 16:
HIP events around 20 steps after 5 warm-up steps, every configuration in a fresh child process under its own time limit.
  python tools/trainable_sets_timing.py [--out FILE.md] [--archs owlvit-base-patch16:32,owlvit-large-patch14:16] [--steps 20] [--warmup 5] [--limit 240]
A first child times the step's dominant GEMM alone (the rate this box holds inside a GEMM).  A child that fails in any way ends the run: nothing more is
started on the device.  The table (markdown) goes to stdout and to --out; profiles/trainable_sets.md keeps the recorded run."""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: F401  (the importable alias of the package directory)

HEADS = ("box", "post_layernorm", "class_predictor", "queries")


def sets_of(layers):
    last = layers - 1
    return [("reference set (layers.11 + heads)", None),
            (f"last layer only (layers.{last} + heads)", (f"layers.{last}.",) + HEADS),
            (f"last two layers (layers.{last - 1}, layers.{last} + heads)", (f"layers.{last - 1}.", f"layers.{last}.") + HEADS),
            ("queries only", ("queries",)),
            ("heads only (queries, class_predictor, box)", ("queries", "class_predictor", "box")),
            ("everything", ("backbone", "post_post_layernorm", "class_predictor", "box_head", "queries"))]


def child(arch, batch, idx, steps, warmup):
    import torch
    from owl_vit_object_detection_amd import synth, weights
    from owl_vit_object_detection_amd.config import get_config
    from owl_vit_object_detection_amd.losses import PushPullLoss
    from owl_vit_object_detection_amd.models import OwlViT
    from owl_vit_object_detection_amd.optim import FusedAdamW
    cfg = get_config(arch)
    name, keep = sets_of(cfg.layers)[idx]
    dev = "cuda"
    model = OwlViT(cfg, weights.make_weights(cfg), dev, trainable=keep)
    img = torch.from_numpy(synth.make_images(cfg, batch)).to(dev)
    labels, boxes = synth.make_targets(cfg, batch, max_boxes=6)
    lab = [torch.from_numpy(x).to(dev) for x in labels]; box = [torch.from_numpy(x).to(dev) for x in boxes]
    crit = PushPullLoss(cfg.n_classes, None)
    opt = FusedAdamW(model, lr=3e-6, weight_decay=0.1)

    def step():
        opt.zero_grad()
        pb, _, ps, _ = model(img)
        l = crit(ps, lab, pb, box)
        (l["loss_ce"] + l["loss_bg"] + l["loss_bbox"] + l["loss_giou"]).backward()
        opt.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / steps
    print("RESULT " + json.dumps(dict(arch=arch, batch=batch, set=name, ms_per_step=round(ms, 3), images_per_s=round(batch / ms * 1e3, 1), trainable_elements=model.flat_numel,
                                      floor=model.backward_floor, trainable_layers=len(model.trainable_layers),
                                      gflop_backward=round(cfg.flops_backward(model.trainable_layers, model.backward_floor) * batch / 1e9, 1))), flush=True)


def gemm_child():
    """The box's GEMM rate under load: the step's dominant op (bias-epilogue GEMM, fc2's shape at B/16 batch 32 rounded to 16384 rows), 200 launches back to
    back after 50.  Boxes differ by a few per cent in the clock they hold inside a GEMM; this figure lets a reader separate the box from the build."""
    import torch
    from owl_vit_object_detection_amd import ops
    M, N, K = 16384, 768, 3072
    g = torch.Generator(device="cpu").manual_seed(0)
    A = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16).cuda()
    Wt = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16).cuda()
    bias = torch.zeros(N, device="cuda"); out = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
    run = lambda: ops.gemm(ops.EPI_BIAS_BF16, A, Wt, out, bias=bias, M=M, N=N, K=K)
    for _ in range(50):
        run()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(200):
        run()
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) / 200 * 1e3
    print("RESULT " + json.dumps(dict(gemm_us=round(us, 2), gemm_tflops=round(2.0 * M * N * K / us / 1e6, 1), shape=[M, N, K])), flush=True)


def run_child(argv, limit):
    """One fresh process under its own time limit -> (result dict or None, what went wrong or None).  ANY failure -- time limit, signal, non-zero exit, no
    result line -- is reported as such, and the caller starts nothing more on the device after it: a HIP fault usually surfaces as a Python exception
    (exit 1), and a card that has faulted is not to be used again."""
    cmd = [sys.executable, os.path.abspath(__file__)] + argv
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return None, f"no result within {limit} s"
    res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not res:
        return None, f"exit {r.returncode}\n{r.stderr[-2000:]}"
    return json.loads(res[-1][7:]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--archs", default="owlvit-base-patch16:32,owlvit-large-patch14:16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per configuration (its own child process)")
    ap.add_argument("--child", nargs=3, default=None, metavar=("ARCH", "BATCH", "SET_INDEX"))
    ap.add_argument("--gemm-child", action="store_true")
    args = ap.parse_args()
    if args.gemm_child:
        gemm_child()
        return
    if args.child:
        child(args.child[0], int(args.child[1]), int(args.child[2]), args.steps, args.warmup)
        return
    from owl_vit_object_detection_amd.config import get_config
    rows, stopped = [], None
    box, err = run_child(["--gemm-child"], args.limit)
    if err:
        stopped = f"GEMM rate: {err}"
    for spec in ([] if stopped else args.archs.split(",")):
        arch, batch = spec.split(":")
        for idx, (name, _) in enumerate(sets_of(get_config(arch).layers)):
            res, err = run_child(["--child", arch, batch, str(idx), "--steps", str(args.steps), "--warmup", str(args.warmup)], args.limit)
            if err:
                stopped = f"{arch} / {name}: {err}"
                rows.append(dict(arch=arch, batch=int(batch), set=name, error=err.splitlines()[0]))
                break
            rows.append(res)
            print("RESULT " + json.dumps(res), flush=True)
        if stopped:
            break
    if stopped:
        print(f"{stopped}\n-- stopped: nothing more is started on the device after a failed child", flush=True)
    lines = ["| model, batch | trainable set | floor | trainable elements | backward GFLOP (algorithmic) | ms / step | images / s | vs reference set |", "|---|---|---|---|---|---|---|---|"]
    base = {}
    for r in rows:
        if "error" in r:
            lines.append(f"| {r['arch']}, {r['batch']} | {r['set']} | | | | {r['error']} | | |")
            continue
        base.setdefault(r["arch"], r["ms_per_step"])
        lines.append(f"| {r['arch']}, {r['batch']} | {r['set']} | {r['floor']} | {r['trainable_elements']:,} | {r['gflop_backward']} | {r['ms_per_step']:.2f} | {r['images_per_s']} | "
                     f"{r['ms_per_step'] / base[r['arch']]:.3f}x |")
    lines.append("")
    lines.append(f"{args.steps} steps after {args.warmup} warm-up steps, HIP events around the timed steps, one fresh process per row.  This box's GEMM rate under load "
                 "(the clock it holds inside a GEMM, stated as the time of one op): "
                 + (f"bias-epilogue GEMM {box['shape'][0]} x {box['shape'][1]} x {box['shape'][2]} in {box['gemm_us']:.1f} us = {box['gemm_tflops']} TFLOP/s, 200 launches back to back."
                    if box else "not measured."))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        open(args.out, "w").write(text)
    if stopped:
        sys.exit(1)


if __name__ == "__main__":
    main()
