"""Timing record for rectangular inputs -> profiles/rect_inputs.md (needs an MI355X; nothing here is asserted by a test).

  1. The default benchmark (bench.py, square 768 x 768): this tree against a checkout of the parent commit (`--parent DIR`, its library built), run in
     alternation in the same session on the same card; per run the median of five windows and the window spread.  The square path's only change is one
     operand of the patch gather.
  2. A rectangular train step against the square step of the same build: B/16, batch 32, at (576, 1024) = 36 x 64 = 2304 patches, the P of 768 x 768.
     Every launch above the embeddings has the same shape, so the difference is the rectangular gather and the resampled table.  The patch-embedding
     launch is also timed on its own with HIP events.
  3. The covering square: the same batch at 1024 x 1024 (4096 patches) -- what a user of 16:9 images paid before.

Steps are timed with HIP events around whole windows that end in a synchronise; every shape is warmed up first.

  python tools/rect_timing.py --parent /path/to/parent/checkout --out profiles/rect_inputs.md
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_line(tree, steps, warmup):
    tree = os.path.abspath(tree)
    cmd = [sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--windows", "5", "--no-cpu-baseline",
           "--no-compare"]
    out = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    return dict(value=line["value"], windows=line["config"]["window_values"], spread=line["config"]["window_spread_pct"])


def step_times(size, batch, steps, windows, warmup):
    """Median window's ms per train step (forward, PushPullLoss, backward, FusedAdamW) of B/16 at `size`, and the patch-embedding launch's own time."""
    import torch
    from owl_vit_object_detection_amd import ops, synth
    from owl_vit_object_detection_amd.losses import PushPullLoss
    from owl_vit_object_detection_amd.models import load_model
    from owl_vit_object_detection_amd.optim import FusedAdamW
    dev = torch.device("cuda", 0)
    model = load_model({i: f"c{i}" for i in range(10)}, dev, arch="owlvit-base-patch16", image_size=size)
    cfg = model.cfg
    H, W = cfg.image_hw
    gen = torch.Generator(device="cpu").manual_seed(3)
    img = torch.randn(batch, 3, H, W, generator=gen).to(dev).bfloat16()
    labels, boxes = synth.make_targets(cfg, batch, max_boxes=16)
    lab = [torch.from_numpy(x).to(dev) for x in labels]
    box = [torch.from_numpy(x).to(dev) for x in boxes]
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
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            step()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    model.finish()
    # the patch-embedding launch alone: the model's own operands, 50 launches between one pair of events
    x = torch.empty(batch * cfg.tokens_padded, cfg.hidden, dtype=torch.float32, device=dev)
    pos = model._pos_table()
    for _ in range(5):
        ops.patch_embed_hw(img, model._fz["w_pe"], pos, x, batch, H, W, cfg.patch_size, cfg.hidden, cfg.tokens_padded)
    torch.cuda.synchronize()
    pe = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(50):
            ops.patch_embed_hw(img, model._fz["w_pe"], pos, x, batch, H, W, cfg.patch_size, cfg.hidden, cfg.tokens_padded)
        b.record()
        torch.cuda.synchronize()
        pe.append(a.elapsed_time(b) / 50 * 1e3)
    out = dict(size=list(cfg.image_hw), patches=cfg.patches, ms=statistics.median(ms), ms_windows=[round(v, 3) for v in ms],
               spread_pct=100.0 * (max(ms) - min(ms)) / statistics.median(ms), images_per_s=batch / statistics.median(ms) * 1e3,
               patch_embed_us=statistics.median(pe), resampled=model._pos_used is not None)
    del model, opt
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built (part 1 is skipped without it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rect_inputs.md"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="alternations parent / this tree")
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "rect_timing.py measures on the GPU: there is no CPU path"
    md = ["# Rectangular inputs: timing", "", f"Device: {torch.cuda.get_device_name(0)}.  Written by `tools/rect_timing.py`; nothing here is asserted by a test.", ""]
    if args.parent:
        runs = []
        for r in range(args.rounds):
            for name, tree in (("parent", args.parent), ("this tree", ROOT)):
                runs.append((name, bench_line(tree, args.steps, args.warmup)))
                print(name, runs[-1][1], flush=True)
        md += ["## 1. The default benchmark (768 x 768, B/16, batch 32): this tree against the parent commit", "",
               f"`bench.py --gpus 1 --steps {args.steps} --warmup {args.warmup} --windows 5`, alternating, same session, same card.", "",
               "| run | tree | images/s (median window) | windows | window spread % |", "|---|---|---|---|---|"]
        for i, (name, b) in enumerate(runs):
            md.append(f"| {i} | {name} | {b['value']:.2f} | {b['windows']} | {b['spread']:.2f} |")
        p = statistics.median(b["value"] for n, b in runs if n == "parent")
        t = statistics.median(b["value"] for n, b in runs if n == "this tree")
        md += ["", f"Median of the runs: parent {p:.2f}, this tree {t:.2f} images/s: {100.0 * (t - p) / p:+.2f} % "
                   f"(largest window spread of a run: {max(b['spread'] for _, b in runs):.2f} %).", ""]
    sq = step_times(768, args.batch, args.steps, 5, args.warmup)
    print(sq, flush=True)
    rc = step_times((576, 1024), args.batch, args.steps, 5, args.warmup)
    print(rc, flush=True)
    cover = step_times(1024, max(1, args.batch), max(2, args.steps // 2), 5, 3)
    print(cover, flush=True)
    md += ["## 2. and 3. A rectangular step against the square step and the covering square (B/16, batch %d, full train step)" % args.batch, "",
           "| size | patches | table | ms / step (median of 5 windows) | windows | spread % | images/s | patch-embedding launch, us |", "|---|---|---|---|---|---|---|---|"]
    for r in (sq, rc, cover):
        md.append(f"| {r['size'][0]} x {r['size'][1]} | {r['patches']} | {'resampled' if r['resampled'] else 'native'} | {r['ms']:.3f} | {r['ms_windows']} | "
                  f"{r['spread_pct']:.2f} | {r['images_per_s']:.1f} | {r['patch_embed_us']:.1f} |")
    md += ["", f"(576, 1024) against 768 x 768 (the same P, every launch above the embeddings the same shape): step time ratio {rc['ms'] / sq['ms']:.4f}, "
               f"patch-embedding launch {rc['patch_embed_us']:.1f} against {sq['patch_embed_us']:.1f} us.",
           f"(576, 1024) against the covering square 1024 x 1024: {cover['ms'] / rc['ms']:.2f}x less time per step "
           f"({rc['images_per_s']:.1f} against {cover['images_per_s']:.1f} images/s).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(md))
    print("\n".join(md))


if __name__ == "__main__":
    main()
