"""HIP-event medians of owl_pos_resample / owl_pos_resample_bwd at the two full-size tables (48 -> 60: B/16 at 960; 60 -> 72: L/14 at 1008) and
full-step images/s of B/16 at another input size than its table's (profiles/pos_resample.md).
  python tools/pos_resample_timing.py [--steps 10] [--warmup 3] [--batch 16] [--sizes 960,768] [--out FILE.json]
A step is forward + matcher + loss + backward + FusedAdamW on synthetic data, timed by a host clock around a device synchronise; each size runs with the
reference trainable set and with everything trainable (the position table then trains: both kernels on the per-step path)."""
import argparse, json, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: F401  (the importable alias of the package directory)
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--sizes", default="960,768")
ap.add_argument("--arch", default="owlvit-base-patch16")
ap.add_argument("--out", default=None)
args = ap.parse_args()
from owl_vit_object_detection_amd import ops, synth
from owl_vit_object_detection_amd.config import get_config
from owl_vit_object_detection_amd.losses import PushPullLoss
from owl_vit_object_detection_amd.models import load_model
from owl_vit_object_detection_amd.optim import FusedAdamW

dev = "cuda"
out = {"kernels": {}, "steps": {}}
for g0, g, D in ((48, 60, 768), (60, 72, 1024)):
    gen = torch.Generator(device=dev).manual_seed(0)
    pos = torch.randn(g0 * g0 + 1, D, device=dev, generator=gen) * 0.02
    U = torch.zeros(g * g + 1, D, device=dev)
    dU = torch.randn(g * g + 1, D, device=dev, generator=gen)
    dpos = torch.zeros(g0 * g0 + 1, D, device=dev)
    fns = {"owl_pos_resample": lambda: ops.pos_resample(pos, U, g0, g, D), "owl_pos_resample_bwd": lambda: ops.pos_resample_bwd(dU, dpos, g0, g, D)}
    times = {k: [] for k in fns}
    for rnd in range(6):                      # round 0 = warm-up
        for k, f in fns.items():
            evs = []
            for _ in range(20):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); f(); b.record()
                evs.append((a, b))
            torch.cuda.synchronize()
            if rnd:
                times[k] += [a.elapsed_time(b) * 1e3 for a, b in evs]
    nbytes = {"owl_pos_resample": 4 * D * (g0 * g0 + 1 + g * g + 1), "owl_pos_resample_bwd": 4 * D * (g * g + 1 + 2 * (g0 * g0 + 1))}
    for k, t in times.items():
        med = statistics.median(t)
        out["kernels"][f"{k} {g0}->{g} D={D}"] = dict(median_us=round(med, 2), min_us=round(min(t), 2), p90_us=round(sorted(t)[int(0.9 * len(t))], 2), launches=len(t),
                                                      compulsory_bytes=nbytes[k], gb_per_s_at_median=round(nbytes[k] / med / 1e3, 1))
    print(json.dumps({k: v for k, v in out["kernels"].items() if f"{g0}->{g}" in k}), flush=True)

EVERYTHING = ("backbone", "post_post_layernorm", "class_predictor", "box_head", "queries")
labelmap = {i: f"c{i}" for i in range(10)}
for S in (int(s) for s in args.sizes.split(",")):
    for tag, keep in (("reference set", None), ("everything", EVERYTHING)):
        model = load_model(labelmap, dev, arch=args.arch, image_size=S, trainable=keep)
        cfg = model.cfg
        img = torch.from_numpy(synth.make_images(cfg, args.batch)).to(dev).to(torch.bfloat16)
        labels, boxes = synth.make_targets(cfg, args.batch)
        lab = [torch.from_numpy(x).to(dev) for x in labels]; box = [torch.from_numpy(x).to(dev) for x in boxes]
        crit = PushPullLoss(cfg.n_classes, None)
        opt = FusedAdamW(model, lr=3e-6, weight_decay=0.1)
        ts = []
        for s in range(args.warmup + args.steps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            opt.zero_grad()
            pb, _, ps, _ = model(img)
            l = crit(ps, lab, pb, box)
            (l["loss_ce"] + l["loss_bg"] + l["loss_bbox"] + l["loss_giou"]).backward()
            opt.step()
            torch.cuda.synchronize()
            if s >= args.warmup:
                ts.append(time.perf_counter() - t0)
        med = statistics.median(ts)
        out["steps"][f"{args.arch} at {S}, batch {args.batch}, {tag}"] = dict(
            native_grid=cfg.native_grid, grid=cfg.grid, tokens=cfg.tokens, resampled=model._pos_used is not None, ms_per_step=round(med * 1e3, 2),
            images_per_s=round(args.batch / med, 1), min_ms=round(min(ts) * 1e3, 2), max_ms=round(max(ts) * 1e3, 2), steps=len(ts))
        print(json.dumps({k: v for k, v in out["steps"].items() if f" {S}," in k and k.endswith(tag)}), flush=True)
        del model, opt, img, crit
        torch.cuda.empty_cache()
print(json.dumps(out, indent=1))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
