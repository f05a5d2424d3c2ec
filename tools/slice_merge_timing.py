"""What sliced inference costs on the card (recorded, not asserted; profiles/slice_merge.md).
  python tools/slice_merge_timing.py [--out profiles/slice_merge.md] [--rounds 5] [--launches 40] [--limit 600]
1. The merge alone: `ops.slice_merge` (three launches of csrc/slice_merge.hip) on one source image of T = 13 and T = 40 slices x K = 200 candidate slots,
   every slot live (n = 2600 and 8000: the 4096- and 8192-key sorts), clustered boxes, both metrics.  HIP events around `--launches` back-to-back calls,
   `--rounds` rounds with the variants alternated, median (min .. max).
2. `detect_sliced` on one 3000 x 4000 uint8 image at OWL-ViT-B/16 (768^2 windows, overlap 0.2: 5 x 7 + 1 = 36 slices, two forward chunks of 32 + 4) against the
   plain path on the same image (`DeviceImageProcessor.__call__` + forward + `PostProcess(top_k=200)`): host clock around calls that end in a device
   synchronise, image already on the device, random weights (the detections are noise: the merge's share depends on how many pass the threshold, which is
   printed beside it).
One fresh child process under its own time limit; a child that fails ends the run: nothing more is started on the device."""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: F401  (the importable alias of the package directory)

K, H, W = 200, 3000, 4000


def child(rounds, launches, arch):
    import numpy as np
    import torch
    from owl_vit_object_detection_amd import ops, weights
    from owl_vit_object_detection_amd.config import get_config
    from owl_vit_object_detection_amd.models import OwlViT
    from owl_vit_object_detection_amd.postprocess import PostProcess, SlicedPostProcess, detect_sliced
    from owl_vit_object_detection_amd.preprocess import DeviceImageProcessor
    dev = "cuda"
    rng = np.random.default_rng(0)
    out = dict(rounds=rounds, launches=launches, arch=arch, merge={}, detect={})

    def between_events(fn, n):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    # ---- 1. the merge alone ----
    for T in (13, 40):
        n = T * K
        centers = rng.random((64, 2)).astype(np.float32) * 0.8 + 0.05
        c = centers[rng.integers(0, 64, n)] + rng.normal(0, 0.01, (n, 2)).astype(np.float32)
        wh = (0.05 + rng.normal(0, 0.005, (n, 2))).astype(np.float32)
        boxes = torch.from_numpy(np.concatenate([c, c + wh], 1).reshape(T, K, 4)).to(dev)
        scores = torch.from_numpy(rng.random((T, K)).astype(np.float32)).to(dev)
        classes = torch.from_numpy(rng.integers(0, 10, (T, K))).to(dev)
        counts = torch.full((T,), K, dtype=torch.int32, device=dev)
        xform = torch.tensor([[1.0, 0.0, 1.0, 0.0]] * T, device=dev)
        offs = torch.tensor([0, T], dtype=torch.int32, device=dev)
        forms = {m: (lambda m=m: ops.slice_merge(boxes, scores, classes, counts, xform, offs, 1, n, 200, 0.3, m, True)) for m in ("iou", "ios")}
        kept = {m: int(fn()[4][0]) for m, fn in forms.items()}
        full = {m: int(ops.slice_merge(boxes, scores, classes, counts, xform, offs, 1, n, n, 0.3, m, True)[4][0]) for m in forms}
        for fn in forms.values():
            between_events(fn, 10)
        ms = {m: [] for m in forms}
        for _ in range(rounds):
            for m, fn in forms.items():
                ms[m].append(between_events(fn, launches))
        out["merge"][str(T)] = {m: dict(median=statistics.median(v), lo=min(v), hi=max(v), kept=kept[m], kept_uncut=full[m]) for m, v in ms.items()}
    torch.cuda.synchronize()

    # ---- 2. detect_sliced against the plain path ----
    cfg = get_config(arch)
    S = cfg.image_size
    model = OwlViT(cfg, weights.make_weights(cfg), dev).eval()
    ip = DeviceImageProcessor(size=S, dtype=torch.bfloat16)
    image = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
    conf = 0.0                                             # random weights: a threshold in the middle of the similarities
    post, plain_pp = SlicedPostProcess(conf, 0.3), PostProcess(conf, 0.3)

    def sliced():
        return detect_sliced(model, ip, [image], post, batch=32, top_k=200)

    def plain():
        with torch.no_grad():
            pb, _, ps, _ = model(ip(images=image)["pixel_values"])
        return plain_pp(pb, ps, top_k=200)

    def wall(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    plan = sliced()[3]
    forms = dict(plain=plain, sliced=sliced)
    for fn in forms.values():
        wall(fn, 3)
    ms = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            ms[k].append(wall(fn, 5))
    sliced()
    out["detect"] = dict(slices=len(plan.tiles), size=S, kept=int(post.last_counts[0]), **{k: dict(median=statistics.median(v), lo=min(v), hi=max(v)) for k, v in ms.items()})
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--arch", default="owlvit-base-patch16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--limit", type=int, default=600, help="seconds for the child process")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.rounds, args.launches, args.arch)
        return
    argv = ["--child", "--arch", args.arch, "--rounds", str(args.rounds), "--launches", str(args.launches)]
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"no result within {args.limit} s -- stopped: nothing more is started on the device")
    res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not res:
        sys.exit(f"exit {r.returncode}\n{r.stderr[-3000:]}\n-- stopped: nothing more is started on the device")
    print(res[-1], flush=True)
    text = table(json.loads(res[-1][7:]))
    print(text)
    if args.out:
        open(args.out, "w").write(text)


def table(o):
    f = lambda x: f"{x['median']:.4f} ({x['lo']:.4f}–{x['hi']:.4f})"
    lines = ["# Sliced inference: the merge and `detect_sliced` on one MI355X", "",
             "Written by `tools/slice_merge_timing.py`; recorded, not asserted anywhere.", "",
             "| `ops.slice_merge`, one source image, K = 200, every slot live, `max_out` 200 | T = 13 (n = 2600) | T = 40 (n = 8000) |", "|---|---|---|"]
    for m in ("iou", "ios"):
        lines.append(f"| metric `{m}`, ms per call | " + " | ".join(f(o["merge"][t][m]) for t in ("13", "40")) + " |")
        lines.append(f"| metric `{m}`, kept without the cut | " + " | ".join(str(o["merge"][t][m]["kept_uncut"]) for t in ("13", "40")) + " |")
    d = o["detect"]
    lines += ["", f"ms per call (sort + pair mask + scan + the wrapper's five output fills), median (min–max) of {o['rounds']} rounds of {o['launches']} back-to-back calls between "
              "two HIP events, metrics alternated; 64 clusters of boxes, 10 classes, threshold 0.3.", "",
              f"| one {H} x {W} uint8 image on the device, {o['arch']} ({d['size']}²), bf16 input stage, random weights | ms per image |", "|---|---|",
              f"| plain: `DeviceImageProcessor()` + forward + `PostProcess(top_k=200)` | {f(d['plain'])} |",
              f"| `detect_sliced`: {d['slices']} slices, forward in chunks of 32, `SlicedPostProcess(top_k=200)` ({d['kept']} kept) | {f(d['sliced'])} |",
              f"| ratio | {d['sliced']['median'] / d['plain']['median']:.2f} |",
              "", f"Host clock around 5 calls that end in a device synchronise, median (min–max) of {o['rounds']} rounds, the two paths alternated, 3 warm-up calls each.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
