"""What the colour jitter of the device input stage costs on the card (recorded, not asserted; profiles/color_jitter.md).
  python tools/color_jitter_timing.py [--out profiles/color_jitter.md] [--rounds 5] [--launches 40] [--windows 4] [--steps 20] [--limit 900]
1. Kernels: `owl_preprocess_u8_tiles_color` next to `owl_preprocess_u8_tiles` (unchanged object code) on the SAME tile lists -- `TrainAugment(768, mosaic=(g,))`
   draws for g = 1, 2, 3 over 32 uint8 sources of 480 x 640 -> 768^2 bf16 -- with `ColorJitter(0.4, 0.4, 0.4, gray=0.1)` rows, with the same rows but no
   contrast (fc = 1: no sum), and with the all-ones array (the passes alone).  HIP events around `--launches` back-to-back launches, `--rounds` rounds with
   the variants alternated, median (min .. max); the colour output is compared with the plain one under the all-ones array before anything is timed.
2. The full B/16 batch-32 train step fed by `DevicePrefetcher` (threaded, depth 2) from pageable host uint8 batches, `color` off and on, at mosaic (1,) and
   (1, 2, 3): `--windows` windows of `--steps` steps per feed, the feeds alternated window by window in one process after 4 warm-up steps each; host clock
   around steps that end in a device synchronise.
One fresh child process under its own time limit; a child that fails ends the run: nothing more is started on the device."""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: F401  (the importable alias of the package directory)

B, H, W, S = 32, 480, 640, 768


def child(rounds, launches, windows, steps, arch):
    import numpy as np
    import torch
    from owl_vit_object_detection_amd import weights
    from owl_vit_object_detection_amd import preprocess as P
    from owl_vit_object_detection_amd.config import get_config
    from owl_vit_object_detection_amd.losses import PushPullLoss
    from owl_vit_object_detection_amd.models import OwlViT
    from owl_vit_object_detection_amd.optim import FusedAdamW
    dev = "cuda"
    rng = np.random.default_rng(0)
    u8 = torch.from_numpy(rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8))
    boxes = [np.stack([rng.uniform(0, W / 2, 3), rng.uniform(0, H / 2, 3), rng.uniform(W / 4, W / 2, 3), rng.uniform(H / 4, H / 2, 3)], axis=1) for _ in range(B)]
    cfg = get_config(arch)
    assert cfg.image_size == S
    labels = [rng.integers(0, cfg.n_classes, 3) for _ in range(B)]
    shapes = [(H, W)] * B
    jitter = P.ColorJitter(0.4, 0.4, 0.4, gray=0.1)
    out = dict(rounds=rounds, launches=launches, windows=windows, steps=steps, arch=arch, kernels={}, feeds={})

    def between_events(fn, n):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    # ---- 1. the launches ----
    ip = P.DeviceImageProcessor(size=S, dtype=torch.bfloat16)
    src_d = u8.to(dev)
    for g in (1, 2, 3):
        tiles, _, _ = P.TrainAugment(S, mosaic=(g,), seed=g).sample(shapes, boxes, labels, 0, 0)
        P.check_tile_cover(tiles, B, S, shapes)
        desc, arena, tmp_bytes, max_rows = P.build_tile_tables(shapes, tiles)
        arena_d = torch.from_numpy(arena).to(dev)
        P.resolve_tile_descs(desc, [src_d[i].data_ptr() for i in range(B)], arena_d.data_ptr())
        desc_d = torch.from_numpy(desc).to(dev)
        n = len(tiles)
        rows = jitter.sample(n, (0, 0, 0, g))
        flat = rows.copy(); flat[:, 1] = 1.0
        col = {k: torch.from_numpy(v).to(dev) for k, v in (("jitter", rows), ("no_contrast", flat), ("ones", np.ones((n, 4), dtype=np.float32)))}
        run = lambda c=None: ip.run_tiles(desc_d, n, max_rows, tmp_bytes, B, color=c)
        assert torch.equal(run(), run(col["ones"])), "the all-ones colour array must give the plain launch's bits"
        forms = dict(plain=lambda: run(), ones=lambda: run(col["ones"]), no_contrast=lambda: run(col["no_contrast"]), jitter=lambda: run(col["jitter"]))
        for fn in forms.values():
            between_events(fn, 10)
        ms = {k: [] for k in forms}
        for _ in range(rounds):
            for k, fn in forms.items():
                ms[k].append(between_events(fn, launches))
        out["kernels"][str(g)] = dict(tiles=n, **{k: dict(median=statistics.median(v), lo=min(v), hi=max(v)) for k, v in ms.items()})
        torch.cuda.synchronize()

    # ---- 2. the train step behind the prefetcher ----
    model = OwlViT(cfg, weights.make_weights(cfg), dev)
    crit = PushPullLoss(cfg.n_classes, None)
    opt = FusedAdamW(model, lr=3e-6, weight_decay=0.1)
    lab_t, box_t = [torch.from_numpy(l) for l in labels], [torch.from_numpy(b).float() for b in boxes]

    def loader():
        while True:
            yield u8, lab_t, box_t

    def feed(mosaic, color):
        aug = P.TrainAugment(S, mosaic=mosaic, seed=3, color=jitter if color else None)
        pf = P.DevicePrefetcher(loader(), dev, size=S, dtype=torch.bfloat16, depth=2, augment=aug)
        return pf, iter(pf)

    def train(it):
        img, lab, box = next(it)
        opt.zero_grad()
        pb, _, ps, _ = model(img)
        l = crit(ps, lab, pb, box)
        (l["loss_ce"] + l["loss_bg"] + l["loss_bbox"] + l["loss_giou"]).backward()
        opt.step()

    def window(it, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            train(it)
        torch.cuda.synchronize()
        return B * n / (time.perf_counter() - t0)

    feeds = {f"{m}/{'on' if c else 'off'}": feed(m, c) for m in ((1,), (1, 2, 3)) for c in (False, True)}
    for pf, it in feeds.values():
        window(it, 4)
    rate = {k: [] for k in feeds}
    for _ in range(windows):
        for k, (pf, it) in feeds.items():
            rate[k].append(window(it, steps))
    for k, (pf, it) in feeds.items():
        out["feeds"][k] = dict(windows=rate[k], median=statistics.median(rate[k]), bytes_per_image=int(pf.bytes_h2d / max(1, pf.batches) / B),
                               augment_ms=pf.augment_seconds / max(1, pf.batches) * 1e3)
        pf.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--arch", default="owlvit-base-patch16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=900, help="seconds for the child process")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.rounds, args.launches, args.windows, args.steps, args.arch)
        return
    argv = ["--child", "--arch", args.arch, "--rounds", str(args.rounds), "--launches", str(args.launches), "--windows", str(args.windows), "--steps", str(args.steps)]
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
    names = dict(plain="`owl_preprocess_u8_tiles` (the parent's object code)", ones="colour entry, all-ones array (bitwise the row above)",
                 no_contrast="colour entry, jitter rows with fc = 1 (no sum)", jitter="colour entry, `ColorJitter(0.4, 0.4, 0.4, gray=0.1)` rows")
    lines = ["| launch | g = 1 (32 tiles) | g = 2 (128) | g = 3 (288) |", "|---|---|---|---|"]
    for k in ("plain", "ones", "no_contrast", "jitter"):
        lines.append(f"| {names[k]} | " + " | ".join(f(o["kernels"][g][k]) for g in ("1", "2", "3")) + " |")
    lines.append("| colour rows over plain, ms | " + " | ".join(f"{o['kernels'][g]['jitter']['median'] - o['kernels'][g]['plain']['median']:+.4f}" for g in ("1", "2", "3")) + " |")
    lines += ["", f"ms per batch of 32, median (min–max) of {o['rounds']} rounds of {o['launches']} back-to-back launches between two HIP events, variants alternated.", "",
              "| feed | img/s (median; windows) | vs colour off | spread of the windows | H2D bytes per image | host ms per batch (sampling + tables) |", "|---|---|---|---|---|---|"]
    for m in ("(1,)", "(1, 2, 3)"):
        off = o["feeds"][f"{m}/off"]
        for c in ("off", "on"):
            x = o["feeds"][f"{m}/{c}"]
            lines.append(f"| `mosaic={m}`, colour {c} | {x['median']:.1f} ({', '.join(f'{w:.1f}' for w in x['windows'])}) | {x['median'] / off['median']:.4f} | "
                         f"{(max(x['windows']) - min(x['windows'])) / x['median'] * 100:.2f} % | {x['bytes_per_image']:,} | {x['augment_ms']:.2f} |")
    lines += ["", f"{o['arch']}, batch 32, full step; {o['windows']} windows of {o['steps']} steps per feed, alternated window by window in one process, 4 warm-up steps each.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
