"""What the frozen-prefix activation cache is worth on the card: full train step (forward, loss, backward, FusedAdamW) and eval forward at B/16 768^2
batch 32 and L/14 840^2 batch 16, in three states -- cache off (no image_ids: the path of every earlier commit), cold (every id new: the prefix runs, the
states are stored) and warm (every id kept: the prefix is skipped) -- plus the two streams of csrc/prefix_cache.hip next to a device-to-device copy_ of
the same bytes.
  python tools/prefix_cache_timing.py [--out profiles/prefix_cache.md] [--archs owlvit-base-patch16:32,owlvit-large-patch14:16] [--windows 5] [--steps 6] [--limit 400]
Method: one fresh child process per model under its own time limit; inside it the three states ALTERNATE window by window (off, cold, warm, off, ...), each
window = `--steps` steps between two HIP events after a warm-up window of every state; the table gives the median window and the spread (min .. max) per
step.  A cold window uses ids the cache has never seen (the cache is cleared before it, outside the events); a warm window reuses one set of kept ids
with the batch order rotated.  Emit / gather / copy_: 50 launches between events after 10, alternated three times, median.  A child that fails ends the
run: nothing more is started on the device.  The table (markdown) goes to stdout and to --out."""
import argparse, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: F401  (the importable alias of the package directory)


def child(arch, batch, windows, steps):
    import torch
    from owl_vit_object_detection_amd import ops, synth, weights
    from owl_vit_object_detection_amd.config import get_config
    from owl_vit_object_detection_amd.losses import PushPullLoss
    from owl_vit_object_detection_amd.models import OwlViT
    from owl_vit_object_detection_amd.optim import FusedAdamW
    from owl_vit_object_detection_amd.prefix_cache import DEFAULT_MAX_BYTES
    cfg = get_config(arch)
    dev = "cuda"
    model = OwlViT(cfg, weights.make_weights(cfg), dev)
    cache = model.enable_prefix_cache()
    img = torch.from_numpy(synth.make_images(cfg, batch)).to(dev)
    labels, boxes = synth.make_targets(cfg, batch, max_boxes=6)
    lab = [torch.from_numpy(x).to(dev) for x in labels]; box = [torch.from_numpy(x).to(dev) for x in boxes]
    crit = PushPullLoss(cfg.n_classes, None)
    opt = FusedAdamW(model, lr=3e-6, weight_decay=0.1)
    fresh = [10 ** 6]

    def ids_for(state, k):
        if state == "off":
            return None
        if state == "warm":
            return [(j + k) % batch for j in range(batch)]
        fresh[0] += batch
        return list(range(fresh[0], fresh[0] + batch))

    def train(ids):
        opt.zero_grad()
        pb, _, ps, _ = model(img, image_ids=ids)
        l = crit(ps, lab, pb, box)
        (l["loss_ce"] + l["loss_bg"] + l["loss_bbox"] + l["loss_giou"]).backward()
        opt.step()

    def evalf(ids):
        with torch.no_grad():
            model(img, image_ids=ids)

    def window(fn, state, n):
        if state == "cold":
            cache.clear()          # (every cold window starts from an empty cache and refills it; `n` batches of new ids fit the default budget many times over)
        elif state == "warm" and not all(cache.contains(range(batch))):
            evalf(list(range(batch)))
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(n):
            fn(ids_for(state, k))
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    out = dict(arch=arch, batch=batch, image_size=cfg.image_size, boundary_layer=model._chain_low, layers=cfg.layers,
               bytes_per_image=cache.block_bytes, images_in_default_budget=DEFAULT_MAX_BYTES // cache.block_bytes, default_budget_bytes=DEFAULT_MAX_BYTES)
    for what, fn in (("train", train), ("eval", evalf)):
        for state in ("off", "cold", "warm"):
            window(fn, state, 2)          # warm-up of every state: code objects, workspaces, slabs
        ms = {s: [] for s in ("off", "cold", "warm")}
        for _ in range(windows):
            for state in ("off", "cold", "warm"):
                ms[state].append(window(fn, state, steps))
        out[what] = {s: dict(median=statistics.median(v), lo=min(v), hi=max(v)) for s, v in ms.items()}

    # ---- the two streams against copy_ of the same bytes (what one batch moves: `batch` blocks) ----
    E, M = cache.block_elems, batch * cfg.tokens_padded
    xs = torch.randn(batch, E, device=dev)
    d1 = torch.randn(M, cfg.hidden, device=dev).to(torch.bfloat16); d2 = torch.randn(M, cfg.hidden, device=dev).to(torch.bfloat16)
    dst, slots, other = torch.empty(batch, E, device=dev), torch.empty(batch, E, device=dev), torch.empty(batch, E, device=dev)
    da, sa = [dst[j].data_ptr() for j in range(batch)], [slots[j].data_ptr() for j in range(batch)]
    runs = dict(emit=lambda: ops.prefix_emit(xs, d1, d2, batch, E, da, sa), gather=lambda: ops.prefix_gather(batch, E, sa, da), copy=lambda: other.copy_(slots))

    def timed(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(50):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / 50 * 1e3

    us = {k: [] for k in runs}
    for _ in range(3):
        for k, fn in runs.items():
            us[k].append(timed(fn))
    blk = batch * E * 4
    out["streams"] = dict(us={k: dict(median=statistics.median(v), lo=min(v), hi=max(v)) for k, v in us.items()},
                          bytes=dict(emit=blk * 3 + 2 * batch * E * 2, gather=blk * 2, copy=blk * 2))          # emit: xs in, two bf16 deltas in, block + slot out
    print("RESULT " + json.dumps(out), flush=True)


def run_child(argv, limit):
    """One fresh process under its own time limit -> (result dict or None, what went wrong or None); after any failure the caller starts nothing more."""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=limit)
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
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--limit", type=int, default=400, help="seconds per model (its own child process)")
    ap.add_argument("--child", nargs=2, default=None, metavar=("ARCH", "BATCH"))
    args = ap.parse_args()
    if args.child:
        child(args.child[0], int(args.child[1]), args.windows, args.steps)
        return
    rows, stopped = [], None
    for spec in args.archs.split(","):
        arch, batch = spec.split(":")
        res, err = run_child(["--child", arch, batch, "--windows", str(args.windows), "--steps", str(args.steps)], args.limit)
        if err:
            stopped = f"{arch}: {err}"
            break
        rows.append(res)
        print("RESULT " + json.dumps(res), flush=True)
    f = lambda d: f"{d['median']:.2f} ({d['lo']:.2f} .. {d['hi']:.2f})"
    lines = ["| model, input, batch | pass | cache off, ms | cold, ms | warm, ms | cold / off | warm / off |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        for what in ("train", "eval"):
            t = r[what]
            lines.append(f"| {r['arch']}, {r['image_size']}^2, {r['batch']} | {'train step' if what == 'train' else 'eval forward'} | {f(t['off'])} | {f(t['cold'])} | {f(t['warm'])} | "
                         f"{t['cold']['median'] / t['off']['median']:.3f} | {t['warm']['median'] / t['off']['median']:.3f} |")
    lines += ["", f"Median of {args.windows} windows of {args.steps} steps (min .. max of the windows), per step; the three states alternate window by window in one process per "
              "model, HIP events around each window.", "",
              "| model, batch | stream | us / batch | bytes moved | GB/s | vs copy_ of the same blocks |", "|---|---|---|---|---|---|"]
    for r in rows:
        s = r["streams"]
        for k in ("emit", "gather", "copy"):
            u = s["us"][k]
            lines.append(f"| {r['arch']}, {r['batch']} | {'owl_prefix_' + k if k != 'copy' else 'torch copy_ (device to device)'} | {u['median']:.1f} ({u['lo']:.1f} .. {u['hi']:.1f}) | "
                         f"{s['bytes'][k]:,} | {s['bytes'][k] / u['median'] / 1e3:.0f} | {u['median'] / s['us']['copy']['median']:.2f}x the time, "
                         f"{s['bytes'][k] / s['bytes']['copy']:.2f}x the bytes |")
    lines += ["", "50 launches between events after 10, three alternated rounds, median (min .. max).  emit reads the f32 block and two bf16 deltas and writes the block and its slot; "
              "gather and copy_ read and write one f32 block per image.", ""]
    for r in rows:
        lines.append(f"{r['arch']} at {r['image_size']}^2: boundary at encoder layer {r['boundary_layer']} of {r['layers']}; {r['bytes_per_image']:,} bytes per image; "
                     f"{r['images_in_default_budget']:,} images fit the default budget of {r['default_budget_bytes'] / 2 ** 30:.0f} GiB.")
    if stopped:
        lines += ["", f"{stopped}", "-- stopped: nothing more is started on the device after a failed child"]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        open(args.out, "w").write(text)
    if stopped:
        sys.exit(1)


if __name__ == "__main__":
    main()
