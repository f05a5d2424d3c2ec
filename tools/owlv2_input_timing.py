"""What OWLv2's input stage costs on the card (recorded, not asserted; profiles/owlv2_input.md).
  python tools/owlv2_input_timing.py [--out profiles/owlv2_input.md] [--rounds 7] [--launches 200] [--limit 300]
32 uint8 images of 480 x 640, resident in HBM, -> 960 x 960 bf16: `DeviceImageProcessor(960, resize="owlv2")` = owl_preprocess_u8_pad_resize (pad to 640^2,
no blur when upsampling, bilinear zoom, f32 intermediate) alternated in the same process with the Pillow path, owl_preprocess_u8_batch, on the same images and
output size (bicubic warp, u8 intermediate) as the comparison point.  The C entries are timed on prepared descriptors (the host side -- table cache lookups and
one small H2D copy of the descriptors -- is timed apart, through `__call__`, by a host clock around calls that end in a device synchronise).  HIP events
around `--launches` back-to-back calls, 20 warm-up calls per variant, `--rounds` rounds with the variants alternated, median (min .. max).  Bytes are the
compulsory traffic computed from the shapes: source once, the intermediate written and read once, the output once.
One fresh child process under its own time limit; a child that fails ends the run: nothing more is started on the device."""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: F401  (the importable alias of the package directory)

B, H, W, N = 32, 480, 640, 960


def child(rounds, launches):
    import numpy as np
    import torch
    from owl_vit_object_detection_amd import _lib, ops
    from owl_vit_object_detection_amd.preprocess import DeviceImageProcessor
    dev = "cuda"
    rng = np.random.default_rng(0)
    imgs = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev) for _ in range(B)]
    v2 = DeviceImageProcessor(N, device=dev, dtype=torch.bfloat16, resize="owlv2")
    pil = DeviceImageProcessor(N, device=dev, dtype=torch.bfloat16)
    out = torch.empty(B, 3, N, N, dtype=torch.bfloat16, device=dev)
    # ---- prepared descriptors: the launches alone
    rows, tmp_bytes, max_h = v2._pad_resize_plan(imgs)
    live4 = v2._pad_axis_tables(W, max(H, W), N)[3]
    tmp_f32 = torch.empty(tmp_bytes // 4, dtype=torch.float32, device=dev)
    desc_v2 = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(dev)
    prow, off = [], 0
    for im in imgs:
        bx, kx, ksx = pil._axis_tables(W, N)
        by, ky, ksy = pil._axis_tables(H, N)
        prow.append((im.data_ptr(), H, W, bx.data_ptr(), kx.data_ptr(), ksx, by.data_ptr(), ky.data_ptr(), ksy, off))
        off += (H * N * 3 + 255) // 256 * 256
    tmp_u8 = torch.empty(off, dtype=torch.uint8, device=dev)
    desc_pil = torch.from_numpy(np.asarray(prow, dtype=np.int64)).to(dev)
    stream = ops.stream()
    forms = {
        "owlv2": lambda: _lib.call("owl_preprocess_u8_pad_resize", stream, desc_v2, B, max_h, tmp_f32, v2._norm, 0.0, out, 1, N, N),
        "pillow": lambda: _lib.call("owl_preprocess_u8_batch", stream, desc_pil, B, H, tmp_u8, pil.lut, out, 1, N, N),
    }
    bytes_moved = {
        "owlv2": dict(source=B * H * W * 3, intermediate=2 * B * H * live4 * 12, output=B * 3 * N * N * 2),
        "pillow": dict(source=B * H * W * 3, intermediate=2 * B * H * N * 3, output=B * 3 * N * N * 2),
    }

    def between_events(fn, n):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    def wall(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for fn in forms.values():
        between_events(fn, 20)
    ms = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            ms[k].append(between_events(fn, launches))
    calls = {"owlv2": lambda: v2(imgs), "pillow": lambda: pil(imgs)}
    for fn in calls.values():
        wall(fn, 10)
    ws = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            ws[k].append(wall(fn, 50))
    res = dict(rounds=rounds, launches=launches, live4=live4,
               kernels={k: dict(median=statistics.median(v), lo=min(v), hi=max(v), bytes=bytes_moved[k]) for k, v in ms.items()},
               calls={k: dict(median=statistics.median(v), lo=min(v), hi=max(v)) for k, v in ws.items()})
    print("RESULT " + json.dumps(res), flush=True)


def table(o):
    f = lambda x: f"{x['median']:.4f} ({x['lo']:.4f}–{x['hi']:.4f})"
    lines = ["# OWLv2's input stage on one MI355X", "", "Written by `tools/owlv2_input_timing.py`; recorded, not asserted anywhere.", "",
             f"{B} uint8 images of {H} x {W}, resident in HBM, -> {N} x {N} bf16; both paths on the same images, output buffer and size, alternated in one process.", "",
             "| launch pair, ms per batch | `owl_preprocess_u8_pad_resize` (OWLv2: pad, zoom; f32 intermediate) | `owl_preprocess_u8_batch` (Pillow bicubic; u8 intermediate) |", "|---|---|---|",
             f"| time | {f(o['kernels']['owlv2'])} | {f(o['kernels']['pillow'])} |"]
    for part in ("source", "intermediate", "output"):
        lines.append(f"| bytes, {part}{' (written + read)' if part == 'intermediate' else ''} | " + " | ".join(f"{o['kernels'][k]['bytes'][part] / 1e6:.1f} MB" for k in ("owlv2", "pillow")) + " |")
    tot = {k: sum(o["kernels"][k]["bytes"].values()) for k in ("owlv2", "pillow")}
    lines.append("| bytes, total | " + " | ".join(f"{tot[k] / 1e6:.1f} MB" for k in ("owlv2", "pillow")) + " |")
    lines.append("| achieved bandwidth (total bytes / median time) | " + " | ".join(f"{tot[k] / (o['kernels'][k]['median'] * 1e-3) / 1e12:.2f} TB/s" for k in ("owlv2", "pillow")) + " |")
    lines.append(f"| `DeviceImageProcessor.__call__`, host clock, ms per batch | {f(o['calls']['owlv2'])} | {f(o['calls']['pillow'])} |")
    r = o["kernels"]["owlv2"]["median"] / o["kernels"]["pillow"]["median"]
    lines += ["", f"The OWLv2 pair takes {r:.2f} x the Pillow pair's time on {tot['owlv2'] / tot['pillow']:.2f} x its bytes (the f32 intermediate of {o['live4']} live columns "
              "per row is four times the u8 one's bytes per pixel).", "",
              f"Launch pairs: median (min–max) of {o['rounds']} rounds of {o['launches']} back-to-back calls of the C entry on prepared descriptors between two HIP events, 20 warm-up "
              "calls each.  `__call__`: host clock around 50 calls that end in a device synchronise (tables cached, one descriptor copy per call), same rounds.  "
              "Bytes: compulsory traffic from the shapes -- source once, intermediate written and read once, output once; cache re-reads of overlapping taps are not counted.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--limit", type=int, default=300, help="seconds for the child process")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.rounds, args.launches)
        return
    argv = ["--child", "--rounds", str(args.rounds), "--launches", str(args.launches)]
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


if __name__ == "__main__":
    main()
