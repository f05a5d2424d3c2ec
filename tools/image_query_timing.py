"""What the query bank from image exemplars costs on the card: `owl_image_query_select` (its two launches) and `owl_query_bank_fill` at
(N, P, Dt) = (32, 2304, 512) and (16, 3600, 768), set against the bytes the selection must read -- e [N, P, Dt] f32 TWICE in the worst case (once for the
column sums, once more if every box is selected; on random boxes the second pass reads a few rows only) -- and against a device-to-device copy of e
timed in the same process (read + write of the same bytes: the device's copy rate).
  python tools/image_query_timing.py [--out profiles/image_queries.md] [--windows 7] [--launches 50] [--limit 300]
Method: one fresh child process under its own time limit; a window is `--launches` launches between two HIP events, the forms alternate window by
window after a warm-up window of each; every figure is the median of `--windows` windows (min .. max).  Initialisation-time work outside the step:
recorded, not asserted.  The table (markdown) goes to stdout and to --out."""
import argparse, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: F401  (the importable alias of the package directory)

SHAPES = [(32, 2304, 512), (16, 3600, 768)]


def child(windows, launches):
    import torch
    from owl_vit_object_detection_amd import _lib, models, ops
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

    out = []
    for N, P, Dt in SHAPES:
        g = torch.Generator().manual_seed(P + Dt)
        e = (0.7 * torch.randn(N, P, Dt, generator=g)).to(dev)
        c = torch.sigmoid(torch.randn(N, P, 4, generator=g))
        boxes = torch.stack([c[..., 0] - c[..., 2] / 2, c[..., 1] - c[..., 3] / 2, c[..., 0] + c[..., 2] / 2, c[..., 1] + c[..., 3] / 2], -1).contiguous().to(dev)
        same = torch.tensor([0.2, 0.25, 0.8, 0.75], device=dev).repeat(N, P, 1).contiguous()          # every box selected: e is read twice
        ws = torch.empty(ops.image_query_workspace_bytes(N, P, Dt), dtype=torch.uint8, device=dev)
        best = torch.empty(N, dtype=torch.int32, device=dev); info = torch.empty(N, 2, dtype=torch.int32, device=dev)
        query = torch.empty(N, Dt, device=dev); dst = torch.empty_like(e)
        C = max(1, N // 2)
        row_ptr, members = models.slots_csr(models.exemplar_slots([n % C for n in range(N)], C))
        row_ptr, members = torch.from_numpy(row_ptr).to(dev), torch.from_numpy(members).to(dev)
        bank = torch.randn(3 * C, Dt, device=dev)
        sel = lambda b: _lib.call("owl_image_query_select", ops.stream(), e, b, None, N, P, Dt, ws, ws.numel(), best, query, info, None, None, None)
        forms = dict(select_random=lambda: sel(boxes), select_all=lambda: sel(same), fill=lambda: ops.query_bank_fill(query, row_ptr, members, bank, N, 3 * C, Dt),
                     copy=lambda: dst.copy_(e))
        for fn in forms.values():
            between_events(fn, 5)
        ms = {k: [] for k in forms}
        for _ in range(windows):
            for k, fn in forms.items():
                ms[k].append(between_events(fn, launches))
        nsel = info[:, 1].float().mean().item()
        out.append(dict(N=N, P=P, Dt=Dt, e_bytes=N * P * Dt * 4, selected_all=nsel, bank_rows=3 * C,
                        us={k: dict(median=statistics.median(v), lo=min(v), hi=max(v)) for k, v in ms.items()}))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--limit", type=int, default=300, help="seconds for the child process")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.windows, args.launches)
        return
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--windows", str(args.windows), "--launches", str(args.launches)],
                           capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"no result within {args.limit} s -- stopped: nothing more is started on the device")
    res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not res:
        sys.exit(f"exit {r.returncode}\n{r.stderr[-2000:]}\n-- stopped: nothing more is started on the device")
    print(res[-1], flush=True)
    f = lambda x: f"{x['median']:.1f} ({x['lo']:.1f} .. {x['hi']:.1f})"
    lines = ["| (N, P, Dt) | launch | us, median (min .. max) | bytes it must read | at the median |", "|---|---|---|---|---|"]
    for o in json.loads(res[-1][7:]):
        eb, u = o["e_bytes"], o["us"]
        shape = f"({o['N']}, {o['P']}, {o['Dt']})"
        rate = lambda b, k: f"{b / u[k]['median'] / 1e6:.2f} TB/s"
        lines.append(f"| {shape} | `owl_image_query_select`, random boxes | {f(u['select_random'])} | {eb / 1e6:.1f} MB (e once + the selected rows) | {rate(eb, 'select_random')} |")
        lines.append(f"| {shape} | `owl_image_query_select`, every box selected | {f(u['select_all'])} | {2 * eb / 1e6:.1f} MB (e twice) | {rate(2 * eb, 'select_all')} |")
        lines.append(f"| {shape} | `owl_query_bank_fill`, {o['bank_rows']} rows | {f(u['fill'])} | {o['N'] * o['Dt'] * 8 / 1e3:.0f} KB | launch-bound |")
        lines.append(f"| {shape} | device copy of e (`Tensor.copy_`) | {f(u['copy'])} | {eb / 1e6:.1f} MB read + as much written | {rate(2 * eb, 'copy')} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
